"""oracle/gemm_tn_ref.py on the CPU: the launcher's host rules against cases worked by hand from the text of launch_tn_group and
unimm_gemm_tn_grouped_ws (csrc/gemm.hip), the measurement behind C_ACC for the weight-gradient product, mutation checks that
show the per-element gate of tests/test_gpu_gemm_tn_edges.py bites, and the 32-bit descriptor arithmetic of the ping-pong
kernel at the 4 GiB case of that suite's section G.  Run with -s for the figures."""
import pytest
import torch

from oracle import gemm_tn_ref as GT

U32 = GT.U32
LENGTHS = (1, 2, 33, 64, 129, 1024, 1089, 4096, 31162)
N, K = 96, 80


# ----------------------------------------------------------------------------------------------------------------------
# host rules
# ----------------------------------------------------------------------------------------------------------------------
def test_class_boundary():
    assert GT.is_big(1024, 256, 256)
    assert not GT.is_big(1023, 256, 256) and not GT.is_big(1024, 255, 256) and not GT.is_big(1024, 256, 255)
    assert GT.tiles(256, 256, True) == 1 and GT.tiles(257, 256, True) == 2 and GT.tiles(768, 513, True) == 9
    assert GT.tiles(128, 128, False) == 1 and GT.tiles(129, 255, False) == 4


def test_splits_by_hand():
    # one 256x256 tile, M = 4096: max_s = 4, one round for every s, cost = 64 / s + 8 = 72, 40, 29.3, 24: each below 0.98 of the last
    assert GT.splits([(4096, 256, 256)]) == 4
    assert GT.rows_per_split(4096, 4) == 1024 and GT.nsplit(4096, 4) == 4
    # M = 1024: max_s = 1
    assert GT.splits([(1024, 256, 256)]) == 1
    assert GT.rows_per_split(1024, 1) == 1024
    # M = 32768 alone: 512 / s + 8 falls by more than 2 % per step up to s = 32 (31: 24.52 < 0.98 x 25.07; 32: 24.0 < 0.98 x 24.52)
    assert GT.splits([(32768, 256, 256)]) == 32
    # with the hint the fixed cost is 40: 30: 57.07; 31: 56.52 and 32: 56.0 are not below 0.98 x 57.07 = 55.93
    assert GT.splits([(32768, 256, 256)], shared=True) == 30
    assert GT.rows_per_split(32768, 30) == 1152 and GT.nsplit(32768, 30) == 29      # ceil(32768 / 30) = 1093 -> 1152; 28 x 1152 < 32768
    # M = 3073, 5000: max_s = 3, 4
    assert GT.splits([(3073, 256, 256)]) == 3 and GT.rows_per_split(3073, 3) == 1088 and GT.nsplit(3073, 3) == 3
    assert GT.splits([(5000, 256, 256)]) == 4 and GT.rows_per_split(5000, 4) == 1280
    # 300 tiles of 256x256 at M = 2048: s = 1: 2 rounds x (32 + 8) = 80; s = 2: 3 rounds x (16 + 8) = 72 < 78.4
    assert GT.splits([(2048, 256 * 15, 256 * 20)]) == 2
    # 256 tiles: s = 1: 1 x 40; s = 2: 2 x 24 = 48: stays 1
    assert GT.splits([(2048, 256 * 16, 256 * 16)]) == 1
    # the two test_gpu_row_edges.py forms
    assert GT.single_rows_per_split(4096, 384, 320) == 1024 and GT.single_rows_per_split(3000, 200, 136) == 1536


def test_launches_by_hand():
    # 49 problems of one class: 48 + 1
    L = GT.launches([(64 + i, 128, 128) for i in range(49)])
    assert [(b, len(o)) for b, o in L] == [(False, 48), (False, 1)]
    assert L[0][1] == list(range(47, -1, -1)) and L[1][1] == [48]            # descending M inside the chunk
    # stable: equal M keeps caller order
    assert GT.launches([(100, 8, 8), (200, 8, 8), (100, 16, 8), (200, 16, 8)])[0][1] == [1, 3, 0, 2]
    # mixed, interleaved: the big class first
    mix = [(1024, 256, 256) if i % 2 else (512, 256, 256) for i in range(98)]
    L = GT.launches(mix)
    assert [(b, len(o)) for b, o in L] == [(True, 48), (True, 1), (False, 48), (False, 1)]
    assert L[0][1] == list(range(1, 96, 2)) and L[1][1] == [97] and L[3][1] == [96]


def test_short_problem_and_workspace_by_hand():
    # big class: M = 32768 beside M = 1024: 2 tiles, one round, 32 splits; the short problem's ranges are 64 rows: 16 own rows
    chunk = [(32768, 256, 256), (1024, 256, 256)]
    assert GT.splits(chunk) == 32
    assert GT.rows_per_split(1024, 32) == 64 and GT.nsplit(1024, 32) == 16 and GT.nsplit(32768, 32) == 32
    assert GT.ws_bytes(chunk) == 16384 + 2 * 32 * 256 * 256 * 4
    # small class: M = 4096 beside M = 60: 4 splits, the short one has a single contributor
    chunk = [(4096, 128, 128), (60, 128, 128)]
    assert GT.splits(chunk) == 4 and GT.nsplit(60, 4) == 1 and GT.nsplit(100, 4) == 2
    need = 16384 + 2 * 4 * 128 * 128 * 4
    assert GT.ws_bytes(chunk) == need
    assert GT.uses_ws(chunk, need) and not GT.uses_ws(chunk, need - 1) and not GT.uses_ws(chunk, None)
    assert not GT.uses_ws([(4096, 128, 128), GT.Prob(60, 128, 128, True)], need)           # a device row count in the chunk
    assert not GT.uses_ws([(1024, 128, 128)], 1 << 30)                                     # one split
    assert not GT.uses_ws([(4096, 128 * 65, 128 * 64)], 1 << 40)                           # 4160 tiles > 4096 counters
    p = GT.plan([(60, 128, 128), (4096, 128, 128), (4096, 256, 512)], ws=1 << 30)
    assert [d["kernel"] for d in p] == [GT.PP, GT.SMALL]
    assert p[1]["order"] == [1, 0] and p[1]["tile0"] == [0, 1] and p[1]["nsplit"] == [4, 1] and p[1]["ws"]
    assert p[0]["tiles"] == 2 and p[0]["splits"] == 4


def test_joins_by_hand():
    # 128x128 / lock-step: one bias join per split with rows; ping-pong: per split, min(nbk, steps)
    assert GT.bias_joins(4096, 128, 4, GT.SMALL) == 4 and GT.dw_joins(4096, 4) == 4
    assert GT.bias_joins(4096, 768, 4, GT.LOCK_STEP) == 4
    assert GT.bias_joins(4096, 768, 4, GT.PP) == 12
    # K = 768 (nbk = 3), capacity 1024, one split: 64 rows = 1 step -> 1 tile column; 128 -> 2; 192 -> 3; 1024 -> 3
    assert [GT.bias_joins(1024, 768, 1, GT.PP, c) for c in (64, 128, 192, 1024, 0, 5000)] == [1, 2, 3, 3, 0, 3]
    # a device count of 1100 in 4 splits of 1024 rows: 2 splits own rows, the second 76 rows = 2 steps
    assert GT.dw_joins(4096, 4, 1100) == 2 and GT.bias_joins(4096, 768, 4, GT.PP, 1100) == 3 + 2
    jw, jb = GT.joins([(4096, 128, 128), (60, 128, 128)])
    assert jw == [4, 1] and jb == [4, 1]


def test_pp_descriptor_wraps_at_4gib():
    """Section G of the GPU suite: dy [1024, 256] with lddy = 2^21.  One split of 1024 rows: the descriptor's num_records, computed
    in 32 bits as the kernel does, is 0 -- every DMA of that operand fails the range check and returns zeros --, while every
    offset the kernel forms (row 63 of the last step, the last chunk) stays below 2^32: nothing stray is addressed."""
    M, ld = 1024, 1 << 21
    assert GT.splits([(M, 256, 256)]) == 1 and GT.rows_per_split(M, 1) == 1024
    assert M * ld * 2 == 1 << 32
    assert GT.pp_num_records(1024, ld) == 0
    assert GT.pp_num_records(1024, 264) == 1024 * 264 * 2                         # the ordinary operand is unaffected
    last = 63 * ld * 2 + 255 * 2 + (1024 // 64 - 1) * 64 * ld * 2                 # per-lane offset + the last step's scalar offset
    assert last < 1 << 32
    # the launcher's guard: such a chunk leaves the ping-pong kernel, whichever operand it is; M = 1023 is the 128x128 class
    assert GT.kernel([GT.Prob(M, 256, 256, False, ld, 264)]) == GT.LOCK_STEP
    assert GT.kernel([GT.Prob(M, 256, 256, False, 264, ld)]) == GT.LOCK_STEP
    assert GT.kernel([GT.Prob(M, 256, 256, False, ld // 2, 264)]) == GT.PP
    assert GT.kernel([GT.Prob(1023, 256, 256, False, ld, 264)]) == GT.SMALL
    # it holds for the chunk: an ordinary problem sharing the launch goes with it
    assert GT.kernel([GT.Prob(M, 256, 256, False, ld, 264), GT.Prob(1500, 512, 256)]) == GT.LOCK_STEP
    # (beside M = 2048 the launch has two splits of 512 rows = 2 GiB: the descriptor holds, the ping-pong kernel stays)
    assert GT.kernel([GT.Prob(M, 256, 256, False, ld, 264), GT.Prob(2048, 512, 256)]) == GT.PP
    # the production reach of the hole: the fp32x3 loss-gradient planes (ld 91,584): 23,449 rows per split
    assert GT.pp_num_records(23449, 91584) != 23449 * 91584 * 2


# ----------------------------------------------------------------------------------------------------------------------
# the measurement behind C_ACC, and mutations
# ----------------------------------------------------------------------------------------------------------------------
def _operands(M, seed):
    g = torch.Generator().manual_seed(seed * 1009 + M)
    dy = torch.randn((M, N), generator=g)
    x = torch.randn((M, K), generator=g)
    dy[:, 0::7] *= 1e3                       # hostile along N and K only: the reduction axis stays well-scaled
    dy[:, 1::5] *= 1e-3
    x[:, 0::9] *= 1e3
    x[:, 2::11] *= 1e-3
    return dy.bfloat16(), x.bfloat16()


def _fp32(dy, x, prior_w, prior_b):
    """The reference implementation under measurement: torch's CPU float32 product, joined to the prior by one addition."""
    return prior_w + dy.float().t() @ x.float(), prior_b + dy.float().sum(0)


@pytest.fixture(scope="module")
def cases():
    out = {}
    for M in LENGTHS:
        dy, x = _operands(M, 1)
        g = torch.Generator().manual_seed(M)
        pw, pb = torch.randn((N, K), generator=g), torch.randn(N, generator=g)
        r = GT.problem(dy, x, pw, pb, M, N, K)
        out[M] = (dy, x, pw, pb, r, GT.gate(r, pw, pb, 1, 1))
    return out


def test_c_acc_measured_on_the_fp32_product():
    worst_all = 0.0
    for M in LENGTHS:
        worst = 0.0
        for seed in (1, 2, 3):
            dy, x = _operands(M, seed)
            ref = dy.double().t() @ x.double()
            S = dy.double().abs().t() @ x.double().abs()
            got = (dy.float().t() @ x.float()).double()
            worst = max(worst, float(((got - ref).abs() / (U32 * S)).max()))
        print(f"[gemm_tn ref] M = {M:6d}: worst |fp32 - fp64| / (2^-24 S) = {worst:.3f}  (x 8 = {8 * worst:.2f}, C_ACC = {GT.C_ACC:g})")
        worst_all = max(worst_all, worst)
        assert 8.0 * worst <= GT.C_ACC, (M, worst)
    assert worst_all > 0.0


def test_reference_product_passes_the_gate_with_margin(cases):
    """The fp32 CPU product against the gate.  Where the constant decides (live >= C_ACC) the pure accumulation (zero prior, no
    join) stays within 1/8 of E: that IS the 8 x margin of C_ACC.  Below C_ACC rows E is the order-free bound live 2^-24 S,
    a theorem without a margin to assert (two rows: one addition, up to half of E), so there the condition is <= 1.  With a
    random prior joined by one fp32 addition (J = 1) the product passes at every length."""
    for M in LENGTHS:
        dy, x, pw, pb, r, (Ew, Eb) = cases[M]
        gw, gb = _fp32(dy, x, pw, pb)
        rw, rb = GT.worst_ratio(gw, r["ref_w"], Ew), GT.worst_ratio(gb, r["ref_b"], Eb)
        zw, zb = torch.zeros_like(pw), torch.zeros_like(pb)
        g0w, g0b = _fp32(dy, x, zw, zb)
        aw = GT.worst_ratio(g0w, r["ref_w"] - pw.double(), r["acc_w"])
        ab = GT.worst_ratio(g0b, r["ref_b"] - pb.double(), r["acc_b"])
        print(f"[gemm_tn ref] M = {M:6d}: fp32 product |err| / E: accumulation alone dw {aw:.4f} dbias {ab:.4f}; "
              f"on a prior (J = 1) dw {rw:.4f} dbias {rb:.4f}")
        assert rw <= 1.0 and rb <= 1.0, (M, rw, rb)
        lim = 1.0 / 8 if M >= GT.C_ACC else 1.0
        assert aw <= lim and ab <= lim, (M, aw, ab)


def _fail_rate(got, ref, E):
    return float(((got.double() - ref).abs() > E).double().mean())


def test_mutations_fail_the_gate(cases):
    for M in LENGTHS:
        dy, x, pw, pb, r, (Ew, Eb) = cases[M]
        rates = {}
        if M > 1:
            gw, gb = _fp32(dy[:-1], x[:-1], pw, pb)                                     # the last reduction row dropped
            rates["row dropped"] = _fail_rate(gw, r["ref_w"], Ew)
            assert _fail_rate(gb, r["ref_b"], Eb) >= 0.5, M
            mid = M // 2
            gw, _ = _fp32(torch.cat([dy[:mid], dy[mid + 1:]]), torch.cat([x[:mid], x[mid + 1:]]), pw, pb)
            rates["middle row dropped"] = _fail_rate(gw, r["ref_w"], Ew)
        gw, gb = _fp32(torch.cat([dy, dy[-1:]]), torch.cat([x, x[-1:]]), pw, pb)        # the last live row counted twice
        rates["last row twice"] = _fail_rate(gw, r["ref_w"], Ew)
        assert _fail_rate(gb, r["ref_b"], Eb) >= 0.5, M
        _, gb = _fp32(dy, x, pw, pb)
        rates["dbias shifted one column"] = _fail_rate(torch.roll(gb - pb, 1) + pb, r["ref_b"], Eb)
        print(f"[gemm_tn ref] M = {M:6d}: fraction of elements outside E: " + "  ".join(f"{k}: {v:.3f}" for k, v in rates.items()))
        for k, v in rates.items():
            assert v >= 0.5, (M, k, v)


def test_swapped_descriptors_and_aliases():
    """A group of two problems of one shape: dw of one swapped with its neighbour's fails; two problems into one dw pass
    against the summed reference and fail against either alone."""
    M = 129
    (dy0, x0), (dy1, x1) = _operands(M, 5), _operands(M, 6)
    g = torch.Generator().manual_seed(9)
    pw0, pw1, pb = torch.randn((N, K), generator=g), torch.randn((N, K), generator=g), torch.randn(N, generator=g)
    r0, r1 = GT.problem(dy0, x0, pw0, pb, M, N, K), GT.problem(dy1, x1, pw1, pb, M, N, K)
    g0, g1 = _fp32(dy0, x0, pw0, pb)[0], _fp32(dy1, x1, pw1, pb)[0]
    E0, E1 = GT.gate(r0, pw0, pb, 1, 1)[0], GT.gate(r1, pw1, pb, 1, 1)[0]
    assert GT.worst_ratio(g0, r0["ref_w"], E0) <= 1.0 and GT.worst_ratio(g1, r1["ref_w"], E1) <= 1.0
    assert _fail_rate(g1, r0["ref_w"], E0) >= 0.5 and _fail_rate(g0, r1["ref_w"], E1) >= 0.5
    # the right products on the neighbour's prior (a descriptor whose dw pointer alone is swapped)
    assert _fail_rate(g0 - pw0 + pw1, r0["ref_w"], E0) >= 0.5
    ra = GT.problem([dy0, dy1, dy0], [x0, x1, x1], pw0, pb, [M, M, 7], N, K, bias=[True, True, False])
    Ew, Eb = GT.gate(ra, pw0, pb, 3, 2)
    gw = pw0 + dy0.float().t() @ x0.float() + dy1.float().t() @ x1.float() + dy0[:7].float().t() @ x1[:7].float()
    gb = pb + dy0.float().sum(0) + dy1.float().sum(0)
    assert GT.worst_ratio(gw, ra["ref_w"], Ew) <= 1.0 and GT.worst_ratio(gb, ra["ref_b"], Eb) <= 1.0
    assert _fail_rate(g0, ra["ref_w"], Ew) >= 0.5
    assert _fail_rate(gb + dy0[:7].float().sum(0), ra["ref_b"], Eb) >= 0.5         # the third problem must not reach dbias
