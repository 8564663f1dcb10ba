"""Every form of the weight-gradient GEMM (unimm_gemm_tn, unimm_gemm_tn_grouped, unimm_gemm_tn_grouped_ws: csrc/gemm.hip)
against the float64 restatement of one call (oracle/gemm_tn_ref.py), element by element.

Gate (oracle/gemm_tn_ref.py has the derivation): |got - ref| <= E for EVERY element of dw and dbias,
E = min(32, live) 2^-24 S  +  J 2^-24 (|prior| + S),  S = |dy|^T |x| (dbias: sum |dy|), J = the number of fp32 additions that
join partial results in the element, counted from the launcher's own rules (splits that own rows; for the ping-pong kernel's
bias also the tile columns that own reduction steps).  dw and dbias are fp32: no output-rounding term.  The operands are
well-scaled along the reduction axis M (the constant 32 is measured for that: tests/test_gemm_tn_ref_cpu.py); all hostility is
in N and K: columns of dy x1e3 / x1e-3 on strides 61 / 67, columns of x x1e3 on stride 59 (the outputs span 12 orders of
magnitude), and the last two dy columns equal up to sign with priors that cancel them (outputs ~ 0 beside O(1)).

Every launch runs under the launch profiler (lib.prof_enable(2) / prof_collect()): which kernel symbols ran, and how many
launches of each, must equal what the oracle's restatement of the launcher says -- so a case provably reaches the form it is
named after (gemm_tn_pp, gemm_tn<128x128>, gemm_tn<256x256 lock-step>).

Poison.  dy and x are views at a column offset (a multiple of 8) of wider NaN-filled buffers: rows past M and past the device
row count hold NaN, so do the columns past N / K, the readable pad up to the next multiple of 8 included (the header allows
reading those; they must reach no stored element).  dw is a view (row 1, column 3, lddw > K) of a buffer pre-filled with a
NaN bit pattern, dbias a view of such a vector: every bit outside [0, N) x [0, K) and [0, N) must come back unchanged.  The
priors are random, so += is tested, not =.

Sections
  A  geometry x form, one problem: the 128x128 kernel at N, K in {1 .. 257} and M in {1 .. 1023}; the ping-pong kernel at
     N, K in {256 .. 768}, M in {1024 .. 3000}; the class boundary; the lock-step 256x256 loop (shared_chip bit 1); with and
     without dbias, overwrite, m_dev absent / = M / > M / < M / 0, unimm_gemm_tn and the grouped entry points; the ping-pong
     bias dealing with fewer, as many and more reduction steps than tile columns.
  B  splits and workspace: 2 .. 32 splits under both values of the chip-sharing hint, on the atomic path and in a workspace of
     exactly ws_bytes() inside a sentinel-filled buffer (slabs written per tile = the oracle's nsplit; counters left zero;
     nothing past the end; a second launch on the same workspace); a workspace one byte short; a device row count in the
     chunk; a short problem whose nsplit is below the group's splits, and one with a single contributor and overwrite.
  C  grouping: 1, 2, 3, 47, 48, 49, 97 problems of one class and 49 + 49 of both classes interleaved (TN_MAXG = 48: the
     chunking path), first / middle / last problem with many tiles, unequal and equal M (the stable sort), aliased dw and
     dbias inside a launch, across the two launches of a class and across the classes.
  D  the three-problem split-operand product of the fp32x3 engine (engine_x3._wgrad3) over column planes of lib.x3_split's
     output, two of the three adding into one dbias; the reference is float64 on the bf16 plane values actually passed.
  E  the decoder-input formulation of engine._decoder_dx: the long axis is the reduction, one zeroed slab per chunk; per
     element, and bit-identical between two runs.
  F  refusals, each before any launch and with the outputs bit-unchanged.
  G  a split whose rows span 4 GiB of an operand.  Reading gemm_tn_pp_kernel showed that its buffer descriptors are built in
     32 bits (num_records = rows * ld * 2): at 4 GiB the operand reads as zeros and the gradient comes back as its prior,
     without an error (tests/test_gemm_tn_ref_cpu.py has the arithmetic).  launch_tn_group now sends such a launch to the
     lock-step loop (64-bit addressing), as launch_nt does for its ping-pong tile; this section is the case that needs it.

A module fixture prints the worst |err| / E of dw and dbias per section and kernel symbol (run with -s)."""
import ctypes as C
from collections import Counter, defaultdict

import pytest
import torch

from oracle import gemm_tn_ref as GT

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN32 = 0x7FA5A5A5
SENT8, SENT32 = 0xA5, 0xA5A5A5A5 - (1 << 32)
ROWPAD = 96
BF16, F32 = torch.bfloat16, torch.float32

STATS = defaultdict(lambda: [0, 0.0, 0.0])       # (section, kernel symbol) -> [gated launches, worst dw ratio, worst dbias ratio]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if not STATS:
        return
    print("\n\n==== unimm_gemm_tn edges: gated launches and worst |err| / E ====")
    print(f"{'section':8s}{'kernel':30s}{'launches':>9s}{'dw':>9s}{'dbias':>9s}")
    for (sec, kern), (n, w, b) in sorted(STATS.items()):
        print(f"{sec:8s}{kern:30s}{n:9d}{w:9.3f}{b:9.3f}")
    by = defaultdict(lambda: [0, 0.0, 0.0])
    for (sec, kern), (n, w, b) in STATS.items():
        for k in kern.split(" + "):
            by[k] = [by[k][0] + n, max(by[k][1], w), max(by[k][2], b)]
    for k, (n, w, b) in sorted(by.items()):
        print(f"{'all':8s}{k:30s}{n:9d}{w:9.3f}{b:9.3f}")


def _rup(a, b):
    return (a + b - 1) // b * b


def _sent32(*shape):
    return torch.full(shape, NAN32, dtype=torch.int32, device=DEV).view(F32)


class Dw:
    """One dw target: a [N, K] view at (1, 3) of a sentinel-filled buffer with lddw > K, and its random (or zero) prior."""

    def __init__(self, N, K, gen, zero=False, extra=5):
        self.N, self.K = N, K
        self.buf = _sent32(N + 3, K + 3 + extra)
        self.view = self.buf[1:1 + N, 3:3 + K]
        self.prior = torch.zeros((N, K), device=DEV) if zero else torch.randn((N, K), generator=gen, device=DEV)
        self.arm()

    def arm(self):
        self.view.copy_(self.prior)

    def outside_unchanged(self):
        iv = self.buf.view(torch.int32).clone()
        iv[1:1 + self.N, 3:3 + self.K] = NAN32
        return bool((iv == NAN32).all())

    def untouched(self):
        return self.outside_unchanged() and torch.equal(self.view.contiguous().view(torch.int32), self.prior.view(torch.int32))


class Db:
    def __init__(self, N, gen):
        self.N = N
        self.buf = _sent32(N + 16)
        self.view = self.buf[4:4 + N]
        self.prior = torch.randn(N, generator=gen, device=DEV)
        self.arm()

    def arm(self):
        self.view.copy_(self.prior)

    def outside_unchanged(self):
        iv = self.buf.view(torch.int32).clone()
        iv[4:4 + self.N] = NAN32
        return bool((iv == NAN32).all())

    def untouched(self):
        return self.outside_unchanged() and torch.equal(self.view.contiguous().view(torch.int32), self.prior.view(torch.int32))


def _poisoned(rows, cols, off):
    buf = torch.full((rows + ROWPAD, _rup(off + cols + 8, 8)), float("nan"), dtype=BF16, device=DEV)
    return buf[:rows, off:off + cols]


class Op:
    """One problem: poisoned operands, its dw / dbias targets and what the launcher is told."""

    def __init__(self, M, N, K, seed, dw=None, db=True, count=None, overwrite=False, dyoff=8, xoff=16, hostile=True, cancel=True,
                 dy=None, x=None, values=None):
        g = torch.Generator(device=DEV).manual_seed(seed * 7919 + M * 31 + N * 17 + K)
        self.M, self.N, self.K, self.count, self.overwrite = M, N, K, count, overwrite
        self.live = live = GT.live_rows(M, count)
        self.dy = _poisoned(M, N, dyoff) if dy is None else dy
        self.x = _poisoned(M, K, xoff) if x is None else x
        assert self.dy.data_ptr() % 16 == 0 and self.x.data_ptr() % 16 == 0
        if values is None:
            dyf = torch.randn((live, N), generator=g, device=DEV)
            xf = torch.randn((live, K), generator=g, device=DEV)
            if hostile:                          # along N and K only: the reduction axis stays well-scaled
                dyf[:, 0::61] *= 1e3
                dyf[:, 1::67] *= 1e-3
                xf[:, 0::59] *= 1e3
            own = dw is None and not overwrite and cancel and N >= 2
            if own:
                dyf[:, N - 2] = -dyf[:, N - 1]
            self.dy[:live] = dyf.to(BF16)
            self.x[:live] = xf.to(BF16)
        else:
            own = False
        self.dw = Dw(N, K, g, zero=overwrite) if dw is None else dw
        self.db = Db(N, g) if db is True else (db or None)
        if own:
            # dw rows N-1 and N-2 (and their dbias elements) cancel against the prior: ~ 0 beside O(1)
            P = (self.dy[:live, N - 1].double()[None, :] @ self.x[:live].double()).float()[0]
            self.dw.prior[N - 1], self.dw.prior[N - 2] = -P, P
            self.dw.arm()
            if self.db is not None and db is True:
                sb = self.dy[:live, N - 1].double().sum().float()
                self.db.prior[N - 1], self.db.prior[N - 2] = -sb, sb
                self.db.arm()
        self.m_dev = torch.tensor([count], dtype=torch.int32, device=DEV) if count is not None else None

    def args(self):
        return (self.dy, self.x, self.dw.view, self.M, self.N, self.K, self.db.view if self.db is not None else None, self.m_dev,
                self.overwrite)

    def spec(self):
        return GT.Prob(self.M, self.N, self.K, self.count is not None, self.dy.stride(0), self.x.stride(0))


def _launch(ops, shared=False, lock_step=False, ws=None, single=False):
    """Run one call under the launch profiler; assert the kernel symbols and launch counts the oracle predicts; -> plan"""
    from unimm_amd import lib
    plan = GT.plan([o.spec() for o in ops], shared, lock_step, ws.numel() if ws is not None else None)
    flags = (1 if shared else 0) | (2 if lock_step else 0)
    lib.prof_enable(2)
    try:
        if single:
            o, = ops
            assert not o.overwrite and not flags and ws is None
            lib.gemm_tn(o.dy, o.x, o.dw.view, M=o.M, N=o.N, K=o.K, dbias=o.db.view if o.db is not None else None, m_dev=o.m_dev)
        else:
            lib.gemm_tn_grouped([o.args() for o in ops], shared=flags if (flags or ws is not None) else None, ws=ws)
        torch.cuda.synchronize()
        got = {k: v[2] for k, v in lib.prof_collect().items()}
    finally:
        lib.prof_enable(0)
    want = dict(Counter(L["kernel"] for L in plan))
    assert got == want, ("kernel symbols x launches", got, "expected", want)
    return plan


def _check(section, ops, plan, shared=False, lock_step=False):
    """Sentinels + the per-element gate over every dw and dbias of the call; -> (worst dw ratio, worst dbias ratio)"""
    torch.cuda.synchronize()
    specs = [o.spec() for o in ops]
    jw, jb = GT.joins(specs, shared, lock_step, [o.count for o in ops])
    kern = {i: L["kernel"] for L in plan for i in L["order"]}
    by_dw, by_db = defaultdict(list), defaultdict(list)
    for i, o in enumerate(ops):
        by_dw[id(o.dw)].append(i)
        if o.db is not None:
            by_db[id(o.db)].append(i)
    worst_w = worst_b = 0.0
    for idx in by_dw.values():
        t = ops[idx[0]].dw
        what = (section, [(ops[i].M, ops[i].N, ops[i].K, ops[i].count, ops[i].overwrite) for i in idx])
        assert t.outside_unchanged(), ("dw: written outside [0, N) x [0, K)",) + what
        r = GT.problem([ops[i].dy for i in idx], [ops[i].x for i in idx], t.prior, None, [ops[i].live for i in idx], t.N, t.K)
        Ew, _ = GT.gate(r, t.prior, None, sum(jw[i] for i in idx), 0)
        ratio = GT.worst_ratio(t.view, r["ref_w"], Ew)
        if all(ops[i].live == 0 for i in idx):
            assert t.untouched(), ("dw changed by a problem without rows",) + what
        key = (section, " + ".join(sorted({kern[i] for i in idx})))
        STATS[key][1] = max(STATS[key][1], ratio)
        worst_w = max(worst_w, ratio)
        assert ratio <= 1.0, ("dw |err| / E", ratio, "joins", [jw[i] for i in idx]) + what
    for idx in by_db.values():
        t = ops[idx[0]].db
        what = (section, [(ops[i].M, ops[i].N, ops[i].K, ops[i].count) for i in idx])
        assert t.outside_unchanged(), ("dbias: written outside [0, N)",) + what
        r = GT.colsums([ops[i].dy for i in idx], t.prior, [ops[i].live for i in idx], t.N)
        ratio = GT.worst_ratio(t.view, r["ref_b"], GT.gate_b(r, t.prior, sum(jb[i] for i in idx)))
        if all(ops[i].live == 0 for i in idx):
            assert t.untouched(), ("dbias changed by a problem without rows",) + what
        key = (section, " + ".join(sorted({kern[i] for i in idx})))
        STATS[key][2] = max(STATS[key][2], ratio)
        worst_b = max(worst_b, ratio)
        assert ratio <= 1.0, ("dbias |err| / E", ratio, "joins", [jb[i] for i in idx]) + what
    for L in plan:
        STATS[(section, L["kernel"])][0] += 1
    return worst_w, worst_b


def _run(section, ops, **kw):
    single = kw.pop("single", False)
    ws = kw.pop("ws", None)
    plan = _launch(ops, ws=ws, single=single, **kw)
    return plan, _check(section, ops, plan, **kw)


# ----------------------------------------------------------------------------------------------------------------------
# A. geometry x form, one problem
# ----------------------------------------------------------------------------------------------------------------------
NK_SMALL = [1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 136, 255, 257]
M_SMALL = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1023]
NK_PP = [256, 257, 264, 383, 384, 385, 511, 512, 513, 768]
M_PP = [1024, 1025, 1087, 1088, 1089, 2047, 2048, 2049, 3000]
MODES = [None, "eq", "gt", "zero", "lt"]


def _count(mode, M):
    return {None: None, "eq": M, "gt": M + 61, "zero": 0, "lt": max(1, M // 2 + 1)}[mode]


def _options(i):
    """Rotating options (periods 3, 4, 5, 7: no full product): bias, overwrite, device-count mode, entry point, column offsets"""
    over = i % 4 == 1
    return dict(db=(i % 3 != 0), overwrite=over, mode=MODES[i % 5], single=(i % 7 == 0 and not over), dyoff=8 * (i % 3),
                xoff=8 * ((i + 1) % 4))


def _case_a(M, N, K, i, **kw):
    o = _options(i)
    op = Op(M, N, K, seed=i, db=o["db"], count=_count(o["mode"], M), overwrite=o["overwrite"], dyoff=o["dyoff"], xoff=o["xoff"])
    return op, _run("A", [op], single=o["single"] and not kw, **kw)


def test_a_small_form_geometry():
    seen_n, seen_k, seen_m = set(), set(), set()
    for i in range(32):
        N, K, M = NK_SMALL[i % 16], NK_SMALL[(5 * i + 2 + 3 * (i // 16)) % 16], M_SMALL[(7 * i + i // 12) % 12]
        op, (plan, _) = _case_a(M, N, K, i)
        assert [L["kernel"] for L in plan] == [GT.SMALL]
        seen_n.add(N), seen_k.add(K), seen_m.add(M)
    assert seen_n == set(NK_SMALL) and seen_k == set(NK_SMALL) and seen_m == set(M_SMALL)


def test_a_ping_pong_geometry():
    seen_n, seen_k, seen_m = set(), set(), set()
    for i in range(20):
        N, K, M = NK_PP[i % 10], NK_PP[(3 * i + 1 + i // 10) % 10], M_PP[(i + i // 9) % 9]
        op, (plan, _) = _case_a(M, N, K, 100 + i)
        assert [L["kernel"] for L in plan] == [GT.PP]
        seen_n.add(N), seen_k.add(K), seen_m.add(M)
    assert seen_n == set(NK_PP) and seen_k == set(NK_PP) and seen_m == set(M_PP)


@pytest.mark.parametrize("M,N,K,kern", [(1023, 256, 256, GT.SMALL), (1024, 255, 256, GT.SMALL), (1024, 256, 255, GT.SMALL),
                                        (1024, 256, 256, GT.PP)])
def test_a_class_boundary(M, N, K, kern):
    for i in (2, 5):                                   # both with dbias; 2: m_dev > M; 5: overwrite, no m_dev
        op, (plan, _) = _case_a(M, N, K, i)
        assert [L["kernel"] for L in plan] == [kern]


@pytest.mark.parametrize("i", [1, 3, 6, 12])
def test_a_lock_step_loop(i):
    """The lock-step 256x256 loop (shared_chip bit 1) on four of the ping-pong cases."""
    N, K, M = NK_PP[i % 10], NK_PP[(3 * i + 1 + i // 10) % 10], M_PP[(i + i // 9) % 9]
    op, (plan, _) = _case_a(M, N, K, 100 + i, lock_step=True)
    assert [L["kernel"] for L in plan] == [GT.LOCK_STEP]


@pytest.mark.parametrize("count", [64, 128, 192, 1024])
def test_a_ping_pong_bias_dealing(count):
    """K = 768: three tile columns; tile column tk sums the reduction steps t = tk mod 3.  64 / 128 / 192 / 1024 live rows
    = fewer steps than tile columns, then as many, then more."""
    op = Op(1024, 300, 768, seed=300 + count, count=count)
    plan, _ = _run("A", [op])
    assert [L["kernel"] for L in plan] == [GT.PP]
    assert GT.bias_joins(1024, 768, 1, GT.PP, count) == min(3, count // 64)


# ----------------------------------------------------------------------------------------------------------------------
# B. splits and workspace
# ----------------------------------------------------------------------------------------------------------------------
def _ws_buf(need, extra=4096):
    buf = torch.full((need + extra + 256,), SENT8, dtype=torch.uint8, device=DEV)
    buf = buf[-buf.data_ptr() % 256:][:need + extra]                 # a 256-byte aligned start
    buf[:GT.COUNTER_BYTES] = 0
    assert buf.data_ptr() % 256 == 0
    return buf


def _ws_check(buf, need, L, what):
    """Counters zero, nothing past `need` touched, and exactly the slabs (tile, split < nsplit of the tile's problem) written."""
    torch.cuda.synchronize()
    assert int(buf[:GT.COUNTER_BYTES].count_nonzero()) == 0, ("arrival counters not left at zero",) + what
    assert bool((buf[need:] == SENT8).all()), ("workspace written past ws_bytes()",) + what
    tb = GT.tile_dim(L["big"])
    slabs = buf[GT.COUNTER_BYTES:GT.COUNTER_BYTES + L["tiles"] * L["splits"] * tb * tb * 4].view(torch.int32)
    slabs = slabs.view(L["tiles"], L["splits"], tb * tb)
    sent = (slabs == SENT32).sum(-1)                     # sentinel words left per slab
    want = torch.zeros((L["tiles"], L["splits"]), dtype=torch.bool)
    bounds = L["tile0"] + [L["tiles"]]
    for j, ns in enumerate(L["nsplit"]):
        if L["ws"] and ns > 1:
            want[bounds[j]:bounds[j + 1], :ns] = True
    written = (sent < tb * tb).cpu()
    assert torch.equal(written, want), ("slabs written per tile != the oracle's nsplit", written.sum(1).tolist(), want.sum(1).tolist()) + what
    assert int(sent.cpu()[want].sum()) == 0, ("a published slab has unwritten words",) + what


B_SHAPES = [(256, 256), (257, 512), (128, 128), (136, 129)]
B_CASES = [(M, sh, j) for j, M in enumerate((2048, 3073, 4096, 5000, 32768)) for sh in (False, True)]


@pytest.mark.parametrize("M,shared,j", B_CASES)
def test_b_splits_atomic_and_workspace(M, shared, j):
    N, K = B_SHAPES[(2 * j + shared) % 4]
    seed = 400 + 2 * j + shared
    want_s = GT.splits([(M, N, K)], shared)
    assert want_s == {2048: 2, 3073: 3, 4096: 4, 5000: 4, 32768: 30 if shared else 32}[M]
    # atomic path
    op = Op(M, N, K, seed=seed)
    plan, _ = _run("B", [op], shared=shared)
    assert plan[0]["splits"] == want_s and not plan[0]["ws"]
    # workspace of exactly ws_bytes(); a second launch on it
    need = GT.ws_bytes([(M, N, K)], shared=shared)
    buf = _ws_buf(need)
    for rep in range(2):
        op = Op(M, N, K, seed=seed + 50 * rep)
        plan, _ = _run("B", [op], shared=shared, ws=buf[:need])
        assert plan[0]["ws"] and plan[0]["ws_bytes"] == need and plan[0]["nsplit"] == [GT.nsplit(M, want_s)]
        _ws_check(buf, need, plan[0], (M, N, K, shared, rep))
    # one byte short: the atomic path, slabs untouched
    buf = _ws_buf(need)
    op = Op(M, N, K, seed=seed)
    plan, _ = _run("B", [op], shared=shared, ws=buf[:need - 1])
    assert not plan[0]["ws"]
    _ws_check(buf, need, plan[0], (M, N, K, shared, "one byte short"))


@pytest.mark.parametrize("N,K", [(300, 256), (100, 136)])
def test_b_device_count_ignores_workspace(N, K):
    ops = [Op(4096, N, K, seed=450), Op(2048, N, K, seed=451, count=1500)]
    need = GT.ws_bytes([o.spec() for o in ops])
    buf = _ws_buf(need)
    plan, _ = _run("B", ops, ws=buf[:need])
    assert len(plan) == 1 and plan[0]["splits"] == 4 and not plan[0]["ws"]
    _ws_check(buf, need, plan[0], (N, K, "m_dev in the chunk"))


@pytest.mark.parametrize("with_ws", [False, True])
def test_b_short_problem_in_a_group(with_ws):
    # ping-pong: 32 splits of the long problem; the short one's ranges are 64 rows, 16 of them own rows
    ops = [Op(1024, 257, 256, seed=460), Op(32768, 256, 256, seed=461)]
    specs = [o.spec() for o in ops]
    need = GT.ws_bytes(specs)
    buf = _ws_buf(need) if with_ws else None
    plan, _ = _run("B", ops, ws=buf[:need] if with_ws else None)
    assert len(plan) == 1 and plan[0]["order"] == [1, 0] and plan[0]["splits"] == 32 and plan[0]["nsplit"] == [32, 16]
    assert plan[0]["ws"] == with_ws
    if with_ws:
        _ws_check(buf, need, plan[0], ("short problem, ping-pong",))
    # 128x128: 4 splits; a problem of 100 rows has 2, one of 60 rows a single contributor -- with overwrite it is stored plainly
    ops = [Op(60, 100, 128, seed=462, overwrite=True), Op(4096, 128, 128, seed=463), Op(100, 64, 129, seed=464)]
    specs = [o.spec() for o in ops]
    need = GT.ws_bytes(specs)
    buf = _ws_buf(need) if with_ws else None
    plan, _ = _run("B", ops, ws=buf[:need] if with_ws else None)
    assert len(plan) == 1 and plan[0]["order"] == [1, 2, 0] and plan[0]["splits"] == 4 and plan[0]["nsplit"] == [4, 2, 1]
    if with_ws:
        _ws_check(buf, need, plan[0], ("short problems, 128x128",))


# ----------------------------------------------------------------------------------------------------------------------
# C. grouping
# ----------------------------------------------------------------------------------------------------------------------
def _small_op(i, n, seed0, **kw):
    many = i in (0, n // 2, n - 1)                                   # many tiles at both ends of the tile0 search and inside
    N, K = (300, 200) if many else (1 + (i * 29) % 128, 1 + (i * 53) % 128)
    M = 40 + ((i - i % 10 if i % 10 == 1 else i) * 37) % 211         # problems 10j and 10j + 1 have equal M: caller order holds
    return Op(M, N, K, seed=seed0 + i, db=(i % 2 == 0), cancel=(i % 3 == 0), **kw)


def _big_op(i, n, seed0, **kw):
    many = i in (0, n // 2, n - 1)
    N, K = (513, 520) if many else (256, 256 + 8 * (i % 4) * (i % 2))    # one tile, or two
    j = i - 1 if i % 10 == 1 else i
    M = 1024 + 64 * ((j * 7) % 5) + j % 3
    return Op(M, N, K, seed=seed0 + i, db=(i % 2 == 1), cancel=(i % 3 == 0), **kw)


@pytest.mark.parametrize("n", [1, 2, 3, 47, 48, 49, 97])
def test_c_groups_of_one_class(n):
    ops = [_small_op(i, n, 1000 * n) for i in range(n)]
    plan, _ = _run("C", ops)
    assert [len(L["order"]) for L in plan] == [48] * (n // 48) + ([n % 48] if n % 48 else [])
    assert len(plan) == -(-n // GT.TN_MAXG)
    if n >= 12:
        first = plan[0]["order"]
        assert first != sorted(first), "the sort by M was meant to reorder the descriptors"
        assert first.index(10) + 1 == first.index(11), "equal M: caller order"


def test_c_mixed_classes_interleaved():
    ops = []
    for i in range(49):
        ops.append(_small_op(i, 49, 5000))
        ops.append(_big_op(i, 49, 6000))
    plan, _ = _run("C", ops)
    assert [(L["kernel"], len(L["order"])) for L in plan] == [(GT.PP, 48), (GT.PP, 1), (GT.SMALL, 48), (GT.SMALL, 1)]


def test_c_big_class_group_of_49_lock_step():
    ops = [_big_op(i, 49, 7000) for i in range(49)]
    plan, _ = _run("C", ops, lock_step=True)
    assert [(L["kernel"], len(L["order"])) for L in plan] == [(GT.LOCK_STEP, 48), (GT.LOCK_STEP, 1)]


def test_c_aliased_outputs():
    g = torch.Generator(device=DEV).manual_seed(77)
    # two problems into one dw (the second without bias), two of different K into one dbias
    a = Op(100, 70, 90, seed=801)
    b = Op(231, 70, 90, seed=802, dw=a.dw, db=None)
    c = Op(50, 70, 33, seed=803, db=a.db)
    plan, _ = _run("C", [a, b, c])
    assert len(plan) == 1
    # an alias across the two launches of a 49-problem class
    ops = [_small_op(i, 49, 8000) for i in range(48)]
    ops.append(Op(77, ops[0].N, ops[0].K, seed=8048, dw=ops[0].dw, db=ops[0].db))
    plan, _ = _run("C", ops)
    assert [len(L["order"]) for L in plan] == [48, 1]
    # an alias across the classes: the same N and K at M = 1024 (ping-pong) and M = 512 (128x128)
    dw, db = Dw(256, 256, g), Db(256, g)
    ops = [Op(1024, 256, 256, seed=811, dw=dw, db=db), Op(512, 256, 256, seed=812, dw=dw, db=db)]
    plan, _ = _run("C", ops)
    assert [L["kernel"] for L in plan] == [GT.PP, GT.SMALL]


# ----------------------------------------------------------------------------------------------------------------------
# D. split-operand use (engine_x3._wgrad3)
# ----------------------------------------------------------------------------------------------------------------------
def _planes(M, C_, Cp, gen, scale_cols):
    """fp32 [M, C] -> x-type split operand [M + pad, 3 Cp] by lib.x3_split; rows past M and columns C .. Cp of the first two
    planes NaN afterwards (the weight-gradient problems may read up to the next multiple of 8, and must use none of it)."""
    from unimm_amd import lib
    src = torch.randn((M, C_), generator=gen, device=DEV)
    for start, stride, s in scale_cols:
        src[:, start::stride] *= s
    out3 = torch.zeros((M + ROWPAD, 3 * Cp), dtype=BF16, device=DEV)
    lib.x3_split(src, out3=out3, rows=M, cols=C_, cp=Cp)
    torch.cuda.synchronize()
    out3[M:] = float("nan")
    out3[:, C_:Cp] = float("nan")
    out3[:, Cp + C_:2 * Cp] = float("nan")
    return out3


@pytest.mark.parametrize("M,N,K,xcol0,kern", [(1100, 1601, 1024, 0, GT.PP), (300, 768, 264, 0, GT.SMALL), (1024, 256, 256, 64, GT.PP)])
def test_d_split_operand_product(M, N, K, xcol0, kern):
    g = torch.Generator(device=DEV).manual_seed(900 + M)
    Np, Kp = _rup(N, 64), _rup(xcol0 + K, 64)
    dy3 = _planes(M, N, Np, g, [(0, 61, 1e3), (1, 67, 1e-3)])
    x3 = _planes(M, xcol0 + K, Kp, g, [(0, 59, 1e3)])
    dyh, dyl = dy3[:M, :N], dy3[:M, Np:Np + N]
    xh, xl = x3[:M, xcol0:xcol0 + K], x3[:M, Kp + xcol0:Kp + xcol0 + K]
    assert float(dyl.float().abs().max()) > 0 and float(xl.float().abs().max()) > 0
    a = Op(M, N, K, seed=901, dy=dyh, x=xh, values="given")
    b = Op(M, N, K, seed=902, dy=dyl, x=xh, values="given", dw=a.dw, db=a.db)
    c = Op(M, N, K, seed=903, dy=dyh, x=xl, values="given", dw=a.dw, db=None)
    plan, _ = _run("D", [a, b, c])
    assert [L["kernel"] for L in plan] == [kern] and len(plan[0]["order"]) == 3


# ----------------------------------------------------------------------------------------------------------------------
# E. the decoder-input formulation (engine._decoder_dx)
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ldT,kern", [(64, GT.SMALL), (640, GT.PP)])
def test_e_decoder_input_gradient(ldT, kern):
    from unimm_amd import lib
    S, chunk, H = 4, 1152, 256
    V = (S - 1) * chunk + 2303
    g = torch.Generator(device=DEV).manual_seed(950 + ldT)
    dlogT = torch.full((V + ROWPAD, ldT), float("nan"), dtype=BF16, device=DEV)
    w = torch.full((V + ROWPAD, H), float("nan"), dtype=BF16, device=DEV)
    t = torch.randn((V, ldT), generator=g, device=DEV)
    t[:, 0::61] *= 1e3
    t[:, 1::67] *= 1e-3
    dlogT[:V] = t.to(BF16)
    w[:V] = torch.randn((V, H), generator=g, device=DEV).to(BF16)
    ends = [(s + 1) * chunk for s in range(S - 1)] + [V]
    bounds = list(zip([0] + ends[:-1], ends))
    assert [e1 - e0 for e0, e1 in bounds] == [1152, 1152, 1152, 2303]
    runs = []
    for rep in range(2):
        ops = [Op(e1 - e0, ldT, H, seed=960 + s, dy=dlogT[e0:e1], x=w[e0:e1], values="given", db=None, overwrite=False,
                  dw=Dw(ldT, H, g, zero=True)) for s, (e0, e1) in enumerate(bounds)]
        plan = _launch(ops, shared=False)
        assert [L["kernel"] for L in plan] == [kern] and len(plan[0]["order"]) == S
        _check("E", ops, plan)
        runs.append([o.dw.view.contiguous().view(torch.int32) for o in ops])
    for a, b in zip(*runs):
        assert torch.equal(a, b), "two runs of the same grouped launch differ in bits"


# ----------------------------------------------------------------------------------------------------------------------
# F. refusals
# ----------------------------------------------------------------------------------------------------------------------
def _raw(ops, mutate=None, count=None, ws=None, ws_bytes=0):
    """The C entry point on a hand-built argument array -> return code"""
    from unimm_amd import lib
    arr = (lib.GemmTnArgs * max(1, len(ops)))()
    for a, o in zip(arr, ops):
        a.dy, a.x, a.dw = o.dy.data_ptr(), o.x.data_ptr(), o.dw.view.data_ptr()
        a.dbias = o.db.view.data_ptr() if o.db is not None else None
        a.M, a.N, a.K, a.lddy, a.ldx, a.lddw = o.M, o.N, o.K, o.dy.stride(0), o.x.stride(0), o.dw.view.stride(0)
        a.m_dev, a.overwrite = None, 0
    if mutate is not None:
        mutate(arr)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return lib.lib().unimm_gemm_tn_grouped_ws(C.addressof(arr) if count != "null" else None, len(ops) if count is None or count == "null" else count,
                                              0, ws, ws_bytes, stream)


def _refused(ops, call, rc_want=None):
    """`call` must be refused (an error return / UnimmHipError) without a launch and with every output bit-unchanged."""
    from unimm_amd import lib
    lib.prof_enable(2)
    try:
        if rc_want is None:
            with pytest.raises(lib.UnimmHipError):
                call()
        else:
            assert call() == rc_want
        torch.cuda.synchronize()
        assert lib.prof_collect() == {}, "a refused call launched a kernel"
    finally:
        lib.prof_enable(0)
    for o in ops:
        assert o.dw.untouched() and (o.db is None or o.db.untouched())


def test_f_refusals():
    from unimm_amd import lib
    E_ARG, E_SHAPE, E_ALIGN = -1, -2, -3
    o = Op(200, 72, 88, seed=990)
    ops = [o]
    assert _raw(ops, count="null") == E_ARG                                          # NULL argument array
    for field in ("dy", "x", "dw"):
        _refused(ops, lambda f=field: _raw(ops, lambda arr: setattr(arr[0], f, None)), E_ARG)
    _refused(ops, lambda: _raw(ops, count=0), E_ARG)
    _refused(ops, lambda: _raw(ops, count=-1), E_ARG)
    for field in ("M", "N", "K"):
        for v in (0, -5):
            _refused(ops, lambda f=field, v=v: _raw(ops, lambda arr: setattr(arr[0], f, v)), E_SHAPE)
            kw = {field: v}
            _refused(ops, lambda kw=kw: lib.gemm_tn(o.dy, o.x, o.dw.view, **{**dict(M=o.M, N=o.N, K=o.K), **kw}))
    # leading dimensions: not a multiple of 8 / smaller than the extent / lddw < K
    wide = torch.zeros((200, 100), dtype=BF16, device=DEV)
    _refused(ops, lambda: lib.gemm_tn_grouped([(wide[:, :72], o.x, o.dw.view, 200, 72, 88, None)]))           # lddy = 100
    _refused(ops, lambda: lib.gemm_tn_grouped([(o.dy, wide[:, :88], o.dw.view, 200, 72, 88, None)]))          # ldx = 100
    _refused(ops, lambda: lib.gemm_tn_grouped([(o.dy, o.x, o.dw.view, 200, o.dy.stride(0) + 8, 88, None)]))   # lddy < N
    _refused(ops, lambda: lib.gemm_tn_grouped([(o.dy, o.x, o.dw.view, 200, 72, o.x.stride(0) + 8, None)]))    # ldx < K (and lddw < K)
    narrow = torch.zeros((72, 80), device=DEV)
    _refused(ops, lambda: lib.gemm_tn_grouped([(o.dy, o.x, narrow, 200, 72, 88, o.db.view)]))                 # lddw = 80 < K = 88
    assert int(narrow.count_nonzero()) == 0
    # a view at a column offset that is not a multiple of 8 (4 columns = 8 bytes)
    wide8 = torch.zeros((200, 104), dtype=BF16, device=DEV)
    _refused(ops, lambda: lib.gemm_tn_grouped([(wide8[:, 4:76], o.x, o.dw.view, 200, 72, 88, None)]))
    _refused(ops, lambda: lib.gemm_tn_grouped([(o.dy, wide8[:, 4:92], o.dw.view, 200, 72, 88, None)]))
    # a workspace that is not 256-byte aligned
    buf = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    _refused(ops, lambda: lib.gemm_tn_grouped([o.args()], ws=buf[8:]))
    assert _raw(ops, ws=buf.data_ptr(), ws_bytes=-1) == E_ARG
    # the call still works (the refusals left nothing behind)
    _run("F", ops)


def test_f_bad_problem_late_in_a_long_list():
    """A bad problem at index 60 of 97: nothing may have launched for the first 48."""
    from unimm_amd import lib
    ops = [_small_op(i, 97, 9900) for i in range(97)]
    args = [o.args() for o in ops]
    bad = list(args[60])
    bad[5] = ops[60].x.stride(0) + 8                       # K past ldx
    args[60] = tuple(bad)
    _refused(ops, lambda: lib.gemm_tn_grouped(args))
    _refused(ops, lambda: lib.gemm_tn_grouped(args, shared=1))


# ----------------------------------------------------------------------------------------------------------------------
# G. a split whose rows span 4 GiB of an operand
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def four_gib():
    """[1024 (+ 1), 256] bf16 at row stride 2^21 and column 8 of a 4 GiB + pad buffer: 1024 rows x 2^21 x 2 bytes = 2^32.  Only the
    view and a NaN band around it (8 columns on either side, one row below) are ever written."""
    ld, M, N = 1 << 21, 1024, 256
    buf = torch.empty(M * ld + 4096, dtype=BF16, device=DEV)
    buf.as_strided((M + 1, N + 16), (ld, 1), 0).fill_(float("nan"))
    yield buf.as_strided((M, N), (ld, 1), 8)
    del buf
    torch.cuda.empty_cache()


@pytest.mark.parametrize("M,wide,kern", [(1024, "dy", GT.LOCK_STEP), (1024, "x", GT.LOCK_STEP), (1023, "dy", GT.SMALL),
                                         (1023, "x", GT.SMALL)])
def test_g_rows_spanning_4gib(four_gib, M, wide, kern):
    """The unguarded ping-pong kernel would compute num_records = 1024 * 2^21 * 2 mod 2^32 = 0 for the wide operand, read it as
    zeros and leave dw at its prior.  M = 1023 is the control: the 128x128 kernel addresses with size_t."""
    four_gib.fill_(float("nan"))
    view = four_gib[:M]
    assert view.stride(0) * 2 * 1024 == 1 << 32
    op = Op(M, 256, 256, seed=1200 + M, dy=view if wide == "dy" else None, x=view if wide == "x" else None)
    plan, (rw, rb) = _run("G", [op])
    assert [L["kernel"] for L in plan] == [kern]
    assert not torch.equal(op.dw.view, op.dw.prior)
