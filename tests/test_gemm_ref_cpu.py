"""oracle/gemm_ref.py checked on the CPU: the float64 epilogues against autograd and against their materialised forms, the
host rules of split-K against cases worked by hand from the text of include/unimm_hip.h, and the two MEASUREMENTS the
gates of tests/test_gpu_gemm_edges.py rest on (printed: run with -s to see them):

  * the worst |fp32 matmul - fp64| / (2^-24 S) of a reference fp32 matmul (torch on the CPU) on bf16-valued operands,
    per K -- C_ACC is 8 x that, rounded up to a power of two;
  * the distance of the kernels' erf polynomial (Abramowitz-Stegun 7.1.26), evaluated in float64, from math.erf --
    ERF_ABS is 4 x that."""
import math

import numpy as np
import torch

from oracle import gemm_ref as GR


def _bf(shape, gen, scale=1.0):
    return (torch.randn(shape, generator=gen) * scale).to(torch.bfloat16)


def test_fp32_matmul_error_ratio_sets_c_acc():
    g = torch.Generator().manual_seed(1)
    worst = {}
    for K in (64, 192, 768, 2304, 3072, 9216):
        x, w = _bf((160, K), g), _bf((192, K), g, 0.05)
        x[:8] *= 1e3                       # loud and quiet rows: the ratio is per element, so scale must not matter
        x[8:16] *= 1e-3
        got = x.float() @ w.float().t()
        ref = x.double() @ w.double().t()
        S = x.double().abs() @ w.double().abs().t()
        worst[K] = float(((got.double() - ref).abs() / (GR.U32 * S)).max())
    print("\nfp32 matmul |err| / (2^-24 S) per K: " + "  ".join(f"{k}: {v:.2f}" for k, v in worst.items()))
    m = max(worst.values())
    print(f"worst {m:.2f} -> 8 x = {8 * m:.1f}, C_ACC = {GR.C_ACC:g}")
    assert 8 * m <= GR.C_ACC
    assert GR.C_ACC == 2 ** math.ceil(math.log2(GR.C_ACC))           # a power of two
    assert all(v <= K for K, v in worst.items())                     # the order-free bound


def test_erf_polynomial_error_sets_erf_abs():
    x = torch.linspace(-8, 8, 1_600_001, dtype=torch.float64)
    d = float((GR.fast_erf64(x) - torch.erf(x)).abs().max())
    print(f"\nA&S 7.1.26 in float64: max |erf_poly - erf| = {d:.3e}; ERF_POLY = {GR.ERF_POLY:.1e}, ERF_ABS = {GR.ERF_ABS:.1e}")
    assert d <= GR.ERF_POLY
    assert d >= GR.ERF_POLY / 4            # the constant is the measured size, not a loose stand-in
    assert GR.ERF_ABS == 4 * GR.ERF_POLY
    assert abs(float(GR.fast_erf64(torch.tensor([0.3], dtype=torch.float64))) - math.erf(0.3)) <= GR.ERF_POLY


def test_gelu_constants():
    u = torch.linspace(-10, 10, 400_001, dtype=torch.float64, requires_grad=True)
    GR.gelu(u).sum().backward()
    assert float((u.grad - GR.gelu_grad(u.detach())).abs().max()) <= 1e-14
    d1 = u.grad.abs().max().item()
    ud = u.detach()
    d2 = (GR.phi(ud) * (2 - ud * ud)).abs().max().item()             # GELU'' = phi(u) (2 - u^2)
    assert 1.12 < d1 <= GR.GELU_D1_MAX and 0.79 < d2 <= GR.GELU_D2_MAX


def _case(M=24, N=20, K=64, seed=3):
    g = torch.Generator().manual_seed(seed)
    return _bf((M, K), g), _bf((N + 3, K), g, 0.1), torch.randn(N + 3, generator=g), g


def test_second_outputs_and_multipliers_against_autograd():
    x, w, bias, g = _case()
    N = 20
    aux = _bf((24, N + 4), g)
    acc = (x.double() @ w[:N].double().t())
    # BIAS_GELU_DG: out = GELU(u), out2 = dGELU/du
    u = (acc + bias[:N].double()).requires_grad_(True)
    GR.gelu(u).sum().backward()
    r = GR.launch(x, w, bias, None, GR.EPI_BIAS_GELU_DG, N=N)
    assert torch.allclose(r["ref"], GR.gelu(u.detach()), rtol=0, atol=1e-14) and torch.allclose(r["ref2"], u.grad, rtol=0, atol=1e-14)
    # BIAS_GELU: out2 = u
    r = GR.launch(x, w, bias, None, GR.EPI_BIAS_GELU, N=N)
    assert torch.equal(r["ref2"], u.detach())
    # DGELU: out = acc * GELU'(aux) is the gradient of sum(acc * GELU(aux)) with respect to aux
    a = aux[:, :N].double().requires_grad_(True)
    (acc * GR.gelu(a)).sum().backward()
    r = GR.launch(x, w, None, aux, GR.EPI_DGELU, N=N)
    assert torch.allclose(r["ref"], a.grad, rtol=0, atol=1e-13)
    # MUL with aux = the stored GELU'(u) equals DGELU with aux = u
    r2 = GR.launch(x, w, None, aux, GR.EPI_MUL, N=N)
    assert torch.equal(r2["ref"], acc * aux[:, :N].double())
    # ADD, RELU
    assert torch.equal(GR.launch(x, w, bias, aux, GR.EPI_ADD, N=N)["ref"], acc + bias[:N].double() + aux[:, :N].double())
    assert torch.equal(GR.launch(x, w, bias, None, GR.EPI_BIAS_RELU, N=N)["ref"], torch.relu(acc + bias[:N].double()))
    for e in (GR.EPI_BIAS, GR.EPI_BIAS_GELU, GR.EPI_BIAS_RELU, GR.EPI_BIAS_GELU_DG):
        r = GR.launch(x, w, bias, None, e, N=N, out_bf16=True)
        assert r["ref"].shape == (24, N) and bool((r["E"] > 0).all()) and r["ref"].dtype == torch.float64


def test_lazy_layernorm_equals_the_materialised_one_and_dropout_keys():
    from unimm_amd import dropout as DR
    x, w, bias, g = _case()
    M, N = 24, 20
    h = torch.randn((M, N + 4), generator=g) * 3 + 1
    gamma, beta = torch.randn(N, generator=g), torch.randn(N, generator=g)
    mean = h[:, :N].mean(1)
    rstd = torch.rsqrt(h[:, :N].var(1, unbiased=False) + 1e-12)
    y = (h[:, :N].double() - mean.double()[:, None]) * rstd.double()[:, None] * gamma.double() + beta.double()
    key, salt = DR.make_key(3, 9, 77), 0x9E3779B1
    drop = DR.drop_arg(0.25, key)
    lazy = GR.launch(x, w, bias, h, GR.EPI_BIAS_DROP_RESID, drop=drop, aux_ln=(mean, rstd, gamma, beta), N=N)
    mat = GR.launch(x, w, bias, y, GR.EPI_BIAS_DROP_RESID, drop=drop, N=N)
    assert torch.allclose(lazy["ref"], mat["ref"], rtol=0, atol=1e-13)
    assert bool((lazy["E"] >= mat["E"]).all())                      # the lazy form combines more (and larger) terms
    keep = lazy["keep"]
    assert 0.6 < float(keep.double().mean()) < 0.9
    # a dropped element is the residual alone, and its budget has no accumulation term
    dropped = ~keep
    assert torch.equal(mat["ref"][dropped], y[dropped])
    assert bool((mat["E"][dropped] == GR.C_EPI * GR.U32 * y.abs()[dropped]).all())
    # (key, salt) == (key ^ salt, no salt); a different salt is a different mask
    a = GR.launch(x, w, bias, y, GR.EPI_BIAS_DROP_RESID, drop=drop, N=N, salt=salt)
    b = GR.launch(x, w, bias, y, GR.EPI_BIAS_DROP_RESID, drop=DR.drop_arg(0.25, key ^ salt), N=N)
    assert torch.equal(a["keep"], b["keep"]) and torch.equal(a["ref"], b["ref"]) and not torch.equal(a["keep"], keep)
    assert np.array_equal(a["keep"].numpy(), DR.keep_mask2d(key ^ salt, drop[1], M, N))
    # no dropout: every element carries the accumulation term
    nod = GR.launch(x, w, bias, y, GR.EPI_BIAS_DROP_RESID, drop=(0, 0, 0.0), N=N)
    assert nod["keep"] is None and torch.equal(nod["ref"], x.double() @ w[:N].double().t() + bias[:N].double() + y)


def test_tile_and_split_rules_worked_by_hand():
    assert GR.TILE_CODES == (1, 3, 6, 7, 8, 9, 10, 12, 14, 15)
    assert GR.tile_dims(7)[:3] == (64, 128, 3) and GR.tile_dims(9)[:3] == (64, 128, 2) and GR.tile_dims(15)[:3] == (64, 128, 2)
    assert GR.tile_dims(1)[:3] == (128, 128, 2) and GR.tile_dims(10)[:3] == (128, 128, 1) and GR.tile_dims(14)[:3] == (128, 128, 2)
    assert GR.tile_dims(3)[:2] == GR.tile_dims(8)[:2] == (256, 256) and GR.tile_dims(6)[:2] == GR.tile_dims(12)[:2] == (192, 256)
    assert GR.tile_dims(3107) == GR.tile_dims(7) and GR.tile_dims(8)[3] == "pp"
    assert GR.SPLIT_CODES == (1, 7, 9, 10, 14, 15)
    # "16 KiB + tiles * splits * tile bytes (a 64 x 128 tile is 32 KiB)": 3900 x 768 is 61 x 6 = 366 tiles of 64 x 128
    assert GR.ws_bytes(3900, 768, 7, 2) == 16384 + 366 * 2 * 32768
    assert GR.ws_bytes(3900, 768, 1, 3) == 16384 + 31 * 6 * 3 * 65536
    big = 1 << 40
    # ">= 8 K-steps each", "<= 4"
    assert GR.splits(3900, 768, 512, 1, 2, big, 256) == 1            # 8 steps: 4 per split
    assert GR.splits(3900, 768, 1024, 1, 4, big, 256) == 2           # 16 steps: 4 -> 3 (5 each) -> 2 (8 each)
    assert GR.splits(3900, 768, 1024, 1, 2, big, 256) == 2
    assert GR.splits(3900, 768, 2304, 7, 4, big, 256) == 4           # 36 steps: 9 each
    assert GR.splits(3900, 768, 2368, 7, 4, big, 256) == 4           # 37 steps: 10, 10, 10, 7
    assert GR.split_ranges(2368, 4) == [(0, 10), (10, 10), (20, 10), (30, 7)]
    assert GR.split_ranges(2368, 3) == [(0, 13), (13, 13), (26, 11)]
    assert GR.splits(3900, 768, 3072, 1, 8, big, 256) == 4
    assert GR.splits(3900, 768, 3072, 1, 3, big, 256) == 3
    # -1: "as many as stay resident at once": 256 CUs x 2 workgroups of 128 x 128 against 186 tiles -> 2; 3 per CU of 64 x 128
    # against 366 tiles -> 2; 111 tiles of 64 x 128 (1110 x 768) -> 6, capped at 4; a full chip -> unsplit
    assert GR.splits(3900, 768, 3072, 1, -1, big, 256) == 2
    assert GR.splits(3900, 768, 3072, 7, -1, big, 256) == 2
    assert GR.splits(1110, 768, 3072, 7, -1, big, 256) == 4
    assert GR.splits(31162, 768, 3072, 1, -1, big, 256) == 1
    assert GR.splits(3900, 768, 3072, 10, -1, big, 256) == 1         # one 128 x 128 workgroup of the 3-slot ring per CU: 256 // 186
    # off, 8-wave tiles, workspace one byte short (unsplit, not fewer splits), no workspace
    assert GR.splits(3900, 768, 3072, 1, 0, big, 256) == GR.splits(3900, 768, 3072, 1, 1, big, 256) == 1
    for code in (3, 6, 8, 12):
        assert GR.splits(3900, 768, 3072, code, 4, big, 256) == 1
    need = GR.ws_bytes(3900, 768, 1, 4)
    assert GR.splits(3900, 768, 3072, 1, 4, need, 256) == 4 and GR.splits(3900, 768, 3072, 1, 4, need - 1, 256) == 1
    assert GR.splits(3900, 768, 3072, 1, 4, None, 256) == 1
    # more than 4096 tiles: one ticket word each in the 16 KiB of counters
    assert GR.tiles(8300, 3072, 7) == 130 * 24 and GR.splits(8300, 4096, 3072, 7, 2, big, 256) == 1


def test_worst_ratio_counts_every_element():
    ref = torch.zeros((3, 4), dtype=torch.float64)
    E = torch.full((3, 4), 1e-3, dtype=torch.float64)
    got = torch.zeros((3, 4))
    assert GR.worst_ratio(got, ref, E) == 0.0
    got[2, 3] = 2e-3
    assert abs(GR.worst_ratio(got, ref, E) - 2.0) < 1e-6
    got[0, 0] = float("nan")
    assert GR.worst_ratio(got, ref, E) == math.inf


def test_bf16_half_ulp_bounds_round_to_nearest_even():
    """Half an ulp of bf16 is 2^(e-8) on [2^e, 2^(e+1)): it bounds the conversion of every value, and the flat 2^-9 |v| does
    not (the worst relative error of a correctly rounded conversion is 2^-8, at the bottom of a binade)."""
    v = torch.cat([torch.linspace(0.9, 4.1, 200_001, dtype=torch.float64), torch.tensor([1.0, 2.0, 1.0 + 2.0 ** -8 - 1e-9, 3e-5, 770.0], dtype=torch.float64)])
    r = v.float().to(torch.bfloat16).double()
    err = (r - v.float().double()).abs()
    hu = GR.half_ulp_bf16(v)
    assert bool((err <= hu).all())
    assert float((err / hu).max()) > 0.999                                  # and it is attained
    flat = float((err / (GR.U16_FLAT * v)).max())
    print(f"\nbf16 round to nearest even: worst error / half ulp = {float((err / hu).max()):.4f}, / (2^-9 |v|) = {flat:.4f}")
    assert 1.9 < flat <= 2.0
    assert float(GR.half_ulp_bf16(torch.tensor([1.0], dtype=torch.float64))) == 2.0 ** -8
    assert float(GR.half_ulp_bf16(torch.tensor([1.99], dtype=torch.float64))) == 2.0 ** -8
    assert float(GR.half_ulp_bf16(torch.tensor([0.0], dtype=torch.float64))) == 0.0
