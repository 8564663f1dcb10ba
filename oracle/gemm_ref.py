"""float64 restatement of ONE unimm_gemm_nt launch (include/unimm_hip.h), for the edge tests
(tests/test_gpu_gemm_edges.py): what the C ABI defines, so that a test does not re-derive it.

  * `launch`   -- the eight epilogues in float64 (torch, on the device the operands live on) together with the per-element
                  error budget of section "gate" below (`budget_acc`, `half_ulp_bf16` and the constants are its pieces);
  * `tile_dims`, `splits`, `ws_bytes` -- the host rules of the launcher (unimm_amd/csrc/gemm_nt.h: launch_nt_cfg) that
                  decide whether a launch splits K and how much workspace it needs;
  * `fast_erf64` -- the kernels' erf polynomial (Abramowitz-Stegun 7.1.26) in float64, for the CPU test that measures it.

Gate.  For output element (m, n) with float64 reference ref:  |got - ref| <= E[m, n],  E = the sum of

  accumulation   min(C_ACC, K) * 2^-24 * S,  S = sum_k |x[m,k]| |w[n,k]|.  A bf16 x bf16 product has 16 significant bits
                 and is exact in fp32, so only the additions round.  Any order of K - 1 correctly rounded fp32 additions
                 of terms whose magnitudes sum to S is within (K - 1) 2^-24 S (1 + O(2^-24)) of the exact sum, hence the
                 cap at K.  C_ACC is 8 x the worst ratio |fp32 matmul - fp64| / (2^-24 S) MEASURED on a reference
                 implementation (torch's CPU float32 matmul on bf16-valued operands, K in {64 .. 9216}:
                 tests/test_gemm_ref_cpu.py: worst 2.2 - 2.7 depending on the sample, so 18 - 22), rounded up to a power of two: 32.  The factor 8 is for
                 what that measurement does not cover: the matrix instruction's internal order and rounding over its 32
                 products, and the reassociation of a 3- or 4-way split of K.
  epilogue       8 * 2^-24 * T,  T = the sum of the magnitudes of the terms the epilogue combines in fp32 (accumulator
                 times dropout scale, bias, residual or the LayerNorm pieces, the multiplier product, the activation's
                 own products): a handful of fp32 operations, each within 2^-24 of its result.
  activation     the kernels evaluate erf by A&S 7.1.26 with a 1-ulp reciprocal and the hardware exp.  ERF_ABS is 4 x the
                 polynomial's measured distance from math.erf in float64 (tests/test_gemm_ref_cpu.py: 1.5e-7 as published;
                 the factor 4 is for the fp32 evaluation).  GELU(u) = u (1 + erf(u / sqrt 2)) / 2 sees it times |u| / 2;
                 GELU'(u) = Phi(u) + u phi(u) sees it times 1/2 + |u| phi(u) (the exp is shared by the erf tail and the
                 pdf).  The budget of the pre-activation propagates times max |GELU'| = 1.13 and max |GELU''| = 0.80
                 (phi(0) * 2).  Absolute: GELU's far negative tail is smaller than any relative bound.
  output         a bf16 output (round to nearest even): half an ulp of a value of magnitude v = |ref| + everything above,
                 i.e. 2^(floor(log2 v) - 8): bf16 has 8 significant bits, an ulp in [2^e, 2^(e+1)) is 2^(e-7).  Relative to
                 v that is between 2^-9 (just below a power of two) and 2^-8 (at one); the flat 2^-9 v is NOT a bound of a
                 correctly rounded conversion (1 + 2^-8 - eps rounds to 1: relative error 2^-8), and every bf16 kernel
                 measures 1.98-1.99 against it (`lit` in launch()'s result keeps that figure available).  Nothing for
                 fp32.  The second output likewise.

A dropped element (keep bit 0) has no accumulation term: it must equal the residual term within the epilogue budget.
A keep bit that differs from the host mirror is an O(1) error and fails by itself."""
from __future__ import annotations

import math

import torch

EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_DROP_RESID, EPI_BIAS_RELU, EPI_DGELU, EPI_ADD, EPI_MUL, EPI_BIAS_GELU_DG = range(8)
EPI_NAMES = ("BIAS", "BIAS_GELU", "BIAS_DROP_RESID", "BIAS_RELU", "DGELU", "ADD", "MUL", "BIAS_GELU_DG")
NEEDS_AUX = (EPI_BIAS_DROP_RESID, EPI_DGELU, EPI_ADD, EPI_MUL)

U32 = 2.0 ** -24          # unit roundoff of fp32
U16_FLAT = 2.0 ** -9      # the flat relative figure (see "output" above): reported, not gated on
C_ACC = 32.0              # see "accumulation" above
C_EPI = 8.0
ERF_POLY = 1.5e-7         # A&S 7.1.26, published bound; tests/test_gemm_ref_cpu.py measures it
ERF_ABS = 4.0 * ERF_POLY
GELU_D1_MAX = 1.13        # max |GELU'|  (1.1289 at u = sqrt 2)
GELU_D2_MAX = 0.80        # max |GELU''| (2 phi(0) = 0.7979 at u = 0)

# tile code -> (BM, BN, workgroups per CU, K loop).  "ring": the lock-step ring loop (splits K on request when it has 4
# waves); "ring8": the ring loop of the 8-wave tiles and "pp": the ping-pong loop, which never split.
_TILES = {
    1: (128, 128, 2, "ring"), 3: (256, 256, 1, "ring8"), 6: (192, 256, 1, "ring8"), 7: (64, 128, 3, "ring"),
    8: (256, 256, 1, "pp"), 9: (64, 128, 2, "ring"), 10: (128, 128, 1, "ring"), 12: (192, 256, 1, "ring8"),
    14: (128, 128, 2, "ring"), 15: (64, 128, 2, "ring"),
}
TILE_CODES = tuple(sorted(_TILES))
SPLIT_CODES = tuple(c for c in TILE_CODES if _TILES[c][3] == "ring")
SAME_K_ORDER = ((9, 7), (15, 7), (10, 1), (14, 1), (8, 3), (12, 6))      # bit-identical pairs
BK = 64
COUNTER_BYTES = 16384      # the first 16 KiB of a split-K workspace: one int32 ticket per output tile
WS_MIN_BYTES = 32768       # unimm_gemm_nt rejects a split request with a smaller workspace (UNIMM_E_ARG)


def tile_dims(code):
    """(BM, BN, workgroups per CU, loop) of tile code `code` (its last two digits; p and gn do not change the tile)."""
    return _TILES[code % 100]


def tiles(M, N, code):
    BM, BN = tile_dims(code)[:2]
    return -(-M // BM) * -(-N // BN)


def ws_bytes(M, N, code, nsplit):
    """Workspace a launch needs to split every tile `nsplit` ways: 16 KiB of counters + tiles x splits x tile bytes, a tile
    being BM x BN fp32 partial sums (64 x 128: 32 KiB)."""
    BM, BN = tile_dims(code)[:2]
    return COUNTER_BYTES + tiles(M, N, code) * nsplit * BM * BN * 4


def splits(M, N, K, code, want, ws, cus):
    """Number of K slices the launch really uses (1 = unsplit).  want: unimm_gemm_nt_args.splitk (0 / 1 off, 2..8 at most
    that many, -1 the library's choice); ws: bytes of workspace given; cus: compute units of the device.
    Rules: 4-wave ring tiles only; at most 4; at least 8 K steps of 64 per split; no empty split; at most 4096 tiles (one
    ticket each); the workspace must hold ws_bytes() of THAT split count, else the launch runs unsplit (not with fewer)."""
    BM, BN, wpc, loop = tile_dims(code)
    if loop != "ring" or want in (0, 1) or ws is None:
        return 1
    nwg, nk = tiles(M, N, code), K // BK
    slots = (cus & ~7) * wpc
    ks = want if want > 1 else (slots // nwg if nwg > 0 else 1)
    ks = min(ks, 4)
    while ks > 1 and nk // ks < 8:
        ks -= 1
    if ks > 1:
        per = -(-nk // ks)
        while ks > 1 and (ks - 1) * per >= nk:
            ks -= 1
    if ks > 1 and nwg <= COUNTER_BYTES // 4 and ws_bytes(M, N, code, ks) <= ws:
        return ks
    return 1


def split_ranges(K, nsplit):
    """K-step ranges [(first, count)] of the slices (the kernel: per = ceil(steps / splits), the last slice is shorter)."""
    nk = K // BK
    per = -(-nk // nsplit)
    return [(s * per, min(per, nk - s * per)) for s in range(nsplit)]


def phi(u):
    return torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)


def cdf(u):
    return 0.5 * (1.0 + torch.erf(u / math.sqrt(2.0)))


def gelu(u):
    return u * cdf(u)


def gelu_grad(u):
    return cdf(u) + u * phi(u)


def fast_erf64(x):
    """The kernels' erf (csrc/common.h: fast_erf) evaluated in float64: Abramowitz-Stegun 7.1.26."""
    ax = x.abs()
    t = 1.0 / (1.0 + 0.3275911 * ax)
    p = 1.061405429 * t - 1.453152027
    p = p * t + 1.421413741
    p = p * t - 0.284496736
    p = p * t + 0.254829592
    return torch.copysign(1.0 - p * t * torch.exp(-ax * ax), x)


def layernorm_resid(aux, aux_ln, N):
    """(aux - mean) * rstd * gamma + beta in float64, and the sum of the magnitudes of its pieces."""
    mean, rstd, gamma, beta = (t.double() for t in aux_ln)
    a = aux[:, :N].double()
    sc = rstd[:, None] * gamma[None, :N]
    val = (a - mean[:, None]) * sc + beta[None, :N]
    mag = (a.abs() + mean.abs()[:, None]) * sc.abs() + beta.abs()[None, :N]
    return val, mag


def keep_bits(drop, salt, M, N, device):
    """Keep mask [M, N] (bool, on `device`) of a dropout triple (key, thr, scale) with an optional salt WORD (int): the
    host mirror of drop_word with key ^ salt."""
    from unimm_amd import dropout as DR
    key = (int(drop[0]) ^ (int(salt) if salt is not None else 0)) & 0xFFFFFFFF
    return torch.from_numpy(DR.keep_mask2d(key, int(drop[1]), M, N)).to(device)


def budget_acc(S, K):
    return min(C_ACC, float(K)) * U32 * S


def half_ulp_bf16(v):
    """Half an ulp of bf16 at magnitude v >= 0 (float64 tensor): 2^(floor(log2 v) - 8); 0 at v = 0."""
    _, ex = torch.frexp(v)                                   # v = m 2^ex, m in [0.5, 1): floor(log2 v) = ex - 1
    return torch.where(v > 0, torch.exp2((ex - 9).double()), torch.zeros_like(v))


def _round_out(ref, E, out_bf16):
    return E + half_ulp_bf16(ref.abs() + E) if out_bf16 else E


def launch(x, w, bias, aux, epilogue, drop=None, aux_ln=None, N=None, salt=None, out_bf16=False, out2_bf16=True):
    """One launch in float64.  x [M, K], w [>= N, K] bf16 (views allowed), bias [>= N] fp32 or None, aux the epilogue
    operand ([M, >= N]: fp32 for BIAS_DROP_RESID, bf16 otherwise) or None, drop = (key, thr, scale) or None,
    aux_ln = (mean[M], rstd[M], gamma[N], beta[N]) or None, salt = the VALUE of the device salt word or None.
    -> dict(ref, ref2, E, E2, keep, lit, lit2): float64 [M, N] (ref2 / E2 / lit2 None without a second output; keep None
    without dropout).  E / E2 include the output rounding of a bf16 output when out_bf16 / out2_bf16; lit / lit2 are the
    same budgets with the flat 2^-9 (|ref| + ...) in its place (a figure to report)."""
    M, K = x.shape
    N = w.shape[0] if N is None else N
    xd, wd = x.double(), w[:N].double()
    acc = xd @ wd.t()
    S = xd.abs() @ wd.abs().t()
    e_acc = budget_acc(S, K)
    del S
    b = bias[:N].double()[None, :] if bias is not None else torch.zeros((1, N), dtype=torch.float64, device=x.device)
    pre = acc + b
    t_pre = acc.abs() + b.abs()
    e_pre = e_acc + C_EPI * U32 * t_pre
    ref2 = E2 = keep = None
    if epilogue == EPI_BIAS:
        ref, E = pre, e_pre
    elif epilogue == EPI_BIAS_RELU:
        ref, E = torch.relu(pre), e_pre
    elif epilogue in (EPI_BIAS_GELU, EPI_BIAS_GELU_DG):
        ref = gelu(pre)
        E = GELU_D1_MAX * e_pre + ERF_ABS * pre.abs() / 2 + C_EPI * U32 * (pre.abs() + ref.abs())
        if epilogue == EPI_BIAS_GELU:
            ref2, E2 = pre, e_pre
        else:
            ref2 = gelu_grad(pre)
            upd = pre.abs() * phi(pre)
            E2 = GELU_D2_MAX * e_pre + ERF_ABS * (0.5 + upd) + C_EPI * U32 * (cdf(pre) + upd)
    elif epilogue == EPI_DGELU:
        a = aux[:, :N].double()
        g = gelu_grad(a)
        upd = a.abs() * phi(a)
        ref = pre * g
        E = g.abs() * e_pre + pre.abs() * (ERF_ABS * (0.5 + upd) + C_EPI * U32 * (cdf(a) + upd)) + C_EPI * U32 * ref.abs()
    elif epilogue == EPI_ADD:
        a = aux[:, :N].double()
        ref, E = pre + a, e_pre + C_EPI * U32 * a.abs()
    elif epilogue == EPI_MUL:
        a = aux[:, :N].double()
        ref = pre * a
        E = a.abs() * e_pre + C_EPI * U32 * ref.abs()
    elif epilogue == EPI_BIAS_DROP_RESID:
        if aux_ln is not None:
            resid, t_res = layernorm_resid(aux, aux_ln, N)
        else:
            resid = aux[:, :N].double()
            t_res = resid.abs()
        if drop is not None and int(drop[1]) != 0:
            keep = keep_bits(drop, salt, M, N, x.device)
            scale = float(torch.tensor(float(drop[2]), dtype=torch.float32))      # the kernel multiplies by the fp32 argument
            kd = keep.double() * scale
            ref = pre * kd + resid
            E = kd * e_acc + C_EPI * U32 * (kd * t_pre + t_res)
        else:
            ref, E = pre + resid, e_pre + C_EPI * U32 * t_res
    else:
        raise ValueError(epilogue)
    lit = E + U16_FLAT * (ref.abs() + E) if out_bf16 else E
    lit2 = None
    E = _round_out(ref, E, out_bf16)
    if ref2 is not None:
        lit2 = E2 + U16_FLAT * (ref2.abs() + E2) if out2_bf16 else E2
        E2 = _round_out(ref2, E2, out2_bf16)
    return dict(ref=ref, ref2=ref2, E=E, E2=E2, keep=keep, lit=lit, lit2=lit2)


def worst_ratio(got, ref, E):
    """max over ALL elements of |got - ref| / E (inf where got is not finite or E is 0 with a nonzero error)."""
    err = (got.double() - ref).abs()
    r = torch.where(E > 0, err / torch.where(E > 0, E, torch.ones_like(E)), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    r = torch.where(torch.isfinite(got.double()), r, torch.full_like(r, math.inf))
    return float(r.max()) if r.numel() else 0.0
