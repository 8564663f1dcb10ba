"""`unimm_linear_f32` and `unimm_rows_add_f32` (csrc/heads.hip: the exact-fp32 MFMA kernel under both poolers and the NSP
head, forward and backward) per element against an fp64 matmul of the same fp32 inputs, through the C ABI.

Each case is named after the path it must reach.  The kernel takes one 16x16 output tile per workgroup, splits the
reduction over its four waves in whole 16-deep chunks (wave w starts at k = w * 16 * ceil(ceil(K / 16) / 4)), and has
  * a 16-byte path (both operands reduction-contiguous, K % 16 == 0, row strides % 4 == 0, 16-byte aligned bases) with a
    64-deep main loop and a 16-deep tail loop, and
  * a strided scalar path, 32 deep with a guard on k, for everything else.
Every (M, N, K) runs in the three production forms of the engine:
    fwd  y = relu(x W^T + b)        A = x  [M, K] rows,      B = W [N, K] rows       (reduction K, contiguous on both)
    dx   dx = dy W                  A = dy [M, N] rows,      B = W [N, K] columns    (reduction N, sb_k != 1)
    dW   dW += dy^T x, db += colsum(dy)   A = dy columns, B = x [M, K] columns       (reduction M, sa_k != 1; rowsum)

Gate, per element and derived, with u = 2^-24:
    |got - ref| <= (K / 4 + 4) u sum_k |a(m,k) b(k,n)| + u |ref|  (+ u |prior| under `accumulate`)
K / 4 + 4 is the depth of one wave's fma chain plus the three cross-wave adds and the bias add; sum |a||b| is |A| @ |B| in
fp64.  `rowsum` gets the same rule with depth K.  A dropped or doubled product is about sum|ab| / K, more than 50 times
over this gate at every K of the table.

Probes: the product at the last valid k and at the first k of each wave's share is about 100 times the typical term; every
operand element the kernel must not use is NaN (columns [K, stride) of a row-strided operand, two rows past the last one of
the same allocation, the element before a misaligned view); outputs start as a NaN bit pattern with three sentinel columns
(ldo = N + 3) and two sentinel rows, which must come back bit-unchanged.

`unimm_rows_add_f32` is bit-exact bf16(float(dst) + src) on the listed rows, every other row bit-unchanged, below and
above the 2048 x 256-element grid of one pass (683 rows of 768).

Measured on an MI355X (printed per launch): the largest linear error is 0.65 of its derived bound, at reduction lengths
15 to 17 where the bound allows about four roundings; 0.13 to 0.45 at K >= 240; the largest rowsum error is 0.34 of its
bound; rows_add is bit-exact at every size."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN16, NAN32 = 0x7FA5, 0x7FA5A5A5
U = 2.0 ** -24
LOUD = 10.0                                  # on both operands: the product is 100 times the typical term


def loud_ks(R):
    per = ((R + 15) // 16 + 3) // 4          # ceil(ceil(R / 16) / 4) chunks per wave
    return sorted({R - 1} | {w * 16 * per for w in range(4) if w * 16 * per < R})


class Operand:
    """logical [outer, R] fp32 matrix in a NaN-filled allocation.  layout "r": rows of R (+ pad NaN columns), two NaN
    rows after the last; layout "o": stored transposed, R rows of `outer` (+ pad) elements.  `off` leading elements
    shift the view off its alignment."""

    def __init__(self, logical, layout, pad, off):
        outer, R = logical.shape
        stored = logical if layout == "r" else logical.T
        rows, cols = stored.shape
        ld = cols + pad
        host = np.full(off + (rows + 2) * ld, np.nan, np.float32)
        host[off:].reshape(rows + 2, ld)[:rows, :cols] = stored
        self.buf = torch.from_numpy(host).to(DEV)
        self.view = self.buf[off:]
        self.s_outer, self.s_r = (ld, 1) if layout == "r" else (1, ld)
        self.ld = ld


FORMS = {"fwd": ("r", "r"), "dx": ("r", "o"), "dW": ("o", "o")}


def run_linear(name, form, Mo, No, R, seed, bias=False, relu=False, accumulate=False, rowsum=False,
               pad=(4, 4), off=(0, 0)):
    """one launch: OUT[Mo, No] (+)= act(A[Mo, R] B[R, No] + bias); returns (worst error / gate, the same for rowsum)"""
    from unimm_amd import lib
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((Mo, R)).astype(np.float32)
    Bt = (0.05 * rng.standard_normal((No, R))).astype(np.float32)
    ks = loud_ks(R)
    A[:, ks] *= LOUD
    Bt[:, ks] *= LOUD
    b = (0.1 * rng.standard_normal(No)).astype(np.float32) if bias else None
    prior = rng.standard_normal((Mo, No)).astype(np.float32) if accumulate else None
    rs_prior = rng.standard_normal(Mo).astype(np.float32) if rowsum else None
    la, lb = FORMS[form]
    a_op, b_op = Operand(A, la, pad[0], off[0]), Operand(Bt, lb, pad[1], off[1])
    ldo = No + 3
    obuf = torch.full((Mo + 2, ldo), NAN32, dtype=torch.int32, device=DEV).view(torch.float32)
    if accumulate:
        obuf[:Mo, :No] = torch.from_numpy(prior).to(DEV)
    rsbuf = None
    if rowsum:
        rsbuf = torch.full((Mo + 8,), NAN32, dtype=torch.int32, device=DEV).view(torch.float32)
        rsbuf[:Mo] = torch.from_numpy(rs_prior).to(DEV)
    bias_d = None
    if bias:
        bias_d = torch.full((No + 2,), float("nan"), device=DEV)
        bias_d[:No] = torch.from_numpy(b).to(DEV)
    lib.linear_f32(a_op.view, b_op.view, obuf, Mo, No, R, (a_op.s_outer, a_op.s_r), (b_op.s_r, b_op.s_outer),
                   bias=bias_d, relu=relu, accumulate=accumulate, rowsum=rsbuf)
    torch.cuda.synchronize()
    A64, B64 = A.astype(np.float64), Bt.astype(np.float64).T
    ref = A64 @ B64
    if bias:
        ref = ref + b.astype(np.float64)
    if relu:
        ref = np.maximum(ref, 0.0)
    gate = (R / 4 + 4) * U * (np.abs(A64) @ np.abs(B64))
    if accumulate:
        ref = ref + prior.astype(np.float64)
        gate = gate + U * np.abs(prior)
    gate = gate + U * np.abs(ref)
    bits = obuf.view(torch.int32).cpu().numpy()
    got = bits[:Mo, :No].view(np.float32).astype(np.float64)
    assert (bits[Mo:, :] == NAN32).all(), f"{name}: rows past M written"
    assert (bits[:Mo, No:] == NAN32).all(), f"{name}: sentinel columns written"
    assert np.isfinite(got).all(), f"{name}: non-finite output (an operand element outside the matrices was used)"
    frac = float(((np.abs(got - ref)) / gate).max())
    rs_frac = 0.0
    if rowsum:
        rbits = rsbuf.view(torch.int32).cpu().numpy()
        assert (rbits[Mo:] == NAN32).all(), f"{name}: rowsum written past M"
        rs_got = rbits[:Mo].view(np.float32).astype(np.float64)
        rs_ref = rs_prior.astype(np.float64) + A64.sum(1)
        rs_gate = R * U * np.abs(A64).sum(1) + U * np.abs(rs_ref) + U * np.abs(rs_prior)
        assert np.isfinite(rs_got).all()
        rs_frac = float((np.abs(rs_got - rs_ref) / rs_gate).max())
    print(f"\n{name} [{form}] out {Mo}x{No} reduction {R} loud k {ks}: max |err| / gate {frac:.3f}"
          + (f"  rowsum {rs_frac:.3f}" if rowsum else ""))
    assert frac <= 1.0, f"{name} [{form}]: {frac:.3f} of the gate"
    assert rs_frac <= 1.0, f"{name} [{form}]: rowsum {rs_frac:.3f} of the gate"
    return frac, rs_frac


def three_forms(name, M, N, K, seed, **kw):
    run_linear(name, "fwd", M, N, K, seed, bias=True, relu=True, **kw)
    run_linear(name, "fwd", M, N, K, seed, bias=True, **kw)           # the same without relu: a clipped output hides its sum
    run_linear(name, "dx", M, K, N, seed + 1, **kw)
    run_linear(name, "dW", N, K, M, seed + 2, accumulate=True, rowsum=True, **kw)


VEC = [(1, 1, 16, "one wave works, tail only"), (17, 2, 48, "three waves, tail only"), (16, 16, 64, "one chunk per wave"),
       (33, 17, 80, "two waves with two chunks, one with one"), (15, 50, 272, "main loop plus tail"),
       (6, 2, 1024, "main loop only, dx / dW reductions 2 and 6"), (17, 33, 1040, "main loop plus tail, 65 chunks"),
       (240, 1024, 768, "production")]


@pytest.mark.parametrize("M,N,K,what", VEC, ids=[f"16-byte path M={m} N={n} K={k}: {w}" for m, n, k, w in VEC])
def test_linear_f32_16_byte_path(M, N, K, what):
    three_forms(f"16-byte path ({what})", M, N, K, seed=M + N + K)


RAGGED = [(1, 1, 1), (15, 16, 15), (16, 17, 17), (17, 15, 31), (15, 17, 33), (17, 16, 63), (16, 15, 65), (17, 17, 100)]


@pytest.mark.parametrize("M,N,K", RAGGED, ids=[f"strided path, K % 16 != 0: M={m} N={n} K={k}" for m, n, k in RAGGED])
def test_linear_f32_strided_path_ragged_k(M, N, K):
    three_forms("strided path (K % 16 != 0)", M, N, K, seed=7 * K + M)


@pytest.mark.parametrize("what,pad,off", [("row stride K + 1", (1, 4), (0, 0)), ("W row stride K + 1", (4, 1), (0, 0)),
                                          ("x base 4 bytes off", (4, 4), (1, 0)), ("W base 4 bytes off", (4, 4), (0, 1))])
def test_linear_f32_strided_path_by_stride_and_alignment(what, pad, off):
    """K % 16 == 0 and reduction-contiguous operands: only the named condition keeps the call off the 16-byte path"""
    for M, N, K in ((17, 33, 80), (6, 18, 272)):
        run_linear(f"strided path ({what})", "fwd", M, N, K, seed=K + pad[0] + off[1], bias=True, relu=True, pad=pad, off=off)


STRIDED = [(2, 6, 32), (37, 240, 16), (257, 37, 20), (240, 257, 48)]


@pytest.mark.parametrize("M,N,K", STRIDED, ids=[f"sa_k != 1: dx reduction {n}, dW reduction {m} (K={k})" for m, n, k in STRIDED])
def test_linear_f32_strided_reductions(M, N, K):
    """the dx and dW forms at reduction lengths 2, 6, 37, 240, 257 (257 and 37 give an odd chunk count per wave)"""
    three_forms("strided path (sa_k / sb_k != 1)", M, N, K, seed=M + 3 * N)


def test_linear_f32_epilogue():
    # bias = None, relu off, on both paths
    for K in (64, 33):
        run_linear("epilogue: no bias, no relu", "fwd", 17, 18, K, seed=K)
        run_linear("epilogue: bias, no relu", "fwd", 17, 18, K, seed=K + 1, bias=True)
        run_linear("epilogue: relu, no bias", "fwd", 17, 18, K, seed=K + 2, relu=True)
    # accumulate on the forward form (atomic add onto non-zero prior content), with bias
    run_linear("epilogue: accumulate onto a prior", "fwd", 33, 17, 80, seed=3, bias=True, accumulate=True)
    # rowsum with the output spanning four column tiles: added once, onto a non-zero prior value
    run_linear("epilogue: rowsum once over 4 column tiles", "dW", 18, 50, 37, seed=4, accumulate=True, rowsum=True)
    run_linear("epilogue: rowsum, 16-byte path, 3 column tiles", "fwd", 18, 40, 80, seed=5, accumulate=True, rowsum=True)
    # rowsum with accumulate = False: the output is stored, the row sums still add onto their prior
    run_linear("epilogue: rowsum without accumulate", "dW", 18, 50, 37, seed=6, rowsum=True)
    run_linear("epilogue: rowsum without accumulate, 16-byte path", "fwd", 5, 33, 64, seed=7, rowsum=True)


def test_linear_f32_refusals():
    from unimm_amd import lib
    x = torch.randn((16, 32), device=DEV)
    w = torch.randn((16, 32), device=DEV)
    out = torch.full((16, 20), NAN32, dtype=torch.int32, device=DEV).view(torch.float32)
    narrow = torch.full((16 * 16 + 16,), NAN32, dtype=torch.int32, device=DEV).view(torch.float32)
    with pytest.raises(lib.UnimmHipError, match="UNIMM_E_ALIGN"):
        lib.linear_f32(x, w, narrow[:16 * 15].view(16, 15), 16, 16, 32, (32, 1), (1, 32))      # ldo = 15 < N = 16
    for M, N, K in ((0, 16, 32), (16, 0, 32), (16, 16, 0)):
        with pytest.raises(lib.UnimmHipError, match="UNIMM_E_SHAPE"):
            lib.linear_f32(x, w, out, M, N, K, (32, 1), (1, 32))
    torch.cuda.synchronize()
    assert (out.view(torch.int32) == NAN32).all() and (narrow.view(torch.int32) == NAN32).all()


ROWS = [(1, 8, "one row"), (3, 1024, "three rows"), (682, 768, "last size of a single pass"),
        (683, 768, "first grid-stride size"), (1400, 768, "third pass, ragged")]


@pytest.mark.parametrize("n,H,what", ROWS, ids=[f"rows_add n={n} H={h}: {w}" for n, h, w in ROWS])
def test_rows_add_f32_bit_exact(n, H, what):
    from unimm_amd import lib
    rng = np.random.default_rng(n + H)
    rows = 2 * n + 3
    # a permutation sample without repeats that includes row 0 and the last row (n = 1: the last row alone)
    inner = 1 + rng.permutation(rows - 2)[:max(n - 2, 0)]
    idx = rng.permutation(np.concatenate([[0][:n - 1], inner, [rows - 1]])).astype(np.int32)
    assert len(idx) == n and len(set(idx.tolist())) == n and rows - 1 in idx and (n == 1 or 0 in idx)
    g = torch.Generator().manual_seed(n)
    dst_h = torch.randn((rows, H), generator=g).to(torch.bfloat16)
    src_h = torch.randn((n, H), generator=g)
    buf = torch.full((rows * H + 64,), NAN16, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    buf[:rows * H] = dst_h.reshape(-1).to(DEV)
    lib.rows_add_f32(buf, torch.from_numpy(idx).to(DEV), src_h.to(DEV), n, H)
    torch.cuda.synchronize()
    want = dst_h.clone()
    want[torch.from_numpy(idx).long()] = (dst_h.float()[torch.from_numpy(idx).long()] + src_h).to(torch.bfloat16)
    bits = buf.view(torch.int16).cpu()
    assert (bits[rows * H:] == NAN16).all(), "written past the last row"
    got = bits[:rows * H].view(rows, H)
    wrong = (got != want.view(torch.int16)).any(1)
    touched = torch.zeros(rows, dtype=torch.bool)
    touched[torch.from_numpy(idx).long()] = True
    print(f"\nrows_add n={n} H={H} ({what}): rows wrong {int(wrong.sum())} (listed {int((wrong & touched).sum())},"
          f" unlisted {int((wrong & ~touched).sum())})")
    assert not wrong.any()
