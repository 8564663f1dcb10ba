"""Every tile, epilogue, launch form and K split of unimm_gemm_nt against the float64 restatement of one launch
(oracle/gemm_ref.py), element by element.

Gate (oracle/gemm_ref.py has the derivations): |got - ref| <= E for EVERY element, E = accumulation (min(32, K) 2^-24
sum_k |x||w|) + epilogue arithmetic (8 x 2^-24 x the magnitudes combined) + activation (4 x the erf polynomial's error, scaled
by the formula) + the output's own rounding (bf16: half an ulp at the magnitude of the value, 2^(floor(log2 v) - 8); a flat
2^-9 v is not a bound of round-to-nearest -- every bf16 kernel measures 1.98-1.99 against it -- and is only reported).  Each test prints its worst |err| / E; the module prints a table per tile code and
per epilogue at the end (run with -s).

Poison.  x, w, aux, bias and the LayerNorm vectors are views into larger buffers whose rows past M / N and columns past K / N
hold NaN (allocated memory: an edge row that was read instead of masked turns an output into NaN, nothing is read out of
bounds).  out and out2 are views into buffers with 8 more rows and their pad columns, pre-filled with a NaN bit pattern that
must come back bit-unchanged outside [0, M) x [0, N); a NaN inside fails the gate.

Sections
  A  geometry x kernel: per tile code, M in {1, BM-1, BM, BM+1, 2BM+17}, N in {64, BN, 2BN} (every working wave on the FAST
     walk) and {1, 7, 63, 65, BN-1, BN+8, 2BN+36} (a wave straddles N: element-wise walk), K in {64, 128, 192, 448}; the 15
     (epilogue, output type) kernels rotated over them, out2 given and NULL for the GELU pair, 16-byte paths allowed and
     forbidden independently for out and aux, operands and outputs as column slices of wider buffers.
  B  launch forms x1xx / x2xx on a grid of several rounds with the heaviest epilogue state; tiles that accumulate in the same
     K order are bit-identical (9 = 15 = 7, 10 = 14 = 1, 8 = 3, 12 = 6) from 1 to 48 K steps; the measured accumulation ratio
     |err| / (2^-24 S) per tile code.
  C  tile order: gn in {1, 3, 7, 100} against the default on 5 tile columns.
  D  split-K on the six 4-wave ring tiles: requested splits x K (8 .. 48 steps, 37 included) x the small-batch epilogues, in a
     workspace of exactly ws_bytes() inside a sentinel-filled buffer; what the launch did (split or not) against
     oracle.gemm_ref.splits.  (This section found tile 10's split launches wrong in one element of 16: a store-data hazard
     in the slab publication, see nt_split_join in csrc/gemm_nt.h.)
  E  the dropout salt word.
  F  the shapes the engines issue (engine.py / engine_x3.py: _linear, _linear_bwd, _lin3, _lin3_bwd), automatic tile choice
     unless the engine names one, with inputs hostile to a global gate.  At 240 sequences: 31,162 text rows, 8,880 image rows,
     4,675 masked tokens.  (M, N, K, epilogue, output):
        text layer     (31162, 2304, 768, BIAS, bf16)  (31162, 768, 768, DROP_RESID + dropout + lazy LayerNorm, fp32)
                       (31162, 3072, 768, BIAS_GELU_DG, bf16 + out2)  (31162, 768, 3072, DROP_RESID + dropout, fp32)
        its backward   (31162, 3072, 768, MUL, bf16)  (31162, 768, 3072, ADD, bf16)  (31162, 768, 768, BIAS without bias, bf16)
                       (31162, 768, 2304, ADD, bf16)
        image layer    (8880, 3072, 1024, BIAS, bf16)  (8880, 1024, 1024, DROP_RESID + dropout, fp32)
                       (8880, 1024, 1024, BIAS_GELU_DG, bf16 + out2)  (8880, 1024, 1024, MUL, bf16)
        heads          (4675, 768, 768, BIAS_GELU, fp32 + bf16 out2)  (4675, 30522, 768, BIAS, fp32, ldo 30528)
                       (8880, 1024, 1024, BIAS_GELU, fp32 + bf16 out2)  (8880, 1601, 1024, BIAS, fp32, ldo 1604)
                       (4675, 768, 30528, BIAS without bias, bf16: the decoder's input gradient)
        three planes   (31162, 768, 2304, BIAS, fp32)  (3900, 768, 9216, DROP_RESID without dropout, fp32, tile 1, splitk 2)
                       (3900, 768, 2304, BIAS, fp32, tile 9)
     At the 30-sequence share (3,900 text rows, 1,110 image rows; engine._tile / _splitk):
                       (3900, 768, 3072, DROP_RESID + dropout, fp32, tile 1, splitk 2)  (3900, 768, 2304, ADD, bf16, tile 1, splitk 2)
                       (3900, 2304, 768, BIAS, bf16, tile 1)  (3900, 768, 768, DROP_RESID + lazy LayerNorm, fp32, tile 7)
                       (3900, 3072, 768, BIAS_GELU_DG, bf16 + out2, tile 1)
                       (1110, 1024, 1024, BIAS_GELU_DG, bf16 + out2, tile 14)  (1110, 3072, 1024, BIAS, bf16, tile 14)
  G  operands whose rows span 4 GiB: x as a [31162, 64] view of row stride 68,928 (the ping-pong loop's 32-bit offsets would
     wrap: the launcher must take the ring), and a w view of 30,522 rows of the same buffer (4.2 GB: the largest offset 32 bits
     still hold)."""
from collections import defaultdict

import pytest
import torch

from oracle import gemm_ref as GR

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN16, NAN32 = 0x7FA5, 0x7FA5A5A5
PAD = 8
BF16, F32 = torch.bfloat16, torch.float32

# the 15 (epilogue, fp32 output) kernels of a tile configuration
KERNELS = [(e, f) for e in range(8) for f in (False, True) if not (e == GR.EPI_BIAS_DROP_RESID and not f)]
assert len(KERNELS) == 15
GELUS = (GR.EPI_BIAS_GELU, GR.EPI_BIAS_GELU_DG)

STATS = defaultdict(float)        # (section, tile code or 0 = automatic, epilogue name, "f32" / "bf16") -> worst |err| / E
ACC_RATIO = defaultdict(float)    # tile code -> worst measured |err| / (2^-24 S) of a pure accumulation
COUNT = defaultdict(int)          # section -> gated launches
FLAT = defaultdict(float)         # (tile code, epilogue, output) -> worst |err| / E with a flat 2^-9 (|ref| + ...) as the bf16 term


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if not STATS:
        return
    print("\n\n==== unimm_gemm_nt edges: worst |err| / E ====")
    print("gated launches per section: " + "  ".join(f"{k}: {v}" for k, v in sorted(COUNT.items())) + f"  total {sum(COUNT.values())}")
    by_code, by_epi = defaultdict(float), defaultdict(float)
    for (sec, code, epi, ot), r in STATS.items():
        by_code[code] = max(by_code[code], r)
        by_epi[(epi, ot)] = max(by_epi[(epi, ot)], r)
    print("per tile code (0 = automatic): " + "  ".join(f"{c}: {r:.3f}" for c, r in sorted(by_code.items())))
    print("per epilogue: " + "  ".join(f"{e}/{o}: {r:.3f}" for (e, o), r in sorted(by_epi.items())))
    print("with the bf16 rounding term as a flat 2^-9 (|ref| + ...) instead of half an ulp (not a bound of round-to-nearest: "
          "reported, not gated): worst %.3f over the fp32-only kernels, %.3f over those with a bf16 output" % (
              max([0.0] + [r for (c, e, o), r in FLAT.items() if o == "f32" and e not in ("BIAS_GELU", "BIAS_GELU_DG")]),
              max([0.0] + [r for (c, e, o), r in FLAT.items() if o == "bf16" or e in ("BIAS_GELU", "BIAS_GELU_DG")])))
    print("accumulation |err| / (2^-24 S) per tile code (C_ACC = %g): " % GR.C_ACC + "  ".join(f"{c}: {r:.2f}" for c, r in sorted(ACC_RATIO.items())))


def _rup(a, b):
    return (a + b - 1) // b * b


def _poisoned(rows, cols, dtype, off=0, ld=None, pad_r=PAD):
    """-> (buffer [rows + pad_r, ld] full of NaN, its [rows, cols] view at column `off`)"""
    ld = ld if ld is not None else _rup(off + cols + PAD, 8)
    assert off + cols <= ld
    buf = torch.full((rows + pad_r, ld), float("nan"), dtype=dtype, device=DEV)
    return buf, buf[:rows, off:off + cols]


def _vec(n, gen, scale=1.0, shift=0.0):
    buf = torch.full((n + PAD,), float("nan"), device=DEV)
    buf[:n] = torch.randn(n, generator=gen, device=DEV) * scale + shift
    return buf[:n]


class Case:
    """Operands of one launch (poisoned buffers + views) and, lazily, its float64 reference."""

    def __init__(self, M, N, K, epi, f32, *, want2=None, p=0.0, ln=False, salt=None, seed=0, xoff=0, woff=0, ooff=0, auxoff=0,
                 ldo=None, ldaux=None, bias=True, hostile=False, x=None, w=None):
        from unimm_amd import dropout as DR
        g = torch.Generator(device=DEV).manual_seed(seed * 7919 + M * 31 + N * 17 + K + epi)
        self.M, self.N, self.K, self.epi, self.f32 = M, N, K, epi, f32
        self.want2 = (epi in GELUS) if want2 is None else want2
        self.ooff, self.ldo = ooff, ldo if ldo is not None else _rup(ooff + N, 8) + 8
        if x is None:
            self.xbuf, self.x = _poisoned(M, K, BF16, xoff)
            self.x.copy_(torch.randn((M, K), generator=g, device=DEV))
        else:
            self.x = x
        if w is None:
            self.wbuf, self.w = _poisoned(N, K, BF16, woff)
            self.w.copy_(torch.randn((N, K), generator=g, device=DEV) * 0.05)
        else:
            self.w = w
        self.bias = _vec(N, g) if bias else None
        if hostile and x is None:
            # a global gate would not see: rows a thousand times louder / quieter than the rest, loud bias columns, and
            # rows whose product with w cancels the bias (columns 0 .. 15 of rows 5 and M - 1: outputs ~ 0 beside O(1))
            self.x[0::61] *= 1e3
            self.x[1::67] *= 1e-3
            if bias:
                self.bias[3::97] *= 50.0
                c = min(16, N)
                self.x[M - 1] = self.x[5 % M]
                self.bias[:c] = -(self.x[5 % M].double() @ self.w[:c].double().t()).float()
        self.aux = self.aux_ln = None
        if epi in GR.NEEDS_AUX:
            adt = F32 if epi == GR.EPI_BIAS_DROP_RESID else BF16
            self.auxbuf, self.aux = _poisoned(M, N, adt, auxoff, ldaux)
            self.aux.copy_(torch.randn((M, N), generator=g, device=DEV) * 2 + 0.5)
            if hostile and epi in (GR.EPI_ADD, GR.EPI_BIAS_DROP_RESID) and p == 0.0 and not ln:
                # rows where the accumulator cancels the residual operand
                acc = (self.x[:4].double() @ self.w.double().t()) + (self.bias.double() if bias else 0.0)
                self.aux[:4] = (-acc).to(adt)
            if ln and epi == GR.EPI_BIAS_DROP_RESID:
                mean, rstd = _vec(M, g, 0.3, 0.5), _vec(M, g, 0.2, 1.5).abs_()
                self.aux_ln = (mean, rstd, _vec(N, g), _vec(N, g))
        self.drop, self.salt, self.salt_val = None, None, None
        if p > 0.0:
            self.drop = DR.drop_arg(p, DR.make_key(3, seed + 1, 77))
            if salt is not None:
                self.salt_val = salt
                self.salt = torch.tensor([salt - (1 << 32) if salt >= (1 << 31) else salt], dtype=torch.int32, device=DEV)
        self._ref = None

    def ref(self):
        if self._ref is None:
            self._ref = GR.launch(self.x, self.w, self.bias, self.aux, self.epi, drop=self.drop, aux_ln=self.aux_ln, N=self.N,
                                  salt=self.salt_val, out_bf16=not self.f32, out2_bf16=True)
        return self._ref

    def run(self, tile=0, splitk=0, ws=None):
        """-> (out buffer, out2 buffer or None), each [M + 8, ldo] with the result at [:M, ooff:ooff + N]"""
        from unimm_amd import lib
        M, N, o = self.M, self.N, self.ooff
        ob = torch.full((M + PAD, self.ldo), NAN32 if self.f32 else NAN16, dtype=torch.int32 if self.f32 else torch.int16,
                        device=DEV).view(F32 if self.f32 else BF16)
        ob2 = torch.full((M + PAD, self.ldo), NAN16, dtype=torch.int16, device=DEV).view(BF16) if self.want2 else None
        drop = None if self.drop is None else (self.drop + ((self.salt,) if self.salt is not None else ()))
        lib.gemm_nt(self.x, self.w, ob[:M, o:o + N], bias=self.bias, epilogue=self.epi, aux=self.aux,
                    out2=None if ob2 is None else ob2[:M, o:o + N], drop=drop, M=M, N=N, K=self.K, aux_ln=self.aux_ln, tile=tile,
                    splitk=splitk, splitk_ws=ws)
        return ob, ob2

    def _outside_unchanged(self, buf):
        f32 = buf.dtype == F32
        iv = buf.view(torch.int32 if f32 else torch.int16).clone()
        iv[:self.M, self.ooff:self.ooff + self.N] = NAN32 if f32 else NAN16
        return bool((iv == (NAN32 if f32 else NAN16)).all())

    def check(self, res, section, code):
        """Sentinels + the per-element gate over all M x N elements of out (and out2); -> worst |err| / E"""
        ob, ob2 = res
        torch.cuda.synchronize()
        r = self.ref()
        M, N, o = self.M, self.N, self.ooff
        what = (section, code, GR.EPI_NAMES[self.epi], M, N, self.K, self.f32, self.ldo)
        key = (section, code % 100, GR.EPI_NAMES[self.epi], "f32" if self.f32 else "bf16")
        assert self._outside_unchanged(ob), ("out: written outside [0, M) x [0, N)",) + what
        worst = GR.worst_ratio(ob[:M, o:o + N], r["ref"], r["E"])
        lit = GR.worst_ratio(ob[:M, o:o + N], r["ref"], r["lit"])
        if ob2 is not None:
            assert self._outside_unchanged(ob2), ("out2: written outside [0, M) x [0, N)",) + what
            worst = max(worst, GR.worst_ratio(ob2[:M, o:o + N], r["ref2"], r["E2"]))
            lit = max(lit, GR.worst_ratio(ob2[:M, o:o + N], r["ref2"], r["lit2"]))
        FLAT[key[1:]] = max(FLAT[key[1:]], lit)
        STATS[key] = max(STATS[key], worst)
        COUNT[section] += 1
        assert worst <= 1.0, ("|err| / E", worst) + what
        return worst


def _bits(res):
    ob, ob2 = res
    a = ob.view(torch.int32 if ob.dtype == F32 else torch.int16)
    return a if ob2 is None else (a, ob2.view(torch.int16))


def _same(ra, rb):
    a, b = _bits(ra), _bits(rb)
    if isinstance(a, tuple):
        return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    return torch.equal(a, b)


# ----------------------------------------------------------------------------------------------------------------------
# A. geometry x kernel
# ----------------------------------------------------------------------------------------------------------------------
def _plan_a(code):
    BM, BN = GR.tile_dims(code)[:2]
    Ms = [1, BM - 1, BM, BM + 1, 2 * BM + 17]
    Nfast = [64, BN, 2 * BN]
    Nedge = [1, 7, 63, 65, BN - 1, BN + 8, 2 * BN + 36]
    Ks = [64, 128, 192, 448]
    plan, i = [], 0
    for k, (epi, f32) in enumerate(KERNELS):
        for want2 in ((True, False) if epi in GELUS else (None,)):
            for fast in (True, False):
                M, K = Ms[(i + k) % 5], Ks[(i // 2 + i) % 4]
                N = Nfast[i % 3] if fast else Nedge[i % 7]
                vo, va = (True, True) if fast else ((i // 2) % 2 == 0, (i // 4) % 2 == 0)     # 16-byte paths of out / aux
                plan.append(dict(M=M, N=N, K=K, epi=epi, f32=f32, want2=want2, fast=fast, vo=vo, va=va, i=i))
                i += 1
    return plan


@pytest.mark.parametrize("code", GR.TILE_CODES)
def test_a_geometry_and_every_kernel(code):
    plan = _plan_a(code)
    BM, BN = GR.tile_dims(code)[:2]
    seen = defaultdict(set)
    worst = 0.0
    for c in plan:
        i, N, epi = c["i"], c["N"], c["epi"]
        ooff, auxoff = (8, 8) if i % 2 else (0, 0)
        ldo = _rup(ooff + N, 8) + 8 + (0 if c["vo"] else 4)               # e.g. 1000 / 1004: rows 16-byte aligned or not
        ldaux = _rup(auxoff + N, 8) + 16 + (0 if c["va"] else 4)          # != ldo
        p = 0.1 if epi == GR.EPI_BIAS_DROP_RESID else 0.0
        case = Case(c["M"], N, c["K"], epi, c["f32"], want2=c["want2"], p=p, ln=(i % 3 != 0), seed=code * 100 + i,
                    xoff=8 * (i % 3), woff=8 * ((i + 1) % 4), ooff=ooff, auxoff=auxoff, ldo=ldo, ldaux=ldaux,
                    bias=not (epi in (GR.EPI_DGELU, GR.EPI_ADD, GR.EPI_MUL) and i % 2))
        worst = max(worst, case.check(case.run(tile=code), "A", code))
        seen["M"].add(c["M"]); seen["N"].add(N); seen["K"].add(c["K"])
        seen["kernel", c["fast"]].add((epi, c["f32"]))
        if epi in GELUS:
            seen["gelu"].add((epi, c["f32"], c["fast"], case.want2))
        if not c["fast"]:
            seen["strides"].add((c["vo"], c["va"]))
    assert seen["M"] == {1, BM - 1, BM, BM + 1, 2 * BM + 17} and seen["K"] == {64, 128, 192, 448}
    assert seen["N"] == {64, BN, 2 * BN, 1, 7, 63, 65, BN - 1, BN + 8, 2 * BN + 36}
    assert seen["kernel", True] == seen["kernel", False] == set(KERNELS)
    assert len(seen["gelu"]) == 16 and len(seen["strides"]) == 4
    print(f"\nA tile {code}: {len(plan)} launches, worst |err| / E {worst:.3f}")


# ----------------------------------------------------------------------------------------------------------------------
# B. launch forms, same-K-order pairs
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_case():
    c = Case(8300, 3072, 768, GR.EPI_BIAS_DROP_RESID, True, p=0.1, ln=True, seed=41, ldo=3072, ldaux=3072 + 8)
    c.ref()
    yield c
    c._ref = None


@pytest.mark.parametrize("code", GR.TILE_CODES)
def test_b_persistent_and_one_per_tile_forms_are_bit_identical(code, big_case):
    """x1xx (persistent workgroups) and x2xx (one workgroup per tile) on a grid of several rounds, dropout + lazy LayerNorm
    residual: the same bits, and they pass the gate."""
    a = big_case.run(tile=100 + code)
    b = big_case.run(tile=200 + code)
    w = big_case.check(a, "B", code)
    assert _same(a, b)
    print(f"\nB tile {code}: worst |err| / E {w:.3f}")


@pytest.mark.parametrize("K", [64, 128, 192, 768, 3072])
def test_b_tiles_with_the_same_k_order_are_bit_identical(K):
    """A pure accumulation (fp32 output, no bias) from 1 to 48 K steps on every tile: the gate, the measured accumulation
    ratio, and bit-identity of the tiles that differ only in how they stage their operands."""
    c = Case(777, 1000, K, GR.EPI_BIAS, True, bias=False, seed=K, hostile=True)
    S = c.x.double().abs() @ c.w.double().abs().t()
    res = {}
    for code in GR.TILE_CODES:
        res[code] = c.run(tile=code)
        c.check(res[code], "B", code)
        got = res[code][0][:c.M, :c.N].double()
        ACC_RATIO[code] = max(ACC_RATIO[code], float(((got - c.ref()["ref"]).abs() / (GR.U32 * S)).max()))
    for a, b in GR.SAME_K_ORDER:
        assert _same(res[a], res[b]), (a, b, K)
    print(f"\nB K = {K}: accumulation |err| / (2^-24 S): " + "  ".join(f"{k}: {ACC_RATIO[k]:.2f}" for k in GR.TILE_CODES))


# ----------------------------------------------------------------------------------------------------------------------
# C. tile order
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("code", GR.TILE_CODES)
def test_c_tile_order_groups(code):
    """gn tile columns per group on 5 tile columns: gn = 3 and 4 leave a narrower last group, 7 and 100 exceed the number of
    tile columns, 1 is column-major.  Which workgroup computes a tile must not change a bit of it."""
    BM, BN = GR.tile_dims(code)[:2]
    c = Case(3 * BM + 5, 5 * BN - 20, 128, GR.EPI_ADD, False, seed=code, ooff=8)
    base = c.run(tile=code)
    c.check(base, "C", code)
    for gn in (1, 3, 7, 100):
        r = c.run(tile=gn * 1000 + code)
        assert _same(base, r), (code, gn)
        c.check(r, "C", code)


# ----------------------------------------------------------------------------------------------------------------------
# D. split-K
# ----------------------------------------------------------------------------------------------------------------------
class Workspace:
    """A split-K workspace of exactly `nbytes` at a 256-byte aligned offset inside a buffer filled with a NaN pattern; the
    counters (first 16 KiB) zeroed, the slabs left as NaN: a slab word read before it was written poisons the output."""
    OFF = 4096

    def __init__(self, cap):
        self.pool = torch.empty((self.OFF + cap + 4096) // 4, dtype=torch.int32, device=DEV)
        self.init = None

    def view(self, nbytes):
        self.pool.fill_(NAN32)
        b = self.pool.view(torch.uint8)
        self.nbytes = nbytes
        b[self.OFF:self.OFF + GR.COUNTER_BYTES].zero_()
        self.init = b.clone()
        ws = b[self.OFF:self.OFF + nbytes]
        assert ws.data_ptr() % 256 == 0
        return ws

    def after(self):
        """-> (the launch split, i.e. wrote slabs; counters all zero; bytes outside the workspace unchanged)"""
        torch.cuda.synchronize()
        b, o, n = self.pool.view(torch.uint8), self.OFF, self.nbytes
        split = not torch.equal(b[o + GR.COUNTER_BYTES:o + n], self.init[o + GR.COUNTER_BYTES:o + n])
        zero = int(b[o:o + GR.COUNTER_BYTES].max()) == 0
        outside = torch.equal(b[:o], self.init[:o]) and torch.equal(b[o + n:], self.init[o + n:])
        return split, zero, outside


D_M, D_N = 3900, 768
D_EPIS = [(GR.EPI_BIAS, False), (GR.EPI_ADD, False), (GR.EPI_MUL, False), (GR.EPI_BIAS_DROP_RESID, True), (GR.EPI_BIAS_GELU_DG, False),
          (GR.EPI_BIAS_GELU, True)]
D_KS = [512, 1024, 2304, 2368, 3072]


@pytest.fixture(scope="module")
def d_cases():
    cache = {}

    def get(K, epi, f32):
        if (K, epi, f32) not in cache:
            cache[K, epi, f32] = Case(D_M, D_N, K, epi, f32, p=0.1 if epi == GR.EPI_BIAS_DROP_RESID else 0.0, seed=K, ldo=D_N,
                                      hostile=True)
        return cache[K, epi, f32]
    yield get
    cache.clear()


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("code", GR.SPLIT_CODES)
def test_d_split_k(code, d_cases):
    cus = _cus()
    W = Workspace(GR.ws_bytes(D_M, D_N, code, 4))
    i, worst, nsplit_seen = code, 0.0, set()
    for want in (2, 3, 4, -1):
        for K in D_KS:
            epi, f32 = D_EPIS[i % len(D_EPIS)]
            i += 1
            c = d_cases(K, epi, f32)
            # the workspace this request needs if it splits as far as it may (the library's choice: given room for 4)
            ns_room = GR.splits(D_M, D_N, K, code, want, 1 << 40, cus)
            need = max(GR.ws_bytes(D_M, D_N, code, ns_room), GR.WS_MIN_BYTES)
            ns = GR.splits(D_M, D_N, K, code, want, need, cus)
            assert ns == ns_room
            res = c.run(tile=code, splitk=want, ws=W.view(need))
            split, zero, outside = W.after()
            worst = max(worst, c.check(res, "D", code))
            assert split == (ns > 1), (code, want, K, ns)
            assert zero and outside, (code, want, K, zero, outside)
            nsplit_seen.add(ns)
            if K == 512:
                assert ns == 1                  # 8 steps: fewer than 8 per split, must run unsplit
            if ns > 1:                          # one byte less: unsplit, and still right
                res = c.run(tile=code, splitk=want, ws=W.view(need - 1))
                split, zero, outside = W.after()
                assert not split and zero and outside, (code, want, K)
                c.check(res, "D", code)
                assert GR.splits(D_M, D_N, K, code, want, need - 1, cus) == 1
    assert {1, 2, 3, 4} <= nsplit_seen
    # two splits: bit-identical from launch to launch (a + b does not depend on who arrives last), with p = 1 and p = 2 alike
    for epi, f32 in D_EPIS:
        c = d_cases(2368, epi, f32)
        need = GR.ws_bytes(D_M, D_N, code, 2)
        first = c.run(tile=code, splitk=2, ws=W.view(need))
        assert W.after() == (True, True, True)
        for tile in (code, 100 + code, 200 + code):
            again = c.run(tile=tile, splitk=2, ws=W.view(need))
            assert W.after() == (True, True, True), (code, tile)       # x1xx: the host drops persistence and still splits
            assert _same(first, again), (code, tile, GR.EPI_NAMES[epi])
    print(f"\nD tile {code}: worst |err| / E {worst:.3f}")


@pytest.mark.parametrize("code", [3, 6, 8, 12])
def test_d_split_request_on_an_eight_wave_tile_is_ignored(code, d_cases):
    W = Workspace(GR.ws_bytes(D_M, D_N, 1, 4))
    for K, (epi, f32) in zip((2304, 3072), (D_EPIS[3], D_EPIS[4])):
        c = d_cases(K, epi, f32)
        base = c.run(tile=code)
        c.check(base, "D", code)
        for want in (2, 4, -1):
            res = c.run(tile=code, splitk=want, ws=W.view(GR.ws_bytes(D_M, D_N, 1, 4)))
            assert W.after() == (False, True, True)
            assert _same(base, res), (code, want)


# ----------------------------------------------------------------------------------------------------------------------
# E. salt
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("code", GR.TILE_CODES)
def test_e_dropout_salt_word(code):
    """(key, salt word S) draws the mask of (key ^ S, no salt); rewriting the device word changes the mask of an otherwise
    identical launch to the one the host mirror predicts.  N = 520: FAST waves (the split-column map of the fp32 epilogue) and
    a ragged edge."""
    from unimm_amd import dropout as DR
    S1, S2 = 0x9E3779B1, 0x00C0FFEE
    salted = Case(300, 520, 128, GR.EPI_BIAS_DROP_RESID, True, p=0.3, ln=True, salt=S1, seed=code)
    plain = Case(300, 520, 128, GR.EPI_BIAS_DROP_RESID, True, p=0.3, ln=True, seed=code)
    assert torch.equal(salted.x, plain.x) and torch.equal(salted.aux, plain.aux)
    key = salted.drop[0]
    a = salted.run(tile=code)
    salted.check(a, "E", code)
    plain.drop = DR.drop_arg(0.3, key ^ S1)
    b = plain.run(tile=code)
    assert _same(a, b)
    plain.drop = DR.drop_arg(0.3, key)
    c = plain.run(tile=code)
    plain.check(c, "E", code)
    assert not _same(a, c)                      # the salt is not ignored
    salted.salt.fill_(S2)                       # the next step's word, same launch arguments
    salted.salt_val, salted._ref = S2, None
    d = salted.run(tile=code)
    salted.check(d, "E", code)
    assert not _same(a, d)


# ----------------------------------------------------------------------------------------------------------------------
# F. production shapes
# ----------------------------------------------------------------------------------------------------------------------
_E = GR                                   # (epilogue constants)
TXT, IMG, MSK, TXT30, IMG30 = 31162, 8880, 4675, 3900, 1110
F_CASES = [
    # (M, N, K, epilogue, fp32 out, kwargs of Case, tile, splitk)
    (TXT, 2304, 768, _E.EPI_BIAS, False, {}, 0, 0),
    (TXT, 768, 768, _E.EPI_BIAS_DROP_RESID, True, dict(p=0.1, ln=True), 0, 0),
    (TXT, 3072, 768, _E.EPI_BIAS_GELU_DG, False, {}, 0, 0),
    (TXT, 768, 3072, _E.EPI_BIAS_DROP_RESID, True, dict(p=0.1), 0, 0),
    (TXT, 3072, 768, _E.EPI_MUL, False, dict(bias=False), 0, 0),
    (TXT, 768, 3072, _E.EPI_ADD, False, dict(bias=False), 0, 0),
    (TXT, 768, 768, _E.EPI_BIAS, False, dict(bias=False), 0, 0),
    (TXT, 768, 2304, _E.EPI_ADD, False, dict(bias=False), 0, 0),
    (IMG, 3072, 1024, _E.EPI_BIAS, False, {}, 0, 0),
    (IMG, 1024, 1024, _E.EPI_BIAS_DROP_RESID, True, dict(p=0.1), 0, 0),
    (IMG, 1024, 1024, _E.EPI_BIAS_GELU_DG, False, {}, 0, 0),
    (IMG, 1024, 1024, _E.EPI_MUL, False, dict(bias=False), 0, 0),
    (MSK, 768, 768, _E.EPI_BIAS_GELU, True, {}, 0, 0),
    (MSK, 30522, 768, _E.EPI_BIAS, True, dict(ldo=30528), 0, 0),
    (IMG, 1024, 1024, _E.EPI_BIAS_GELU, True, {}, 0, 0),
    (IMG, 1601, 1024, _E.EPI_BIAS, True, dict(ldo=1604), 0, 0),
    (MSK, 768, 30528, _E.EPI_BIAS, False, dict(bias=False), 0, 0),
    (TXT, 768, 2304, _E.EPI_BIAS, True, {}, 0, 0),
    (TXT30, 768, 9216, _E.EPI_BIAS_DROP_RESID, True, dict(bias=False), 1, 2),
    (TXT30, 768, 2304, _E.EPI_BIAS, True, {}, 9, 0),
    (TXT30, 768, 3072, _E.EPI_BIAS_DROP_RESID, True, dict(p=0.1), 1, 2),
    (TXT30, 768, 2304, _E.EPI_ADD, False, dict(bias=False), 1, 2),
    (TXT30, 2304, 768, _E.EPI_BIAS, False, {}, 1, 0),
    (TXT30, 768, 768, _E.EPI_BIAS_DROP_RESID, True, dict(p=0.1, ln=True), 7, 0),
    (TXT30, 3072, 768, _E.EPI_BIAS_GELU_DG, False, {}, 1, 0),
    (IMG30, 1024, 1024, _E.EPI_BIAS_GELU_DG, False, {}, 14, 0),
    (IMG30, 3072, 1024, _E.EPI_BIAS, False, {}, 14, 0),
]


@pytest.mark.parametrize("idx", range(len(F_CASES)))
def test_f_production_shapes(idx):
    M, N, K, epi, f32, kw, tile, sk = F_CASES[idx]
    kw = dict(kw)
    kw.setdefault("ldo", N)
    c = Case(M, N, K, epi, f32, seed=idx, hostile=True, ldaux=N if epi in GR.NEEDS_AUX else None, **kw)
    ws = None
    if sk:
        W = Workspace(GR.ws_bytes(M, N, tile, sk))
        ws = W.view(GR.ws_bytes(M, N, tile, sk))
    res = c.run(tile=tile, splitk=sk, ws=ws)
    if sk:
        assert W.after() == (GR.splits(M, N, K, tile, sk, GR.ws_bytes(M, N, tile, sk), _cus()) > 1, True, True)
    w = c.check(res, "F", tile)
    print(f"\nF {M} x {N} x {K} {GR.EPI_NAMES[epi]} {'f32' if f32 else 'bf16'} tile {tile} splitk {sk}: worst |err| / E {w:.3f}")


# ----------------------------------------------------------------------------------------------------------------------
# G. past 4 GiB
# ----------------------------------------------------------------------------------------------------------------------
G_ROWS, G_LD = 31162, 68928


@pytest.fixture(scope="module")
def wide_buffer():
    need = G_ROWS * G_LD * 2
    free = torch.cuda.mem_get_info()[0]
    if free < need + (2 << 30):
        pytest.skip(f"needs {need + (2 << 30)} bytes of free device memory, the device reports {free}")
    buf = torch.empty((G_ROWS, G_LD), dtype=BF16, device=DEV)
    buf.view(torch.int16).fill_(NAN16)
    assert buf.numel() * 2 > 1 << 32
    g = torch.Generator(device=DEV).manual_seed(99)
    buf[:, 1024:1088] = torch.randn((G_ROWS, 64), generator=g, device=DEV).to(BF16)
    buf[:30522, 40000:40064] = (torch.randn((30522, 64), generator=g, device=DEV) * 0.05).to(BF16)     # rows past N stay NaN
    yield buf
    del buf
    torch.cuda.empty_cache()


@pytest.mark.parametrize("code", [8, 12, 1])
def test_g_x_rows_span_more_than_4_gib(code, wide_buffer):
    """x = [31162, 64] at row stride 68,928: its last rows lie past byte 2^32 of the view.  A request for the ping-pong tile
    must take the lock-step ring (its bits are tile 3's).  Gated over all rows, the last row tile included."""
    x = wide_buffer[:, 1024:1088]
    assert (x[-1].data_ptr() - x.data_ptr()) >= 1 << 32
    c = Case(G_ROWS, 200, 64, GR.EPI_BIAS, True, x=x, seed=code)
    res = c.run(tile=code)
    w = c.check(res, "G", code)
    BM = GR.tile_dims(code)[0]
    last = slice((G_ROWS - 1) // BM * BM, G_ROWS)
    tail = GR.worst_ratio(res[0][last, :200], c.ref()["ref"][last], c.ref()["E"][last])
    assert tail <= 1.0
    if code == 8:
        assert _same(res, c.run(tile=3))
    print(f"\nG x past 4 GiB, tile {code}: worst |err| / E {w:.3f} (last row tile {tail:.3f})")


@pytest.mark.parametrize("code", [8, 12, 1])
def test_g_w_rows_up_to_4_gib(code, wide_buffer):
    """w = 30,522 rows of the same buffer at another column offset (4.2 GB: byte offsets that need all 32 bits), small M."""
    w = wide_buffer[:30522, 40000:40064]
    assert (w[-1].data_ptr() - w.data_ptr()) >= 1 << 31
    c = Case(130, 30522, 64, GR.EPI_BIAS, True, w=w, seed=code, ldo=30528)
    res = c.run(tile=code)
    wr = c.check(res, "G", code)
    BN = GR.tile_dims(code)[1]
    last = slice((30522 - 1) // BN * BN, 30522)
    assert GR.worst_ratio(res[0][:130, last], c.ref()["ref"][:, last], c.ref()["E"][:, last]) <= 1.0
    print(f"\nG w up to 4 GiB, tile {code}: worst |err| / E {wr:.3f}")


# ----------------------------------------------------------------------------------------------------------------------
# argument checks (host side: nothing is launched)
# ----------------------------------------------------------------------------------------------------------------------
def test_misaligned_aux_and_out2_are_rejected():
    from unimm_amd import lib
    x = torch.zeros((128, 64), device=DEV, dtype=BF16)
    w = torch.zeros((128, 64), device=DEV, dtype=BF16)
    out = torch.zeros((128, 128), device=DEV, dtype=BF16)
    aux = torch.zeros((129, 136), device=DEV, dtype=BF16)
    out2 = torch.zeros((129, 128), device=DEV, dtype=BF16)
    lib.gemm_nt(x, w, out, epilogue=lib.EPI_ADD, aux=aux[:128, 8:])                 # 16 bytes in: fine
    with pytest.raises(lib.UnimmHipError, match="ALIGN"):
        lib.gemm_nt(x, w, out, epilogue=lib.EPI_ADD, aux=aux[:128, 4:])             # 8 bytes in
    with pytest.raises(lib.UnimmHipError, match="ALIGN"):
        lib.gemm_nt(x, w, out, epilogue=lib.EPI_BIAS_GELU, out2=out2.view(-1)[4:4 + 128 * 128].view(128, 128))
    o32 = torch.zeros((128, 128), device=DEV)
    a32 = torch.zeros((129, 132), device=DEV)
    with pytest.raises(lib.UnimmHipError, match="ALIGN"):
        lib.gemm_nt(x, w, o32, epilogue=lib.EPI_BIAS_DROP_RESID, aux=a32[:128, 2:130])
    lib.gemm_nt(x, w, out, aux=aux[:128, 4:])                                       # an epilogue that does not read aux ignores it
    torch.cuda.synchronize()
