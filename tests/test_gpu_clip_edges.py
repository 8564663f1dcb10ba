"""`unimm_grad_norm` and `unimm_adamw_step_clipped` (csrc/optim.hip) through the C ABI against tests/clip_ref.py and
oracle/adamw_ref.adamw_step, at the sizes where the norm kernel's grid-stride loop and the chunk -> group table can go wrong.

One pass of the norm kernel covers 2048 workgroups x 256 lanes x 2 vectors x 4 elements = 4,194,304 elements (lib.GRAD_NORM_PASS,
the same count as one pass of the update kernel):
    n = 64, 192            one chunk; three chunks
    n = PASS               one full pass (every lane's second vector is the last it can take)
    n = PASS + 64          one chunk in the second pass
    n = 64 x 163,841       a ragged third pass
Arrays, group table and sentinels are those of tests/test_gpu_optim_edges.py (64 NaN-pattern elements around every array, a table
that changes at every chunk, the first and the last chunk alone in groups 0 and 7); chunks with the ids 8, 200 and 255 hold NaN
gradients here, since the norm pass must not read them.  The workspace and the state block sit between sentinels too.

Bounds.  Sums of squares: every term is an exact fp64 product and non-negative, every addition an fp64 addition, and no chain
of additions is longer than 2 n / PASS + 48 < 4096, so |sum - exact| <= 4096 x 1.1e-16 = 4.5e-13 relative for any summation tree;
numpy's pairwise sum obeys the same bound: rtol 1e-12.  scale = fp32(grad_scale x coef) may differ from the restatement's by one
fp32 neighbour when the last bits of the fp64 norm move the rounding; which it was is printed.  The update: the project's rule of
tests/test_gpu_optim_edges.py (m, v bit-equal, p within rtol 1e-6 / atol 1e-9, w16 bit-equal to bf16(p)) against the oracle fed
g x (the device's own scale).

Measured on an MI355X: every sum and norm within 2 units of the 17th digit of the restatement's (relative 2e-16), scale the
restatement's own fp32 value in all 21 comparisons, never the neighbour."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import adamw_ref as AR
from tests.clip_ref import clip_ref
from tests.test_gpu_optim_edges import DEV, GUARD, LRS, NAN16, SKIP_IDS, WDS, Arena, bf16_bits, gradients, group_table

pytestmark = pytest.mark.gpu
NAN64 = 0x7FF8A5A5A5A5A5A5
RTOL = 1e-12


def _lib():
    from unimm_amd import lib
    return lib


def PASS():
    return _lib().GRAD_NORM_PASS


class Blocks:
    """workspace and state block, each between GUARD sentinel doubles (a NaN pattern)"""

    def __init__(self):
        lib = _lib()
        self.nws, self.nst = lib.GRAD_NORM_WS_DOUBLES, lib.CLIP_STATE_DOUBLES + 1            # state padded to 112 bytes: 16-B guards
        self.ws_buf = torch.full((self.nws + 2 * GUARD,), NAN64, dtype=torch.int64, device=DEV).view(torch.float64)
        self.st_buf = torch.full((self.nst + 2 * GUARD,), NAN64, dtype=torch.int64, device=DEV).view(torch.float64)
        self.state.zero_()

    @property
    def ws(self):
        return self.ws_buf[GUARD:GUARD + self.nws]

    @property
    def state(self):
        return self.st_buf[GUARD:GUARD + self.nst]

    def guards_ok(self):
        w, s = self.ws_buf.view(torch.int64).cpu().numpy(), self.st_buf.view(torch.int64).cpu().numpy()
        return all((a[:GUARD] == NAN64).all() and (a[-GUARD:] == NAN64).all() for a in (w, s)) and s[GUARD + self.nst - 1] == 0

    def read(self):
        """the state block as host values, and its raw bytes"""
        lib = _lib()
        raw = self.state.cpu().numpy().tobytes()[:C.sizeof(lib.ClipState)]
        st = lib.ClipState.from_buffer_copy(raw)
        return dict(group_sumsq=np.array(st.group_sumsq[:]), sumsq=st.sumsq, norm=st.norm, coef=st.coef,
                    scale=np.float32(st.scale), nonfinite=st.nonfinite, skipped=st.skipped), raw


def make(n, seed=0, table=None, n_groups=8):
    """host arrays and their device Arena; gradients of the chunks that do not count are NaN.
    Second moments are bounded below, sqrt(v) >= 5e-4 against |m| ~ 1e-3: the rule's rtol is relative to the UPDATED p, so it
    cannot absorb the single-ulp difference of the update's sqrt / divide (tests/test_gpu_optim_edges.py) once the update is
    large and cancels p; its atol of 1e-9 can, while the update stays below 2^-6 (ulp 9.3e-10).  Here |m / (sqrt(v) + eps)| <=
    (1 - b1) / sqrt(1 - b2) + 0.9 |m0| / sqrt(0.999 v0) <= 3.2 + 1.8 x 5.5 = 13 and step size <= 1e-3 x 0.316: |update| < 2^-7."""
    rng = np.random.default_rng(2000 + seed + n % 9973)
    table = group_table(n // 64, rng) if table is None else table
    eg = np.repeat(table, 64)
    p = rng.standard_normal(n).astype(np.float32)
    m = (rng.standard_normal(n) * 1e-3).astype(np.float32)
    v = np.square((np.abs(rng.standard_normal(n)) + 0.5) * 1e-3).astype(np.float32)
    g, _ = gradients(n, rng, v, eg)                                   # includes 0, 1e-30 and 1e25 elements
    g[eg >= n_groups] = np.nan
    return dict(n=n, table=table, eg=eg, p=p, m=m, v=v, g=g, n_groups=n_groups)


def arena_of(h):
    A = Arena(h["n"], h["p"], h["m"], h["v"], h["table"])
    A.view("g").copy_(torch.from_numpy(h["g"]))
    return A


def host_all(A):
    torch.cuda.synchronize()
    out = {}
    for k in ("p", "g", "m", "v", "w16"):
        bits, ok = A.host(k)
        assert ok, f"sentinels of {k} written"
        out[k] = bits.copy()
    return out


def norm_pass(A, B, h, grad_scale, max_norm):
    _lib().grad_norm(A.view("g"), A.table(), h["n_groups"], B.ws, B.state, grad_scale=grad_scale, max_norm=max_norm)
    got, raw = B.read()
    assert B.guards_ok(), "sentinels of the workspace or the state block written"
    return got, raw


def step(A, h, t=1, grad_scale=1.0, zero_grad=False, state=None, skip_nonfinite=False, w16=True):
    n_groups = h["n_groups"]
    _lib().adamw_step(A.view("p"), A.view("g"), A.view("m"), A.view("v"), A.table(), LRS[:n_groups], WDS[:n_groups], t,
                      w16=A.view("w16") if w16 else None, grad_scale=grad_scale, zero_grad=zero_grad, clip_state=state,
                      skip_nonfinite=skip_nonfinite)


def check_against_ref(name, got, ref, max_norm):
    for k in range(8):
        a, b = got["group_sumsq"][k], ref["group_sumsq"][k]
        assert abs(a - b) <= RTOL * b, f"{name}: group_sumsq[{k}] {a!r} vs {b!r}"
    for key in ("sumsq", "norm"):
        assert abs(got[key] - ref[key]) <= RTOL * ref[key], f"{name}: {key} {got[key]!r} vs {ref[key]!r}"
    assert got["nonfinite"] == ref["nonfinite"] == 0
    assert (got["coef"] == 1.0) == (got["norm"] < max_norm), f"{name}: coef {got['coef']!r} norm {got['norm']!r}"
    assert abs(got["coef"] - ref["coef"]) <= 2 * RTOL * ref["coef"]
    near = (ref["scale"], np.nextafter(ref["scale"], np.float32(np.inf)), np.nextafter(ref["scale"], np.float32(-np.inf)))
    which = "the restatement's value" if got["scale"] == ref["scale"] else "its fp32 neighbour"
    print(f"\n{name}: norm {got['norm']:.17g} (ref {ref['norm']:.17g}) coef {got['coef']:.17g} scale {got['scale']!r}: {which}")
    assert got["scale"] in near, f"{name}: scale {got['scale']!r} vs {ref['scale']!r}"


def oracle_update(h, scale, t=1):
    """the oracle per group on g * scale -> (p, m, v) of the updated arrays; chunks with an id >= n_groups keep their values here
    (what happens to them is pinned by tests/test_gpu_optim_edges.py and not looked at)"""
    p, m, v = h["p"].copy(), h["m"].copy(), h["v"].copy()
    with np.errstate(over="ignore", invalid="ignore"):
        for gi in range(h["n_groups"]):
            sel = h["eg"] == gi
            if sel.any():
                pp, mm, vv = p[sel], m[sel], v[sel]
                AR.adamw_step(pp, h["g"][sel] * np.float32(scale), mm, vv, LRS[gi], WDS[gi], t)
                p[sel], m[sel], v[sel] = pp, mm, vv
    return p, m, v


def SIZES():
    P = 2048 * 256 * 2 * 4
    return [(64, "one chunk"), (192, "three chunks"), (P, "one full pass"), (P + 64, "one chunk in the second pass"),
            (64 * 163841, "ragged third pass")]


@pytest.mark.parametrize("n,what", SIZES(), ids=[f"n={n} {w}" for n, w in SIZES()])
def test_norm_and_clipped_update(n, what):
    assert SIZES()[2][0] == PASS()
    h = make(n)
    counted = h["eg"] < 8
    assert h["table"][0] == 0 and h["table"][-1] == (7 if n > 64 else 0)
    if n >= PASS():
        assert all((h["table"] == s).any() for s in SKIP_IDS)
    B = Blocks()
    grad_scale = 0.25
    # the 1e25 elements dominate the sums above: once more without them, so that the ordinary elements are held to the bound too
    h2 = dict(h, g=np.where(h["g"] == np.float32(1e25), np.float32(0.37), h["g"]))
    got2, _ = norm_pass(arena_of(h2), B, h2, 1.0, 1.0)
    check_against_ref(f"{what}, no huge elements", got2, clip_ref(h2["g"], h2["eg"], 8, 1.0, 1.0), 1.0)
    measured = clip_ref(h["g"], h["eg"], 8, grad_scale)["norm"]
    for case, max_norm in (("clipping", 0.5 * measured), ("not clipping", 10.0 * measured), ("measure only", float("inf"))):
        A = arena_of(h)
        ref = clip_ref(h["g"], h["eg"], 8, grad_scale, max_norm)
        got, raw = norm_pass(A, B, h, grad_scale, max_norm)
        check_against_ref(f"{what}, {case}", got, ref, max_norm)
        # the first and the last chunk sit alone in their groups
        x0, x1 = h["g"][:64].astype(np.float64), h["g"][-64:].astype(np.float64)
        if n > 64:
            assert abs(got["group_sumsq"][0] - np.sum(x0 * x0)) <= RTOL * np.sum(x0 * x0)
            assert abs(got["group_sumsq"][7] - np.sum(x1 * x1)) <= RTOL * np.sum(x1 * x1)
        _, raw2 = norm_pass(A, B, h, grad_scale, max_norm)
        assert raw2 == raw, "two launches on one input differ"
        if case == "measure only":
            assert got["coef"] == 1.0 and got["scale"] == np.float32(grad_scale)
            continue
        p_ref, m_ref, v_ref = oracle_update(h, got["scale"])
        for zero_grad in (False, True):
            A = arena_of(h)
            step(A, h, grad_scale=123.0, zero_grad=zero_grad, state=B.state)        # args.grad_scale is ignored
            out = host_all(A)
            assert np.array_equal(out["m"][counted], m_ref.view(np.int32)[counted]), f"{what}, {case}: m"
            assert np.array_equal(out["v"][counted], v_ref.view(np.int32)[counted]), f"{what}, {case}: v"
            p_got = out["p"].view(np.float32)
            assert np.allclose(p_got[counted], p_ref[counted], rtol=1e-6, atol=1e-9), f"{what}, {case}: p"
            assert np.array_equal(out["w16"][counted], bf16_bits(p_got)[counted]), f"{what}, {case}: w16"
            for k in ("p", "m", "v"):
                assert np.array_equal(out[k][~counted], h[k].view(np.int32)[~counted]), f"{what}, {case}: skipped {k}"
            assert (out["w16"][~counted] == np.int16(NAN16)).all()
            g_expect = h["g"].copy()
            if zero_grad:
                g_expect[counted] = 0.0
            assert np.array_equal(out["g"], g_expect.view(np.int32)), f"{what}, {case}: g (zero_grad={zero_grad})"
            if case == "not clipping":                                               # coef == 1: the plain step's bits
                assert got["coef"] == 1.0 and got["scale"].tobytes() == np.float32(grad_scale).tobytes()
                A2 = arena_of(h)
                step(A2, h, grad_scale=grad_scale, zero_grad=zero_grad)
                plain = host_all(A2)
                for k in plain:
                    assert np.array_equal(out[k], plain[k]), f"{what}: {k} differs from unimm_adamw_step (zero_grad={zero_grad})"


def test_chunks_of_an_unused_group_add_nothing():
    """n_groups = 4: chunk ids 4 .. 7 hold NaN gradients here and must not reach the norm"""
    rng = np.random.default_rng(3)
    table = rng.integers(0, 8, size=64).astype(np.uint8)
    table[[0, 9, 63]] = (5, 6, 7)
    table[[5, 17, 40]] = SKIP_IDS
    h = make(64 * 64, table=table, n_groups=4)
    assert np.isnan(h["g"][h["eg"] >= 4]).all() and ((h["eg"] >= 4) & (h["eg"] < 8)).sum() >= 3 * 64
    A, B = arena_of(h), Blocks()
    ref = clip_ref(h["g"], h["eg"], 4, 1.0, 1.0)
    got, _ = norm_pass(A, B, h, 1.0, 1.0)
    check_against_ref("n_groups=4", got, ref, 1.0)
    assert (got["group_sumsq"][4:] == 0).all() and (got["group_sumsq"][:4] > 0).all()


@pytest.mark.parametrize("n", [64 * 41, 2048 * 256 * 2 * 4 + 64], ids=["n=2624", "n=PASS+64"])
def test_nonfinite_guard(n):
    """+inf, then NaN, in a counted chunk (the last one: the second pass at the larger size)"""
    h = make(n, seed=5)
    counted = h["eg"] < 8
    B = Blocks()
    skipped = 0
    for bad in (np.inf, np.nan, -np.inf):
        hb = dict(h, g=h["g"].copy())
        hb["g"][n - 7] = bad
        for zero_grad in (False, True):
            A = arena_of(hb)
            got, _ = norm_pass(A, B, hb, 0.5, 1.0)
            skipped += 1
            assert got["nonfinite"] == 1 and got["coef"] == 1.0 and got["scale"].tobytes() == np.float32(0.5).tobytes()
            assert got["skipped"] == skipped and not np.isfinite(got["norm"])
            step(A, hb, grad_scale=123.0, zero_grad=zero_grad, state=B.state, skip_nonfinite=True)
            out = host_all(A)
            for k in ("p", "m", "v"):
                assert np.array_equal(out[k], h[k].view(np.int32)), f"{k} changed by a skipped step"
            assert (out["w16"] == np.int16(NAN16)).all()
            g_expect = hb["g"].copy()
            if zero_grad:
                g_expect[counted] = 0.0
            assert np.array_equal(out["g"], g_expect.view(np.int32)), f"g after a skipped step (zero_grad={zero_grad})"
            # without skip_nonfinite the flag changes nothing: unimm_adamw_step's bits, poison and all
            A1, A2 = arena_of(hb), arena_of(hb)
            step(A1, hb, grad_scale=123.0, zero_grad=zero_grad, state=B.state, skip_nonfinite=False)
            step(A2, hb, grad_scale=0.5, zero_grad=zero_grad)
            a, b = host_all(A1), host_all(A2)
            for k in a:
                assert np.array_equal(a[k], b[k]), f"{k}: skip_nonfinite off differs from unimm_adamw_step"
            assert not np.array_equal(a["p"], h["p"].view(np.int32))
    # a clean gradient after the poisoned ones: the flag clears, the counter stays, skip_nonfinite lets the update through
    A = arena_of(h)
    got, _ = norm_pass(A, B, h, 0.5, 1.0)
    assert got["nonfinite"] == 0 and got["skipped"] == skipped
    step(A, h, grad_scale=123.0, state=B.state, skip_nonfinite=True)
    out = host_all(A)
    p_ref, m_ref, _ = oracle_update(h, got["scale"])
    assert np.array_equal(out["m"][counted], m_ref.view(np.int32)[counted])
    assert np.allclose(out["p"].view(np.float32)[counted], p_ref[counted], rtol=1e-6, atol=1e-9)


def test_refusals():
    lib = _lib()
    n = 256
    h = make(n, seed=9, table=np.zeros(n // 64, np.uint8))
    A, B = arena_of(h), Blocks()
    before = host_all(A)
    st0 = B.state.cpu().numpy().tobytes()
    fn = lib.lib().unimm_grad_norm
    ok = dict(g=A.view("g").data_ptr(), group=A.table().data_ptr(), n=n, n_groups=1, grad_scale=1.0, max_norm=1.0,
              ws=B.ws.data_ptr(), ws_n=lib.GRAD_NORM_WS_DOUBLES, st=B.state.data_ptr())

    def rc(**kw):
        a = dict(ok, **kw)
        return fn(a["g"], a["group"], a["n"], a["n_groups"], a["grad_scale"], a["max_norm"], a["ws"], a["ws_n"], a["st"], lib._stream())

    ARG, SHAPE, ALIGN = -1, -2, -3
    assert {lib._ERR[c] for c in (ARG, SHAPE, ALIGN)} == {"UNIMM_E_ARG", "UNIMM_E_SHAPE", "UNIMM_E_ALIGN"}
    for k in ("g", "group", "ws", "st"):
        assert rc(**{k: None}) == ARG, k
    for bad_n in (0, -64, 100, 65):
        assert rc(n=bad_n) == SHAPE, bad_n
    for ng in (0, -1, 9):
        assert rc(n_groups=ng) == ARG, ng
    for mx in (float("nan"), 0.0, -1.0, float("-inf")):
        assert rc(max_norm=mx) == ARG, mx
    assert rc(ws_n=lib.GRAD_NORM_WS_DOUBLES - 1) == ARG
    assert rc(g=A.view("g", off=1).data_ptr()) == ALIGN                          # 4 bytes off
    assert rc(ws=B.ws.data_ptr() + 8) == ALIGN
    assert rc(st=B.state.data_ptr() + 8) == ALIGN
    # the clipped step: the refusals of unimm_adamw_step, and the state pointer
    with pytest.raises(lib.UnimmHipError, match="UNIMM_E_ALIGN"):
        lib.adamw_step(A.view("p", off=1), A.view("g"), A.view("m"), A.view("v"), A.table(), [1e-3], [0.01], 1, clip_state=B.state)
    with pytest.raises(lib.UnimmHipError, match="UNIMM_E_ALIGN"):
        lib.adamw_step(A.view("p"), A.view("g"), A.view("m"), A.view("v"), A.table(), [1e-3], [0.01], 1, clip_state=B.state[1:])
    with pytest.raises(lib.UnimmHipError, match="UNIMM_E_ARG"):
        lib.adamw_step(A.view("p"), A.view("g"), A.view("m"), A.view("v"), A.table(), [1e-3], [0.01], 0, clip_state=B.state)
    a = lib.AdamWArgs()
    a.p, a.g, a.m, a.v = (A.view(k).data_ptr() for k in "pgmv")
    a.w16, a.group = A.view("w16").data_ptr(), A.table().data_ptr()
    a.n, a.n_groups, a.step = n, 1, 1
    a.lr[0], a.weight_decay[0], a.beta1, a.beta2, a.eps, a.grad_scale, a.correct_bias = 1e-3, 0.01, 0.9, 0.999, 1e-6, 1.0, 1
    clipped = lib.lib().unimm_adamw_step_clipped
    assert clipped(C.byref(a), None, 0, lib._stream()) == ARG
    a.n = 0
    assert clipped(C.byref(a), B.state.data_ptr(), 0, lib._stream()) == SHAPE
    after = host_all(A)
    for k in before:
        assert np.array_equal(after[k], before[k]), f"{k} written by a refused call"
    assert B.guards_ok() and B.state.cpu().numpy().tobytes() == st0
    assert (B.ws_buf.view(torch.int64) == NAN64).all(), "workspace written by a refused call"
    # and the same arguments, valid, are accepted
    assert rc() == 0 and rc(max_norm=float("inf")) == 0
    torch.cuda.synchronize()
    assert B.read()[0]["norm"] > 0 and B.guards_ok()
