"""Every form of the bf16 attention kernels (and the fp32-class entry points) against the fp64 restatement of one launch
(oracle/attention_ref.py), in the packed layout production uses, at every tile edge of the lengths.

Each case is named after the kernel form it must reach.  The dispatch (unimm_amd/csrc/attention.hip, unimm_attn_fwd /
unimm_attn_bwd) looks at D and at the PADDED Tq / Tk of the launch:
  forward    D = 64:  attn_fwd<64, 2> when Tk <= 64, else attn_fwd<64, 8>
             D = 128: attn_fwd<128, 2> when Tk <= 64; attn_fwd_fewq128 when Tq <= 64 < Tk and no shared key segment;
                      else attn_fwd<128, 8>
  backward   D = 64, Tq > 64, Tk > 64: attn_bwd_fused<8> (one kernel)
             D = 128, Tq <= 64 < Tk: attn_bwd_fewq128;  D = 128, Tk <= 64 < Tq: attn_bwd_fewk128
             otherwise attn_bwd_dq<D, Tk <= 64 ? 2 : 8> then attn_bwd_dkv<D, Tq <= 64 ? 2 : 8>

Probes that turn an off-by-one into an O(1) error of one row instead of O(1/Tk) of the tensor:
  * loud keys: some query rows of every item are aligned with one K row so that the scaled score is about +12 -- the last
    valid key, the row just past the item (the next item's first row or a guard row), a masked key, and for spliced
    sequences both sides of each splice boundary;
  * mask bits SET where they must be ignored: past k_len in every packed row, past Tk in the last word of a fixed-layout
    row, and on every query row past q_len;
  * outputs, gradients, lse and guard rows start as a NaN bit pattern: every bit outside (valid rows x head columns) and every
    lse entry past q_len must come back unchanged.
Errors are per head and per valid row, relative to the row's own max |ref| floored at 2^-3 of the head's max |ref|."""
import math
from collections import namedtuple

import numpy as np
import pytest
import torch

from oracle import attention_ref as AR

pytestmark = pytest.mark.gpu
DEV = "cuda"

H = 3                                  # odd, so that no head count hides a per-head indexing slip
LONG = [1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 160, 191, 192, 193, 224, 255, 256]
SHORT = [1, 2, 17, 31, 32, 33, 37, 63, 64]
LEAD, GUARD = 5, 40                    # guard rows before the first and after the last item
NAN16, NAN32 = 0x7FA5, 0x7FA5A5A5      # bf16 / fp32 NaN bit patterns of the sentinels
LOUD = 12.0                            # scaled score of a loud key
GATES = dict(out=2 ** -6, dq=2 ** -5, dk=2 ** -5, dv=2 ** -5, lse=1e-3, lse_dead=1e-2,
             dq_exact=2 ** -5, dk_exact=2 ** -5, dv_exact=2 ** -5)
X3_GATES = dict(out=2e-5, dq=5e-5, dk=5e-5, dv=5e-5, lse=1e-4, lse_dead=1e-2, dq_exact=5e-5, dk_exact=5e-5, dv_exact=5e-5)


def cyc(xs, n):
    return (xs * (n // len(xs) + 1))[:n]


# layout "packed": one item per length pair; "fixed": B sequences of Tq / Tk rows.  ks = (shared lengths, ks_ins) or None.
Case = namedtuple("Case", "form D Tq Tk layout ql kl dense order p ks")


def packed(form, D, Tq, Tk, ql, kl, dense=True, order=False, p=0.0, ks=None):
    return Case(form, D, Tq, Tk, "packed", list(ql), list(kl), dense, order, p, ks)


def fixed(form, D, Tq, Tk, B=2, dense=True, p=0.0):
    return Case(form, D, Tq, Tk, "fixed", [Tq] * B, [Tk] * B, dense, False, p, None)


F64_8, F64_2, F128_2, F128_8, FQ = "attn_fwd<64,8>", "attn_fwd<64,2>", "attn_fwd<128,2>", "attn_fwd<128,8>", "attn_fwd_fewq128"
CASES = [
    # D = 64, Tq > 64, Tk > 64: text self-attention
    packed(F64_8 + " + attn_bwd_fused<8>", 64, 256, 256, LONG, LONG, order=True, p=0.1),
    packed(F64_8 + " + attn_bwd_fused<8> (q_len != k_len)", 64, 256, 256, LONG, LONG[::-1]),
    fixed(F64_8 + " + attn_bwd_fused<8>", 64, 193, 193),
    # D = 64, both sides <= 64
    packed(F64_2 + " + dq<64,2> + dkv<64,2>", 64, 64, 64, SHORT, SHORT[::-1], order=True, p=0.1),
    fixed(F64_2 + " + dq<64,2> + dkv<64,2>", 64, 63, 33),
    # D = 64, Tq <= 64 < Tk
    packed(F64_8 + " + dq<64,8> + dkv<64,2>", 64, 64, 256, cyc(SHORT, 21), LONG, order=True, p=0.1),
    fixed(F64_8 + " + dq<64,8> + dkv<64,2>", 64, 33, 97),
    # D = 64, Tk <= 64 < Tq
    packed(F64_2 + " + dq<64,2> + dkv<64,8>", 64, 256, 64, LONG, cyc(SHORT, 21), order=True, p=0.1),
    fixed(F64_2 + " + dq<64,2> + dkv<64,8>", 64, 129, 31),
    # D = 128, Tq <= 64 < Tk: regions attend text
    packed(FQ + " + attn_bwd_fewq128", 128, 64, 256, cyc(SHORT, 21), LONG, order=True, p=0.1),
    fixed(FQ + " + attn_bwd_fewq128", 128, 37, 255),
    # D = 128, Tk <= 64 < Tq: text attends regions (image key-padding mask)
    packed(F128_2 + " + attn_bwd_fewk128", 128, 256, 64, LONG, cyc(SHORT, 21), dense=False, order=True, p=0.1),
    fixed(F128_2 + " + attn_bwd_fewk128", 128, 200, 37, dense=False),
    # D = 128, both sides <= 64: image self-attention
    packed(F128_2 + " + dq<128,2> + dkv<128,2>", 128, 64, 64, SHORT, SHORT, dense=False, order=True, p=0.1),
    fixed(F128_2 + " + dq<128,2> + dkv<128,2>", 128, 33, 33),
    # D = 128, both sides > 64: more than 64 regions
    packed(F128_8 + " + dq<128,8> + dkv<128,8>", 128, 256, 256, LONG, LONG, order=True, p=0.1),
    fixed(F128_8 + " + dq<128,8> + dkv<128,8>", 128, 97, 65),
]


def _spliced(form, D, Tq, Tk, totals, ins, order):
    """k_len + ks_len = each total; the shared part is about half (none when the total leaves no private row past ks_ins)"""
    sl = [max(0, min(t - ins, t // 2)) for t in totals]
    return packed(form, D, Tq, Tk, cyc(SHORT, len(totals)), [t - s for t, s in zip(totals, sl)], order=order, ks=(sl, ins))


SPLICED = [   # forward only (the ABI refuses a shared segment with dropout and has no backward for it); ks_ins = 1 as in scoring
    _spliced(F64_8 + " spliced", 64, 64, 256, LONG, 1, True),
    _spliced(F64_2 + " spliced", 64, 64, 64, SHORT, 1, False),
    _spliced(F128_8 + " spliced (Tq <= 64)", 128, 64, 256, LONG, 1, False),
]


def _record(form, errs):
    print(f"\n{form}: " + "  ".join(f"{k} {v:.2e}" for k, v in sorted(errs.items())))


# ----------------------------------------------------------------------------------------------------------------------
# case builder: host tensors in BUFFER coordinates (LEAD guard rows first, GUARD rows last; the kernels get views)
# ----------------------------------------------------------------------------------------------------------------------
def build(c, seed, fp32=False):
    g = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    B, D, Tq, Tk = len(c.ql), c.D, c.Tq, c.Tk
    HD = H * D
    sl, ins = (c.ks[0], c.ks[1]) if c.ks else ([0] * B, 0)
    nk = [c.kl[b] + sl[b] for b in range(B)]                        # key POSITIONS of each sequence
    assert all(n <= Tk for n in nk) and all(q <= Tq for q in c.ql)
    if c.layout == "packed":
        q_off = LEAD + np.concatenate([[0], np.cumsum(c.ql)[:-1]]).astype(np.int64)
        k_off = LEAD + np.concatenate([[0], np.cumsum(c.kl)[:-1]]).astype(np.int64)
        Rq, Rk = LEAD + sum(c.ql) + GUARD, LEAD + sum(c.kl) + GUARD
        base = 0                                                     # the kernels see the buffers from row 0
    else:
        q_off, k_off = LEAD + Tq * np.arange(B), LEAD + Tk * np.arange(B)
        Rq, Rk = LEAD + B * Tq + GUARD, LEAD + B * Tk + GUARD
        base = LEAD                                                  # the fixed layout starts at the view's row 0
    ks_off = None
    if c.ks:
        ks_off = Rk + (np.arange(B) % 2) * 256                      # two shared segments, as two dialog rounds' contexts
        Rk += 2 * 256 + GUARD
    qbuf = torch.randn((Rq, 3 * HD), generator=g)
    kbuf = torch.randn((Rk, 3 * HD), generator=g)
    if not fp32:
        qbuf, kbuf = qbuf.bfloat16(), kbuf.bfloat16()
    scale = 1.0 / math.sqrt(D)

    def krows(b):
        return AR.key_rows(b, k_off, c.kl, ks_off, sl, ins) if c.ks else np.arange(k_off[b], k_off[b] + c.kl[b])

    # mask bits of key positions 0 .. 32 nw - 1
    nw = (Tk + 31) // 32
    mrows = Tq if c.dense else 1
    bits = rng.random((B, mrows, nw * 32)) < (0.6 if c.dense else 0.8)
    bits[:, :, 0] = True
    if c.layout == "packed":
        for b in range(B):
            bits[b, :, nk[b]:] = True                                # past k_len: set, must be ignored
            if c.dense:
                bits[b, c.ql[b]:, :] = True                          # query rows past q_len: set, must not matter
    else:
        bits[:, :, Tk:] = True                                       # past Tk in the last word
        if c.dense:
            bits[0, Tq // 2:, :Tk] = False                           # fully masked rows (the generative mask's pad rows)

    # loud keys
    for b in range(B):
        nq, kr = c.ql[b], krows(b)
        past = k_off[b] + c.kl[b]                                    # the private row after the item
        want = [("attend", nk[b] - 1, kr[-1]), ("absent", None, past)]
        if nk[b] >= 3:
            want.append(("masked", nk[b] // 2, kr[nk[b] // 2]))
        if c.ks and sl[b] > 0:
            for pos in (ins - 1, ins, ins + sl[b] - 1, ins + sl[b]):
                if 0 <= pos < nk[b]:
                    want.append(("attend", pos, kr[pos]))
        rows = list(dict.fromkeys([0, nq - 1, nq // 2] + list(range(1, nq))))
        for (kind, pos, krow), qi in zip(want, rows):
            if kind != "absent":
                mr = qi if c.dense else 0
                if kind == "masked" and not c.dense and any(w[1] == pos for w in want if w[0] == "attend"):
                    continue
                bits[b, mr, pos] = kind == "attend"
            kk = kbuf[krow, HD:2 * HD].float().reshape(H, D)
            cq = LOUD / (scale * (kk * kk).sum(1, keepdim=True))
            qbuf[q_off[b] + qi, :HD] = (cq * kk).reshape(HD).to(qbuf.dtype)
    words = AR.pack_bits(bits)                                       # [B, mrows, nw]
    mq, mb = (nw if c.dense else 0), mrows * nw

    order = np.argsort(-np.maximum(c.ql, c.kl), kind="stable").astype(np.int32) if c.order else None
    dout_buf = torch.randn((Rq, HD + 16), generator=g).to(qbuf.dtype)
    return dict(c=c, B=B, HD=HD, nk=nk, q_off=q_off, k_off=k_off, Rq=Rq, Rk=Rk, base=base, ks_off=ks_off, sl=sl, ins=ins,
                qbuf=qbuf, kbuf=kbuf, dout_buf=dout_buf, words=words, bits=bits, mq=mq, mb=mb, scale=scale, order=order)


def _drop(c, seed):
    from unimm_amd import dropout as DR
    return DR.drop_arg(c.p, DR.make_key(11, 3, seed))


def _nan_like(rows, cols, fp32):
    if fp32:
        return torch.full((rows, cols), NAN32, dtype=torch.int32, device=DEV).view(torch.float32)
    return torch.full((rows, cols), NAN16, dtype=torch.int16, device=DEV).view(torch.bfloat16)


def run(s, drop, fp32=False, backward=True):
    """One forward (+ backward) launch on the GPU; returns the raw output buffers."""
    from unimm_amd import lib
    c, B, HD, base = s["c"], s["B"], s["HD"], s["base"]
    qbuf, kbuf = s["qbuf"].to(DEV), s["kbuf"].to(DEV)
    q, k, v = qbuf[base:, :HD], kbuf[base:, HD:2 * HD], kbuf[base:, 2 * HD:]
    words = torch.from_numpy(s["words"].view(np.int32)).to(DEV)
    obuf = _nan_like(s["Rq"], HD + 24, fp32)
    lse_buf = torch.full((B * H * c.Tq + 64,), NAN32, dtype=torch.int32, device=DEV).view(torch.float32)
    out, lse = obuf[base:, 8:8 + HD], lse_buf[:B * H * c.Tq].view(B, H, c.Tq)
    qvar = kvar = kshared = None
    if c.layout == "packed":
        def i32(x):
            return torch.tensor(np.asarray(x), dtype=torch.int32, device=DEV)
        order = i32(s["order"]) if s["order"] is not None else None
        qvar = (i32(s["q_off"]), i32(c.ql), None, order)
        kvar = (i32(s["k_off"]), i32(c.kl))
        if c.ks:
            kshared = (i32(s["ks_off"]), i32(s["sl"]), s["ins"])
    fwd = lib.x3_attn_fwd if fp32 else lib.attn_fwd
    kw = dict(qvar=qvar, kvar=kvar) if fp32 else dict(qvar=qvar, kvar=kvar, kshared=kshared)
    fwd(q, k, v, out, lse, words, B, H, c.Tq, c.Tk, c.D, s["scale"], s["mq"], s["mb"], drop, **kw)
    res = dict(obuf=obuf, lse_buf=lse_buf)
    if backward:
        dout = s["dout_buf"].to(DEV)[base:, 16:16 + HD]
        gq, gk = _nan_like(s["Rq"], HD + 24, fp32), _nan_like(s["Rk"], 2 * HD + 32, fp32)
        dq, dk, dv = gq[base:, 8:8 + HD], gk[base:, 8:8 + HD], gk[base:, HD + 24:2 * HD + 24]
        delta = torch.zeros((B, H, c.Tq), device=DEV)
        bwd = lib.x3_attn_bwd if fp32 else lib.attn_bwd
        bwd(q, k, v, out, dout, lse, delta, dq, dk, dv, words, B, H, c.Tq, c.Tk, c.D, s["scale"], s["mq"], s["mb"], drop,
            qvar=qvar, kvar=kvar)
        res.update(gq=gq, gk=gk)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in res.items()}


def reference(s, drop, backward=True, out_arg=None):
    """The fp64 restatement in buffer coordinates.  out_arg: the `out` the backward launch was given (view coordinates): the
    gradients as that launch defines them (dq_bwd, ...: delta = rowsum(dO o out)) next to the exact ones (dq, ...)."""
    c, base = s["c"], s["base"]
    HD = s["HD"]
    qv, kv, vv = s["qbuf"][base:, :HD], s["kbuf"][base:, HD:2 * HD], s["kbuf"][base:, 2 * HD:]
    qvar = kvar = kshared = None
    if c.layout == "packed":
        qvar, kvar = (s["q_off"], c.ql), (s["k_off"], c.kl)
        if c.ks:
            kshared = (s["ks_off"], s["sl"], s["ins"])
    dout = s["dout_buf"][base:, 16:16 + HD] if backward else None
    r = AR.attention(qv, kv, vv, s["words"], B=s["B"], H=H, Tq=c.Tq, Tk=c.Tk, D=c.D, scale=s["scale"], mask_q_stride=s["mq"],
                     mask_b_stride=s["mb"], qvar=qvar, kvar=kvar, kshared=kshared, drop=drop, dout=dout, out_arg=out_arg)
    def pad(t, R):                                                  # back to buffer coordinates
        return torch.cat([torch.zeros((base, HD), dtype=t.dtype), t, torch.zeros((R - base - t.shape[0], HD), dtype=t.dtype)])

    out = dict(out=pad(r["out"], s["Rq"]), lse=r["lse"])
    if backward:
        for k, R in (("dq", s["Rq"]), ("dk", s["Rk"]), ("dv", s["Rk"])):
            out[k] = pad(r[k], R)
            if out_arg is not None:
                out[k + "_bwd"] = pad(r[k + "_bwd"], R)
    return out


def row_errors(got, ref, rows, D):
    """max over the valid rows and heads of max|got - ref| over the head's columns / max(row max|ref|, 2^-3 head max|ref|)"""
    g = got[rows].double().reshape(len(rows), H, D)
    r = ref[rows].double().reshape(len(rows), H, D)
    assert torch.isfinite(g).all(), "non-finite values in valid rows"
    rowmax = r.abs().amax(-1)                                       # [rows, H]
    floor = 2.0 ** -3 * rowmax.amax(0, keepdim=True)
    e = (g - r).abs().amax(-1) / torch.maximum(rowmax, floor).clamp_min(1e-30)
    return float(e.max()), e


def sentinel_ok(buf, rows, c0, c1, pattern):
    """every element outside (rows x columns c0 .. c1 - 1) still holds the sentinel bit pattern"""
    bitsv = buf.view(torch.int16 if buf.dtype == torch.bfloat16 else torch.int32)
    keep = torch.ones(bitsv.shape, dtype=torch.bool)
    keep[torch.as_tensor(rows, dtype=torch.long)[:, None], torch.arange(c0, c1)[None, :]] = False
    bad = (bitsv != pattern) & keep
    return int(bad.sum()), (bad.nonzero()[:4].tolist() if bad.any() else [])


def check(s, got, ref, gates, backward=True):
    c, B, HD, D = s["c"], s["B"], s["HD"], s["c"].D
    qrows = np.concatenate([np.arange(s["q_off"][b], s["q_off"][b] + c.ql[b]) for b in range(B)])
    krows = np.concatenate([np.arange(s["k_off"][b], s["k_off"][b] + c.kl[b]) for b in range(B)])
    fp32 = got["obuf"].dtype == torch.float32
    pat = NAN32 if fp32 else NAN16
    errs = {}
    errs["out"], _ = row_errors(got["obuf"][:, 8:8 + HD], ref["out"], qrows, D)
    n, where = sentinel_ok(got["obuf"], qrows, 8, 8 + HD, pat)
    assert n == 0, f"out: {n} elements outside the valid rows / head columns were written, e.g. {where}"
    # lse: rows that attend a key, fully masked rows, and untouched entries past q_len (and past the tensor)
    lse = got["lse_buf"][:B * H * c.Tq].view(B, H, c.Tq).double()
    lbits = got["lse_buf"].view(torch.int32)
    past = torch.ones((B, H, c.Tq), dtype=torch.bool)
    live = torch.zeros((B, H, c.Tq), dtype=torch.bool)
    for b in range(B):
        past[b, :, :c.ql[b]] = False
        mb = s["bits"][b, :c.ql[b] if c.dense else 1, :s["nk"][b]].any(-1)
        live[b, :, :c.ql[b]] = torch.from_numpy(np.broadcast_to(mb, (c.ql[b],)).copy())[None]
    assert bool((lbits[:B * H * c.Tq].view(B, H, c.Tq)[past] == NAN32).all()), "lse written past q_len"
    assert bool((lbits[B * H * c.Tq:] == NAN32).all()), "lse written past [B, H, Tq]"
    d = (lse - ref["lse"]).abs()
    assert torch.isfinite(lse[~past]).all()
    errs["lse"] = float(d[live].max())
    dead = ~live & ~past
    if dead.any():
        errs["lse_dead"] = float(d[dead].max())
    if backward:
        # per row against the gradients the launch defines (delta from the `out` it is given), and globally (today's gate in
        # tests/test_gpu_kernels.py: max error / max |ref| of the tensor) against the exact ones
        for k, buf, c0, rows in (("dq", "gq", 8, qrows), ("dk", "gk", 8, krows), ("dv", "gk", HD + 24, krows)):
            g = got[buf][:, c0:c0 + HD]
            errs[k], _ = row_errors(g, ref[k + "_bwd"], rows, D)
            errs[k + "_exact"] = float((g[rows].double() - ref[k][rows]).abs().max() / ref[k][rows].abs().max())
        n, where = sentinel_ok(got["gq"], qrows, 8, 8 + HD, pat)
        assert n == 0, f"dq: {n} elements outside the valid rows / head columns were written, e.g. {where}"
        # dk / dv share one buffer: the union of their column ranges is what may change
        gk = got["gk"]
        gkb = gk.view(torch.int16 if not fp32 else torch.int32)
        keep = torch.ones(gkb.shape, dtype=torch.bool)
        kr = torch.as_tensor(krows, dtype=torch.long)[:, None]
        keep[kr, torch.arange(8, 8 + HD)[None, :]] = False
        keep[kr, torch.arange(HD + 24, 2 * HD + 24)[None, :]] = False
        bad = (gkb != pat) & keep
        assert not bad.any(), f"dk / dv: {int(bad.sum())} elements outside the valid rows / head columns were written, " \
                              f"e.g. {bad.nonzero()[:4].tolist()}"
    for k, v in errs.items():
        assert v <= gates[k], (c.form, c.layout, k, v, errs)
    return errs


def _same(a, b):
    for k in a:
        x, y = a[k], b[k]
        iv = torch.int16 if x.dtype == torch.bfloat16 else torch.int32
        if not torch.equal(x.view(iv), y.view(iv)):
            return k
    return None


@pytest.mark.parametrize("c", CASES + SPLICED, ids=lambda c: f"{c.form}|{c.layout}")
def test_attention_form_against_fp64(c):
    seed = sum(map(ord, c.form + c.layout))
    s = build(c, seed)
    drop = _drop(c, seed)
    bwd = c.ks is None
    got = run(s, drop, backward=bwd)
    ref = reference(s, drop, backward=bwd, out_arg=got["obuf"][s["base"]:, 8:8 + s["HD"]] if bwd else None)
    errs = check(s, got, ref, GATES, backward=bwd)
    _record(f"{c.form} [{c.layout}{', p=%g' % c.p if c.p else ''}]", errs)
    again = run(s, drop, backward=bwd)
    assert _same(got, again) is None, f"two identical launches differ in {_same(got, again)}"


# ----------------------------------------------------------------------------------------------------------------------
# unimm_attn_probs
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dense", [True, False])
@pytest.mark.parametrize("Tk", [1, 31, 33, 64, 65, 200, 255, 256])
def test_attention_probs_against_fp64_and_fwd(Tk, dense, D):
    from unimm_amd import dropout as DR
    from unimm_amd import lib
    Tq, B = 33, 2
    c = fixed("attn_probs", D, Tq, Tk, B=B, dense=dense, p=0.1)
    seed = Tk * 7 + D + dense
    s = build(c, seed)
    drop = _drop(c, seed)
    HD, base = s["HD"], s["base"]
    qbuf, kbuf = s["qbuf"].to(DEV), s["kbuf"].to(DEV)
    q, k = qbuf[base:, :HD], kbuf[base:, HD:2 * HD]
    words = torch.from_numpy(s["words"].view(np.int32)).to(DEV)
    n = B * H * Tq * Tk
    pbuf = torch.full((n + 256,), NAN32, dtype=torch.int32, device=DEV).view(torch.float32)
    lib.attn_probs(q, k, pbuf[:n].view(B, H, Tq, Tk), words, B, H, Tq, Tk, D, s["scale"], s["mq"], s["mb"], drop)
    torch.cuda.synchronize()
    pbuf = pbuf.cpu()
    assert bool((pbuf[n:].view(torch.int32) == NAN32).all()), "written past [B, H, Tq, Tk]"
    probs = pbuf[:n].view(B, H, Tq, Tk).double()
    assert torch.isfinite(probs).all()
    ref = reference(s, drop, backward=False)
    rp = AR.attention(s["qbuf"][base:, :HD], s["kbuf"][base:, HD:2 * HD], s["kbuf"][base:, 2 * HD:], s["words"], B=B, H=H,
                      Tq=Tq, Tk=Tk, D=D, scale=s["scale"], mask_q_stride=s["mq"], mask_b_stride=s["mb"], drop=drop)["probs"]
    live = torch.from_numpy(s["bits"][:, :, :Tk].any(-1))                              # [B, rows]
    live = live[:, None, :].expand(B, H, Tq)                                            # (a key mask's one row broadcasts)
    e = (probs - rp).abs().amax(-1) / rp.abs().amax(-1).clamp_min(1e-30)
    errs = {"probs": float(e[live].max())}
    if (~live).any():
        errs["probs_dead"] = float(e[~live].max())
    keep = torch.from_numpy(DR.keep_mask_nd(drop[0], drop[1], (B, H, Tq, Tk)))
    assert bool((probs[~keep] == 0).all()), "a dropped probability is not zero"
    assert bool((probs[keep & (rp > 1e-30)] > 0).all()), "a kept probability is zero"
    # probs @ V in fp64 == the forward with the same dropout key: the two kernels use the same dropout words
    got = run(s, drop, backward=False)
    pv = (probs @ s["kbuf"][base:, 2 * HD:].double()[:B * Tk].reshape(B, Tk, H, D).transpose(1, 2))
    pv = pv.transpose(1, 2).reshape(B * Tq, HD)
    qrows = np.arange(B * Tq)
    errs["probs@V vs fwd"], _ = row_errors(got["obuf"][base:, 8:8 + HD], pv, qrows, D)
    errs["fwd out"], _ = row_errors(got["obuf"][:, 8:8 + HD], ref["out"], qrows + base, D)
    _record(f"attn_probs<{D}> Tk={Tk} {'dense' if dense else 'key'}", errs)
    assert errs["probs"] <= 1e-4 and errs.get("probs_dead", 0.0) <= 4e-3, errs
    assert errs["probs@V vs fwd"] <= GATES["out"] and errs["fwd out"] <= GATES["out"], errs


# ----------------------------------------------------------------------------------------------------------------------
# the fp32 class (unimm_x3_attn_fwd / _bwd): the packed sweep, bits past the lengths, sentinels
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [c for c in CASES if c.layout == "packed"], ids=lambda c: f"D{c.D}-Tq{c.Tq}-Tk{c.Tk}-{c.form}")
def test_fp32_attention_packed_against_fp64(c):
    seed = sum(map(ord, c.form)) + 5
    s = build(c, seed, fp32=True)
    drop = _drop(c, seed)
    got = run(s, drop, fp32=True)
    ref = reference(s, drop, out_arg=got["obuf"][s["base"]:, 8:8 + s["HD"]])
    errs = check(s, got, ref, X3_GATES)
    _record(f"x3 D={c.D} Tq={c.Tq} Tk={c.Tk} [packed{', p=%g' % c.p if c.p else ''}]", errs)
