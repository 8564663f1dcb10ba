"""The shared key/value segment of the fp32-class attention forward (unimm_x3_attn_fwd with unimm_attn_args.ks_*): all six
instantiations of the matrix-instruction kernel, D = 64 / 128 x 4 / 8 / 16 key tiles, through `lib.x3_attn_fwd`.

Cases are built as tests/test_gpu_attention_edges.py builds its SPLICED ones (H = 3, guard rows, loud keys on both sides of
each splice boundary, mask bits set past the key count, NaN-pattern sentinels) and checked
  1. against the fp64 restatement of the launch (oracle/attention_ref.py, `kshared=`), per head and valid row, at the gates the
     unspliced form of the same kernel meets (X3_GATES: out 2e-5, lse 1e-4);
  2. bit for bit -- out, lse and the split planes -- against an UNSPLICED launch over K / V gathered into position order on the
     host with the same masks: the kernel consumes key positions in the same order and chunks either way;
  3. out3 == x3_split(out), planes [hi | lo | hi];
  4. every sentinel bit outside (valid rows x head columns) unchanged, in out, lse and out3;
  5. the refusals, each before any launch."""
import inspect

import numpy as np
import pytest
import torch

from oracle import attention_ref as AR
from tests.test_gpu_attention_edges import (DEV, H, LEAD, GUARD, LONG, NAN16, NAN32, SHORT, X3_GATES, _nan_like, _record, _spliced, build, check,
                                            cyc, packed, reference, sentinel_ok)

pytestmark = pytest.mark.gpu

MID = [1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128]
NAME = "x3m_attn_fwd<%d,%d> spliced"


def _mixed(form, D, Tq, Tk, ins):
    """ks_len = 0 items beside spliced ones, an item of shared rows only (k_len = 0; needs ks_ins = 0), items with no more
    private rows than ks_ins (they carry no segment, as `_spliced` builds them), and two items on the same segment."""
    kl = [5, 0 if ins == 0 else ins, 9, 2, max(ins, 1), 17, 30, 1]
    sl = [0, 21, 23, 0, 0, 33, 34, 40 if ins <= 1 else 0]
    return packed(form, D, Tq, Tk, cyc([1, 2, 17, 31, 32, 33, 37, 63, 64], len(kl)), kl, ks=(sl, ins))


CASES = [
    _spliced(NAME % (64, 4), 64, 64, 64, SHORT, 1, False),
    _spliced(NAME % (64, 8), 64, 64, 128, MID, 1, True),                 # with an `order` permutation
    _spliced(NAME % (64, 16), 64, 64, 256, LONG, 1, False),
    _spliced(NAME % (128, 4), 128, 64, 64, SHORT, 1, False),
    _spliced(NAME % (128, 8), 128, 64, 128, MID, 1, False),
    _spliced(NAME % (128, 16), 128, 64, 256, LONG, 1, False),
    _spliced(NAME % (64, 8) + " ks_ins=0", 64, 64, 128, MID, 0, False),
    _spliced(NAME % (64, 8) + " ks_ins=3", 64, 64, 128, MID, 3, False),
    _mixed(NAME % (64, 4) + " mixed ks_ins=0", 64, 64, 64, 0),
    _mixed(NAME % (128, 8) + " mixed ks_ins=1", 128, 64, 128, 1),
    _mixed(NAME % (64, 16) + " mixed ks_ins=3", 64, 64, 256, 3),
    # the launch shape scoring makes: one 32-row query tile, at most 31 rows: only the first two waves have rows
    packed(NAME % (64, 16) + " Tq=32", 64, 32, 256, [31, 3, 17, 16, 1], [32, 7, 36, 1, 30], ks=([199, 100, 220, 63, 0], 1)),
]


def _i32(x):
    return torch.tensor(np.asarray(x), dtype=torch.int32, device=DEV)


def _buffers(s):
    c, B, HD = s["c"], s["B"], s["HD"]
    cp = HD + 64                                                     # plane stride with pad columns the kernel must not touch
    obuf = _nan_like(s["Rq"], HD + 24, True)
    lse_buf = torch.full((B * H * c.Tq + 64,), NAN32, dtype=torch.int32, device=DEV).view(torch.float32)
    o3buf = _nan_like(s["Rq"], 3 * cp + 16, False)
    return dict(obuf=obuf, lse_buf=lse_buf, o3buf=o3buf, cp=cp)


def _launch(s, bufs, k, v, kvar, kshared, drop=None, with_kvar=True, planes=True):
    from unimm_amd import lib
    c, B, HD, cp = s["c"], s["B"], s["HD"], bufs["cp"]
    q = s["qbuf"].to(DEV)[:, :HD]
    words = torch.from_numpy(s["words"].view(np.int32)).to(DEV)
    order = _i32(s["order"]) if s["order"] is not None else None
    qvar = (_i32(s["q_off"]), _i32(c.ql), None, order)
    out, lse = bufs["obuf"][:, 8:8 + HD], bufs["lse_buf"][:B * H * c.Tq].view(B, H, c.Tq)
    out3 = bufs["o3buf"][:, 8:8 + 3 * cp]
    lib.x3_attn_fwd(q, k, v, out, lse, words, B, H, c.Tq, c.Tk, c.D, s["scale"], s["mq"], s["mb"], drop or lib.NO_DROP, qvar=qvar,
                    kvar=kvar if with_kvar else None, out3=out3 if planes else None, kshared=kshared)


def run_spliced(s):
    HD = s["HD"]
    kbuf = s["kbuf"].to(DEV)
    bufs = _buffers(s)
    _launch(s, bufs, kbuf[:, HD:2 * HD], kbuf[:, 2 * HD:], (_i32(s["k_off"]), _i32(s["c"].kl)),
            (_i32(s["ks_off"]), _i32(s["sl"]), s["ins"]))
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in bufs.items() if k != "cp"}, bufs["cp"]


def run_gathered(s):
    """The same launch without a segment: every item's K / V rows gathered into position order on the host."""
    c, B, HD = s["c"], s["B"], s["HD"]
    rows = [AR.key_rows(b, s["k_off"], c.kl, s["ks_off"], s["sl"], s["ins"]) for b in range(B)]
    goff = LEAD + np.concatenate([[0], np.cumsum(s["nk"])[:-1]]).astype(np.int64)
    g = torch.randn((LEAD + sum(s["nk"]) + GUARD, 2 * HD), generator=torch.Generator().manual_seed(1))
    for b in range(B):
        g[goff[b]:goff[b] + s["nk"][b]] = s["kbuf"][torch.from_numpy(rows[b]), HD:]
    g = g.to(DEV)
    bufs = _buffers(s)
    _launch(s, bufs, g[:, :HD], g[:, HD:], (_i32(goff), _i32(s["nk"])), None)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in bufs.items() if k != "cp"}


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.form)
def test_x3_spliced_forward(c):
    from unimm_amd import lib
    seed = sum(map(ord, c.form)) + 11
    s = build(c, seed, fp32=True)
    B, HD, D = s["B"], s["HD"], c.D
    sl, ins = s["sl"], s["ins"]
    assert all(sl[b] == 0 or c.kl[b] >= ins for b in range(B)), "the position rule needs ks_ins private rows in front of a segment"
    got, cp = run_spliced(s)
    # 1. the fp64 restatement; 4. sentinels of out / lse (check() asserts both)
    ref = reference(s, (0, 0, 1.0), backward=False)
    errs = check(s, got, ref, X3_GATES, backward=False)
    _record(c.form, errs)
    # 2. bit-equal to the unspliced launch over gathered rows
    flat = run_gathered(s)
    for k in ("obuf", "lse_buf", "o3buf"):
        iv = torch.int16 if got[k].dtype == torch.bfloat16 else torch.int32
        assert torch.equal(got[k].view(iv), flat[k].view(iv)), f"{k}: the spliced launch differs from the launch over gathered rows"
    # 3. the split planes are the split of the fp32 result; 4. sentinels of out3
    qrows = np.concatenate([np.arange(s["q_off"][b], s["q_off"][b] + c.ql[b]) for b in range(B)])
    valid = got["obuf"][torch.from_numpy(qrows), 8:8 + HD].contiguous().to(DEV)
    want3 = torch.empty((len(qrows), 3 * HD), dtype=torch.bfloat16, device=DEV)
    lib.x3_split(valid, out3=want3, rows=len(qrows), cols=HD, cp=HD)
    want3 = want3.cpu().view(torch.int16)
    o3 = got["o3buf"].view(torch.int16)
    keep = torch.ones(o3.shape, dtype=torch.bool)
    qr = torch.from_numpy(qrows)
    for p in range(3):
        c0 = 8 + p * cp
        assert torch.equal(o3[qr, c0:c0 + HD], want3[:, p * HD:(p + 1) * HD]), f"plane {p} is not the split of out"
        keep[qr[:, None], torch.arange(c0, c0 + HD)[None, :]] = False
    assert torch.equal(want3[:, :HD], want3[:, 2 * HD:])
    bad = (o3 != NAN16) & keep
    assert not bad.any(), f"out3: {int(bad.sum())} elements outside the valid rows / head columns were written, e.g. {bad.nonzero()[:4].tolist()}"
    n, where = sentinel_ok(got["obuf"], qrows, 8, 8 + HD, NAN32)
    assert n == 0, where


def test_x3_spliced_refusals_leave_outputs_untouched():
    from unimm_amd import lib
    c = _spliced(NAME % (64, 4), 64, 64, 64, SHORT, 1, False)
    s = build(c, 3, fp32=True)
    HD = s["HD"]
    kbuf = s["kbuf"].to(DEV)
    k, v = kbuf[:, HD:2 * HD], kbuf[:, 2 * HD:]
    kvar = (_i32(s["k_off"]), _i32(c.kl))
    ks = (_i32(s["ks_off"]), _i32(s["sl"]), 1)
    bufs = _buffers(s)

    def refused(**kw):
        with pytest.raises(lib.UnimmHipError, match="UNIMM_E_ARG"):
            _launch(s, bufs, k, v, kvar, **kw)

    refused(kshared=ks, drop=(123, 1 << 28, 1.0 / (1 - 1 / 16)))     # a segment with dropout
    refused(kshared=ks, with_kvar=False)                              # a segment without k_off / k_len
    refused(kshared=(ks[0], None, 1))                                 # only one of ks_off / ks_len
    refused(kshared=(None, ks[1], 1))
    refused(kshared=(ks[0], ks[1], -1))                               # ks_ins < 0
    lib.x3_attn_set_impl(0)
    try:
        refused(kshared=ks, planes=False)                             # the vector-ALU kernels have no segment (nor split planes)
    finally:
        lib.x3_attn_set_impl(1)
    torch.cuda.synchronize()
    for name, pat in (("obuf", NAN32), ("lse_buf", NAN32), ("o3buf", NAN16)):
        b = bufs[name].cpu()
        assert bool((b.view(torch.int16 if pat == NAN16 else torch.int32) == pat).all()), f"a refused launch wrote {name}"
    # the backward entry point has no way to pass a segment
    assert not any("shared" in p or p.startswith("ks") for p in inspect.signature(lib.x3_attn_bwd).parameters)
    assert not any(f[0].startswith("ks_") for f in lib.AttnBwdArgs._fields_)
