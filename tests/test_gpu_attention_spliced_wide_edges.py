"""The training pair of the spliced launch for up to 64 private rows (unimm_attn_spliced_wide_fwd / unimm_attn_spliced_wide_bwd)
against the fp64 restatement of one launch (oracle/attention_ref.py with `kshared=`), with the buffer discipline of
tests/test_gpu_attention_spliced_bwd_edges.py: guard rows, NaN-pattern sentinels in every output, Q / K / V and their gradients as
column slices of wider buffers, mask bits set where they must be ignored, loud keys on both sides of each splice boundary and on
both sides of the 32-row boundary of the private keys.

Tq = 64, Tk = 256.  A launch is a list of GROUPS: a shared segment of s rows and members (q_len, k_len, has_segment).  Segment lengths
sit on every 32-key tile edge; 224 and 250 come with members short enough for 256 key positions (250: the wave of the private tiles
owns a shared tile too, and its accumulators are parked while it serves a member of two query tiles, or a member without a
segment that has two private key tiles).  Members mix two-tile and one-tile sequences in one group, with unequal query and key
counts; the members of different groups are interleaved in the batch.

ks_ins = 33 and 40 put the splice inside the second private key tile.  In those launches every member that names a segment has
k_len >= ks_ins: the forward launch takes key positions below ks_ins from the private rows whatever k_len is (as unimm_attn_fwd
always has), so a shorter member has no defined result.

Gates are tests/test_gpu_attention_edges.py's GATES, per head and valid row, on the private rows AND on the shared rows.

What the host cannot see it cannot refuse: k_len lives in device memory.  The kernel clamps it to 64; the last test shows that a
launch with k_len = 65 writes the 64 rows and nothing else."""
import math
from collections import namedtuple

import numpy as np
import pytest
import torch

from oracle import attention_ref as AR
from tests.test_gpu_attention_edges import DEV, GATES, GUARD, LEAD, LOUD, NAN16, NAN32, _nan_like, sentinel_ok
from tests.test_gpu_attention_spliced_bwd_edges import _drop, _i32, _same, row_errors

pytestmark = pytest.mark.gpu

D, TQ, TK = 64, 64, 256
Case = namedtuple("Case", "name groups H ins order p acc")
T, F = True, False


def _seg(*m):
    return [(ql, kl, True) for ql, kl in m]


EDGE_GROUPS = [
    (1, _seg((33, 33), (3, 3))), (31, _seg((34, 34), (17, 17))), (32, _seg((48, 48), (32, 32), (64, 33))),
    (33, _seg((63, 63), (33, 64))), (64, _seg((64, 64), (3, 64), (64, 3))), (191, _seg((64, 64), (17, 17))),
    (192, _seg((64, 64), (3, 3))), (223, _seg((33, 33), (64, 33), (32, 32))), (224, _seg((64, 3), (32, 32), (17, 17))),
    (250, _seg((64, 3), (33, 5), (3, 3)) + [(64, 64, F)]),           # a shared tile on the private wave: its sums are parked
]
MIXED_GROUPS = [
    (33, [(48, 48, T), (3, 3, F), (64, 64, T), (40, 64, F)]),        # members without a segment (ks_len = 0)
    (65, [(34, 50, F)]),                                             # a group whose only member has none: its rows get nothing
    (223, _seg((64, 33))), (1, _seg((64, 64), (3, 3))),
    (64, _seg(*[[(64, 64), (17, 17), (33, 64), (3, 3), (63, 63), (32, 32), (64, 33), (34, 34)][i % 8] for i in range(16)])),
]
DEEP_GROUPS = [                                                      # every segment member has k_len >= 40
    (31, _seg((48, 48), (63, 63))), (64, _seg((64, 64), (33, 64), (3, 64))), (191, _seg((64, 64), (48, 48))),
    (33, _seg((63, 63)) + [(3, 3, F), (17, 17, F)]), (192, _seg((3, 64))),
]
CASES = [
    Case("edges ks_ins=1 order p=0.1", EDGE_GROUPS, 2, 1, True, 0.1, False),
    Case("edges ks_ins=0", EDGE_GROUPS, 2, 0, False, 0.0, False),
    Case("mixed ks_ins=1 accumulate", MIXED_GROUPS, 2, 1, False, 0.0, True),
    Case("mixed ks_ins=0 p=0.1 accumulate order", MIXED_GROUPS, 2, 0, True, 0.1, True),
    Case("deep ks_ins=33 p=0.1", DEEP_GROUPS, 2, 33, False, 0.1, False),
    Case("deep ks_ins=40 accumulate order", DEEP_GROUPS, 2, 40, True, 0.0, True),
    Case("12 heads ks_ins=1 p=0.1", [(33, _seg((48, 48), (3, 3))), (65, _seg((64, 64), (17, 17), (33, 64)))], 12, 1, False, 0.1, False),
]


def build(c, seed):
    g = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    H, HD, ins = c.H, c.H * D, c.ins
    todo = [list(m) for _, m in c.groups]                            # interleave the groups' members: round-robin over the groups
    seqs = []
    while any(todo):
        for gi, t in enumerate(todo):
            if t:
                seqs.append((gi,) + tuple(t.pop(0)))
    B, G = len(seqs), len(c.groups)
    gid, ql, kl, seg = (np.array([s[i] for s in seqs]) for i in range(4))
    s_len = np.array([s for s, _ in c.groups])
    q_off = LEAD + np.concatenate([[0], np.cumsum(ql)[:-1]])
    k_off = LEAD + np.concatenate([[0], np.cumsum(kl)[:-1]])
    Rq = LEAD + int(ql.sum()) + GUARD
    s_off = LEAD + int(kl.sum()) + GUARD + np.concatenate([[0], np.cumsum(s_len + 3)[:-1]])      # 3 guard rows between segments
    Rk = int(s_off[-1] + s_len[-1]) + GUARD
    ks_off = s_off[gid]
    ks_len = np.where(seg, s_len[gid], 0)
    nk = kl + ks_len
    assert (nk <= TK).all() and (ql <= TQ).all() and (kl <= 64).all() and (kl[ks_len > 0] >= ins).all()
    qbuf = torch.randn((Rq, 3 * HD), generator=g).bfloat16()
    kbuf = torch.randn((Rk, 3 * HD), generator=g).bfloat16()
    scale = 1.0 / math.sqrt(D)
    nw = TK // 32
    bits = rng.random((B, TQ, TK)) < 0.6
    bits[:, :, 0] = True
    for b in range(B):
        bits[b, :, nk[b]:] = True                                    # past the keys: set, must be ignored
        bits[b, ql[b]:, :] = True                                    # query rows past q_len: set, must not matter
        if ql[b] >= 3 and b % 2 == 0:
            bits[b, ql[b] - 2, :nk[b]] = False                       # a fully masked row
    for b in range(B):                                               # loud keys
        kr = AR.key_rows(b, k_off, kl, ks_off, ks_len, ins)
        pos_of = lambda i: i if i < ins else i + ks_len[b]           # position of private key i
        want = [(nk[b] - 1, True), (nk[b] // 2, False)]
        if ks_len[b] > 0:
            want += [(pos, True) for pos in (ins - 1, ins, ins + ks_len[b] - 1, ins + ks_len[b]) if 0 <= pos < nk[b]]
        if kl[b] > 32:
            want += [(pos_of(31), True), (pos_of(32), True)]         # the 32-row boundary of the private keys
        skip = ql[b] - 2 if (ql[b] >= 3 and b % 2 == 0) else -1
        rows = [qi for qi in dict.fromkeys([0, ql[b] - 1, ql[b] // 2, min(32, ql[b] - 1), min(31, ql[b] - 1)] + list(range(1, ql[b]))) if qi != skip]
        for (pos, attend), qi in zip(want, rows):
            bits[b, qi, pos] = attend
            kk = kbuf[kr[pos], HD:2 * HD].float().reshape(H, D)
            cq = LOUD / (scale * (kk * kk).sum(1, keepdim=True))
            qbuf[q_off[b] + qi, :HD] = (cq * kk).reshape(HD).bfloat16()
    words = AR.pack_bits(bits)                                       # [B, TQ, nw]
    order = np.argsort(-(ql + nk), kind="stable").astype(np.int32) if c.order else None
    dout_buf = torch.randn((Rq, HD + 16), generator=g).bfloat16()
    seed_kv = (0.5 * torch.randn((Rk, 2 * HD), generator=g)).bfloat16()     # what the shared rows hold before an accumulating launch
    from unimm_amd import lib
    g_first, g_seq = lib.group_lists(gid, G)
    live = np.array([bool(seg[gid == gi].any()) for gi in range(G)])  # groups some member names
    cat = lambda xs: np.concatenate(xs or [np.zeros(0, np.int64)]).astype(np.int64)
    srows = cat([np.arange(s_off[gi], s_off[gi] + s_len[gi]) for gi in range(G) if live[gi]])
    prows = cat([np.arange(k_off[b], k_off[b] + kl[b]) for b in range(B)])
    qrows = cat([np.arange(q_off[b], q_off[b] + ql[b]) for b in range(B)])
    return dict(c=c, B=B, G=G, H=H, HD=HD, ql=ql, kl=kl, nk=nk, q_off=q_off, k_off=k_off, ks_off=ks_off, ks_len=ks_len, Rq=Rq, Rk=Rk,
                qbuf=qbuf, kbuf=kbuf, dout_buf=dout_buf, seed_kv=seed_kv, words=words, bits=bits, nw=nw, scale=scale, order=order,
                g_first=g_first, g_seq=g_seq, srows=srows, prows=prows, qrows=qrows)


def run(s, drop, backward=True, entry="wide"):
    from unimm_amd import lib
    c, B, H, HD = s["c"], s["B"], s["H"], s["HD"]
    qbuf, kbuf = s["qbuf"].to(DEV), s["kbuf"].to(DEV)
    q, k, v = qbuf[:, :HD], kbuf[:, HD:2 * HD], kbuf[:, 2 * HD:]
    words = torch.from_numpy(s["words"].view(np.int32)).to(DEV)
    obuf = _nan_like(s["Rq"], HD + 24, False)
    lse_buf = torch.full((B * H * TQ + 64,), NAN32, dtype=torch.int32, device=DEV).view(torch.float32)
    out, lse = obuf[:, 8:8 + HD], lse_buf[:B * H * TQ].view(B, H, TQ)
    order = _i32(s["order"]) if s["order"] is not None else None
    qvar, kvar = (_i32(s["q_off"]), _i32(s["ql"]), None, order), (_i32(s["k_off"]), _i32(s["kl"]))
    kshared = (_i32(s["ks_off"]), _i32(s["ks_len"]), c.ins)
    if entry == "wide":
        lib.attn_spliced_fwd(q, k, v, out, lse, words, B, H, TQ, TK, D, s["scale"], s["nw"], TQ * s["nw"], drop, qvar, kvar, kshared, wide=True)
    else:
        lib.attn_fwd(q, k, v, out, lse, words, B, H, TQ, TK, D, s["scale"], s["nw"], TQ * s["nw"], drop, qvar=qvar, kvar=kvar, kshared=kshared)
    res = dict(obuf=obuf, lse_buf=lse_buf)
    if backward:
        dout = s["dout_buf"].to(DEV)[:, 16:16 + HD]
        gq, gk = _nan_like(s["Rq"], HD + 24, False), _nan_like(s["Rk"], 2 * HD + 32, False)
        dq, dk, dv = gq[:, 8:8 + HD], gk[:, 8:8 + HD], gk[:, HD + 24:2 * HD + 24]
        if c.acc:
            sr = torch.from_numpy(s["srows"]).to(DEV)
            sk = s["seed_kv"].to(DEV)
            dk[sr] = sk[sr, :HD]
            dv[sr] = sk[sr, HD:]
        lib.attn_spliced_bwd(q, k, v, out, dout, lse, dq, dk, dv, words, B, H, TQ, TK, D, s["scale"], s["nw"], TQ * s["nw"], drop,
                             qvar, kvar, kshared, (_i32(s["g_first"]), _i32(s["g_seq"])), accumulate=c.acc, wide=True)
        res.update(gq=gq, gk=gk)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in res.items()}


def reference(s, drop, out_arg):
    c, HD = s["c"], s["HD"]
    r = AR.attention(s["qbuf"][:, :HD], s["kbuf"][:, HD:2 * HD], s["kbuf"][:, 2 * HD:], s["words"], B=s["B"], H=s["H"], Tq=TQ, Tk=TK, D=D,
                     scale=s["scale"], mask_q_stride=s["nw"], mask_b_stride=TQ * s["nw"], qvar=(s["q_off"], s["ql"]),
                     kvar=(s["k_off"], s["kl"]), kshared=(s["ks_off"], s["ks_len"], c.ins), drop=drop,
                     dout=s["dout_buf"][:, 16:16 + HD], out_arg=out_arg)
    if c.acc:                                                        # the rows held these values: they are part of the one rounding
        sr = torch.from_numpy(s["srows"])
        sk = s["seed_kv"].double()
        for key, cols in (("dk", slice(0, HD)), ("dv", slice(HD, 2 * HD))):
            for suf in ("", "_bwd"):
                r[key + suf] = r[key + suf].clone()
                r[key + suf][sr] += sk[sr, cols]
    return r


def check(s, got, ref):
    c, B, H, HD = s["c"], s["B"], s["H"], s["HD"]
    qrows, krows = s["qrows"], np.concatenate([s["prows"], s["srows"]])
    errs = {"out": row_errors(got["obuf"][:, 8:8 + HD], ref["out"], qrows, H)}
    n, where = sentinel_ok(got["obuf"], qrows, 8, 8 + HD, NAN16)
    assert n == 0, f"out: {n} elements outside the valid rows / head columns were written, e.g. {where}"
    lse = got["lse_buf"][:B * H * TQ].view(B, H, TQ).double()
    lbits = got["lse_buf"].view(torch.int32)
    past = torch.ones((B, H, TQ), dtype=torch.bool)
    live = torch.zeros((B, H, TQ), dtype=torch.bool)
    for b in range(B):
        past[b, :, :s["ql"][b]] = False
        live[b, :, :s["ql"][b]] = torch.from_numpy(s["bits"][b, :s["ql"][b], :s["nk"][b]].any(-1))[None]
    assert bool((lbits[:B * H * TQ].view(B, H, TQ)[past] == NAN32).all()), "lse written past q_len"
    assert bool((lbits[B * H * TQ:] == NAN32).all()), "lse written past [B, H, Tq]"
    d = (lse - ref["lse"]).abs()
    errs["lse"] = float(d[live].max())
    dead = ~live & ~past
    if dead.any():
        errs["lse_dead"] = float(d[dead].max())
    gk = got["gk"]
    for k, g, rows in (("dq", got["gq"][:, 8:8 + HD], qrows), ("dk", gk[:, 8:8 + HD], krows), ("dv", gk[:, HD + 24:2 * HD + 24], krows)):
        errs[k] = row_errors(g, ref[k + "_bwd"], rows, H)
        errs[k + "_exact"] = float((g[rows].double() - ref[k][rows]).abs().max() / ref[k][rows].abs().max())
    if len(s["srows"]):                                              # the shared rows on their own: no wider gate
        errs["dk_shared"] = row_errors(gk[:, 8:8 + HD], ref["dk_bwd"], s["srows"], H)
        errs["dv_shared"] = row_errors(gk[:, HD + 24:2 * HD + 24], ref["dv_bwd"], s["srows"], H)
    n, where = sentinel_ok(got["gq"], qrows, 8, 8 + HD, NAN16)
    assert n == 0, f"dq: {n} elements outside the valid rows / head columns were written, e.g. {where}"
    gkb = gk.view(torch.int16)
    keep = torch.ones(gkb.shape, dtype=torch.bool)
    kr = torch.as_tensor(krows, dtype=torch.long)[:, None]
    keep[kr, torch.arange(8, 8 + HD)[None, :]] = False
    keep[kr, torch.arange(HD + 24, 2 * HD + 24)[None, :]] = False
    bad = (gkb != NAN16) & keep
    assert not bad.any(), f"dk / dv: {int(bad.sum())} elements outside the valid rows / head columns were written, e.g. {bad.nonzero()[:4].tolist()}"
    print(f"\n{c.name}: " + "  ".join(f"{k} {v:.2e}" for k, v in sorted(errs.items())))
    gates = dict(GATES, dk_shared=GATES["dk"], dv_shared=GATES["dv"])
    for k, v in errs.items():
        assert v <= gates[k], (c.name, k, v, errs)
    return errs


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_wide_pair_against_fp64(c):
    seed = sum(map(ord, c.name))
    s = build(c, seed)
    drop = _drop(c, seed)
    got = run(s, drop)
    ref = reference(s, drop, got["obuf"][:, 8:8 + s["HD"]])
    check(s, got, ref)
    again = run(s, drop)
    assert _same(got, again) is None, f"two identical launches differ in {_same(got, again)}"


def test_wide_fwd_equals_attn_fwd_without_dropout():
    s = build(CASES[1], 5)
    a, b = run(s, (0, 0, 1.0), backward=False), run(s, (0, 0, 1.0), backward=False, entry="plain")
    assert _same(a, b) is None, f"unimm_attn_spliced_wide_fwd and unimm_attn_fwd differ in {_same(a, b)}"


def _refusal_setup():
    H, HD, B = 2, 2 * D, 2
    qkv = torch.randn((160, 3 * HD + 8), device=DEV).bfloat16()
    dout = torch.randn((160, HD), device=DEV).bfloat16()
    words = torch.full((B, TQ, 8), -1, dtype=torch.int32, device=DEV)
    return H, HD, B, qkv, dout, words


def test_refusals_write_nothing():
    from unimm_amd import lib
    H, HD, B, qkv, dout, words = _refusal_setup()
    q, k, v = qkv[:, :HD], qkv[:, HD:2 * HD], qkv[:, 2 * HD:3 * HD]
    qv, kv = (_i32([0, 70]), _i32([40, 4])), (_i32([0, 70]), _i32([40, 4]))
    ks, gr = (_i32([140, 140]), _i32([20, 20]), 1), (_i32([0, 1, 2]), _i32([0, 1]))
    bufs = {}

    def fresh():
        bufs.update(out=_nan_like(160, HD, False), gq=_nan_like(160, HD, False), gk=_nan_like(160, HD, False), gv=_nan_like(160, HD, False),
                    lse=torch.full((B, H, TQ), NAN32, dtype=torch.int32, device=DEV).view(torch.float32))
        return bufs

    def untouched():
        torch.cuda.synchronize()
        return all(bool((t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32) == (NAN16 if t.dtype == torch.bfloat16 else NAN32)).all())
                   for t in bufs.values())

    def fwd(code, q=q, lse=True, Tq=TQ, Tk=TK, Dh=D, qv=qv, kv=kv, ks=ks):
        b = fresh()
        with pytest.raises(lib.UnimmHipError, match=code):
            lib.attn_spliced_fwd(q, k, v, b["out"], b["lse"] if lse else None, words, B, H, Tq, Tk, Dh, 0.125, 8, TQ * 8, (0, 0, 1.0), qv, kv, ks,
                                 wide=True)
        assert untouched(), code

    def bwd(code, q=q, Tq=TQ, Tk=TK, Dh=D, kv=kv, ks=ks, gr=gr, dk=None):
        b = fresh()
        lse = torch.zeros((B, H, TQ), device=DEV)
        with pytest.raises(lib.UnimmHipError, match=code):
            lib.attn_spliced_bwd(q, k, v, dout, dout, lse, b["gq"], b["gk"] if dk is None else dk, b["gv"], words, B, H, Tq, Tk, Dh, 0.125, 8,
                                 TQ * 8, (0, 0, 1.0), qv, kv, ks, gr, wide=True)
        assert untouched(), code

    for f in (fwd, bwd):
        f("UNIMM_E_ARG", Dh=128)
        f("UNIMM_E_ARG", Tq=65)                                      # more than 64 private rows
        f("UNIMM_E_ARG", Tq=0)
        f("UNIMM_E_ARG", Tk=257)
        f("UNIMM_E_ARG", ks=(ks[0], ks[1], -1))
        f("UNIMM_E_ARG", ks=(None, None, 1))
        f("UNIMM_E_ARG", kv=None)
        f("UNIMM_E_ALIGN", q=qkv[:, 4:4 + HD])                       # 8-byte aligned base
    fwd("UNIMM_E_ARG", lse=False)
    fwd("UNIMM_E_ARG", qv=None)
    bwd("UNIMM_E_ARG", gr=(None, None))
    bwd("UNIMM_E_ARG", gr=(_i32([0]), gr[1]))                        # no group
    bwd("UNIMM_E_ALIGN", dk=_nan_like(160, HD + 4, False)[:, :HD])   # row stride not a multiple of 8


def test_k_len_65_is_clamped_to_64_rows():
    """k_len is device data: the launch cannot be refused on the host.  The backward takes the first 64 private rows and writes
    dk / dv of exactly those (finite values), dq of the q_len rows, and nothing else."""
    from unimm_amd import lib
    H, HD, B, qkv, dout, words = _refusal_setup()
    q, k, v = qkv[:, :HD], qkv[:, HD:2 * HD], qkv[:, 2 * HD:3 * HD]
    qv, kv = (_i32([0, 70]), _i32([40, 4])), (_i32([0, 70]), _i32([65, 4]))
    ks, gr = (_i32([140, 150]), _i32([10, 10]), 1), (_i32([0, 1, 2]), _i32([0, 1]))
    gq, gk, gv = (_nan_like(160, HD, False) for _ in range(3))
    lse = torch.zeros((B, H, TQ), device=DEV)
    lib.attn_spliced_bwd(q, k, v, dout, dout, lse, gq, gk, gv, words, B, H, TQ, TK, D, 0.125, 8, TQ * 8, (0, 0, 1.0), qv, kv, ks, gr, wide=True)
    torch.cuda.synchronize()
    krows = np.concatenate([np.arange(0, 64), np.arange(70, 74), np.arange(140, 160)])
    for t in (gk, gv):
        n, where = sentinel_ok(t.cpu(), krows, 0, HD, NAN16)
        assert n == 0, where
        assert bool(torch.isfinite(t[torch.from_numpy(krows).to(DEV)].float()).all())
    n, where = sentinel_ok(gq.cpu(), np.concatenate([np.arange(0, 40), np.arange(70, 74)]), 0, HD, NAN16)
    assert n == 0, where
