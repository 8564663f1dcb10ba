"""The kernels that decide what the arithmetic kernels see -- mask packing / synthesis, the step plan, casts, transposes, region
packing, column sums and the fp32x3 operand makers -- per element at their edges, in the conventions of
tests/test_gpu_row_edges.py: every output starts as a sentinel NaN bit pattern with extra rows / columns / words behind it
that must come back unchanged, integer results are compared for equality with a restatement (np.packbits, DialogMaskSpec.dense,
oracle/plan_ref.py), float results bit for bit with the CPU's own rounding or per element against float64, and every check
prints "bit-exact" or its worst ratio next to its gate.

Gates.  Everything is bit-exactness except:
  * unimm_colsum: per column |got - (db0 + sum_m dy)| <= (M + 8) 2^-24 (|db0| + sum_m |dy|): the plain fp32 summation bound (the
    atomics make the order free), against the float64 sum of the bf16 inputs;
  * unimm_x3_layernorm_fwd y32: the gate and the offset allowance of test_layernorm_fwd_wave_grid (nothing new);
  * unimm_x3_split GELU / MUL_DGELU: per element, |err| / (2^-24 max(|ref|, 2^-10 row max |ref|)), MEASURED (see SPLIT_GATES).

The split of a value is DEFINED as hi = bf16_rne(y), lo = bf16_rne(y - float(hi)), formed on the CPU from the kernel's own fp32
result; planes are [hi | lo | hi] (x-type) or [hi | hi | lo] (w-type)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from oracle import plan_ref as PR
from oracle import rows_ref as RR
from tests.test_gpu_row_edges import (CONST, DEV, NAN16, NAN32, U, bits, f64, ln_gamma_beta, ln_rows, offset_allowance, sent16,
                                      sent32, untouched)

pytestmark = pytest.mark.gpu

SENT64 = 0x7FA5A5A57FA5A5A5


def rup(x, m):
    return (x + m - 1) // m * m


def gate(name, ratios, limit):
    """the printer of tests/test_gpu_row_edges.py: worst ratio next to its gate, then the assertion"""
    r = np.asarray(ratios, np.float64).reshape(-1)
    lim = np.broadcast_to(np.asarray(limit, np.float64), r.shape)
    if r.size == 0:
        return
    bad = ~(r <= lim)
    i = int(np.argmax(r))
    print(f"[prep-edges] {name}: worst {r[i]:.3g} (gate {lim[i]:.3g})")
    assert not bad.any(), (name, int(np.argmax(bad)), float(r[np.argmax(bad)]), float(lim[np.argmax(bad)]))


def exact(name, ok=True):
    assert bool(np.all(ok)), name
    print(f"[prep-edges] {name}: bit-exact")


def sent_i32(n):
    return torch.full((n,), NAN32, dtype=torch.int32, device=DEV)


def sent_i64(n):
    return torch.full((n,), SENT64, dtype=torch.int64, device=DEV)


def from_bits32(words):
    return torch.from_numpy(np.asarray(words, dtype=np.uint32).view(np.float32).copy())


def bf16_bits_cpu(t):
    """bits of tensor.bfloat16() formed on the CPU (round to nearest even)"""
    return t.detach().cpu().float().bfloat16().contiguous().view(torch.int16).numpy()


def isnan16(v):
    v = np.asarray(v).view(np.uint16)
    return (v & np.uint16(0x7FFF)) > np.uint16(0x7F80)


def same_bf16(got, want):
    """bf16 bit patterns equal; where the CPU's conversion gives a NaN (its bits depend on which of torch's code paths ran:
    0x7FC0 or 0xFFFF), any NaN"""
    return (got == want) | (isnan16(want) & isnan16(got))


def split_def(y32):
    """the definition of the split, on the CPU: (hi bits, lo bits) of an fp32 tensor"""
    y = y32.detach().cpu().float()
    hi = y.bfloat16()
    lo = (y - hi.float()).bfloat16()
    return hi.contiguous().view(torch.int16).numpy(), lo.contiguous().view(torch.int16).numpy()


# fp32 bit patterns at the edges of the bf16 rounding: ties in both directions (to even: down / up), just off a tie, +-0,
# subnormals (incl. ties among them), the largest finite values (which round to bf16 inf), +-inf and the canonical NaN
CAST_EDGES = [0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F808001, 0x3F807FFF, 0xBF808001, 0x3F817FFF,
              0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00008000, 0x00018000, 0x00008001,
              0x00800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF, 0xFF7F8000, 0x7F800000, 0xFF800000, 0x7FC00000]


def with_edges(x, edges=CAST_EDGES, finite=False):
    """a flat fp32 tensor with the edge patterns written over its head and its tail (every third element when it is short)"""
    e = np.asarray(edges, np.uint32)
    if finite:
        e = e[(e & 0x7F800000) != 0x7F800000]
    flat = x.reshape(-1).numpy().view(np.uint32)
    n = flat.size
    if n <= 4 * len(e):
        idx = np.arange(0, n, 3)
        flat[idx] = e[np.arange(len(idx)) % len(e)]
    else:
        flat[:len(e)] = e
        flat[n - len(e):] = e[::-1]
    return x


# ----------------------------------------------------------------------------------------------
# A. mask_pack
# ----------------------------------------------------------------------------------------------
def mask_values(dtype, shape, rng):
    if dtype == torch.bool:
        return torch.from_numpy(rng.random(shape) < 0.5)
    if dtype == torch.uint8:
        vals = np.asarray([0, 0, 1, 2, 255], np.uint8)
    elif dtype == torch.int32:
        vals = np.asarray([0, 0, 0, 1, -1, -2 ** 31], np.int32)
    elif dtype == torch.int64:
        vals = np.asarray([0, 0, 0, 0, 1, -1, 1 << 32, 1 << 40], np.int64)      # the last two: zero low word
    else:
        vals = np.asarray([0x00000000, 0x80000000, 0x00000000, 0x80000000, 0x3F800000, 0x00000001, 0x7FC00000, 0xFF800000],
                          np.uint32).view(np.float32)                             # 0, -0 = "not attend"; 1, 1e-45, NaN, -inf = "attend"
    return torch.from_numpy(vals[rng.integers(0, len(vals), shape)])


def packed_want(m):
    """np.packbits(m != 0), 32 columns per little-endian word"""
    a = m.numpy()
    nz = a if a.dtype == np.bool_ else (a != 0)
    rows, t = nz.shape
    padded = np.zeros((rows, rup(t, 32)), np.uint8)
    padded[:, :t] = nz
    return np.packbits(padded.reshape(rows, -1, 32), axis=-1, bitorder="little").view(np.uint32)[..., 0].view(np.int32)


@pytest.mark.parametrize("dtype", [torch.bool, torch.uint8, torch.int32, torch.int64, torch.float32], ids=str)
def test_mask_pack_values_shapes_and_host_packer(dtype):
    """Every element type with values other than 0 / 1; t on both sides of the 32- and 64-column edges (ballot kernel when
    t % 64 == 0, with 1, 3 and 5 wave groups -- no multiple of the 4 waves of a workgroup; generic kernel otherwise); one case of
    16,400 groups (> 4096 workgroups x 4 waves: the ballot kernel's grid-stride loop); the host packer on the same arrays."""
    from unimm_amd import lib
    rng = np.random.default_rng(11)
    shapes = [(rows, t) for t in (1, 31, 32, 33, 63, 64, 65, 96, 128, 192, 255, 256) for rows in (1, 3, 5)] + [(4100, 256)]
    for rows, t in shapes:
        m = mask_values(dtype, (rows, t), rng)
        want = packed_want(m)
        nw = want.shape[1]
        out = sent_i32(rows * nw + 9)
        lib.mask_pack(m.to(DEV), out=out)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.array_equal(got[:rows * nw].reshape(rows, nw), want), (dtype, rows, t)
        assert (got[rows * nw:] == NAN32).all(), ("words past the end", dtype, rows, t)
        host = lib.host_mask_pack(m).numpy()
        assert np.array_equal(host, want), ("host packer", dtype, rows, t)
    exact(f"mask_pack {dtype} ({len(shapes)} shapes, device and host)")


# ----------------------------------------------------------------------------------------------
# B. mask_synth
# ----------------------------------------------------------------------------------------------
def synth_check(T, descs):
    from unimm_amd import lib
    from unimm_amd.inputs import DialogMaskSpec
    mode, Ls, ns = (list(c) for c in zip(*descs))
    spec = DialogMaskSpec(mode, Ls, ns)
    B, nw = len(spec), (T + 31) // 32
    dm, dl, dn = spec.to_device(DEV)
    tw, cw = sent_i32(B * T * nw + 7), sent_i32(B * nw + 7)
    rc = lib.lib().unimm_mask_synth(lib._ptr(dm), lib._ptr(dl), lib._ptr(dn), lib._ptr(tw), lib._ptr(cw), C.c_int32(B), C.c_int32(T),
                                    lib._stream())
    assert rc == 0
    dt, dc = spec.dense(T)
    want_t = lib.mask_pack(dt.to(DEV)).reshape(-1)
    want_c = lib.mask_pack(dc.to(DEV)).reshape(-1)
    torch.cuda.synchronize()
    assert torch.equal(tw[:B * T * nw], want_t), ("text words", T)
    assert torch.equal(cw[:B * nw], want_c), ("co-attention words", T)
    assert (tw[B * T * nw:] == NAN32).all() and (cw[B * nw:] == NAN32).all()
    if T % 32:
        last_t = tw[:B * T * nw].reshape(B * T, nw)[:, -1].cpu().numpy().view(np.uint32)
        last_c = cw[:B * nw].reshape(B, nw)[:, -1].cpu().numpy().view(np.uint32)
        assert not (last_t >> np.uint32(T % 32)).any() and not (last_c >> np.uint32(T % 32)).any(), "bits at or past T"
    exact(f"mask_synth T={T} ({B} descriptors)")


@pytest.mark.parametrize("T", [33, 64])
def test_mask_synth_exhaustive(T):
    """Both modes, every L in 1..T, every n in 1..L-1 for generative sequences (L + n > T: the copy block is cut at T);
    discriminative ones with n = 0 and with a nonzero n, which must be ignored."""
    descs = [(1, L, n) for L in range(1, T + 1) for n in range(1, L)]
    descs += [(0, L, n) for L in range(1, T + 1) for n in (0, 5)]
    synth_check(T, descs)


def test_mask_synth_last_word_at_256():
    Ls = (1, 2, 31, 32, 33, 224, 225, 255, 256)
    descs = [(1, L, n) for L in Ls for n in sorted({1, 2, 31, 32, 33, L - 1}) if 1 <= n < L]
    descs += [(0, L, n) for L in Ls for n in (0, 33)]
    synth_check(256, descs)


# ----------------------------------------------------------------------------------------------
# C. plan_lengths / plan_build against oracle/plan_ref.py
# ----------------------------------------------------------------------------------------------
def plan_case(B, T, R, text_kind, co_kind, use_w, seed, labelled=True, image=True):
    """Dense inputs of one batch.  text_kind / co_kind: "dense", "row" (query stride 0) or None.  Lengths come from a small
    set (many ties for the rank sort); sequences 1.. carry the hostile kinds when the batch has 8 sequences or more:
      b % 7 == 1: nothing valid at all;  == 2: valid only through a co-attention bit;  == 3: valid only through a label at T - 1;
      == 4: a valid token whose own dense mask row is empty.
    Labels sit inside the prefix: 5 per sequence, four weighted (1, -1, 1, -1), one labelled with weight 0, and one weighted
    row (2) with label -1."""
    rng = np.random.default_rng(seed)
    pool = sorted({1, max(1, T // 3), max(1, T // 2), max(1, T - 1), T})
    n_true = rng.choice(pool, size=B)
    text = np.zeros((B, T, T), bool) if text_kind == "dense" else (np.zeros((B, T), bool) if text_kind == "row" else None)
    co = None
    if co_kind is not None and R > 0:
        co = np.zeros((B, R, T), bool) if co_kind == "dense" else np.zeros((B, T), bool)
    labels = np.full((B, T), -1, np.int64)
    weights = np.zeros((B, T), np.int64)
    for b in range(B):
        n = int(n_true[b])
        kind = b % 7 if B >= 8 else int(b == 1 and B >= 5)        # small batches: one empty sequence, the rest ordinary
        if kind == 4:
            n = max(n, min(T, 3))
        if kind == 1:
            continue
        if kind == 2 and co is not None:
            p = int(rng.integers(0, T))
            if co.ndim == 3:
                co[b, int(rng.integers(0, R)), p] = True
            else:
                co[b, p] = True
            continue
        if kind == 3:
            labels[b, T - 1] = 11
            weights[b, T - 1] = 1
            continue
        if text is not None and text.ndim == 3:
            text[b, :n, :n] = rng.random((n, n)) < 0.5
            text[b, np.arange(n), np.arange(n)] = True                # no empty row inside the prefix ...
            if kind == 4 and n >= 2:
                j = int(rng.integers(1, n))
                text[b, j, :] = False                                 # ... except this one, which token 0 still attends
                text[b, 0, j] = True
        elif text is not None:
            text[b, :n] = rng.random(n) < 0.8
            text[b, n - 1] = True
        if co is not None:
            k = max(1, n - 3)
            if co.ndim == 3:
                co[b, :, :k] = rng.random((R, k)) < 0.3
            else:
                co[b, :k] = rng.random(k) < 0.5
        if text is None and co is None:
            labels[b, n - 1] = 5                                      # the prefix exists through a label alone
            weights[b, n - 1] = 1
        pos = rng.permutation(n)[:5]
        labels[b, pos] = rng.integers(0, 1000, len(pos))
        weights[b, pos[:4]] = np.asarray([1, -1, 1, -1])[:len(pos[:4])]
        if n >= 7:
            weights[b, rng.permutation(n)[0]] = 2                     # weighted, possibly with label -1
    il = rng.integers(-1, 2, (B, max(R, 1))).astype(np.int64)[:, :R] if (image and R > 0) else None
    if not labelled:
        labels[:], weights[:] = -1, 0
    return dict(B=B, T=T, R=R, text=text, co=co, labels=labels, weights=weights if use_w else None, il=il)


def dev_lengths(c, nsp=None, with_labels=True):
    """unimm_plan_lengths through the C ABI on a sentinel-filled header with guard words behind it"""
    from unimm_amd import lib
    B, T, R = c["B"], c["T"], c["R"]
    nw = (T + 31) // 32
    t_arg, c_arg = (None, 0, 0), (None, 0, 0)
    if c["text"] is not None:
        tw = lib.mask_pack(torch.from_numpy(c["text"]).to(DEV))
        t_arg = (tw, nw, T * nw) if c["text"].ndim == 3 else (tw, 0, nw)
    if c["co"] is not None:
        cw = lib.mask_pack(torch.from_numpy(c["co"]).to(DEV))
        c_arg = (cw, nw, R * nw) if c["co"].ndim == 3 else (cw, 0, nw)
    lab32 = torch.from_numpy(c["labels"]).to(torch.int32).to(DEV) if with_labels else None
    w32 = torch.from_numpy(c["weights"]).to(torch.int32).to(DEV) if (c["weights"] is not None and with_labels) else None
    il32 = torch.from_numpy(c["il"]).to(torch.int32).contiguous().to(DEV) if c["il"] is not None else None
    nspd = torch.tensor(nsp, dtype=torch.float32).to(DEV) if nsp is not None else None
    header = sent_i32(3 * B + 2 + 8)
    P, I = lib._ptr, C.c_int32
    rc = lib.lib().unimm_plan_lengths(P(t_arg[0]), I(t_arg[1]), I(t_arg[2]), P(c_arg[0]), I(c_arg[1]), I(c_arg[2]), I(R), P(lab32),
                                      P(w32), P(nspd), P(il32), I(B), I(T), P(header), lib._stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return header, lab32, w32


def ref_header(c, nsp=None, with_labels=True):
    return PR.lengths(c["text"], c["co"], c["labels"] if with_labels else None, c["weights"] if with_labels else None, c["il"],
                      c["B"], c["T"], nsp_weight=nsp)


def check_header(c, header, nsp=None, with_labels=True):
    B = c["B"]
    got = header.cpu().numpy()
    want = ref_header(c, nsp, with_labels)
    if nsp is None:
        assert (got[2 * B:2 * B + 2] == NAN32).all(), "NSP words must be left as the caller set them when nsp_weight is NULL"
        got = got.copy()
        got[2 * B:2 * B + 2] = 0
    assert np.array_equal(got[:3 * B + 2], want), ("header", got[:3 * B + 2].tolist(), want.tolist())
    assert (got[3 * B + 2:] == NAN32).all(), "words behind the header"
    return want


GUARD = 16
LISTS32 = ("off", "lens", "order", "lm_pos", "lm_idx", "lm_label", "lm_weight", "dims_i")


def dev_build(header, lab32, w32, B, T, rows_cap, lm_cap, want_rows=True, want_lm=True, expect_rc=0):
    """unimm_plan_build through the C ABI; every list is sentinel-filled and GUARD entries longer than its capacity"""
    from unimm_amd import lib
    o = dict(off=sent_i32(B + GUARD), lens=sent_i32(B + GUARD), order=sent_i32(B + GUARD), dims_i=sent_i32(4 + GUARD),
             dims_f=sent32(2 + GUARD), rows=None, inv=None, lm_pos=None, lm_idx=None, lm_label=None, lm_weight=None)
    if want_rows:
        o["rows"], o["inv"] = sent_i64(max(rows_cap, 0) + GUARD), sent_i64(B * T + GUARD)
    if want_lm:
        for k in ("lm_pos", "lm_idx", "lm_label", "lm_weight"):
            o[k] = sent_i32(max(lm_cap, 0) + GUARD)
    P, I = lib._ptr, C.c_int32
    rc = lib.lib().unimm_plan_build(P(header), P(lab32), P(w32), I(B), I(T), P(o["off"]), P(o["lens"]), P(o["rows"]), P(o["inv"]),
                                    P(o["lm_pos"]), P(o["lm_idx"]), P(o["lm_label"]), P(o["lm_weight"]), I(rows_cap), I(lm_cap),
                                    P(o["dims_i"]), P(o["dims_f"]), P(o["order"]), lib._stream())
    assert rc == expect_rc, (rc, expect_rc)
    torch.cuda.synchronize()
    out = {k: (v.cpu().numpy() if v is not None else None) for k, v in o.items()}
    out["dims_f"] = out["dims_f"].view(np.int32)                     # compared as bit patterns
    return out


def sizes(B, T, rows_cap, lm_cap):
    return dict(off=B, lens=B, order=B, dims_i=4, dims_f=2, rows=rows_cap, inv=B * T, lm_pos=lm_cap, lm_idx=lm_cap, lm_label=lm_cap,
                lm_weight=lm_cap)


def guards_intact(name, got, B, T, rows_cap, lm_cap):
    for k, n in sizes(B, T, rows_cap, lm_cap).items():
        if got[k] is not None:
            s = SENT64 if got[k].dtype == np.int64 else NAN32
            assert (got[k][n:] == s).all() and len(got[k]) == n + GUARD, (name, "sentinels behind", k)


def check_fit(name, got, want, B, T, rows_cap, lm_cap):
    """a plan that fits its capacities equals the restatement entry for entry (tails of surplus capacity included)"""
    guards_intact(name, got, B, T, rows_cap, lm_cap)
    for k, n in sizes(B, T, rows_cap, lm_cap).items():
        if want[k] is None:
            assert got[k] is None
            continue
        w = want[k].view(np.int32) if k == "dims_f" else want[k]
        assert np.array_equal(got[k][:n], w), (name, k, got[k][:n].tolist()[:40], w.tolist()[:40])


def check_short(name, got, B, T, rows_cap, lm_cap):
    """a plan that does NOT fit: flagged, NaN denominators, counts clamped to the capacities, every index inside its list"""
    guards_intact(name, got, B, T, rows_cap, lm_cap)
    di = got["dims_i"][:4]
    assert di[3] == 1 and di[0] == rows_cap and di[1] == lm_cap, (name, di.tolist(), rows_cap, lm_cap)
    assert np.isnan(got["dims_f"][:2].view(np.float32)).all(), name
    off, lens = got["off"][:B], got["lens"][:B]
    assert (off >= 0).all() and (lens >= 1).all() and (off + lens <= rows_cap).all(), (name, off.tolist(), lens.tolist())
    assert (got["lm_idx"][:lm_cap] >= 0).all() and (got["lm_idx"][:lm_cap] < rows_cap).all(), name
    assert (got["lm_pos"][:lm_cap] >= 0).all() and (got["lm_pos"][:lm_cap] < B * T).all(), name
    assert (got["rows"][:rows_cap] >= 0).all() and (got["rows"][:rows_cap] < B * T).all(), name


def plan_battery(c, name, nsp=None):
    """lengths, then build with exact capacities, surplus capacities, one row short, one decoded row short, omitted lists"""
    B, T = c["B"], c["T"]
    header, lab32, w32 = dev_lengths(c, nsp)
    hw = check_header(c, header, nsp)
    total, nlm = int(hw[:B].sum()), int(hw[B:2 * B].sum())
    want_lm = nlm > 0
    for tag, rc_, lc_ in (("exact", total, nlm), ("surplus", total + 37, nlm + 5)):
        want = PR.build(hw, c["labels"], c["weights"], B, T, rc_, lc_, want_lm=want_lm)
        got = dev_build(header, lab32, w32, B, T, rc_, lc_ if want_lm else 0, want_lm=want_lm)
        check_fit(f"{name} {tag}", got, want, B, T, rc_, lc_)
    if total >= 2 and want_lm:
        check_short(f"{name} one row short", dev_build(header, lab32, w32, B, T, total - 1, nlm), B, T, total - 1, nlm)
    if nlm >= 2:
        check_short(f"{name} one decoded row short", dev_build(header, lab32, w32, B, T, total, nlm - 1), B, T, total, nlm - 1)
    # omitted lists: no rows / inv, no lm group -- off / lens / order and the counts are still right
    want = PR.build(hw, c["labels"], c["weights"], B, T, want_rows=False, want_lm=False)
    got = dev_build(header, lab32, w32, B, T, 0, 0, want_rows=False, want_lm=False)
    check_fit(f"{name} omitted lists", got, want, B, T, 0, 0)
    assert got["dims_i"][1] == 0
    return hw


KINDS = ("dense", "row", None)


@pytest.mark.parametrize("B", [1, 2, 255, 256, 257, 300])
def test_plan_batch_sizes(B):
    """T = 33 at batch sizes on both sides of the 256-thread strides: the prefix sums over the sequences before b, the totals
    block and the rank sort (lengths from a set of five values: ties fall back to batch order)."""
    for i, (tk, ck, use_w) in enumerate((("dense", "dense", True), ("row", "row", False), ("dense", None, True))):
        c = plan_case(B, 33, 37, tk, ck, use_w, seed=B * 7 + i)
        hw = plan_battery(c, f"plan B={B} text={tk} co={ck} w={use_w}", nsp=(5.0, 1.0))
        assert B < 255 or len(set(hw[:B].tolist())) <= 33                 # T = 33: equal lengths are unavoidable
    exact(f"plan_lengths / plan_build B={B}")


@pytest.mark.parametrize("T", [1, 31, 32, 33, 64, 255, 256])
def test_plan_sequence_lengths(T):
    for i, (tk, ck, use_w) in enumerate((("dense", "dense", True), ("row", "dense", False), (None, "row", True))):
        c = plan_case(5, T, 37, tk, ck, use_w, seed=T * 3 + i)
        plan_battery(c, f"plan T={T} text={tk} co={ck} w={use_w}")
    exact(f"plan_lengths / plan_build T={T}")


@pytest.mark.parametrize("R", [0, 1, 37, 256])
def test_plan_region_counts(R):
    for i, (tk, ck, use_w) in enumerate((("dense", "dense", True), ("row", "row", True), (None, "dense", False))):
        if R == 0 and tk is None:
            tk = "row"
        c = plan_case(6, 33, R, tk, ck, use_w, seed=R * 5 + i)
        plan_battery(c, f"plan R={R} text={tk} co={ck} w={use_w}")
    exact(f"plan_lengths / plan_build R={R}")


@pytest.mark.parametrize("text_kind", KINDS, ids=lambda k: f"text-{k}")
@pytest.mark.parametrize("co_kind", KINDS, ids=lambda k: f"co-{k}")
def test_plan_mask_kinds_and_hostile_sequences(text_kind, co_kind):
    """Dense, key-padding (query stride 0) and NULL text masks x dense, one-row and NULL co-attention masks, with and without
    weights, on a batch that holds every hostile sequence (plan_case), and the expected lengths of those stated outright."""
    B, T, R = 12, 33, 5
    for use_w in (True, False):
        c = plan_case(B, T, R, text_kind, co_kind, use_w, seed=17 + use_w)
        hw = plan_battery(c, f"plan kinds text={text_kind} co={co_kind} w={use_w}", nsp=(-0.0, 1e-40))
        assert hw[1] == 1 and hw[8] == 1                                  # nothing valid at all -> 1
        assert hw[3] == T and hw[10] == T                                 # valid only through a label at T - 1
        if co_kind is not None:
            p = int(np.nonzero(c["co"][2].reshape(-1, T).any(0))[0][0])
            assert hw[2] == (T if text_kind == "dense" else p + 1)        # valid only through a co-attention bit
        if text_kind == "dense":
            assert hw[4] == T and hw[11] == T                             # a valid token whose own row is empty
        assert hw[2 * B] == PR.f32_bits(-0.0) and hw[2 * B + 1] == PR.f32_bits(1e-40) and hw[2 * B + 1] != 0
    exact(f"plan hostile sequences text={text_kind} co={co_kind}")


def test_plan_nothing_decoded_and_no_masked_region():
    """No decoded row in the whole batch: dims_f[0] == 1.0; no image_label == 1 anywhere: dims_f[1] == +inf.  Labels NULL,
    labels all -1, image_label NULL and image_label without a 1."""
    B, T, R = 5, 33, 37
    c = plan_case(B, T, R, "dense", "dense", False, seed=3, labelled=False)
    c["il"] = np.where(c["il"] == 1, 0, c["il"])
    for with_labels in (True, False):
        header, lab32, w32 = dev_lengths(c, with_labels=with_labels)
        hw = check_header(c, header, with_labels=with_labels)
        total = int(hw[:B].sum())
        assert not hw[B:2 * B].any() and not hw[2 * B + 2:].any()
        want = PR.build(hw, c["labels"] if with_labels else None, None, B, T, total + 37, 5, want_lm=with_labels)
        got = dev_build(header, lab32, w32, B, T, total + 37, 5 if with_labels else 0, want_lm=with_labels)
        check_fit(f"plan nothing decoded labels={with_labels}", got, want, B, T, total + 37, 5)
        assert got["dims_i"][:4].tolist() == [total, 0, 0, 0]
        assert got["dims_f"][:2].tolist() == [PR.f32_bits(1.0), PR.f32_bits(float("inf"))]
    c["il"] = None
    header, lab32, w32 = dev_lengths(c)
    hw = check_header(c, header)
    got = dev_build(header, lab32, w32, B, T, int(hw[:B].sum()), 0, want_lm=False)
    assert got["dims_f"][:2].tolist() == [PR.f32_bits(1.0), PR.f32_bits(float("inf"))]
    exact("plan with nothing decoded and no masked region")


def test_plan_build_refuses_a_list_without_a_capacity():
    """A list that is given needs a capacity >= 1 (include/unimm_hip.h): the call returns UNIMM_E_ARG, launches nothing and
    leaves every sentinel-filled list bit for bit unchanged.  (The refused calls are never run the old way.)"""
    B, T = 5, 33
    c = plan_case(B, T, 37, "dense", "dense", True, seed=9)
    header, lab32, w32 = dev_lengths(c)
    hw = check_header(c, header)
    total, nlm = int(hw[:B].sum()), int(hw[B:2 * B].sum())
    for rows_cap, lm_cap, want_rows, want_lm in ((0, nlm, True, True), (-1, nlm, True, True), (total, 0, True, True),
                                                 (total, -3, True, True), (0, 0, True, False), (0, 0, False, True)):
        got = dev_build(header, lab32, w32, B, T, rows_cap, lm_cap, want_rows=want_rows, want_lm=want_lm, expect_rc=-1)
        for k, v in got.items():
            if v is not None:
                s = SENT64 if v.dtype == np.int64 else NAN32
                assert (v == s).all(), ("a refused call wrote", k, rows_cap, lm_cap)
    got = dev_build(header, lab32, w32, B, T, 0, 0, want_rows=False, want_lm=False)       # capacities of NULL lists are ignored
    assert got["off"][:B].tolist() == PR.build(hw, None, None, B, T, want_rows=False)["off"].tolist()
    exact("plan_build refusal of non-positive capacities")


# ----------------------------------------------------------------------------------------------
# D. casts, transposes, region packing, column sums
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 8, 9, 2047, 2048 * 8 + 3, 8 * 256 * 4096 + 5])
def test_cast_f32_bf16_tails_and_special_values(n):
    """Bit-exact against tensor.bfloat16() on the CPU (a NaN must come back as a NaN: same_bf16): ties both ways, +-0,
    subnormals, +-inf, NaN, values that round to inf;
    n below / at / past one 8-element chunk, and 8 x 256 x 4096 + 5 (every thread loops once more, then the tail)."""
    from unimm_amd import lib
    g = torch.Generator().manual_seed(n)
    x = with_edges(torch.randn(n, generator=g))
    want = bf16_bits_cpu(x)
    src = torch.cat([x, torch.full((24,), float("nan"))]).to(DEV)
    dst = sent16(n + 24)
    lib.cast_f32_bf16(src, dst, n)
    torch.cuda.synchronize()
    got = bits(dst)
    bad = np.nonzero(~same_bf16(got[:n], want))[0]
    assert bad.size == 0, (n, int(bad[0]), hex(int(x.numpy().view(np.uint32)[bad[0]])), hex(int(got[bad[0]]) & 0xFFFF))
    untouched("cast_f32_bf16 past n", dst[n:], NAN16)
    exact(f"cast_f32_bf16 n={n}")


@pytest.mark.parametrize("R", [1, 31, 32, 33, 65])
def test_transpose_cast_tiles_and_surplus_columns(R):
    from unimm_amd import lib
    for Cc in (1, 31, 32, 33, 100):
        for ldd in (R, rup(R, 64), rup(R, 64) + 64):
            g = torch.Generator().manual_seed(R * 1000 + Cc)
            x = with_edges(torch.randn((R, Cc), generator=g))
            dst = sent16(Cc + 2, ldd)
            lib.transpose_cast(x.to(DEV), dst, R, Cc, ldd)
            torch.cuda.synchronize()
            got = bits(dst)
            assert same_bf16(got[:Cc, :R], bf16_bits_cpu(x).T).all(), (R, Cc, ldd)
            assert not got[:Cc, R:].any(), ("surplus columns must be +0", R, Cc, ldd)
            untouched("transpose_cast rows behind C", dst[Cc:], NAN16)
    exact(f"transpose_cast R={R}")


@pytest.mark.parametrize("R,C_,lds,extra", [(65, 100, 104, 0), (65, 100, 104, 64), (37, 1000, 1008, 64), (64, 64, 64, 64),
                                            (1, 9, 16, 64), (65, 1, 8, 64)])
def test_transpose_bf16_surplus_tiles(R, C_, lds, extra):
    """unimm_transpose_bf16 with R = 65 (a second row tile of one row) and ldd = roundup(R, 64) + 64 (destination tiles that
    hold no source row): bit for bit, surplus columns zero, rows behind C unchanged."""
    from unimm_amd import lib
    g = torch.Generator().manual_seed(R * 131 + C_)
    src = torch.randn((R, lds), generator=g).to(torch.bfloat16)
    src[:, C_:] = float("nan")                                        # source padding is never copied
    ldd = rup(R, 64) + extra
    dst = sent16(C_ + 2, ldd)
    lib.transpose_bf16(src.to(DEV)[:, :C_], dst, R, C_)
    torch.cuda.synchronize()
    got = bits(dst)
    assert np.array_equal(got[:C_, :R], src[:, :C_].contiguous().view(torch.int16).numpy().T)
    assert not got[:C_, R:].any()
    untouched("transpose_bf16 rows behind C", dst[C_:], NAN16)
    exact(f"transpose_bf16 R={R} C={C_} ldd={ldd}")


@pytest.mark.parametrize("F,rows", [(8, 1), (8, 111), (2048, 1), (2048, 111), (8, 262147)])
def test_pack_image_seam_and_grid_stride(F, rows):
    """[feat | loc | 0] bit-exact against torch.cat(...).bfloat16(): the chunk that holds the seam (ld = F + 8) and zero chunks
    behind it (ld = roundup(F + 5, 64)), loc at an address that is not 16-byte aligned, and 262,147 rows x 8 chunks
    (> 8192 x 256 threads: the grid-stride loop)."""
    from unimm_amd import lib
    for ld in ((F + 8, rup(F + 5, 64)) if rows < 1000 else (rup(F + 5, 64),)):
        g = torch.Generator().manual_seed(F + rows + ld)
        feat = with_edges(torch.randn((rows, F), generator=g))
        loc = with_edges(torch.rand((rows, 5), generator=g))
        want = bf16_bits_cpu(torch.cat([feat, loc, torch.zeros(rows, ld - F - 5)], 1))
        locbuf = torch.cat([torch.full((1,), float("nan")), loc.reshape(-1)]).to(DEV)
        locd = locbuf[1:].view(rows, 5)
        assert locd.data_ptr() % 16 == 4
        out = sent16(rows + 3, ld)
        lib.pack_image(feat.to(DEV), locd, out, rows, F, ld)
        torch.cuda.synchronize()
        got = bits(out)
        assert same_bf16(got[:rows], want).all(), (F, rows, ld)
        untouched("pack_image rows behind the last", out[rows:], NAN16)
    exact(f"pack_image F={F} rows={rows}")


@pytest.mark.parametrize("M", [1, 3, 255, 256, 257, 64 * 256 + 1])
def test_colsum_row_split_and_padding(M):
    """db += column sums, per column against float64 with the fp32 summation bound (module docstring).  M on both sides of
    one row block, and 64 x 256 + 1 (the row split hits its cap of 64); N below / at / past one 512-column workgroup and ragged;
    NaN in the padding columns [N, ld) must reach no column, entries of db past N stay."""
    from unimm_amd import lib
    for N in (8, 504, 512, 520, 1601):
        ld = rup(N, 8) + 8
        g = torch.Generator().manual_seed(M + N)
        dy = (torch.randn((M, ld), generator=g) + 0.25).to(torch.bfloat16)
        dy[:, N:] = float("nan")
        db0 = torch.randn(N, generator=g)
        db = sent32(N + 8)
        db[:N] = db0.to(DEV)
        lib.colsum(dy.to(DEV), db, M, N)
        torch.cuda.synchronize()
        d = dy[:, :N].double()
        want = db0.double() + d.sum(0)
        scale = db0.double().abs() + d.abs().sum(0)
        got = db[:N].cpu().double()
        assert torch.isfinite(got).all(), ("padding NaN reached a column", M, N)
        gate(f"colsum M={M} N={N} |err| / (2^-24 (|db0| + sum |dy|))", ((got - want).abs() / (U * scale)).numpy(), M + 8)
        untouched("colsum db past N", db[N:], NAN32)


# ----------------------------------------------------------------------------------------------
# E. the fp32x3 operand makers
# ----------------------------------------------------------------------------------------------
# Gates of the two measured ops of unimm_x3_split: worst |err| / (2^-24 max(|ref|, 2^-10 row max |ref|)) over every case of
# test_x3_split_ops_and_layouts on an MI355X, doubled, and never above 64.
# (With the bf16 path's fast_erf, which these ops used before, the same cases gave 2.71e3 at a = -3.63 and 2.38e3 at
# b = -0.7534: 1 + erf(x) cancels on the negative side and GELU' crosses zero at b = -0.7518.  erfc and a derivative formed in
# double, csrc/x3ops.hip, brought them to the figures below.)
SPLIT_GATES = {2: 28.2,     # GELU: worst observed 14.1 (cols = 1601, rows = 37, a = -2.929: the rounded erfc argument)
               3: 3.84}     # MUL_DGELU: worst observed 1.92 (cols = 1601, rows = 37, a = 1.994, b = 0.838)
SQRT1_2 = 0.70710678118654752


def split_ref(op, a, b):
    a, b = a.double(), (b.double() if b is not None else None)
    if op == 2:
        return 0.5 * a * torch.special.erfc(-a * SQRT1_2)
    cdf = 0.5 * torch.special.erfc(-b * SQRT1_2)
    pdf = torch.exp(-0.5 * b * b) / math.sqrt(2 * math.pi)
    return a * (cdf + b * pdf)                                        # the derivative, written out: Phi(b) + b phi(b)


def odd_ld(cols):
    """a row stride > cols that is no multiple of 4"""
    return cols + 3 if (cols + 3) % 4 else cols + 2


def check_planes(name, out3, rows, cols, cp, hi, lo, wtype):
    got = bits(out3)
    p = [got[:rows, k * cp:(k + 1) * cp] for k in range(3)]
    want = (hi, hi, lo) if wtype else (hi, lo, hi)
    for k in range(3):
        assert np.array_equal(p[k][:, :cols], want[k]), (name, "plane", k)
        assert not p[k][:, cols:].any(), (name, "padding columns of plane", k)
    untouched(f"{name} out3 rows past the last", out3[rows:], NAN16)


@pytest.mark.parametrize("layout", ["aligned", "odd-a", "odd-out32"])
@pytest.mark.parametrize("op", [0, 1, 2, 3], ids=["copy", "add", "gelu", "mul_dgelu"])
def test_x3_split_ops_and_layouts(op, layout):
    """All four ops x both plane orders, at widths on both sides of the 8-column chunk and the 64-column plane padding.
    aligned: 16-byte vector paths; odd-a: a (and b) sliced from a wider buffer at column 1 (lda % 4 != 0, base misaligned: the
    scalar loads); odd-out32: out32 with ld32 > cols, ld32 % 4 != 0 (the scalar stores)."""
    from unimm_amd import lib
    worst, worst_at = 0.0, None
    for cols in (1, 7, 8, 9, 63, 64, 65, 1601):
        for rows in (1, 37):
            g = torch.Generator().manual_seed(cols * 100 + rows + op)
            cp = rup(cols, 64)
            lda = odd_ld(cols) if layout == "odd-a" else rup(cols, 4) + 4
            shift = 1 if layout == "odd-a" else 0
            wa = torch.randn((rows + 2, lda), generator=g) * 1.5
            wb = torch.randn((rows + 2, lda), generator=g) * 1.5
            wa[rows:], wb[rows:] = float("nan"), float("nan")
            a, b = wa[:rows, shift:shift + cols], wb[:rows, shift:shift + cols]
            ad, bd = wa.to(DEV)[:rows, shift:shift + cols], wb.to(DEV)[:rows, shift:shift + cols]
            assert ad.stride(0) == lda and (ad.data_ptr() % 16 == 0) == (layout != "odd-a")
            ld32 = odd_ld(cols) if layout == "odd-out32" else rup(cols, 4) + 4
            for wtype in (False, True):
                o32 = sent32(rows + 2, ld32)
                out3 = sent16(rows + 2, 3 * cp)
                lib.x3_split(ad, out3=out3, out32=o32[:, :cols], op=op, b=bd if op in (1, 3) else None, rows=rows, cols=cols,
                             cp=cp, wtype=wtype)
                torch.cuda.synchronize()
                name = f"x3_split op={op} {layout} cols={cols} rows={rows} w={int(wtype)}"
                y32 = o32[:rows, :cols].cpu()
                untouched(f"{name} out32 columns past cols", o32[:, cols:], NAN32)
                untouched(f"{name} out32 rows past the last", o32[rows:], NAN32)
                if op == 0:
                    assert np.array_equal(bits(y32), bits(a)), name
                elif op == 1:
                    assert np.array_equal(bits(y32), bits(a + b)), name
                else:
                    ref = split_ref(op, a, b).numpy()
                    floor = 2.0 ** -10 * np.abs(ref).max(1, keepdims=True)
                    ratio = np.abs(y32.double().numpy() - ref) / (U * np.maximum(np.abs(ref), floor))
                    if float(ratio.max()) > worst:
                        i, j = np.unravel_index(int(ratio.argmax()), ratio.shape)
                        worst = float(ratio.max())
                        worst_at = (name, float(a[i, j]), float(b[i, j]), float(ref[i, j]), float(y32[i, j]))
                hi, lo = split_def(y32)
                check_planes(name, out3, rows, cols, cp, hi, lo, wtype)
    if op >= 2:
        print(f"[prep-edges] x3_split op={op} {layout}: worst {worst:.3g} (gate {SPLIT_GATES[op]:.3g}) at {worst_at}; planes bit-exact")
        assert worst <= SPLIT_GATES[op], (worst, SPLIT_GATES[op], worst_at)
    else:
        exact(f"x3_split op={op} {layout} (fp32 result and planes)")


def test_x3_split_single_outputs_and_grid_stride():
    """out32 only and out3 only (the other pointer NULL), and 262,150 rows x 8 chunks (> 8192 x 256 threads: the grid-stride
    loop) at cols = 8."""
    from unimm_amd import lib
    g = torch.Generator().manual_seed(77)
    for rows, cols in ((37, 65), (3, 8)):
        cp = rup(cols, 64)
        a, b = torch.randn((rows, cols), generator=g), torch.randn((rows, cols), generator=g)
        ad, bd = a.to(DEV), b.to(DEV)
        o32 = sent32(rows + 2, cols + 4)
        lib.x3_split(ad, out3=None, out32=o32[:, :cols], op=lib.X3_ADD, b=bd, rows=rows, cols=cols, cp=cp)
        out3 = sent16(rows + 2, 3 * cp)
        lib.x3_split(ad, out3=out3, out32=None, op=lib.X3_ADD, b=bd, rows=rows, cols=cols, cp=cp, wtype=True)
        torch.cuda.synchronize()
        y32 = o32[:rows, :cols].cpu()
        assert np.array_equal(bits(y32), bits(a + b))
        untouched("x3_split out32-only guards", o32[:, cols:], NAN32)
        untouched("x3_split out32-only rows", o32[rows:], NAN32)
        check_planes("x3_split out3 only", out3, rows, cols, cp, *split_def(y32), True)
    rows, cols, cp = 262150, 8, 64
    a = torch.randn((rows, cols), generator=g)
    out3 = sent16(rows + 2, 3 * cp)
    o32 = sent32(rows + 2, cols)
    lib.x3_split(a.to(DEV), out3=out3, out32=o32, rows=rows, cols=cols, cp=cp)
    torch.cuda.synchronize()
    assert np.array_equal(bits(o32[:rows]), bits(a))
    untouched("x3_split grid-stride out32 rows past the last", o32[rows:], NAN32)
    check_planes("x3_split grid-stride", out3, rows, cols, cp, *split_def(a), False)
    exact("x3_split single outputs and the grid-stride loop")


BF16_MAX = 0x7F7F0000          # the largest finite bf16, as fp32 bits


def test_x3_split_value_edges():
    """The split itself, through COPY, on hand-made bit patterns.  For every finite input with |x| <= the bf16 maximum the
    planes equal the definition bit for bit: +-0, ties of the hi rounding in both directions, values whose lo itself needs
    rounding (24 significant bits), a small normal value whose lo is an fp32 subnormal, values just below the bf16 maximum.
    Subnormal INPUTS may come back as the definition or as signed zeros (printed).  +-inf and NaN keep their class in hi, and
    their lo is NaN (inf - inf).

    Known property of the scheme, not a failure: a finite value ABOVE the bf16 maximum's rounding boundary has hi = +-inf and
    therefore lo = -+inf, so a GEMM over the planes forms inf - inf; only hi = +-inf is asserted for those."""
    from unimm_amd import lib
    finite = [0x00000000, 0x80000000, 0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F808001, 0x3F807FFF,
              0x3F8000FF, 0x3F80FFFF, 0xBF7FFFFF, 0x3FFFFFFF, 0x40490FDB, 0xC0490FDB, 0x3EAAAAAB, 0x4B7FFFFF,     # lo needs rounding
              0x03808001, 0x83818001, 0x00800000, 0x00FFFFFF,                                                     # lo is subnormal
              0x7F7F0000, 0xFF7F0000, 0x7F7E8001, 0x7F7EFFFF, 0xFF7EFFFF, 0x7F000001, 0x7EFFFFFF]                 # near the bf16 maximum
    subn = [0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00008000, 0x00018000, 0x00400000]
    over = [0x7F7F8000, 0x7F7FFFFF, 0xFF7F8000, 0xFF7FFFFF, 0x7F7FC123]
    special = [0x7F800000, 0xFF800000, 0x7FC00000]
    words = finite + subn + over + special
    assert all((w & 0x7FFFFFFF) <= BF16_MAX for w in finite + subn)
    cols, cp = len(words), rup(len(words), 64)
    a = from_bits32([words, words[::-1]])
    rows = 2
    for wtype in (False, True):
        out3, o32 = sent16(rows + 1, 3 * cp), sent32(rows + 1, cols + 3)
        lib.x3_split(a.to(DEV), out3=out3, out32=o32[:, :cols], rows=rows, cols=cols, cp=cp, wtype=wtype)
        torch.cuda.synchronize()
        assert np.array_equal(bits(o32[:rows, :cols]), bits(a)), "COPY must pass every bit pattern through"
        got = bits(out3[:rows]).view(np.uint16)
        p = [got[:, k * cp:k * cp + cols] for k in range(3)]
        hi_g, lo_g = p[0], (p[2] if wtype else p[1])
        assert np.array_equal(p[0], p[1] if wtype else p[2]), "the two hi planes differ"
        assert not got.reshape(rows, 3, cp)[:, :, cols:].any()
        hi_d, lo_d = (x.view(np.uint16) for x in split_def(a))
        abits = a.numpy().view(np.uint32)
        mag = abits & 0x7FFFFFFF
        fin = (mag <= BF16_MAX) & (mag >= 0x00800000) | (mag == 0)
        assert np.array_equal(hi_g[fin], hi_d[fin]) and np.array_equal(lo_g[fin], lo_d[fin]), \
            [(hex(int(w)), hex(int(h)), hex(int(l)), hex(int(hd)), hex(int(ld_))) for w, h, l, hd, ld_ in
             zip(abits[fin], hi_g[fin], lo_g[fin], hi_d[fin], lo_d[fin]) if h != hd or l != ld_]
        sub = (mag > 0) & (mag < 0x00800000)
        as_def = (hi_g[sub] == hi_d[sub]) & (lo_g[sub] == lo_d[sub])
        sign = (abits[sub] >> 16).astype(np.uint16) & np.uint16(0x8000)
        as_zero = (hi_g[sub] == sign) & ((lo_g[sub] & np.uint16(0x7FFF)) == 0)
        assert (as_def | as_zero).all(), "subnormal inputs: neither the definition nor signed zeros"
        print(f"[prep-edges] x3_split subnormal inputs (w={int(wtype)}): {int(as_def.sum())} of {int(sub.sum())} as the definition, "
              f"{int((as_zero & ~as_def).sum())} as signed zeros")
        ov = (mag > BF16_MAX) & (mag < 0x7F800000)
        assert np.array_equal(hi_g[ov], np.where(abits[ov] >> 31, 0xFF80, 0x7F80).astype(np.uint16)), "hi of a value that rounds to inf"
        inf = mag == 0x7F800000
        assert np.array_equal(hi_g[inf], (abits[inf] >> 16).astype(np.uint16))
        nan = mag > 0x7F800000
        assert isnan16(hi_g[nan]).all() and isnan16(lo_g[nan | inf]).all()
    exact("x3_split value edges (finite inputs up to the bf16 maximum)")


@pytest.mark.parametrize("R", [1, 31, 32, 33, 65])
def test_x3_split_wt_tiles_strides_and_untouched_padding(R):
    """The transposed w-type split: three planes bit-exact transposes of the definition; columns [R, Rp) of every plane are NOT
    written (the caller zero-fills once), with Rp = roundup(R, 64) and one whole surplus tile more; source row stride C and C + 3."""
    from unimm_amd import lib
    for Cc in (1, 31, 33, 70):
        for lds in (Cc, Cc + 3):
            for Rp in (rup(R, 64), rup(R, 64) + 64):
                g = torch.Generator().manual_seed(R * 977 + Cc)
                w = torch.randn((R, lds), generator=g)
                w[:, :Cc] = with_edges(w[:, :Cc].contiguous(), finite=True)
                w[:, Cc:] = float("nan")
                dst = sent16(Cc + 1, 3 * Rp)
                lib.x3_split_wt(w.to(DEV)[:, :Cc], dst, R, Cc, Rp)
                torch.cuda.synchronize()
                got = bits(dst)
                x = w[:, :Cc].contiguous()
                hi, lo = split_def(x)
                mag = x.numpy().view(np.uint32) & 0x7FFFFFFF
                ok = ((mag <= BF16_MAX) & (mag >= 0x00800000) | (mag == 0)).T      # subnormal / overflowing inputs: see test_x3_split_value_edges
                for k, want in enumerate((hi, hi, lo)):
                    pl = got[:Cc, k * Rp:(k + 1) * Rp]
                    assert np.array_equal(pl[:, :R][ok], want.T[ok]), (R, Cc, lds, Rp, k)
                    assert (pl[:, R:] == np.int16(NAN16)).all(), ("columns [R, Rp) must not be written", R, Cc, lds, Rp, k)
                untouched("x3_split_wt rows behind C", dst[Cc:], NAN16)
    exact(f"x3_split_wt R={R}")


@pytest.mark.parametrize("H", [64, 128, 768, 1024])
@pytest.mark.parametrize("M", [1, 3, 4, 5, 8191, 8193])
def test_x3_layernorm_fwd_rows_planes_and_wave_grid(M, H):
    """y32 / mean / rstd bit-equal to unimm_layernorm_fwd on the same rows, planes bit-equal to the definition applied to y32,
    y32 per row against float64 with the gate and offset allowance of test_layernorm_fwd_wave_grid; with and without dropout,
    without y32, without mean / rstd; constant rows give exactly beta (times the dropout scale where kept); rows behind M stay.
    M = 8193 is past the grid's 8192 waves."""
    from unimm_amd import dropout as DR
    from unimm_amd import lib
    x, kind = ln_rows(M, H, seed=M + H)
    gamma, beta = ln_gamma_beta(H, M)
    xd, gd, bd = x.double().numpy(), gamma.double().numpy(), beta.double().numpy()
    mu = xd.mean(1)
    rs = 1.0 / np.sqrt(((xd - mu[:, None]) ** 2).mean(1) + 1e-12)
    yref = (xd - mu[:, None]) * rs[:, None] * gd + bd
    extra = offset_allowance(xd, rs, gd, yref, kind)
    xg = torch.cat([x, torch.full((4, H), float("nan"))]).to(DEV)
    gg, bg = gamma.to(DEV), beta.to(DEV)
    drop = DR.drop_arg(0.1, DR.make_key(3, 1, M + H))
    cst = kind == CONST
    for dr in (lib.NO_DROP, drop):
        tag = "drop" if dr[1] else "plain"
        y32, y3, mean, rstd = sent32(M + 4, H), sent16(M + 4, 3 * H), sent32(M + 4), sent32(M + 4)
        lib.x3_layernorm_fwd(xg, gg, bg, y32, y3, mean, rstd, M, H, drop=dr)
        r32, r16, rmean, rrstd = sent32(M + 4, H), sent16(M + 4, H), sent32(M + 4), sent32(M + 4)
        lib.layernorm_fwd(xg, gg, bg, r32, r16, rmean, rrstd, M, H, drop=dr)
        torch.cuda.synchronize()
        for a_, b_ in ((y32, r32), (mean, rmean), (rstd, rrstd)):
            assert np.array_equal(bits(a_), bits(b_)), f"x3_layernorm_fwd {tag}: fp32 outputs differ from unimm_layernorm_fwd"
        hi, lo = split_def(y32[:M])
        check_planes(f"x3_layernorm_fwd {tag}", y3, M, H, H, hi, lo, False)
        for t in (y32[M:], mean[M:], rstd[M:]):
            untouched("x3_layernorm_fwd rows past M", t, NAN32)
        want = yref
        keep = None
        if dr[1]:
            keep = DR.keep_mask2d(dr[0], dr[1], M, H)
            want = np.where(keep, yref * dr[2], 0.0)
        gate(f"x3_layernorm_fwd y32 {tag} M={M} H={H}", RR.row_ratio(f64(y32[:M]), want), 1e-5 + extra)
        if cst.any():
            yb = y32[:M].cpu().numpy()[cst]
            bexp = np.broadcast_to(beta.numpy(), yb.shape)
            if keep is not None:
                bexp = np.where(keep[cst], bexp * np.float32(dr[2]), np.float32(0))
            assert np.array_equal(yb, bexp.astype(np.float32)), f"constant rows {tag}"
        # the same planes without y32 and without the statistics
        y3b = sent16(M + 4, 3 * H)
        lib.x3_layernorm_fwd(xg, gg, bg, None, y3b, None, None, M, H, drop=dr)
        torch.cuda.synchronize()
        assert np.array_equal(bits(y3b), bits(y3)), f"x3_layernorm_fwd {tag}: planes change when y32 / mean / rstd are NULL"
    exact(f"x3_layernorm_fwd M={M} H={H} (fp32 outputs vs unimm_layernorm_fwd, planes vs the definition)")
