"""fp64 restatements of the two kernels of speculative decoding (unimm_attn_verify, unimm_kv_cache_append; include/unimm_hip.h)
and the inputs their tests share -- TEST INFRASTRUCTURE, built on oracle/generate_ref.py.

attn_verify
  unimm_attn_decode with another key set among the new rows: new row i of a slot (pair i // 2, kind i % 2) attends the group's
  context rows, the slot's private rows [0, pl) and the new rows `pair_keys(i)`: the answer (even) rows of the pairs <= its own
  and, a copy row, itself.  Lengths are clamped as the header says (generate_ref.clamped_lengths with this launch's nr).
  The restatements ARE generate_ref's (attn_decode in float64 with its T32, attn_decode_f32 in the kernel's order of
  operations -- the kernel keeps attn_decode_kernel's order), evaluated with that key set, so the error model carries over:

  gate  |got - want| <= E = half_ulp_bf16(|want|) + C_VER * T32, T32 as derived in generate_ref's header.  C_VER is set by
  C_DEC's rule: the power of two >= 8 x the worst |fp32 restatement - fp64| / T32 over `verify_cases()`, measured on the CPU.

kv_cache_append: plain indexing, bit-exact (compare the int16 views).
"""
from __future__ import annotations

import contextlib

import numpy as np
import torch

from oracle import generate_ref as GR
from oracle.gemm_ref import half_ulp_bf16

BF16 = torch.bfloat16
GUARD = GR.GUARD

# measured on the CPU (tests/test_speculative_cpu.py::test_f32_restatement_inside_budget prints it again):
VER_MEASURED = 1.068      # worst |fp32 restatement - fp64| / T32 over verify_cases()
C_VER = 16.0              # the power of two >= 8 x VER_MEASURED


def pair_keys(i):
    """The new rows of its slot that new row i attends, in key order."""
    return list(range(0, i // 2 * 2 + 1, 2)) + ([i] if i % 2 else [])


def verify_key_rows(ctx_off, ctx_len, plen, g, s, i, beams, nr, pcap):
    """generate_ref.decode_key_rows under the pair rule."""
    c, pl = GR.clamped_lengths(ctx_len, plen, g, s, pcap, nr)
    co = int(ctx_off[g])
    return np.arange(co, co + c), s * pcap + np.arange(pl), s * nr + np.asarray(pair_keys(i), dtype=np.int64)


@contextlib.contextmanager
def _pair_rule():
    """generate_ref's two restatements walk `decode_key_rows`: evaluate them with the pair rule's key set."""
    was = GR.decode_key_rows
    GR.decode_key_rows = verify_key_rows
    try:
        yield
    finally:
        GR.decode_key_rows = was


def attn_verify(*args):
    """The arguments of generate_ref.attn_decode -> dict(out float64, T32, E with C_VER, nk)."""
    with _pair_rule():
        ref = GR.attn_decode(*args)
    ref["E"] = half_ulp_bf16(ref["out"].abs()) + C_VER * ref["T32"]
    return ref


def attn_verify_f32(*args):
    with _pair_rule():
        return GR.attn_decode_f32(*args)


# ---- inputs -------------------------------------------------------------------------------------------------------------------
VER_H = (1, 2, 3)
VER_G = (1, 3)
VER_BN = ((1, 2), (1, 4), (1, 10), (1, 32), (2, 16), (4, 8), (16, 2))
VER_CTX = (0, 1, 63, 64, 65, 255, 256)
VER_PCAP = (20, 6)


def verify_cross_cases(H, beams, nr):
    """G in {1, 3} for one (H, beams, nr): ctx_len per group cycles through VER_CTX and plen per slot through {0, 1, 3, pcap,
    pcap + 2, -1} (the last two are clamped), pcap alternates 20 / 6; contexts in reverse group order with gaps
    (generate_ref.decode_case)."""
    cases = []
    n = VER_H.index(H) * len(VER_BN) + VER_BN.index((beams, nr))
    for G in VER_G:
        pcap = VER_PCAP[(n + G) % 2]
        cl = [VER_CTX[(n + 3 * g + G) % 7] for g in range(G)]
        pls = (0, 1, 3, pcap, pcap + 2, -1)
        pl = [pls[(n + s) % len(pls)] for s in range(G * beams)]
        cases.append(GR.decode_case(5000 + 100 * n + G, H, beams, nr, G, pcap, cl, pl))
        n += 1
    return cases


def truncation_case():
    """ctx_len = 256, nr = 32, pcap = 40: plen 40 / 33 / 32 all see 320 - 32 - 256 = 32 private rows (beams = 1: three groups)."""
    return GR.decode_case(78, 2, 1, 32, 3, 40, [256, 256, 256], [40, 33, 32])


PROBE_B = GR.PROBE_B


def probe_case():
    """One launch (G = 2, beams = 2, nr = 8, pcap = 20, H = 2) in the style of generate_ref.probe_case: every V row carries its
    identity (column 0 of each head = id % 64, column 1 = id // 64; id = buffer row for the context, 4096 + row private, 8192 +
    row new), a probing query row puts all its mass on one chosen key, and real rows just outside its key set -- another copy
    row, the answer row of a later pair, the next slot's rows -- carry twice the probe on the same dims: seen by mistake, they
    take all the mass.  A probe is (query row, head, wanted id)."""
    G, beams, nr, pcap, H = 2, 2, 8, 20, 2
    case = GR.decode_case(4343, H, beams, nr, G, pcap, [9, 64], [0, 5, 20, 3])
    new, ctx, priv = case["new"], case["ctx"], case["priv"]
    D, HD = 64, H * 64
    for buf, base, col0 in ((ctx, 0, 2 * HD), (priv, 4096, HD), (new, 8192, 2 * HD)):
        ok = ~torch.isnan(buf[:, col0].float())
        rid = torch.arange(buf.shape[0]) + base
        for h in range(H):
            buf[ok, col0 + h * D] = (rid % 64).to(BF16)[ok]
            buf[ok, col0 + h * D + 1] = (rid // 64).to(BF16)[ok]
    probes, count = [], [0]
    off = case["ctx_off"].tolist()
    kcol = {"ctx": HD, "priv": 0, "new": HD}
    bufs = {"ctx": ctx, "priv": priv, "new": new}

    def plant(qrow, where, row, forbid=()):
        n = count[0]
        count[0] += 1
        h, dims = n % H, slice(4 * (n // H), 4 * (n // H) + 4)
        assert 4 * (n // H) + 4 <= D
        new[GUARD + qrow, h * D:(h + 1) * D] = 0
        new[GUARD + qrow, h * D:(h + 1) * D][dims] = PROBE_B
        bufs[where][row, kcol[where] + h * D:kcol[where] + (h + 1) * D][dims] = PROBE_B
        for w, r in forbid:
            bufs[w][r, kcol[w] + h * D:kcol[w] + (h + 1) * D][dims] = 2 * PROBE_B
        probes.append((qrow, h, {"ctx": 0, "priv": 4096, "new": 8192}[where] + row))

    qr = lambda s, i: s * nr + i                # noqa: E731
    nrow = lambda s, i: GUARD + s * nr + i      # noqa: E731
    prow = lambda s, r: GUARD + s * pcap + r    # noqa: E731
    # slot 0 (group 0, c = 9, plen 0)
    plant(qr(0, 0), "new", nrow(0, 0), forbid=[("new", nrow(0, 1)), ("new", nrow(0, 2))])      # answer 0: itself | its copy, answer 1
    plant(qr(0, 1), "new", nrow(0, 1), forbid=[("new", nrow(0, 2)), ("new", nrow(0, 3))])      # copy 0: itself | pair 1
    plant(qr(0, 3), "new", nrow(0, 0), forbid=[("new", nrow(0, 1))])                            # copy 1 sees answer 0 | not copy 0
    plant(qr(0, 4), "new", nrow(0, 2), forbid=[("new", nrow(0, 3)), ("new", nrow(0, 6))])      # answer 2 sees answer 1 | copy 1, answer 3
    plant(qr(0, 5), "new", nrow(0, 5), forbid=[("new", nrow(0, 3)), ("new", nrow(0, 7))])      # copy 2: itself | copies 1 and 3
    plant(qr(0, 6), "new", nrow(0, 6), forbid=[("new", nrow(0, 5)), ("new", nrow(0, 7))])      # answer 3 (last pair): itself
    plant(qr(0, 7), "new", nrow(0, 7), forbid=[("new", nrow(1, 0)), ("new", nrow(0, 5))])      # last copy | next slot's first
    plant(qr(0, 2), "ctx", off[0] + 8)                                                          # last context row
    # slot 1 (group 0, plen 5)
    plant(qr(1, 7), "new", nrow(1, 6), forbid=[("new", nrow(1, 5))])                            # last copy sees its answer row
    plant(qr(1, 6), "new", nrow(1, 4), forbid=[("new", nrow(1, 3))])                            # answer 3 sees answer 2
    plant(qr(1, 2), "priv", prow(1, 4), forbid=[("priv", prow(2, 0)), ("new", nrow(1, 4))])     # last private row | later answer
    plant(qr(1, 1), "priv", prow(1, 0), forbid=[("new", nrow(1, 2))])
    plant(qr(1, 5), "ctx", off[0], forbid=[("new", nrow(1, 1)), ("new", nrow(1, 3))])
    # slot 2 (group 1, c = 64, plen 20 = pcap), slot 3 (plen 3)
    plant(qr(2, 0), "priv", prow(2, 19), forbid=[("new", nrow(2, 2))])                          # full private cache
    plant(qr(2, 3), "ctx", off[1] + 63, forbid=[("ctx", off[0])])                               # last context row | next context
    plant(qr(2, 5), "new", nrow(2, 4), forbid=[("new", nrow(2, 6)), ("new", nrow(2, 1))])
    plant(qr(3, 2), "new", nrow(3, 2), forbid=[("new", nrow(3, 3)), ("new", nrow(3, 4)), ("new", nrow(2, 7))])
    plant(qr(3, 7), "priv", prow(3, 2), forbid=[("new", nrow(3, 1)), ("new", nrow(3, 3)), ("new", nrow(3, 5))])
    plant(qr(3, 1), "new", nrow(3, 0), forbid=[("new", nrow(3, 2))])
    case["probes"] = probes
    return case


def verify_cases():
    """Every attn_verify input of the suites: what C_VER is measured on."""
    out = []
    for H in VER_H:
        for beams, nr in VER_BN:
            out += verify_cross_cases(H, beams, nr)
    return out + [truncation_case(), probe_case()]


def measure(cases=None):
    """worst |fp32 restatement - fp64| / T32 over the cases"""
    w = 0.0
    for case in (verify_cases() if cases is None else cases):
        args = GR.decode_args(case, GR.decode_views(case))
        ref = attn_verify(*args)
        w = max(w, float(((attn_verify_f32(*args) - ref["out"]).abs() / ref["T32"]).max()))
    return w


# ---- kv_cache_append -------------------------------------------------------------------------------------------------------
def kv_cache_append(cache, new_kv, count, plen, layers, slots, pcap, width, max_count, new_layer_stride, new_row_mul, new_row_step):
    """The arguments of unimm_amd.lib.kv_cache_append as HOST tensors (cache [layers, slots, pcap, ldp] BEFORE the launch;
    new_kv a 2-D view at the first K column of layer 0's new rows, inside a buffer that holds every layer's).
    -> (cache after the launch, plen_out int32 [slots]); compare bit patterns."""
    want = cache.clone()
    flat = new_kv.new_empty(0).set_(new_kv.untyped_storage())
    base, ld_new = new_kv.storage_offset(), new_kv.stride(0)
    plen_out = torch.zeros(slots, dtype=torch.int32)
    for s in range(slots):
        pl = min(max(int(plen[s]), 0), pcap)
        cnt = min(max(int(count[s]), 0), max_count, pcap - pl)
        for l in range(layers):
            for j in range(cnt):
                o = base + l * new_layer_stride + (s * new_row_mul + j * new_row_step) * ld_new
                want[l, s, pl + j, :width] = flat[o:o + width]
        plen_out[s] = pl + cnt
    return want, plen_out


if __name__ == "__main__":
    print("worst fp32 / budget term over verify_cases(): %.4f" % measure())
