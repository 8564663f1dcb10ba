"""The row, loss, gather and weight-gradient kernels against float64 restatements (oracle/rows_ref.py for the launch
semantics, plain numpy / torch float64 for the math), at the row counts the full-size step runs and at every edge a
device-side count can sit on.

Every gate is PER ROW: the error of a row divided by the largest |reference| of that row (rows_ref.row_ratio; an all-zero
reference row must come back exactly zero).  Column sums are gated per column against max(|sum|, rss of its terms)
(rows_ref.col_ratio).  Each check prints its worst ratio next to its gate ("[row-edges] name: worst .. (gate ..)").

Wave grids.  layernorm_fwd_kernel / embed_fwd_kernel start at most 2048 x 4 = 8192 waves, layernorm_bwd_kernel /
embed_bwd_kernel at most UNIMM_RED_BLOCKS (512) x 4 = 2048: past those row counts a wave loops over rows and prefetches
its next row, which is what the full-size step (31k text rows, 8.9k regions) always runs.

Device counts.  A launch sized for a capacity reads the real count from a device word.  Every float input in rows at or
past the count is NaN, every buffer is allocated larger than the capacity with NaN in the extra rows (a missing clamp reads
NaN inside the allocation instead of reading past it), indices in the tails point at valid rows that hold NaN, and outputs
start as a sentinel NaN bit pattern that must survive wherever the header says a row is not written.

Stated fp32 allowances (U = 2^-24):
  * LayerNorm rows with a large offset: the fp32 mean is a sum over <= 16 values per lane and a 6-level wave tree, so it
    may be off by 24 U mean|x|; such rows get 24 U mean|x| rstd max|gamma| / max|y| on top of the ordinary gate.
  * log-sum-exp of a row: A = U (256 + 4 |lse|) absolute (the fp32 sum of exponentials and the rounding of lse itself).
  * 1 - p_y (unlikelihood) is formed in fp32 from exp(logp), as the reference does: relative error up to
    (T p_y + 2 U) / (1 - p_y) -- the "2^-23 / (1 - p)" cancellation bound, with T = U (16 + 4 |lse|) the error of logp when
    p_y is near 1 (the sum of exponentials is then the label's 1 plus small terms: <= 8 tree levels of rounding around 1).
    Only unlikelihood rows get it.  The label column of the gradient, p_y - 1, cancels the same way: a row may be off by
    2 (A max p + 2 U) / (its max |p - onehot|) on top of the bf16 gate."""
import math

import numpy as np
import pytest
import torch

from oracle import gemm_tn_ref as GT
from oracle import rows_ref as RR

pytestmark = pytest.mark.gpu
DEV = "cuda"

U = 2.0 ** -24
NAN16 = 0x7FA5                         # bf16 sentinel bit pattern (a NaN no kernel produces)
NAN32 = 0x7FA5A5A5                     # fp32 sentinel bit pattern
BF = 2.0 ** -8                         # bf16 rounding, relative to the element (hence to its row's max)
F32 = 2.0 ** -14                       # fp32 arithmetic slack added to a bf16 gate


def gate(name, ratios, limit):
    r = np.asarray(ratios, np.float64).reshape(-1)
    lim = np.broadcast_to(np.asarray(limit, np.float64), r.shape)
    if r.size == 0:
        return
    bad = ~(r <= lim)
    i = int(np.argmax(r))
    print(f"[row-edges] {name}: worst {r[i]:.3g} (gate {lim[i]:.3g})")
    assert not bad.any(), (name, int(np.argmax(bad)), float(r[np.argmax(bad)]), float(lim[np.argmax(bad)]))


def sent16(*shape):
    return torch.full(shape, NAN16, dtype=torch.int16, device=DEV).view(torch.bfloat16)


def sent32(*shape):
    return torch.full(shape, NAN32, dtype=torch.int32, device=DEV).view(torch.float32)


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).cpu().numpy()


def f64(t):
    return t.detach().float().cpu().double().numpy()


def dword(v, dtype=torch.int32):
    return torch.tensor([v], dtype=dtype, device=DEV)


def untouched(name, t, sentinel_bits):
    b = bits(t)
    assert (b == (sentinel_bits if b.dtype == np.int32 else np.int16(sentinel_bits))).all(), name


def split_value(t3, cp, width):
    """x-type split operand [rows, 3 cp] -> (hi + lo as float64 [rows, width], plane 2 == plane 0)"""
    hi, lo, hi2 = t3[:, :width], t3[:, cp:cp + width], t3[:, 2 * cp:2 * cp + width]
    return f64(hi) + f64(lo), bool((bits(hi) == bits(hi2)).all())


# ----------------------------------------------------------------------------------------------
# A. LayerNorm across the wave-grid edges
# ----------------------------------------------------------------------------------------------
OFFSET, CONST, ONEHOT = 1, 2, 3


def ln_rows(M, H, seed):
    """fp32 rows N(0.5, 2) with three kinds of hostile rows mixed in (every 97th row, and the last three rows)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((M, H), generator=g) * 2 + 0.5
    kind = np.zeros(M, np.int64)
    r = np.arange(M)
    for k in (OFFSET, CONST, ONEHOT):
        kind[r % 97 == k] = k
    if M >= 4:
        kind[-3:] = [OFFSET, CONST, ONEHOT]
    for i in np.nonzero(kind == OFFSET)[0]:
        x[i] = 1e3 + torch.randn(H, generator=g)
    x[torch.from_numpy(kind == CONST)] = 1.5                 # dyadic: the fp32 mean is exact and y must equal beta
    for i in np.nonzero(kind == ONEHOT)[0]:
        x[i] = 0.0
        x[i, i % H] = 1e4
    return x, kind


def ln_gamma_beta(H, seed):
    g = torch.Generator().manual_seed(seed + 1)
    return torch.randn(H, generator=g) * 0.2 + 1, torch.randn(H, generator=g) * 0.1


def offset_allowance(xd, rs, gd, yref, kind):
    """per-row extra for the large-offset rows (module docstring); 0 elsewhere"""
    extra = np.zeros(len(xd))
    sel = kind == OFFSET
    if sel.any():
        extra[sel] = 24 * U * np.abs(xd[sel]).mean(1) * rs[sel] * np.abs(gd).max() / np.abs(yref[sel]).max(1)
    return extra


@pytest.mark.parametrize("H", [8, 512, 520, 768, 1024])
@pytest.mark.parametrize("M", [1, 8191, 8192, 8193, 20000])
def test_layernorm_fwd_wave_grid(M, H):
    from unimm_amd import dropout as DR
    from unimm_amd import lib
    x, kind = ln_rows(M, H, seed=M + H)
    gamma, beta = ln_gamma_beta(H, M)
    xd, gd, bd = x.double().numpy(), gamma.double().numpy(), beta.double().numpy()
    mu = xd.mean(1)
    rs = 1.0 / np.sqrt(((xd - mu[:, None]) ** 2).mean(1) + 1e-12)
    yref = (xd - mu[:, None]) * rs[:, None] * gd + bd
    extra = offset_allowance(xd, rs, gd, yref, kind)
    xg = torch.cat([x, torch.full((4, H), float("nan"))]).to(DEV)       # rows past M are NaN: never read
    gg, bg = gamma.to(DEV), beta.to(DEV)
    drop = DR.drop_arg(0.1, DR.make_key(3, 1, M + H))
    for dr in (lib.NO_DROP, drop):
        y32, y16 = sent32(M + 4, H), sent16(M + 4, H)
        mean, rstd = sent32(M + 4), sent32(M + 4)
        lib.layernorm_fwd(xg, gg, bg, y32, y16, mean, rstd, M, H, drop=dr)
        torch.cuda.synchronize()
        want = yref
        if dr[1]:
            want = np.where(DR.keep_mask2d(dr[0], dr[1], M, H), yref * dr[2], 0.0)
        tag = "drop" if dr[1] else "plain"
        gate(f"layernorm_fwd y32 {tag}", RR.row_ratio(f64(y32[:M]), want), 1e-5 + extra)
        gate(f"layernorm_fwd y16 {tag}", RR.row_ratio(f64(y16[:M]), want), BF + F32 + extra)
        gate("layernorm_fwd mean (in row std)", np.abs(f64(mean[:M]) - mu) * rs, 1e-5 + extra)
        gate("layernorm_fwd rstd", np.abs(f64(rstd[:M]) - rs) / rs, 1e-5)
        for t in (y32[M:], y16[M:], mean[M:], rstd[M:]):
            untouched("layernorm_fwd rows past M", t, NAN32 if t.element_size() == 4 else NAN16)
        if not dr[1]:
            c = kind == CONST
            assert np.array_equal(y32[:M].cpu().numpy()[c], np.broadcast_to(beta.numpy(), (int(c.sum()), H)))
            assert (mean[:M].cpu().numpy()[c] == 1.5).all()


def ln_bwd_inputs(M, H, seed, cap=None, count=None):
    """x / saved statistics / dy for LayerNorm backward; rows >= count (and the extra rows past cap) NaN."""
    cap = M if cap is None else cap
    total = max(cap, count or 0) + 64
    x, kind = ln_rows(total, H, seed)
    mean = x.mean(1)                                             # fp32 statistics: what the forward would have saved
    rstd = torch.rsqrt(x.var(1, unbiased=False) + 1e-12)
    g = torch.Generator().manual_seed(seed + 7)
    dy = (torch.randn((total, H), generator=g) + 0.25).to(torch.bfloat16)
    live = RR.live(count, cap) if count is not None else M
    x[live:] = float("nan")
    mean[live:] = float("nan")
    rstd[live:] = float("nan")
    dy[live:] = float("nan")
    return x, mean, rstd, dy, kind, live


def ln_bwd_ref(x, mean, rstd, dy, gamma, live, H, drop=None, out_drop=None):
    from unimm_amd import dropout as DR
    keep = DR.keep_mask2d(drop[0], drop[1], live, H) if drop else None
    okeep = DR.keep_mask2d(out_drop[0], out_drop[1], live, H) if out_drop else None
    dyd = dy[:live].double().numpy()
    res = RR.layernorm_bwd(dyd, x[:live].double().numpy(), mean[:live].double().numpy(), rstd[:live].double().numpy(),
                           gamma.double().numpy(), keep, drop[2] if drop else 1.0, okeep, out_drop[2] if out_drop else 1.0)
    dyo = dyd if okeep is None else np.where(okeep, dyd * out_drop[2], 0.0)
    xh = (x[:live].double().numpy() - mean[:live].double().numpy()[:, None]) * rstd[:live].double().numpy()[:, None]
    return res, dict(dgamma=dyo * xh, dbeta=dyo, dbias=res[1])        # the terms of the three column sums


def check_colsums(name, got, prior, sums, terms):
    for q, key in enumerate(("dgamma", "dbeta", "dbias")):
        if got[q] is None:
            continue
        rss = np.sqrt((terms[key] ** 2).sum(0) + prior[q] ** 2)
        gate(f"{name} {key} (per column)", RR.col_ratio(f64(got[q]), prior[q] + sums[q], rss[None, :]), 1e-4)


@pytest.mark.parametrize("M,H", [(1, 768), (2047, 768), (2048, 768), (2049, 768), (2049, 520), (4097, 1024), (31000, 768)])
def test_layernorm_bwd_wave_grid(M, H):
    from unimm_amd import dropout as DR
    from unimm_amd import lib
    x, mean, rstd, dy, kind, live = ln_bwd_inputs(M, H, seed=M + 3 * H)
    gamma, _ = ln_gamma_beta(H, M + 1)
    drop = DR.drop_arg(0.1, DR.make_key(4, 2, M))
    odrop = DR.drop_arg(0.15, DR.make_key(4, 3, M))
    xg, mg, rg, dyg, gg = (t.to(DEV) for t in (x, mean, rstd, dy, gamma))
    part = torch.empty(lib.colpartials_bytes(H) // 4, device=DEV)
    rng = np.random.default_rng(M)
    for path, dr, od in (("full", drop, odrop), ("partials", drop, None), ("partials", None, odrop)):
        (dx_r, dxd_r, dg_r, db_r, dbias_r), terms = ln_bwd_ref(x, mean, rstd, dy, gamma, M, H, dr, od)
        dx, dxd = sent16(M + 64, H), sent16(M + 64, H)
        prior = [rng.standard_normal(H) for _ in range(3)]
        dsts = [torch.from_numpy(p).float().to(DEV) for p in prior]
        prior = [f64(d) for d in dsts]
        if path == "full":
            lib.layernorm_bwd(dyg, xg, mg, rg, gg, dx, dxd, *dsts, part, M, H, drop=dr, out_drop=od)
        else:
            blocks = lib.layernorm_bwd_partials(dyg, xg, mg, rg, gg, dx, dxd, part, M, H, drop=dr, out_drop=od)
            assert blocks == min((M + 3) // 4, 512)
            lib.colpartials_finish_grouped([(part, blocks, H, dsts)])
        torch.cuda.synchronize()
        tag = f"layernorm_bwd{'' if path == 'full' else '_partials'}"
        gate(f"{tag} dx", RR.row_ratio(f64(dx[:M]), dx_r), BF + F32)
        gate(f"{tag} dx_drop", RR.row_ratio(f64(dxd[:M]), dxd_r), BF + F32)
        untouched(f"{tag} rows past M", dx[M:], NAN16)
        check_colsums(tag, dsts, prior, (dg_r, db_r, dbias_r), terms)


def test_colpartials_finish_grouped_many_descriptors():
    """11 pending reductions in one call (> UNIMM_FINISH_MAX = 8: two launches), mixed H / blocks / nq, some destinations
    NULL; each destination is a slice followed by guard words that must not change."""
    from unimm_amd import lib
    rng = np.random.default_rng(5)
    shapes = [(768, 512, 3), (8, 1, 1), (520, 17, 2), (1024, 129, 4), (100, 16, 3), (768, 7, 3), (64, 512, 4), (1000, 3, 1),
              (768, 33, 3), (24, 2, 4), (512, 300, 2)]
    descs, want, keep = [], [], []
    for i, (H, blocks, nq) in enumerate(shapes):
        p = rng.standard_normal(blocks * nq * H).astype(np.float32)
        part = torch.cat([torch.from_numpy(p), torch.full((97,), float("nan"))]).to(DEV)
        dsts = []
        for q in range(nq):
            if (i + q) % 3 == 1:
                dsts.append(None)
                continue
            buf = torch.cat([torch.from_numpy(rng.standard_normal(H).astype(np.float32)), torch.full((16,), 7.0)]).to(DEV)
            dsts.append(buf)
        descs.append((part, blocks, H, [d[:H] if d is not None else None for d in dsts]))
        want.append(RR.finish([(p, blocks, H, [f64(d[:H]) if d is not None else None for d in dsts])])[0])
        keep.append((dsts, p.reshape(blocks, nq, H)))
    lib.colpartials_finish_grouped(descs)
    torch.cuda.synchronize()
    for (part, blocks, H, views), ref, (bufs, p) in zip(descs, want, keep):
        for q, (v, r, b) in enumerate(zip(views, ref, bufs)):
            if v is None:
                continue
            terms = np.concatenate([r[None, :] - p[:, q].astype(np.float64).sum(0), p[:, q].astype(np.float64)])
            gate("colpartials_finish_grouped (per column)", RR.col_ratio(f64(v), r, terms), 1e-5)
            assert (b[H:].cpu().numpy() == 7.0).all()


# ----------------------------------------------------------------------------------------------
# A. Embeddings
# ----------------------------------------------------------------------------------------------
V_WORD, V_POS, V_EXT = 3000, 512, 10


def embed_case(M, H, cap, count, seed, with_rows=True):
    """Tables with one NaN row each (word V-1, position V-1, extension 9) that only tail rows point at; rows map into a
    padded index space of 2 cap entries; 30 % of the live rows share one word id and one position."""
    g = torch.Generator().manual_seed(seed)
    live = RR.live(count, cap) if count is not None else M
    tabs = [torch.randn((n, H), generator=g) * 0.05 for n in (V_WORD, V_POS, 2, V_EXT)]
    for t in (tabs[0], tabs[1], tabs[3]):
        t[-1] = float("nan")
    P = 2 * cap + 64
    ids = torch.randint(0, V_WORD - 1, (P,), generator=g, dtype=torch.int32)
    pos = torch.randint(0, V_POS - 1, (P,), generator=g, dtype=torch.int32)
    typ = torch.randint(0, 2 + V_EXT - 1, (P,), generator=g, dtype=torch.int32)
    hot = torch.rand(P, generator=g) < 0.3
    ids[hot] = 103
    pos[hot] = 7
    rows = torch.randperm(P, generator=g).long() if with_rows else None
    src = rows[:live].numpy() if with_rows else np.arange(live)
    tail = rows[live:].numpy() if with_rows else np.arange(live, P)
    ids[tail] = V_WORD - 1                                  # tails point at valid rows that hold NaN
    pos[tail] = V_POS - 1
    typ[tail] = 2 + V_EXT - 1
    gamma, beta = ln_gamma_beta(H, seed)
    idx = RR.gather_index(live, None if rows is None else rows.numpy())
    il, pl, tl = ids.long().numpy()[idx], pos.long().numpy()[idx], typ.long().numpy()[idx]
    T = [t.double().numpy() for t in tabs]
    tvec = np.where((tl >= 2)[:, None], T[3][np.clip(tl - 2, 0, None)], T[2][np.clip(tl, 0, 1)])
    xs = T[0][il] + T[1][pl] + tvec
    return dict(tabs=tabs, ids=ids, pos=pos, typ=typ, rows=rows, gamma=gamma, beta=beta, live=live, xs=xs, il=il, pl=pl, tl=tl)


def run_embed(c, M, H, count, drop, dy_f32, seed):
    from unimm_amd import dropout as DR
    from unimm_amd import lib
    live = c["live"]
    tabs = [t.to(DEV) for t in c["tabs"]]
    ids, pos, typ = c["ids"].to(DEV), c["pos"].to(DEV), c["typ"].to(DEV)
    rows = c["rows"].to(DEV) if c["rows"] is not None else None
    gamma, beta = c["gamma"].to(DEV), c["beta"].to(DEV)
    m_dev = dword(count) if count is not None else None
    extra = max(M, count or 0) + 64
    y32, y16 = sent32(extra, H), sent16(extra, H)
    lib.embed_fwd(ids, pos, typ, *tabs, gamma, beta, y32, y16, M, H, drop=drop, m_dev=m_dev, rows=rows)
    xs = c["xs"]
    gd, bd = c["gamma"].double().numpy(), c["beta"].double().numpy()
    mu = xs.mean(1)
    rs = 1.0 / np.sqrt(((xs - mu[:, None]) ** 2).mean(1) + 1e-12)
    xh = (xs - mu[:, None]) * rs[:, None]
    yref = xh * gd + bd
    keep = DR.keep_mask2d(drop[0], drop[1], live, H) if drop[1] else None
    want = yref if keep is None else np.where(keep, yref * drop[2], 0.0)
    # dy: fp32 or bf16 upstream gradient, NaN past the count
    g = torch.Generator().manual_seed(seed + 11)
    dy = torch.randn((extra, H), generator=g) + 0.1
    if not dy_f32:
        dy = dy.to(torch.bfloat16)
    dy[live:] = float("nan")
    grads = [torch.zeros((n, H), device=DEV) for n in (V_WORD, V_POS, 2, V_EXT)]
    prng = np.random.default_rng(seed)
    prior = [torch.from_numpy(prng.standard_normal(H)).float().to(DEV) for _ in range(2)]
    dgam, dbet = prior[0].clone(), prior[1].clone()
    part = torch.empty(lib.colpartials_bytes(H) // 4, device=DEV)
    fn = lib.embed_bwd_f32 if dy_f32 else lib.embed_bwd
    fn(ids, pos, typ, *tabs, gamma, beta, dy.to(DEV), *grads, dgam, dbet, part, M, H, drop=drop, m_dev=m_dev, rows=rows)
    torch.cuda.synchronize()
    tag = "embed" + (" (m_dev)" if count is not None else "")
    if live:
        gate(f"{tag} fwd y32", RR.row_ratio(f64(y32[:live]), want), 1e-5)
        gate(f"{tag} fwd y16", RR.row_ratio(f64(y16[:live]), want), BF + F32)
    untouched(f"{tag} fwd rows past the count", y32[live:], NAN32)
    untouched(f"{tag} fwd rows past the count", y16[live:], NAN16)
    # backward reference: LayerNorm backward of the re-gathered rows, scattered into the tables
    d = dy[:live].double().numpy()
    if keep is not None:
        d = np.where(keep, d * drop[2], 0.0)
    gg = d * gd
    dx = rs[:, None] * (gg - gg.mean(1, keepdims=True) - xh * (gg * xh).mean(1, keepdims=True))
    il, pl, tl = c["il"], c["pl"], c["tl"]
    ext = tl >= 2
    ref_w = RR.scatter_add(np.zeros((V_WORD, H)), il, dx)
    ref_p = RR.scatter_add(np.zeros((V_POS, H)), pl, dx)
    ref_e = RR.scatter_add(np.zeros((V_EXT, H)), tl[ext] - 2, dx[ext])
    kname = "embed_bwd_f32" if dy_f32 else "embed_bwd"
    for name, got, ref in (("dword", grads[0], ref_w), ("dpos", grads[1], ref_p), ("dext", grads[3], ref_e)):
        gate(f"{kname} {name} (per table row)", RR.row_ratio(f64(got), ref), 2e-4)
    for t in range(2):
        terms = dx[tl == t]
        gate(f"{kname} dtype (per column)", RR.col_ratio(f64(grads[2][t]), terms.sum(0), terms), 1e-4)
    p0, p1 = f64(prior[0]), f64(prior[1])
    gate(f"{kname} dgamma (per column)", RR.col_ratio(f64(dgam), p0 + (d * xh).sum(0), np.concatenate([p0[None], d * xh])), 1e-4)
    gate(f"{kname} dbeta (per column)", RR.col_ratio(f64(dbet), p1 + d.sum(0), np.concatenate([p1[None], d])), 1e-4)


@pytest.mark.parametrize("M", [2049, 8193, 31000])
def test_embeddings_wave_grid_row_map_hot_ids(M):
    from unimm_amd import dropout as DR
    H = 768
    c = embed_case(M, H, M, None, seed=M)
    run_embed(c, M, H, None, DR.drop_arg(0.1, DR.make_key(6, 1, M)), dy_f32=False, seed=M)
    run_embed(c, M, H, None, (0, 0, 1.0), dy_f32=True, seed=M + 1)


EMB_CAP = 8300


@pytest.mark.parametrize("count", [0, 1, 2048, 2049, 8192, 8193, EMB_CAP, EMB_CAP + 500])
def test_embeddings_device_count(count):
    from unimm_amd import dropout as DR
    H = 768
    c = embed_case(EMB_CAP, H, EMB_CAP, count, seed=count + 17)
    run_embed(c, EMB_CAP, H, count, DR.drop_arg(0.1, DR.make_key(6, 2, count)), dy_f32=False, seed=count)
    run_embed(c, EMB_CAP, H, count, (0, 0, 1.0), dy_f32=True, seed=count + 1)


# ----------------------------------------------------------------------------------------------
# B. LayerNorm backward with a device-side row count (bf16 and fp32x3 forms)
# ----------------------------------------------------------------------------------------------
LNB_CAP = 4200


@pytest.mark.parametrize("count", [0, 1, 2047, 2048, 2049, 4096, 4097, LNB_CAP, LNB_CAP + 800])
def test_layernorm_bwd_partials_device_count(count):
    from unimm_amd import dropout as DR
    from unimm_amd import lib
    H, cap = 768, LNB_CAP
    x, mean, rstd, dy, kind, live = ln_bwd_inputs(cap, H, seed=count, cap=cap, count=count)
    gamma, _ = ln_gamma_beta(H, count)
    drop = DR.drop_arg(0.1, DR.make_key(5, 1, count))
    odrop = DR.drop_arg(0.1, DR.make_key(5, 2, count))
    (dx_r, dxd_r, dg_r, db_r, dbias_r), terms = ln_bwd_ref(x, mean, rstd, dy, gamma, live, H, drop, odrop)
    xg, mg, rg, gg = (t.to(DEV) for t in (x, mean, rstd, gamma))
    m_dev = dword(count)
    rng = np.random.default_rng(count)
    for form in ("bf16", "x3"):
        total = x.shape[0]
        part = torch.empty(lib.colpartials_bytes(H) // 4, device=DEV)
        prior = [torch.from_numpy(rng.standard_normal(H)).float().to(DEV) for _ in range(3)]
        dsts = [p.clone() for p in prior]
        if form == "bf16":
            dx, dxd = sent16(total, H), sent16(total, H)
            blocks = lib.layernorm_bwd_partials(dy.to(DEV), xg, mg, rg, gg, dx, dxd, part, cap, H, drop=drop, out_drop=odrop,
                                                m_dev=m_dev)
        else:
            dx, dxd = sent32(total, H), sent16(total, 3 * H)
            blocks = lib.x3_layernorm_bwd_partials(dy.float().to(DEV), xg, mg, rg, gg, dx, dxd, part, cap, H, drop=drop,
                                                   out_drop=odrop, m_dev=m_dev)
        lib.colpartials_finish_grouped([(part, blocks, H, dsts)])
        torch.cuda.synchronize()
        tag = "layernorm_bwd_partials (m_dev)" if form == "bf16" else "x3_layernorm_bwd_partials (m_dev)"
        if form == "bf16":
            gate(f"{tag} dx", RR.row_ratio(f64(dx[:live]), dx_r), BF + F32)
            gate(f"{tag} dx_drop", RR.row_ratio(f64(dxd[:live]), dxd_r), BF + F32)
            untouched(f"{tag} dx_drop rows past the count", dxd[live:], NAN16)
        else:
            gate(f"{tag} dx32", RR.row_ratio(f64(dx[:live]), dx_r), 1e-5)
            v, same = split_value(dxd[:live], H, H)
            assert same
            gate(f"{tag} dx_drop split", RR.row_ratio(v, dxd_r), 2.0 ** -16 + 1e-5)
            untouched(f"{tag} dx_drop rows past the count", dxd[live:], NAN16)
        untouched(f"{tag} dx rows past the count", dx[live:], NAN32 if form == "x3" else NAN16)
        check_colsums(tag, dsts, [f64(p) for p in prior], (dg_r, db_r, dbias_r), terms)


# ----------------------------------------------------------------------------------------------
# B. Weight-gradient GEMM with a device-side row count
# ----------------------------------------------------------------------------------------------
def tn_rows_per_split(M, N, K):
    """The split heuristic of launch_tn_group (csrc/gemm.hip) for one problem alone on the chip: the row ranges whose
    edges a device count must be tested at (oracle/gemm_tn_ref.py restates the launcher's rules)."""
    return GT.single_rows_per_split(M, N, K)


TN_FORMS = {"pp": (4096, 384, 320), "small": (3000, 200, 136)}     # gemm_tn_pp_kernel / gemm_tn_kernel<2,2,4>


def tn_operands(M, N, K, count, seed, extra=96):
    g = torch.Generator().manual_seed(seed)
    live = RR.live(count, M)
    dy = torch.randn((M + extra, N), generator=g).to(torch.bfloat16)
    x = torch.randn((M + extra, K), generator=g).to(torch.bfloat16)
    dy[live:] = float("nan")
    x[live:] = float("nan")
    prior_w = torch.randn((N, K), generator=g)
    prior_b = torch.randn(N, generator=g)
    return dy, x, prior_w, prior_b, live


def tn_check(tag, dw, db, dy, x, prior_w, prior_b, live, N, K):
    dyl, xl = dy[:live].double().numpy(), x[:live].double().numpy()
    ref_w = prior_w.double().numpy() + dyl.T @ xl
    gate(f"{tag} dw (per row)", RR.row_ratio(f64(dw[:N, :K]), ref_w), 1e-5)
    if db is not None:
        pb = prior_b.double().numpy()
        gate(f"{tag} dbias (per column)", RR.col_ratio(f64(db[:N]), pb + dyl.sum(0), np.concatenate([pb[None], dyl])), 1e-5)
        untouched(f"{tag} dbias guard", db[N:], NAN32)
    untouched(f"{tag} dw guard columns", dw[:, K:], NAN32)
    untouched(f"{tag} dw guard rows", dw[N:], NAN32)


def tn_out(prior_w, prior_b, N, K):
    dw = sent32(N + 3, K + 16)
    dw[:N, :K] = prior_w.to(DEV)
    db = sent32(N + 8)
    db[:N] = prior_b.to(DEV)
    return dw, db


@pytest.mark.parametrize("form", ["pp", "small"])
def test_gemm_tn_device_count_edges(form):
    from unimm_amd import lib
    M, N, K = TN_FORMS[form]
    rps = tn_rows_per_split(M, N, K)
    counts = sorted({0, 1, 63, 64, 65, rps - 1, rps, rps + 1, M, M + 61})
    print(f"[row-edges] gemm_tn {form}: rows_per_split {rps}, counts {counts}")
    for count in counts:
        dy, x, pw, pb, live = tn_operands(M, N, K, count, seed=count)
        dw, db = tn_out(pw, pb, N, K)
        lib.gemm_tn_grouped([(dy.to(DEV), x.to(DEV), dw, M, N, K, db, dword(count))])
        torch.cuda.synchronize()
        tn_check(f"gemm_tn {form} (m_dev)", dw, db, dy, x, pw, pb, live, N, K)


def test_gemm_tn_mixed_group_overwrite_and_workspace():
    from unimm_amd import lib
    probs = [("pp", 1500), ("pp", None), ("small", 700), ("small", None)]
    ops, launch = [], []
    for i, (form, count) in enumerate(probs):
        M, N, K = TN_FORMS[form]
        if count is None:
            M = M // 2 + 5                                          # exact row count: no tail, no NaN
        dy, x, pw, pb, live = tn_operands(M, N, K, count, seed=100 + i)
        dw, db = tn_out(pw, pb, N, K)
        ops.append((form, dy, x, pw, pb, live, N, K, dw, db))
        launch.append((dy.to(DEV), x.to(DEV), dw, M, N, K, db, dword(count) if count is not None else None))
    lib.gemm_tn_grouped(launch)                                      # both kernel forms, m_dev and exact problems mixed
    torch.cuda.synchronize()
    for form, dy, x, pw, pb, live, N, K, dw, db in ops:
        tn_check(f"gemm_tn {form} (mixed group)", dw, db, dy, x, pw, pb, live, N, K)

    # overwrite = 1 with m_dev = 0: the zero gradient stays zero; with a count it is the plain product
    for form, count in (("pp", 0), ("small", 0), ("small", 100), ("pp", 777)):
        M, N, K = TN_FORMS[form]
        dy, x, _, pb, live = tn_operands(M, N, K, count, seed=200 + count)
        zero = torch.zeros((N, K))
        dw, db = tn_out(zero, pb, N, K)
        lib.gemm_tn_grouped([(dy.to(DEV), x.to(DEV), dw, M, N, K, db, dword(count), True)])
        torch.cuda.synchronize()
        if count == 0:
            assert (bits(dw[:N, :K]) == 0).all()
        tn_check(f"gemm_tn {form} (overwrite)", dw, db, dy, x, zero, pb, live, N, K)

    # workspace: with a device count it must go unused (and stay zero); without one it carries the split partials
    ws = torch.zeros(64 << 20, dtype=torch.uint8, device=DEV)
    for count in (1025, None):
        M, N, K = TN_FORMS["pp"]
        dy, x, pw, pb, live = tn_operands(M, N, K, count, seed=300)
        dw, db = tn_out(pw, pb, N, K)
        lib.gemm_tn_grouped([(dy.to(DEV), x.to(DEV), dw, M, N, K, db, dword(count) if count is not None else None)], ws=ws)
        torch.cuda.synchronize()
        tn_check(f"gemm_tn pp (workspace, m_dev {count})", dw, db, dy, x, pw, pb, live, N, K)
        if count is not None:
            assert int(ws.count_nonzero()) == 0, "a launch with a device count wrote to the workspace"
    assert int(ws[:16384].count_nonzero()) == 0, "arrival counters were not left at zero"


# ----------------------------------------------------------------------------------------------
# B / D. gathers, reductions
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [0, 1, 199, 200, 260])
def test_gather_rows_device_count_bit_exact(count):
    """fp32 rows of 768 moved as 1536 16-bit values (the engine's use), gather and scatter, n_dev at and past the capacity."""
    from unimm_amd import lib
    cap, S, H = 200, 300, 1536
    live = RR.live(count, cap)
    g = torch.Generator().manual_seed(count)
    src = torch.randn((S, H // 2), generator=g).view(torch.bfloat16)
    src[S - 1] = float("nan")                                     # the row tail indices point at
    idx = torch.randperm(S - 1, generator=g)[:cap + 80].int()
    idx[live:] = S - 1
    srcg = src.to(DEV)
    dst = sent16(cap + 80, H)
    lib.gather_rows(srcg, idx.to(DEV), dst, cap, H, n_dev=dword(count))
    # scatter: rows i < count of a [cap + 40] source go to dst2[idx[i]]; tail source rows are NaN
    s2 = torch.randn((cap + 80, H // 2), generator=g).view(torch.bfloat16)
    s2[live:] = float("nan")
    dst2 = sent16(S, H)
    lib.gather_rows(s2.to(DEV), idx.to(DEV), dst2, cap, H, scatter=True, n_dev=dword(count))
    torch.cuda.synchronize()
    sb = bits(src)
    assert np.array_equal(bits(dst[:live]), sb[idx[:live].long().numpy()])
    untouched("gather_rows rows past the count", dst[live:], NAN16)
    want = np.full((S, H), NAN16, np.int16)
    want[idx[:live].long().numpy()] = bits(s2[:live])
    assert np.array_equal(bits(dst2), want)
    print(f"[row-edges] gather_rows count {count}: bit-exact")


@pytest.mark.parametrize("count", [0, 1, 255, 256, 257, 1000, 1300])
def test_reduce_sum_device_count_and_scale(count):
    from unimm_amd import lib
    cap = 1000
    live = RR.live(count, cap)
    src = torch.randn(cap + 400, generator=torch.Generator().manual_seed(count)) + 0.2
    src[live:] = float("nan")
    sd = src[:live].double().numpy()
    for scale_dev, scale in ((0.37, 1.0), (None, -2.5)):
        dst = sent32(4)
        lib.reduce_sum(src.to(DEV), cap, dst, scale=scale, n_dev=dword(count),
                       scale_dev=dword(scale_dev, torch.float32) if scale_dev is not None else None)
        torch.cuda.synchronize()
        s = scale_dev if scale_dev is not None else scale
        got = float(dst[0])
        assert math.isfinite(got)
        gate("reduce_sum (m_dev)", [abs(got - s * sd.sum()) / max(abs(s) * np.abs(sd).sum(), 1e-30)], 2e-6)
        untouched("reduce_sum past dst[0]", dst[1:], NAN32)


def test_segment_sum_negative_sign_few_segments():
    from unimm_amd import lib
    n = 5003
    g = torch.Generator().manual_seed(3)
    src = torch.randn(n, generator=g)
    seg = torch.randint(0, 3, (n,), generator=g, dtype=torch.int32)
    prior = torch.tensor([0.5, -1.0, 2.0, 9.0])
    dst = prior.to(DEV)
    lib.segment_sum(src.to(DEV), seg.to(DEV), dst, n, sign=-1.0)
    torch.cuda.synchronize()
    sd, sg = src.double().numpy(), seg.numpy()
    for s in range(3):
        terms = np.concatenate([[prior[s].item()], -sd[sg == s]])
        gate("segment_sum (per segment)", RR.col_ratio([float(dst[s])], [terms.sum()], terms[:, None]), 1e-5)
    assert float(dst[3]) == 9.0


# ----------------------------------------------------------------------------------------------
# C. Losses
# ----------------------------------------------------------------------------------------------
NORMAL, DOMINANT, NEAR_CLAMP, HUGE, FLAT = range(5)


def lm_logits(kinds, V, ld, seed):
    rng = np.random.default_rng(seed)
    n = len(kinds)
    z = np.full((n, ld), np.nan, np.float32)                        # columns V .. ld must never be read
    y = rng.integers(0, V, n)
    for i, k in enumerate(kinds):
        if k == NORMAL:
            z[i, :V] = rng.standard_normal(V) * 2
        elif k == DOMINANT:                                         # 1 - p_y ~ 5e-9: below the 1e-6 clamp
            z[i, :V] = rng.standard_normal(V)
            z[i, y[i]] = 30.0
        elif k == NEAR_CLAMP:                                       # 1 - p_y ~ 1.2e-5: just above the clamp
            c = math.log((V - 1) / 1.2e-5)
            z[i, :V] = -c + 0.01 * rng.standard_normal(V)
            z[i, y[i]] = 0.0
        elif k == HUGE:
            z[i, :V] = rng.uniform(-1e4, 1e4, V)
        else:
            z[i, :V] = 5.0
    return z, y


def lm_ref(z, y, w, V, gs):
    zd = z[:, :V].astype(np.float64)
    m = zd.max(1, keepdims=True)
    lse = (m + np.log(np.exp(zd - m).sum(1, keepdims=True)))[:, 0]
    p = np.exp(zd - lse[:, None])
    n = len(y)
    loss, nll, coef, py = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    for i in range(n):
        if y[i] < 0:
            continue
        logp = zd[i, y[i]] - lse[i]
        py[i] = math.exp(logp)
        nll[i] = -logp
        om = -math.expm1(logp)
        if w[i] > 0:
            loss[i], coef[i] = -logp * w[i], gs * w[i]
        elif w[i] == -1:
            loss[i] = -math.log(max(om, 1e-6))
            coef[i] = -gs * py[i] / om if om >= 1e-6 else 0.0
    onehot = np.zeros_like(p)
    ok = y >= 0
    onehot[np.nonzero(ok)[0], y[ok]] = 1.0
    grad = coef[:, None] * (p - onehot)
    return lse, loss, nll, grad, p, py


def lm_gates(lse, y, w, p, py):
    """per-row allowances of the module docstring: A (lse), the cancellation term of 1 - p_y / p_y - 1"""
    A = U * (256 + 4 * np.abs(lse))
    T = U * (16 + 4 * np.abs(lse))
    om = np.where(y >= 0, 1.0 - py, 1.0)
    canc = (T * py + 2 * U) / np.maximum(om, 1e-300)
    ul = (w == -1) & (y >= 0) & (om >= 1e-6)
    pm = p.max(1)
    D = np.maximum(om, np.where(y >= 0, np.where(np.arange(p.shape[1])[None, :] == y[:, None], 0.0, p).max(1), pm))
    grad_extra = 2 * (A * pm + 2 * U) / D + np.where(ul, 2 * canc, 0.0)
    return A, canc, ul, grad_extra


@pytest.mark.parametrize("V,ld", [(30522, 30522), (30522, 30528), (1000, 1001)])
def test_lm_loss_numerical_edges(V, ld):
    from unimm_amd import lib
    combos = [(k, wt) for k in range(5) for wt in (1, 3, 0, -1)] + [(NORMAL, 1), (DOMINANT, -1), (HUGE, 1), (FLAT, -1)]
    kinds = [k for k, _ in combos]
    z, y = lm_logits(kinds, V, ld, seed=V + ld)
    w = np.array([wt for _, wt in combos])
    y[-4:] = -1
    n = len(combos)
    g, inv = 0.75, 1.0 / 37
    gs = float(np.float32(g) * np.float32(inv))
    lse_r, loss_r, nll_r, grad_r, p, py = lm_ref(z, y, w, V, gs)
    A, canc, ul, gx = lm_gates(lse_r, y, w, p, py)
    zg = torch.from_numpy(z).to(DEV)
    yg, wg = torch.from_numpy(y.astype(np.int32)).to(DEV), torch.from_numpy(w.astype(np.int32)).to(DEV)
    rowloss, rownll, lse = sent32(n), sent32(n), sent32(n)
    lib.lm_loss_fwd(zg, yg, wg, rowloss, rownll, lse, n, V)
    ldd = (V + 7) // 8 * 8 + 8
    dl = sent16(n, ldd)
    gdev = dword(g, torch.float32)
    lib.lm_loss_bwd(zg, yg, wg, lse, gdev, inv, dl, n, V)
    cp = (V + 63) // 64 * 64
    d3 = sent16(n, 3 * cp)
    lib.x3_lm_loss_bwd(zg, yg, wg, lse, gdev, inv, d3, n, V)
    torch.cuda.synchronize()
    got_lse, got_loss, got_nll = f64(lse), f64(rowloss), f64(rownll)
    gate(f"lm_loss_fwd lse V={V} ld={ld} (abs / A)", np.abs(got_lse - lse_r) / A, 1.0)
    has = y >= 0
    gate(f"lm_loss_fwd rownll (abs)", np.abs(got_nll - nll_r)[has], (A + 1e-6 * np.abs(nll_r))[has])
    assert (got_nll[~has] == 0).all() and (got_loss[(w == 0) | ~has] == 0).all()
    lik = (w > 0) & has
    gate(f"lm_loss_fwd likelihood rowloss (abs)", np.abs(got_loss - loss_r)[lik], (w * A + 1e-6 * np.abs(loss_r))[lik])
    gate(f"lm_loss_fwd unlikelihood rowloss (abs, cancellation bound)", np.abs(got_loss - loss_r)[ul],
         (2 * canc + 1e-6 * np.abs(loss_r))[ul])
    clamped = (w == -1) & has & ~ul
    assert clamped.sum() >= 1
    gate("lm_loss_fwd clamped rowloss (rel)", np.abs(got_loss - loss_r)[clamped] / loss_r[clamped], 1e-6)
    r16 = RR.row_ratio(f64(dl[:, :V]), grad_r)
    tight = gx < F32                                                 # rows without a cancelling term, reported apart
    gate(f"lm_loss_bwd V={V} ld={ld}", r16[tight], (BF + F32 + gx)[tight])
    gate(f"lm_loss_bwd V={V} ld={ld} (rows with 1 - p_y or p_y - 1 cancelling)", r16[~tight], (BF + F32 + gx)[~tight])
    assert (bits(dl[:, V:]) == 0).all(), "dlogits columns V .. ldd must be zero"
    assert (f64(dl)[clamped] == 0).all(), "a clamped unlikelihood row has an exactly zero gradient"
    v3, same = split_value(d3, cp, V)
    assert same and (bits(d3[:, V:cp]) == 0).all()
    r3 = RR.row_ratio(v3, grad_r)
    gate(f"x3_lm_loss_bwd V={V}", r3[tight], (2.0 ** -16 + 2.0 ** -20 + gx)[tight])
    gate(f"x3_lm_loss_bwd V={V} (rows with 1 - p_y or p_y - 1 cancelling)", r3[~tight], (2.0 ** -16 + 2.0 ** -20 + gx)[~tight])


LM_CAP = 40


@pytest.mark.parametrize("count", [0, 1, LM_CAP - 1, LM_CAP, LM_CAP + 7])
def test_lm_loss_device_count(count):
    """n_dev / inv_dev, tails of NaN logits with valid labels; reduce_sum of the rows with n_dev and scale_dev."""
    from unimm_amd import lib
    V, ld, cap = 1000, 1004, LM_CAP
    live = RR.live(count, cap)
    total = cap + 8
    kinds = [NORMAL] * total
    z, y = lm_logits(kinds, V, ld, seed=count)
    w = np.array([(1, 3, 0, -1)[i % 4] for i in range(total)])
    z[live:] = np.nan
    y[live:] = 5
    w[live:] = 1
    inv = 0.125
    lse_r, loss_r, nll_r, grad_r, p, py = lm_ref(z[:live], y[:live], w[:live], V, 0.5 * inv)
    A, canc, ul, gx = lm_gates(lse_r, y[:live], w[:live], p, py)
    zg = torch.from_numpy(z).to(DEV)
    yg, wg = torch.from_numpy(y.astype(np.int32)).to(DEV), torch.from_numpy(w.astype(np.int32)).to(DEV)
    n_dev, inv_dev, gdev = dword(count), dword(inv, torch.float32), dword(0.5, torch.float32)
    rowloss, rownll, lse = sent32(total), sent32(total), sent32(total)
    lib.lm_loss_fwd(zg, yg, wg, rowloss, rownll, lse, cap, V, n_dev=n_dev)
    tot = sent32(2)
    lib.reduce_sum(rowloss, cap, tot, n_dev=n_dev, scale_dev=inv_dev)
    dl = sent16(total, 1008)
    lib.lm_loss_bwd(zg, yg, wg, lse, gdev, 99.0, dl, cap, V, n_dev=n_dev, inv_dev=inv_dev)
    d3 = sent16(total, 3 * 1024)
    lib.x3_lm_loss_bwd(zg, yg, wg, lse, gdev, 99.0, d3, cap, V, n_dev=n_dev, inv_dev=inv_dev)
    torch.cuda.synchronize()
    for name, t in (("rowloss", rowloss), ("rownll", rownll), ("lse", lse)):
        untouched(f"lm_loss_fwd {name} rows past the count", t[live:], NAN32)
    if live:
        gate("lm_loss_fwd (n_dev) lse (abs / A)", np.abs(f64(lse[:live]) - lse_r) / A, 1.0)
        gate("lm_loss_fwd (n_dev) rowloss (abs)", np.abs(f64(rowloss[:live]) - loss_r),
             np.maximum(w[:live], 1) * A + 2 * np.where(ul, canc, 0) + 1e-6 * np.abs(loss_r))
        gate("lm_loss_bwd (n_dev, inv_dev)", RR.row_ratio(f64(dl[:live, :V]), grad_r), BF + F32 + gx)
        v3, same = split_value(d3[:live], 1024, V)
        assert same
        gate("x3_lm_loss_bwd (n_dev, inv_dev)", RR.row_ratio(v3, grad_r), 2.0 ** -16 + 2.0 ** -20 + gx)
    got = float(tot[0])
    assert math.isfinite(got)
    gate("reduce_sum of rowloss (n_dev, scale_dev)", [abs(got - inv * loss_r.sum()) / max(inv * np.abs(loss_r).sum() + 1e-3, 1e-30)],
         1e-5)
    untouched("lm_loss_bwd rows past the count (not written)", dl[live:], NAN16)
    assert (bits(d3[live:cap]) == 0).all(), "x3_lm_loss_bwd writes zeros in rows past the count"
    untouched("x3_lm_loss_bwd rows past the launch", d3[cap:], NAN16)


def test_kl_loss_zero_targets_and_nan_rows():
    from unimm_amd import lib
    rows, C, ld = 40, 1601, 1608
    rng = np.random.default_rng(1)
    z = np.full((rows, ld), np.nan, np.float32)
    z[:, :C] = rng.standard_normal((rows, C)) * 2
    t = rng.random((rows, C)) ** 3
    t[rng.random((rows, C)) < 0.3] = 0.0
    t[4, :] = 0.0                                                    # a one-hot target on a live row
    t[4, 17] = 1.0
    t = (t / t.sum(1, keepdims=True)).astype(np.float32)
    lab = (np.arange(rows) % 3 != 2).astype(np.int32)
    z[lab == 0, :C] = np.nan                                         # ignored rows: loss and gradient exactly 0
    zg, tg, lg = torch.from_numpy(z).to(DEV), torch.from_numpy(t).to(DEV), torch.from_numpy(lab).to(DEV)
    rowloss, lse = sent32(rows), sent32(rows)
    lib.kl_loss_fwd(zg, tg, lg, rowloss, lse, rows, C)
    g, inv = 1.5, 1.0 / 9
    gdev, inv_dev = dword(g, torch.float32), dword(inv, torch.float32)
    ldd = 1616
    dz = sent16(rows, ldd)
    lib.kl_loss_bwd(zg, tg, lg, lse, gdev, 123.0, dz, rows, C, inv_dev=inv_dev)
    cp = 1664
    d3 = sent16(rows, 3 * cp)
    lib.x3_kl_loss_bwd(zg, tg, lg, lse, gdev, 123.0, d3, rows, C, inv_dev=inv_dev)
    torch.cuda.synchronize()
    on = lab == 1
    zd, td = z[on, :C].astype(np.float64), t[on].astype(np.float64)
    m = zd.max(1, keepdims=True)
    lse_r = (m + np.log(np.exp(zd - m).sum(1, keepdims=True)))[:, 0]
    logp = zd - lse_r[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        tl = np.where(td > 0, td * (np.log(np.where(td > 0, td, 1.0)) - logp), 0.0)
    loss_r = tl.sum(1)
    A = U * (256 + 4 * np.abs(lse_r))
    S = (td * (np.abs(np.log(np.where(td > 0, td, 1.0))) + np.abs(logp))).sum(1)
    gate("kl_loss_fwd rowloss (abs)", np.abs(f64(rowloss)[on] - loss_r), 1e-5 * S + td.sum(1) * A)
    gate("kl_loss_fwd lse (abs / A)", np.abs(f64(lse)[on] - lse_r) / A, 1.0)
    assert (f64(rowloss)[~on] == 0).all()
    gs = float(np.float32(g) * np.float32(inv))
    grad_r = gs * (np.exp(logp) * td.sum(1, keepdims=True) - td)
    gate("kl_loss_bwd", RR.row_ratio(f64(dz)[on, :C], grad_r), BF + F32 + 2 * A.max())
    assert (bits(dz[:, C:]) == 0).all() and (bits(dz[torch.from_numpy(~on).to(DEV)]) == 0).all()
    v3, same = split_value(d3, cp, C)
    assert same and (bits(d3[:, C:cp]) == 0).all()
    gate("x3_kl_loss_bwd", RR.row_ratio(v3[on], grad_r), 2.0 ** -16 + 2.0 ** -20 + 2 * A.max())
    assert (v3[~on] == 0).all()


def test_mse_loss_split_and_ignored_rows():
    from unimm_amd import lib
    rows, C, ld, ldd = 40, 2048, 2056, 2064
    rng = np.random.default_rng(2)
    z = np.full((rows, ld), np.nan, np.float32)
    z[:, :C] = rng.standard_normal((rows, C))
    t = rng.standard_normal((rows, C)).astype(np.float32)
    lab = (np.arange(rows) % 4 != 1).astype(np.int32)
    z[lab == 0, :C] = np.nan
    zg, tg, lg = torch.from_numpy(z).to(DEV), torch.from_numpy(t).to(DEV), torch.from_numpy(lab).to(DEV)
    rowloss = sent32(rows)
    lib.mse_loss_fwd(zg, tg, lg, rowloss, rows, C)
    g, inv = 0.8, 1.0 / 17
    gdev = dword(g, torch.float32)
    d16 = sent16(rows, ldd)
    lib.mse_loss_bwd(zg, tg, lg, gdev, inv, d16, rows, C)
    d3 = sent16(rows, 3 * ldd)
    lib.mse_loss_bwd(zg, tg, lg, gdev, inv, d3, rows, C, split=True)
    torch.cuda.synchronize()
    on = lab == 1
    diff = z[on, :C].astype(np.float64) - t[on]
    gate("mse_loss_fwd rowloss (rel)", np.abs(f64(rowloss)[on] - (diff ** 2).sum(1) / C) / ((diff ** 2).sum(1) / C), 1e-5)
    assert (f64(rowloss)[~on] == 0).all()
    gs = float(np.float32(np.float32(g) * np.float32(inv)) * np.float32(2.0) / np.float32(C))
    grad_r = gs * diff
    gate("mse_loss_bwd out_split 0", RR.row_ratio(f64(d16)[on, :C], grad_r), BF + F32)
    assert (bits(d16[:, C:]) == 0).all() and (bits(d16[torch.from_numpy(~on).to(DEV)]) == 0).all()
    v3, same = split_value(d3, ldd, C)
    assert same and (bits(d3[:, C:ldd]) == 0).all()
    gate("mse_loss_bwd out_split 1 (hi + lo)", RR.row_ratio(v3[on], grad_r), 2.0 ** -16 + 2.0 ** -20)
    assert (v3[~on] == 0).all()


@pytest.mark.parametrize("B", [1, 255, 256, 257, 600])
def test_nsp_loss_zero_class_weight_extra_and_fill(B):
    from unimm_amd import lib
    rng = np.random.default_rng(B)
    ld, ldd = 3, 5
    z = np.full((B, ld), np.nan, np.float32)
    z[:, :2] = rng.standard_normal((B, 2)) * 1.5
    lab = rng.integers(0, 2, B).astype(np.int32)
    lab[0] = 0
    extra = (rng.standard_normal((B, 2)) * 0.01).astype(np.float32)
    zg, lg, eg = torch.from_numpy(z).to(DEV), torch.from_numpy(lab).to(DEV), torch.from_numpy(extra).to(DEV)
    g = 1.3
    for w0, w1 in ((1.0, 0.0), (1.0, 2.5)):
        loss = sent32(2)
        lib.nsp_loss_fwd(zg, lg, w0, w1, loss, B)
        dl = sent32(B + 2, ldd)
        lib.nsp_loss_bwd(zg, lg, w0, w1, dword(g, torch.float32), dl, B, extra=eg)
        torch.cuda.synchronize()
        zd = z[:, :2].astype(np.float64)
        lse = np.logaddexp(zd[:, 0], zd[:, 1])
        wy = np.where(lab == 0, w0, w1)
        den = wy.sum()
        ref_loss = (wy * (lse - zd[np.arange(B), lab])).sum() / den
        gate(f"nsp_loss_fwd B={B} w1={w1}", [abs(float(loss[0]) - ref_loss) / max(abs(ref_loss), 1e-30)], 1e-5)
        untouched("nsp_loss_fwd past loss[0]", loss[1:], NAN32)
        p = np.exp(zd - lse[:, None])
        oh = np.eye(2)[lab]
        gsc = wy[:, None] * (g / den)
        ref = np.zeros((B, ldd))
        ref[:, :2] = gsc * (p - oh) + extra
        allow = (8 * U * np.abs(gsc[:, 0]) + 2 * U * np.abs(extra).max(1)) / np.maximum(np.abs(ref).max(1), 1e-30)
        gate(f"nsp_loss_bwd B={B} w1={w1}", RR.row_ratio(f64(dl[:B]), ref), 1e-5 + allow)
        assert (bits(dl[:B, 2:]) == 0).all()
        untouched("nsp_loss_bwd rows past B", dl[B:], NAN32)


# ----------------------------------------------------------------------------------------------
# D. Entry points without a direct test
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2, 7])
def test_sum_slabs_bf16_bit_exact(S):
    from unimm_amd import lib
    n, stride = 4104, 4116
    rng = np.random.default_rng(S)
    slabs = (rng.standard_normal((S, stride)) * (10.0 ** rng.integers(-3, 3, (S, stride)))).astype(np.float32)
    out = sent16(n + 16)
    lib.sum_slabs_bf16(torch.from_numpy(slabs).to(DEV), out, n)
    torch.cuda.synchronize()
    acc = np.zeros(n, np.float32)
    for s in range(S):
        acc = acc + slabs[s, :n]
    assert np.array_equal(bits(out[:n]), bits(torch.from_numpy(acc).to(torch.bfloat16)))
    untouched("sum_slabs_bf16 past n", out[n:], NAN16)
    print(f"[row-edges] sum_slabs_bf16 S={S}: bit-exact")


def test_transpose_cast_grouped_bit_exact():
    from unimm_amd import lib
    sizes = [(1, 1), (33, 31), (768, 3072), (5, 70), (64, 64), (100, 7), (1, 300), (300, 1), (40, 33), (33, 40), (2, 2),
             (768, 768), (31, 33)]
    rng = np.random.default_rng(0)
    entries, keep = [], []
    for R, C_ in sizes:
        ldd = R + 3 + (R % 5)
        ldd += 1 if ldd % 32 == 0 else 0
        src = torch.from_numpy(rng.standard_normal((R, C_)).astype(np.float32)).to(DEV)
        dst = sent16(C_ + 1, ldd)
        entries.append((src, dst[:C_]))
        keep.append((src, dst, R, C_, ldd))
    table, count, tiles = lib.transpose_table(entries, DEV)
    lib.transpose_cast_grouped(table, count, tiles)
    torch.cuda.synchronize()
    for src, dst, R, C_, ldd in keep:
        assert np.array_equal(bits(dst[:C_, :R]), bits(src.to(torch.bfloat16).t().contiguous())), (R, C_)
        assert (bits(dst[:C_, R:]) == 0).all(), (R, C_, ldd)
        untouched("transpose_cast_grouped guard row", dst[C_:], NAN16)
    print(f"[row-edges] transpose_cast_grouped {count} entries, {tiles} tiles: bit-exact")


def test_gelu_bwd_against_fp64_erf_derivative():
    from unimm_amd import lib
    n = 8 * 4099
    u = torch.linspace(-10, 10, n, dtype=torch.float64)
    u[::97] = 0.0
    u[1::97] = -0.7518                                             # GELU'(u) crosses zero here
    ub = u.to(torch.bfloat16)
    dt = torch.randn(n, generator=torch.Generator().manual_seed(1), dtype=torch.float64).to(torch.bfloat16)
    du = sent16(n + 8)
    lib.gelu_bwd(dt.to(DEV), ub.to(DEV), du, n)
    torch.cuda.synchronize()
    x = ub.double()
    dg = 0.5 * (1 + torch.special.erf(x / math.sqrt(2))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)
    ref = (dt.double() * dg).numpy()
    got = f64(du[:n])
    gate("gelu_bwd (per element, |ref| + 2^-12 |dt|)", np.abs(got - ref) / (np.abs(ref) + 2.0 ** -12 * np.abs(dt.double().numpy())),
         BF + F32)
    untouched("gelu_bwd past n", du[n:], NAN16)


def test_sum_dropout_fwd_bwd_with_keep_mask():
    from unimm_amd import dropout as DR
    from unimm_amd import lib
    n = 4099
    g = torch.Generator().manual_seed(8)
    a, b, dout = (torch.randn(n, generator=g) for _ in range(3))
    drop = DR.drop_arg(0.1, DR.make_key(1, 2, 9))
    keep = DR.keep_mask2d(drop[0], drop[1], 1, n)[0]
    sc = float(np.float32(drop[2]))
    out, da, db = sent32(n + 4), sent32(n + 4), sent32(n + 4)
    ag, bg = a.to(DEV), b.to(DEV)
    lib.mul_dropout(ag, bg, out, n, drop=drop, fusion_sum=True)
    lib.mul_dropout_bwd(ag, bg, dout.to(DEV), da, db, n, drop=drop, fusion_sum=True)
    torch.cuda.synchronize()
    ad, bd, dd = a.double().numpy(), b.double().numpy(), dout.double().numpy()
    want = np.where(keep, (ad + bd) * sc, 0.0)
    dk = np.where(keep, dd * sc, 0.0)
    for name, got, ref in (("sum_dropout", out, want), ("sum_dropout_bwd da", da, np.where(ad > 0, dk, 0.0)),
                           ("sum_dropout_bwd db", db, np.where(bd > 0, dk, 0.0))):
        gate(name + " (per element)", RR.row_ratio(f64(got[:n])[:, None], ref[:, None]), 2.0 ** -22)
        untouched(name + " past n", got[n:], NAN32)


def test_x3_rows_add_leaves_columns_past_h():
    from unimm_amd import lib
    R, H, ldd, n = 50, 768, 776, 20
    g = torch.Generator().manual_seed(4)
    dst0 = torch.randn((R, ldd), generator=g)
    dst0[:, H:] = 7.0
    idx = torch.randperm(R, generator=g)[:n].int()
    src = torch.randn((n, H), generator=g)
    dst = dst0.to(DEV)
    lib.x3_rows_add(dst[:, :H], idx.to(DEV), src.to(DEV), n, H)
    torch.cuda.synchronize()
    want = dst0.double().numpy()[:, :H].copy()
    want[idx.long().numpy()] += src.double().numpy()
    gate("x3_rows_add", RR.row_ratio(f64(dst[:, :H]), want), 2.0 ** -23)
    assert (dst[:, H:].cpu() == 7.0).all()
