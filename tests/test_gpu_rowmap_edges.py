"""Row maps of the dropout + residual epilogue and of the LayerNorm backward (unimm_gemm_nt_args.drop_rows / aux_rows,
unimm_layernorm_bwd*.drop_rows): a launch on a SUBSET of rows must give every row exactly what the launch over all rows
gives it -- the dropout mask is hashed from the row a gathered row came from, the residual (dense, or a LayerNorm evaluated
on the fly from its statistics) is read there.

Every comparison of rows is bit for bit (torch.equal) against the same kernel run on all 200 rows and indexed afterwards;
one tile code per case and no split-K, so both launches reduce K in the same order.  The mapped launch has 70 rows (one full
and one partial 64-row slab, not a multiple of 16), listed unsorted with one row twice.

The column sums of the LayerNorm backward cannot be indexed out of a launch over other rows.  They are checked twice: with
the identity as the map they must equal the launch without a map bit for bit (same rows per wave), and with the unsorted map
they are held against an fp64 sum over the rows the kernel itself wrote, with the masks taken from the host mirror
(unimm_amd/dropout.py) at the MAPPED rows; the bound is the fp32 error of a sum of 70 terms that were themselves formed in fp32
(up to four roundings each), (70 + 8) * 2^-24 * sum|term|, plus for dbias the bf16 rounding of the rows it is recomputed from, 2^-9 * sum|term|.

EPI_BIAS_DROP_RESID writes the fp32 residual stream only: the entry point rejects a bf16 output (UNIMM_E_ARG), with or without
a map, and that is what the bf16 case here checks."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

M_FULL, M_MAP = 200, 70
DROP_P = 0.1
KEY = 0x9E3779B9
# (N, K): whole 64-column waves / a ragged edge walk with whole 8-column lanes / the split-column map of the fp32 FAST walk /
# a lane that straddles N (element-wise loads and stores)
SHAPES = [(128, 64), (72, 64), (768, 128), (76, 64)]
TILES = [7, 1, 12]          # 64x128, 128x128, 192x256 with the three-slot X ring


def _map(gen):
    m = torch.randperm(M_FULL, generator=gen)[:M_MAP].clone()
    m[41] = m[7]                                    # one row twice
    assert len(set(m.tolist())) == M_MAP - 1 and not torch.equal(m, m.sort().values)
    return m.to(torch.int32).cuda()


@pytest.fixture(scope="module")
def nt_case():
    """Operands and the full-row results, computed once per (N, K, tile, residual form)."""
    from unimm_amd import dropout as DR
    from unimm_amd import lib as L
    cache = {}

    def get(N, K, tile, ln):
        key = (N, K, tile, ln)
        if key in cache:
            return cache[key]
        gen = torch.Generator().manual_seed(1000 * N + K)
        x = (torch.randn(M_FULL, K, generator=gen) * 0.5).to(torch.bfloat16).cuda()
        w = (torch.randn(N, K, generator=gen) * 0.2).to(torch.bfloat16).cuda()
        bias = torch.randn(N, generator=gen).cuda()
        aux = torch.randn(M_FULL, N, generator=gen).cuda()
        aux_ln = None
        if ln:
            mean = aux.mean(1).contiguous()
            rstd = (1.0 / torch.sqrt(aux.var(1, unbiased=False) + 1e-12)).contiguous()
            aux_ln = (mean, rstd, (1.0 + 0.1 * torch.randn(N, generator=gen)).cuda(), (0.1 * torch.randn(N, generator=gen)).cuda())
        drop = DR.drop_arg(DROP_P, KEY)
        full = torch.full((M_FULL, N), float("nan"), device="cuda")
        L.gemm_nt(x, w, full, bias=bias, epilogue=L.EPI_BIAS_DROP_RESID, aux=aux, drop=drop, aux_ln=aux_ln, tile=tile)
        torch.cuda.synchronize()
        assert torch.isfinite(full).all()
        keep = DR.keep_mask2d(drop[0], drop[1], M_FULL, N)
        assert 0.05 < 1.0 - keep.mean() < 0.2          # dropout really is on
        cache[key] = dict(x=x, w=w, bias=bias, aux=aux, aux_ln=aux_ln, drop=drop, full=full, rows=_map(gen))
        return cache[key]
    return get


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("N,K", SHAPES)
def test_gemm_nt_drop_rows(nt_case, N, K, tile):
    """The mask of the mapped row, the residual gathered by the caller (dense fp32)."""
    from unimm_amd import lib as L
    c = nt_case(N, K, tile, False)
    rows = c["rows"].long()
    out = torch.full((M_MAP + 8, N), float("nan"), device="cuda")
    L.gemm_nt(c["x"][rows].contiguous(), c["w"], out, bias=c["bias"], epilogue=L.EPI_BIAS_DROP_RESID, aux=c["aux"][rows].contiguous(),
              drop=c["drop"], M=M_MAP, tile=tile, drop_rows=c["rows"])
    torch.cuda.synchronize()
    assert torch.equal(out[:M_MAP], c["full"][rows])
    assert torch.isnan(out[M_MAP:]).all()                      # nothing past row M
    # without the map the rows draw other masks: the comparison above is not vacuous
    plain = torch.empty((M_MAP, N), device="cuda")
    L.gemm_nt(c["x"][rows].contiguous(), c["w"], plain, bias=c["bias"], epilogue=L.EPI_BIAS_DROP_RESID, aux=c["aux"][rows].contiguous(),
              drop=c["drop"], M=M_MAP, tile=tile)
    assert not torch.equal(plain, c["full"][rows])


@pytest.mark.parametrize("ln", [False, True], ids=["dense", "lazy_ln"])
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("N,K", SHAPES)
def test_gemm_nt_aux_rows(nt_case, N, K, tile, ln):
    """The residual -- dense fp32, or (pre, mean, rstd, gamma, beta) -- read from the full-row stream at the mapped row."""
    from unimm_amd import lib as L
    c = nt_case(N, K, tile, ln)
    rows = c["rows"].long()
    out = torch.full((M_MAP + 8, N), float("nan"), device="cuda")
    L.gemm_nt(c["x"][rows].contiguous(), c["w"], out, bias=c["bias"], epilogue=L.EPI_BIAS_DROP_RESID, aux=c["aux"], drop=c["drop"],
              aux_ln=c["aux_ln"], M=M_MAP, tile=tile, drop_rows=c["rows"], aux_rows=c["rows"])
    torch.cuda.synchronize()
    assert torch.equal(out[:M_MAP], c["full"][rows])
    assert torch.isnan(out[M_MAP:]).all()
    # the two maps are independent: the residual alone mapped, masks of the compact rows
    a = torch.empty((M_MAP, N), device="cuda")
    b = torch.empty((M_MAP, N), device="cuda")
    aux_c = c["aux"][rows].contiguous()
    ln_c = (c["aux_ln"][0][rows].contiguous(), c["aux_ln"][1][rows].contiguous()) + c["aux_ln"][2:] if ln else None
    L.gemm_nt(c["x"][rows].contiguous(), c["w"], a, bias=c["bias"], epilogue=L.EPI_BIAS_DROP_RESID, aux=c["aux"], drop=c["drop"],
              aux_ln=c["aux_ln"], M=M_MAP, tile=tile, aux_rows=c["rows"])
    L.gemm_nt(c["x"][rows].contiguous(), c["w"], b, bias=c["bias"], epilogue=L.EPI_BIAS_DROP_RESID, aux=aux_c, drop=c["drop"],
              aux_ln=ln_c, M=M_MAP, tile=tile)
    assert torch.equal(a, b)


def test_gemm_nt_row_maps_need_the_dropout_residual_epilogue(nt_case):
    from unimm_amd import lib as L
    c = nt_case(128, 64, 7, False)
    rows = c["rows"].long()
    x = c["x"][rows].contiguous()
    out16 = torch.empty((M_MAP, 128), dtype=torch.bfloat16, device="cuda")
    with pytest.raises(L.UnimmHipError):          # the residual stream is fp32: no bf16 output of this epilogue, mapped or not
        L.gemm_nt(x, c["w"], out16, bias=c["bias"], epilogue=L.EPI_BIAS_DROP_RESID, aux=c["aux"], drop=c["drop"], M=M_MAP, tile=7,
                  drop_rows=c["rows"], aux_rows=c["rows"])
    with pytest.raises(L.UnimmHipError):
        L.gemm_nt(x, c["w"], out16, bias=c["bias"], epilogue=L.EPI_BIAS_DROP_RESID, aux=c["aux"], drop=c["drop"], M=M_MAP, tile=7)
    with pytest.raises(L.UnimmHipError):          # a map with another epilogue
        L.gemm_nt(x, c["w"], out16, bias=c["bias"], epilogue=L.EPI_BIAS, M=M_MAP, tile=7, drop_rows=c["rows"])


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm backward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ln_case():
    from unimm_amd import dropout as DR
    from unimm_amd import lib as L
    cache = {}

    def get(H):
        if H in cache:
            return cache[H]
        gen = torch.Generator().manual_seed(H)
        dy = torch.randn(M_FULL, H, generator=gen).to(torch.bfloat16).cuda()
        x = (torch.randn(M_FULL, H, generator=gen) * 1.5 + 0.3).cuda()
        mean = x.mean(1).contiguous()
        rstd = (1.0 / torch.sqrt(x.var(1, unbiased=False) + 1e-12)).contiguous()
        gamma = (1.0 + 0.1 * torch.randn(H, generator=gen)).cuda()
        drop, odrop = DR.drop_arg(DROP_P, KEY), DR.drop_arg(0.2, KEY ^ 0x55AA55AA)
        dx = torch.empty((M_FULL, H), dtype=torch.bfloat16, device="cuda")
        dxd = torch.empty_like(dx)
        part = torch.empty(L.colpartials_bytes(H) // 4, device="cuda")
        L.layernorm_bwd_partials(dy, x, mean, rstd, gamma, dx, dxd, part, M_FULL, H, drop=drop, out_drop=odrop)
        torch.cuda.synchronize()
        cache[H] = dict(dy=dy, x=x, mean=mean, rstd=rstd, gamma=gamma, drop=drop, odrop=odrop, dx=dx, dxd=dxd, rows=_map(gen))
        return cache[H]
    return get


def _ln_run(c, H, rows, entry, drop_rows):
    """The kernel on the gathered rows -> (dx, dxd, dgamma, dbeta, dbias)."""
    from unimm_amd import lib as L
    r = rows.long()
    n = r.numel()
    dy, x, mean, rstd = (c[k][r].contiguous() for k in ("dy", "x", "mean", "rstd"))
    dx = torch.full((n + 4, H), float("nan"), dtype=torch.bfloat16, device="cuda")
    dxd = torch.full((n + 4, H), float("nan"), dtype=torch.bfloat16, device="cuda")
    sums = [torch.zeros(H, device="cuda") for _ in range(3)]
    part = torch.empty(L.colpartials_bytes(H) // 4, device="cuda")
    if entry == "partials":
        blocks = L.layernorm_bwd_partials(dy, x, mean, rstd, c["gamma"], dx, dxd, part, n, H, drop=c["drop"], out_drop=c["odrop"],
                                          drop_rows=drop_rows)
        L.colpartials_finish_grouped([(part, blocks, H, sums)])
    else:
        L.layernorm_bwd(dy, x, mean, rstd, c["gamma"], dx, dxd, sums[0], sums[1], sums[2], part, n, H, drop=c["drop"],
                        out_drop=c["odrop"], drop_rows=drop_rows)
    torch.cuda.synchronize()
    assert torch.isnan(dx[n:].float()).all() and torch.isnan(dxd[n:].float()).all()
    return dx[:n], dxd[:n], sums


@pytest.mark.parametrize("entry", ["partials", "fused"])
@pytest.mark.parametrize("H", [768, 1024])
def test_layernorm_bwd_drop_rows(ln_case, H, entry):
    from unimm_amd import dropout as DR
    c = ln_case(H)
    rows = c["rows"]
    r = rows.long()
    dx, dxd, (dg, db, dbias) = _ln_run(c, H, rows, entry, rows)
    assert torch.equal(dx, c["dx"][r])
    assert torch.equal(dxd, c["dxd"][r])
    assert not torch.equal(dxd, dx)                                         # both masks are on
    dx_plain, dxd_plain, _ = _ln_run(c, H, rows, entry, None)
    assert not torch.equal(dx_plain, dx) and not torch.equal(dxd_plain, dxd)       # (out_drop changes dx, drop changes dxd)
    # column sums: fp64 over the mapped rows, masks from the host mirror at the rows of the map
    rn = r.cpu().numpy()
    ko = torch.from_numpy(DR.keep_mask2d(c["odrop"][0], c["odrop"][1], M_FULL, H)[rn]).cuda()
    d = torch.where(ko, c["dy"][r].double() * float(np.float32(c["odrop"][2])), torch.zeros((), dtype=torch.float64, device="cuda"))
    xh = (c["x"][r].double() - c["mean"][r].double()[:, None]) * c["rstd"][r].double()[:, None]
    eps32 = (M_MAP + 8) * 2.0 ** -24
    for got, terms, extra, what in ((dg, d * xh, 0.0, "dgamma"), (db, d, 0.0, "dbeta"), (dbias, dxd.double(), 2.0 ** -9, "dbias")):
        want, mag = terms.sum(0), terms.abs().sum(0)
        err = (got.double() - want).abs()
        print(f"{what}: max err {float(err.max()):.3e}, bound at that column {float(((eps32 + extra) * mag + 1e-30)[err.argmax()]):.3e}")
        assert (err <= (eps32 + extra) * mag + 1e-30).all(), what
    # the identity as the map = no map, bit for bit, column sums included
    ident = torch.arange(M_MAP, dtype=torch.int32, device="cuda")
    a = _ln_run(c, H, ident, entry, ident)
    b = _ln_run(c, H, ident, entry, None)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for sa, sb in zip(a[2], b[2]):
        assert torch.equal(sa, sb)
