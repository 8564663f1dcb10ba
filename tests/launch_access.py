"""What each launch touches: one table keyed by the wrapper functions of unimm_amd/lib.py (the engine reaches the C ABI only
through these).  An entry names the tensor parameters a launch WRITES ('W') or accumulates into with ATOMICS ('A'); every other
tensor among a wrapper's arguments (tuples such as dropout salts, length descriptors and LayerNorm statistics included) is read
('R').  Extents come from the tensor VIEW handed to the wrapper (data_ptr, shape, strides, element size): where a wrapper passes
a capacity larger than the rows in use, the larger extent stands.

Entry forms, per parameter name:
    (kind, abi, reason)         kind 'W' / 'A', or a function of the bound arguments returning one; abi = the names of the
                                header's pointer parameters (or struct fields) the tensor(s) feed; reason: one line, required
                                for every 'A' and every refined extent
    NEW                         the pseudo-parameter for tensors the wrapper allocates itself (outputs it returns, a default
                                workspace): written by its kernel
    HOST_OUT                    a host word the C side fills before it returns (no device access, but a non-const pointer)
    a function under "members"  for list parameters: yields (tensor, kind) per member
    a function under "extent"   a finer or wider extent than the view, per parameter

No entry is an exemption by buffer name, stream or call site: a false report is answered here by stating the access more
exactly.  tests/stream_trace.py checks the table against the raw pointers that reach the ABI (no non-const pointer outside a
declared write), tests/test_stream_order_cpu.py its completeness and, for flat prototypes, its names against the header.

No torch import: tensors are used through data_ptr() / shape / stride() / element_size() only."""
import inspect
import re

NEW, HOST_OUT = "<new>", "<host out>"
HOST_TIMELINE = "host"          # wrappers that run on the host (pinned staging): their launches sit on the host timeline


def W(abi, reason=None):
    return ("W", abi, reason)


def A(abi, reason):
    return ("A", abi, reason)


def is_tensor(x):
    return hasattr(x, "data_ptr") and hasattr(x, "element_size") and hasattr(x, "stride")


def extent(t, kind):
    """The access of a tensor view: a flat byte range when the view is dense, rows x column range when one stride separates dense
    rows (column slices of one buffer then do not alias), the bounding range otherwise.  None for an empty view."""
    shape, es = tuple(t.shape), t.element_size()
    if any(s == 0 for s in shape):
        return None
    lo = t.data_ptr()
    dims = sorted(((st, n) for n, st in zip(shape, t.stride()) if n > 1), key=lambda d: d[0])
    if any(st <= 0 for st, _ in dims):                          # broadcast or reversed views: bounding range
        span = sum((n - 1) * abs(st) for st, n in dims) + 1
        return (lo, lo + span * es, kind)
    run, k = 1, 0                                                # the dense inner part: elements [0, run)
    while k < len(dims) and dims[k][0] == run:
        run *= dims[k][1]
        k += 1
    rest = dims[k:]
    if not rest:
        return (lo, lo + run * es, kind)
    if len(rest) == 1 or all(rest[i + 1][0] == rest[i][0] * rest[i][1] for i in range(len(rest) - 1)):
        rows = 1
        for _, n in rest:
            rows *= n
        return (lo, lo + run * es, kind, rows, rest[0][0] * es)
    span = sum((n - 1) * st for st, n in dims) + 1
    return (lo, lo + span * es, kind)


def tensors_in(x):
    """Every tensor inside an argument (a tensor, or tuples / lists / dicts of them, or objects with a `words` tensor)."""
    if x is None:
        return
    if is_tensor(x):
        yield x
    elif isinstance(x, (tuple, list)):
        for y in x:
            yield from tensors_in(y)
    elif isinstance(x, dict):
        for y in x.values():
            yield from tensors_in(y)


# ---- members of the list parameters -------------------------------------------------------------------------------------
def _tn_problems(problems):
    """gemm_tn_grouped: (dy, x, dw, M, N, K, dbias[, m_dev[, overwrite]])"""
    for dy, x, dw, M, N, K, dbias, *rest in problems:
        yield dy, "R"
        yield x, "R"
        # dw += dy^T x in fp32 atomics (several split tiles, and several problems, may add into one dw); with `overwrite` the
        # kernel owns the zeroed tile and stores it
        yield dw, ("W" if len(rest) > 1 and rest[1] else "A")
        if dbias is not None:
            yield dbias, "A"                                     # column sums of dy added with atomics
        if rest and rest[0] is not None:
            yield rest[0], "R"


def _finish_pending(pending):
    """colpartials_finish_grouped: (partials, blocks, H, [dst ...]): dst += column sums, one workgroup per column block (no atomics)"""
    for part, blocks, H, dsts in pending:
        yield part, "R"
        for t in dsts:
            if t is not None:
                yield t, "W"


_transpose_tables = {}          # data_ptr of a device table -> its (src, dst) entries (filled by the traced `transpose_table`)


def note_transpose_table(entries, result):
    _transpose_tables[result[0].data_ptr()] = [(s, d) for s, d in entries]


def _transpose_members(table):
    for src, dst in _transpose_tables.get(table.data_ptr(), ()):
        yield src, "R"
        yield dst, "W"


def _x3_planes(name):
    """dq / dk / dv of x3_attn_bwd with `planes`: the view is the slice's columns in plane 0 of a split buffer; the kernel writes
    the same columns of all three planes (column offsets 0, cp3, 2 cp3 of the same rows) -> three row-strided accesses, so that
    the slices of one buffer that the two streams' launches fill stay apart."""
    def ext(t, kind, bound):
        planes = bound.get("planes")
        base = extent(t, kind)
        if planes is None or base is None:
            return base
        cp3, ld3 = planes
        es = t.element_size()
        width = t.shape[1] * es
        return [(base[0] + p * cp3 * es, base[0] + p * cp3 * es + width, kind, t.shape[0], ld3 * es) for p in range(3)]
    return ext


_ATT_OUT = dict(out=W("out"), lse=W("lse"))
_ATT_BWD = dict(delta=W("delta"), dq=W("dq"), dk=W("dk"), dv=W("dv"))
_LM_OUT = dict(token=W("token"), logp=W("logp"), logq=W("logq"), lse=W("lse"))
_EMB_BWD = dict(
    dword=A("dword", "rows of the word table are added with atomics (many tokens share a row)"),
    dpos=A("dpos", "position rows are added with atomics"),
    dext=A("dext", "extra-embedding rows are added with atomics"),
    dtype=W("dtype"), dgamma=W("dgamma"), dbeta=W("dbeta"), partials=W("partials"))

TABLE = {
    # ---- GEMMs
    "gemm_nt": dict(out=W("out"), out2=W("out2"), splitk_ws=W("splitk_ws")),
    "gemm_tn": dict(dw=A("dw", "dw += dy^T x with fp32 atomics"), dbias=A("dbias", "column sums added with atomics")),
    "gemm_tn_grouped": dict(members=dict(problems=_tn_problems), ws=W("ws")),
    # ---- attention
    "attn_fwd": dict(_ATT_OUT),
    "attn_spliced_fwd": dict(_ATT_OUT),
    "attn_spliced_bwd": dict(dq=W("dq"), dk=W("dk"), dv=W("dv")),
    "attn_probs": dict(probs=W("probs")),
    "attn_bwd": dict(_ATT_BWD),
    "attn_decode": dict(out=W("out")),
    "kv_cache_update": dict(dst=W("dst"), plen_out=W("plen_out")),
    "attn_verify": dict(out=W("out")),
    "kv_cache_append": dict(cache=W("cache"), plen_out=W("plen_out")),
    "lm_topk": dict(vals=W("vals"), ids=W("ids"), lse=W("lse")),
    "lm_sample": dict(_LM_OUT),
    "lm_sample_rows": dict(_LM_OUT),
    "lm_spec_verify": dict(accept=W("accept"), token=W("token"), logp=W("logp"), logq=W("logq"), lse=W("lse"),
                           log_ratio=W("log_ratio")),
    "lm_topk_hist": dict(vals=W("vals"), ids=W("ids"), lse=W("lse")),
    "lm_sample_hist": dict(_LM_OUT),
    # ---- row kernels
    "mask_pack": {"out": W("out"), NEW: W("out")},
    "mask_synth": {NEW: W("text_words co_words")},
    "plan_lengths": {NEW: W("header")},
    "plan_build": {NEW: W("off lens rows inv lm_pos lm_idx lm_label lm_weight order"), "dims": W("dims_i dims_f")},
    "layernorm_fwd": dict(y32=W("y32"), y16=W("y16"), mean=W("mean"), rstd=W("rstd")),
    "layernorm_bwd": dict(dx=W("dx"), dx_drop=W("dx_drop"), dgamma=W("dgamma"), dbeta=W("dbeta"), dbias=W("dbias"),
                          partials=W("partials")),
    # blocks_out: a host int32 the C side fills before it returns (the number of partial blocks): no device access
    "layernorm_bwd_partials": {"dx": W("dx"), "dx_drop": W("dx_drop"), "partials": W("partials"), HOST_OUT: W("blocks_out")},
    "colpartials_finish_grouped": dict(members=dict(pending=_finish_pending)),
    "embed_fwd": dict(y32=W("y32"), y16=W("y16")),
    "embed_bwd": dict(_EMB_BWD),
    "embed_bwd_rows": dict(drow=W("drow"), dtype=W("dtype"), dgamma=W("dgamma"), dbeta=W("dbeta"), partials=W("partials")),
    "rows_scatter_sum_f32": dict(dst=W("dst")),
    "colsum": dict(db=A("db", "column sums added with atomics")),
    "cast_f32_bf16": dict(dst=W("dst")),
    "transpose_cast": dict(dst=W("dst")),
    "transpose_bf16": dict(dst=W("dst")),
    "sum_slabs_bf16": dict(out=W("out")),
    "segment_rows_sum_bf16": dict(dst=W("dst")),
    "transpose_cast_grouped": dict(members=dict(table=_transpose_members)),
    "pack_image": dict(out=W("out")),
    "mul_dropout": dict(out=W("out")),
    "mul_dropout_bwd": dict(da=W("da"), db=W("db")),
    "linear_f32": dict(out=(lambda b: "A" if b.get("accumulate") else "W", "out", "accumulate=True adds with fp32 atomics"),
                       rowsum=A("rowsum", "rowsum[m] += ... with atomics")),
    "rows_add_f32": dict(dst=W("dst")),
    "reduce_sum": dict(dst=W("dst")),
    "segment_sum": dict(dst=A("dst", "dst[seg[i]] += ... with atomics")),
    "gelu_bwd": dict(du=W("du")),
    "gather_rows": dict(dst=W("dst")),
    # ---- losses
    "lm_loss_fwd": dict(rowloss=W("rowloss"), rownll=W("rownll"), lse=W("lse")),
    "lm_loss_bwd": dict(dlogits=W("dlogits")),
    "pg_loss_fwd": dict(rowloss=W("rowloss"), rownll=W("rownll"), lse=W("lse"), ent=W("ent")),
    "pg_loss_bwd": dict(dlogits=W("dlogits")),
    "pg_kl_loss_fwd": dict(rowloss=W("rowloss"), rownll=W("rownll"), lse=W("lse"), ent=W("ent"), kl=W("kl"), ref_lse=W("ref_lse")),
    "pg_kl_loss_bwd": dict(dlogits=W("dlogits")),
    "distill_loss_fwd": dict(rowloss=W("rowloss"), rownll=W("rownll"), lse=W("lse"), lse_t=W("lse_t"), ref_lse_t=W("ref_lse_t"),
                             kd=W("kd")),
    "distill_loss_bwd": dict(dlogits=W("dlogits")),
    "seq_pref": {"adv": W("adv"), "seq_score": W("seq_score"), "seq_prob": W("seq_prob"), "group_loss": W("group_loss"),
                 "alive_inv": W("alive_inv"), "workspace": W("workspace"), NEW: W("workspace")},
    "kl_loss_fwd": dict(rowloss=W("rowloss"), lse=W("lse")),
    "kl_loss_bwd": dict(dpred=W("dpred")),
    "mse_loss_fwd": dict(rowloss=W("rowloss")),
    "mse_loss_bwd": dict(dpred=W("dpred")),
    "nsp_loss_fwd": dict(loss=W("loss")),
    "nsp_loss_bwd": dict(dlogits=W("dlogits")),
    # ---- optimizer
    "adamw_step": dict(p=W("p"), m=W("m"), v=W("v"), w16=W("w16"),
                       g=W("g", "zeroed in place under zero_grad; stated as a write for every call (a read of the gradients "
                                "conflicts with the same launches: every one that writes or accumulates them)")),
    "grad_norm": dict(workspace=W("workspace"), state=W("state")),
    "neural_ndcg": {NEW: W("ndcg alive dpred iters")},
    # ---- fp32x3
    "x3_split": dict(out32=W("out32"), out3=W("out3")),
    "x3_split_wt": dict(dst=W("dst")),
    # blocks_out: as layernorm_bwd_partials
    "x3_layernorm_bwd_partials": {"dx32": W("dx32"), "dxd3": W("dxd3"), "partials": W("partials"), HOST_OUT: W("blocks_out")},
    "embed_bwd_f32": dict(_EMB_BWD),
    "x3_lm_loss_bwd": dict(out3=W("out3")),
    "x3_kl_loss_bwd": dict(out3=W("out3")),
    "x3_rows_add": dict(dst=W("dst")),
    "x3_attn_fwd": dict(out=W("out"), lse=W("lse"), out3=W("out3")),
    "x3_attn_bwd": dict(delta=W("delta"),
                        dq=W("dq dq3", "with planes: the view's columns in all three planes of the split buffer, not in plane 0 alone"),
                        dk=W("dk dk3", "as dq"), dv=W("dv dv3", "as dq"),
                        extent=dict(dq=_x3_planes("dq"), dk=_x3_planes("dk"), dv=_x3_planes("dv"))),
    "x3_layernorm_fwd": dict(y32=W("y32"), y3=W("y3"), mean=W("mean"), rstd=W("rstd")),
    # ---- host-side staging (not streamed: they run on the calling thread and sit on the host timeline)
    "host_mask_pack": {"out": W("out"), NEW: W("out"), "timeline": HOST_TIMELINE},
    "host_copy": {"dst": W("dst"), "timeline": HOST_TIMELINE},
}

_RESERVED = ("members", "extent", "timeline")


def symbols_of(fn, names):
    """The C entry points (among `names`) a wrapper's source names."""
    return [s for s in dict.fromkeys(re.findall(r"unimm_\w+", inspect.getsource(fn))) if s in names]


def declared_abi_names(entry):
    """The header pointer names an entry declares written (members of list parameters are struct fields: not included)."""
    out = []
    for k, v in entry.items():
        if k not in _RESERVED:
            out += v[1].split()
    return set(out)


def accesses(name, bound, created=()):
    """The accesses of one call of wrapper `name`: bound = its arguments by parameter name (defaults applied), created = the
    tensors allocated while it ran.  -> [(access tuple, tensor)]"""
    entry = TABLE[name]
    members, finer = entry.get("members", {}), entry.get("extent", {})
    out = []

    def add(t, kind, param=None):
        ext = finer[param](t, kind, bound) if param in finer else extent(t, kind)
        if isinstance(ext, list):
            out.extend(ext)
        elif ext is not None:
            out.append(ext)

    for param, value in bound.items():
        if value is None:
            continue
        if param in members:
            for t, kind in members[param](value):
                add(t, kind)
            if is_tensor(value):
                add(value, "R")
            continue
        spec = entry.get(param)
        kind = "R" if spec is None else (spec[0](bound) if callable(spec[0]) else spec[0])
        for t in tensors_in(value):
            add(t, kind, param)
    if NEW in entry:
        for t in created:
            add(t, entry[NEW][0])
    return out
