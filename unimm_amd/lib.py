"""ctypes binding of libunimm_hip.so (the C ABI in include/unimm_hip.h).

There is no CPU fallback: if the library is missing or a kernel call fails, this raises.
PyTorch is used only for device memory and streams; every compute call below goes straight to a
hand-written HIP kernel on torch's current stream.
A new entry point goes in three places: its prototype in the header, its row in `SIGNATURES` (and, for a new argument struct, its
class in `STRUCTS`) and its wrapper function; tests/test_abi.py fails until the first two agree."""
from __future__ import annotations

import ctypes as C
import os
import threading

import torch

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "libunimm_hip.so")
ABI_VERSION = 24

EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_DROP_RESID, EPI_BIAS_RELU, EPI_DGELU, EPI_ADD, EPI_MUL, EPI_BIAS_GELU_DG = range(8)

_ERR = {-1: "UNIMM_E_ARG", -2: "UNIMM_E_SHAPE", -3: "UNIMM_E_ALIGN", -4: "UNIMM_E_HIP"}


class UnimmHipError(RuntimeError):
    pass


# Every entry point include/unimm_hip.h declares, in header order: name -> (result type, argument types).  A pointer of any kind is
# VP; tests/test_abi.py compares each row with the header's prototype and the .so's exports with the keys.
VP, I32, U32, F32, I64, _INT = C.c_void_p, C.c_int32, C.c_uint32, C.c_float, C.c_int64, C.c_int
_DROP = [U32, U32, F32]                                             # a dropout triple: key, threshold, scale
_LM_ROWS = [VP, I32, I32, I32, VP, I32, VP, I32]                    # logits, rows, V, ldl, banned, nbanned, flags, sep
SIGNATURES = {
    "unimm_version": (_INT, []),
    "unimm_arch": (C.c_char_p, []),
    "unimm_gemm_nt": (_INT, [VP, VP]),
    "unimm_gemm_tn": (_INT, [VP, VP]),
    "unimm_gemm_tn_grouped": (_INT, [VP, I32, VP]),
    "unimm_gemm_tn_grouped_ws": (_INT, [VP, I32, I32, VP, I64, VP]),
    "unimm_attn_fwd": (_INT, [VP, VP]),
    "unimm_attn_probs": (_INT, [VP, VP, VP]),
    "unimm_attn_bwd": (_INT, [VP, VP]),
    "unimm_attn_spliced_fwd": (_INT, [VP, VP]),
    "unimm_attn_spliced_bwd": (_INT, [VP, VP]),
    "unimm_attn_spliced_wide_fwd": (_INT, [VP, VP]),
    "unimm_attn_spliced_wide_bwd": (_INT, [VP, VP]),
    # row kernels
    "unimm_mask_pack": (_INT, [VP, _INT, VP, I64, I32, VP]),
    "unimm_host_mask_pack": (_INT, [VP, _INT, VP, I64, I32, I32]),
    "unimm_host_memcpy": (_INT, [VP, VP, I64, I32]),
    "unimm_mask_synth": (_INT, [VP] * 5 + [I32, I32, VP]),
    "unimm_plan_lengths": (_INT, [VP, I32, I32, VP, I32, I32, I32, VP, VP, VP, VP, I32, I32, VP, VP]),
    "unimm_plan_build": (_INT, [VP] * 3 + [I32, I32] + [VP] * 8 + [I32, I32] + [VP] * 4),
    "unimm_layernorm_fwd": (_INT, [VP] * 7 + [I32, I32, F32] + _DROP + [VP, VP]),
    "unimm_colpartials_bytes": (I64, [I32]),
    "unimm_layernorm_bwd": (_INT, [VP] * 11 + [I32, I32] + _DROP + _DROP + [VP, VP, VP]),
    "unimm_layernorm_bwd_partials": (_INT, [VP] * 8 + [I32, I32] + _DROP + _DROP + [VP] * 5),
    "unimm_colpartials_finish_grouped": (_INT, [VP, I32, VP]),
    "unimm_embed_fwd": (_INT, [VP] * 4),
    "unimm_embed_bwd": (_INT, [VP] * 10),
    "unimm_embed_bwd_rows": (_INT, [VP] * 8),
    "unimm_rows_scatter_sum_f32": (_INT, [VP, VP, VP, I32, I32, VP, I32, VP]),
    "unimm_colsum": (_INT, [VP, VP, I32, I32, I32, VP]),
    "unimm_cast_f32_bf16": (_INT, [VP, VP, I64, VP]),
    "unimm_transpose_cast": (_INT, [VP, VP, I32, I32, I32, VP]),
    "unimm_transpose_bf16": (_INT, [VP, VP, I32, I32, I32, I32, VP]),
    "unimm_sum_slabs_bf16": (_INT, [VP, I32, I64, VP, I64, VP]),
    "unimm_segment_rows_sum_bf16": (_INT, [VP, I32, VP, VP, I32, I32, VP, I32, I32, I32, VP]),
    "unimm_transpose_cast_grouped": (_INT, [VP, I32, I32, VP]),
    "unimm_pack_image": (_INT, [VP, VP, VP, I32, I32, I32, VP]),
    "unimm_mul_dropout": (_INT, [VP] * 3 + [I64] + _DROP + [VP, VP]),
    "unimm_mul_dropout_bwd": (_INT, [VP] * 5 + [I64] + _DROP + [VP, VP]),
    "unimm_sum_dropout": (_INT, [VP] * 3 + [I64] + _DROP + [VP, VP]),
    "unimm_sum_dropout_bwd": (_INT, [VP] * 5 + [I64] + _DROP + [VP, VP]),
    "unimm_linear_f32": (_INT, [VP, VP]),
    "unimm_rows_add_f32": (_INT, [VP, VP, VP, I32, I32, VP]),
    "unimm_gelu_bwd": (_INT, [VP, VP, VP, I64, VP]),
    "unimm_gather_rows": (_INT, [VP, VP, VP, I32, I32, I32, VP, VP]),
    # losses
    "unimm_lm_loss_fwd": (_INT, [VP] * 6 + [I32] * 3 + [VP, VP]),
    "unimm_lm_loss_bwd": (_INT, [VP] * 5 + [F32, VP] + [I32] * 4 + [VP, VP, VP]),
    "unimm_pg_loss_fwd": (_INT, [VP] * 5 + [I32, I32, F32, F32] + [VP] * 4 + [I32] * 3 + [VP, VP]),
    "unimm_pg_loss_bwd": (_INT, [VP] * 5 + [I32, I32, F32, F32, VP, VP, VP, F32, VP] + [I32] * 4 + [VP, VP, VP]),
    "unimm_pg_kl_loss_fwd": (_INT, [VP] * 5 + [I32, I32, F32, F32] + [VP] * 4 + [I32] * 3 + [VP, VP, I32, F32, VP, VP, VP]),
    "unimm_pg_kl_loss_bwd": (_INT, [VP] * 5 + [I32, I32, F32, F32, VP, VP, VP, F32, VP] + [I32] * 4 +
                             [VP, VP, VP, I32, F32, VP, VP, VP]),
    "unimm_distill_loss_fwd": (_INT, [VP] * 4 + [I32, F32, F32] + [VP] * 6 + [I32] * 3 + [VP, VP]),
    "unimm_distill_loss_bwd": (_INT, [VP] * 4 + [I32, F32, F32] + [VP] * 4 + [F32, VP] + [I32] * 4 + [VP, VP, VP]),
    "unimm_seq_pref": (_INT, [VP, VP]),
    "unimm_kl_loss_fwd": (_INT, [VP] * 5 + [I32] * 3 + [VP]),
    "unimm_kl_loss_bwd": (_INT, [VP] * 5 + [F32, VP] + [I32] * 4 + [VP, VP]),
    "unimm_mse_loss_fwd": (_INT, [VP] * 4 + [I32] * 3 + [VP]),
    "unimm_mse_loss_bwd": (_INT, [VP] * 4 + [F32, VP] + [I32] * 5 + [VP]),
    "unimm_nsp_loss_fwd": (_INT, [VP, VP, F32, F32, VP, I32, I32, VP]),
    "unimm_nsp_loss_bwd": (_INT, [VP, VP, F32, F32, VP, VP, VP, I32, I32, I32, VP]),
    "unimm_reduce_sum": (_INT, [VP, I64, VP, F32, VP, VP, VP]),
    "unimm_segment_sum": (_INT, [VP, VP, VP, I64, F32, VP]),
    "unimm_adamw_step": (_INT, [VP, VP]),
    "unimm_grad_norm": (_INT, [VP, VP, I64, I32, F32, C.c_double, VP, I64, VP, VP]),
    "unimm_adamw_step_clipped": (_INT, [VP, VP, I32, VP]),
    "unimm_neural_ndcg": (_INT, [VP, VP]),
    # the fp32-accuracy mode (csrc/x3ops.hip)
    "unimm_x3_split": (_INT, [VP, VP]),
    "unimm_x3_split_wt": (_INT, [VP, VP, I32, I32, I32, I32, VP]),
    "unimm_x3_layernorm_bwd_partials": (_INT, [VP] * 8 + [I32, I32] + _DROP + _DROP + [VP] * 4),
    "unimm_x3_layernorm_fwd": (_INT, [VP] * 7 + [I32, I32, F32] + _DROP + [VP, VP]),
    "unimm_embed_bwd_f32": (_INT, [VP] * 10),
    "unimm_x3_lm_loss_bwd": (_INT, [VP] * 5 + [F32, VP] + [I32] * 4 + [VP, VP, VP]),
    "unimm_x3_kl_loss_bwd": (_INT, [VP] * 5 + [F32, VP] + [I32] * 4 + [VP, VP]),
    "unimm_x3_rows_add": (_INT, [VP, VP, VP, I32, I32, I32, VP]),
    "unimm_x3_attn_fwd": (_INT, [VP, VP, VP]),
    "unimm_x3_attn_bwd": (_INT, [VP, VP, VP]),
    "unimm_x3_attn_set_impl": (_INT, [I32]),
    # answer generation (csrc/generate.hip)
    "unimm_attn_decode": (_INT, [VP, VP]),
    "unimm_kv_cache_update": (_INT, [VP, VP]),
    "unimm_attn_verify": (_INT, [VP, VP]),
    "unimm_kv_cache_append": (_INT, [VP, VP]),
    "unimm_lm_topk": (_INT, _LM_ROWS + [I32, VP, VP, VP, VP]),
    "unimm_lm_sample": (_INT, _LM_ROWS + [F32, I32, F32, U32] + [VP] * 6),
    "unimm_lm_sample_rows": (_INT, _LM_ROWS + [VP, VP, VP, U32] + [VP] * 6),
    "unimm_lm_topk_hist": (_INT, _LM_ROWS + [I32, VP, VP, VP, VP, VP]),
    "unimm_lm_sample_hist": (_INT, _LM_ROWS + [VP, VP, VP, U32] + [VP] * 7),
    "unimm_lm_spec_verify": (_INT, [VP, VP]),
    # launch profiler
    "unimm_prof_enable": (_INT, [I32]),
    "unimm_prof_collect": (_INT, [VP, VP, VP, I32]),
    "unimm_prof_tag": (_INT, [I32]),
    "unimm_prof_tagged": (_INT, [VP, VP, VP, VP, I32]),
}
SYMBOLS = list(SIGNATURES)
_STREAMED = {name for name, (_, args) in SIGNATURES.items() if args and args[-1] is VP}    # the only trailing pointer: `void* stream`


class GemmNtArgs(C.Structure):
    _fields_ = [("x", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("aux", C.c_void_p),
                ("out", C.c_void_p), ("out2", C.c_void_p),
                ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
                ("ldx", C.c_int32), ("ldw", C.c_int32), ("ldaux", C.c_int32), ("ldo", C.c_int32),
                ("epilogue", C.c_int32), ("out_f32", C.c_int32),
                ("drop_key", C.c_uint32), ("drop_thr", C.c_uint32), ("drop_scale", C.c_float),
                ("aux_mean", C.c_void_p), ("aux_rstd", C.c_void_p), ("aux_gamma", C.c_void_p), ("aux_beta", C.c_void_p),
                ("tile", C.c_int32), ("drop_salt", C.c_void_p),
                ("splitk_ws", C.c_void_p), ("splitk_ws_bytes", C.c_int64), ("splitk", C.c_int32),
                ("drop_rows", C.c_void_p), ("aux_rows", C.c_void_p)]


class GemmTnArgs(C.Structure):
    _fields_ = [("dy", C.c_void_p), ("x", C.c_void_p), ("dw", C.c_void_p), ("dbias", C.c_void_p),
                ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
                ("lddy", C.c_int32), ("ldx", C.c_int32), ("lddw", C.c_int32), ("m_dev", C.c_void_p), ("overwrite", C.c_int32)]


_lib = None


def lib():
    """Load the shared library once; fail loudly when it is absent (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("UNIMM_HIP_LIB", LIB_PATH)      # A/B runs of two builds in one process tree (tools only)
    if not os.path.exists(path):
        raise UnimmHipError(
            f"{path} is missing: build it with `python -m unimm_amd.build` (hipcc, gfx950). "
            "unimm_amd has no CPU or PyTorch fallback for its kernels.")
    L = C.CDLL(path)
    if L.unimm_version() != ABI_VERSION:
        raise UnimmHipError(f"libunimm_hip.so ABI {L.unimm_version()} != expected {ABI_VERSION}: rebuild")
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def _check(rc, what):
    if rc != 0:
        raise UnimmHipError(f"{what} failed: {_ERR.get(rc, rc)}")


_tls = threading.local()      # per thread: argument structs of the hot wrappers (the C side reads them before it returns)
                              # and the raw stream of the innermost stream_scope() (None = ask torch on every call)


def scoped_stream():
    """The raw stream object the calling thread's innermost `stream_scope` installed, or None."""
    return getattr(_tls, "stream", None)


def _stream():
    s = getattr(_tls, "stream", None)
    if s is not None:
        return s
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class stream_scope:
    """`with stream_scope(stream):` pins the stream every launch inside the block goes to (the block must also run
    under `torch.cuda.stream(stream)` / on that current stream for torch's own ops).  The engine brackets forward and
    backward with it: `torch.cuda.current_stream()` costs ~4 us and was asked ~240 times per step."""

    def __init__(self, stream):
        self.ptr = C.c_void_p(stream.cuda_stream)         # an object of its own: the engine tells scopes apart by its identity

    def __enter__(self):
        self.old, _tls.stream = getattr(_tls, "stream", None), self.ptr
        return self

    def __exit__(self, *exc):
        _tls.stream = self.old
        return False


def _call(name, *args):
    """One cold entry point by name, on the current stream where its prototype ends in one; a failure is raised under that name."""
    fn = getattr(lib(), name)
    _check(fn(*args, _stream()) if name in _STREAMED else fn(*args), name)


def _ptr(t):
    """raw address of a tensor's data (None = NULL): what a c_void_p argument or struct field takes"""
    return t.data_ptr() if t is not None else None


def _salt(*drops):
    """Device address of the salt word a dropout triple may carry as a 4th element: (key, thr, scale[, salt tensor])."""
    for d in drops:
        if d is not None and len(d) > 3 and d[3] is not None:
            return d[3].data_ptr()
    return None


def _dev(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise UnimmHipError("unimm_amd kernels need device tensors (got a CPU tensor)")


def gemm_nt(x, w, out, bias=None, epilogue=EPI_BIAS, aux=None, out2=None, drop=None, M=None, N=None, K=None, aux_ln=None, tile=0,
            splitk=0, splitk_ws=None, drop_rows=None, aux_rows=None):
    """out[M,N] = epi(x[M,K] @ w[N,K]^T).  x/w bf16 2-D (row stride = stride(0)); out bf16 or fp32.
    aux_ln = (mean[M], rstd[M], gamma[N], beta[N]): the DROP_RESID residual is LayerNorm(aux) computed on the fly.
    tile: per-call tuning code (include/unimm_hip.h: unimm_gemm_nt_args.tile); 0 = automatic.
    drop_rows / aux_rows (int32 [M], DROP_RESID): the rows whose dropout mask output row m draws / whose residual it reads."""
    _dev(x, w, out, bias, aux, out2, drop_rows, aux_rows)
    st = getattr(_tls, "nt", None)
    if st is None:
        a = GemmNtArgs()
        st = _tls.nt = (a, C.addressof(a), lib().unimm_gemm_nt)
    a, addr, fn = st
    a.x, a.w, a.out = x.data_ptr(), w.data_ptr(), out.data_ptr()
    a.bias = bias.data_ptr() if bias is not None else None
    a.out2 = out2.data_ptr() if out2 is not None else None
    if aux is not None:
        a.aux, a.ldaux = aux.data_ptr(), aux.stride(0)
    else:
        a.aux, a.ldaux = None, 0
    a.M = x.shape[0] if M is None else M
    a.N = w.shape[0] if N is None else N
    a.K = x.shape[1] if K is None else K
    a.ldx, a.ldw, a.ldo = x.stride(0), w.stride(0), out.stride(0)
    a.epilogue = epilogue
    a.tile = tile
    a.out_f32 = 1 if out.dtype == torch.float32 else 0
    a.drop_key, a.drop_thr, a.drop_scale = drop[:3] if drop is not None else (0, 0, 0.0)
    a.drop_salt = _salt(drop)
    if splitk_ws is not None and splitk not in (0, 1):          # (see include/unimm_hip.h: unimm_gemm_nt_args.splitk)
        a.splitk, a.splitk_ws, a.splitk_ws_bytes = splitk, splitk_ws.data_ptr(), splitk_ws.numel() * splitk_ws.element_size()
    else:
        a.splitk, a.splitk_ws, a.splitk_ws_bytes = 0, None, 0
    if aux_ln is not None:
        _dev(*aux_ln)
        a.aux_mean, a.aux_rstd, a.aux_gamma, a.aux_beta = (t.data_ptr() for t in aux_ln)
    else:
        a.aux_mean = a.aux_rstd = a.aux_gamma = a.aux_beta = None
    a.drop_rows = drop_rows.data_ptr() if drop_rows is not None else None
    a.aux_rows = aux_rows.data_ptr() if aux_rows is not None else None
    rc = fn(addr, _stream())
    if rc != 0:
        _check(rc, "unimm_gemm_nt")
    return out


def gemm_tn(dy, x, dw, M=None, N=None, K=None, dbias=None, m_dev=None):
    """dw[N,K] += dy[M,N]^T @ x[M,K] (fp32 atomics); dbias[N] += colsum(dy) when given.
    m_dev: int32 device word with the rows actually present (M is then a capacity)."""
    _dev(dy, x, dw, dbias, m_dev)
    a = GemmTnArgs()
    a.dy, a.x, a.dw, a.dbias, a.m_dev = _ptr(dy), _ptr(x), _ptr(dw), _ptr(dbias), _ptr(m_dev)
    a.M = dy.shape[0] if M is None else M
    a.N = dy.shape[1] if N is None else N
    a.K = x.shape[1] if K is None else K
    a.lddy, a.ldx, a.lddw = dy.stride(0), x.stride(0), dw.stride(0)
    _call("unimm_gemm_tn", C.byref(a))
    return dw


def gemm_tn_grouped(problems, shared=None, ws=None):
    """problems: list of (dy, x, dw, M, N, K, dbias[, m_dev[, overwrite]]) -- every dw[N,K] += dy[:M,:N]^T @ x[:M,:K] in as few
    launches as possible (one per <= 48 problems of the same tile class: csrc/gemm.hip TN_MAXG).  overwrite: dw is known to be zero and has no other
    contributor -> plain stores instead of atomics (unimm_gemm_tn_args.overwrite).
    shared: the launches run beside another stream's kernels (split heuristic hint; None = the process-wide default).
    ws: zero-initialised uint8 device tensor private to the launch stream (partial-tile slabs + arrival counters);
    None = every split adds its partial tile with fp32 atomics."""
    n = len(problems)
    if n == 0:
        return
    arr = (GemmTnArgs * n)()
    for a, (dy, x, dw, M, N, K, dbias, *rest) in zip(arr, problems):
        _dev(dy, x, dw, dbias)
        a.dy, a.x, a.dw, a.dbias = dy.data_ptr(), x.data_ptr(), dw.data_ptr(), _ptr(dbias)
        a.m_dev = _ptr(rest[0]) if rest else None
        a.overwrite = 1 if (len(rest) > 1 and rest[1]) else 0
        a.M = dy.shape[0] if M is None else M
        a.N = dy.shape[1] if N is None else N
        a.K = x.shape[1] if K is None else K
        a.lddy, a.ldx, a.lddw = dy.stride(0), x.stride(0), dw.stride(0)
    if shared is None and ws is None:
        _call("unimm_gemm_tn_grouped", C.addressof(arr), n)
        return
    _call("unimm_gemm_tn_grouped_ws", C.addressof(arr), n, int(shared or 0), _ptr(ws), ws.numel() if ws is not None else 0)


# ---------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------
class AttnArgs(C.Structure):
    _fields_ = [("q", C.c_void_p), ("k", C.c_void_p), ("v", C.c_void_p), ("out", C.c_void_p),
                ("lse", C.c_void_p), ("mask", C.c_void_p),
                ("q_off", C.c_void_p), ("q_len", C.c_void_p), ("k_off", C.c_void_p), ("k_len", C.c_void_p),
                ("B", C.c_int32), ("H", C.c_int32), ("Tq", C.c_int32), ("Tk", C.c_int32), ("D", C.c_int32),
                ("ldq", C.c_int32), ("ldk", C.c_int32), ("ldv", C.c_int32), ("ldo", C.c_int32),
                ("mask_q_stride", C.c_int32), ("mask_b_stride", C.c_int32), ("scale", C.c_float),
                ("drop_key", C.c_uint32), ("drop_thr", C.c_uint32), ("drop_scale", C.c_float), ("drop_salt", C.c_void_p),
                ("ks_off", C.c_void_p), ("ks_len", C.c_void_p), ("ks_ins", C.c_int32), ("order", C.c_void_p)]


class AttnBwdArgs(C.Structure):
    _fields_ = [("q", C.c_void_p), ("k", C.c_void_p), ("v", C.c_void_p), ("out", C.c_void_p), ("dout", C.c_void_p),
                ("lse", C.c_void_p), ("delta", C.c_void_p),
                ("dq", C.c_void_p), ("dk", C.c_void_p), ("dv", C.c_void_p), ("mask", C.c_void_p),
                ("q_off", C.c_void_p), ("q_len", C.c_void_p), ("k_off", C.c_void_p), ("k_len", C.c_void_p),
                ("B", C.c_int32), ("H", C.c_int32), ("Tq", C.c_int32), ("Tk", C.c_int32), ("D", C.c_int32),
                ("ldq", C.c_int32), ("ldk", C.c_int32), ("ldv", C.c_int32), ("ldo", C.c_int32), ("lddo", C.c_int32),
                ("lddq", C.c_int32), ("lddk", C.c_int32), ("lddv", C.c_int32),
                ("mask_q_stride", C.c_int32), ("mask_b_stride", C.c_int32), ("scale", C.c_float),
                ("drop_key", C.c_uint32), ("drop_thr", C.c_uint32), ("drop_scale", C.c_float), ("drop_salt", C.c_void_p),
                ("order", C.c_void_p)]


class AttnSplicedBwdArgs(C.Structure):
    _fields_ = AttnBwdArgs._fields_ + [("ks_off", C.c_void_p), ("ks_len", C.c_void_p), ("ks_ins", C.c_int32),
                                       ("g_first", C.c_void_p), ("g_seq", C.c_void_p), ("G", C.c_int32), ("accumulate", C.c_int32)]


def _item_order(qvar, kvar):
    """The item order of an attention launch (unimm_attn_args.order): element 3 of a variable-length descriptor, if it has one."""
    for v in (qvar, kvar):
        if v is not None and len(v) > 3 and v[3] is not None:
            return v[3].data_ptr()
    return None


NO_DROP = (0, 0, 1.0)


def _attn_common(a, q, k, v, mask, B, H, Tq, Tk, D, scale, mask_q_stride, mask_b_stride, drop, qvar=None, kvar=None):
    """The fields `AttnArgs` and `AttnBwdArgs` share, for every attention wrapper (v = None: the launch reads no values)."""
    a.q, a.k, a.v, a.mask = q.data_ptr(), k.data_ptr(), _ptr(v), mask.data_ptr()
    a.q_off, a.q_len = (qvar[0].data_ptr(), qvar[1].data_ptr()) if qvar is not None else (None, None)
    a.k_off, a.k_len = (kvar[0].data_ptr(), kvar[1].data_ptr()) if kvar is not None else (None, None)
    a.order = _item_order(qvar, kvar)
    a.B, a.H, a.Tq, a.Tk, a.D = B, H, Tq, Tk, D
    a.ldq, a.ldk, a.ldv = q.stride(0), k.stride(0), (v.stride(0) if v is not None else 0)
    a.mask_q_stride, a.mask_b_stride, a.scale = mask_q_stride, mask_b_stride, scale
    a.drop_key, a.drop_thr, a.drop_scale = drop[:3]
    a.drop_salt = _salt(drop)


def attn_fwd(q, k, v, out, lse, mask, B, H, Tq, Tk, D, scale, mask_q_stride, mask_b_stride, drop=NO_DROP,
             qvar=None, kvar=None, kshared=None):
    """q/k/v/out: 2-D bf16 views [rows, >=H*D] (row stride = stride(0)); mask: packed uint32 words.
    qvar / kvar: (offsets, lengths) int32 [B] tensors for the variable-length layout, or None.
    kshared: (offsets, lengths, ins) -- a shared key/value segment spliced into every sequence's keys after its first `ins`
    private rows (unimm_attn_args.ks_*; needs kvar, inference only)."""
    _dev(q, k, v, out, lse, mask)
    st = getattr(_tls, "af", None)
    if st is None:
        a = AttnArgs()
        st = _tls.af = (a, C.addressof(a), lib().unimm_attn_fwd)
    a, addr, fn = st
    _attn_common(a, q, k, v, mask, B, H, Tq, Tk, D, scale, mask_q_stride, mask_b_stride, drop, qvar, kvar)
    a.out, a.lse, a.ldo = out.data_ptr(), _ptr(lse), out.stride(0)
    if kshared is not None:
        a.ks_off, a.ks_len, a.ks_ins = kshared[0].data_ptr(), kshared[1].data_ptr(), int(kshared[2])
    else:
        a.ks_off, a.ks_len, a.ks_ins = None, None, 0
    rc = fn(addr, _stream())
    if rc != 0:
        _check(rc, "unimm_attn_fwd")


def group_lists(gid, G=None):
    """Host lists that name the groups of a spliced backward launch (unimm_attn_spliced_bwd_args.g_first / g_seq): gid = one group
    index in 0 .. G - 1 per sequence -> (g_first int32 [G + 1], g_seq int32 [B]): the sequences group by group, each group's members
    in batch order."""
    import numpy as np
    gid = np.asarray(gid, dtype=np.int64).reshape(-1)
    G = int(gid.max()) + 1 if G is None else int(G)
    if gid.size == 0 or gid.min() < 0 or gid.max() >= G:
        raise ValueError("group_lists: one group index in [0, G) per sequence")
    g_seq = np.argsort(gid, kind="stable").astype(np.int32)
    g_first = np.concatenate([[0], np.cumsum(np.bincount(gid, minlength=G))]).astype(np.int32)
    return g_first, g_seq


def attn_spliced_fwd(q, k, v, out, lse, mask, B, H, Tq, Tk, D, scale, mask_q_stride, mask_b_stride, drop, qvar, kvar, kshared, wide=False):
    """attn_fwd with a shared key/value segment in its training form (unimm_attn_spliced_fwd): lse is written, dropout allowed.
    wide: unimm_attn_spliced_wide_fwd, up to 64 private rows per sequence."""
    _dev(q, k, v, out, lse, mask)
    a = AttnArgs()
    _attn_common(a, q, k, v, mask, B, H, Tq, Tk, D, scale, mask_q_stride, mask_b_stride, drop, qvar, kvar)
    a.out, a.lse, a.ldo = out.data_ptr(), _ptr(lse), out.stride(0)
    a.ks_off, a.ks_len, a.ks_ins = _ptr(kshared[0]), _ptr(kshared[1]), int(kshared[2])
    _call("unimm_attn_spliced_wide_fwd" if wide else "unimm_attn_spliced_fwd", C.byref(a))


def spliced_bwd_args(q, k, v, out, dout, lse, dq, dk, dv, mask, B, H, Tq, Tk, D, scale, mask_q_stride, mask_b_stride, drop, qvar, kvar,
                     kshared, groups, accumulate=False):
    """The argument struct of `attn_spliced_bwd` (groups = (g_first int32 [G + 1], g_seq int32 [B]) device tensors)."""
    a = AttnSplicedBwdArgs()
    _attn_common(a, q, k, v, mask, B, H, Tq, Tk, D, scale, mask_q_stride, mask_b_stride, drop, qvar, kvar)
    a.order = None                                  # a workgroup is a (group, head): the sequence order does not apply
    a.out, a.dout, a.lse, a.delta = out.data_ptr(), dout.data_ptr(), _ptr(lse), None
    a.dq, a.dk, a.dv = dq.data_ptr(), dk.data_ptr(), dv.data_ptr()
    a.ldo, a.lddo = out.stride(0), dout.stride(0)
    a.lddq, a.lddk, a.lddv = dq.stride(0), dk.stride(0), dv.stride(0)
    a.ks_off, a.ks_len, a.ks_ins = _ptr(kshared[0]), _ptr(kshared[1]), int(kshared[2])
    a.g_first, a.g_seq = _ptr(groups[0]), _ptr(groups[1])
    a.G = (groups[0].numel() - 1) if groups[0] is not None else 0
    a.accumulate = 1 if accumulate else 0
    return a


def attn_spliced_bwd(q, k, v, out, dout, lse, dq, dk, dv, mask, B, H, Tq, Tk, D, scale, mask_q_stride, mask_b_stride, drop, qvar, kvar,
                     kshared, groups, accumulate=False, wide=False):
    """Backward of `attn_spliced_fwd` (unimm_attn_spliced_bwd): dq of the private queries, dk / dv of the private keys and -- summed
    over each group's sequences in fp32, rounded once; accumulate: on top of what the rows hold -- of the groups' shared rows.
    wide: unimm_attn_spliced_wide_bwd, up to 64 private rows per sequence."""
    _dev(q, k, v, out, dout, lse, dq, dk, dv, mask, *groups)
    a = spliced_bwd_args(q, k, v, out, dout, lse, dq, dk, dv, mask, B, H, Tq, Tk, D, scale, mask_q_stride, mask_b_stride, drop, qvar,
                         kvar, kshared, groups, accumulate)
    _call("unimm_attn_spliced_wide_bwd" if wide else "unimm_attn_spliced_bwd", C.byref(a))


class AttnDecodeArgs(C.Structure):
    _fields_ = [("q", C.c_void_p), ("k", C.c_void_p), ("v", C.c_void_p), ("out", C.c_void_p),
                ("ctx_k", C.c_void_p), ("ctx_v", C.c_void_p), ("ctx_off", C.c_void_p), ("ctx_len", C.c_void_p),
                ("priv_k", C.c_void_p), ("priv_v", C.c_void_p), ("plen", C.c_void_p),
                ("G", C.c_int32), ("beams", C.c_int32), ("nr", C.c_int32), ("H", C.c_int32), ("D", C.c_int32), ("pcap", C.c_int32),
                ("ldq", C.c_int32), ("ldk", C.c_int32), ("ldv", C.c_int32), ("ldo", C.c_int32), ("ldc", C.c_int32), ("ldp", C.c_int32),
                ("scale", C.c_float)]


class KvUpdateArgs(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("new_kv", C.c_void_p),
                ("parent", C.c_void_p), ("plen", C.c_void_p), ("plen_out", C.c_void_p),
                ("layers", C.c_int32), ("slots", C.c_int32), ("pcap", C.c_int32), ("ldp", C.c_int32), ("width", C.c_int32),
                ("new_layer_stride", C.c_int64), ("ld_new", C.c_int32), ("new_row_mul", C.c_int32)]


class KvAppendArgs(C.Structure):
    _fields_ = [("cache", C.c_void_p), ("new_kv", C.c_void_p), ("count", C.c_void_p), ("plen", C.c_void_p), ("plen_out", C.c_void_p),
                ("layers", C.c_int32), ("slots", C.c_int32), ("pcap", C.c_int32), ("ldp", C.c_int32), ("width", C.c_int32),
                ("max_count", C.c_int32),
                ("new_layer_stride", C.c_int64), ("ld_new", C.c_int32), ("new_row_mul", C.c_int32), ("new_row_step", C.c_int32)]


class LmSpecVerifyArgs(C.Structure):
    _fields_ = [("x", C.c_void_p), ("xd", C.c_void_p), ("draft_token", C.c_void_p),
                ("banned", C.c_void_p), ("flags", C.c_void_p), ("stream_ids", C.c_void_p),
                ("temperature", C.c_void_p), ("top_k", C.c_void_p), ("top_p", C.c_void_p),
                ("accept", C.c_void_p), ("token", C.c_void_p),
                ("logp", C.c_void_p), ("logq", C.c_void_p), ("lse", C.c_void_p), ("log_ratio", C.c_void_p),
                ("rows", C.c_int32), ("V", C.c_int32), ("ldl", C.c_int32), ("ldd", C.c_int32), ("nbanned", C.c_int32),
                ("sep", C.c_int32), ("key_accept", C.c_uint32), ("key_residual", C.c_uint32)]


def attn_decode(q, k, v, out, ctx_k, ctx_v, ctx_off, ctx_len, priv_k, priv_v, plen, G, beams, nr, H, pcap, scale, D=64):
    """Text self-attention of the decode rows (unimm_attn_decode): q / k / v / out / ctx_k / ctx_v are 2-D bf16 views (row stride =
    stride(0)); priv_k / priv_v: 2-D views whose row (slot * pcap + r) is cached answer row r of a slot (or None when pcap = 0)."""
    _dev(q, k, v, out, ctx_k, ctx_v, ctx_off, ctx_len, priv_k, priv_v, plen)
    a = AttnDecodeArgs()
    a.q, a.k, a.v, a.out = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()
    a.ctx_k, a.ctx_v, a.ctx_off, a.ctx_len = ctx_k.data_ptr(), ctx_v.data_ptr(), ctx_off.data_ptr(), ctx_len.data_ptr()
    a.priv_k, a.priv_v, a.plen = _ptr(priv_k), _ptr(priv_v), plen.data_ptr()
    a.G, a.beams, a.nr, a.H, a.D, a.pcap = G, beams, nr, H, D, pcap
    a.ldq, a.ldk, a.ldv, a.ldo, a.ldc = q.stride(0), k.stride(0), v.stride(0), out.stride(0), ctx_k.stride(0)
    if ctx_v.stride(0) != ctx_k.stride(0):
        raise UnimmHipError("attn_decode: ctx_k and ctx_v need one row stride")
    a.ldp = priv_k.stride(0) if priv_k is not None else 0
    if priv_v is not None and priv_v.stride(0) != a.ldp:
        raise UnimmHipError("attn_decode: priv_k and priv_v need one row stride")
    a.scale = scale
    _call("unimm_attn_decode", C.byref(a))


def kv_cache_update(src, dst, new_kv, parent, plen, plen_out, layers, slots, pcap, width, new_layer_stride, new_row_mul):
    """Private-cache append + reorder (unimm_kv_cache_update).  src / dst: bf16 [layers, slots, pcap, ldp]; new_kv: 2-D bf16 view
    (row stride = stride(0)) at the first K column of layer 0's new rows; the new answer row of slot p is row p * new_row_mul."""
    _dev(src, dst, new_kv, parent, plen, plen_out)
    a = KvUpdateArgs()
    a.src, a.dst, a.new_kv = src.data_ptr(), dst.data_ptr(), new_kv.data_ptr()
    a.parent, a.plen, a.plen_out = parent.data_ptr(), plen.data_ptr(), plen_out.data_ptr()
    a.layers, a.slots, a.pcap, a.ldp, a.width = layers, slots, pcap, src.shape[-1], width
    a.new_layer_stride, a.ld_new, a.new_row_mul = new_layer_stride, new_kv.stride(0), new_row_mul
    _call("unimm_kv_cache_update", C.byref(a))


def attn_verify(q, k, v, out, ctx_k, ctx_v, ctx_off, ctx_len, priv_k, priv_v, plen, G, beams, nr, H, pcap, scale, D=64):
    """unimm_attn_verify: the arguments of `attn_decode`; nr even, the new rows of a slot are nr / 2 (answer, copy) pairs."""
    _dev(q, k, v, out, ctx_k, ctx_v, ctx_off, ctx_len, priv_k, priv_v, plen)
    a = AttnDecodeArgs()
    a.q, a.k, a.v, a.out = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()
    a.ctx_k, a.ctx_v, a.ctx_off, a.ctx_len = ctx_k.data_ptr(), ctx_v.data_ptr(), ctx_off.data_ptr(), ctx_len.data_ptr()
    a.priv_k, a.priv_v, a.plen = _ptr(priv_k), _ptr(priv_v), plen.data_ptr()
    a.G, a.beams, a.nr, a.H, a.D, a.pcap = G, beams, nr, H, D, pcap
    a.ldq, a.ldk, a.ldv, a.ldo, a.ldc = q.stride(0), k.stride(0), v.stride(0), out.stride(0), ctx_k.stride(0)
    if ctx_v.stride(0) != ctx_k.stride(0):
        raise UnimmHipError("attn_verify: ctx_k and ctx_v need one row stride")
    a.ldp = priv_k.stride(0) if priv_k is not None else 0
    if priv_v is not None and priv_v.stride(0) != a.ldp:
        raise UnimmHipError("attn_verify: priv_k and priv_v need one row stride")
    a.scale = scale
    _call("unimm_attn_verify", C.byref(a))


def kv_cache_append(cache, new_kv, count, plen, plen_out, layers, slots, pcap, width, max_count, new_layer_stride, new_row_mul,
                    new_row_step):
    """unimm_kv_cache_append.  cache: bf16 [layers, slots, pcap, ldp]; new_kv: 2-D bf16 view (row stride = stride(0)) at the first
    K column of layer 0's new rows; new row j of slot s is row s * new_row_mul + j * new_row_step."""
    _dev(cache, new_kv, count, plen, plen_out)
    a = KvAppendArgs()
    a.cache, a.new_kv = cache.data_ptr(), new_kv.data_ptr()
    a.count, a.plen, a.plen_out = count.data_ptr(), plen.data_ptr(), plen_out.data_ptr()
    a.layers, a.slots, a.pcap, a.ldp, a.width, a.max_count = layers, slots, pcap, cache.shape[-1], width, max_count
    a.new_layer_stride, a.ld_new, a.new_row_mul, a.new_row_step = new_layer_stride, new_kv.stride(0), new_row_mul, new_row_step
    _call("unimm_kv_cache_append", C.byref(a))


def lm_topk(logits, rows, V, banned, flags, sep, K, vals, ids, lse=None):
    """log-softmax + top-K of fp32 logits [rows, >= V] (unimm_lm_topk): vals fp32 [rows, K], ids int32 [rows, K]."""
    _dev(logits, banned, flags, vals, ids, lse)
    nb = 0 if banned is None else banned.numel()
    _call("unimm_lm_topk", logits.data_ptr(), rows, V, logits.stride(0), _ptr(banned), nb, _ptr(flags), sep, K, vals.data_ptr(),
          ids.data_ptr(), _ptr(lse))


def lm_sample(logits, rows, V, banned, flags, sep, temperature, top_k, top_p, key, streams, token, logp, logq, lse=None):
    """One draw per row of fp32 logits [rows, >= V] after temperature / top-k / nucleus filtering (unimm_lm_sample): token int32
    [rows], logp (unmodified distribution) and logq (the one sampled from) fp32 [rows]; streams int32 [rows], key a 32-bit word."""
    _dev(logits, banned, flags, streams, token, logp, logq, lse)
    nb = 0 if banned is None else banned.numel()
    _call("unimm_lm_sample", logits.data_ptr(), rows, V, logits.stride(0), _ptr(banned), nb, _ptr(flags), sep, temperature, top_k,
          top_p, key & 0xFFFFFFFF, _ptr(streams), _ptr(token), _ptr(logp), _ptr(logq), _ptr(lse))


def lm_sample_rows(logits, rows, V, banned, flags, sep, temperature, top_k, top_p, key, streams, token, logp, logq, lse=None):
    """lm_sample with per-row decoding parameters (unimm_lm_sample_rows): temperature fp32 [rows], top_k int32 [rows], top_p fp32
    [rows] on the device.  A row with top_k = 1 is greedy (logq = 0); a row with invalid parameters returns token = -1."""
    _dev(logits, banned, flags, temperature, top_k, top_p, streams, token, logp, logq, lse)
    nb = 0 if banned is None else banned.numel()
    _call("unimm_lm_sample_rows", logits.data_ptr(), rows, V, logits.stride(0), _ptr(banned), nb, _ptr(flags), sep, _ptr(temperature),
          _ptr(top_k), _ptr(top_p), key & 0xFFFFFFFF, _ptr(streams), _ptr(token), _ptr(logp), _ptr(logq), _ptr(lse))


def lm_spec_verify(x, xd, rows, V, draft_token, banned, flags, sep, temperature, top_k, top_p, key_accept, key_residual, streams,
                   accept, token, logp, logq, lse, log_ratio=None):
    """unimm_lm_spec_verify: accept the draft's token of every row with probability min(1, P~ / Q~) or draw from the residual.
    x / xd: fp32 logits [rows, >= V] of the model and the draft (2-D views, row stride = stride(0)); draft_token int32 [rows]
    (-1: no draft, a plain draw keyed by key_residual); the rest as `lm_sample_rows`.  accept / token int32 [rows],
    logp / logq / lse (/ log_ratio) fp32 [rows]."""
    _dev(x, xd, draft_token, banned, flags, temperature, top_k, top_p, streams, accept, token, logp, logq, lse, log_ratio)
    a = LmSpecVerifyArgs()
    a.x, a.xd, a.draft_token = _ptr(x), _ptr(xd), _ptr(draft_token)
    a.banned, a.flags, a.stream_ids = _ptr(banned), _ptr(flags), _ptr(streams)
    a.temperature, a.top_k, a.top_p = _ptr(temperature), _ptr(top_k), _ptr(top_p)
    a.accept, a.token = _ptr(accept), _ptr(token)
    a.logp, a.logq, a.lse, a.log_ratio = _ptr(logp), _ptr(logq), _ptr(lse), _ptr(log_ratio)
    a.rows, a.V, a.ldl, a.ldd = rows, V, x.stride(0) if x is not None else 0, xd.stride(0) if xd is not None else 0
    a.nbanned, a.sep = 0 if banned is None else banned.numel(), sep
    a.key_accept, a.key_residual = key_accept & 0xFFFFFFFF, key_residual & 0xFFFFFFFF
    _call("unimm_lm_spec_verify", C.byref(a))


class LmHistory(C.Structure):
    _fields_ = [("hist", C.c_void_p), ("hist_len", C.c_void_p), ("ctx", C.c_void_p), ("ctx_len", C.c_void_p), ("ctx_idx", C.c_void_p),
                ("ldh", C.c_int32), ("nctx", C.c_int32), ("ldc", C.c_int32), ("ngram", C.c_int32), ("sep", C.c_int32),
                ("penalty", C.c_float), ("inv_penalty", C.c_float)]


def lm_history(hist, hist_len, ngram, penalty, sep, ctx=None, ctx_len=None, ctx_idx=None):
    """The per-row history of lm_topk_hist / lm_sample_hist (unimm_lm_history): hist int32 [rows, ldh] with hist_len int32 [rows],
    optionally a context table ctx int32 [nctx, ldc] with ctx_len int32 [nctx] and the rows' ctx_idx int32 [rows].  penalty is
    rounded to fp32 and inv_penalty is the fp32 value of 1 / that.  The struct holds addresses: keep the tensors alive."""
    _dev(hist, hist_len, ctx, ctx_len, ctx_idx)
    h = LmHistory()
    h.hist, h.hist_len, h.ctx, h.ctx_len, h.ctx_idx = _ptr(hist), _ptr(hist_len), _ptr(ctx), _ptr(ctx_len), _ptr(ctx_idx)
    h.ldh = hist.stride(0) if hist is not None else 0
    h.nctx, h.ldc = (ctx.shape[0], ctx.stride(0)) if ctx is not None else (0, 0)
    h.ngram, h.sep = ngram, sep
    h.penalty = penalty
    h.inv_penalty = 1.0 / h.penalty                 # 1 / (the fp32 penalty), rounded to fp32 by the field
    return h


def lm_topk_hist(logits, rows, V, banned, flags, sep, K, history, vals, ids, lse=None):
    """lm_topk with a per-row history (unimm_lm_topk_hist; history: lm_history): no-repeat n-gram bans, and under a repetition
    penalty the ids in the order of the penalised logits with their unpenalised log p."""
    _dev(logits, banned, flags, vals, ids, lse)
    nb = 0 if banned is None else banned.numel()
    _call("unimm_lm_topk_hist", logits.data_ptr(), rows, V, logits.stride(0), _ptr(banned), nb, _ptr(flags), sep, K,
          C.addressof(history), vals.data_ptr(), ids.data_ptr(), _ptr(lse))


def lm_sample_hist(logits, rows, V, banned, flags, sep, temperature, top_k, top_p, key, streams, history, token, logp, logq,
                   lse=None):
    """lm_sample_rows with a per-row history (unimm_lm_sample_hist; history: lm_history): the draw, and logq, under the
    no-repeat n-gram bans and the repetition penalty; logp stays that of the unmodified row."""
    _dev(logits, banned, flags, temperature, top_k, top_p, streams, token, logp, logq, lse)
    nb = 0 if banned is None else banned.numel()
    _call("unimm_lm_sample_hist", logits.data_ptr(), rows, V, logits.stride(0), _ptr(banned), nb, _ptr(flags), sep,
          _ptr(temperature), _ptr(top_k), _ptr(top_p), key & 0xFFFFFFFF, _ptr(streams), C.addressof(history), _ptr(token),
          _ptr(logp), _ptr(logq), _ptr(lse))


def attn_probs(q, k, probs, mask, B, H, Tq, Tk, D, scale, mask_q_stride, mask_b_stride, drop=NO_DROP):
    """probs: fp32 [B, H, Tq, Tk] = dropout(softmax(q k^T scale + additive mask)); fixed row layout (diagnostic output)."""
    _dev(q, k, probs, mask)
    a = AttnArgs()                  # out / lse / ldo / ks_* stay zero
    _attn_common(a, q, k, None, mask, B, H, Tq, Tk, D, scale, mask_q_stride, mask_b_stride, drop)
    _call("unimm_attn_probs", C.byref(a), _ptr(probs))


def attn_bwd(q, k, v, out, dout, lse, delta, dq, dk, dv, mask, B, H, Tq, Tk, D, scale, mask_q_stride,
             mask_b_stride, drop=NO_DROP, qvar=None, kvar=None):
    _dev(q, k, v, out, dout, lse, delta, dq, dk, dv, mask)
    st = getattr(_tls, "ab", None)
    if st is None:
        a = AttnBwdArgs()
        st = _tls.ab = (a, C.addressof(a), lib().unimm_attn_bwd)
    a, addr, fn = st
    _attn_common(a, q, k, v, mask, B, H, Tq, Tk, D, scale, mask_q_stride, mask_b_stride, drop, qvar, kvar)
    a.out, a.dout, a.lse, a.delta = out.data_ptr(), dout.data_ptr(), lse.data_ptr(), delta.data_ptr()
    a.dq, a.dk, a.dv = dq.data_ptr(), dk.data_ptr(), dv.data_ptr()
    a.ldo, a.lddo = out.stride(0), dout.stride(0)
    a.lddq, a.lddk, a.lddv = dq.stride(0), dk.stride(0), dv.stride(0)
    rc = fn(addr, _stream())
    if rc != 0:
        _check(rc, "unimm_attn_bwd")


# ---------------------------------------------------------------------------------------------
# row kernels
# ---------------------------------------------------------------------------------------------
_DT = {torch.bool: 0, torch.uint8: 0, torch.int32: 1, torch.int64: 2, torch.float32: 3}


def mask_pack(mask, out=None):
    """0/1 mask [..., T] -> uint32 words [..., ceil(T/32)] (stored in an int32 tensor)."""
    _dev(mask)
    if mask.dtype not in _DT:
        raise UnimmHipError(f"mask dtype {mask.dtype} not supported (bool, uint8, int32, int64, float32)")
    mask = mask.contiguous()
    t = mask.shape[-1]
    rows = mask.numel() // t
    nw = (t + 31) // 32
    if out is None:
        out = torch.empty(mask.shape[:-1] + (nw,), dtype=torch.int32, device=mask.device)
    _call("unimm_mask_pack", _ptr(mask), _DT[mask.dtype], _ptr(out), rows, t)
    return out


def host_mask_pack(mask, out=None, threads=0):
    """The words of `mask_pack` for a mask in HOST memory, computed on the host (unimm_host_mask_pack): 0/1 mask [..., T] ->
    int32 words [..., ceil(T/32)] in `out` (e.g. a pinned staging buffer) or a new CPU tensor."""
    if mask.is_cuda:
        raise UnimmHipError("host_mask_pack takes a CPU tensor (device masks: mask_pack)")
    if mask.dtype not in _DT:
        raise UnimmHipError(f"mask dtype {mask.dtype} not supported (bool, uint8, int32, int64, float32)")
    mask = mask.contiguous()
    t = mask.shape[-1]
    rows = mask.numel() // t
    nw = (t + 31) // 32
    if out is None:
        out = torch.empty(mask.shape[:-1] + (nw,), dtype=torch.int32)
    if out.is_cuda or out.dtype != torch.int32 or out.numel() != rows * nw or not out.is_contiguous():
        raise UnimmHipError("host_mask_pack: out must be a contiguous int32 CPU tensor of rows x ceil(T/32) words")
    _call("unimm_host_mask_pack", mask.data_ptr(), _DT[mask.dtype], out.data_ptr(), rows, t, threads)
    return out


def host_copy(dst, src, threads=0):
    """dst.copy_(src) for two CPU tensors of one shape and dtype, both contiguous, on several threads (unimm_host_memcpy);
    anything else falls back to torch's copy_."""
    if (dst.is_cuda or src.is_cuda or dst.dtype != src.dtype or dst.shape != src.shape or not dst.is_contiguous()
            or not src.is_contiguous() or src.numel() * src.element_size() < (8 << 20)):
        dst.copy_(src)
        return dst
    _call("unimm_host_memcpy", dst.data_ptr(), src.data_ptr(), src.numel() * src.element_size(), threads)
    return dst


def colpartials_bytes(H):
    return int(lib().unimm_colpartials_bytes(H))


class FinishDesc(C.Structure):
    _fields_ = [("partials", C.c_void_p), ("dst", C.c_void_p * 4), ("blocks", C.c_int32), ("nq", C.c_int32), ("H", C.c_int32),
                ("pad_", C.c_int32)]


def layernorm_bwd_partials(dy, x, mean, rstd, gamma, dx, dx_drop, partials, M, H, drop=None, out_drop=None, m_dev=None,
                           drop_rows=None):
    """LayerNorm backward row kernel only; returns the number of partial blocks (see unimm_layernorm_bwd_partials)."""
    drop = drop or NO_DROP
    out_drop = out_drop or NO_DROP
    _dev(dy, x, mean, rstd, gamma, dx, dx_drop, partials, drop_rows)
    blocks = C.c_int32(0)
    _call("unimm_layernorm_bwd_partials", dy.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(),
          dx.data_ptr(), _ptr(dx_drop), partials.data_ptr(), M, H, *drop[:3], *out_drop[:3], C.addressof(blocks), _ptr(m_dev),
          _salt(drop, out_drop), _ptr(drop_rows))
    return blocks.value


def colpartials_finish_grouped(pending):
    """pending: list of (partials, blocks, H, [dst tensors or None, up to 4]) -> their column sums added in one launch."""
    n = len(pending)
    if n == 0:
        return
    arr = (FinishDesc * n)()
    for d, (part, blocks, H, dsts) in zip(arr, pending):
        d.partials, d.blocks, d.nq, d.H = part.data_ptr(), blocks, len(dsts), H
        for q, t in enumerate(dsts):
            d.dst[q] = _ptr(t)
    _call("unimm_colpartials_finish_grouped", C.addressof(arr), n)


def layernorm_fwd(x, gamma, beta, y32, y16, mean, rstd, M, H, eps=1e-12, drop=NO_DROP):
    _dev(x, gamma, beta, y32, y16, mean, rstd)
    _call("unimm_layernorm_fwd", x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _ptr(y32), _ptr(y16), _ptr(mean), _ptr(rstd), M, H,
          eps, *drop[:3], _salt(drop))


def layernorm_bwd(dy, x, mean, rstd, gamma, dx, dx_drop, dgamma, dbeta, dbias, partials, M, H, drop=NO_DROP,
                  out_drop=NO_DROP, drop_rows=None):
    _dev(dy, x, mean, rstd, gamma, dx, dx_drop, dgamma, dbeta, dbias, partials, drop_rows)
    _call("unimm_layernorm_bwd", _ptr(dy), _ptr(x), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(dx), _ptr(dx_drop), _ptr(dgamma),
          _ptr(dbeta), _ptr(dbias), _ptr(partials), M, H, *drop[:3], *out_drop[:3], _salt(drop, out_drop), _ptr(drop_rows))


class EmbedArgs(C.Structure):
    _fields_ = [("ids", C.c_void_p), ("pos", C.c_void_p), ("typ", C.c_void_p),
                ("word", C.c_void_p), ("post", C.c_void_p), ("type", C.c_void_p), ("ext", C.c_void_p),
                ("gamma", C.c_void_p), ("beta", C.c_void_p),
                ("M", C.c_int32), ("H", C.c_int32), ("type_vocab", C.c_int32), ("eps", C.c_float),
                ("drop_key", C.c_uint32), ("drop_thr", C.c_uint32), ("drop_scale", C.c_float),
                ("m_dev", C.c_void_p), ("rows", C.c_void_p), ("drop_salt", C.c_void_p)]


def _embed_args(ids, pos, typ, word, post, type_, ext, gamma, beta, M, H, type_vocab, eps, drop, m_dev=None, rows=None):
    _dev(ids, pos, typ, word, post, type_, ext, gamma, beta, m_dev, rows)
    a = EmbedArgs()
    a.ids, a.pos, a.typ = _ptr(ids), _ptr(pos), _ptr(typ)
    a.word, a.post, a.type, a.ext = _ptr(word), _ptr(post), _ptr(type_), _ptr(ext)
    a.gamma, a.beta = _ptr(gamma), _ptr(beta)
    a.M, a.H, a.type_vocab, a.eps = M, H, type_vocab, eps
    a.drop_key, a.drop_thr, a.drop_scale = drop[:3]
    a.drop_salt = _salt(drop)
    a.m_dev, a.rows = _ptr(m_dev), _ptr(rows)
    return a


def embed_fwd(ids, pos, typ, word, post, type_, ext, gamma, beta, y32, y16, M, H, type_vocab=2, eps=1e-12, drop=NO_DROP,
              m_dev=None, rows=None):
    """rows (int64 [M]): row r embeds ids / pos / typ at index rows[r]; m_dev: int32 device word, rows actually present."""
    a = _embed_args(ids, pos, typ, word, post, type_, ext, gamma, beta, M, H, type_vocab, eps, drop, m_dev, rows)
    _dev(y32, y16)
    _call("unimm_embed_fwd", C.byref(a), _ptr(y32), _ptr(y16))


def embed_bwd(ids, pos, typ, word, post, type_, ext, gamma, beta, dy, dword, dpos, dtype, dext, dgamma, dbeta,
              partials, M, H, type_vocab=2, eps=1e-12, drop=NO_DROP, m_dev=None, rows=None):
    a = _embed_args(ids, pos, typ, word, post, type_, ext, gamma, beta, M, H, type_vocab, eps, drop, m_dev, rows)
    _dev(dy, dword, dpos, dtype, dext, dgamma, dbeta, partials)
    _call("unimm_embed_bwd", C.byref(a), _ptr(dy), _ptr(dword), _ptr(dpos), _ptr(dtype), _ptr(dext), _ptr(dgamma), _ptr(dbeta),
          _ptr(partials))


def embed_bwd_rows(ids, pos, typ, word, post, type_, ext, gamma, beta, dy, drow, dtype, dgamma, dbeta, partials, M, H,
                   type_vocab=2, eps=1e-12, drop=NO_DROP, rows=None):
    """embed_bwd without atomics: the rows' gradients are stored in drow (fp32 [M, H]); `rows_scatter_sum_f32` adds them up."""
    a = _embed_args(ids, pos, typ, word, post, type_, ext, gamma, beta, M, H, type_vocab, eps, drop, None, rows)
    _dev(dy, drow, dtype, dgamma, dbeta, partials)
    _call("unimm_embed_bwd_rows", C.byref(a), _ptr(dy), _ptr(drow), _ptr(dtype), _ptr(dgamma), _ptr(dbeta), _ptr(partials))


def rows_scatter_sum_f32(src, keys, order, dst):
    """dst[keys[j]] += src[order[j]] over each key's run, in a fixed order (keys ascending int32 [M], negative = skipped): one writer
    per destination row, no atomics (unimm_rows_scatter_sum_f32).  src fp32 [M, H], dst fp32 [n, H], both contiguous."""
    _dev(src, keys, order, dst)
    _call("unimm_rows_scatter_sum_f32", _ptr(src), _ptr(keys), _ptr(order), src.shape[0], src.shape[1], _ptr(dst), dst.shape[0])


def colsum(dy, db, M, N):
    _dev(dy, db)
    _call("unimm_colsum", _ptr(dy), _ptr(db), M, N, dy.stride(0))


def cast_f32_bf16(src, dst, n=None):
    _dev(src, dst)
    _call("unimm_cast_f32_bf16", _ptr(src), _ptr(dst), src.numel() if n is None else n)


def mask_synth(mode, length, nans, T):
    """Packed text mask [B, T, ceil(T/32)] and co-attention key mask [B, ceil(T/32)] from int32 descriptors."""
    _dev(mode, length, nans)
    B, nw = mode.numel(), (T + 31) // 32
    text = torch.empty((B, T, nw), dtype=torch.int32, device=mode.device)
    co = torch.empty((B, nw), dtype=torch.int32, device=mode.device)
    _call("unimm_mask_synth", _ptr(mode), _ptr(length), _ptr(nans), _ptr(text), _ptr(co), B, T)
    return text, co


def plan_lengths(text_mask, co_mask, R, labels, weights, nsp_weight, B, T, image_label=None):
    """-> int32 header [3B+2] on the device (see include/unimm_hip.h: unimm_plan_lengths).  text_mask / co_mask are
    (words, q_stride, b_stride) tuples or None."""
    tw, tq, tb = text_mask if text_mask is not None else (None, 0, 0)
    cw, cq, cb = co_mask if co_mask is not None else (None, 0, 0)
    ref = tw if tw is not None else (cw if cw is not None else labels)
    header = torch.zeros(3 * B + 2, dtype=torch.int32, device=ref.device)
    _dev(tw, cw, labels, weights, nsp_weight, image_label)
    _call("unimm_plan_lengths", _ptr(tw), tq, tb, _ptr(cw), cq, cb, R, _ptr(labels), _ptr(weights), _ptr(nsp_weight),
          _ptr(image_label), B, T, _ptr(header))
    return header


def plan_build(header, labels, weights, B, T, Mv, n_lm, want_rows=True, dims=None):
    """-> dict(off, lens, rows, inv, lm_pos, lm_idx, lm_label, lm_weight) built on the device from the header.
    Mv / n_lm are CAPACITIES (>= the header's totals): the lists' unused tails get safe values.  dims = (int32 [>=4],
    fp32 [>=2]) device tensors that receive the step's real counts and loss denominators (unimm_hip.h; int32 needs >= 4
    words: [3] = 1 when the batch did not fit the capacities)."""
    dev = header.device
    i32 = lambda n: torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    off, lens = i32(B), i32(B)
    rows = torch.empty(Mv, dtype=torch.int64, device=dev) if want_rows else None
    inv = torch.empty(B * T, dtype=torch.int64, device=dev) if want_rows else None
    lm = [i32(n_lm) for _ in range(4)] if (n_lm > 0 and labels is not None) else [None] * 4
    di, df = dims if dims is not None else (None, None)
    _dev(di, df)
    order = i32(B)                     # the sequences by length, longest first: the item order of the attention launches
    _call("unimm_plan_build", _ptr(header), _ptr(labels), _ptr(weights), B, T, _ptr(off), _ptr(lens), _ptr(rows), _ptr(inv),
          *[_ptr(t) for t in lm], Mv if want_rows else 0, n_lm if lm[0] is not None else 0, _ptr(di), _ptr(df), _ptr(order))
    return dict(off=off, lens=lens, rows=rows, inv=inv, lm_pos=lm[0], lm_idx=lm[1], lm_label=lm[2], lm_weight=lm[3], order=order)


def transpose_cast(src, dst, R, C_, ldd):
    _dev(src, dst)
    _call("unimm_transpose_cast", _ptr(src), _ptr(dst), R, C_, ldd)


def transpose_bf16(src, dst, R, C_):
    """dst[c, r] = src[r, c] (bf16 [R, C] -> bf16 [C, ldd >= R], surplus columns zero)."""
    _dev(src, dst)
    _call("unimm_transpose_bf16", _ptr(src), _ptr(dst), R, C_, src.stride(0), dst.stride(0))


def sum_slabs_bf16(slabs, out, n):
    """out[:n] (bf16) = slabs.sum(0) in slab order; slabs: fp32 [S, ...] contiguous, n a multiple of 8."""
    _dev(slabs, out)
    _call("unimm_sum_slabs_bf16", _ptr(slabs), slabs.shape[0], slabs.stride(0), _ptr(out), n)


def segment_rows_sum_bf16(src, first, items, dst, R, W):
    """dst block g (R rows x W, 2-D bf16 view) = sum of src's R-row blocks items[first[g] : first[g + 1]], fp32 in list order,
    rounded once (unimm_segment_rows_sum_bf16); first int32 [G + 1], items int32 device tensors."""
    _dev(src, first, items, dst)
    _call("unimm_segment_rows_sum_bf16", _ptr(src), src.stride(0), _ptr(first), _ptr(items), items.numel(), first.numel() - 1,
          _ptr(dst), dst.stride(0), R, W)


class TransposeDesc(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("R", C.c_int32), ("C", C.c_int32), ("ldd", C.c_int32),
                ("tile0", C.c_int32)]


def transpose_table(entries, device):
    """entries: list of (src fp32 [R, C] tensor, dst bf16 [C, ldd] tensor) -> (device table tensor, count, tiles)."""
    arr = (TransposeDesc * len(entries))()
    tiles = 0
    for d, (src, dst) in zip(arr, entries):
        _dev(src, dst)
        R, Cc = src.shape
        d.src, d.dst, d.R, d.C, d.ldd, d.tile0 = src.data_ptr(), dst.data_ptr(), R, Cc, dst.shape[1], tiles
        tiles += ((Cc + 31) // 32) * ((dst.shape[1] + 31) // 32)
    raw = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)
    return raw, len(entries), tiles


def transpose_cast_grouped(table, count, tiles):
    _call("unimm_transpose_cast_grouped", _ptr(table), count, tiles)


def pack_image(feat, loc, out, rows, F, ld):
    _dev(feat, loc, out)
    _call("unimm_pack_image", _ptr(feat), _ptr(loc), _ptr(out), rows, F, ld)


def mul_dropout(a, b, out, n, drop=NO_DROP, fusion_sum=False):
    """out = dropout(a * b) (fusion_method 'mul') or dropout(a + b) ('sum')."""
    _dev(a, b, out)
    _call("unimm_sum_dropout" if fusion_sum else "unimm_mul_dropout", _ptr(a), _ptr(b), _ptr(out), n, *drop[:3], _salt(drop))


def mul_dropout_bwd(a, b, dout, da, db, n, drop=NO_DROP, fusion_sum=False):
    _dev(a, b, dout, da, db)
    _call("unimm_sum_dropout_bwd" if fusion_sum else "unimm_mul_dropout_bwd", _ptr(a), _ptr(b), _ptr(dout), _ptr(da), _ptr(db), n,
          *drop[:3], _salt(drop))


# ---------------------------------------------------------------------------------------------
# losses
# ---------------------------------------------------------------------------------------------
def lm_loss_fwd(logits, labels, weights, rowloss, rownll, lse, n, V, n_dev=None):
    _dev(logits, labels, weights, rowloss, rownll, lse, n_dev)
    _call("unimm_lm_loss_fwd", _ptr(logits), _ptr(labels), _ptr(weights), _ptr(rowloss), _ptr(rownll), _ptr(lse), n, V,
          logits.stride(0), _ptr(n_dev))


def lm_loss_bwd(logits, labels, weights, lse, g, inv_denom, dlogits, n, V, n_dev=None, inv_dev=None):
    _dev(logits, labels, weights, lse, g, dlogits, n_dev, inv_dev)
    _call("unimm_lm_loss_bwd", _ptr(logits), _ptr(labels), _ptr(weights), _ptr(lse), _ptr(g), inv_denom, _ptr(dlogits), n, V,
          logits.stride(0), dlogits.stride(0), _ptr(n_dev), _ptr(inv_dev))


PG_LOGP, PG_RATIO = 0, 1


def pg_loss_fwd(logits, labels, pos, adv, blogp, mode, clip_eps, beta, rowloss, rownll, lse, ent, n, V, n_dev=None):
    """Policy-gradient rows (include/unimm_hip.h: unimm_pg_loss_fwd).  adv / blogp: fp32, indexed by pos[row] (pos None: by row)."""
    _dev(logits, labels, pos, adv, blogp, rowloss, rownll, lse, ent, n_dev)
    _call("unimm_pg_loss_fwd", _ptr(logits), _ptr(labels), _ptr(pos), _ptr(adv), _ptr(blogp), adv.numel(), mode, clip_eps, beta,
          _ptr(rowloss), _ptr(rownll), _ptr(lse), _ptr(ent), n, V, logits.stride(0), _ptr(n_dev))


def pg_loss_bwd(logits, labels, pos, adv, blogp, mode, clip_eps, beta, lse, ent, g, inv_denom, dlogits, n, V, n_dev=None,
                inv_dev=None):
    _dev(logits, labels, pos, adv, blogp, lse, ent, g, dlogits, n_dev, inv_dev)
    _call("unimm_pg_loss_bwd", _ptr(logits), _ptr(labels), _ptr(pos), _ptr(adv), _ptr(blogp), adv.numel(), mode, clip_eps, beta, _ptr(lse),
          _ptr(ent), _ptr(g), inv_denom, _ptr(dlogits), n, V, logits.stride(0), dlogits.stride(0), _ptr(n_dev), _ptr(inv_dev))


def pg_kl_loss_fwd(logits, labels, pos, adv, blogp, mode, clip_eps, beta, rowloss, rownll, lse, ent, n, V, ref_logits, kl_coef,
                   kl, ref_lse, n_dev=None):
    """Policy-gradient rows with the penalty kl_coef KL(p || p_ref) (include/unimm_hip.h: unimm_pg_kl_loss_fwd).  ref_logits: the
    frozen reference's fp32 rows for the same n rows (its own row stride); kl / ref_lse: fp32 [n], written here, read by the backward."""
    _dev(logits, labels, pos, adv, blogp, rowloss, rownll, lse, ent, n_dev, ref_logits, kl, ref_lse)
    _call("unimm_pg_kl_loss_fwd", _ptr(logits), _ptr(labels), _ptr(pos), _ptr(adv), _ptr(blogp), adv.numel(), mode, clip_eps, beta,
          _ptr(rowloss), _ptr(rownll), _ptr(lse), _ptr(ent), n, V, logits.stride(0), _ptr(n_dev), _ptr(ref_logits),
          ref_logits.stride(0) if ref_logits is not None else 0, kl_coef, _ptr(kl), _ptr(ref_lse))


def pg_kl_loss_bwd(logits, labels, pos, adv, blogp, mode, clip_eps, beta, lse, ent, g, inv_denom, dlogits, n, V, ref_logits, kl_coef,
                   kl, ref_lse, n_dev=None, inv_dev=None):
    _dev(logits, labels, pos, adv, blogp, lse, ent, g, dlogits, n_dev, inv_dev, ref_logits, kl, ref_lse)
    _call("unimm_pg_kl_loss_bwd", _ptr(logits), _ptr(labels), _ptr(pos), _ptr(adv), _ptr(blogp), adv.numel(), mode, clip_eps, beta,
          _ptr(lse), _ptr(ent), _ptr(g), inv_denom, _ptr(dlogits), n, V, logits.stride(0), dlogits.stride(0), _ptr(n_dev),
          _ptr(inv_dev), _ptr(ref_logits), ref_logits.stride(0) if ref_logits is not None else 0, kl_coef, _ptr(kl), _ptr(ref_lse))


def distill_loss_fwd(logits, labels, weights, ref_logits, tau, alpha, rowloss, rownll, lse, lse_t, ref_lse_t, kd, n, V, n_dev=None):
    """Knowledge-distillation rows (include/unimm_hip.h: unimm_distill_loss_fwd).  ref_logits: the frozen teacher's fp32 rows for the
    same n rows (its own row stride; None with alpha == 1); lse_t / ref_lse_t / kd: fp32 [n], written here."""
    _dev(logits, labels, weights, ref_logits, rowloss, rownll, lse, lse_t, ref_lse_t, kd, n_dev)
    _call("unimm_distill_loss_fwd", _ptr(logits), _ptr(labels), _ptr(weights), _ptr(ref_logits),
          ref_logits.stride(0) if ref_logits is not None else 0, tau, alpha, _ptr(rowloss), _ptr(rownll), _ptr(lse), _ptr(lse_t),
          _ptr(ref_lse_t), _ptr(kd), n, V, logits.stride(0), _ptr(n_dev))


def distill_loss_bwd(logits, labels, weights, ref_logits, tau, alpha, lse, lse_t, ref_lse_t, g, inv_denom, dlogits, n, V, n_dev=None,
                     inv_dev=None):
    _dev(logits, labels, weights, ref_logits, lse, lse_t, ref_lse_t, g, dlogits, n_dev, inv_dev)
    _call("unimm_distill_loss_bwd", _ptr(logits), _ptr(labels), _ptr(weights), _ptr(ref_logits),
          ref_logits.stride(0) if ref_logits is not None else 0, tau, alpha, _ptr(lse), _ptr(lse_t), _ptr(ref_lse_t), _ptr(g),
          inv_denom, _ptr(dlogits), n, V, logits.stride(0), dlogits.stride(0), _ptr(n_dev), _ptr(inv_dev))


PREF_MAX_MEMBERS, PREF_WS_ITEM_BYTES = 128, 16


class SeqPrefArgs(C.Structure):
    _fields_ = [("rownll", C.c_void_p), ("ref_rownll", C.c_void_p), ("row_seq", C.c_void_p), ("n_dev", C.c_void_p),
                ("seq_group", C.c_void_p), ("seq_weight", C.c_void_p), ("adv", C.c_void_p), ("seq_score", C.c_void_p),
                ("seq_prob", C.c_void_p), ("group_loss", C.c_void_p), ("alive_inv", C.c_void_p), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_int64), ("n", C.c_int32), ("B", C.c_int32), ("groups", C.c_int32),
                ("length_normalize", C.c_int32), ("beta", C.c_float)]


def seq_pref(rownll, ref_rownll, row_seq, n, seq_group, seq_weight, groups, beta, length_normalize, adv, seq_score, seq_prob,
             group_loss, alive_inv, n_dev=None, workspace=None):
    """Listwise preference over candidate sequences (include/unimm_hip.h: unimm_seq_pref).  rownll / ref_rownll (or None) / adv:
    fp32 [>= n]; row_seq int32 [>= n]; seq_group int32 [B], seq_weight fp32 [B]; seq_score / seq_prob fp32 [B]; group_loss fp32
    [groups]; alive_inv fp32 [1].  workspace: uint8, >= PREF_WS_ITEM_BYTES * (B + groups) bytes (None: allocated here)."""
    _dev(rownll, ref_rownll, row_seq, seq_group, seq_weight, adv, seq_score, seq_prob, group_loss, alive_inv, n_dev, workspace)
    B = seq_group.numel()
    if seq_weight.numel() != B or seq_score.numel() < B or seq_prob.numel() < B or group_loss.numel() < groups:
        raise UnimmHipError(f"seq_pref: {B} sequences in {groups} groups, but seq_weight / seq_score / seq_prob / group_loss hold "
                            f"{seq_weight.numel()} / {seq_score.numel()} / {seq_prob.numel()} / {group_loss.numel()} elements")
    if min(rownll.numel(), row_seq.numel(), adv.numel()) < n or (ref_rownll is not None and ref_rownll.numel() < n):
        raise UnimmHipError(f"seq_pref: rownll / ref_rownll / row_seq / adv hold fewer than n = {n} rows")
    if workspace is None:
        workspace = torch.empty(PREF_WS_ITEM_BYTES * (B + max(int(groups), 0)), dtype=torch.uint8, device=seq_group.device)
    a = SeqPrefArgs()
    a.rownll, a.ref_rownll, a.row_seq, a.n_dev = _ptr(rownll), _ptr(ref_rownll), _ptr(row_seq), _ptr(n_dev)
    a.seq_group, a.seq_weight, a.adv, a.seq_score, a.seq_prob = _ptr(seq_group), _ptr(seq_weight), _ptr(adv), _ptr(seq_score), _ptr(seq_prob)
    a.group_loss, a.alive_inv, a.workspace, a.workspace_bytes = _ptr(group_loss), _ptr(alive_inv), _ptr(workspace), workspace.numel()
    a.n, a.B, a.groups, a.length_normalize, a.beta = int(n), B, int(groups), 1 if length_normalize else 0, float(beta)
    _call("unimm_seq_pref", C.byref(a))
    workspace.record_stream(torch.cuda.current_stream())


def kl_loss_fwd(pred, target, label, rowloss, lse, rows, Cn):
    _dev(pred, target, label, rowloss, lse)
    _call("unimm_kl_loss_fwd", _ptr(pred), _ptr(target), _ptr(label), _ptr(rowloss), _ptr(lse), rows, Cn, pred.stride(0))


def kl_loss_bwd(pred, target, label, lse, g, inv_denom, dpred, rows, Cn, inv_dev=None):
    _dev(pred, target, label, lse, g, dpred, inv_dev)
    _call("unimm_kl_loss_bwd", _ptr(pred), _ptr(target), _ptr(label), _ptr(lse), _ptr(g), inv_denom, _ptr(dpred), rows, Cn,
          pred.stride(0), dpred.stride(0), _ptr(inv_dev))


def mse_loss_fwd(pred, target, label, rowloss, rows, Cn):
    _dev(pred, target, label, rowloss)
    _call("unimm_mse_loss_fwd", _ptr(pred), _ptr(target), _ptr(label), _ptr(rowloss), rows, Cn, pred.stride(0))


def mse_loss_bwd(pred, target, label, g, inv_denom, dpred, rows, Cn, split=False):
    """dpred: bf16 [rows, ldd], or (split=True) an x-type split operand [rows, 3 ldd]."""
    _dev(pred, target, label, g, dpred)
    ldd = dpred.shape[1] // 3 if split else dpred.stride(0)
    _call("unimm_mse_loss_bwd", _ptr(pred), _ptr(target), _ptr(label), _ptr(g), inv_denom, _ptr(dpred), rows, Cn, pred.stride(0), ldd,
          1 if split else 0)


def nsp_loss_fwd(logits, labels, w0, w1, loss, B):
    _dev(logits, labels, loss)
    _call("unimm_nsp_loss_fwd", _ptr(logits), _ptr(labels), w0, w1, _ptr(loss), B, logits.stride(0))


def nsp_loss_bwd(logits, labels, w0, w1, g, dlogits, B, extra=None):
    """dlogits: fp32 [B, >= 2]; extra: fp32 [B, 2] contiguous gradient added in (or None)."""
    _dev(logits, labels, g, dlogits, extra)
    if dlogits.dtype != torch.float32 or (extra is not None and (extra.dtype != torch.float32 or not extra.is_contiguous())):
        raise UnimmHipError("nsp_loss_bwd: dlogits / extra must be fp32 (extra contiguous [B, 2])")
    _call("unimm_nsp_loss_bwd", _ptr(logits), _ptr(labels), w0, w1, _ptr(g), _ptr(extra), _ptr(dlogits), B, logits.stride(0),
          dlogits.stride(0))


class LinearF32Args(C.Structure):
    _fields_ = [("a", C.c_void_p), ("b", C.c_void_p), ("bias", C.c_void_p), ("out", C.c_void_p), ("rowsum", C.c_void_p),
                ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
                ("sa_m", C.c_int64), ("sa_k", C.c_int64), ("sb_k", C.c_int64), ("sb_n", C.c_int64), ("ldo", C.c_int64),
                ("relu", C.c_int32), ("accumulate", C.c_int32)]


def linear_f32(a, b, out, M, N, K, sa, sb, bias=None, relu=False, accumulate=False, rowsum=None):
    """out[M, N] (+)= act(A . B + bias), all fp32; sa = (stride of A over m, over k), sb = (stride of B over k, over n),
    in elements (include/unimm_hip.h: unimm_linear_f32)."""
    _dev(a, b, out, bias, rowsum)
    for t in (a, b, out, bias, rowsum):
        if t is not None and t.dtype != torch.float32:
            raise UnimmHipError("linear_f32: every operand is fp32")
    g = LinearF32Args()
    g.a, g.b, g.bias, g.out, g.rowsum = a.data_ptr(), b.data_ptr(), _ptr(bias), out.data_ptr(), _ptr(rowsum)
    g.M, g.N, g.K = M, N, K
    g.sa_m, g.sa_k, g.sb_k, g.sb_n, g.ldo = sa[0], sa[1], sb[0], sb[1], out.stride(0)
    g.relu, g.accumulate = int(bool(relu)), int(bool(accumulate))
    _call("unimm_linear_f32", C.byref(g))
    return out


def rows_add_f32(dst, idx, src, n, H):
    """dst (bf16 [*, H] contiguous rows)[idx[r], :] += src (fp32 [n, H] contiguous)[r, :]"""
    _dev(dst, idx, src)
    _call("unimm_rows_add_f32", _ptr(dst), _ptr(idx), _ptr(src), n, H)


def reduce_sum(src, n, dst, scale=1.0, n_dev=None, scale_dev=None):
    _dev(src, dst, n_dev, scale_dev)
    _call("unimm_reduce_sum", _ptr(src), n, _ptr(dst), scale, _ptr(n_dev), _ptr(scale_dev))


def segment_sum(src, seg, dst, n, sign=1.0):
    _dev(src, seg, dst)
    _call("unimm_segment_sum", _ptr(src), _ptr(seg), _ptr(dst), n, sign)


def gelu_bwd(dt, u, du, n):
    _dev(dt, u, du)
    _call("unimm_gelu_bwd", _ptr(dt), _ptr(u), _ptr(du), n)


def gather_rows(src, idx, dst, n, H, scatter=False, n_dev=None):
    _dev(src, idx, dst, n_dev)
    _call("unimm_gather_rows", _ptr(src), _ptr(idx), _ptr(dst), n, H, 1 if scatter else 0, _ptr(n_dev))


_EPI_NAMES = ["BIAS", "BIAS_GELU", "BIAS_DROP_RESID", "BIAS_RELU", "DGELU", "ADD", "MUL", "BIAS_GELU_DG"]
_TILE_NAMES = {1: "128x128", 3: "256x256", 6: "192x256", 7: "64x128", 8: "256x256pp", 9: "64x128s3", 10: "128x128s3", 12: "192x256x3", 14: "128x128x3", 15: "64x128x3"}
PROF_VARIANTS = 516


def gemm_variant_name(i):
    """Name of a profiler variant = one kernel symbol (csrc/gemm.hip: PROF_VARIANTS): the persistent form is gemm_ntp."""
    if i >= 512:
        return {512: "gemm_tn_pp", 513: "gemm_tn<256x256 lock-step>", 514: "gemm_tn<128x128>"}.get(i, f"variant{i}")
    f32, epi, tile, persist = i & 1, (i >> 1) & 7, (i >> 4) & 15, i >> 8
    return f"gemm_nt{'p' if persist else ''}<{_TILE_NAMES.get(tile, tile)},{_EPI_NAMES[epi]},{'f32' if f32 else 'bf16'}>"


ADAMW_MAX_GROUPS = 8
ADAMW_SKIP = 255          # chunk group id of parameters that never receive a gradient


class AdamWArgs(C.Structure):
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("w16", C.c_void_p),
                ("group", C.c_void_p), ("n", C.c_int64), ("n_groups", C.c_int32), ("step", C.c_int32),
                ("lr", C.c_double * ADAMW_MAX_GROUPS), ("weight_decay", C.c_double * ADAMW_MAX_GROUPS),
                ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("grad_scale", C.c_float),
                ("correct_bias", C.c_int32), ("zero_grad", C.c_int32)]


def adamw_step(p, g, m, v, group, lrs, wds, step, beta1=0.9, beta2=0.999, eps=1e-6, w16=None, grad_scale=1.0,
               correct_bias=True, zero_grad=False, clip_state=None, skip_nonfinite=False):
    """One fused AdamW step over flat fp32 arenas (see include/unimm_hip.h: unimm_adamw_step).  clip_state: the state block a
    `grad_norm` call filled; the step then is unimm_adamw_step_clipped, which takes its gradient scale from the block (grad_scale
    is ignored) and, with skip_nonfinite, updates nothing when the block's non-finite flag is set."""
    _dev(p, g, m, v, group, w16)
    if len(lrs) != len(wds) or not 1 <= len(lrs) <= ADAMW_MAX_GROUPS:
        raise UnimmHipError(f"adamw_step: 1..{ADAMW_MAX_GROUPS} (lr, weight_decay) groups, got {len(lrs)}")
    a = AdamWArgs()
    a.p, a.g, a.m, a.v, a.w16, a.group = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), _ptr(w16), group.data_ptr()
    a.n, a.n_groups, a.step = p.numel(), len(lrs), int(step)
    for i, (lr, wd) in enumerate(zip(lrs, wds)):
        a.lr[i], a.weight_decay[i] = float(lr), float(wd)
    a.beta1, a.beta2, a.eps, a.grad_scale = beta1, beta2, eps, grad_scale
    a.correct_bias, a.zero_grad = int(bool(correct_bias)), int(bool(zero_grad))
    if clip_state is None:
        _call("unimm_adamw_step", C.byref(a))
    else:
        _dev(clip_state)
        _call("unimm_adamw_step_clipped", C.byref(a), clip_state.data_ptr(), int(bool(skip_nonfinite)))


GRAD_NORM_WS_DOUBLES = 16384          # UNIMM_GRAD_NORM_WS_DOUBLES: one partial per workgroup (2048) and group (8)
GRAD_NORM_PASS = 2048 * 256 * 2 * 4   # elements one grid-stride pass of the norm kernel covers (csrc/optim.hip)


class ClipState(C.Structure):
    """The device-resident result of `grad_norm` (include/unimm_hip.h: unimm_clip_state), 104 bytes."""
    _fields_ = [("group_sumsq", C.c_double * ADAMW_MAX_GROUPS), ("sumsq", C.c_double), ("norm", C.c_double), ("coef", C.c_double),
                ("scale", C.c_float), ("nonfinite", C.c_int32), ("skipped", C.c_int32)]


CLIP_STATE_DOUBLES = C.sizeof(ClipState) // 8


def new_clip_state(device):
    """A zeroed state block as an fp64 tensor (torch allocations are at least 256-byte aligned)."""
    return torch.zeros(CLIP_STATE_DOUBLES, dtype=torch.float64, device=device)


def clip_state_views(state):
    """Named views of a state block tensor: no copy, no sync."""
    f32, i32 = state.view(torch.float32), state.view(torch.int32)
    o = ClipState.scale.offset // 4
    return dict(group_sumsq=state[:ADAMW_MAX_GROUPS], sumsq=state[ClipState.sumsq.offset // 8],
                norm=state[ClipState.norm.offset // 8], coef=state[ClipState.coef.offset // 8],
                scale=f32[o], nonfinite=i32[o + 1], skipped=i32[o + 2])


def grad_norm(g, group, n_groups, workspace, state, grad_scale=1.0, max_norm=float("inf")):
    """Norm of grad_scale * g over the chunks whose group id is below n_groups, and the clip coefficient for max_norm, left in
    `state` on the device (see include/unimm_hip.h: unimm_grad_norm).  workspace: fp64, >= GRAD_NORM_WS_DOUBLES elements."""
    _dev(g, group, workspace, state)
    _call("unimm_grad_norm", g.data_ptr(), group.data_ptr(), g.numel(), int(n_groups), float(grad_scale), float(max_norm),
          workspace.data_ptr(), workspace.numel(), state.data_ptr())


NDCG_MAX_OPTIONS, NDCG_MAX_ITER = 128, 64


class NdcgArgs(C.Structure):
    _fields_ = [("pred", C.c_void_p), ("truth", C.c_void_p), ("ndcg", C.c_void_p), ("alive", C.c_void_p), ("dpred", C.c_void_p),
                ("iters", C.c_void_p), ("slates", C.c_int32), ("n", C.c_int32), ("k", C.c_int32),
                ("powered_relevancies", C.c_int32), ("max_iter", C.c_int32), ("pad_label", C.c_float),
                ("temperature", C.c_float), ("tol", C.c_float)]


def neural_ndcg(pred, truth, pad_label=-1.0, temperature=1.0, powered=True, k=None, max_iter=50, tol=1e-6):
    """pred, truth fp32 [slates, n] on the device -> (ndcg [slates], alive [slates], dpred [slates, n], iters [slates])
    (see include/unimm_hip.h: unimm_neural_ndcg)."""
    _dev(pred, truth)
    if pred.dtype != torch.float32 or truth.dtype != torch.float32 or pred.shape != truth.shape or pred.dim() != 2:
        raise UnimmHipError("neural_ndcg: pred and truth must be fp32 [slates, n] of the same shape")
    pred, truth = pred.contiguous(), truth.contiguous()
    S, n = pred.shape
    if not 1 <= n <= NDCG_MAX_OPTIONS or not 1 <= max_iter <= NDCG_MAX_ITER:
        raise UnimmHipError(f"neural_ndcg: n <= {NDCG_MAX_OPTIONS} options and max_iter <= {NDCG_MAX_ITER} (got {n}, {max_iter})")
    ndcg = torch.empty(S, dtype=torch.float32, device=pred.device)
    alive = torch.empty_like(ndcg)
    dpred = torch.empty_like(pred)
    iters = torch.empty(S, dtype=torch.int32, device=pred.device)
    a = NdcgArgs()
    a.pred, a.truth, a.ndcg, a.alive, a.dpred, a.iters = (t.data_ptr() for t in (pred, truth, ndcg, alive, dpred, iters))
    a.slates, a.n, a.k, a.powered_relevancies, a.max_iter = S, n, (0 if k is None else int(k)), int(bool(powered)), int(max_iter)
    a.pad_label, a.temperature, a.tol = float(pad_label), float(temperature), float(tol)
    _call("unimm_neural_ndcg", C.byref(a))
    return ndcg, alive, dpred, iters


def prof_enable(on):
    """False / 0 = off, True / 1 = every GEMM launch, 2 = weight-gradient launches only."""
    _call("unimm_prof_enable", int(on))


def prof_collect():
    """-> {variant name: (total_ms, total_flops, launches)} for the launches since prof_enable(True)."""
    n = PROF_VARIANTS
    ms, fl, cnt = (C.c_double * n)(), (C.c_double * n)(), (C.c_int32 * n)()
    _call("unimm_prof_collect", ms, fl, cnt, n)
    return {gemm_variant_name(i): (ms[i], fl[i], cnt[i]) for i in range(n) if cnt[i] > 0}


def prof_tag(tag):
    """Tag (0 .. 7) of the GEMM launches that follow (see include/unimm_hip.h: unimm_prof_tag)."""
    lib().unimm_prof_tag(int(tag))


def prof_tagged(ntags=8):
    """-> {tag: (total_ms, total_flops, launches, union_ms)} of the NT launches the last prof_collect() consumed; union_ms = the
    wall time during which at least one launch of the tag was executing (launches of two streams side by side count once)."""
    ms, fl, cnt, un = (C.c_double * ntags)(), (C.c_double * ntags)(), (C.c_int32 * ntags)(), (C.c_double * ntags)()
    _call("unimm_prof_tagged", ms, fl, cnt, un, ntags)
    return {t: (ms[t], fl[t], cnt[t], un[t]) for t in range(ntags)}


# ---------------------------------------------------------------------------------------------
# fp32-accuracy mode (csrc/x3ops.hip; include/unimm_hip.h "fp32x3")
# ---------------------------------------------------------------------------------------------
X3_COPY, X3_ADD, X3_GELU, X3_MUL_DGELU = range(4)


class X3SplitArgs(C.Structure):
    _fields_ = [("a", C.c_void_p), ("b", C.c_void_p), ("out32", C.c_void_p), ("out3", C.c_void_p), ("rows", C.c_int64),
                ("cols", C.c_int32), ("cp", C.c_int32), ("lda", C.c_int32), ("ldb", C.c_int32), ("ld32", C.c_int32),
                ("op", C.c_int32), ("wtype", C.c_int32)]


def x3_split(a, out3=None, out32=None, op=X3_COPY, b=None, rows=None, cols=None, cp=None, wtype=False):
    """y = op(a, b) (fp32 [rows, cols]) -> out32 (fp32) and / or out3 (split operand, bf16 [rows, 3 cp])."""
    _dev(a, b, out32, out3)
    st = getattr(_tls, "x3s", None)
    if st is None:
        s = X3SplitArgs()
        st = _tls.x3s = (s, C.addressof(s), lib().unimm_x3_split)
    s, addr, fn = st
    s.a, s.b, s.out32, s.out3 = a.data_ptr(), _ptr(b), _ptr(out32), _ptr(out3)
    s.rows = a.shape[0] if rows is None else rows
    s.cols = a.shape[1] if cols is None else cols
    s.cp = (out3.shape[1] // 3) if cp is None else cp
    s.lda, s.ldb, s.ld32 = a.stride(0), (b.stride(0) if b is not None else 0), (out32.stride(0) if out32 is not None else 0)
    s.op, s.wtype = op, 1 if wtype else 0
    rc = fn(addr, _stream())
    if rc != 0:
        _check(rc, "unimm_x3_split")


def x3_split_wt(src, dst, R, C_, Rp):
    """transposed w-type split: src fp32 [R, C] -> dst bf16 [C, 3 Rp] (zero-filled by the caller once)."""
    _dev(src, dst)
    _call("unimm_x3_split_wt", _ptr(src), _ptr(dst), R, C_, src.stride(0), Rp)


def x3_layernorm_bwd_partials(dy, x, mean, rstd, gamma, dx32, dxd3, partials, M, H, drop=None, out_drop=None, m_dev=None):
    drop = drop or NO_DROP
    out_drop = out_drop or NO_DROP
    _dev(dy, x, mean, rstd, gamma, dx32, dxd3, partials)
    blocks = C.c_int32(0)
    _call("unimm_x3_layernorm_bwd_partials", _ptr(dy), _ptr(x), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(dx32), _ptr(dxd3),
          _ptr(partials), M, H, *drop[:3], *out_drop[:3], C.byref(blocks), _ptr(m_dev), _salt(drop, out_drop))
    return blocks.value


def embed_bwd_f32(ids, pos, typ, word, post, type_, ext, gamma, beta, dy, dword, dpos, dtype, dext, dgamma, dbeta,
                  partials, M, H, type_vocab=2, eps=1e-12, drop=NO_DROP, m_dev=None, rows=None):
    a = _embed_args(ids, pos, typ, word, post, type_, ext, gamma, beta, M, H, type_vocab, eps, drop, m_dev, rows)
    _dev(dy, dword, dpos, dtype, dext, dgamma, dbeta, partials)
    _call("unimm_embed_bwd_f32", C.byref(a), _ptr(dy), _ptr(dword), _ptr(dpos), _ptr(dtype), _ptr(dext), _ptr(dgamma), _ptr(dbeta),
          _ptr(partials))


def x3_lm_loss_bwd(logits, labels, weights, lse, g, inv_denom, out3, n, V, n_dev=None, inv_dev=None):
    _dev(logits, labels, weights, lse, g, out3)
    _call("unimm_x3_lm_loss_bwd", _ptr(logits), _ptr(labels), _ptr(weights), _ptr(lse), _ptr(g), inv_denom, _ptr(out3), n, V,
          logits.stride(0), out3.shape[1] // 3, _ptr(n_dev), _ptr(inv_dev))


def x3_kl_loss_bwd(pred, target, label, lse, g, inv_denom, out3, rows, Cn, inv_dev=None):
    _dev(pred, target, label, lse, g, out3)
    _call("unimm_x3_kl_loss_bwd", _ptr(pred), _ptr(target), _ptr(label), _ptr(lse), _ptr(g), inv_denom, _ptr(out3), rows, Cn,
          pred.stride(0), out3.shape[1] // 3, _ptr(inv_dev))


def x3_rows_add(dst, idx, src, n, H):
    _dev(dst, idx, src)
    _call("unimm_x3_rows_add", _ptr(dst), _ptr(idx), _ptr(src), n, H, dst.stride(0))


class X3AttnPlanes(C.Structure):
    _fields_ = [("out3", C.c_void_p), ("dq3", C.c_void_p), ("dk3", C.c_void_p), ("dv3", C.c_void_p), ("ld3", C.c_int32), ("cp3", C.c_int32)]


def x3_attn_fwd(q, k, v, out, lse, mask, B, H, Tq, Tk, D, scale, mask_q_stride, mask_b_stride, drop=NO_DROP, qvar=None, kvar=None,
                out3=None, kshared=None):
    """unimm_attn_fwd on fp32 q / k / v / out (2-D views, row stride = stride(0)).  out3 (bf16 [rows, 3 cp]): the context also
    as an x-type split operand.  kshared: (offsets, lengths, ins) as in `attn_fwd` (needs kvar, inference only, the
    matrix-instruction kernels)."""
    _dev(q, k, v, out, lse, mask, out3)
    pl = None
    if out3 is not None:
        pl = X3AttnPlanes()
        pl.out3, pl.ld3, pl.cp3 = out3.data_ptr(), out3.stride(0), out3.shape[1] // 3
    a = AttnArgs()
    _attn_common(a, q, k, v, mask, B, H, Tq, Tk, D, scale, mask_q_stride, mask_b_stride, drop, qvar, kvar)
    a.out, a.lse, a.ldo = out.data_ptr(), _ptr(lse), out.stride(0)
    if kshared is not None:
        a.ks_off, a.ks_len, a.ks_ins = _ptr(kshared[0]), _ptr(kshared[1]), int(kshared[2])
    _call("unimm_x3_attn_fwd", C.byref(a), C.byref(pl) if pl is not None else None)


def x3_attn_bwd(q, k, v, out, dout, lse, delta, dq, dk, dv, mask, B, H, Tq, Tk, D, scale, mask_q_stride, mask_b_stride,
                drop=NO_DROP, qvar=None, kvar=None, planes=None):
    """planes = (cp3, ld3): dq / dk / dv are bf16 views of plane 0 of x-type split buffers (plane stride cp3, row stride ld3) and
    receive the gradients as split operands instead of fp32."""
    _dev(q, k, v, out, dout, lse, delta, dq, dk, dv, mask)
    a = AttnBwdArgs()
    pl = None
    if planes is not None:
        pl = X3AttnPlanes()
        pl.dq3, pl.dk3, pl.dv3, pl.cp3, pl.ld3 = dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), planes[0], planes[1]
    _attn_common(a, q, k, v, mask, B, H, Tq, Tk, D, scale, mask_q_stride, mask_b_stride, drop, qvar, kvar)
    a.out, a.dout, a.lse, a.delta = out.data_ptr(), dout.data_ptr(), lse.data_ptr(), delta.data_ptr()
    a.ldo, a.lddo = out.stride(0), dout.stride(0)
    if pl is None:
        a.dq, a.dk, a.dv = dq.data_ptr(), dk.data_ptr(), dv.data_ptr()
        a.lddq, a.lddk, a.lddv = dq.stride(0), dk.stride(0), dv.stride(0)
    _call("unimm_x3_attn_bwd", C.byref(a), C.byref(pl) if pl is not None else None)


def x3_attn_set_impl(impl):
    """1 = fp32 matrix-instruction attention kernels (default), 0 = the vector-ALU kernels (A/B runs)."""
    _call("unimm_x3_attn_set_impl", int(impl))


def x3_layernorm_fwd(x, gamma, beta, y32, y3, mean, rstd, M, H, eps=1e-12, drop=NO_DROP):
    """LayerNorm forward writing fp32 rows (or None) and the x-type split operand y3 [M, 3 H]."""
    _dev(x, gamma, beta, y32, y3, mean, rstd)
    _call("unimm_x3_layernorm_fwd", x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _ptr(y32), y3.data_ptr(), _ptr(mean), _ptr(rstd),
          M, H, eps, *drop[:3], _salt(drop))


# the header's name of every argument struct -> the class above that mirrors it (tests/test_abi.py compares fields and layout)
STRUCTS = {
    "unimm_gemm_nt_args": GemmNtArgs, "unimm_gemm_tn_args": GemmTnArgs, "unimm_attn_args": AttnArgs,
    "unimm_attn_bwd_args": AttnBwdArgs, "unimm_attn_spliced_bwd_args": AttnSplicedBwdArgs, "unimm_finish_desc": FinishDesc,
    "unimm_embed_args": EmbedArgs, "unimm_transpose_desc": TransposeDesc, "unimm_linear_f32_args": LinearF32Args,
    "unimm_adamw_args": AdamWArgs, "unimm_clip_state": ClipState, "unimm_ndcg_args": NdcgArgs, "unimm_x3_split_args": X3SplitArgs,
    "unimm_x3_attn_planes": X3AttnPlanes, "unimm_attn_decode_args": AttnDecodeArgs, "unimm_kv_update_args": KvUpdateArgs,
    "unimm_kv_append_args": KvAppendArgs, "unimm_lm_spec_verify_args": LmSpecVerifyArgs,
    "unimm_seq_pref_args": SeqPrefArgs, "unimm_lm_history": LmHistory,
}
