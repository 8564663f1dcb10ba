"""ctypes binding of libunimm_mix.so (the C ABI in include/unimm_mix.h): `unimm_lm_mix`, the row kernel that turns the logits rows
of K models into one, for ensemble and contrastive answer generation (unimm_amd/generation.py).

The extension library is built by `unimm_amd.build` beside libunimm_hip.so; as for that one there is no fallback: a missing library
or a refused call raises `lib.UnimmHipError`.  Launches go to the stream `lib.stream_scope` pins, or torch's current one.
tests/test_mix_build_cpu.py holds `SIGNATURES` and `STRUCTS` to the header and the library's kernel to its resource ledger."""
from __future__ import annotations

import ctypes as C
import os

from . import lib as L

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libunimm_mix.so")
ABI_VERSION = 1
MAX_MEMBERS = 5
LOGIT, PROB = 0, 1
MODES = {"logit": LOGIT, "prob": PROB}

SIGNATURES = {                                   # in header order, as lib.SIGNATURES
    "unimm_mix_version": (C.c_int, []),
    "unimm_lm_mix": (C.c_int, [C.c_void_p, C.c_void_p]),
}


class LmMixArgs(C.Structure):
    _fields_ = [("x", C.c_void_p * MAX_MEMBERS), ("out", C.c_void_p), ("banned", C.c_void_p), ("flags", C.c_void_p),
                ("ld", C.c_int32 * MAX_MEMBERS), ("w", C.c_float * MAX_MEMBERS),
                ("K", C.c_int32), ("mode", C.c_int32), ("rows", C.c_int32), ("V", C.c_int32), ("ldo", C.c_int32),
                ("nbanned", C.c_int32), ("sep", C.c_int32), ("log_alpha", C.c_float)]


STRUCTS = {"unimm_lm_mix_args": LmMixArgs}
_lib = None


def lib():
    """Load the extension library once; fail loudly when it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise L.UnimmHipError(f"{LIB_PATH} is missing: build it with `python -m unimm_amd.build` (hipcc, gfx950). "
                                  "unimm_amd has no CPU or PyTorch fallback for its kernels.")
        M = C.CDLL(LIB_PATH)
        if M.unimm_mix_version() != ABI_VERSION:
            raise L.UnimmHipError(f"libunimm_mix.so ABI {M.unimm_mix_version()} != expected {ABI_VERSION}: rebuild")
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(M, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = M
    return _lib


def _call(name, *args):
    """One entry point of the extension library by name, on the current stream; a failure is raised under that name."""
    L._check(getattr(lib(), name)(*args, L._stream()), name)


def lm_mix(rows_list, weights, mode, V, banned, flags, sep, log_alpha, out):
    """unimm_lm_mix: out[r, :V] = the mixture of the members' rows r.  rows_list: K = 1 .. 5 fp32 logits blocks [rows, >= V] (2-D
    views, row stride = stride(0), one row count); weights: K floats, member 0 first; mode: "logit" (z = sum_m w_m x_m, rounded
    product by product) or "prob" (z = log sum_m w_m softmax(x_m)), or the header's number; log_alpha: float("-inf") = no
    plausibility cut, else ids with x_0 < max over the eligible ids of x_0 + log_alpha become -inf (banned / flags / sep say which
    ids are eligible, as for `lib.lm_topk`).  out: fp32 [rows, >= V], no member's memory."""
    L._dev(*rows_list, banned, flags, out)
    a = LmMixArgs()
    a.K, a.mode = len(rows_list), MODES.get(mode, -1) if isinstance(mode, str) else mode     # an unknown name: refused by the C side
    if a.K != len(weights):
        raise L.UnimmHipError(f"lm_mix: {len(weights)} weights for {a.K} members")
    for m, (x, w) in enumerate(zip(rows_list[:MAX_MEMBERS], weights)):
        a.x[m], a.ld[m], a.w[m] = L._ptr(x), x.stride(0) if x is not None else 0, w
    a.out, a.ldo = L._ptr(out), out.stride(0) if out is not None else 0
    a.banned, a.flags = L._ptr(banned), L._ptr(flags)
    a.rows = rows_list[0].shape[0] if rows_list and rows_list[0] is not None else 0
    a.V, a.nbanned, a.sep, a.log_alpha = V, 0 if banned is None else banned.numel(), sep, log_alpha
    _call("unimm_lm_mix", C.byref(a))
