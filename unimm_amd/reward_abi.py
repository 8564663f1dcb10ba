"""ctypes binding of libunimm_reward.so (the C ABI in include/unimm_reward.h): `unimm_ngram_reward`, the kernel that scores
hypothesis rows against their dialogs' references with the CIDEr-D consensus reward (unimm_amd/reward.py is the surface).

The extension library is built by `unimm_amd.build` beside libunimm_hip.so; as for that one there is no fallback: a missing library
or a refused call raises `lib.UnimmHipError`.  Launches go to the stream `lib.stream_scope` pins, or torch's current one.
tests/test_reward_build_cpu.py holds `SIGNATURES` and `STRUCTS` to the header and the library's kernel to its resource ledger."""
from __future__ import annotations

import ctypes as C
import os

from . import lib as L

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libunimm_reward.so")
ABI_VERSION = 1
MAX_LEN, MAX_REFS, ORDERS = 64, 128, 4
EMPTY = -2
HASH_BASIS, HASH_PRIME = 2166136261, 16777619

SIGNATURES = {                                   # in header order, as lib.SIGNATURES
    "unimm_reward_version": (C.c_int, []),
    "unimm_ngram_reward": (C.c_int, [C.c_void_p, C.c_void_p]),
}


class NgramRewardArgs(C.Structure):
    _fields_ = [("hyp", C.c_void_p), ("hyp_len", C.c_void_p), ("hyp_group", C.c_void_p), ("ref", C.c_void_p), ("ref_len", C.c_void_p),
                ("ref_weight", C.c_void_p), ("table_keys", C.c_void_p), ("table_idf", C.c_void_p), ("reward", C.c_void_p),
                ("per_order", C.c_void_p), ("default_idf", C.c_double), ("sigma", C.c_double),
                ("S", C.c_int32), ("ldh", C.c_int32), ("G", C.c_int32), ("M", C.c_int32), ("ldr", C.c_int32), ("cap", C.c_int32),
                ("max_hyp_len", C.c_int32), ("max_ref_len", C.c_int32)]


STRUCTS = {"unimm_ngram_reward_args": NgramRewardArgs}
_lib = None


def loaded():
    """whether this process has loaded the extension library (a step with a host reward never does)"""
    return _lib is not None


def lib():
    """Load the extension library once; fail loudly when it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise L.UnimmHipError(f"{LIB_PATH} is missing: build it with `python -m unimm_amd.build` (hipcc, gfx950). "
                                  "unimm_amd has no CPU or PyTorch fallback for its kernels.")
        M = C.CDLL(LIB_PATH)
        if M.unimm_reward_version() != ABI_VERSION:
            raise L.UnimmHipError(f"libunimm_reward.so ABI {M.unimm_reward_version()} != expected {ABI_VERSION}: rebuild")
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(M, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = M
    return _lib


def _call(name, *args):
    """One entry point of the extension library by name, on the current stream; a failure is raised under that name."""
    L._check(getattr(lib(), name)(*args, L._stream()), name)


def ngram_reward(hyp, hyp_len, hyp_group, ref, ref_len, ref_weight, table_keys, table_idf, default_idf, sigma, reward,
                 per_order=None, max_hyp_len=None, max_ref_len=None):
    """unimm_ngram_reward: reward[s] = the CIDEr-D reward of hypothesis row s against the references of dialog hyp_group[s].
    hyp int32 [S, >= len] (row stride = stride(0)), hyp_len / hyp_group int32 [S]; ref int32 [G, M, ldr] contiguous in G and M,
    ref_len int32 [G, M], ref_weight fp32 [G, M] or None; table_keys int32 [cap, 4] / table_idf fp64 [cap] or both None;
    reward fp32 [S]; per_order fp64 [S, 4] or None.  max_hyp_len / max_ref_len: the bounds on the device lengths the caller
    vouches for (default: the row stride, at most 65)."""
    L._dev(hyp, hyp_len, hyp_group, ref, ref_len, ref_weight, table_keys, table_idf, reward, per_order)
    a = NgramRewardArgs()
    a.hyp, a.hyp_len, a.hyp_group = L._ptr(hyp), L._ptr(hyp_len), L._ptr(hyp_group)
    a.ref, a.ref_len, a.ref_weight = L._ptr(ref), L._ptr(ref_len), L._ptr(ref_weight)
    a.table_keys, a.table_idf, a.reward, a.per_order = L._ptr(table_keys), L._ptr(table_idf), L._ptr(reward), L._ptr(per_order)
    a.default_idf, a.sigma = default_idf, sigma
    a.S, a.ldh = hyp.shape[0], hyp.stride(0) if hyp.shape[0] > 1 else hyp.shape[1]
    a.G, a.M, a.ldr = ref.shape[0], ref.shape[1], ref.shape[2]
    a.cap = 0 if table_keys is None else table_keys.shape[0]
    a.max_hyp_len = min(a.ldh, MAX_LEN + 1) if max_hyp_len is None else max_hyp_len
    a.max_ref_len = min(a.ldr, MAX_LEN + 1) if max_ref_len is None else max_ref_len
    _call("unimm_ngram_reward", C.byref(a))
