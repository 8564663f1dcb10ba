"""What the attention entry points refuse, and in which order: unimm_attn_fwd, unimm_attn_probs, unimm_attn_bwd and the four
spliced entries, called through ctypes on their argument structs, one table of (case, changed fields, code) per entry.

A case starts from arguments the entry accepts (B = 1, H = 2, Tq = Tk = 8, D = 64) and changes some fields; every rule appears
once, and cases that break two rules pin which one answers.  Callers tell the codes apart (a shape the kernels do not take is
not a misaligned view), so code and precedence are part of the interface, whichever function of attention.hip holds the check.
A refused call returns before any HIP call, so the same table runs

  * without a GPU, on made-up 16-byte aligned addresses (skipped where a GPU is present: a case that a regression accepts must
    not launch on addresses that mean nothing), and
  * on the GPU, on real tensors (large enough for every shape a case names), where the NaN-filled outputs must also come back
    bit for bit."""
import ctypes as C

import pytest
import torch

from unimm_amd import lib

OK, E_ARG, E_SHAPE, E_ALIGN = 0, -1, -2, -3
PTR, OFF8 = "PTR", "OFF8"        # field values of a case: a valid address of its own / that address plus 8 bytes (4 bf16 elements)

_FWD_PTRS = ["q", "k", "v", "out", "lse", "mask"]
_BWD_PTRS = ["q", "k", "v", "out", "dout", "lse", "delta", "dq", "dk", "dv", "mask"]
_VAR = ["q_off", "q_len", "k_off", "k_len"]
_SHAPE = dict(B=1, H=2, Tq=8, Tk=8, D=64, mask_q_stride=1, mask_b_stride=8, scale=0.125, drop_key=0, drop_thr=0, drop_scale=1.0)
_FWD_LD = ["ldq", "ldk", "ldv", "ldo"]
_BWD_LD = _FWD_LD + ["lddo", "lddq", "lddk", "lddv"]
_SEG = dict(k_off=PTR, k_len=PTR, ks_off=PTR, ks_len=PTR, ks_ins=1)
_DROP = dict(drop_key=1, drop_thr=1 << 28, drop_scale=1.1)


def _base(ptrs, lds, **more):
    return dict({f: PTR for f in ptrs}, **{f: 128 for f in lds}, **_SHAPE, **more)


def _each(fields, change, code, what):
    return [(f"{what} {f}", {f: change}, code) for f in fields]


def _dims(code):
    return [(f"{f} = {v}", {f: v}, code) for f in ("B", "H", "Tq", "Tk") for v in (0, -1)] + \
           [("Tq = 257", dict(Tq=257), code), ("Tk = 257", dict(Tk=257), code), ("D = 96", dict(D=96), code)]


# ---- unimm_attn_fwd: pointers, shape, alignment, then the variable-length and segment words
FWD_BASE = _base(_FWD_PTRS, _FWD_LD)
FWD_CASES = (
    _each(["q", "k", "v", "out", "mask"], None, E_ARG, "null") + _dims(E_SHAPE) +
    _each(_FWD_LD, 60, E_ALIGN, "60 =") + _each(["q", "k", "v", "out"], OFF8, E_ALIGN, "8 bytes off:") + [
        ("q_off without q_len", dict(q_off=PTR), E_ARG),
        ("q_len without q_off", dict(q_len=PTR), E_ARG),
        ("k_off without k_len", dict(k_off=PTR), E_ARG),
        ("ks_off without ks_len", dict(_SEG, ks_len=None), E_ARG),
        ("ks_off without k_off", dict(ks_off=PTR, ks_len=PTR, ks_ins=1), E_ARG),
        ("ks_ins = -1", dict(_SEG, ks_ins=-1), E_ARG),
        ("dropout with a shared segment", dict(_SEG, **_DROP), E_ARG),
        ("Tq = 257 and ldq = 60", dict(Tq=257, ldq=60), E_SHAPE),
        ("null k and D = 96", dict(k=None, D=96), E_ARG),
        ("D = 96 and q 8 bytes off", dict(D=96, q=OFF8), E_SHAPE),
        ("ldq = 60 and q_off without q_len", dict(ldq=60, q_off=PTR), E_ALIGN),
        ("v 8 bytes off and ks_off without ks_len", dict(_SEG, ks_len=None, v=OFF8), E_ALIGN),
    ])

# ---- unimm_attn_probs: reads q, k and the mask only, fixed layout only -- and says so before it looks at the shape
PROBS_BASE = _base(["q", "k", "mask"], ["ldq", "ldk"], ldv=0, ldo=0, probs=PTR)
PROBS_CASES = (
    _each(["q", "k", "mask", "probs"], None, E_ARG, "null") + _dims(E_SHAPE) +
    _each(["ldq", "ldk"], 60, E_ALIGN, "60 =") + _each(["q", "k"], OFF8, E_ALIGN, "8 bytes off:") +
    _each(_VAR + ["ks_off", "ks_len"], PTR, E_ARG, "set:") + [
        ("a whole variable-length description", dict({f: PTR for f in _VAR}), E_ARG),
        ("q_off and Tq = 257", dict(q_off=PTR, Tq=257), E_ARG),
        ("k_len and ldk = 60", dict(k_len=PTR, ldk=60), E_ARG),
        ("Tq = 257 and ldq = 60", dict(Tq=257, ldq=60), E_SHAPE),
        ("null k and D = 96", dict(k=None, D=96), E_ARG),
    ])

# ---- unimm_attn_bwd
BWD_BASE = _base(_BWD_PTRS, _BWD_LD)
_BWD_ALIGNED = ["q", "k", "v", "out", "dout", "dq", "dk", "dv"]
BWD_CASES = (
    _each(_BWD_PTRS, None, E_ARG, "null") + _dims(E_SHAPE) +
    _each(_BWD_LD, 60, E_ALIGN, "60 =") + _each(_BWD_ALIGNED, OFF8, E_ALIGN, "8 bytes off:") + [
        ("q_off without q_len", dict(q_off=PTR), E_ARG),
        ("k_off without k_len", dict(k_off=PTR), E_ARG),
        ("k_len without k_off", dict(k_len=PTR), E_ARG),
        ("Tq = 257 and ldq = 60", dict(Tq=257, ldq=60), E_SHAPE),
        ("null delta and D = 96", dict(delta=None, D=96), E_ARG),
        ("D = 96 and dv 8 bytes off", dict(D=96, dv=OFF8), E_SHAPE),
        ("lddk = 60 and q_off without q_len", dict(lddk=60, q_off=PTR), E_ALIGN),
        ("dq 8 bytes off and k_off without k_len", dict(dq=OFF8, k_off=PTR), E_ALIGN),
    ])

# ---- the spliced entries: every word of the layout is required, and a shape they do not take is an argument error, answered
# before alignment; max_tq = 32 (unimm_attn_spliced_*) or 64 (unimm_attn_spliced_wide_*)
_SPL = dict({f: PTR for f in _VAR}, ks_off=PTR, ks_len=PTR, ks_ins=1)


def _spliced_common(max_tq):
    return (_each(_VAR + ["ks_off", "ks_len"], None, E_ARG, "null") + _dims(E_ARG) + [
        ("ks_ins = -1", dict(ks_ins=-1), E_ARG),
        ("D = 128", dict(D=128), E_ARG),
        (f"Tq = {max_tq + 1}", dict(Tq=max_tq + 1), E_ARG),
        ("Tq = 257 and ldq = 60", dict(Tq=257, ldq=60), E_ARG),
        (f"Tq = {max_tq + 1} and q 8 bytes off", dict(Tq=max_tq + 1, q=OFF8), E_ARG),
        ("null k and D = 96", dict(k=None, D=96), E_ARG),
        ("null ks_len and ldk = 60", dict(ks_len=None, ldk=60), E_ARG),
    ])


SPL_FWD_BASE = _base(_FWD_PTRS, _FWD_LD, **_SPL)


def spl_fwd_cases(max_tq):
    return (_each(_FWD_PTRS, None, E_ARG, "null") + _spliced_common(max_tq) +
            _each(_FWD_LD, 60, E_ALIGN, "60 =") + _each(["q", "k", "v", "out"], OFF8, E_ALIGN, "8 bytes off:"))


SPL_BWD_BASE = _base(_BWD_PTRS, _BWD_LD, **_SPL, delta=None, g_first=PTR, g_seq=PTR, G=1, accumulate=0)


def spl_bwd_cases(max_tq):
    return (_each([f for f in _BWD_PTRS if f != "delta"] + ["g_first", "g_seq"], None, E_ARG, "null") + _spliced_common(max_tq) +
            _each(_BWD_LD, 60, E_ALIGN, "60 =") + _each(_BWD_ALIGNED, OFF8, E_ALIGN, "8 bytes off:") + [
                ("G = 0", dict(G=0), E_ARG),
                ("G = 0 and lddq = 60", dict(G=0, lddq=60), E_ARG),
            ])


# entry point -> (argument struct, accepted arguments, cases)
ENTRIES = {
    "unimm_attn_fwd": (lib.AttnArgs, FWD_BASE, FWD_CASES),
    "unimm_attn_probs": (lib.AttnArgs, PROBS_BASE, PROBS_CASES),
    "unimm_attn_bwd": (lib.AttnBwdArgs, BWD_BASE, BWD_CASES),
    "unimm_attn_spliced_fwd": (lib.AttnArgs, SPL_FWD_BASE, spl_fwd_cases(32)),
    "unimm_attn_spliced_wide_fwd": (lib.AttnArgs, SPL_FWD_BASE, spl_fwd_cases(64)),
    "unimm_attn_spliced_bwd": (lib.AttnSplicedBwdArgs, SPL_BWD_BASE, spl_bwd_cases(32)),
    "unimm_attn_spliced_wide_bwd": (lib.AttnSplicedBwdArgs, SPL_BWD_BASE, spl_bwd_cases(64)),
}


def _codes(entry, address, stream):
    """Every case of the entry -> [(case, expected, returned)]; address(field) = the valid address a PTR / OFF8 field stands for."""
    struct, base, cases = ENTRIES[entry]
    fn = getattr(lib.lib(), entry)
    names = {f for f, _ in struct._fields_}

    def call(fields):
        a = struct()
        probs = None
        for f, v in fields.items():
            if v == PTR or v == OFF8:
                v = address(f) + (8 if v == OFF8 else 0)
            if f == "probs":
                probs = v
            else:
                assert f in names, f
                setattr(a, f, v)
        return fn(C.byref(a), probs, stream) if entry == "unimm_attn_probs" else fn(C.byref(a), stream)

    got = [("null struct", E_ARG, fn(None, address("probs"), stream) if entry == "unimm_attn_probs" else fn(None, stream))]
    for name, change, want in cases:
        assert any(base.get(f) != v for f, v in change.items()), (name, "changes nothing")
        got.append((name, want, call(dict(base, **change))))
    return got


def _wrong(got):
    return [(name, lib._ERR.get(want, want), lib._ERR.get(rc, rc)) for name, want, rc in got if rc != want]


@pytest.mark.skipif(torch.cuda.is_available(), reason="made-up addresses: only where nothing can be launched")
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_refusal_codes_without_a_gpu(entry):
    fields = sorted({f for _, base, _ in ENTRIES.values() for f in base})
    got = _codes(entry, lambda f: 0x10000 * (1 + fields.index(f)), None)
    assert len(got) >= 30 and _wrong(got) == []


@pytest.mark.gpu
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_refusals_write_nothing(entry):
    from tests.test_gpu_attention_edges import DEV, NAN16, NAN32, _nan_like
    rows, width = 264, 2 * 64 + 8                                   # room for Tq = Tk = 257 and for a view 4 elements in
    ins = {f: torch.randn((rows, width), device=DEV).bfloat16() for f in ("q", "k", "v", "dout")}
    ins["mask"] = torch.full((rows, 16), -1, dtype=torch.int32, device=DEV)
    ins.update({f: torch.zeros(8, dtype=torch.int32, device=DEV) for f in _VAR + ["ks_off", "ks_len", "g_first", "g_seq"]})
    outs = {f: _nan_like(rows, width, False) for f in ("dq", "dk", "dv")}
    outs.update(lse=_nan_like(2, rows, True), delta=_nan_like(2, rows, True), probs=_nan_like(2 * rows, rows, True))
    if entry.endswith("bwd"):
        ins.update(out=torch.randn((rows, width), device=DEV).bfloat16(), lse=torch.zeros((2, rows), device=DEV))
        del outs["lse"]
    else:
        outs["out"] = _nan_like(rows, width, False)
    bufs = dict(ins, **outs)
    got = _codes(entry, lambda f: bufs[f].data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert len(got) >= 30 and _wrong(got) == []
    for f, t in outs.items():
        bits = t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)
        assert bool((bits == (NAN16 if t.dtype == torch.bfloat16 else NAN32)).all()), f"{entry}: a refused call wrote to {f}"
