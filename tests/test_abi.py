"""CPU-side checks of the drop-in boundary: the C-ABI library builds for gfx950, loads, and exports
every symbol include/unimm_hip.h declares (no compute call is made without a GPU); the binding's signature table, argument
structs and constants (unimm_amd/lib.py) equal what the header declares, read by tests/header_reader.py and, for the struct
layout, by the host C compiler."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from tests import header_reader as HR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


@pytest.fixture(scope="module")
def built_lib():
    from unimm_amd import build
    return build.build()


@pytest.fixture(scope="module")
def header():
    with open(os.path.join(INCLUDE, "unimm_hip.h")) as f:
        return f.read()


def test_library_exports_every_declared_symbol(built_lib):
    hdr = open(os.path.join(ROOT, "include", "unimm_hip.h")).read()
    declared = set(re.findall(r"\b(unimm_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) >= 4
    so = ctypes.CDLL(built_lib)
    for name in sorted(declared):
        assert hasattr(so, name), f"{name} declared in include/unimm_hip.h but not exported"
    from unimm_amd import lib
    assert set(lib.SYMBOLS) == declared


def test_version_and_arch(built_lib):
    from unimm_amd import lib
    L = lib.lib()
    assert L.unimm_version() == lib.ABI_VERSION
    assert L.unimm_arch() == b"gfx950"


def test_signature_table_equals_the_header_prototypes(header):
    """names, result type and every argument type in order, under the fixed C -> ctypes mapping of header_reader.ctype"""
    from unimm_amd import lib
    assert len(HR.prototypes(header)) == len(lib.SYMBOLS) >= 76
    assert HR.signature_mismatches(header, lib.SIGNATURES) == []
    assert [p[0] for p in HR.prototypes(header)] == lib.SYMBOLS                    # the table is in header order
    assert HR.streamed(header) == lib._STREAMED                                    # where `_call` appends the stream


def test_loaded_library_has_every_signature_applied(built_lib):
    from unimm_amd import lib
    L = lib.lib()
    for name in lib.SYMBOLS:
        fn, (restype, argtypes) = getattr(L, name), lib.SIGNATURES[name]
        assert fn.argtypes is not None and list(fn.argtypes) == list(argtypes), name
        assert fn.restype is restype, name


def test_struct_registry_equals_the_header_structs(header):
    """every `typedef struct` of the header has a ctypes mirror with the same field names, order, types and array lengths"""
    from unimm_amd import lib
    assert len(HR.structs(header)) == len(lib.STRUCTS) >= 15
    assert HR.struct_mismatches(header, lib.STRUCTS) == []


def _host_cc():
    cc = shutil.which("cc")
    if cc:
        return cc
    for rocm in filter(None, (os.environ.get("ROCM_PATH"), "/opt/rocm")):
        for sub in ("llvm/bin/clang", "lib/llvm/bin/clang"):
            if os.path.exists(os.path.join(rocm, sub)):
                return os.path.join(rocm, sub)
    return None


def test_struct_layout_equals_the_host_compilers(header, tmp_path):
    """sizeof of every struct and offsetof of every field, as the host C compiler lays the header out, equal ctypes' layout of
    the mirrors: a check independent of the reader's type mapping."""
    from unimm_amd import lib
    cc = _host_cc()
    if cc is None:
        pytest.skip("no host C compiler (cc, or the clang of the ROCm installation)")
    src, exe = tmp_path / "layout_probe.c", tmp_path / "layout_probe"
    src.write_text(HR.layout_probe_source(header))
    subprocess.run([cc, "-std=c99", "-I", INCLUDE, str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    printed = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    compiled = dict(line.split() for line in printed.splitlines())
    mine = {}
    for name, cls in lib.STRUCTS.items():
        mine[name] = str(ctypes.sizeof(cls))
        mine.update({f"{name}.{f}": str(getattr(cls, f).offset) for f, _ in cls._fields_})
    assert len(compiled) > 15 and compiled == mine


def test_constants_equal_the_header(header):
    from unimm_amd import lib
    c = HR.constants(header)
    assert c["UNIMM_OK"] == 0
    assert {name: code for code, name in lib._ERR.items()} == {n: v for n, v in c.items() if n.startswith("UNIMM_E_")}
    assert len(lib._ERR) == 4
    assert (lib.ADAMW_MAX_GROUPS, lib.NDCG_MAX_OPTIONS, lib.NDCG_MAX_ITER) == \
        (c["UNIMM_ADAMW_MAX_GROUPS"], c["UNIMM_NDCG_MAX_OPTIONS"], c["UNIMM_NDCG_MAX_ITER"])
    for prefix, count in (("EPI_", 8), ("X3_", 4)):
        theirs = {n[len("UNIMM_"):]: v for n, v in c.items() if n.startswith("UNIMM_" + prefix)}
        assert len(theirs) == count and theirs == {n: getattr(lib, n, None) for n in theirs}, prefix
    dt = {n[len("UNIMM_DT_"):]: v for n, v in c.items() if n.startswith("UNIMM_DT_")}
    assert lib._DT == {torch.bool: dt["U8"], torch.uint8: dt["U8"], torch.int32: dt["I32"], torch.int64: dt["I64"],
                       torch.float32: dt["F32"]} and len(dt) == 4


def _mutated(text, old, new):
    assert text.count(old) == 1, old
    return text.replace(old, new)


def test_a_header_that_differs_is_reported(header):
    """The comparisons above run on mutated copies of the header text: each must name the struct or symbol that was touched (a
    reader that skipped what it cannot read would pass everything)."""
    from unimm_amd import lib
    swapped = _mutated(header, "int32_t lddy, ldx, lddw;", "int32_t ldx, lddy, lddw;")              # two adjacent fields swapped
    found = HR.struct_mismatches(swapped, lib.STRUCTS)
    assert len(found) == 2 and all(m.startswith("unimm_gemm_tn_args: field ") for m in found), found
    assert HR.signature_mismatches(swapped, lib.SIGNATURES) == []

    widened = _mutated(header, "int unimm_colsum(const void* dy, float* db, int32_t M,", "int unimm_colsum(const void* dy, float* db, int64_t M,")
    found = HR.signature_mismatches(widened, lib.SIGNATURES)
    assert len(found) == 1 and found[0].startswith("unimm_colsum: arguments "), found

    removed = _mutated(header, "int unimm_gelu_bwd(const void* dt, const void* u, void* du, int64_t n, void* stream);", "")
    assert HR.signature_mismatches(removed, lib.SIGNATURES) == ["unimm_gelu_bwd: in the table, not declared in the header"]

    resized = _mutated(header, "float* dst[4];", "float* dst[8];")                                   # one array length changed
    found = HR.struct_mismatches(resized, lib.STRUCTS)
    assert len(found) == 1 and found[0].startswith("unimm_finish_desc: field 1 is dst (c_void_p, length 8) in the header"), found

    for broken in (_mutated(header, "int32_t tile;", "unsigned int tile;"),                           # what the reader cannot read raises
                   _mutated(header, "int unimm_prof_tag(int32_t tag);", "int unimm_prof_tag(int32_t);")):
        with pytest.raises(ValueError):
            HR.struct_mismatches(broken, lib.STRUCTS), HR.signature_mismatches(broken, lib.SIGNATURES)
