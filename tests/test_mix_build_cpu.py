"""The extension library libunimm_mix.so without a GPU, by the means tests/test_abi.py and tests/test_kernel_resources_cpu.py hold
the main library with: it builds for gfx950 and exports what include/unimm_mix.h declares; the binding's signature table and argument
struct (unimm_amd/mix.py) equal the header, for the struct's layout by the host C compiler too; its kernel's registers, spills,
scratch and static LDS are those of tests/golden/kernel_resources_mix.json (regenerate: `python -m tests.test_mix_build_cpu --write`);
and the main library holds no kernel of it and exports nothing of it."""
import ctypes
import os
import subprocess
import sys

import pytest

from tests import header_reader as HR
from tests import kernel_resources as KR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
LEDGER = os.path.join(ROOT, "tests", "golden", "kernel_resources_mix.json")


@pytest.fixture(scope="module")
def built():
    from unimm_amd import build, mix
    build.build()
    assert os.path.exists(mix.LIB_PATH) and mix.LIB_PATH == build.MIX_LIB
    return mix.LIB_PATH


@pytest.fixture(scope="module")
def header():
    """the extension header's own text: what it includes (unimm_hip.h) is the main library's and is checked by tests/test_abi.py"""
    with open(os.path.join(INCLUDE, "unimm_mix.h")) as f:
        return f.read().replace('#include "unimm_hip.h"', "")


def test_library_exports_what_the_header_declares(built, header):
    from unimm_amd import lib, mix
    names = [p[0] for p in HR.prototypes(header)]
    assert names == list(mix.SIGNATURES) == ["unimm_mix_version", "unimm_lm_mix"]
    so = ctypes.CDLL(built)
    for name in names:
        assert hasattr(so, name), name
    assert mix.lib().unimm_mix_version() == mix.ABI_VERSION
    assert HR.signature_mismatches(header, mix.SIGNATURES) == []
    assert HR.streamed(header) == {"unimm_lm_mix"}
    main = ctypes.CDLL(lib.LIB_PATH)                         # the main library and its table know nothing of the extension
    assert not any(hasattr(main, n) for n in names) and not set(names) & set(lib.SYMBOLS)


def test_struct_equals_the_header_and_the_host_compilers_layout(header, tmp_path):
    from tests.test_abi import _host_cc
    from unimm_amd import mix
    assert list(HR.structs(header)) == list(mix.STRUCTS) == ["unimm_lm_mix_args"]
    assert HR.struct_mismatches(header, mix.STRUCTS) == []
    c = HR.constants(header)
    assert (c["UNIMM_MIX_MAX_MEMBERS"], c["UNIMM_MIX_LOGIT"], c["UNIMM_MIX_PROB"]) == (mix.MAX_MEMBERS, mix.LOGIT, mix.PROB)
    assert mix.MODES == {"logit": mix.LOGIT, "prob": mix.PROB}
    cc = _host_cc()
    if cc is None:
        pytest.skip("no host C compiler (cc, or the clang of the ROCm installation)")
    src, exe = tmp_path / "layout_probe.c", tmp_path / "layout_probe"
    src.write_text(HR.layout_probe_source(header).replace('#include "unimm_hip.h"', '#include "unimm_mix.h"'))
    subprocess.run([cc, "-std=c99", "-I", INCLUDE, str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    compiled = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    cls = mix.LmMixArgs
    mine = {"unimm_lm_mix_args": str(ctypes.sizeof(cls))}
    mine.update({f"unimm_lm_mix_args.{f}": str(getattr(cls, f).offset) for f, _ in cls._fields_})
    assert compiled == mine and len(mine) == 15


def test_kernel_resources_are_the_ledgers(built):
    """one kernel, no scratch, no spills, no dynamic stack; under the ledger's toolchain every field equals the ledger"""
    from unimm_amd import lib
    table = KR.read(built)
    want_id, want = KR.load_ledger(LEDGER)
    assert set(table) == set(want) == {"lm_mix_kernel(MixParams)"}
    (r,) = table.values()
    assert (r.vgpr_spill_count, r.sgpr_spill_count, r.private_segment_fixed_size, r.uses_dynamic_stack) == (0, 0, 0, False)
    assert r.max_flat_workgroup_size == 256 and r.group_segment_fixed_size <= 16 * 1024
    assert not set(table) & set(KR.read(lib.LIB_PATH))
    if KR.toolchain_id() != want_id:
        pytest.skip(f"another toolchain than the ledger's ({want_id!r}): exact figures are not compared; the rest ran")
    assert table == want
    with open(LEDGER) as f:
        assert f.read() == KR.dumps(table, want_id), "the ledger's text is not what --write writes"


if __name__ == "__main__":
    if "--write" in sys.argv:
        from unimm_amd import mix
        with open(LEDGER, "w") as f:
            f.write(KR.dumps(KR.read(mix.LIB_PATH), KR.toolchain_id()))
        print(LEDGER)
