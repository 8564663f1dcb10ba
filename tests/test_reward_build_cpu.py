"""The extension library libunimm_reward.so without a GPU, by the means tests/test_mix_build_cpu.py holds libunimm_mix.so with: it
builds for gfx950 and exports what include/unimm_reward.h declares; the binding's signature table and argument struct
(unimm_amd/reward_abi.py) equal the header, for the struct's layout by the host C compiler too; its kernel's registers, spills,
scratch and static LDS are those of tests/golden/kernel_resources_reward.json (regenerate: `python -m tests.test_reward_build_cpu
--write`); and the other two libraries hold no kernel of it and export nothing of it."""
import ctypes
import os
import subprocess
import sys

import pytest

from tests import header_reader as HR
from tests import kernel_resources as KR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
LEDGER = os.path.join(ROOT, "tests", "golden", "kernel_resources_reward.json")


@pytest.fixture(scope="module")
def built():
    from unimm_amd import build, reward_abi
    build.build()
    assert os.path.exists(reward_abi.LIB_PATH) and reward_abi.LIB_PATH == build.REWARD_LIB
    return reward_abi.LIB_PATH


@pytest.fixture(scope="module")
def header():
    """the extension header's own text: what it includes (unimm_hip.h) is the main library's and is checked by tests/test_abi.py"""
    with open(os.path.join(INCLUDE, "unimm_reward.h")) as f:
        return f.read().replace('#include "unimm_hip.h"', "")


def test_library_exports_what_the_header_declares(built, header):
    from unimm_amd import lib, mix, reward_abi
    names = [p[0] for p in HR.prototypes(header)]
    assert names == list(reward_abi.SIGNATURES) == ["unimm_reward_version", "unimm_ngram_reward"]
    so = ctypes.CDLL(built)
    for name in names:
        assert hasattr(so, name), name
    assert reward_abi.lib().unimm_reward_version() == reward_abi.ABI_VERSION
    assert HR.signature_mismatches(header, reward_abi.SIGNATURES) == []
    assert HR.streamed(header) == {"unimm_ngram_reward"}
    for other in (lib.LIB_PATH, mix.LIB_PATH):               # the other libraries and their tables know nothing of the extension
        so = ctypes.CDLL(other)
        assert not any(hasattr(so, n) for n in names)
    assert not set(names) & (set(lib.SYMBOLS) | set(mix.SIGNATURES))


def test_struct_equals_the_header_and_the_host_compilers_layout(header, tmp_path):
    from tests.test_abi import _host_cc
    from unimm_amd import reward_abi as A
    assert list(HR.structs(header)) == list(A.STRUCTS) == ["unimm_ngram_reward_args"]
    assert HR.struct_mismatches(header, A.STRUCTS) == []
    c = HR.constants(header)
    assert (c["UNIMM_REWARD_MAX_LEN"], c["UNIMM_REWARD_MAX_REFS"], c["UNIMM_REWARD_ORDERS"]) == (A.MAX_LEN, A.MAX_REFS, A.ORDERS)
    assert (c["UNIMM_NGRAM_EMPTY"], c["UNIMM_NGRAM_HASH_BASIS"], c["UNIMM_NGRAM_HASH_PRIME"]) == (A.EMPTY, A.HASH_BASIS, A.HASH_PRIME)
    assert sum(A.MAX_LEN - n for n in range(A.ORDERS)) == 250 < 256
    cc = _host_cc()
    if cc is None:
        pytest.skip("no host C compiler (cc, or the clang of the ROCm installation)")
    src, exe = tmp_path / "layout_probe.c", tmp_path / "layout_probe"
    src.write_text(HR.layout_probe_source(header).replace('#include "unimm_hip.h"', '#include "unimm_reward.h"'))
    subprocess.run([cc, "-std=c99", "-I", INCLUDE, str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    compiled = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    cls = A.NgramRewardArgs
    mine = {"unimm_ngram_reward_args": str(ctypes.sizeof(cls))}
    mine.update({f"unimm_ngram_reward_args.{f}": str(getattr(cls, f).offset) for f, _ in cls._fields_})
    assert compiled == mine and len(mine) == 21


def test_kernel_resources_are_the_ledgers(built):
    """one kernel, no scratch, no spills, no dynamic stack; under the ledger's toolchain every field equals the ledger"""
    from unimm_amd import lib, mix
    table = KR.read(built)
    want_id, want = KR.load_ledger(LEDGER)
    assert set(table) == set(want) == {"ngram_reward_kernel(RewardParams)"}
    (r,) = table.values()
    assert (r.vgpr_spill_count, r.sgpr_spill_count, r.private_segment_fixed_size, r.uses_dynamic_stack) == (0, 0, 0, False)
    assert r.max_flat_workgroup_size == 256 and r.group_segment_fixed_size <= 8 * 1024
    assert not set(table) & (set(KR.read(lib.LIB_PATH)) | set(KR.read(mix.LIB_PATH)))
    if KR.toolchain_id() != want_id:
        pytest.skip(f"another toolchain than the ledger's ({want_id!r}): exact figures are not compared; the rest ran")
    assert table == want
    with open(LEDGER) as f:
        assert f.read() == KR.dumps(table, want_id), "the ledger's text is not what --write writes"


if __name__ == "__main__":
    if "--write" in sys.argv:
        from unimm_amd import reward_abi
        with open(LEDGER, "w") as f:
            f.write(KR.dumps(KR.read(reward_abi.LIB_PATH), KR.toolchain_id()))
        print(LEDGER)
