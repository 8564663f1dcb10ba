"""What the compiler made of every kernel: registers, spills, scratch and static LDS, read from the metadata notes of the gfx950
code objects inside a built library or object file (nothing is recompiled, disassembled or run).

    python -m tests.kernel_resources [path] [substring]   the table (default path: unimm_amd/libunimm_hip.so)
    python -m tests.kernel_resources --write              regenerate tests/golden/kernel_resources.json from the built library

tests/test_kernel_resources_cpu.py holds the library to that ledger and to what the sources and documents say about its kernels;
tools/obj_regs.py prints through this reader."""
from __future__ import annotations

import json
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile
from typing import NamedTuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LEDGER = os.path.join(ROOT, "tests", "golden", "kernel_resources.json")
REGENERATE = "python -m tests.kernel_resources --write"
TRIPLE = b"hipv4-amdgcn-amd-amdhsa--gfx950"
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
VGPR_GRANULE, VGPR_FILE, MAX_WAVES, LDS_CU_BYTES = 8, 512, 8, 160 * 1024     # per lane and SIMD; per CU


class Res(NamedTuple):
    """One kernel's row of the notes.  vgpr_count already includes agpr_count."""
    vgpr_count: int
    agpr_count: int
    sgpr_count: int
    vgpr_spill_count: int
    sgpr_spill_count: int
    private_segment_fixed_size: int
    group_segment_fixed_size: int
    max_flat_workgroup_size: int
    uses_dynamic_stack: bool

    @property
    def allocation(self) -> int:
        """registers a wave of this kernel takes out of its SIMD's file: whole granules of 8"""
        return max(VGPR_GRANULE, -(-self.vgpr_count // VGPR_GRANULE) * VGPR_GRANULE)

    @property
    def waves_per_simd(self) -> int:
        """as far as registers decide (LDS and the launch may allow fewer)"""
        return min(MAX_WAVES, VGPR_FILE // self.allocation)

    @property
    def workgroups_per_cu_static_lds(self):
        """as far as the kernel's static LDS decides; None without any (dynamic LDS is the launch's, and not in the notes)"""
        g = self.group_segment_fixed_size
        return LDS_CU_BYTES // g if g else None


FIELDS = Res._fields


class ToolMissing(RuntimeError):
    pass


def llvm_tool(name: str) -> str:
    """the LLVM tools live next to the compiler hipcc drives"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    for d in (os.path.join(rocm, "llvm", "bin"), os.path.join(rocm, "lib", "llvm", "bin"),
              "/opt/rocm/llvm/bin", "/opt/rocm/lib/llvm/bin"):
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    raise ToolMissing(f"{name} not found next to hipcc ({hipcc})")


def code_objects(data: bytes) -> list:
    """every gfx950 device ELF in the offload bundles of a library or object file, in file order"""
    out = []
    for m in re.finditer(re.escape(BUNDLE_MAGIC), data):
        base = m.start()
        (n,) = struct.unpack_from("<Q", data, base + len(BUNDLE_MAGIC))
        o = base + len(BUNDLE_MAGIC) + 8
        if n > 64:                                       # the magic as a string of some other section, not a bundle header
            continue
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", data, o)
            triple = data[o + 24:o + 24 + tl]
            o += 24 + tl
            if triple == TRIPLE and size:
                elf = data[base + off:base + off + size]
                if elf[:4] != b"\x7fELF":
                    raise ValueError(f"bundle entry at {base + off:#x} is not an ELF image")
                out.append(elf)
    return out


_KEY = re.compile(r"^(?:  - |    )\.(\w+):\s*(.*)$")      # a key of a kernel's own map (argument maps sit deeper)


def parse_notes(text: str) -> list:
    """[(mangled name, Res)] of one code object's `llvm-readelf --notes`"""
    kernels, cur, inside = [], None, False
    for line in text.splitlines():
        if not inside:
            inside = line.startswith("amdhsa.kernels:")
            continue
        if line[:1] not in (" ", ""):                    # the next top-level key (amdhsa.target, ...) ends the list
            break
        if line.startswith("  - "):
            cur = {}
            kernels.append(cur)
        m = _KEY.match(line)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2).strip()
    out = []
    for k in kernels:
        missing = [f for f in FIELDS + ("name",) if f not in k]
        if missing:
            raise ValueError(f"kernel note without {missing}: {k.get('name', '?')}")
        vals = [k[f] == "true" if f == "uses_dynamic_stack" else int(k[f]) for f in FIELDS]
        out.append((k["name"].strip("'\""), Res(*vals)))
    return out


def demangle(names: list) -> list:
    if not names:
        return []
    tool = shutil.which("c++filt")
    if tool is None:
        try:
            tool = llvm_tool("llvm-cxxfilt")
        except ToolMissing:
            raise ToolMissing("neither c++filt nor llvm-cxxfilt found")
    out = subprocess.run([tool], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(names)
    return [d.replace("(anonymous namespace)::", "") for d in out]


def read_objects(path: str) -> list:
    """one {demangled kernel name: Res} per gfx950 code object of `path`"""
    readelf = llvm_tool("llvm-readelf")
    with open(path, "rb") as f:
        elfs = code_objects(f.read())
    if not elfs:
        raise ValueError(f"no {TRIPLE.decode()} code object in {path}")
    tables = []
    with tempfile.TemporaryDirectory() as tmp:
        for i, elf in enumerate(elfs):
            co = os.path.join(tmp, f"{i}.co")
            with open(co, "wb") as f:
                f.write(elf)
            r = subprocess.run([readelf, "--notes", co], capture_output=True, text=True, check=True)
            recs = parse_notes(r.stdout)
            tables.append(dict(zip(demangle([n for n, _ in recs]), (res for _, res in recs))))
            if len(tables[-1]) != len(recs):
                raise ValueError(f"two kernels of code object {i} demangle to one name")
    return tables


def read(lib_path: str) -> dict:
    """{demangled kernel name: Res} of every kernel in the file"""
    out = {}
    for table in read_objects(lib_path):
        for name, res in table.items():
            if name in out:
                raise ValueError(f"kernel {name} is in two code objects of {lib_path}")
            out[name] = res
    return out


def toolchain_id() -> str:
    """the compiler's version line and the flags the library is built with: the ledger's figures hold for this pair only"""
    from unimm_amd import build as B
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    txt = subprocess.run([hipcc, "--version"], capture_output=True, text=True, check=True).stdout
    line = next((l for l in txt.splitlines() if "clang version" in l), txt.splitlines()[0])
    return line.strip() + " | " + " ".join(B.FLAGS)


def dumps(table: dict, toolchain: str) -> str:
    """the ledger's text: one compact line per kernel, sorted by name, fields in FIELDS order"""
    lines = ["{", ' "toolchain_id": ' + json.dumps(toolchain) + ",", ' "fields": ' + json.dumps(list(FIELDS)) + ",",
             ' "kernels": {']
    rows = [f"  {json.dumps(n)}: {json.dumps([int(v) for v in table[n]], separators=(',', ':'))}" for n in sorted(table)]
    lines.append(",\n".join(rows))
    lines += [" }", "}"]
    return "\n".join(lines) + "\n"


def load_ledger(path: str = LEDGER):
    """(toolchain_id, {name: Res})"""
    with open(path) as f:
        j = json.load(f)
    assert tuple(j["fields"]) == FIELDS, "the ledger was written with other fields: " + REGENERATE
    return j["toolchain_id"], {n: Res(*v[:-1], bool(v[-1])) for n, v in j["kernels"].items()}


def format_row(name: str, r: Res) -> str:
    return (f"vgpr {r.vgpr_count:>3} agpr {r.agpr_count:>3} sgpr {r.sgpr_count:>3} spill {r.vgpr_spill_count:>3} "
            f"sspill {r.sgpr_spill_count:>3} scratch {r.private_segment_fixed_size:>4} lds {r.group_segment_fixed_size:>6} "
            f"wg {r.max_flat_workgroup_size:>4} waves {r.waves_per_simd}  {name[:130]}")


def main(argv: list) -> int:
    from unimm_amd import lib
    if "--write" in argv:
        tables = read_objects(lib.LIB_PATH)
        table = read(lib.LIB_PATH)
        with open(LEDGER, "w") as f:
            f.write(dumps(table, toolchain_id()))
        print(f"{LEDGER}: {len(table)} kernels in {len(tables)} code objects")
        return 0
    if argv and not os.path.exists(argv[0]):             # a substring alone: the built library
        argv = [lib.LIB_PATH] + argv
    path = argv[0] if argv else lib.LIB_PATH
    flt = argv[1] if len(argv) > 1 else ""
    for name, r in read(path).items():
        if flt in name:
            print(format_row(name, r))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
