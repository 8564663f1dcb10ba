"""VGPR / spill / scratch / LDS of every kernel in a built object or library (no recompilation: the device ELF is cut out of
the offload bundle and its notes are read):  python tools/obj_regs.py unimm_amd/csrc/_obj/gemm.o [substring]
The reader is tests/kernel_resources.py, the one the suite holds the library to (tests/test_kernel_resources_cpu.py)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import kernel_resources as KR

flt = sys.argv[2] if len(sys.argv) > 2 else ""
for name, r in KR.read(sys.argv[1]).items():
    if flt in name:
        print(KR.format_row(name, r))
