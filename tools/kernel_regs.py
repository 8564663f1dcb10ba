"""Print VGPR / spill / scratch of every kernel in a hipcc -S listing:  python tools/kernel_regs.py file.s [substring]
(a listing carries the same metadata text as a code object's notes: parsed by tests/kernel_resources.py, as tools/obj_regs.py)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import kernel_resources as KR

flt = sys.argv[2] if len(sys.argv) > 2 else ""
txt = open(sys.argv[1]).read()
recs = [r for part in txt.split(".amdgpu_metadata")[1:] for r in KR.parse_notes(part.split(".end_amdgpu_metadata")[0])]
for d, (_, r) in zip(KR.demangle([n for n, _ in recs]), recs):
    if flt in d:
        print(KR.format_row(d, r))
