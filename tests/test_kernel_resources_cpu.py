"""What the compiler made of every kernel of libunimm_hip.so -- registers, spills, scratch, static LDS -- held to a ledger
(tests/golden/kernel_resources.json) and to what the header, DESIGN.md and the source comments say about it.  Needs the built
library and the LLVM tools next to hipcc, no GPU: the metadata notes of the code objects are read (tests/kernel_resources.py),
nothing is disassembled or run.

  a. the library's kernels are the ledger's                         c. every documented figure holds for the library just read
  b. no dynamic stack anywhere; spills and scratch only where        d. under the ledger's toolchain: every field of every kernel
     ALLOWED_SCRATCH lists them, at exactly the listed bytes         e. the reader and the checks of b and c see what they must

After a change that moves a figure on purpose: `python -m tests.kernel_resources --write`, then update the statement and its row."""
import fnmatch
import os
import shutil
import subprocess

import pytest

from tests import kernel_resources as KR
from unimm_amd import build as B
from unimm_amd import lib

HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
pytestmark = pytest.mark.skipif(HIPCC is None, reason="no hipcc on this machine: the library cannot have been built here")

# ---- b. the kernels that may spill.  pattern -> (vgpr_spill_count, bytes of scratch per lane, why it is tolerated).  The figures
# are the ledger's: more fails, and so does less (take the row out, or lower it, when a kernel improves).
ALLOWED_SCRATCH = {
    "attn_spliced_bwd_kernel(*": (4, 20, "shared-context backward, untuned (DESIGN.md 5.2); spills sit outside the matrix loops"),
    "attn_spliced_wide_bwd_kernel(*": (63, 256, "8 waves per workgroup cap a wave at 256; loop invariants of the walk, reloaded per answer"),
    "attn_bwd_dkv_kernel<128, 2, 512>(*": (27, 112, "37 x 37 image self-attention backward at two waves per SIMD; cost never measured"),
    "attn_bwd_dkv_kernel<128, 8, 512>(*": (16, 68, "D = 128 with Tq, Tk > 64 (more than 64 regions): not a shape of the benchmarked model; cost never measured"),
    "gemm_ntp_kernel<Cfg<2, 4, 8, 64, 2, 0, 0>, 2, false>(*": (8, 36, "persistent 256x256 dropout-residual epilogue with a bf16 output: both engines take its fp32 sibling, which fits 256"),
    "x3m_attn_bwd_dkv_kernel<128>(*": (3, 16, "fp32x3 engine dK / dV at D = 128 on the two-waves-per-SIMD budget"),
}

# ---- c. what the project states about its kernels: (kernel pattern, {kind: figure}, file, line, words of the statement on that line).
# kinds: registers (N or (lo, hi): vgpr_count, AGPRs included), registers_max, agprs (agpr_count), spilled (vgpr_spill_count), scratch (bytes per lane),
# waves (waves per SIMD that the registers allow, exactly), waves_min (a launch-bound promise: at least so many).
# "no spills" is spilled = 0, "no scratch" is spilled = 0 and scratch = 0.
H, D, A, G, GH, X, O, P, DI = ("include/unimm_hip.h", "DESIGN.md", "unimm_amd/csrc/attention.hip", "unimm_amd/csrc/gemm_nt.h",
                               "unimm_amd/csrc/gemm.hip", "unimm_amd/csrc/x3ops.hip", "unimm_amd/csrc/optim.hip",
                               "unimm_amd/csrc/policy.hip", "unimm_amd/csrc/distill.hip")
NO_SCRATCH = {"spilled": 0, "scratch": 0}
ABSENT = {"absent": True}                           # the statement says that the library holds no such kernel
CLAIMS = [
    # shared-context attention backward
    ("attn_spliced_bwd_kernel(*", {"registers": 256, "spilled": 4, "scratch": 20}, H, 258, "4 of its 256 registers are spilled: 20 bytes of scratch per lane"),
    ("attn_spliced_bwd_kernel(*", {"registers": 256, "spilled": 4, "scratch": 20}, A, 1538, "Registers: 256, 4 of them spilled (20 bytes of scratch per lane)"),
    ("attn_spliced_bwd_kernel(*", {"registers": 256, "spilled": 4, "scratch": 20}, D, 346, "256 registers, 4 of them spilled: 20 bytes of scratch per lane"),
    ("attn_spliced_wide_bwd_kernel(*", {"registers": 256, "spilled": 63, "scratch": 256}, D, 346, "256 registers with 63 spilled (256 bytes of scratch per lane)"),
    ("attn_spliced_wide_bwd_kernel(*", {"registers": 256, "spilled": 63, "scratch": 256, "waves": 2}, A, 1848, "the kernel takes 256 with 63 spilled (256 bytes of scratch per lane)"),
    # attention backward, the kernel pair
    ("attn_bwd_dkv_kernel<128, 8, 256>(*", {"registers": 312, "spilled": 0, "waves": 1}, A, 526, "attn_bwd_dkv_kernel<128, 8, 256> (312 registers, no spills)"),
    ("attn_bwd_dkv_kernel<128, 2, 256>(*", ABSENT, A, 527, "and <128, 2, 256> is never instantiated"),
    ("attn_bwd_dkv_kernel<128, 2, 512>(*", {"registers": 256, "spilled": 27, "scratch": 112, "waves": 2}, A, 528, "is 256 registers with 27 spilled"),
    ("attn_bwd_dkv_kernel<128, 2, 512>(*", {"scratch": 112}, A, 529, "112 bytes of scratch per lane"),
    ("attn_bwd_dkv_kernel<128, 8, 512>(*", {"registers": 256, "spilled": 16, "scratch": 68, "waves": 2}, A, 529, "256 with 16 spilled, 68 bytes"),
    ("attn_bwd_dkv_kernel<64, 8, 512>(*", {"registers": 228, "waves": 2}, A, 715, "which the 228-register dK / dV kernel was already"),
    ("attn_bwd_dkv_kernel<128, 8, 256>(*", {"registers": 312}, A, 1354, "(110 us, 312 registers)"),
    # the one-kernel backward forms and the few-query forward
    ("attn_bwd_fewq128_kernel<2>(*", {"registers_max": 256, "spilled": 0}, A, 1187, "phases so that it fits 256 registers"),
    ("attn_bwd_fewq128_kernel<2>(*", {"registers": 192, **NO_SCRATCH}, D, 493, "192 registers, no spills, 148 KiB of LDS"),
    ("attn_bwd_fewk128_kernel(*", {"registers": 200}, D, 501, "200 registers, 150 KiB."),
    ("attn_fwd_fewq128_kernel(*", {"registers": 122}, D, 423, "122 registers, 116 KiB of LDS"),
    ("attn_fwd_kernel<64, 8>(*", {"waves_min": 2}, A, 2142, "4 waves walk the 8 query tiles: two workgroups per CU"),
    # fp32x3 attention
    ("x3m_attn_fwd_kernel<64, 4, false>(*", {"registers": 78}, D, 459, "VGPRs 78 / 104 / 136 at D = 64"),
    ("x3m_attn_fwd_kernel<64, 8, false>(*", {"registers": 104}, D, 459, "VGPRs 78 / 104 / 136 at D = 64"),
    ("x3m_attn_fwd_kernel<64, 16, false>(*", {"registers": 136}, D, 459, "VGPRs 78 / 104 / 136 at D = 64"),
    ("x3m_attn_fwd_kernel<128, 4, false>(*", {"registers": 118}, D, 459, "118 / 142 / 179 at D = 128"),
    ("x3m_attn_fwd_kernel<128, 8, false>(*", {"registers": 142}, D, 459, "118 / 142 / 179 at D = 128"),
    ("x3m_attn_fwd_kernel<128, 16, false>(*", {"registers": 179}, D, 459, "118 / 142 / 179 at D = 128"),
    ("x3m_attn_fwd_kernel<64, 4, true>(*", {"registers": 78, **NO_SCRATCH}, D, 460, "the spliced ones 78 / 104 / 136 and 118 / 140 / 178, no scratch"),
    ("x3m_attn_fwd_kernel<64, 8, true>(*", {"registers": 104, **NO_SCRATCH}, D, 460, "the spliced ones 78 / 104 / 136 and 118 / 140 / 178, no scratch"),
    ("x3m_attn_fwd_kernel<64, 16, true>(*", {"registers": 136, **NO_SCRATCH}, D, 460, "the spliced ones 78 / 104 / 136 and 118 / 140 / 178, no scratch"),
    ("x3m_attn_fwd_kernel<128, 4, true>(*", {"registers": 118, **NO_SCRATCH}, D, 460, "the spliced ones 78 / 104 / 136 and 118 / 140 / 178, no scratch"),
    ("x3m_attn_fwd_kernel<128, 8, true>(*", {"registers": 140, **NO_SCRATCH}, D, 460, "the spliced ones 78 / 104 / 136 and 118 / 140 / 178, no scratch"),
    ("x3m_attn_fwd_kernel<128, 16, true>(*", {"registers": 178, **NO_SCRATCH}, D, 460, "the spliced ones 78 / 104 / 136 and 118 / 140 / 178, no scratch"),
    ("x3m_attn_bwd_dkv_kernel<128>(*", {"registers": 256, "spilled": 3, "scratch": 16, "waves": 2}, X, 1052, "takes all 256 registers and spills 3: 16 bytes of scratch per lane"),
    ("x3m_attn_bwd_dkv_kernel<64>(*", {"registers": 206}, X, 1052, "D = 64: 206)"),
    ("x3_attn_fwd_kernel<*", {"registers": (176, 184), "waves": 2}, X, 1288, "176-184 registers: two waves per SIMD either way"),
    ("x3_attn_bwd_d*_kernel<*, 32>(*", {"waves_min": 2}, X, 404, "which is what lets the backward kernels keep two waves per SIMD"),
    # NT GEMM: workgroups per CU that the tile comments and the launch bounds promise, as waves per SIMD (4-wave workgroups)
    ("gemm_nt*_kernel<Cfg<2, 2, 4, 64, 2, 0, 0>, *", {"waves_min": 2, "spilled": 0}, G, 70, "128x128, 4 waves, 68 KiB LDS -> 2 workgroups per CU"),
    ("gemm_nt*_kernel<Cfg<2, 2, 2, 64, 2, 0, 0>, *", {"waves_min": 3, "spilled": 0}, G, 74, "(48 KiB, 3 workgroups per CU)"),
    ("gemm_nt*_kernel<Cfg<2, 2, 4, 64, 2, 0, 3>, *", {"waves_min": 2, "spilled": 0}, "unimm_amd/csrc/gemm_nt_cfg14.hip", 1, "80 KiB, two workgroups per CU"),
    ("gemm_nt*_kernel<Cfg<2, 2, 2, 64, 2, 0, 3>, *", {"waves_min": 2, "spilled": 0}, "unimm_amd/csrc/gemm_nt_cfg15.hip", 1, "56 KiB, two workgroups per CU"),
    ("gemm_nt*_kernel<Cfg<2, 4, *", {"waves_min": 2}, G, 98, "waves per SIMD the launch bounds ask for.  As built, every instance has them"),
    ("gemm_ntp_kernel<Cfg<2, 4, 8, 64, 2, 0, 0>, 2, false>(*", {"registers": 256, "spilled": 8, "scratch": 36}, G, 99, "takes 256 registers with 8 spilled (36 bytes of scratch per lane"),
    ("gemm_ntp_kernel<Cfg<2, 4, 8, 64, 2, 0, 0>, 2, true>(*", {"registers": 256, **NO_SCRATCH}, G, 99, "its fp32 sibling"),
    ("gemm_ntp_kernel<Cfg<2, 2, 4, 64, 3, 0, 0>, 2, false>(*", {"registers": 260, "waves": 1, **NO_SCRATCH}, G, 100, "takes 260: one wave per SIMD"),
    ("gemm_nt*_kernel<Cfg<2, 2, 4, 64, 3, 0, 0>, *", {"registers_max": 512, "waves_min": 1, **NO_SCRATCH}, G, 780, "one workgroup per CU, hence a 512-register"),
    ("gemm_nt_kernel<Cfg<2, 4, 6, 64, 2, 0, 3>, 2, true, false>(*", {"registers": 180}, D, 230, "(180 / 228 VGPRs"),
    ("gemm_ntp_kernel<Cfg<2, 4, 6, 64, 2, 0, 3>, 2, true>(*", {"registers": 228}, D, 230, "(180 / 228 VGPRs"),
    ("gemm_nt_kernel<Cfg<2, 4, 6, 64, 2, 0, 3>, 2, true, true>(*", {"registers": 192}, D, 231, "and the mapped one takes 192"),
    ("gemm_nt*_kernel<Cfg<2, 2, 4, 64, 3, 0, 0>, *", {"agprs": 64}, G, 781, "keeps them in AGPRs"),
    ("gemm_nt*_kernel<Cfg<2, 2, 2, 64, 2, 0, 0>, *", {"waves_min": 3}, GH, 694, "take the 64x128 tile (three workgroups per CU"),
    ("gemm_nt*_kernel<Cfg<2, 2, 2, 64, 3, 0, 0>, *", {"waves_min": 2, "spilled": 0}, GH, 727, "9 = 64x128 (72 KiB: two workgroups per CU)"),
    ("gemm_nt*_kernel<Cfg<2, 2, 4, 64, 3, 0, 0>, *", {"waves_min": 1, "spilled": 0}, GH, 727, "10 = 128x128 (96 KiB: one per CU)"),
    ("gemm_ntp2_kernel*", ABSENT, D, 580, "the experiment's kernels, which are not in the library, took 245-256 registers without spills"),
    # TN GEMM
    ("gemm_tn_kernel<2, 2, 4>(*", {"waves_min": 2, "spilled": 0}, GH, 235, "64 KiB LDS (2 workgroups per CU)"),
    ("gemm_tn_kernel<2, 4, 8>(*", {"waves_min": 2, "spilled": 0}, GH, 236, "256x256 tile, 8 waves, 128 KiB LDS"),
    ("gemm_tn_pp_kernel(*", {"waves_min": 2, "spilled": 0}, GH, 440, "__launch_bounds__(512, 2) void gemm_tn_pp_kernel"),
    # optimizer
    ("grad_sumsq_kernel(*", {"waves": 8}, O, 93, "8 resident waves per SIMD on 256 CUs"),
    ("adamw_kernel<*", {"waves": 8}, O, 203, "8 of them resident at a time (8 waves per SIMD)"),
    # LM-head objectives
    ("pg_loss_fwd_kernel<true>(*", {"waves": 8}, P, 98, "6 waves per SIMD instead of the 8 of the pair without a reference"),
    ("pg_loss_*_kernel<false>(*", {"waves": 8}, P, 98, "6 waves per SIMD instead of the 8 of the pair without a reference"),
    ("pg_loss_fwd_kernel<true>(*", {"registers": 59, "waves": 8}, D, 303, "59 VGPRs, the plain forward's 8 waves"),
    ("pg_loss_fwd_kernel<false>(*", {"waves": 8}, D, 303, "59 VGPRs, the plain forward's 8 waves"),
    ("distill_loss_fwd_kernel<true>(*", {"registers": 56, "waves": 8, **NO_SCRATCH}, DI, 13, "distill_loss_fwd_kernel<true>   56 VGPRs, no scratch, 8 waves per SIMD"),
    ("distill_loss_fwd_kernel<false>(*", {"registers": 32, "waves": 8, **NO_SCRATCH}, DI, 15, "distill_loss_fwd_kernel<false>  32 VGPRs, no scratch, 8 waves per SIMD"),
    ("distill_loss_bwd_kernel(*", {"registers": 28, "waves": 8, **NO_SCRATCH}, DI, 16, "distill_loss_bwd_kernel         28 VGPRs, no scratch, 8 waves per SIMD"),
]


def _matches(pattern, name):
    return fnmatch.fnmatchcase(name[5:] if name.startswith("void ") else name, pattern)


def _select(table, pattern):
    return {n: r for n, r in table.items() if _matches(pattern, n)}


def check_invariants(table, allowed=ALLOWED_SCRATCH):
    """(b) as a list of complaints, each naming its kernel"""
    bad = []
    listed = {}
    for pat, (spill, scratch, why) in allowed.items():
        hit = _select(table, pat)
        if len(hit) != 1:
            bad.append(f"ALLOWED_SCRATCH[{pat!r}] names {len(hit)} kernels, not one")
        for n in hit:
            listed[n] = (spill, scratch)
    for name, r in table.items():
        if r.uses_dynamic_stack:
            bad.append(f"{name}: uses a dynamic stack")
        spill, scratch = listed.get(name, (0, 0))
        got = (r.vgpr_spill_count, r.private_segment_fixed_size)
        if got == (spill, scratch):
            continue
        if name not in listed:
            bad.append(f"{name}: {got[0]} VGPRs spilled, {got[1]} bytes of scratch per lane; it is not in ALLOWED_SCRATCH")
        elif got[0] > spill or got[1] > scratch:
            bad.append(f"{name}: spills grew to {got[0]} VGPRs / {got[1]} bytes (ALLOWED_SCRATCH: {spill} / {scratch})")
        else:
            bad.append(f"{name}: now {got[0]} VGPRs spilled / {got[1]} bytes, ALLOWED_SCRATCH still says {spill} / {scratch}: "
                       "lower or remove its row (and the statements about it)")
    return bad


def _figure_ok(kind, want, r):
    if kind == "registers":
        return want[0] <= r.vgpr_count <= want[1] if isinstance(want, tuple) else r.vgpr_count == want
    if kind == "registers_max":
        return r.vgpr_count <= want
    if kind == "spilled":
        return r.vgpr_spill_count == want
    if kind == "scratch":
        return r.private_segment_fixed_size == want
    if kind == "agprs":
        return r.agpr_count == want
    if kind == "waves":
        return r.waves_per_simd == want
    if kind == "waves_min":
        return r.waves_per_simd >= want
    raise KeyError(kind)


def check_claims(table, claims=CLAIMS):
    """(c) as a list of complaints, each naming its kernel and the statement's file and line"""
    bad = []
    for pat, figures, path, line, words in claims:
        hit = _select(table, pat)
        if figures == ABSENT:
            bad += [f"{path}:{line}: \"{words}\" -- but the library has {name}" for name in hit]
            continue
        if not hit:
            bad.append(f"{path}:{line}: no kernel matches {pat!r} (\"{words}\")")
        for name, r in hit.items():
            for kind, want in figures.items():
                if not _figure_ok(kind, want, r):
                    bad.append(f"{path}:{line}: \"{words}\" -- {name}: {kind} {want} stated, the library has vgpr {r.vgpr_count} "
                               f"(allocation {r.allocation}, {r.waves_per_simd} waves per SIMD), {r.vgpr_spill_count} spilled, "
                               f"{r.private_segment_fixed_size} bytes of scratch")
    return bad


def check_statements(claims=CLAIMS):
    """every row of CLAIMS quotes words that stand on its line of its file: a statement edited or moved without its row fails here"""
    bad, cache = [], {}
    for _, _, path, line, words in claims:
        if path not in cache:
            with open(os.path.join(KR.ROOT, path), encoding="utf-8") as f:
                cache[path] = f.read().splitlines()
        lines = cache[path]
        if 1 <= line <= len(lines) and words in lines[line - 1]:
            continue
        now = [i + 1 for i, l in enumerate(lines) if words in l]
        bad.append(f"{path}:{line}: \"{words}\" is not on that line" +
                   (f" (it is on line {now[0]}: update the row)" if now else ": the statement was changed; CLAIMS holds what the build gives"))
    return bad


@pytest.fixture(scope="module")
def table():
    assert os.path.exists(lib.LIB_PATH), f"{lib.LIB_PATH} is not built (python -m unimm_amd.build)"
    return KR.read(lib.LIB_PATH)          # a missing LLVM tool raises: a failure, not a skip


@pytest.fixture(scope="module")
def ledger():
    return KR.load_ledger()


def test_a_the_set_of_kernels_is_the_ledgers(table, ledger):
    names = set(ledger[1])
    added, lost = sorted(set(table) - names), sorted(names - set(table))
    assert not added and not lost, ("kernels in the library but not in the ledger:\n  " + "\n  ".join(added) +
                                    "\nkernels in the ledger but not in the library:\n  " + "\n  ".join(lost) +
                                    f"\nif that is intended: {KR.REGENERATE}")


def test_b_no_dynamic_stack_and_scratch_only_where_listed(table, ledger):
    bad = check_invariants(table)
    assert not bad, "\n".join(bad)
    for pat, (spill, scratch, why) in ALLOWED_SCRATCH.items():        # the caps are today's ledger values, each with its reason
        (r,) = _select(ledger[1], pat).values()
        assert (r.vgpr_spill_count, r.private_segment_fixed_size) == (spill, scratch), pat
        assert why.strip() and "\n" not in why, pat


def test_c_documented_figures_hold_for_this_library(table):
    bad = check_statements() + check_claims(table)
    assert not bad, "\n".join(bad)


def test_d_every_field_equals_the_ledger_under_its_toolchain(table, ledger):
    want_id, want = ledger
    have_id = KR.toolchain_id()
    if have_id != want_id:
        pytest.skip(f"another toolchain ({have_id!r}, the ledger is of {want_id!r}): exact figures are not compared; a to c still ran")
    diff = []
    for name in sorted(set(table) & set(want)):
        if table[name] != want[name]:
            moved = ", ".join(f"{f} {getattr(want[name], f)} -> {getattr(table[name], f)}" for f in KR.FIELDS
                              if getattr(want[name], f) != getattr(table[name], f))
            diff.append(f"{name}: {moved}")
    assert not diff, "\n".join(diff) + f"\nif that is intended: {KR.REGENERATE}"
    with open(KR.LEDGER) as f:
        same = f.read() == KR.dumps(table, have_id)
    assert same, f"the ledger's text is not what {KR.REGENERATE} writes"


# ---- e. the reader and the checks see what they must
INDEXED_SRC = """#include <hip/hip_runtime.h>
__global__ void indexed_kernel(float* out, const int* idx, int n) {
  float a[512];                                     // per-thread, indexed at run time: it has to live in scratch
  for (int i = 0; i < n; ++i) a[idx[i] & 511] = out[i];
  float s = 0.f;
  for (int i = 0; i < n; ++i) s += a[idx[n + i] & 511];
  out[threadIdx.x] = s;
}
"""
CROWDED_SRC = """#include <hip/hip_runtime.h>
__global__ __launch_bounds__(1024) void crowded_kernel(const float* in, float* out, int n) {
  float v[200];                                     // 200 values live across the loop; 1024 threads leave a lane 128 registers
#pragma unroll
  for (int i = 0; i < 200; ++i) v[i] = in[i * 1024 + threadIdx.x];
  for (int k = 0; k < n; ++k) {
#pragma unroll
    for (int i = 0; i < 200; ++i) v[i] = fmaf(v[i], v[(i + 1) % 200], in[k]);
  }
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 200; ++i) s += v[i];
  out[threadIdx.x] = s;
}
"""


def _compile(tmp_path, stem, src):
    path = tmp_path / (stem + ".hip")
    path.write_text(src)
    obj = tmp_path / (stem + ".o")
    r = subprocess.run([HIPCC] + B.FLAGS + ["-c", str(path), "-o", str(obj)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return KR.read(str(obj))


def test_e_reader_sees_scratch_of_a_runtime_indexed_array(tmp_path):
    t = _compile(tmp_path, "indexed", INDEXED_SRC)
    (name,) = t
    assert name.startswith("indexed_kernel(") and t[name].private_segment_fixed_size >= 512 * 4, t
    assert any(name in b for b in check_invariants(t, allowed={}))


def test_e_reader_sees_spills_under_launch_bounds_the_body_cannot_meet(tmp_path):
    t = _compile(tmp_path, "crowded", CROWDED_SRC)
    (name,) = t
    r = t[name]
    assert name.startswith("crowded_kernel(") and r.max_flat_workgroup_size == 1024, t
    assert r.vgpr_count <= 128 and r.vgpr_spill_count > 0 and r.private_segment_fixed_size > 0, r
    assert any(name in b for b in check_invariants(t, allowed={}))


def test_e_checks_report_an_added_spill_and_a_register_over_a_step_by_name(table):
    assert not check_invariants(table) and not check_claims(table)
    clean = "void distill_loss_fwd_kernel<true>"
    (victim,) = [n for n in table if n.startswith(clean)]
    edited = dict(table)
    edited[victim] = table[victim]._replace(vgpr_spill_count=1, private_segment_fixed_size=4)
    bad = check_invariants(edited)
    assert len(bad) == 1 and victim in bad[0] and "not in ALLOWED_SCRATCH" in bad[0], bad
    (victim,) = [n for n in table if n.startswith("grad_sumsq_kernel(")]          # optim.hip: 8 waves per SIMD = allocation <= 64
    edited = dict(table)
    edited[victim] = table[victim]._replace(vgpr_count=65)
    assert edited[victim].allocation == 72 and edited[victim].waves_per_simd == 7
    bad = check_claims(edited)
    assert len(bad) == 1 and victim in bad[0] and "unimm_amd/csrc/optim.hip:93" in bad[0], bad
    (victim,) = [n for n in table if n.startswith("attn_spliced_bwd_kernel(")]    # a listed kernel that stops spilling must leave the list
    edited = dict(table)
    edited[victim] = table[victim]._replace(vgpr_spill_count=0, private_segment_fixed_size=0)
    bad = check_invariants(edited)
    assert len(bad) == 1 and victim in bad[0] and "lower or remove" in bad[0], bad
    edited[victim] = table[victim]._replace(vgpr_spill_count=5, private_segment_fixed_size=24)
    bad = check_invariants(edited)
    assert len(bad) == 1 and victim in bad[0] and "grew" in bad[0], bad


def test_e_derived_values_follow_the_register_file():
    r = KR.Res(0, 0, 0, 0, 0, 0, 0, 256, False)
    for vgpr, alloc, waves in ((1, 8, 8), (57, 64, 8), (64, 64, 8), (65, 72, 7), (80, 80, 6), (96, 96, 5), (128, 128, 4),
                               (129, 136, 3), (168, 168, 3), (169, 176, 2), (256, 256, 2), (257, 264, 1), (512, 512, 1)):
        x = r._replace(vgpr_count=vgpr)
        assert (x.allocation, x.waves_per_simd) == (alloc, waves), vgpr
    assert r.workgroups_per_cu_static_lds is None
    assert r._replace(group_segment_fixed_size=49152).workgroups_per_cu_static_lds == 3
    assert r._replace(group_segment_fixed_size=160 * 1024).workgroups_per_cu_static_lds == 1
