"""float64 restatement of ONE unimm_gemm_tn_grouped_ws call (include/unimm_hip.h), for the edge tests
(tests/test_gpu_gemm_tn_edges.py, tests/test_gemm_tn_ref_cpu.py): what the C ABI defines and what the launcher decides, so
that a test does not re-derive either.

  * `problem`  -- dw[N, K] += dy[:live, :N]^T x[:live, :K] and dbias[N] += column sums of dy[:live, :N] in float64 (torch, on
                  the device the operands live on), with the magnitude sums S = |dy|^T |x| and S_b = sum |dy| the gate needs.
                  dy / x / live may be LISTS: the problems of a group that alias one dw (and, where `bias` says so, one
                  dbias); the references and magnitude sums are then the sums over the aliasing problems;
  * `colsums`  -- one dbias alone (problems of different dw that alias a dbias);
  * `gate`, `gate_b` -- the per-element error budget E of section "gate" below;
  * `is_big`, `launches`, `splits`, `rows_per_split`, `nsplit`, `ws_bytes`, `uses_ws`, `takes_lock_step`, `kernel`,
    `dw_joins`, `bias_joins`, `plan` -- the host rules of the launcher (unimm_amd/csrc/gemm.hip: launch_tn_group and
                  unimm_gemm_tn_grouped_ws): which launches a call makes, which kernel symbol each runs, how the reduction
                  is split, whether the workspace is used and how many fp32 additions join partial results in an element;
  * `pp_num_records` -- the 32-bit arithmetic of the ping-pong kernel's buffer descriptor, for the 4 GiB guard's CPU test.

Gate.  For element (n, k) of dw and (n) of dbias with float64 reference ref:  |got - ref| <= E,  E = the sum of

  accumulation   min(C_ACC, live) * 2^-24 * S,  S = sum_m |dy[m,n]| |x[m,k]| (dbias: S_b = sum_m |dy[m,n]|).  A bf16 x bf16
                 product has 16 significant bits and is exact in fp32, so only the additions round; any order of live - 1
                 correctly rounded fp32 additions of terms whose magnitudes sum to S is within (live - 1) 2^-24 S of the
                 exact sum, hence the cap at `live`.  C_ACC is oracle/gemm_ref.py's 32.  Its basis FOR THIS PRODUCT is
                 measured and re-asserted by tests/test_gemm_tn_ref_cpu.py: torch's CPU float32 dy.T @ x on bf16-valued
                 operands, standard-normal along the reduction axis, x1e3 and x1e-3 scales on output rows and columns,
                 reduction lengths 1 .. 61,440, three seeds: worst |err| / (2^-24 S) = 2.50, so the 8 x margin of 32 holds
                 (8 x: the matrix instruction's internal order over its 32 products, the 64-row steps, the split of M).
                 The same product with one reduction row dropped falls outside E on 0.80 - 1.00 of the elements.
                 SCALES ALONG THE REDUCTION AXIS BREAK THE CONSTANT: x1e3 on some rows of dy and x measured 12.0 at 64 rows
                 (every later addition rounds at the loud magnitude while S stays dominated by few terms).  The operands
                 of these tests are therefore well-scaled along M, and all hostility goes into N and K: loud / quiet columns
                 of dy and x (= rows and columns of dw), cancelling priors.
                 The constant may only be raised by re-measuring a CPU reference that accumulates in the kernel's structure
                 (fp32, 32-row blocks, sequential over blocks), with the 8 x margin, rounded up to a power of two and the
                 figures written here: never fitted to a kernel's own error.
  joins          J * 2^-24 * (|prior| + S),  J = the number of fp32 additions that bring partial results into the element:
                 for dw one per contributing (problem, split that owns rows) -- on the atomic path each is one memory-side
                 atomic, on the workspace path the last arriver adds the other slabs to its registers (nsplit - 1) and the
                 sum to dw (1) --; for dbias one per contributing (problem, split that owns rows, tile column that owns
                 reduction steps): the 128x128 and the lock-step 256x256 kernels sum the bias in tile column 0 only, the
                 ping-pong kernel deals step t to tile column t mod nbk.  Each join is one correctly rounded addition
                 whose operands are bounded by |prior| + S.  J comes from `dw_joins` / `bias_joins`, not from a fit.
  dw and dbias are fp32: no output-rounding term."""
from __future__ import annotations

from collections import namedtuple

import torch

from oracle.gemm_ref import C_ACC, U32, worst_ratio  # noqa: F401  (worst_ratio: re-exported for the tests)

TK = 64                   # reduction rows per step
TN_MAXG = 48              # problems per launch (csrc/gemm.hip: kernel-argument limit)
COUNTER_BYTES = 16384     # the first 16 KiB of a workspace: one int32 arrival counter per tile
MAX_WS_TILES = 4096
MAX_SPLITS = 32
PP, LOCK_STEP, SMALL = "gemm_tn_pp", "gemm_tn<256x256 lock-step>", "gemm_tn<128x128>"     # lib.gemm_variant_name

# One problem as the launcher sees it.  m_dev: a device row count is given; lddy / ldx: leading dimensions (elements), only
# needed for the 4 GiB guard (None = small).
Prob = namedtuple("Prob", "M N K m_dev lddy ldx", defaults=(False, None, None))


def _p(p):
    return p if isinstance(p, Prob) else Prob(*p)


def is_big(M, N, K):
    """The 256x256 class (ping-pong, or the lock-step loop on request / behind the 4 GiB guard); else 128x128."""
    return N >= 256 and K >= 256 and M >= 1024


def tile_dim(big):
    return 256 if big else 128


def tiles(N, K, big):
    tb = tile_dim(big)
    return -(-N // tb) * -(-K // tb)


def launches(problems):
    """-> [(big, [indices into `problems` in descriptor order])], one entry per kernel launch, in launch order: the big class
    first, then the small one; each class in caller order cut into chunks of at most 48; inside a chunk a STABLE sort by
    descending M (problems of one row count keep the caller's order)."""
    problems = [_p(p) for p in problems]
    out = []
    for big in (True, False):
        sel = [i for i, p in enumerate(problems) if is_big(p.M, p.N, p.K) == big]
        for c0 in range(0, len(sel), TN_MAXG):
            chunk = sel[c0:c0 + TN_MAXG]
            out.append((big, sorted(chunk, key=lambda i: -problems[i].M)))       # sorted() is stable
    return out


def splits(chunk, shared=False):
    """Reduction ranges per tile of one launch (the same for every problem of it).  chunk: the launch's problems (one class).
    Workgroups run in rounds of 256 (big) or 512 slots; cost of s splits = rounds(tiles s) x (steps of the longest problem / s
    + a fixed cost of 8 steps, 40 with the chip-sharing hint); s = 1 .. clamp(max M // 1024, 1, 32) in rising order, a new s
    wins only when its cost is below 0.98 of the best so far."""
    chunk = [_p(p) for p in chunk]
    big = is_big(chunk[0].M, chunk[0].N, chunk[0].K)
    slots = 256 if big else 512
    ntiles = sum(tiles(p.N, p.K, big) for p in chunk)
    max_m = max(p.M for p in chunk)
    max_s = min(max(max_m // 1024, 1), MAX_SPLITS)
    steps = max_m / TK
    best, s = 1e30, 1
    for sp in range(1, max_s + 1):
        rounds = -(-(ntiles * sp) // slots)
        cost = rounds * (steps / sp + (40.0 if shared else 8.0))
        if cost < best * 0.98:
            best, s = cost, sp
    return s


def rows_per_split(M, nsplits):
    """ceil(M / splits) rounded up to whole 64-row steps."""
    return -(-(-(-M // nsplits)) // TK) * TK


def nsplit(M, nsplits):
    """Splits of a problem that own rows (a short problem of a group has fewer than the group's `splits`)."""
    return -(-M // rows_per_split(M, nsplits))


def single_rows_per_split(M, N, K, shared=False):
    """rows_per_split of one problem alone in its launch (tests/test_gpu_row_edges.py: the edges of a device row count)."""
    return rows_per_split(M, splits([Prob(M, N, K)], shared))


def ws_bytes(chunk, nsplits=None, shared=False):
    """Workspace one launch needs: 16 KiB of counters + tiles x splits x tile^2 x 4 bytes of partial tiles."""
    chunk = [_p(p) for p in chunk]
    big = is_big(chunk[0].M, chunk[0].N, chunk[0].K)
    s = splits(chunk, shared) if nsplits is None else nsplits
    tb = tile_dim(big)
    return COUNTER_BYTES + sum(tiles(p.N, p.K, big) for p in chunk) * s * tb * tb * 4


def uses_ws(chunk, ws, shared=False):
    """Does the launch meet its splits in the workspace (`ws` bytes given, None = no workspace)?  Only with more than one
    split, no device row count in the chunk (a split without rows would never arrive at the counter), at most 4096 tiles
    and a workspace that holds ws_bytes(); otherwise every split adds with atomics."""
    chunk = [_p(p) for p in chunk]
    big = is_big(chunk[0].M, chunk[0].N, chunk[0].K)
    s = splits(chunk, shared)
    return (ws is not None and s > 1 and not any(p.m_dev for p in chunk)
            and sum(tiles(p.N, p.K, big) for p in chunk) <= MAX_WS_TILES and ws_bytes(chunk, s) <= ws)


def pp_num_records(rows, ld):
    """num_records of the ping-pong kernel's buffer descriptor as the kernel computes it: rows * ld * 2 in 32 bits."""
    return (rows * ld * 2) & 0xFFFFFFFF


def takes_lock_step(chunk, shared=False):
    """The 4 GiB guard: a big-class launch holding a problem whose split spans >= 2^32 bytes of dy or x runs the lock-step
    loop (64-bit addressing) instead of the ping-pong loop (32-bit descriptors and offsets)."""
    chunk = [_p(p) for p in chunk]
    s = splits(chunk, shared)
    return any(rows_per_split(p.M, s) * max(p.lddy or p.N, p.ldx or p.K) * 2 >= 1 << 32 for p in chunk)


def kernel(chunk, shared=False, lock_step=False):
    """Kernel symbol of the launch (lib.gemm_variant_name).  lock_step: bit 1 of shared_chip was given."""
    chunk = [_p(p) for p in chunk]
    if not is_big(chunk[0].M, chunk[0].N, chunk[0].K):
        return SMALL
    return LOCK_STEP if lock_step or takes_lock_step(chunk, shared) else PP


def live_rows(M, count=None):
    """Rows that count: min(M, device count), never negative."""
    return M if count is None else max(0, min(M, count))


def dw_joins(M, nsplits, count=None):
    """fp32 additions that bring partial results into an element of dw from ONE problem: its splits that own live rows."""
    live = live_rows(M, count)
    return -(-live // rows_per_split(M, nsplits))


def bias_joins(M, K, nsplits, kern, count=None):
    """fp32 additions into an element of dbias from ONE problem run by kernel `kern` with `nsplits` group splits: per split
    that owns live rows, one (128x128 and lock-step: tile column 0 holds the sums) or, for the ping-pong kernel, one per
    tile column that owns reduction steps (tile column tk sums steps t = tk mod nbk: min(nbk, steps of the split))."""
    live = live_rows(M, count)
    rps = rows_per_split(M, nsplits)
    j = 0
    for s in range(-(-live // rps)):
        rows = min(rps, live - s * rps)
        j += min(-(-K // 256), -(-rows // TK)) if kern == PP else 1
    return j


def plan(problems, shared=False, lock_step=False, ws=None):
    """Everything the launcher decides for one call.  -> list of dicts, one per launch in launch order:
    big, order (indices into `problems`, descriptor order), kernel, splits, ws (bool: workspace used), ws_bytes, tiles,
    tile0 (first tile of each descriptor), nsplit (per descriptor)."""
    problems = [_p(p) for p in problems]
    out = []
    for big, order in launches(problems):
        chunk = [problems[i] for i in order]
        s = splits(chunk, shared)
        nt = [tiles(p.N, p.K, big) for p in chunk]
        out.append(dict(big=big, order=order, kernel=kernel(chunk, shared, lock_step), splits=s, ws=uses_ws(chunk, ws, shared),
                        ws_bytes=ws_bytes(chunk, s), tiles=sum(nt), tile0=[sum(nt[:i]) for i in range(len(nt))],
                        nsplit=[nsplit(p.M, s) for p in chunk]))
    return out


def joins(problems, shared=False, lock_step=False, counts=None):
    """-> ([J_dw per problem], [J_dbias per problem]) in caller order for one call (counts: device row counts or None)."""
    problems = [_p(p) for p in problems]
    counts = counts if counts is not None else [None] * len(problems)
    jw, jb = [0] * len(problems), [0] * len(problems)
    for L in plan(problems, shared, lock_step):
        for i in L["order"]:
            p = problems[i]
            jw[i] = dw_joins(p.M, L["splits"], counts[i])
            jb[i] = bias_joins(p.M, p.K, L["splits"], L["kernel"], counts[i])
    return jw, jb


def colsums(dy, prior_b, live, N):
    """One dbias in float64: prior_b [N] + column sums of dy[:live, :N]; dy / live may be lists (the problems that alias it).
    -> dict(ref_b, S_b, acc_b)."""
    if not isinstance(dy, (list, tuple)):
        dy, live = [dy], [live]
    dev = dy[0].device
    ref_b = prior_b.double().to(dev).clone()
    S_b = torch.zeros(N, dtype=torch.float64, device=dev)
    acc_b = torch.zeros_like(S_b)
    for d, lv in zip(dy, live):
        dd = d[:lv, :N].double()
        ref_b += dd.sum(0)
        Sb = dd.abs().sum(0)
        S_b += Sb
        acc_b += min(C_ACC, float(lv)) * U32 * Sb
    return dict(ref_b=ref_b, S_b=S_b, acc_b=acc_b)


def problem(dy, x, prior_w, prior_b, live, N, K, bias=None):
    """One dw (and one dbias) in float64.  dy [>= live, >= N], x [>= live, >= K] bf16 (views allowed), prior_w [N, K] and
    prior_b [N] (or None) what dw / dbias held before, live = rows that count.  dy, x and live may be lists of equal length:
    the problems that alias this dw; `bias` then says which of them also add into this dbias (default: all).
    -> dict(ref_w, ref_b, S, S_b, acc_w, acc_b): float64 [N, K] / [N]; S = sum |dy|^T |x|, S_b = sum |dy| over the problems;
    acc_w / acc_b = the accumulation term of the gate (sum over the problems of min(C_ACC, live_i) 2^-24 S_i).
    `gate` adds the join term."""
    if not isinstance(dy, (list, tuple)):
        dy, x, live = [dy], [x], [live]
    bias = [True] * len(dy) if bias is None else list(bias)
    dev = dy[0].device
    ref_w = prior_w.double().to(dev).clone()
    S = torch.zeros((N, K), dtype=torch.float64, device=dev)
    acc_w = torch.zeros_like(S)
    for d, xx, lv in zip(dy, x, live):
        dd, xd = d[:lv, :N].double(), xx[:lv, :K].double()
        ref_w += dd.t() @ xd
        Si = dd.abs().t() @ xd.abs()
        S += Si
        acc_w += min(C_ACC, float(lv)) * U32 * Si
    out = dict(ref_w=ref_w, S=S, acc_w=acc_w, ref_b=None, S_b=None, acc_b=None)
    if prior_b is not None:
        out.update(colsums([d for d, b in zip(dy, bias) if b], prior_b, [lv for lv, b in zip(live, bias) if b], N)
                   if any(bias) else dict(ref_b=prior_b.double().to(dev).clone(), S_b=torch.zeros(N, dtype=torch.float64, device=dev),
                                          acc_b=torch.zeros(N, dtype=torch.float64, device=dev)))
    return out


def gate_b(r, prior_b, J_b):
    """E of a `colsums` (or `problem`) result with summed joins J_b."""
    return r["acc_b"] + float(J_b) * U32 * (prior_b.double().to(r["S_b"].device).abs() + r["S_b"])


def gate(r, prior_w, prior_b, J_w, J_b):
    """(E_w, E_b) of a `problem` result r with summed joins J_w / J_b (E_b None without a bias)."""
    E_w = r["acc_w"] + float(J_w) * U32 * (prior_w.double().to(r["S"].device).abs() + r["S"])
    E_b = None
    if r["ref_b"] is not None:
        E_b = gate_b(r, prior_b, J_b)
    return E_w, E_b
