"""The gradient-exchange plan of one backward pass, as host arithmetic.

Under data parallelism (`parallel.DataParallelRCCL`, the replacement of utils/data_parallel.py:91-132) the engine hands a
gradient bucket to the wrapper once every weight-gradient launch that covers it has been enqueued, and the engine launches
weight gradients GROUPED over several encoder blocks.  Which buckets travel together, in how many collectives and of what
size is therefore a function of the config, the step's row counts and `wgrad_group_rounds` alone.  That rule is written ONCE,
in `Ledger`, and has two drivers: `Engine` (`_wgrad`, `_bucket_done`), which launches what the ledger names and hands over
what it says, and `hand_overs`, which feeds it the backward pass as a list of events, without a device.  `tests/test_bucket_plan_cpu.py`
checks both on the CPU; `tests/test_gpu_dp2.py` holds the plan against the hand-overs and launches of a real backward.

Covers the default encoder options (every layer trained, connection layers on: what bert_base_6layer_6conect.json and every script of
the reference use); under `fixed_t_layer` / `with_coattention=False` the engine reports the buckets of skipped blocks at the end of backward.

Nothing here touches torch."""
from __future__ import annotations

from typing import List, Tuple

from . import params as PM

ARENA_ALIGN = 64          # elements (arena.ALIGN)
CHIP_SLOTS = 256          # 256x256 weight-gradient tiles resident at once (one per CU)


def big_tiles_of(M: int, N: int, K: int) -> int:
    """256x256 output tiles of one weight gradient dW[N, K] = dY[M, N]^T X[M, K] when it takes the big tile
    (csrc/gemm.hip: tn_is_big), else 0."""
    if N >= 256 and K >= 256 and M >= 1024:
        return ((N + 255) // 256) * ((K + 255) // 256)
    return 0


def flush_due(n_problems: int, tiles: int, rounds: int) -> bool:
    """Is a queue of `n_problems` weight gradients with `tiles` big tiles due for its grouped launch?  Due = the tile count
    sits just below a multiple of 256 (<= 12.5 % of the last round idle) and covers at least half of `rounds`, or exceeds
    `rounds` rounds of the chip, or the launch's descriptor table (48 problems) is nearly full."""
    if n_problems >= 40:
        return True
    if tiles >= rounds * CHIP_SLOTS:
        return True
    waste = (-tiles) % CHIP_SLOTS
    return tiles >= max(2, rounds // 2) * CHIP_SLOTS - 32 and waste <= CHIP_SLOTS // 8


class Ledger:
    """The books of a backward pass's weight-gradient queues, per side (0 = text queue, 1 = image queue).  Host arithmetic
    only: the driver keeps the operands and does the launches."""

    def __init__(self, log=None):
        self.queued, self.launched = [0, 0], [0, 0]   # weight-gradient problems ever queued / ever launched
        self.tiles = [0, 0]           # big tiles of the problems now queued
        self.sums = [False, False]    # a column-sum reduction waits for the side's next launch
        self.pending = []             # buckets whose weight gradients are still queued: (group, queued[0], queued[1]) at their mark
        self.reported = set()         # groups marked in this pass
        self.log = log                # list, or None: (side, n_problems, big_tiles) of every launch with problems

    def begin(self):
        self.reported = set()

    def queue(self, side, M, N, K):
        self.queued[side] += 1
        self.tiles[side] += big_tiles_of(M, N, K)

    def colsum(self, side):
        self.sums[side] = True

    def _take(self, side, force, rounds):
        n = self.queued[side] - self.launched[side]
        if not (n or self.sums[side]) or not (force or flush_due(n, self.tiles[side], rounds)):
            return False
        if n and self.log is not None:
            self.log.append((side, n, self.tiles[side]))
        self.launched[side], self.tiles[side], self.sums[side] = self.queued[side], 0, False
        return True

    def flush(self, rounds, on_side=False, force=True, force_img=False):
        """-> the sides to launch now, in launch order: the image side first, the text side only from the text side.  A side
        goes out when it is due (`flush_due`) or forced; the defaults flush everything, for callers outside a backward."""
        sides = [1] if self._take(1, force or force_img, rounds) else []
        return (sides + [0]) if not on_side and self._take(0, force, rounds) else sides

    def mark(self, group, rounds, on_side=False, force=False, force_img=False, hand_over=True):
        """`group`'s backward is enqueued -> (sides to launch now, [(group, more), ...] buckets to hand over after them):
        whatever is complete, oldest first, and only from the text side -- a bucket whose launches are out is not held back by
        an older one that waits for the other side's queue.  hand_over=False (nobody takes buckets): nothing is kept pending."""
        self.reported.add(group)
        if hand_over:
            self.pending.append((group, self.queued[0], self.queued[1]))
        sides = self.flush(rounds, on_side, force, force_img)
        ready = [] if on_side else [p for p in self.pending if self.launched[0] >= p[1] and self.launched[1] >= p[2]]
        self.pending = [p for p in self.pending if p not in ready]
        return sides, [(g, j + 1 < len(ready)) for j, (g, _, _) in enumerate(ready)]


def arena_ranges(cfg) -> List[Tuple[str, int, int]]:
    """(group, lo, hi) element ranges of the flat arena (arena.FlatArena.buckets) without building one."""
    out, off = [], 0
    for gname, items in PM.arena_groups(cfg):
        lo = off
        for _, shape in items:
            n = 1
            for s in shape:
                n *= s
            off += (n + ARENA_ALIGN - 1) // ARENA_ALIGN * ARENA_ALIGN
        out.append((gname, lo, off))
    return out


def _self_block(h, inter):
    return [(h, inter), (inter, h), (h, h), (3 * h, h)]          # backward order: ff2, ff1, attention output, fused QKV


def backward_events(cfg, n_seq: int, text_rows: int, lm_rows: int, regions: int = 37, dual_stream: bool = True,
                    image_head_side: bool = True):
    """The backward pass as the engine enqueues it (Engine._backward): a list of
    ("w", side, M, N, K) weight gradients queued (side 0 = text queue, 1 = image queue) and
    ("b", group, on_side, force, force_img) bucket-done marks, in order.  `dual_stream` does not change the plan: on one stream the
    image side keeps its own queue (Engine._img), so the same launches and hand-overs happen, one after the other."""
    del dual_stream
    H, Hv, Hb = cfg.hidden_size, cfg.v_hidden_size, cfg.bi_hidden_size
    I, Iv = cfg.intermediate_size, cfg.v_intermediate_size
    Mt, Mi = text_rows, n_seq * regions
    img = 1            # the image side keeps its own queue on one stream as on two (Engine._img)
    ev = []
    hs = img if image_head_side else 0
    ev.append(("w", hs, Mi, cfg.v_target_size, Hv))              # image head decoder, transform
    ev.append(("w", hs, Mi, Hv, Hv))
    if lm_rows > 0:
        ev.append(("w", 0, lm_rows, cfg.vocab_size, H))          # tied decoder, MLM transform
        ev.append(("w", 0, lm_rows, H, H))
    ev.append(("b", "heads", False, True, False))
    sched = PM.encoder_schedule(cfg)
    entries = list(reversed(sched))
    pos = 0
    tail_done = False

    def image_tail():          # Engine._backward_encoder: the image embedding as soon as no image / connection layer is left
        nonlocal tail_done
        if tail_done or any(k in ("c", "v") for k, _ in entries[pos:]):
            return
        tail_done = True
        ev.extend([("w", img, Mi, Hv, cfg.v_feature_size), ("w", img, Mi, Hv, 5)])
        ev.append(("b", "image_embeddings", bool(img), False, True))

    while pos < len(entries):
        image_tail()
        seg = []
        while pos < len(entries) and entries[pos][0] != "c":
            seg.append(entries[pos])
            pos += 1
        for kind, i in seg:
            if kind == "v":
                ev += [("w", img, Mi, n, k) for n, k in _self_block(Hv, Iv)]
                ev.append(("b", f"v{i}", bool(img), False, False))
        for kind, i in seg:
            if kind == "t":
                ev += [("w", 0, Mt, n, k) for n, k in _self_block(H, I)]
                ev.append(("b", f"t{i}", False, False, False))
        if pos < len(entries):
            _, i = entries[pos]
            pos += 1
            ev += [("w", img, Mi, Hv, Iv), ("w", img, Mi, Iv, Hv), ("w", img, Mi, Hv, Hb)]
            ev += [("w", 0, Mt, H, I), ("w", 0, Mt, I, H), ("w", 0, Mt, H, Hb)]
            ev += [("w", img, Mi, 3 * Hb, Hv), ("w", 0, Mt, 3 * Hb, H)]
            ev.append(("b", f"c{i}", False, False, False))
    image_tail()
    ev.append(("b", "text_embeddings", False, True, False))
    return ev


def hand_overs(cfg, n_seq, text_rows, lm_rows, regions=37, wgrad_group_rounds=2, dual_stream=True, image_head_side=True):
    """-> ([(group, more), ...] in the order `Engine._bucket_done` calls the data-parallel hook,
           [number of weight-gradient problems per grouped launch, per queue: (side, n_problems, big_tiles), ...])."""
    led, calls = Ledger(log=[]), []
    for e in backward_events(cfg, n_seq, text_rows, lm_rows, regions, dual_stream, image_head_side):
        if e[0] == "w":
            led.queue(*e[1:])
        else:
            calls += led.mark(e[1], wgrad_group_rounds, *e[2:])[1]      # ("b", group, on_side, force, force_img)
    assert not led.pending, led.pending
    return calls, led.log


def collectives(cfg, calls):
    """The (lo, hi, n_buckets) element ranges `DataParallelRCCL._on_bucket` exchanges for that sequence of hook calls:
    adjacent slices handed over in one run travel as ONE collective."""
    ranges = {g: (lo, hi) for g, lo, hi in arena_ranges(cfg)}
    out, run = [], None
    for group, more in calls:
        lo, hi = ranges[group]
        if run and (run[0] == hi or run[1] == lo):
            run = [min(lo, run[0]), max(hi, run[1]), run[2] + 1]
        else:
            if run:
                out.append(tuple(run))
            run = [lo, hi, 1]
        if not more:
            out.append(tuple(run))
            run = None
    assert run is None
    return out


def exchange_plan(cfg, n_seq, text_rows, lm_rows, **kw):
    """-> dict(collectives=[(lo, hi, n_buckets)], bytes=[fp32 bytes per collective], launches=[...], calls=[...])."""
    calls, launches = hand_overs(cfg, n_seq, text_rows, lm_rows, **kw)
    cs = collectives(cfg, calls)
    return dict(calls=calls, launches=launches, collectives=cs, bytes=[(hi - lo) * 4 for lo, hi, _ in cs])
