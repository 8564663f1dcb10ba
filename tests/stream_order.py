"""Cross-stream ordering checker: a launch trace in host program order -> the pairs of launches that touch the same bytes from
different timelines with nothing that orders them, and the storages freed while another stream may still use them.

Pure Python, no torch: tests/test_stream_order_cpu.py feeds it synthetic traces, tests/stream_trace.py the record of a real step.

A trace is a list of `Rec`; the constructors below build them:

    launch(timeline, name, accesses)      accesses: (lo, hi, kind) byte ranges, or (lo, hi, kind, rows, stride) = `rows` rows of
                                          hi - lo bytes, `stride` bytes apart, the first at lo; kind 'R' read, 'W' write,
                                          'A' atomic accumulate ('A' beside 'A' is no conflict; 'A' conflicts with 'R' and 'W')
    record(event, stream)                 the event snapshots the stream's clock (a later record replaces the snapshot)
    wait(stream, event)                   the stream joins the event's snapshot (a wait before the first record joins nothing)
    wait_stream(stream, other)            = record + wait on a private event (two records)
    sync(target, what)                    the host joins a stream's clock, an event's snapshot, or (what = ALL) every stream's
    alloc(storage, lo, hi, stream)        the caching allocator hands out [lo, hi) on `stream`
    record_stream(storage, stream)        ... is told that `stream` uses the block
    free(storage)                         the last tensor of the storage died

Timelines are HOST and the streams (any hashable).  Happens-before is kept in vector clocks: a timeline's launches are ordered
among themselves, every launch and every event record follows the host position that enqueued it, a wait joins the snapshot of
the event, a synchronize joins into HOST.  Host syncs the tracer did not recognise are simply absent: that can only add reports.

Violation 1 (`kind == "conflict"`): two accesses on different timelines, overlapping bytes, not both 'R' and not both 'A',
neither ordered before the other.
Violation 2 (`kind == "lifetime"`): at free(storage) of a block allocated on stream S, an earlier access to it on a stream X != S
that was neither named in a record_stream for the storage nor ordered before S's position at the free -- the allocator may
hand the block to the next allocation on S while X still uses it.  Reported at the free whether or not the address was reused.
After the free the block's earlier accesses no longer take part in violation 1: later users of the bytes own a new allocation.

`analyse(trace)` finds the candidate pairs once (they do not depend on the edges); `Analysis.check(drop)` then evaluates the
ordering, optionally with some records (waits, record_streams) left out: the negative controls and the per-edge count edit the
trace this way, never the run."""
from collections import namedtuple

HOST = "host"
ALL = "all"

Rec = namedtuple("Rec", "op a b c site thread")           # op-specific fields a, b, c; site: short stack summary (tuple of str)


def launch(timeline, name, accesses, site=(), thread=None):
    return Rec("launch", timeline, name, tuple(tuple(x) for x in accesses), tuple(site), thread)


def record(event, stream, site=()):
    return Rec("record", event, stream, None, tuple(site), None)


def wait(stream, event, site=()):
    return Rec("wait", stream, event, None, tuple(site), None)


_private = [0]


def wait_stream(stream, other, site=()):
    """`stream.wait_stream(other)`: a record on `other` and a wait on `stream`, through an event of their own."""
    _private[0] += 1
    ev = ("wait_stream", _private[0])
    return [record(ev, other, site), wait(stream, ev, site)]


def sync(target, what="stream", site=()):
    """The host waits for `target`: what = "stream", "event", or "all" (target ignored)."""
    return Rec("sync", target, what, None, tuple(site), None)


def alloc(storage, lo, hi, stream, site=()):
    return Rec("alloc", storage, (lo, hi), stream, tuple(site), None)


def record_stream(storage, stream, site=()):
    return Rec("record_stream", storage, stream, None, tuple(site), None)


def free(storage, site=()):
    return Rec("free", storage, None, None, tuple(site), None)


Violation = namedtuple("Violation", "kind first second lo hi detail")    # first / second: indices of trace records


def _norm(acc):
    """(lo, width, kind, rows, stride, end): end = one past the last byte of the last row"""
    if len(acc) == 3:
        lo, hi, kind = acc
        return lo, hi - lo, kind, 1, 0, hi
    lo, hi, kind, rows, stride = acc
    if rows <= 1 or stride <= hi - lo:                    # rows touch or overlap: one flat range
        return lo, (hi - lo) + max(rows - 1, 0) * stride, kind, 1, 0, hi + max(rows - 1, 0) * stride
    return lo, hi - lo, kind, rows, stride, lo + (rows - 1) * stride + (hi - lo)


def _flat_hits_rows(flo, fhi, lo, width, rows, stride):
    """Does [flo, fhi) meet one of the rows [lo + r stride, lo + r stride + width)?  -> the first such row's overlap or None"""
    # rows r with lo + r stride < fhi and lo + r stride + width > flo
    r0 = max(0, -((lo + width - flo - 1) // stride))      # smallest r with lo + r stride + width > flo
    if r0 >= rows:
        return None
    start = lo + r0 * stride
    if start >= fhi:
        return None
    return max(start, flo), min(start + width, fhi)


def overlap(a, b):
    """The first overlapping byte range of two normalised accesses, or None.  Rows of one stride are compared column-wise
    (disjoint column slices of one buffer do not alias); rows of different strides fall back to their bounding ranges."""
    alo, aw, _, ar, ast, aend = a
    blo, bw, _, br, bst, bend = b
    if aend <= blo or bend <= alo:
        return None
    if ar == 1 and br == 1:
        return max(alo, blo), min(aend, bend)
    if ar == 1:
        return _flat_hits_rows(alo, aend, blo, bw, br, bst)
    if br == 1:
        return _flat_hits_rows(blo, bend, alo, aw, ar, ast)
    if ast != bst:
        return max(alo, blo), min(aend, bend)
    d = (blo - alo) % ast                                  # column offset of b's rows inside a's row period
    if d < aw or d + bw > ast:                             # b starts inside a's columns, or wraps round into them
        # the bounding ranges overlap and the columns meet: name the first row of the later one
        lo = max(alo, blo)
        return lo, min(lo + min(aw, bw), min(aend, bend))
    return None


def _conflicts(ka, kb):
    return not ((ka == "R" and kb == "R") or (ka == "A" and kb == "A"))


_PAGE = 1 << 16
_BIG = 64                                                  # an access over more pages than this sits in the linear list


class _Index:
    """Live accesses by 64 KiB page; accesses over many pages (whole arenas) in one short list."""

    def __init__(self):
        self.pages, self.big = {}, []

    def add(self, item):
        lo, end = item[0][0], item[0][5]
        p0, p1 = lo // _PAGE, (end - 1) // _PAGE
        if p1 - p0 >= _BIG:
            self.big.append(item)
            return
        for p in range(p0, p1 + 1):
            self.pages.setdefault(p, []).append(item)

    def near(self, acc):
        lo, end = acc[0], acc[5]
        p0, p1 = lo // _PAGE, (end - 1) // _PAGE
        seen = set()
        for item in self.big:
            yield item
        if p1 - p0 >= _BIG:
            for p, items in self.pages.items():
                if p0 <= p <= p1:
                    for item in items:
                        if id(item) not in seen:
                            seen.add(id(item))
                            yield item
            return
        for p in range(p0, p1 + 1):
            for item in self.pages.get(p, ()):
                if p0 == p1 or id(item) not in seen:
                    seen.add(id(item))
                    yield item

    def retire(self, lo, hi):
        """Drop every access that lies inside [lo, hi): the block was freed."""
        inside = lambda it: lo <= it[0][0] and it[0][5] <= hi
        self.big = [it for it in self.big if not inside(it)]
        for p in range(lo // _PAGE, (hi - 1) // _PAGE + 1):
            items = self.pages.get(p)
            if items:
                items[:] = [it for it in items if not inside(it)]


class Analysis:
    """The candidate conflicts and lifetime questions of one trace (see `analyse`)."""

    def __init__(self, trace):
        self.trace = trace
        self.pairs = []           # (earlier launch record, later launch record, lo, hi, kind a, kind b)
        self.lifetimes = []       # (free record, launch record, alloc stream, lo, hi, storage, record_stream indices by stream)
        index = _Index()
        live = {}                 # storage -> (lo, hi, stream, [(record index, stream) of record_stream])
        seen_pairs = set()
        for i, r in enumerate(trace):
            if r.op == "launch":
                for acc in r.c:
                    n = _norm(acc)
                    if n[1] <= 0:
                        continue
                    for other, j, tl in index.near(n):
                        if tl == r.a or not _conflicts(other[2], n[2]) or (j, i) in seen_pairs:
                            continue
                        ov = overlap(other, n)
                        if ov is not None:
                            seen_pairs.add((j, i))
                            self.pairs.append((j, i, ov[0], ov[1], other[2], n[2]))
                    index.add((n, i, r.a))
            elif r.op == "alloc":
                live[r.a] = (r.b[0], r.b[1], r.c, [])
            elif r.op == "record_stream":
                if r.a in live:
                    live[r.a][3].append((i, r.b))
            elif r.op == "free":
                blk = live.pop(r.a, None)
                if blk is None:
                    continue
                lo, hi, s, named = blk
                probe = (lo, hi - lo, "W", 1, 0, hi)
                asked = set()
                for other, j, tl in index.near(probe):
                    if tl == s or tl == HOST or j in asked or overlap(other, probe) is None:
                        continue
                    if not (lo <= other[0] and other[5] <= hi):
                        continue
                    asked.add(j)
                    self.lifetimes.append((i, j, s, lo, hi, r.a, tuple(k for k, x in named if x == tl)))
                index.retire(lo, hi)

    def clocks(self, drop=frozenset()):
        """-> {launch record index: (timeline, position, clock dict)} and {free record index: clock of its alloc stream}"""
        trace = self.trace
        pos, clk, snap = {}, {HOST: {}}, {}
        at, free_clk, owner = {}, {}, {}

        def join(dst, src):
            for k, v in src.items():
                if dst.get(k, 0) < v:
                    dst[k] = v

        def stream_clock(s):
            c = clk.get(s)
            if c is None:
                c = clk[s] = {}
            return c

        for i, r in enumerate(trace):
            if i in drop:
                continue
            if r.op == "launch":
                tl = r.a
                pos[tl] = pos.get(tl, 0) + 1
                c = stream_clock(tl)
                if tl != HOST:
                    join(c, clk[HOST])
                c[tl] = pos[tl]
                at[i] = (tl, pos[tl], dict(c))
            elif r.op == "record":
                c = dict(stream_clock(r.b))
                join(c, clk[HOST])
                snap[r.a] = c
            elif r.op == "wait":
                s = snap.get(r.b)
                if s is not None:
                    join(stream_clock(r.a), s)
            elif r.op == "sync":
                if r.b == ALL:
                    for s, c in list(clk.items()):
                        if s != HOST:
                            join(clk[HOST], c)
                elif r.b == "event":
                    if r.a in snap:
                        join(clk[HOST], snap[r.a])
                elif r.a in clk:
                    join(clk[HOST], clk[r.a])
            elif r.op == "alloc":
                owner[r.a] = r.c
            elif r.op == "free":
                s = owner.get(r.a)
                c = dict(stream_clock(s)) if s is not None else {}
                join(c, clk[HOST])
                free_clk[i] = c
        return at, free_clk

    def check(self, drop=frozenset(), limit=None):
        """-> list of Violation with the records in `drop` (indices) left out of the trace."""
        at, free_clk = self.clocks(drop)
        out = []
        for j, i, lo, hi, ka, kb in self.pairs:
            tj, pj, cj = at[j]
            ti, pi, ci = at[i]
            if ci.get(tj, 0) >= pj or cj.get(ti, 0) >= pi:
                continue
            out.append(Violation("conflict", j, i, lo, hi, f"{ka}/{kb}"))
            if limit is not None and len(out) >= limit:
                return out
        for f, j, s, lo, hi, storage, named in self.lifetimes:
            if any(k not in drop for k in named):
                continue
            tj, pj, _ = at[j]
            if free_clk[f].get(tj, 0) >= pj:
                continue
            out.append(Violation("lifetime", j, f, lo, hi, f"storage {storage!r} of stream {s!r} used on {tj!r}"))
            if limit is not None and len(out) >= limit:
                return out
        return out

    def edges(self):
        """Indices of the wait records whose event was last recorded on another stream (the cross-stream edges), plus syncs."""
        last, out = {}, []
        for i, r in enumerate(self.trace):
            if r.op == "record":
                last[r.a] = r.b
            elif r.op == "wait" and last.get(r.b) is not None and last[r.b] != r.a:
                out.append(i)
        return out

    def describe(self, v, stack=3):
        """One report: both records, their timelines, the byte range and the call site of each."""
        def one(k):
            r = self.trace[k]
            where = " < ".join(r.site[:stack]) if r.site else "?"
            if r.op == "launch":
                return f"{r.b} on {r.a!r} [{where}]"
            return f"{r.op}({r.a!r}) [{where}]"
        return f"{v.kind}: {one(v.first)}  ||  {one(v.second)}  bytes [{v.lo:#x}, {v.hi:#x}) {v.detail}"


def analyse(trace):
    return Analysis(list(trace))


def check(trace, limit=None):
    """All violations of a trace."""
    return analyse(trace).check(limit=limit)


def from_site(trace, name, ops=("wait",)):
    """Indices of the records of the given kinds issued from the function `name` (the innermost frame of the stack summary)."""
    return frozenset(i for i, r in enumerate(trace) if r.op in ops and r.site and r.site[0].split(":")[0] == name)


def summary(an):
    """(launches, timelines, cross-stream edges) of an analysed trace"""
    launches = [r for r in an.trace if r.op == "launch"]
    return len(launches), len({r.a for r in launches}), len(an.edges())


def removable_edges(an):
    """How many single cross-stream edges could be deleted without any report (information for whoever tunes the schedule)."""
    return sum(1 for e in an.edges() if not an.check(frozenset([e]), limit=1))
