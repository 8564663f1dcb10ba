"""The cross-stream ordering checker (tests/stream_order.py) on synthetic traces, one defect each, and the launch-access table
(tests/launch_access.py) against unimm_amd/lib.py and the header.  No GPU."""
import inspect
import os

from tests import header_reader as H
from tests import launch_access as LA
from tests import stream_order as SO
from tests.stream_order import HOST, alloc, check, free, launch, record, record_stream, sync, wait, wait_stream

S, X, Y = "S", "X", "Y"
BUF = (0x1000, 0x2000)
HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "unimm_hip.h")).read()


def w(name, tl, kind="W", rng=BUF, site=()):
    return launch(tl, name, [(rng[0], rng[1], kind)], site=site or (f"{name}:synthetic.py:1",))


def names(trace, v):
    return {trace[v.first].b, trace[v.second].b}


def test_event_edge_orders_two_streams():
    trace = [w("produce", S), record("e", S), wait(X, "e"), w("consume", X, "R")]
    assert check(trace) == []


def test_missing_edge_is_reported_with_both_launches():
    trace = [w("produce", S), w("consume", X, "R")]
    (v,) = check(trace)
    assert v.kind == "conflict" and names(trace, v) == {"produce", "consume"} and (v.lo, v.hi) == BUF
    text = SO.analyse(trace).describe(v)
    for part in ("produce", "consume", "'S'", "'X'", "0x1000", "0x2000", "synthetic.py:1"):
        assert part in text, text


def test_wait_before_its_record_orders_nothing():
    trace = [wait(X, "e"), w("produce", S), record("e", S), w("consume", X, "R")]
    (v,) = check(trace)
    assert names(trace, v) == {"produce", "consume"}


def test_event_recorded_twice_keeps_the_later_snapshot():
    trace = [w("first", S, rng=(0, 16)), record("e", S), w("second", S, rng=(32, 48)), record("e", S), wait(X, "e"),
             w("reads_second", X, "R", rng=(32, 48))]
    assert check(trace) == []
    # ... and a wait between the two records saw the earlier one only
    trace = [w("first", S, rng=(0, 16)), record("e", S), wait(X, "e"), w("second", S, rng=(32, 48)), record("e", S),
             w("reads_second", X, "R", rng=(32, 48)), w("reads_first", X, "R", rng=(0, 16))]
    (v,) = check(trace)
    assert names(trace, v) == {"second", "reads_second"}


def test_access_kinds():
    assert check([w("a", S, "R"), w("b", X, "R")]) == []
    assert check([w("a", S, "A"), w("b", X, "A")]) == []
    for other in ("R", "W"):
        trace = [w("a", S, "A"), w("b", X, other)]
        (v,) = check(trace)
        assert names(trace, v) == {"a", "b"} and v.detail == f"A/{other}"
    assert len(check([w("a", S, "W"), w("b", X, "W")])) == 1


def test_column_slices_of_one_row_strided_buffer():
    # gk: 10 rows of 96 bytes; columns [32, 64) beside [64, 96), then [48, 80) across both
    base, ld = 0x4000, 96
    left = launch(S, "left", [(base + 32, base + 64, "W", 10, ld)], site=("left:s.py:1",))
    right = launch(X, "right", [(base + 64, base + 96, "W", 10, ld)], site=("right:s.py:1",))
    assert check([left, right]) == []
    across = launch(X, "across", [(base + 48, base + 80, "W", 10, ld)], site=("across:s.py:1",))
    trace = [left, across]
    (v,) = check(trace)
    assert names(trace, v) == {"left", "across"} and base + 32 <= v.lo < v.hi <= base + 10 * ld
    # a flat range that falls into the gap between the rows' columns is clean, one that touches a row is not
    assert check([left, launch(X, "gap", [(base + 64, base + 96 + 32, "W")])]) == []
    assert len(check([left, launch(X, "hit", [(base + 64, base + 96 + 33, "W")])])) == 1
    # a slice of other rows of the same columns is clean
    assert check([left, launch(X, "below", [(base + 10 * ld + 32, base + 10 * ld + 64, "W", 4, ld)])]) == []


def test_transitive_order_through_a_third_stream():
    trace = [w("produce", S), record("e1", S), wait(Y, "e1"), launch(Y, "relay", []), record("e2", Y), wait(X, "e2"),
             w("consume", X, "R")]
    assert check(trace) == []
    assert len(check(trace[:1] + trace[3:])) == 1           # without the first hop


def test_host_write_into_a_pinned_slot():
    slot = (0x9000, 0x9100)
    copy = lambda n: launch(S, n, [(slot[0], slot[1], "R"), (0x100000, 0x100100, "W")], site=(f"{n}:s.py:1",))
    fill = lambda n: launch(HOST, n, [(slot[0], slot[1], "W")], site=(f"{n}:s.py:1",))
    trace = [fill("fill0"), copy("copy0"), record("done", S), fill("fill1"), copy("copy1")]
    (v,) = check(trace)
    assert names(trace, v) == {"copy0", "fill1"}
    trace = [fill("fill0"), copy("copy0"), record("done", S), sync("done", "event"), fill("fill1"), copy("copy1")]
    assert check(trace) == []


def test_allocator_lifetime_rule():
    blk = (0x20000, 0x20400)
    use = launch(X, "reader", [(blk[0], blk[1], "R")], site=("reader:s.py:1",))
    head = [alloc("st", blk[0], blk[1], S), w("fill", S, rng=blk)] + wait_stream(X, S)
    # named in a record_stream: clean
    assert check(head + [use, record_stream("st", X), free("st")]) == []
    # neither named nor ordered before S at the free: violation 2, reported at the free
    trace = head + [use, free("st")]
    (v,) = check(trace)
    assert v.kind == "lifetime" and trace[v.first].b == "reader" and trace[v.second].op == "free"
    assert "reader" in SO.analyse(trace).describe(v) and "free" in SO.analyse(trace).describe(v)
    # S waited for X before the free: clean
    assert check(head + [use] + wait_stream(S, X) + [free("st")]) == []
    # the address handed out again after a discharged free: the new owner does not conflict with the old accesses
    again = [alloc("st2", blk[0], blk[1], S), w("refill", S, rng=blk)]
    assert check(head + [use, record_stream("st", X), free("st")] + again) == []
    # ... while without the free the same write is an unordered conflict with the reader
    trace = head + [use, w("refill", S, rng=blk)]
    (v,) = check(trace)
    assert v.kind == "conflict" and names(trace, v) == {"reader", "refill"}


def test_dropping_records_edits_the_trace_only():
    trace = [w("produce", S, site=("p:s.py:1",))] + wait_stream(X, S, site=("_to_img:engine.py:1", "step:s.py:2")) + [w("consume", X, "R")]
    an = SO.analyse(trace)
    assert an.check() == [] and SO.summary(an) == (2, 2, 1) and SO.removable_edges(an) == 0
    drop = SO.from_site(trace, "_to_img")
    assert len(drop) == 1 and len(an.check(drop)) == 1
    assert SO.from_site(trace, "step") == frozenset()         # the innermost frame names the site


def test_extent_of_views():
    class T:                                                 # the four members of a tensor the table reads
        def __init__(self, ptr, shape, stride, es):
            self.ptr, self.shape, self.st, self.es = ptr, shape, stride, es

        def data_ptr(self):
            return self.ptr

        def stride(self):
            return self.st

        def element_size(self):
            return self.es
    assert LA.extent(T(64, (4, 8), (8, 1), 2), "R") == (64, 64 + 64, "R")
    assert LA.extent(T(64, (4, 8), (24, 1), 2), "W") == (64, 80, "W", 4, 48)
    assert LA.extent(T(64, (2, 3, 8), (72, 24, 1), 2), "W") == (64, 80, "W", 6, 48)
    assert LA.extent(T(64, (0, 8), (8, 1), 2), "R") is None
    assert LA.extent(T(64, (3,), (5,), 4), "R") == (64, 68, "R", 3, 20)
    assert LA.extent(T(64, (4, 1), (1, 1), 4), "A") == (64, 80, "A")


def test_table_covers_every_streamed_wrapper():
    from unimm_amd import lib
    reach = {}
    for name, fn in vars(lib).items():
        if inspect.isfunction(fn) and fn.__module__ == lib.__name__ and not name.startswith("_"):
            syms = LA.symbols_of(fn, lib._STREAMED)
            if syms:
                reach[name] = syms
    assert len(reach) > 60
    missing = sorted(set(reach) - set(LA.TABLE))
    assert not missing, f"wrappers that reach a streamed entry point without an entry in tests/launch_access.py: {missing}"
    stale = sorted(n for n in LA.TABLE if not hasattr(lib, n))
    assert not stale, stale
    for name, entry in LA.TABLE.items():
        sig = inspect.signature(getattr(lib, name)).parameters
        for param, spec in entry.items():
            if param in ("members", "extent"):
                assert set(spec) <= set(sig), (name, param)
            elif param not in ("timeline", LA.NEW, LA.HOST_OUT):
                assert param in sig, f"{name}: the table names a parameter {param!r} the wrapper does not have"
                kind = spec[0]
                assert callable(kind) or kind in ("W", "A"), (name, param)
                if callable(kind) or kind == "A" or param in entry.get("extent", {}):
                    assert spec[2], f"{name}.{param}: an 'A' or a refined extent needs its one-line reason"


def test_flat_prototypes_agree_with_the_header_on_what_is_written():
    from unimm_amd import lib
    params = H.pointer_params(HEADER)
    checked = 0
    for name, entry in LA.TABLE.items():
        syms = LA.symbols_of(getattr(lib, name), set(lib.SIGNATURES))
        flat = [s for s in syms if params[s] and all(st is None for _, _, _, _, st in params[s])]
        if len(flat) != len(syms):
            continue                                          # an argument struct: checked call by call on the GPU
        for s in flat:
            written = {p for _, p, _, const, _ in params[s] if not const and p != "stream"}
            assert written == LA.declared_abi_names(entry), (name, s, sorted(written), sorted(LA.declared_abi_names(entry)))
            checked += 1
    assert checked >= 45, checked
