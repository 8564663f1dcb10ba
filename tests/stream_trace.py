"""Launch tracer for tests/test_gpu_stream_order.py: for the duration of a `with Tracer(monkeypatch) as tr:` block it records, in
host program order, what is enqueued on which stream, which bytes each launch reads and writes, and which event edges exist
-- the input of tests/stream_order.py.  Everything it changes is set through pytest's monkeypatch and undone by it.

  wrappers      every wrapper of unimm_amd.lib with an entry in tests/launch_access.py is replaced by one that makes the call and
                records the launch on `lib._stream()`'s stream with the table's accesses
  torch ops     a TorchDispatchMode records torch's own ops as launches on torch.cuda.current_stream(): writes are the schema's
                `alias_info.is_write` arguments and the outputs that do not alias an input; view ops are no launches; ops on CPU
                tensors count (on the host timeline) only when a tensor is pinned; new device storages give `alloc` on the current
                stream and a weakref.finalize on the storage gives `free` (it fires when the last tensor of the storage dies);
                storages that existed before the block are never freed for the checker
  streams       Stream.wait_stream / wait_event / synchronize, Event.record / wait / synchronize, torch.cuda.synchronize and
                Tensor.record_stream are patched on their classes to record the edges
  ABI           `lib._lib` is replaced by a proxy that sees the raw pointer arguments of every C call, the pointer fields of
                argument structs and of struct arrays up to their count included; with the const-ness the header gives each of
                them (tests/header_reader.py), every non-const pointer other than the stream must lie inside a range the table
                declared 'W' or 'A' for that call (`abi_errors`)
  threads       a lib launch on a thread where the dispatch mode is not active is an error (`thread_errors`): torch ops there
                would be missing.  The engine's entries (`_on_text_stream`) push the mode on a thread that lacks it, which is
                what covers the engine's backward when autograd runs it on its own thread."""
import ctypes as C
import inspect
import os
import sys
import threading
import weakref

import torch
from torch.utils._python_dispatch import TorchDispatchMode

from tests import header_reader as H
from tests import launch_access as LA
from tests import stream_order as SO

_HERE = os.path.abspath(__file__)
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_HEADER = os.path.join(_ROOT, "include", "unimm_hip.h")
_DEVICE_STRUCTS = {"unimm_clip_state", "unimm_transpose_desc"}            # structs that live in device memory: plain pointers here
_ARRAYS = {"unimm_gemm_tn_grouped": 1, "unimm_gemm_tn_grouped_ws": 1, "unimm_colpartials_finish_grouped": 1}   # index of the count
_EMPTY = ("empty", "empty_like", "empty_strided", "new_empty", "new_empty_strided", "empty_permuted")


def _site(depth=4):
    """Innermost-first 'function:file:line' of the project frames under the caller (this module's own frames left out)."""
    out, f = [], sys._getframe(1)
    while f is not None and len(out) < depth:
        fn = f.f_code.co_filename
        if fn != _HERE and fn.startswith(_ROOT):
            out.append(f"{f.f_code.co_name}:{os.path.basename(fn)}:{f.f_lineno}")
        f = f.f_back
    return tuple(out)


def _handle(stream):
    return int(stream.cuda_stream)


def _addr(v):
    if v is None:
        return None
    if isinstance(v, int):
        return v
    if isinstance(v, C.c_void_p):
        return v.value
    obj = getattr(v, "_obj", None)                    # byref(x)
    if obj is not None:
        return C.addressof(obj)
    return None


class _Frame:
    __slots__ = ("created", "abi")

    def __init__(self):
        self.created, self.abi = [], []


class _Mode(TorchDispatchMode):
    def __init__(self, tracer):
        super().__init__()
        self.tracer = tracer

    def __enter__(self):
        self.tracer._mode_threads[threading.get_ident()] = self.tracer._mode_threads.get(threading.get_ident(), 0) + 1
        return super().__enter__()

    def __exit__(self, *exc):
        self.tracer._mode_threads[threading.get_ident()] -= 1
        return super().__exit__(*exc)

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        out = func(*args, **kwargs)
        self.tracer._on_op(func, args, kwargs, out)
        return out


class _Proxy:
    """Stands in for the loaded library: every function with pointer parameters logs its raw pointers before the call."""

    def __init__(self, real, tracer):
        self.__dict__["_real"], self.__dict__["_tracer"], self.__dict__["_fns"] = real, tracer, {}

    def __getattr__(self, name):
        fn = self._fns.get(name)
        if fn is not None:
            return fn
        real = getattr(self._real, name)
        params = self._tracer.pointer_params.get(name)
        if not params:
            return real
        tracer = self._tracer

        def call(*args):
            ptrs = tracer._nonconst_pointers(name, params, args)
            stack = tracer._frames()
            if stack:
                stack[-1].abi.append((name, ptrs))
            elif ptrs:
                tracer.abi_errors.append(f"{name}: called outside every wrapper of the table, with non-const pointers "
                                         f"{[p for p, _ in ptrs]} [{' < '.join(_site())}]")
            return real(*args)
        self._fns[name] = call
        return call


class Tracer:
    def __init__(self, monkeypatch):
        self._outer = monkeypatch            # the block's patches live in a context of their own and end with it
        self.trace, self.abi_errors, self.thread_errors = [], [], []
        self.active = False
        self._live = {}                      # data_ptr of a storage allocated inside the block -> storage id
        self._next_storage = 0
        self._events = []                    # every event seen stays alive: an id is never reused inside one trace
        self._tls = threading.local()
        self._mode_threads = {}
        self._nested = threading.local()
        text = open(_HEADER).read()
        self.pointer_params = H.pointer_params(text)
        self.struct_pointers = H.struct_pointers(text)
        self.threads = set()

    # ---- bookkeeping ---------------------------------------------------------------------------------------------------
    def _frames(self):
        st = getattr(self._tls, "frames", None)
        if st is None:
            st = self._tls.frames = []
        return st

    def _event(self, ev):
        self._events.append(ev)
        return ("event", id(ev))

    def _quiet(self):
        return getattr(self._nested, "n", 0) > 0

    def _storage_of(self, t):
        try:
            return self._live.get(t.untyped_storage().data_ptr())
        except Exception:
            return None

    def _freed(self, ptr, sid):
        if self._live.get(ptr) == sid:
            del self._live[ptr]
        if self.active:
            self.trace.append(SO.free(sid, _site()))

    # ---- torch ops -----------------------------------------------------------------------------------------------------
    def _on_op(self, func, args, kwargs, out):
        if not self.active:
            return
        schema = func._schema
        ns, _, op = schema.name.partition("::")
        if op in ("record_stream", "is_pinned"):
            return
        ins = []                              # (tensor, is written)
        sargs = schema.arguments
        for i, a in enumerate(args):
            w = i < len(sargs) and sargs[i].alias_info is not None and sargs[i].alias_info.is_write
            for t in LA.tensors_in(a):
                ins.append((t, w or ns == "c10d"))
        byname = {a.name: a for a in sargs}
        for k, a in kwargs.items():
            w = k in byname and byname[k].alias_info is not None and byname[k].alias_info.is_write
            for t in LA.tensors_in(a):
                ins.append((t, w or ns == "c10d"))
        ins = [(t, w) for t, w in ins if isinstance(t, torch.Tensor) and t.layout == torch.strided and t.device.type in ("cuda", "cpu")]
        outs = [t for t in LA.tensors_in(out) if isinstance(t, torch.Tensor) and t.layout == torch.strided
                and t.device.type in ("cuda", "cpu")] if ns != "c10d" else []
        in_ptrs = {t.untyped_storage().data_ptr() for t, _ in ins}
        new = [t for t in outs if t.untyped_storage().data_ptr() not in in_ptrs]
        on_device = any(t.is_cuda for t, _ in ins) or any(t.is_cuda for t in outs)
        site = None
        stream = _handle(torch.cuda.current_stream()) if on_device else None
        for t in new:
            if not t.is_cuda:
                continue
            st = t.untyped_storage()
            ptr = st.data_ptr()
            if ptr in self._live or st.nbytes() == 0:
                continue
            site = site or _site()
            sid = self._next_storage = self._next_storage + 1
            self._live[ptr] = sid
            self.trace.append(SO.alloc(sid, ptr, ptr + st.nbytes(), stream, site))
            weakref.finalize(st, self._freed, ptr, sid)
            frames = self._frames()
            if frames:
                frames[-1].created.append(t)
        if op in _EMPTY or (not new and not any(w for _, w in ins)):
            return                            # an allocation alone, or a view: no launch
        if not on_device:
            if not any(t.is_pinned() for t, _ in ins) and not any(t.is_pinned() for t in outs):
                return                        # pageable host memory only: nothing a stream ever sees
            timeline = SO.HOST
        else:
            timeline = stream
        acc = []
        for t, w in ins:
            if t.is_cuda or on_device or t.is_pinned():
                e = LA.extent(t, "W" if w else "R")
                if e is not None:
                    acc.append(e)
        for t in new:
            e = LA.extent(t, "W")
            if e is not None:
                acc.append(e)
        self.threads.add(threading.get_ident())
        self.trace.append(SO.launch(timeline, schema.name, acc, site or _site(), threading.get_ident()))

    # ---- lib wrappers --------------------------------------------------------------------------------------------------
    def _wrap(self, lib, name):
        orig = getattr(lib, name)
        sig = inspect.signature(orig)
        entry = LA.TABLE[name]
        host_names = set(entry[LA.HOST_OUT][1].split()) if LA.HOST_OUT in entry else set()
        tracer = self

        def wrapped(*args, **kw):
            if not tracer.active:
                return orig(*args, **kw)
            bound = sig.bind(*args, **kw)
            bound.apply_defaults()
            frames = tracer._frames()
            fr = _Frame()
            frames.append(fr)
            try:
                ret = orig(*args, **kw)
            finally:
                frames.pop()
            acc = LA.accesses(name, bound.arguments, fr.created)
            if entry.get("timeline") == LA.HOST_TIMELINE:
                timeline = SO.HOST
            else:
                timeline = int(lib._stream().value or 0)
            site = _site()
            ident = threading.get_ident()
            tracer.threads.add(ident)
            tracer.trace.append(SO.launch(timeline, name, acc, site, ident))
            if tracer._mode_threads.get(ident, 0) <= 0:
                tracer.thread_errors.append(f"{name} launched on thread {ident} where the dispatch mode is not active [{' < '.join(site)}]")
            writes = [SO._norm(a) for a in acc if a[2] in ("W", "A")]
            for sym, ptrs in fr.abi:
                for pname, addr in ptrs:
                    if pname in host_names:
                        continue
                    if not any(w[0] <= addr < w[5] for w in writes):
                        tracer.abi_errors.append(f"{name} -> {sym}: non-const pointer {pname} = {addr:#x} lies in no range the table "
                                                 f"declares written [{' < '.join(site)}]")
            return ret
        wrapped.__name__ = name
        return wrapped

    def _nonconst_pointers(self, sym, params, args):
        """[(name, address)] of the non-const pointers of one C call, struct fields included."""
        from unimm_amd import lib
        out = []
        for i, pname, ctext, is_const, struct in params:
            if pname == "stream" or i >= len(args):
                continue
            val = args[i]
            if struct is None or struct in _DEVICE_STRUCTS:
                if not is_const:
                    a = _addr(val)
                    if a:
                        out.append((pname, a))
                continue
            cls = lib.STRUCTS.get(struct)
            a = _addr(val)
            if cls is None or not a:
                continue
            n = int(args[_ARRAYS[sym]]) if sym in _ARRAYS else 1
            objs = (cls * n).from_address(a)
            for obj in objs:
                for field, fconst, length in self.struct_pointers[struct]:
                    if fconst:
                        continue
                    v = getattr(obj, field)
                    for x in (v if length else (v,)):
                        if x:
                            out.append((f"{struct}.{field}", int(x)))
        return out

    # ---- the block -----------------------------------------------------------------------------------------------------
    def __enter__(self):
        from unimm_amd import engine as E
        from unimm_amd import lib
        self._ctx = self._outer.context()
        mp = self.mp = self._ctx.__enter__()
        tr = self
        lib.lib()                                           # loaded before the proxy takes its place
        mp.setattr(lib, "_lib", _Proxy(lib._lib, self))
        mp.setattr(lib, "_tls", threading.local())          # the hot wrappers' cached functions would bypass the proxy
        for name in LA.TABLE:
            mp.setattr(lib, name, self._wrap(lib, name))
        table = lib.transpose_table

        def transpose_table(entries, device):
            res = table(entries, device)
            LA.note_transpose_table(entries, res)
            return res
        mp.setattr(lib, "transpose_table", transpose_table)

        S, Ev = torch.cuda.Stream, torch.cuda.Event
        o_ws, o_we, o_ss = S.wait_stream, S.wait_event, S.synchronize
        o_er, o_ew, o_es = Ev.record, Ev.wait, Ev.synchronize
        o_sync, o_rs = torch.cuda.synchronize, torch.Tensor.record_stream

        def quiet(fn, *a, **k):
            tr._nested.n = getattr(tr._nested, "n", 0) + 1
            try:
                return fn(*a, **k)
            finally:
                tr._nested.n -= 1

        def wait_stream(self, stream):
            if tr.active and not tr._quiet():
                tr.trace.extend(SO.wait_stream(_handle(self), _handle(stream), _site()))
            return quiet(o_ws, self, stream)

        def wait_event(self, event):
            if tr.active and not tr._quiet():
                tr.trace.append(SO.wait(_handle(self), tr._event(event), _site()))
            return quiet(o_we, self, event)

        def stream_synchronize(self):
            r = quiet(o_ss, self)
            if tr.active and not tr._quiet():
                tr.trace.append(SO.sync(_handle(self), "stream", _site()))
            return r

        def event_record(self, stream=None):
            if stream is None:
                stream = torch.cuda.current_stream()
            if tr.active and not tr._quiet():
                tr.trace.append(SO.record(tr._event(self), _handle(stream), _site()))
            return quiet(o_er, self, stream)

        def event_wait(self, stream=None):
            if stream is None:
                stream = torch.cuda.current_stream()
            if tr.active and not tr._quiet():
                tr.trace.append(SO.wait(_handle(stream), tr._event(self), _site()))
            return quiet(o_ew, self, stream)

        def event_synchronize(self):
            r = quiet(o_es, self)
            if tr.active and not tr._quiet():
                tr.trace.append(SO.sync(tr._event(self), "event", _site()))
            return r

        def synchronize(device=None):
            r = o_sync(device)
            if tr.active:
                tr.trace.append(SO.sync(None, SO.ALL, _site()))
            return r

        def record_stream(self, stream):
            if tr.active:
                sid = tr._storage_of(self)
                if sid is not None:
                    tr.trace.append(SO.record_stream(sid, _handle(stream), _site()))
            return o_rs(self, stream)

        mp.setattr(S, "wait_stream", wait_stream)
        mp.setattr(S, "wait_event", wait_event)
        mp.setattr(S, "synchronize", stream_synchronize)
        mp.setattr(Ev, "record", event_record)
        mp.setattr(Ev, "wait", event_wait)
        mp.setattr(Ev, "synchronize", event_synchronize)
        mp.setattr(torch.cuda, "synchronize", synchronize)
        mp.setattr(torch.Tensor, "record_stream", record_stream)

        entry = E.Engine._on_text_stream

        def _on_text_stream(self, fn, *args):
            if tr.active and tr._mode_threads.get(threading.get_ident(), 0) <= 0:
                with _Mode(tr):
                    return entry(self, fn, *args)
            return entry(self, fn, *args)
        mp.setattr(E.Engine, "_on_text_stream", _on_text_stream)

        self._mode = _Mode(self)
        self._mode.__enter__()
        self.active = True
        return self

    def __exit__(self, *exc):
        self.active = False
        self._mode.__exit__(*exc)
        self._ctx.__exit__(None, None, None)
        return False

    # ---- results -------------------------------------------------------------------------------------------------------
    def timelines(self):
        return {r.a for r in self.trace if r.op == "launch"}
