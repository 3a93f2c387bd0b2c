"""_lib.shared_context without a GPU: one context per (device, W, H, library variant) and host thread, and the cross-stream
ordering of the contexts it hands out.  The context constructor, the event record and the stream wait are replaced by recording
stubs, so what is checked is the bookkeeping: who gets which context, and which stream is made to wait for which event.

include/mdvt.h: "a ctx is not thread-safe" and the scratch-block entry points "must be issued to ONE stream per ctx at a time".
The Python faces hide their context, so the two rules are kept by shared_context (per thread) and SharedContext (per stream)."""
import ctypes as C
import threading

import pytest

from metric_depth_video_toolbox_amd import _lib


class FakeLib:
    """Every entry point returns MDVT_OK and is logged with its arguments."""

    def __init__(self, log):
        self.log = log

    def __getattr__(self, name):
        def entry(*args):
            self.log.append(("call", name))
            return 0
        return entry


@pytest.fixture
def stubs(monkeypatch):
    """Context.__init__, SharedContext._record_event and ._wait_event replaced; -> the log they write.  Entries:
    ("create", thread, ctx id), ("call", name), ("record", stream, event), ("wait", stream, event), ("close", ctx id)."""
    log, lock, made = [], threading.Lock(), [0]

    def init(self, device, width, height):
        self._L, self._h = FakeLib(log), None
        self.device, self.W, self.H = int(device), int(width), int(height)
        with lock:
            log.append(("create", threading.get_ident(), id(self)))

    def record(self, stream):
        with lock:
            made[0] += 1
            event = f"event{made[0]}"
        log.append(("record", stream, event))
        return event

    def wait(self, stream, event):
        log.append(("wait", stream, event))

    def close(self):
        with lock:
            log.append(("close", id(self)))

    monkeypatch.setattr(_lib.Context, "__init__", init)
    monkeypatch.setattr(_lib.Context, "close", close)
    monkeypatch.setattr(_lib.SharedContext, "_record_event", record)
    monkeypatch.setattr(_lib.SharedContext, "_wait_event", wait)
    monkeypatch.setattr(_lib, "_shared", threading.local())          # this test's contexts are its own, in every thread
    return log


def in_thread(fn):
    out = []
    t = threading.Thread(target=lambda: out.append(fn()))
    t.start()
    t.join()
    return out[0]


def test_one_context_per_key_and_thread(stubs, monkeypatch):
    first = _lib.shared_context(0)
    assert isinstance(first, _lib.SharedContext)
    assert _lib.shared_context(0, 16, 16) is first and _lib.shared_context(0) is first
    by_size = _lib.shared_context(0, 32, 16)
    by_device = _lib.shared_context(1)
    with monkeypatch.context() as m:
        m.setenv("MDVT_LIB_VARIANT", "tuning")
        by_variant = _lib.shared_context(0)
        assert _lib.shared_context(0) is by_variant
    assert len({id(c) for c in (first, by_size, by_device, by_variant)}) == 4
    assert _lib.shared_context(0) is first and _lib.shared_context(0, 32, 16) is by_size and _lib.shared_context(1) is by_device
    assert (by_size.W, by_size.H, by_device.device) == (32, 16, 1)

    # a second thread: another object for the same key, the same object within that thread; closed when the thread has ended
    ids = in_thread(lambda: (id(_lib.shared_context(0)), id(_lib.shared_context(0)), threading.get_ident()))
    assert ids[0] == ids[1] and ids[0] not in {id(c) for c in (first, by_size, by_device, by_variant)}
    assert ("create", ids[2], ids[0]) in stubs
    assert ("close", ids[0]) in stubs, "a thread's contexts are closed when the thread's store goes away"
    assert not any(e[0] == "close" and e[1] == id(first) for e in stubs), "the main thread's contexts stay open"
    assert _lib.shared_context(0) is first


def test_eight_threads_first_calling_for_one_key(stubs):
    barrier = threading.Barrier(8)
    got, errors = {}, []

    def worker(k):
        try:
            barrier.wait(timeout=30)
            a = _lib.shared_context(0)
            b = _lib.shared_context(0, 16, 16)
            got[k] = (threading.get_ident(), a, b)           # (the objects are kept: ids of dead objects may repeat)
            barrier.wait(timeout=30)                         # every thread alive until all have theirs
        except Exception as e:                               # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(k,), daemon=True) for k in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(60)
    assert not errors and len(got) == 8 and not any(t.is_alive() for t in threads)
    assert all(a is b for _, a, b in got.values())
    assert len({id(a) for _, a, _b in got.values()}) == 8, "two threads share a context"
    created = [e for e in stubs if e[0] == "create"]
    assert len(created) == 8, f"{len(created)} contexts constructed for 8 threads"
    assert sorted(t for _, t, _i in created) == sorted(t for t, _a, _b in got.values()), "a thread constructed two, another none"


X, Y = 0x1000, 0x2000


def _stream(v):
    return C.c_void_p(v)                 # as _lib.stream_arg hands it to the entry points


def test_calls_on_another_stream_wait_for_the_latest_call(stubs):
    ctx = _lib.shared_context(0)
    del stubs[:]
    ctx.call("mdvt_scale_shift_fit", 1, 2, _stream(X))
    ctx.call("mdvt_metric_depth_codes", 3, _stream(X))
    assert stubs == [("call", "mdvt_scale_shift_fit"), ("record", X, "event1"), ("call", "mdvt_metric_depth_codes"), ("record", X, "event2")]
    assert not any(e[0] == "wait" for e in stubs), "two calls on one stream issue no wait"
    ctx.call("mdvt_convergence_depths", 4, _stream(Y))
    waits = [e for e in stubs if e[0] == "wait"]
    assert waits == [("wait", Y, "event2")], "exactly one wait: Y on the event recorded behind the second call"
    kinds = [e[0] for e in stubs]
    assert kinds == ["call", "record", "call", "record", "wait", "call", "record"], "the wait precedes the call, the record follows it"
    assert stubs[-1] == ("record", Y, "event3")
    ctx.call("mdvt_scale_shift_fit", 5, _stream(X))           # back on X: waits on Y's event
    assert [e for e in stubs if e[0] == "wait"] == [("wait", Y, "event2"), ("wait", X, "event3")]
    assert stubs[-1] == ("record", X, "event4")
    ctx.call("mdvt_scale_shift_fit", 6, _stream(X))
    assert len([e for e in stubs if e[0] == "wait"]) == 2

    # NULL is the default stream, a stream like any other; an entry point without a stream argument is no call on a stream
    ctx.call("mdvt_swap_rb", 7, None)
    assert [e for e in stubs if e[0] == "wait"][-1] == ("wait", 0, "event5")
    n = len(stubs)
    ctx.call("mdvt_workspace_bytes", object())
    assert [e[0] for e in stubs[n:]] == ["call"]


def test_a_failed_call_still_leaves_its_event(stubs, monkeypatch):
    ctx = _lib.shared_context(0)
    monkeypatch.setattr(_lib.Context, "check", lambda self, rc: (_ for _ in ()).throw(_lib.MdvtError(-1, "refused")))
    del stubs[:]
    with pytest.raises(_lib.MdvtError):
        ctx.call("mdvt_scale_shift_fit", _stream(X))
    assert stubs[-1] == ("record", X, "event1"), "a refused call may have enqueued part of its work"


def test_the_plain_context_records_and_waits_on_nothing(stubs):
    ctx = _lib.Context(0, 16, 16)
    assert type(ctx) is _lib.Context
    del stubs[:]
    for s in (X, X, Y, X):
        ctx.call("mdvt_scale_shift_fit", 1, _stream(s))
    assert [e[0] for e in stubs] == ["call"] * 4
    assert not hasattr(ctx, "_record_event") and not hasattr(ctx, "_wait_event")


# ---- what else the GPU concurrency tests rest on, checked without a GPU ------------------------------------------------------------
def test_no_stream_lists_exactly_the_entry_points_without_one():
    """SharedContext.call reads the stream from an entry point's last argument unless NO_STREAM names it: every entry point of the
    headers that takes a ctx (but for create / destroy / last_error, which are not called through it) ends in `void* stream` or is
    in NO_STREAM, and the bound prototypes agree."""
    import glob
    import os
    import re
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = " ".join(re.sub(r"/\*.*?\*/", " ", open(h).read(), flags=re.S) for h in sorted(glob.glob(os.path.join(repo, "include", "mdvt*.h"))))
    decls = re.findall(r"\b(mdvt_[a-z0-9_]+)\s*\(\s*(?:const\s+)?mdvt_ctx\s*\*\s*\w+\s*([^;{]*)\)\s*;", text)
    names = {n for n, _ in decls} - {"mdvt_destroy", "mdvt_last_error"}
    assert len(names) > 30 and "mdvt_scale_shift_fit" in names and "mdvt_set_config" in names
    without = {n for n, rest in decls if n in names and not re.search(r"void\s*\*\s*stream\s*$", rest)}
    assert without == set(_lib.NO_STREAM)
    L = _lib.load()
    for n in names:
        assert (getattr(L, n).argtypes[-1] is C.c_void_p) == (n not in _lib.NO_STREAM), n


def test_an_entry_point_whose_last_argument_is_no_stream_is_refused(stubs):
    ctx = _lib.shared_context(0)
    ctx._L.mdvt_made_up = lambda *a: 0
    ctx._L.mdvt_made_up.argtypes = [C.c_void_p, C.c_int]
    del stubs[:]
    with pytest.raises(TypeError, match="mdvt_made_up"):
        ctx.call("mdvt_made_up", 7)
    assert stubs == [], "nothing was called, recorded or waited for"


def test_the_threads_schedules_draw_every_family_and_action():
    """tests/concurrency_cases.py's seeded schedules, as the GPU tests run them (four workers, 24 steps; 12 beside the pool thread):
    every worker meets all nine families; together they close and remake contexts, switch a live renderer and grow a scratch block
    of the family whose two calls differ in size for certain (convergence depths: one frame, five frames)."""
    import concurrency_cases as cc
    for steps in (24, 12):
        drawn = [cc.schedule(k, steps) for k in range(4)]
        assert all({fam for fam, *_ in sch} == set(cc.FAMILIES) for sch in drawn)
        actions = {(fam, action) for sch in drawn for fam, _v, action, _t in sch}
        assert ("convergence", "grow") in actions and {"recreate", "switch"} <= {a for _f, a in actions}, (steps, actions)
    assert cc.schedule(2, 24) == cc.schedule(2, 24) and cc.schedule(2, 24) != cc.schedule(3, 24)
