"""The library entered from several host threads at once, and one shared context called on two streams with no host wait between.

include/mdvt.h: "a ctx is not thread-safe, distinct ctxs are independent" and, of the pools, "Process-wide, thread-safe".  The
Python faces hide their context (_lib.shared_context), so they keep both rules themselves: the context is per host thread, and it
orders its calls across streams (_lib.SharedContext; tests/test_shared_context_cpu.py holds that bookkeeping to its rules without
a GPU).  Here, on the GPU:

  C1  a face's call on stream b waits for the same face's call on stream a (which is held up by a calibrated sleep), and calls that
      need no ordering -- the same stream, a plain Context of the caller's own -- do not wait;
  C2  such calls overlapping on two streams give their references' bits;
  C5  the control: four seeded schedules over nine families of calls, one after the other on the main thread;
  C3  the same schedules in four threads at once, each with a stream, contexts and renderers of its own;
  C4  the same beside a fifth thread that reads, empties and resizes the process-wide pool of workspace blocks.

Every expected value is an oracle's or a reference's, computed once (tests/concurrency_cases.py) before any thread starts; every
comparison is equality of bytes, or same bits / both NaN for the fit and the means."""
import ctypes as C
import gc
import threading
import time

import numpy as np
import pytest

import concurrency_cases as cc
import convergence_ref as cr
import metric_align_ref as mr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

STATE = {"control_wall": None, "hung": None, "cycles": None}
POOL_CALLS_BEFORE_STEP = {4: 3, 8: 6}          # C4: a worker's step -> the pool calls that are done before any worker starts it


@pytest.fixture(scope="module")
def mat(orc):
    assert torch.cuda.is_available(), "needs a GPU"
    return cc.Material(orc)


def _not_after_a_hang():
    if STATE["hung"]:
        pytest.fail(f"not run: {STATE['hung']} -- nothing more is started on the GPU")


# ------------------------------------------------------------------------------------------------ the instruments of C1
def _sleep_cycles(target_s=0.2):
    """torch.cuda._sleep's cycle count for about target_s seconds, measured with two events (the counter's rate is the device's)."""
    s = torch.cuda.Stream()
    cycles, ms = 1_000_000, 0.0
    for _ in range(6):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            e0.record()
            torch.cuda._sleep(cycles)
            e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= 10.0:
            break
        cycles *= 8
    assert ms >= 10.0, f"torch.cuda._sleep({cycles}) lasted {ms} ms"
    return int(cycles * target_s * 1000.0 / ms)


def _side_by_side_streams(cycles):
    """(a, b): two streams the hardware runs side by side -- found with torch alone: a kernel on b completes while a sleeps.  (Streams
    that share a hardware queue run one after the other whatever the library does; on them neither half of C1 would mean anything.)"""
    a = torch.cuda.Stream()
    x = torch.zeros(64, device="cuda")
    torch.cuda.synchronize()
    for _ in range(12):
        b = torch.cuda.Stream()
        ea, eb = torch.cuda.Event(), torch.cuda.Event()
        with torch.cuda.stream(a):
            torch.cuda._sleep(cycles // 10)
            ea.record()
        with torch.cuda.stream(b):
            x.add_(1)
            eb.record()
        eb.synchronize()
        beside = not ea.query()
        torch.cuda.synchronize()
        if beside:
            return a, b
    pytest.fail("no stream of torch's pool runs beside another one: every kernel waits for a sleep on another stream")


def _faces(mat):
    """name -> (call(stream, ctx) -> handle, verify(handle)).  ctx None: the Python face (the thread's shared context); else the
    entry point on that plain Context."""
    from metric_depth_video_toolbox_amd import _lib, ffv1_device as fd, find_convergence_depth as fcd, video_metric_convert as vmc
    f, c, d = mat.fit[(5, 41, 83)], mat.convergence["5x205x83"], mat.stream

    def fit(stream, ctx=None):
        if ctx is None:
            return vmc.compute_scale_and_shift_full(f["p"], f["d"], target_is_depth=True, stream=stream).values
        with torch.cuda.stream(stream):              # (the poison is ordered in front of the call that overwrites it)
            out = cc.poisoned((8,), torch.float32)
        ctx.check(cc.raw_fit(_lib, ctx, f["p"], f["d"], None, out, tid=1, stream=stream))
        return out

    def fit_ok(values):
        bad = mr.same_bits(values.cpu().numpy(), f["want"])
        assert bad.size == 0, f"fit: floats {bad.tolist()} differ"

    def conv(stream, ctx=None):
        if ctx is None:
            return fcd.convergence_depths(c["d"], c["m"], stream=stream)
        with torch.cuda.stream(stream):
            means = cc.poisoned((5,), torch.float32)
        ctx.check(cc.raw_convergence(_lib, ctx, c["d"], c["m"], 3, means, stream=stream))
        return means

    def conv_ok(means):
        bad = cr.same_bits(means.cpu().numpy(), c["want"])
        assert bad.size == 0, f"convergence depths: frames {bad.tolist()} differ"

    def decode(stream, ctx=None):
        # decode_stream_on_device's two halves: its enqueue on the same context (_context), its collect in decode_ok -- the face
        # itself waits for its frames on the host, so a second call could not be made while the first is held up
        with torch.cuda.stream(stream):
            out = cc.poisoned((d["N"], d["H"], d["W"], 3))
        return fd.enqueue_decode_stream(fd._context(0) if ctx is None else ctx, d["packets"], d["cfg"], d["W"], d["H"], out=out, stream=stream)

    def decode_ok(p):
        frames = p.collect().cpu().numpy()
        assert p.host_frames == 0 and not p.flags.any(), (p.flags.tolist(), p.host_frames)
        assert np.array_equal(frames, d["want"]), "decoded frames differ"

    return {"compute_scale_and_shift_full": (fit, fit_ok), "convergence_depths": (conv, conv_ok), "decode_stream_on_device": (decode, decode_ok)}


@pytest.mark.parametrize("face", ["compute_scale_and_shift_full", "convergence_depths", "decode_stream_on_device"])
def test_shared_faces_on_two_streams_are_ordered(mat, face):
    """C1.  Stream a sleeps (a cycle count calibrated to about 0.2 s, the sleep itself timed with two events), then runs the face's
    call 1; the same face is called on stream b at once.  The face's context is shared and keeps its scratch block between the
    two, so call 2 has to wait for call 1: the host time from enqueuing call 2 to an event behind it must be at least half the
    sleep's measured duration (unordered, a call this small is done in well under a millisecond).  Then the converse, under one
    more sleep each: two calls on the same stream, and a call on a plain Context of the test's own, do not wait for stream a --
    their event completes while a's still reports not ready.  The third face is the decoder's enqueue on the shared context
    (ffv1_device.enqueue_decode_stream(_context(0), ...)): decode_stream_on_device itself waits for its frames on the host before
    it returns, so two of its calls never overlap and it cannot meet the hazard at all."""
    _not_after_a_hang()
    from metric_depth_video_toolbox_amd import _lib
    call, verify = _faces(mat)[face]
    if STATE["cycles"] is None:
        STATE["cycles"] = _sleep_cycles()            # calibrated once
    cycles = STATE["cycles"]
    a, b = _side_by_side_streams(cycles)
    own = _lib.Context(0, 16, 16)
    try:
        for s in (a, b, a):                          # every lazy allocation and scratch growth happens here, not under the sleep
            r1, r2 = call(s), call(s, own)
            s.synchronize()                          # (verify reads back on the current stream, which does not wait for s)
            verify(r1)
            verify(r2)
        torch.cuda.synchronize()
        shared = _lib.shared_context(0)
        assert type(shared) is _lib.SharedContext and type(own) is _lib.Context

        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(a):
            e0.record()
            torch.cuda._sleep(cycles)
            e1.record()
        r1 = call(a)
        t0 = time.perf_counter()
        r2 = call(b)
        eb = torch.cuda.Event()
        eb.record(b)
        eb.synchronize()
        waited = time.perf_counter() - t0
        a.synchronize()
        slept = e0.elapsed_time(e1) / 1000.0
        print(f"C1 {face}: {cycles} cycles slept {slept * 1000:.1f} ms; call 2 on the other stream was done after {waited * 1000:.1f} ms")
        assert waited >= 0.5 * slept, f"call 2 was done after {waited * 1000:.2f} ms while stream a slept {slept * 1000:.1f} ms: not ordered"
        verify(r1)
        verify(r2)

        # The decoder copies its packets on a stream of torch's pool, a new one at every call, and makes the caller's stream wait for
        # the copy; where that stream shares a hardware queue with a, the copy -- and so the call -- waits for a's sleep whatever
        # the context does.  One try that does not wait shows that the library imposes no order, so the decoder gets up to 12 tries
        # (shorter sleeps); the other two faces get one.
        tries, nap = (12, cycles // 4) if face == "decode_stream_on_device" else (1, cycles)
        for what, ctx in (("two calls on one stream", None), ("a plain Context on another stream", own)):
            for k in range(tries):
                torch.cuda.synchronize()
                ea = torch.cuda.Event()
                with torch.cuda.stream(a):
                    torch.cuda._sleep(nap)
                    ea.record()
                t0 = time.perf_counter()
                r1 = call(b, ctx)
                r2 = call(b, ctx)
                eb = torch.cuda.Event()
                eb.record(b)
                eb.synchronize()
                took = time.perf_counter() - t0
                still_asleep = not ea.query()
                a.synchronize()
                verify(r1)
                verify(r2)
                if still_asleep:
                    break
            print(f"C1 {face}: {what} were done after {took * 1000:.2f} ms, stream a still asleep: {still_asleep} (try {k + 1} of {tries})")
            assert still_asleep, f"{what} waited for the sleep on stream a in every one of {tries} tries (last: {took * 1000:.1f} ms)"
    finally:
        torch.cuda.synchronize()
        own.close()


def test_shared_faces_overlapping_on_two_streams_give_their_bytes(mat):
    """C2.  The fit of (2, 2053, 2047) -- 1026 chunks, two launch sets -- on stream a and, with no host wait, the fit of (1, 3, 43)
    on stream b, 20 times, alternating which goes first; then convergence_depths with a masked batch of 8 and a batch of 1 in the
    same way.  Both share one context's scratch block, so every result has its reference's bits only if the context orders them.
    Probabilistic by nature: unordered calls need not collide in any one run.  C1 is the proof of the ordering, this the proof that
    the bytes survive it."""
    _not_after_a_hang()
    from metric_depth_video_toolbox_amd import find_convergence_depth as fcd, video_metric_convert as vmc
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    big_case = [c for c in mr.FIT_INPUTS["growth"] if c[1] == (2, 2053, 2047)][0]
    p, d, _ = mr.fit_input(*big_case)
    big = dict(p=up(p), d=up(d), want=mr.fit(mr.concat(p), mr.concat(mr.inverse(d))))
    small = mat.fit[(1, 3, 43)]
    W, H = 205, 83
    d8, m8 = cc.convergence_batch(np.random.default_rng(8), 8, 8, H, W, empty=2)
    d1, _m = cc.convergence_batch(np.random.default_rng(1), 1, 0, H, W)
    conv8 = dict(d=up(d8), m=up(m8), want=cr.clip_means(d8, m8)[0])
    conv1 = dict(d=up(d1), m=None, want=cr.clip_means(d1)[0])
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()

    fit = lambda m, s: vmc.compute_scale_and_shift_full(m["p"], m["d"], target_is_depth=True, stream=s).values
    conv = lambda m, s: fcd.convergence_depths(m["d"], m["m"], stream=s)
    for name, fn, same, large, little in (("fit", fit, mr.same_bits, big, small), ("convergence_depths", conv, cr.same_bits, conv8, conv1)):
        got = []
        for k in range(20):
            if k % 2 == 0:
                got.append((fn(large, a), fn(little, b)))
            else:
                second = fn(little, b)
                got.append((fn(large, a), second))
        torch.cuda.synchronize()
        for k, (gl, gs) in enumerate(got):
            for which, g, m in (("larger", gl, large), ("smaller", gs, little)):
                bad = same(g.cpu().numpy(), m["want"])
                assert bad.size == 0, f"{name}, repeat {k}, the {which} call: values {bad.tolist()} differ from the reference"


# ------------------------------------------------------------------------------------------------ the schedules
def _raise_first(workers):
    for w in workers:
        if w.error is not None:
            tag, e = w.error
            raise AssertionError(f"{tag}: {type(e).__name__}: {e}") from e


def _control(mat):
    """The four schedules of C3 one after the other on the main thread -> wall seconds (measured once)."""
    if STATE["control_wall"] is None:
        t0 = time.perf_counter()
        workers = [cc.Worker(mat, k, 24) for k in range(4)]
        for w in workers:
            w.run()
            _raise_first([w])
        torch.cuda.synchronize()
        STATE["control_wall"] = time.perf_counter() - t0
        # a "grow" step of the convergence family really grows its context's scratch block (behind a device synchronisation)
        grown = [sizes for w in workers for fam, sizes in w.growth if fam == "convergence"]
        assert grown and all(small < large == after for small, large, after in grown), f"workspace bytes over the grow steps: {grown}"
        steps = sum(len(w.log) for w in workers)
        longest = max(leave - enter for w in workers for *_x, enter, leave in w.log)
        print(f"C5 control: 4 schedules, {steps} calls, {STATE['control_wall']:.2f} s; the longest call took {longest * 1000:.1f} ms")
    return STATE["control_wall"]


def _join_limit(mat):
    return max(60.0, 10.0 * _control(mat))


def test_the_schedules_single_threaded(mat):
    """C5.  The control of C3 and C4: the same four schedules through the same code, one after the other.  A failure here is a
    case's, not concurrency's.  Its wall time gives the threads' join limit (ten times it, at least 60 s)."""
    _not_after_a_hang()
    wall = _control(mat)
    print(f"C5 control wall time {wall:.2f} s -> join limit {_join_limit(mat):.0f} s")


def _threads(mat, steps, extra=None, gate=None):
    """Four workers behind a barrier (with the extra thread, if any) -> the workers, joined or the test failed."""
    limit = _join_limit(mat)
    barrier = threading.Barrier(4 + (1 if extra else 0))
    workers = [cc.Worker(mat, k, steps, barrier, gate) for k in range(4)]
    alive = cc.run_in_threads(workers, limit, [extra(barrier, workers)] if extra else ())
    if alive:
        STATE["hung"] = f"threads {alive} were still running after {limit:.0f} s"
        pytest.fail(STATE["hung"])
    _raise_first(workers)
    assert all(w.done and len(w.log) >= steps for w in workers)
    return workers


def test_independent_contexts_in_four_threads(mat):
    """C3.  Four threads, each with a stream, a plain Context and renderers of its own and -- through the Python faces -- a shared
    context of its own, run 24 seeded steps over the nine families; at seeded steps a thread closes a context or renderer and
    makes a new one (blocks travel between the threads through the pools), runs a family's smaller, larger and smaller call on fresh
    contexts (the scratch block grows behind a device synchronisation while the others enqueue) or switches a live renderer's grid or budget.
    Every output equals its reference.  It does not pass without overlap: for at least six of the nine families a step must
    have been inside the library (from its first call to its stream's synchronisation) while a step of another thread was."""
    _not_after_a_hang()
    workers = _threads(mat, 24)
    pairs = cc.overlaps([w.log for w in workers])
    print("C3 overlapping pairs of steps of different threads, per family: " + ", ".join(f"{f} {n}" for f, n in pairs.items()))
    assert sum(n > 0 for n in pairs.values()) >= 6, f"too little overlap to mean anything: {pairs}"


def test_pool_calls_from_a_fifth_thread(mat):
    """C4.  The workers of C3 with 12 steps each, and a fifth thread that calls mdvt_cached_memory, mdvt_release_cached_memory and
    mdvt_set_cached_memory_limit (0, 1 MiB, the default 4 GiB in turn), one after the other with a short seeded pause, at most 40
    calls, for as long as a worker runs.  Every status is 0, every worker's outputs equal their references, and once every context
    of the test is closed a release leaves the pool empty.

    How many calls fit beside the workers is not left to the machine's speed: a release synchronises the device, which can take as
    long as the workers keep it busy, and 12 steps take some tens of milliseconds.  So the workers meet the fifth thread twice: none
    starts its step 4 before 3 pool calls are done, nor its step 8 before 6 (POOL_CALLS_BEFORE_STEP).  From there the threads run on
    side by side -- steps 4 to 7 beside calls 4 to 6, with the limit at 0, steps 8 to 11 beside the calls from 7 on -- so at least
    6 calls, two of each kind, were made while a worker still had steps to run; that is what is asserted."""
    _not_after_a_hang()
    from metric_depth_video_toolbox_amd import _lib
    L = _lib.load()
    statuses, ended = [], []
    turnstile = threading.Condition()

    def gate(step):
        need = POOL_CALLS_BEFORE_STEP.get(step)
        if need:
            with turnstile:
                assert turnstile.wait_for(lambda: len(statuses) >= need or ended, timeout=60), f"{len(statuses)} pool calls before step {step}"

    def pool_thread(barrier, workers):
        def pool_calls():
            try:
                rng = np.random.default_rng(20261019 + 5)
                limits = (0, 1 << 20, cc.DEFAULT_LIMIT)
                barrier.wait(timeout=60)
                while len(statuses) < 40 and not all(w.done for w in workers):
                    n = len(statuses)
                    if n % 3 == 0:
                        nbytes, blocks = C.c_uint64(), C.c_uint64()
                        done = ("cached_memory", L.mdvt_cached_memory(0, C.byref(nbytes), C.byref(blocks)))
                    elif n % 3 == 1:
                        done = ("release_cached_memory", L.mdvt_release_cached_memory(0))
                    else:
                        done = (f"set_cached_memory_limit({limits[n // 3 % 3]})", L.mdvt_set_cached_memory_limit(limits[n // 3 % 3]))
                    with turnstile:
                        statuses.append(done)
                        turnstile.notify_all()
                    time.sleep(float(rng.uniform(0.0002, 0.002)))      # (the workers' steps take a millisecond or two each)
            finally:
                with turnstile:                      # (whatever ended this thread, no worker waits for it any longer)
                    ended.append(True)
                    turnstile.notify_all()
        return pool_calls

    try:
        workers = _threads(mat, 12, pool_thread, gate)
    finally:
        L.mdvt_set_cached_memory_limit(cc.DEFAULT_LIMIT)
    print(f"C4: {len(statuses)} pool calls while a worker had steps to run: " + ", ".join(name for name, _ in statuses))
    assert all(rc == 0 for _, rc in statuses), [s for s in statuses if s[1] != 0]
    assert len(statuses) >= max(POOL_CALLS_BEFORE_STEP.values()), f"only {len(statuses)} pool calls: the fifth thread ended early"
    assert all(rc == 0 for w in workers for rc in w.statuses)
    del workers
    gc.collect()                                     # (contexts earlier tests dropped without closing go to the pool now, not later)
    torch.cuda.synchronize()
    assert L.mdvt_release_cached_memory(0) == 0
    assert _lib.cached_memory(0) == (0, 0), f"idle (bytes, blocks) after a release: {_lib.cached_memory(0)}"
