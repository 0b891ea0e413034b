"""The instrument of tests/test_streams_gpu.py: a calibrated spin that holds a stream busy.

torch's default stream is the legacy null stream and torch.cuda.Stream() objects are non-blocking
streams, so nothing orders one after the other.  While a `hold` runs on a stream, everything
queued behind it on that stream is late by the length of the hold and everything on another
stream is early: a fill or a read-back that went to the wrong stream turns into wrong bytes
every time, not now and then (the two positive controls of test_streams_gpu.py show exactly
that with torch ops alone).

`run(config, call, s)` drives one library call in one of the three configurations of the stream
contract ("Streams"):

  "current-held"  the current stream is the default stream and is held; the call gets stream=s.
                  Catches a buffer allocated or filled on the current stream (C3): its fill lands
                  after the kernel on s wrote it.  The call must return while the hold still runs
                  (C6: it waits for no stream but s).
  "own-held"      s itself is held and the call gets stream=s.  Catches a host read-back that is
                  not ordered after the kernel (C4) and a result object that reads on another
                  stream than the one that wrote it (C5), up to the call's first synchronise of s.
  "ambient"       the call runs inside torch.cuda.stream(s) with stream=None while the default
                  stream is held.  Catches anything pinned to the null stream (C1).

Two things about the instrument itself.  A `pending` assertion compares the call's HOST time with
the hold: the first use of a kernel in a process loads its code object, which has been measured
at 0.5 s for the first scan_batch, so a surface whose first use in the process falls under a hold
(the file run alone, or reordered) can outlast 200 ms without waiting for anything; the assertion
messages say so.  And the runtime maps streams onto a few hardware queues (4 by default), where
streams that share a queue run in order: pick_streams probes fresh streams for ones a spin on the
default stream does not delay, and raises AssertionError when a process that has opened very many
streams has none left -- that fails the whole module at its fixture, not one test.
"""
import os

import torch

HOLD_MS = 200            # the project's own delay knobs in test_robust_gpu.py use 300 ms
CONFIGS = ("current-held", "own-held", "ambient")

_spin = None             # (kind, units per millisecond), measured once per session


def _matmul_spin(n):
    a = torch.ones(2048, 2048, device="cuda")
    for _ in range(int(n)):
        a = (a @ a).clamp_(0, 1)


def _time(fn, units):
    """milliseconds `fn(units)` keeps a fresh stream busy, by a pair of events"""
    st = torch.cuda.Stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(st):
        fn(max(units // 100, 1))      # warm up: the first launch pays for loading the kernel
        e0.record()
        fn(units)
        e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _calibrate():
    """torch.cuda._sleep counts device clock ticks whose rate the host does not know: time a known
    count once.  Where it does not spin at all (a count returns at once), a chain of large matmuls
    calibrated the same way takes its place."""
    global _spin
    if _spin is None:
        units = 20_000_000
        ms = _time(torch.cuda._sleep, units)
        if ms > 1.0:
            _spin = ("sleep", units / ms)
        else:
            units = 50
            ms = _time(_matmul_spin, units)
            assert ms > 1.0, f"neither torch.cuda._sleep nor a matmul chain holds the device ({ms} ms)"
            _spin = ("matmul", units / ms)
    return _spin


def hold(stream, ms=HOLD_MS):
    """queue a spin of about `ms` milliseconds on `stream` -> an event recorded behind it
    (event.query() is False for as long as the hold runs)"""
    kind, per_ms = _calibrate()
    with torch.cuda.stream(stream):
        if kind == "sleep":
            torch.cuda._sleep(int(ms * per_ms))
        else:
            _matmul_spin(max(int(ms * per_ms), 1))
        ev = torch.cuda.Event()
        ev.record()
    return ev


def default_stream():
    return torch.cuda.default_stream()


def independent(a, b, ms=20):
    """True when work queued on `b` does not wait for a spin on `a`.  The runtime maps streams onto
    a few hardware queues (4 by default) and two streams that share one run in
    order whatever their flags say: a process that has created many streams, as the whole suite
    has, hands out such streams."""
    torch.cuda.synchronize()
    pending = hold(a, ms)
    with torch.cuda.stream(b):
        torch.zeros(1, device="cuda")
    b.synchronize()
    free = not pending.query()
    torch.cuda.synchronize()
    return free


def pick_streams(n=2, tries=32):
    """n non-default streams that are independent of the default stream and of one another, so a
    hold on one of them delays only what is queued behind it"""
    if bounds_build():
        return tuple(torch.cuda.Stream() for _ in range(n))
    picked = []
    for _ in range(tries):
        c = torch.cuda.Stream()
        if all(independent(o, c) and independent(c, o) for o in [default_stream()] + picked):
            picked.append(c)
            if len(picked) == n:
                return tuple(picked)
    raise AssertionError(f"no {n} streams with hardware queues of their own among {tries} candidates: "
                         f"the holds of this module need them")


def bounds_build():
    """the bounds-checked diagnostic build synchronises every launch (csrc/bounds.h), so no call is
    asynchronous there: the `pending` assertions are skipped, the comparisons stay (as
    tests/test_robust_gpu.py does for its own timing assertion)"""
    return bool(os.environ.get("MTBLX_BOUNDS_CHECK"))


def host(t, s):
    """a returned device tensor on the host, read in stream order on `s`: what a caller of the
    contract (C5: returned tensors are valid in stream order on S) does"""
    with torch.cuda.stream(s):
        return t.cpu().numpy()


def run(config, call, s, asynchronous=False, device_wide=False, ms=HOLD_MS):
    """Run `call(stream)` under `config` (see the module docstring) -> its result.

    asynchronous: the call is documented not to synchronise its stream (the *_into family,
    crc32c_blocks, uncompressed get_batch); under "own-held" it must return while the hold on
    its own stream still runs.  device_wide: the call reaches one of the documented exceptions
    to C6 (an entry point that allocates and frees device memory itself waits for the whole
    device), so it cannot return before a hold on another stream ends and `pending` is not
    asserted.  On return the result is safe to read on `s` ("own-held": nothing was synchronised,
    the result's own host-reading methods or host(t, s) must order the read themselves)."""
    assert config in CONFIGS
    torch.cuda.synchronize()              # inputs are uploaded and finished before a hold is armed
    assert torch.cuda.current_stream() == default_stream()
    check = not bounds_build()
    if config == "current-held":
        pending = hold(default_stream(), ms)
        out = call(s)
        returned_early = not pending.query()
        s.synchronize()
        if check and not device_wide:
            assert returned_early, "the call waited for the held current stream (C6), or outlasted the hold " \
                    "(its host time alone: the first use of a kernel in a process loads its code object)"
    elif config == "own-held":
        pending = hold(s, ms)
        out = call(s)
        if check and asynchronous:
            assert not pending.query(), "an asynchronous call synchronised its stream, or outlasted the hold " \
                "(its host time alone: the first use of a kernel in a process loads its code object)"
    else:
        pending = hold(default_stream(), ms)
        with torch.cuda.stream(s):
            out = call(None)
            returned_early = not pending.query()
        s.synchronize()
        if check and not device_wide:
            assert returned_early, "the call waited for the held null stream (C1 / C6), or outlasted the hold " \
                    "(its host time alone: the first use of a kernel in a process loads its code object)"
    return out
