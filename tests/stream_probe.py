"""The probe of the caller-stream contract (include/h2agg.h: h2agg_set_stream, the queued entry points).

A queued entry point promises two things: its launches go to the caller's stream s (inputs need only be complete ON s, outputs
are valid for what the caller queues on s next), and the call itself does not wait.  Both are invisible to a test that
synchronises the device around the call.  The probe makes them visible with a stream that is held busy:

  d_in holds a DECOY (a second valid input whose result differs); on s a spinning kernel runs for HOLD_MS and, behind it, a
  device-to-device copy puts the TRUE input into d_in.  The library call is made while s is still held.  Work that is ordered
  behind the copy on s sees the true input; work on any other stream, or a call that reads d_in from the host side of the
  hold, sees the decoy.  A snapshot of d_out queued on s behind the call, read after s (and only s) has drained, must be the
  reference of the true input byte for byte.

torch.cuda._sleep is the spinning kernel; its cycles per millisecond are measured once (the slope between two lengths).
Streams that share a hardware queue run one after the other whatever the program says (csrc/h2agg.hip place_streams), so
where a test needs two streams that really run side by side it asks runs_beside() first.

HOLD_MS is max(100, 20 x the slowest host enqueue of any case), measured on an idle stream: DESIGN.md 5.13 has the table."""
import time

import torch

HOLD_MS = 100
PATTERN = 0xA5            # what d_out holds before the call: bytes the call must not write keep it
_CAL = {}


def device():
    return torch.device("cuda", 0)


def to_device(data: bytes):
    """bytes -> a uint8 tensor on the device, complete before this returns"""
    t = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(device())
    torch.cuda.synchronize()
    return t


def to_host(t) -> bytes:
    return bytes(t.cpu().numpy().tobytes())


def _timed_sleep(cycles):
    best = None
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(cycles)
        b.record()
        b.synchronize()
        t = a.elapsed_time(b)
        best = t if best is None else min(best, t)
    return best


def cycles_per_ms():
    """the slope of torch.cuda._sleep between two lengths (the launch overhead drops out), measured once per process"""
    if "slope" not in _CAL:
        torch.cuda._sleep(1000)
        torch.cuda.synchronize()
        lo = 1 << 20
        while _timed_sleep(lo) < 4.0 and lo < 1 << 40:       # whatever the counter's rate is: a first length of >= 4 ms
            lo <<= 1
        hi = 4 * lo
        t_lo, t_hi = _timed_sleep(lo), _timed_sleep(hi)
        assert t_hi > t_lo > 0, (lo, t_lo, t_hi)
        _CAL["slope"] = (hi - lo) / (t_hi - t_lo)
    return _CAL["slope"]


def hold(stream, ms):
    """keep `stream` busy for ms milliseconds from the moment it gets there"""
    cycles = int(ms * cycles_per_ms())
    with torch.cuda.stream(stream):
        torch.cuda._sleep(cycles)


def runs_beside(held, work, ms=20):
    """True when work() (which queues something elsewhere and waits for it) comes back while `held` is still busy: the two do
    not share a hardware queue.  Judged by the host's clock as well as by the stream's own answer — work that had to queue
    behind the hold cannot come back in less than half of it.  Leaves both idle."""
    t0 = time.perf_counter()
    hold(held, ms)
    work()
    took_ms = 1e3 * (time.perf_counter() - t0)
    beside = not held.query() and took_ms < ms / 2
    held.synchronize()
    return beside


def stream_beside(work_on, tries=8):
    """a new torch stream c for which work_on(c) -> (held stream, work) runs side by side; fails when none of `tries` does"""
    kept = []
    for _ in range(tries):
        cand = torch.cuda.Stream()
        kept.append(cand)
        held, work = work_on(cand)
        if runs_beside(held, work):
            return cand
    raise AssertionError("none of %d new streams runs beside the work: every one shares its hardware queue" % tries)


def torch_work(stream):
    """a tiny piece of work on `stream`, waited for"""
    def work():
        with torch.cuda.stream(stream):
            torch.zeros(64, dtype=torch.uint8, device=device()).add_(1)
        stream.synchronize()
    return work


def prepare(eng, call, true_in, decoy_in, d_in, d_out, in_place=False, warm=1):
    """steps 1 and 2a: `warm` calls of exactly this shape on the decoy so that no workspace grows later, then d_in = decoy,
    d_out = PATTERN, the device drained -> (the true input in a device buffer of its own, its bytes), for run()"""
    d_decoy, d_true = to_device(decoy_in), to_device(true_in)
    for _ in range(warm):
        d_in.copy_(d_decoy)
        torch.cuda.synchronize()
        call()
        eng.synchronize()
    d_in.copy_(d_decoy)
    if not in_place:
        d_out.fill_(PATTERN)
    torch.cuda.synchronize()
    return d_true, bytes(true_in)


def run(eng, s, call, staged, d_in, d_out, in_place=False, no_wait=True, after="stream", on_stream_done=None,
        hold_ms=None):
    """steps 2b to 5 -> the bytes d_out held behind the call.
    after = "stream": the snapshot queued on s, read after s.synchronize() alone.  after = "engine": d_out after
    eng.synchronize() (MSMs with tail overlap: the header promises the result only there).
    no_wait: the call must come back while s is still held, and in less than half the hold.
    Nothing here touches the default stream before on_stream_done has been called: the default stream may share its
    hardware queue with a stream that another test holds, and a read-back on it would then wait for that hold."""
    hold_ms = HOLD_MS if hold_ms is None else hold_ms
    d_true, true_in = staged
    snap = None
    with torch.cuda.stream(s):
        hold(s, hold_ms)
        d_in.copy_(d_true, non_blocking=True)                 # the true input arrives on s, behind the hold
        t0 = time.perf_counter()
        call()
        took_ms = 1e3 * (time.perf_counter() - t0)
        busy = not s.query()
        if no_wait:
            assert busy, "the stream had drained when the call came back: the call waited for it (%.1f ms)" % took_ms
            assert took_ms < hold_ms / 2, "the call took %.1f ms of a %d ms hold: it waited" % (took_ms, hold_ms)
        if after == "stream":
            snap = d_out.clone()
    if after == "stream":
        s.synchronize()                                       # s alone: not the context, not the device
        if on_stream_done is not None:
            on_stream_done()
        got = to_host(snap)
        eng.synchronize()                                     # must be clean: no status raised by a run on the decoy's rows
        assert to_host(d_out) == got, "d_out changed after the stream had passed the call"
    else:
        eng.synchronize()
        got = to_host(d_out)
    if not in_place:
        assert to_host(d_in) == true_in, "the input buffer does not hold the true input"
    return got


def probe(eng, s, call, true_in, decoy_in, d_in, d_out, in_place=False, no_wait=True, after="stream", warm=1):
    """the whole probe -> the bytes of d_out as the caller's stream saw them behind the call"""
    staged = prepare(eng, call, true_in, decoy_in, d_in, d_out, in_place, warm)
    return run(eng, s, call, staged, d_in, d_out, in_place, no_wait, after)


def probe_input_side(eng, s, call, true_in, decoy_in, d_in, warm=1):
    """a synchronous entry point that reads device memory: decoy, hold, the true input copied behind the hold, the call ->
    what the call returned.  It waits by contract, so there is nothing to ask of s afterwards."""
    d_decoy, d_true = to_device(decoy_in), to_device(true_in)
    for _ in range(warm):
        d_in.copy_(d_decoy)
        torch.cuda.synchronize()
        call()
    d_in.copy_(d_decoy)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        hold(s, HOLD_MS)
        d_in.copy_(d_true, non_blocking=True)
        out = call()
    eng.synchronize()
    assert to_host(d_in) == bytes(true_in), "the input buffer does not hold the true input"
    return out
