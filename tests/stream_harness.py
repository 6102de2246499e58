"""A call between a delayed producer and an immediate consumer on a caller-owned stream.  TEST INFRASTRUCTURE for
tests/test_gpu_caller_stream.py: include/rt_hip.h calls the device-level entry points "asynchronous on `stream`", and a test on the
legacy null stream cannot tell a launch on `stream` from a launch on stream 0 or on the context's own stream.  Here it can:

* the stream is a NON-BLOCKING one (asserted through hipStreamGetFlags): the null stream does not order itself against it, so work
  that was misdirected to stream 0 runs at once — and it is one that the null stream was SEEN to overtake (overtaken_by_the_null_stream:
  streams share a few hardware queues, and a queue orders what the flag does not);
* every input buffer holds POISON when the call is made — another valid frame of the same shape — and every output a sentinel;
* on the stream, in front of the call: a bounded spin (torch.cuda._sleep), the event `delay_done`, then device-to-device copies of the
  real inputs into the input buffers (and the sentinel into the outputs once more: what ran too early is overwritten); behind it:
  copies of every output into tensors of their own, then poison into the inputs again;
* the host waits for that stream alone (never torch.cuda.synchronize()) and compares.

Whatever of the call was not ordered by the stream met poison or a sentinel.  THE BLINDNESS GUARD: straight after each call returns,
`delay_done` must not have happened yet — the delay was still pending when the call's last launch was enqueued.  A guard that does not
hold fails the test ("delay too short or the call waited"); a call that waits by design is passed with the source line of its wait and
is then held to its results only, and so is every call behind it in the same run (the delay has drained).

The delay is not a constant: the spin's rate is measured once per session with events, the host-side duration of the calls under
test is measured in a warm-up round on the same shapes and stream (which also takes every first-use hipMalloc out of the measured
round; one more round on the poison leaves the context's scratch holding another frame's intermediates), and the spin is sized to
MARGIN x HEADROOM times the longest such duration seen so far in the session, within [MIN_DELAY_MS, MAX_DELAY_MS].
Every tensor stays referenced by its harness until the stream has been waited for: the caching allocator hands nothing on."""
from __future__ import annotations

import ctypes as C
import time
from collections import namedtuple

import numpy as np

SENTINEL = 0x7FC0BEEF  # a NaN with a payload: an untouched word keeps these bits
MARGIN = 10.0  # the delay against the host-side duration of what is enqueued behind it: room for a busy host
HEADROOM = 1.25  # ... and the spin is asked for this much longer again: its rate was measured on one length, the delay has another
MIN_DELAY_MS, MAX_DELAY_MS = 20.0, 2000.0
HIP_STREAM_NON_BLOCKING = 0x01

Step = namedtuple("Step", "harness call label waits", defaults=(None,))  # waits: None, or the source line at which the call waits by design
FIGURES = []  # one dict per measured run: what the records of a session are written from (report())
_spin = {}
_longest_host_ms = [0.0]


def hip_runtime() -> C.CDLL:
    """The libamdhip64.so this process already runs on (torch's copy): found in the process's own mappings, not looked for on disk."""
    with open("/proc/self/maps") as maps:
        paths = {line.split()[-1] for line in maps if "libamdhip64.so" in line}
    assert len(paths) == 1, f"expected one HIP runtime in the process, found {sorted(paths)}"
    return C.CDLL(paths.pop())


def assert_non_blocking(stream) -> None:
    flags = C.c_uint(0xFFFFFFFF)
    status = hip_runtime().hipStreamGetFlags(C.c_void_p(stream.cuda_stream), C.byref(flags))
    assert status == 0, f"hipStreamGetFlags: {status}"
    assert flags.value & HIP_STREAM_NON_BLOCKING, f"the stream is a blocking one (flags {flags.value:#x}): the null stream would order itself behind it and hide a launch on stream 0"


def spin_rate() -> dict:
    """Cycles of torch.cuda._sleep per millisecond, measured once per session with events (the count is raised until the spin lasts
    5 ms: the launch around it no longer matters)."""
    import torch

    if not _spin:
        stream = torch.cuda.Stream()
        cycles = 1 << 20
        while True:
            begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                begin.record(stream)
                torch.cuda._sleep(cycles)
                end.record(stream)
            end.synchronize()
            ms = begin.elapsed_time(end)
            if ms >= 5.0 or cycles >= 1 << 36:
                break
            cycles *= 4
        assert ms > 0.0
        _spin.update(cycles=cycles, ms=ms, cycles_per_ms=cycles / ms)
    return _spin


PROBE_MS, CANDIDATES = 3.0, 16


def overtaken_by_the_null_stream(stream, device) -> bool:
    """Does work on the null stream really run while `stream` is busy?  The flag alone does not say: the runtime maps its streams onto
    a few hardware queues (four by default), and a stream that shares the null stream's queue is ordered with it by the queue itself —
    a launch misdirected to stream 0 would wait its turn there and be invisible again.  So it is tried: a spin on `stream`, a fill and
    an event on the null stream, the host waits for that event and then asks whether the spin has ended."""
    import torch

    spun, filled = torch.cuda.Event(), torch.cuda.Event()
    word = torch.zeros(1, dtype=torch.int32, device=device)
    null = torch.cuda.default_stream(device)
    assert null.cuda_stream == 0, "torch's default stream is not the legacy null stream"
    torch.cuda.synchronize(device)
    with torch.cuda.stream(stream):
        torch.cuda._sleep(int(PROBE_MS * spin_rate()["cycles_per_ms"]))
        spun.record(stream)
    with torch.cuda.stream(null):
        word.fill_(1)
        filled.record(null)
    filled.synchronize()
    overtook = not spun.query()
    stream.synchronize()
    return overtook


def independent_stream(device):
    """A non-blocking stream of torch's pool that the null stream overtakes -> (stream, candidates tried).  None among CANDIDATES fails."""
    import torch

    for tried in range(1, CANDIDATES + 1):
        stream = torch.cuda.Stream(device=device)
        assert_non_blocking(stream)
        if overtaken_by_the_null_stream(stream, device):
            return stream, tried
    raise AssertionError(f"none of {CANDIDATES} streams runs beside the null stream: a launch on stream 0 could not be told from one on the caller's stream")


class Harness:
    """One caller-owned stream and the buffers of the calls made on it."""

    def __init__(self, what: str, device: int = 0):
        import torch

        self.torch, self.what, self.device = torch, what, f"cuda:{device}"
        self.stream, self.candidates = independent_stream(self.device)
        self.delay_begin, self.delay_done = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.feeds, self.sinks, self.reads, self.guards = [], [], {}, []

    @property
    def handle(self) -> int:
        """The hipStream_t, as the entry points take it."""
        return self.stream.cuda_stream

    def _to_device(self, array):
        array = np.array(array, copy=True, order="C")  # (a copy: cached references are read-only)
        assert array.dtype in (np.float32, np.uint32, np.int32), array.dtype
        with self.torch.cuda.stream(self.stream):
            return self.torch.from_numpy(array.view(np.int32) if array.dtype == np.uint32 else array).to(self.device)

    def feed(self, real, poison):
        """An input buffer: it holds `poison` whenever no call is meant to read it; `real` waits on the device and is copied in behind the
        delay.  -> the buffer (a torch tensor; .data_ptr() is what the call gets)."""
        real, poison = np.ascontiguousarray(real), np.ascontiguousarray(poison)
        assert real.shape == poison.shape and real.dtype == poison.dtype, (real.shape, poison.shape)
        assert real.tobytes() != poison.tobytes(), f"{self.what}: the poison is the real input"
        staged, bad = self._to_device(real), self._to_device(poison)
        with self.torch.cuda.stream(self.stream):
            buffer = bad.clone()
        self.feeds.append((buffer, staged, bad))
        return buffer

    def sink(self, shape, fill: int = SENTINEL, read: bool = True):
        """An output buffer of 4-byte words, pre-filled with a sentinel; `read`: the consumer copies it out behind the calls."""
        with self.torch.cuda.stream(self.stream):
            buffer = self.torch.full(tuple(shape) if np.ndim(shape) else (int(shape),), fill, dtype=self.torch.int32, device=self.device)
        self.sinks.append((buffer, fill))
        if read:
            self.read(buffer)
        return buffer

    def read(self, buffer, key=None):
        """Have `buffer` copied out on the stream, into a tensor made here: behind the last call, or — with a `key` — where a call
        sequence says snap(key): an intermediate result that a later call of a chain overwrites."""
        with self.torch.cuda.stream(self.stream):
            self.reads[id(buffer) if key is None else key] = (buffer, self.torch.empty_like(buffer), key is None)
        return buffer

    def snap(self, key) -> None:
        source, copy, at_end = self.reads[key]
        assert not at_end
        with self.torch.cuda.stream(self.stream):
            copy.copy_(source, non_blocking=True)

    def got(self, buffer_or_key) -> np.ndarray:
        """What the consumer copied out of a buffer, as uint32 words (after run())."""
        key = buffer_or_key if isinstance(buffer_or_key, str) else id(buffer_or_key)
        return self.reads[key][1].cpu().numpy().view(np.uint32)

    # ---- the phases of a run (run() below drives them) ---------------------------------------------------------------------------
    def _reset(self, poisoned: bool) -> None:
        with self.torch.cuda.stream(self.stream):
            for buffer, fill in self.sinks:
                buffer.fill_(fill)
            if poisoned:
                for buffer, _, bad in self.feeds:
                    buffer.copy_(bad, non_blocking=True)
        self.stream.synchronize()

    def _produce(self) -> None:
        """On the stream: the sentinel into every output once more (what a launch that ran too early wrote there, or cleared there, is
        gone again), then the real inputs."""
        with self.torch.cuda.stream(self.stream):
            for buffer, fill in self.sinks:
                buffer.fill_(fill)
            for buffer, staged, _ in self.feeds:
                buffer.copy_(staged, non_blocking=True)

    def _delay(self, ms: float) -> None:
        with self.torch.cuda.stream(self.stream):
            self.delay_begin.record(self.stream)
            self.torch.cuda._sleep(int(ms * spin_rate()["cycles_per_ms"]))
            self.delay_done.record(self.stream)
        self._produce()

    def _collect(self) -> None:
        with self.torch.cuda.stream(self.stream):
            for source, copy, at_end in self.reads.values():
                if at_end:
                    copy.copy_(source, non_blocking=True)
            for buffer, _, bad in self.feeds:
                buffer.copy_(bad, non_blocking=True)


def delay_for(host_ms: float) -> float:
    _longest_host_ms[0] = max(_longest_host_ms[0], host_ms)
    return min(max(HEADROOM * MARGIN * _longest_host_ms[0], MIN_DELAY_MS), MAX_DELAY_MS)


def run(steps, warm_steps=None, settle=None) -> list:
    """The measured run of `steps` (Step tuples, in the order the host makes the calls; one or several harnesses) -> what the calls
    returned.  warm_steps: what the warm-up rounds call instead (the same shapes on another context, where the measured calls are to
    find their context fresh).  settle: host-side preparation in front of every round, synchronised before the delay is enqueued."""
    harnesses = list({id(s.harness): s.harness for s in steps}.values())
    host_ms = 0.0
    for _ in range(2):  # the first round takes the first-use allocations and code loads, the second is timed
        for h in harnesses:
            h._reset(poisoned=False)
        if settle is not None:
            settle()
        begin = time.perf_counter()
        for h in harnesses:
            h._produce()
        for s in steps if warm_steps is None else warm_steps:
            s.call()
        host_ms = (time.perf_counter() - begin) * 1e3
        for h in harnesses:
            h.stream.synchronize()
    # a round on the POISON: the context's scratch (histogram, ping-pong blocks, pyramid, counters) now holds another frame's
    # intermediates, not this one's — a launch that runs too early reads something plausible and wrong there too
    for h in harnesses:
        h._reset(poisoned=True)
    if settle is not None:
        settle()
    for s in steps if warm_steps is None else warm_steps:
        s.call()
    for h in harnesses:
        h._reset(poisoned=True)
    if settle is not None:
        settle()
    asked_ms = delay_for(host_ms)
    for h in harnesses:
        h.guards = []
        h._delay(asked_ms)
    results, waited = [], None
    for s in steps:
        results.append(s.call())
        ended = s.harness.delay_done.query()  # straight after the call returned
        s.harness.guards.append((s.label, ended, s.waits, waited))
        waited = waited or s.waits
    for h in harnesses:
        h._collect()
    for h in harnesses:
        h.stream.synchronize()  # this stream alone
    for h in harnesses:
        measured_ms = h.delay_begin.elapsed_time(h.delay_done)
        FIGURES.append({"what": h.what, "candidates": h.candidates, "host_ms": host_ms, "delay_asked_ms": asked_ms, "delay_measured_ms": measured_ms,
                        "guards": [(label, "waits by design: " + waits if waits else ("behind a wait" if before else ("ENDED" if ended else "pending"))) for label, ended, waits, before in h.guards]})
        for label, ended, waits, before in h.guards:
            if waits is None and before is None:
                assert not ended, (f"{h.what} / {label}: delay too short or the call waited (the delay had ended when the call returned; host-side duration in the warm-up {host_ms:.3f} ms, "
                                   f"delay asked for {asked_ms:.1f} ms, measured {measured_ms:.1f} ms)")
    return results


def report() -> str:
    """The session's calibration and every measured run, one line each."""
    lines = []
    if _spin:
        lines.append(f"spin: {_spin['cycles']} cycles took {_spin['ms']:.3f} ms -> {_spin['cycles_per_ms']:.0f} cycles per ms; longest host-side duration {_longest_host_ms[0]:.3f} ms; margin x{MARGIN:g}, delay within [{MIN_DELAY_MS:g}, {MAX_DELAY_MS:g}] ms")
    for f in FIGURES:
        lines.append(f"{f['what']}: stream candidate {f['candidates']}, host {f['host_ms']:.3f} ms, delay asked {f['delay_asked_ms']:.1f} ms, measured {f['delay_measured_ms']:.1f} ms; " + ", ".join(f"{label}: {state}" for label, state in f["guards"]))
    return "\n".join(lines)
