"""What the stream-order tests share (test_gpu_stream_order.py, test_gpu_poison_reuse.py,
test_gpu_robust_streams.py): a pair of streams that really run side by side, queued work on blocks the
code under test allocates next, and LATE LAUNCHES — every launch of the robust pipeline delayed by a
device spin on its own stream, so that the host and the copy stream run ahead of every kernel. That is
the regime in which a missing wait, a buffer freed too early or a missing synchronise changes bits
instead of hiding behind an idle stream."""
import contextlib
import inspect
import time

import pytest
import torch

DEV = "cuda:0"
SPIN_CYCLES = 30_000_000              # torch.cuda._sleep cycles: ~10 ms or more (the poison test's spin)
LATE_OPS = ("trimmed_mean", "pairwise_sqdist", "weighted_mean_sqdist", "centered_clip_step",
            "median_window_mean")


def side_by_side_streams():
    """(staging, compute): two streams of the device that run side by side. torch hands streams out of
    a pool and the runtime maps them onto a few hardware queues; two streams on one queue run in
    order, so the poison (staging stream) would wait behind the busy compute stream and land after
    the read, and the test would say nothing about the knob. Which pooled streams share a queue
    depends on how many streams the process drew before and in which order they were first used,
    so the pair is chosen by looking: a stream whose small fill ends while the other still spins."""
    compute = torch.cuda.Stream(DEV)
    for _ in range(16):
        staging = torch.cuda.Stream(DEV)
        spun, filled = torch.cuda.Event(), torch.cuda.Event()
        with torch.cuda.stream(compute):
            torch.cuda._sleep(30_000_000)                  # ~10 ms or more
            spun.record(compute)
        with torch.cuda.stream(staging):
            torch.zeros(16, device=DEV)
            filled.record(staging)
        filled.synchronize()
        apart = not spun.query()
        compute.synchronize()
        if apart:
            return staging, compute
    pytest.fail("no stream of the pool runs side by side with the compute stream")


def busy_then_zero_fills(nbytes, count=16, folds=200):
    """Queue ~tens of ms of folds on the current stream, then ``count`` blocks of ``nbytes`` (an int or
    a list of sizes, ``count`` of each) zero-filled behind them, and free the blocks (their fills still
    queued)."""
    from fedn_amd import ops
    P = 50_000_000
    ups = [torch.ones(P, device=DEV) for _ in range(8)]
    agg = torch.empty(P, device=DEV)
    for _ in range(folds):
        ops.fedavg_fold(agg, ups, [1] * 8, list(range(1, 9)), init=True)
    sizes = nbytes if isinstance(nbytes, (list, tuple)) else [nbytes]
    blocks = [torch.empty(nb, dtype=torch.uint8, device=DEV) for nb in sizes for _ in range(count)]
    for b in blocks:
        b.zero_()
    del blocks
    return ups, agg                      # kept until the test ends: their folds are still queued too


def require_side_by_side(side, busy, cycles=SPIN_CYCLES, what="the copy stream"):
    """Precondition (a) of a late-launch test — a condition, not a measurement: a marker op on ``side``
    completes while ``busy`` still spins. Returns the spin's length in ms (HIP events)."""
    t0, spun, marked = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), torch.cuda.Event()
    with torch.cuda.stream(busy):
        t0.record(busy)
        torch.cuda._sleep(cycles)
        spun.record(busy)
    with torch.cuda.stream(side):
        torch.zeros(16, device=DEV)
        marked.record(side)
    marked.synchronize()
    ahead = not spun.query()
    busy.synchronize()
    if not ahead:
        pytest.fail(f"precondition (a): {what} does not run ahead of the spinning stream: they share a queue")
    return t0.elapsed_time(spun)


@contextlib.contextmanager
def poison_knob():
    """FEDN_AMD_POISON_REUSE on for the block (fedn_amd/reuse.py): drained before and after, the old
    state restored."""
    from fedn_amd import reuse
    was = reuse.enabled()
    reuse.set_enabled(True)
    reuse.drain()
    try:
        yield reuse
    finally:
        reuse.drain()
        reuse.set_enabled(was)


class LateLaunches:
    """Patches the four entry points the robust pipeline launches through (``fedn_amd.ops``): each call
    first queues a spin of ``cycles`` on the launch's stream, then calls the real function, then records
    an event behind it. ``calls`` keeps, per launch, its walk (``begin_walk``), whether the event behind
    the launch before it had completed when the host entered this one, and the host's clock.

    ``fail_at = i``: the i-th launch (from 0) raises ``FedAggError`` instead — injected at the wrapper,
    no device fault — while the launches before it are still queued (``pending_at_failure`` of them)."""

    def __init__(self, cycles=SPIN_CYCLES, fail_at=None):
        self.cycles, self.fail_at = cycles, fail_at
        self.calls, self.walk, self.failed, self.pending_at_failure = [], 0, 0, None

    def begin_walk(self):
        self.walk += 1

    @contextlib.contextmanager
    def patched(self, monkeypatch):
        from fedn_amd import ops
        with monkeypatch.context() as mp:
            for name in LATE_OPS:
                mp.setattr(ops, name, self._late(name, getattr(ops, name)))
            yield self

    def _late(self, name, real):
        sig = inspect.signature(real)

        def late(*a, **kw):
            from fedn_amd import _abi
            entered = time.perf_counter()
            stream = sig.bind(*a, **kw).arguments.get("stream")
            if stream is None:
                stream = torch.cuda.current_stream(DEV)
            prev_done = self.calls[-1]["after"].query() if self.calls else None
            if self.fail_at is not None and len(self.calls) == self.fail_at:
                self.failed += 1
                self.pending_at_failure = sum(not c["after"].query() for c in self.calls)
                raise _abi.FedAggError(_abi.FA_EHIP, f"{name}: injected failure at launch {self.fail_at}")
            with torch.cuda.stream(stream):
                torch.cuda._sleep(self.cycles)
            got = real(*a, **kw)
            after = torch.cuda.Event()
            after.record(stream)
            self.calls.append({"name": name, "walk": self.walk, "after": after, "prev_done": prev_done,
                               "entered": entered})
            return got

        return late

    def require_late(self, spin_ms, what, sliced=True):
        """Precondition (b) — a condition, not a measurement: for every launch after the first of a walk
        with several launches, the launch before it had not completed when the host entered the
        wrapper. Prints the spin (measured by the caller with events) and the host's time per slice."""
        walks = {}
        for c in self.calls:
            walks.setdefault(c["walk"], []).append(c)
        later, early, gaps = 0, [], []
        for w, calls in walks.items():
            for i, c in enumerate(calls[1:], 1):
                later += 1
                gaps.append(c["entered"] - calls[i - 1]["entered"])
                if c["prev_done"] is not False:
                    early.append((w, i))
        host_ms = 1e3 * max(gaps) if gaps else 0.0
        mean_ms = 1e3 * sum(gaps) / len(gaps) if gaps else 0.0
        print(f"{what}: {len(self.calls)} late launches in {len(walks)} walks, spin {spin_ms:.2f} ms, "
              f"host per slice {mean_ms:.3f} ms (longest {host_ms:.3f} ms)")
        if not self.calls:
            pytest.fail(f"{what}: no launch went through the late wrappers")
        if sliced and not later:
            pytest.fail(f"{what}: no walk was sliced: the ring was not exercised")
        if early:
            pytest.fail(f"precondition (b): {what}: the launch before had already completed at (walk, slice) "
                        f"{early[:6]} of {later}: the spin ({spin_ms:.2f} ms) does not outlast the host's "
                        f"work per slice (longest {host_ms:.3f} ms)")


def late_pipeline(copy, late=None):
    """A ``robust.RobustPipeline`` whose private copy stream is ``copy`` (chosen by looking:
    :func:`side_by_side_streams`) from the moment the pipeline sets it, and which tells ``late`` where
    each walk over a dtype group begins. The product class is not edited: the subclass swaps the value
    the constructor assigns."""
    from fedn_amd import robust

    class LatePipeline(robust.RobustPipeline):
        def __setattr__(self, name, value):
            object.__setattr__(self, name, copy if name == "copy" and copy is not None else value)

        def _walk_group(self, *a, **kw):
            if late is not None:
                late.begin_walk()
            return super()._walk_group(*a, **kw)

    return LatePipeline
