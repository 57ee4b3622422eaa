"""The round protocol (fedn_amd/roundcore.py) on the host alone: no GPU, no native library.

A fake round stands in for the pipelines. Its state is two CPU tensors (two dtype groups, so a
fold is two launches); a launch over a batch adds the batch's values to one group and is
recorded; an update in ``bad`` makes every launch of group ``fail_group`` that holds it raise
FedAggError, as a failing status would. ``add`` and ``result`` are shaped like the pipelines':
batches of staging.BATCH flushed by add, the last one folded by result behind a snapshot and
recovered through ``_recover``. K = 5 updates with BATCH = 3: one batch flushed, one left to result.
"""
import contextlib

import pytest
import torch

from fedn_amd import _abi, ops, roundcore, staging

K = 5
TAGS = [f"u{k}" for k in range(K)]
VALUES = [float(1 << k) for k in range(K)]      # distinct powers of two: a sum names its updates


@pytest.fixture(autouse=True)
def _host_only(monkeypatch):
    """The helpers select a device and a stream per part; on the host there is neither."""
    monkeypatch.setattr(torch.cuda, "device", lambda dv: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "stream", lambda st: contextlib.nullcontext())
    monkeypatch.setattr(staging, "BATCH", 3)


class FakeRound(roundcore.Round):
    def __init__(self, bad=(), fail_group="b", crash=()):
        super().__init__()
        self.bad, self.fail_group, self.crash = set(bad), fail_group, set(crash)
        self.state = {"a": torch.zeros(4), "b": torch.zeros(4)}
        self.started = False
        self.launched = []                       # (group, tags of the batch) per launch that ran
        self.uploads = 0

    # what the protocol asks of a pipeline
    def _started(self):
        return self.started

    def _folded(self):
        self.started = True

    def _state_parts(self):
        return [(None, None, self.state)]

    def _nlaunch(self):
        return len(self.state)

    def _before_flush(self):
        self.uploads += 1

    def _launches(self, entries):
        init = not self.started
        for g in self.state:
            tags = tuple(e[3] for e in entries)
            if self.crash.intersection(tags):
                raise ValueError("not a launch status")
            if g == self.fail_group and self.bad.intersection(tags):
                raise _abi.FedAggError(_abi.FA_EHIP, f"injected failure of group {g} over {tags}")
            total = sum(e[0] for e in entries)
            if init:                             # an init fold rewrites the state
                self.state[g].fill_(total)
            else:
                self.state[g] += total
            self.launched.append((g, tags))
            yield

    # the pipelines' shape of add() and result()
    def add(self, value, n, N, tag=None):
        self._check_broken()
        self.pending.append((value, n, N, tag))
        if len(self.pending) >= staging.BATCH:
            self._flush()
        self.nfolds += 1

    def result(self):
        self._check_broken()
        entries, self.pending = self.pending, []
        snap, ran = None, 0
        try:
            snap = self._snapshot(self._nlaunch()) if entries else None
            for _ in self._launches(entries):
                ran += 1
        except ops.FedAggError:
            self._recover(entries, snap, ran)
            entries = []
        if entries:
            self._folded()
        return {g: float(t[0]) for g, t in self.state.items()}


def _run(r, upto=K):
    for k in range(upto):
        r.add(VALUES[k], k + 1, (k + 1) * (k + 2) // 2, tag=TAGS[k])
    return r


def test_batches_fold_in_fifo_order_and_the_pending_one_is_unsettled():
    r = FakeRound()
    counts = []
    for k in range(K):
        r.add(VALUES[k], 1, k + 1, tag=TAGS[k])
        counts.append(r.unsettled())
    assert counts == [1, 2, 0, 1, 2], "unsettled() is the pending batch"
    assert r.launched == [("a", ("u0", "u1", "u2")), ("b", ("u0", "u1", "u2"))]
    assert r.uploads == 1, "the flush uploads what was admitted on the host first"
    assert r.result() == {"a": 31.0, "b": 31.0}
    assert r.launched[2:] == [("a", ("u3", "u4")), ("b", ("u3", "u4"))]
    assert r.take_skipped() == [] and r.unsettled() == 0 and r.broken is None


@pytest.mark.parametrize("bad", [["u1"], ["u4"], ["u0", "u3"], ["u2", "u4"], ["u0", "u1", "u2"]],
                         ids=lambda b: "bad_" + "_".join(b))
@pytest.mark.parametrize("fail_group", ["a", "b"])
def test_failed_batch_is_refolded_singly_and_only_the_failing_updates_are_skipped(bad, fail_group):
    """The second group failing leaves the first group's launch enqueued: the state must be put back
    before the updates fold one at a time, or the good ones land on a half-advanced state."""
    r = _run(FakeRound(bad=bad, fail_group=fail_group))
    got = r.result()
    want = sum(v for v, t in zip(VALUES, TAGS) if t not in bad)
    assert got == {"a": want, "b": want}, "only the failing updates are left out, from both groups"
    skipped = r.take_skipped()
    assert [t for t, _ in skipped] == bad, "skipped updates are reported with their tags, in FIFO order"
    assert all(isinstance(e, ops.FedAggError) for _, e in skipped)
    assert r.take_skipped() == [], "each skip is reported once"
    assert r.broken is None
    # every update of a failed batch was tried alone, in FIFO order, after the batch
    singles = [tags[0] for g, tags in r.launched if g == "a" and len(tags) == 1]
    first, last = TAGS[:3], TAGS[3:]
    tried = [t for batch in (first, last) if set(batch) & set(bad) for t in batch]
    if fail_group == "a":                        # a failing update's first launch never ran
        tried = [t for t in tried if t not in bad]
    assert singles == tried


def test_other_exception_out_of_a_flush_loses_the_round():
    r = FakeRound(crash=["u1"])
    with pytest.raises(ValueError, match="not a launch status"):
        _run(r, upto=3)
    assert isinstance(r.broken, ValueError)
    assert r.pending == [] and r.take_skipped() == []
    for call in (lambda: r.add(1.0, 1, 1, tag="late"), r.result):
        with pytest.raises(RuntimeError, match="could not be recovered"):
            call()


def _no_room(monkeypatch):
    asked = []

    def copy_aside(parts):
        asked.append(len(parts))
        return roundcore.NO_SNAPSHOT
    monkeypatch.setattr(roundcore, "copy_aside", copy_aside)
    return asked


def test_snapshot_that_cannot_be_taken_does_not_skip_a_valid_update(monkeypatch):
    asked = _no_room(monkeypatch)
    r = _run(FakeRound())
    assert r.result() == {"a": 31.0, "b": 31.0}
    assert asked == [1], "only the continuation fold of two launches asks for a copy"
    assert r.broken is None and r.take_skipped() == []


def test_no_snapshot_matters_only_on_a_part_way_failure(monkeypatch):
    asked = _no_room(monkeypatch)
    # the failing update's FIRST launch fails: nothing ran, nothing to put back, the round goes on
    r = _run(FakeRound(bad=["u4"], fail_group="a"))
    assert r.result() == {"a": 15.0, "b": 15.0}
    assert [t for t, _ in r.take_skipped()] == ["u4"] and r.broken is None and asked
    # its SECOND launch fails after the first advanced the state: that cannot be undone
    r = _run(FakeRound(bad=["u4"], fail_group="b"))
    with pytest.raises(RuntimeError, match="could not be copied aside"):
        r.result()
    assert isinstance(r.broken, RuntimeError)
    with pytest.raises(RuntimeError, match="could not be recovered"):
        r.result()
    # the same inside a flush (u3-u5 continue the state u0-u2 started)
    r = FakeRound(bad=["u4"], fail_group="b")
    _run(r)
    with pytest.raises(RuntimeError, match="could not be copied aside"):
        r.add(32.0, 1, 99, tag="u5")
    with pytest.raises(RuntimeError, match="could not be recovered"):
        r.add(64.0, 1, 100, tag="u6")


def test_put_back_copies_only_after_a_launch_ran():
    r = FakeRound()
    parts = r._state_parts()
    snap = roundcore.copy_aside(parts)
    assert snap[0]["a"] is not r.state["a"], "a copy, not a view"
    r.state["a"] += 5
    roundcore.put_back(r, parts, snap, ran=0)
    assert float(r.state["a"][0]) == 5.0, "no launch ran: nothing is copied"
    roundcore.put_back(r, parts, None, ran=2)
    assert float(r.state["a"][0]) == 5.0, "no snapshot was needed: nothing is copied"
    roundcore.put_back(r, parts, roundcore.NO_SNAPSHOT, ran=0)
    assert r.broken is None, "no launch ran: the missing snapshot does not matter"
    roundcore.put_back(r, parts, snap, ran=1)
    assert float(r.state["a"][0]) == 0.0 and float(r.state["b"][0]) == 0.0


def test_copy_aside_reports_a_full_device_as_no_snapshot():
    class Full:
        def clone(self):
            raise torch.cuda.OutOfMemoryError("injected: HBM full")
    assert roundcore.copy_aside([(None, None, {"a": torch.zeros(2)}), (None, None, {"a": Full()})]) \
        is roundcore.NO_SNAPSHOT
