"""Bulyan's stream order (``RobustPipeline.bulyan``, fedn_amd/robust.py) under LATE LAUNCHES and buffer
reuse, at K = 7 with f = 1 — the stream suite's round (tests/test_gpu_robust_streams.py) has K = 6, where
Bulyan's f is 0 and the rule is the plain mean.

Bulyan shares ``select_mean``'s frame, but its second pass is unlike its first: it walks only the
selected updates. With a budget of two updates FIFO 0 and 1 sit in HBM and 2..6 go through the ring; the
selection [0, 2, 3, 5, 6] drops one update of each side, so pass 1's ring has five rows and pass 2's has
four — a ring of another size, and new result blocks, allocated while pass 1's launches may still be
queued, behind a selection made on the host between the passes, with the selected host-side updates
uploaded a second time. Every launch (``pairwise_sqdist`` in pass 1, ``median_window_mean`` in pass 2) is
delayed by a device spin on the compute stream (tests/late_streams.py) and the copy stream is one that
really runs beside it. Both preconditions of the stream suite are asserted in every late test: (a) the
copy stream runs ahead of the spinning compute stream, (b) inside a sliced walk the launch before had
not completed when the host entered the next one.

Expected values are the oracle's (tests/bulyan_ref.py); a late round's bits are also those of an
undelayed round."""
import functools
import gc
import types

import numpy as np
import pytest
import torch

import bulyan_ref as br
from golden_io import assert_lists_identical
from late_streams import (DEV, LATE_OPS, SPIN_CYCLES, LateLaunches, busy_then_zero_fills, late_pipeline, poison_knob,
                          require_side_by_side, side_by_side_streams)
from robust_checks import same_bits
from test_gpu_bulyan import RING_SPEC as SPEC
from test_gpu_bulyan import _round_updates, _run_round, _selection

pytestmark = pytest.mark.gpu

K, F = 7, 1
SLICE = 16384            # robust.SLICE_BYTES here: the f32 group (61002 elements) takes 15 slices of 4096
HOST_SIDE = 5            # a budget of two updates: FIFO 0 and 1 sit in HBM, 2..6 go through the ring
FRACTION = 0.2           # the plug-in's byzantine_fraction: f = min(floor(0.2 * 7), (7 - 3) // 4) = 1
OPS = ("pairwise_sqdist", "median_window_mean")               # pass 1's launches, pass 2's


@pytest.fixture(autouse=True)
def _gpu(monkeypatch):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from fedn_amd import _abi, robust
    _abi.load()
    monkeypatch.setattr(robust, "SLICE_BYTES", SLICE)
    yield
    torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def _case():
    """The round's data and what the oracle says about it, computed once and read only. The preconditions
    of every test here are asserted on the oracle's output before any device work: the selection's score
    gaps, and at least one selected and one rejected update on each side of the budget."""
    from fedn_amd.layout import Layout
    c = types.SimpleNamespace()
    c.ups, c.hostile = _round_updates(0, K, F, SPEC)
    assert br.byzantine_count(FRACTION, K) == F
    c.selected, c.pick_order, c.scores = _selection(c.ups, F, "bulyan streams")
    c.model, again = br.combine(c.ups, F)
    assert again == c.selected and len(c.selected) == K - 2 * F
    c.rejected = sorted(set(range(K)) - set(c.selected))
    hbm = range(K - HOST_SIDE)
    print(f"bulyan streams: hostile {c.hostile}, selected {c.selected}, pick order {c.pick_order}, rejected {c.rejected}")
    assert any(k in hbm for k in c.selected) and any(k in hbm for k in c.rejected), "precondition: the HBM side"
    assert any(k not in hbm for k in c.selected) and any(k not in hbm for k in c.rejected), "precondition: the host side"
    c.rows = {1: HOST_SIDE, 2: sum(k not in hbm for k in c.selected)}       # the ring's rows, by pass
    assert c.rows[2] < c.rows[1]
    c.layout = Layout.of(c.ups[0])
    return c


def _budget(budgeted):
    from fedn_amd.budget import HbmBudget
    return HbmBudget(limit=(K - HOST_SIDE if budgeted else K) * _case().layout.nbytes)


def _pipeline(copy, late, budget):
    ups = _case().ups
    pipe = late_pipeline(copy, late)(DEV, ups[0], tag=0, budget=budget)
    for k, u in enumerate(ups[1:], 1):
        pipe.add(u, tag=k)
    assert copy is None or pipe.copy is copy
    return pipe


def _scrub_pinned():
    """Pinned blocks of the sizes the results take, filled with 0xFF and returned to torch's host pool: a
    result read before its D2H landed shows as NaN / -1, not as an earlier round's (equal) bits."""
    c = _case()
    sizes = {c.layout.group_elems[dt] * br.rr.out_dtype(dt).itemsize for dt in c.layout.groups}
    blocks = [torch.empty(n, dtype=torch.uint8, pin_memory=True) for n in sizes for _ in range(4)]
    for b in blocks:
        b.fill_(0xFF)
    del blocks


def _reduce(pipe):
    """``(model, state)``: the round, and what the pipeline keeps of it."""
    _scrub_pinned()
    model = pipe.bulyan(F)
    return model, types.SimpleNamespace(selected=list(pipe.selected), pick_order=list(pipe.pick_order),
                                        scores=np.asarray(pipe.scores, dtype=np.float64))


def _check_oracle(model, state, what):
    c = _case()
    assert state.selected == c.selected, f"{what}: selected {state.selected}, the oracle {c.selected}"
    assert state.pick_order == c.pick_order, f"{what}: pick order {state.pick_order}, the oracle {c.pick_order}"
    assert_lists_identical(model, c.model, what)


def _check_same_bits(late, plain, what):
    """The kernels promise the same bits for the same inputs: a late round is an undelayed round."""
    (lm, ls), (pm, ps) = late, plain
    assert_lists_identical(lm, pm, f"{what}: late vs undelayed")
    assert ls.selected == ps.selected and ls.pick_order == ps.pick_order
    same_bits(ls.scores, ps.scores, f"{what}: late vs undelayed, scores")


def _no_nan(model, what):
    for i, a in enumerate(model):
        assert not np.isnan(a).any(), f"{what}: NaN in tensor {i}: poison reached the result"


def _collected(budget, what):
    gc.collect()
    assert budget.used(DEV) == 0, f"{what}: the round's reservations went back to the budget"


def _by_walk(calls, op):
    """{walk: [indices into ``calls``]} of the launches of ``op``."""
    walks = {}
    for i, c in enumerate(calls):
        if c["name"] == op:
            walks.setdefault(c["walk"], []).append(i)
    return walks


@pytest.fixture(scope="module", autouse=True)
def _warm():
    """One undelayed budgeted round before the first late one: the kernels' code objects are loaded
    (``k_median_window``'s is the largest of the library) and the pools hold their first blocks, so no launch
    of a late round pays a first-use cost of milliseconds on the host — precondition (b) compares the spin
    with the host's steady work per slice."""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from fedn_amd import _abi, robust
    _abi.load()
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(robust, "SLICE_BYTES", SLICE)
        for budgeted in (True, False):
            pipe = _pipeline(None, None, _budget(budgeted))
            assert pipe.host_side == (HOST_SIDE if budgeted else 0)
            _check_oracle(*_reduce(pipe), "undelayed")
            pipe.release()
    torch.cuda.synchronize()


# ---- late rounds at pipeline level -----------------------------------------------------------------
def test_late_round_through_the_ring(monkeypatch):
    """Five of seven updates on the host, every launch late, the poison knob on: both passes refill both
    ring buffers many times while the launches that read them are still queued, and pass 2's ring (four
    rows) and result blocks are allocated behind pass 1's."""
    what = "bulyan through the ring"
    _case()
    copy, compute = side_by_side_streams()
    with torch.cuda.stream(compute), poison_knob() as reuse:
        spin_ms = require_side_by_side(copy, compute)
        watched = reuse.stats()["watched"]
        late, budget = LateLaunches(), _budget(True)
        with late.patched(monkeypatch):
            pipe = _pipeline(copy, late, budget)
            assert pipe.host_side == HOST_SIDE
            got = _reduce(pipe)
        late.require_late(spin_ms, what)
        assert {c["name"] for c in late.calls} == set(OPS)
        for op in OPS:
            assert max(len(w) for w in _by_walk(late.calls, op).values()) > 1, f"{what}: no walk of {op} was sliced"
        reuse.drain()
        assert reuse.stats()["watched"] > watched, "the staged updates and the rings are watched"
        _no_nan(got[0], what)
        _check_oracle(*got, what)
        pipe.release()
        del pipe
        _collected(budget, what)
        plain_budget = _budget(True)
        plain = _pipeline(copy, None, plain_budget)
        assert plain.host_side == HOST_SIDE
        _check_same_bits(got, _reduce(plain), what)
        plain.release()
        del plain
        _collected(plain_budget, what)


def test_late_round_in_hbm(monkeypatch):
    """Every update in HBM: one late launch per dtype group and pass, so the model reaches the pinned host
    buffers (scrubbed with 0xFF first) only once the spins are over — the closing synchronise and the D2H
    behind the launches are what the host's read relies on."""
    what = "bulyan in HBM"
    copy, compute = side_by_side_streams()
    with torch.cuda.stream(compute):
        spin_ms = require_side_by_side(copy, compute)
        late = LateLaunches()
        with late.patched(monkeypatch):
            pipe = _pipeline(copy, late, _budget(False))
            assert pipe.host_side == 0
            got = _reduce(pipe)
        late.require_late(spin_ms, what, sliced=False)
        assert {c["name"] for c in late.calls} == set(OPS) <= set(LATE_OPS)
        _check_oracle(*got, what)
        plain = _pipeline(copy, None, _budget(False))
        _check_same_bits(got, _reduce(plain), what)


def test_copy_stream_late_instead():
    """The other way round: the copy stream is late (a spin queued on it ahead of the first refill) and the
    launches are on time. A launch that did not wait for its slice's H2D would read an empty ring. A second
    round on the same pipeline behind a second spin: its refills are late in both passes again."""
    what = "late copy stream"
    copy, compute = side_by_side_streams()
    with torch.cuda.stream(compute), poison_knob():
        require_side_by_side(compute, copy, what="the compute stream")
        pipe = _pipeline(copy, None, _budget(True))
        assert pipe.host_side == HOST_SIDE
        for turn in ("first round", "second round"):
            with torch.cuda.stream(copy):
                torch.cuda._sleep(SPIN_CYCLES)
            _check_oracle(*_reduce(pipe), f"{what}, {turn}")


# ---- late plug-in rounds ----------------------------------------------------------------------------
def _plugin_round(budget, agg=None, uh=None):
    return _run_round(_case().ups, {"byzantine_fraction": FRACTION}, budget=budget, agg=agg, uh=uh)


def _check_plugin(agg, model, data, what):
    c = _case()
    assert agg.host_side == HOST_SIDE and data["nr_aggregated_models"] == K
    assert agg.selected == c.selected and agg.pick_order == c.pick_order, (what, agg.selected, agg.pick_order)
    assert_lists_identical(model, c.model, what)


def test_late_plugin_round(monkeypatch):
    """One budgeted round of the plug-in on the late pipeline, the poison knob on. (bulyan.Aggregator
    inherits ``_combine`` from trimmedmean.Aggregator, which constructs its pipeline as
    ``trimmedmean.RobustPipeline``: that name is the one to patch.)"""
    from fedn_amd.aggregators import trimmedmean
    what = "bulyan plug-in, late"
    _case()
    copy, compute = side_by_side_streams()
    with torch.cuda.stream(compute), poison_knob() as reuse:
        spin_ms = require_side_by_side(copy, compute)
        watched = reuse.stats()["watched"]
        late, budget = LateLaunches(), _budget(True)
        monkeypatch.setattr(trimmedmean, "RobustPipeline", late_pipeline(copy, late))
        with late.patched(monkeypatch):
            model, data, uh, _, agg = _plugin_round(budget)
        late.require_late(spin_ms, what)
        assert {c["name"] for c in late.calls} == set(OPS)
        reuse.drain()
        assert reuse.stats()["watched"] > watched
        _no_nan(model, what)
        _check_plugin(agg, model, data, what)
        assert uh.model_updates.qsize() == 0 and not uh.store.models, "every update is deleted once the result exists"
        _collected(budget, what)


@pytest.mark.parametrize("where", ["distances", "window"])
def test_failed_launch_in_either_pass(where, monkeypatch):
    """The injected ``FedAggError`` is raised at the third launch of the first sliced walk of pass 1
    (``distances``) or of pass 2 (``window``: the pipeline already holds a selection when the round dies),
    under late launches with the knob on, while the launches before it are still queued on the ring: the
    round is ``(None, data)``, the aggregator shows no selection, every update stays in storage, the budget
    is returned, and the same aggregator's next round — late as well — is exact against the oracle. The
    failing launch's index comes from a counted round without a failure."""
    from fedn_amd.aggregators import trimmedmean
    op = OPS[0] if where == "distances" else OPS[1]
    what = f"bulyan, a launch failing at slice 2 of the {where} pass"
    _case()
    copy, compute = side_by_side_streams()
    with torch.cuda.stream(compute), poison_knob():
        spin_ms = require_side_by_side(copy, compute)
        late, budget = LateLaunches(), _budget(True)
        monkeypatch.setattr(trimmedmean, "RobustPipeline", late_pipeline(copy, late))
        with late.patched(monkeypatch):
            model, data, _, _, counted = _plugin_round(budget)
            late.require_late(spin_ms, f"{what}: the counted round")
            _check_plugin(counted, model, data, f"{what}: the counted round")
            n1 =sum(c["name"] == OPS[0] for c in late.calls)
            assert [c["name"] for c in late.calls[:n1]] == [OPS[0]] * n1, "pass 1's launches come first"
            fail_at = 2 if where == "distances" else n1 + 2
            walks = _by_walk(late.calls, op)
            sliced = [w for w in sorted(walks) if len(walks[w]) > 1]
            assert sliced and len(walks[sliced[0]]) >= 3 and walks[sliced[0]][2] == fail_at, \
                f"{what}: launch {fail_at} is not the third of the pass's first sliced walk: {walks}"
            assert not any(w < sliced[0] for w in walks), "the sliced dtype group is the pass's first"
            failing_walk, before = sliced[0], len(late.calls)
            del counted
            _collected(budget, what)

            late.calls, late.walk, late.fail_at = [], 0, fail_at
            model, data, uh, mus, agg = _plugin_round(budget)
            assert late.failed == 1 and len(late.calls) == fail_at and late.walk == failing_walk, \
                f"{what}: failed {late.failed} times after {len(late.calls)} launches in walk {late.walk}"
            assert [(c["name"], c["walk"]) for c in late.calls[-2:]] == [(op, failing_walk)] * 2
            print(f"{what}: launch {fail_at} of {before}: {late.pending_at_failure} launches were still queued")
            if late.pending_at_failure < 1:
                pytest.fail(f"precondition: {what}: no launch was still queued when the third failed")
            assert model is None and data["nr_aggregated_models"] == 0
            assert agg.selected is None and agg.pick_order is None and agg.scores is None
            assert uh.model_updates.qsize() == 0
            assert set(uh.store.models) == {mu.model_update_id for mu in mus}, "every update stays in storage"
            _collected(budget, what)
            late.fail_at = None
            model, data, uh, _, _ = _plugin_round(budget, agg=agg, uh=uh)
        late.require_late(spin_ms, what)
        _no_nan(model, what)
        _check_plugin(agg, model, data, f"{what}: the round after")
        assert set(uh.store.models) == {mu.model_update_id for mu in mus}, "the round after deletes its own updates"
        _collected(budget, what)


# ---- fresh HBM: a buffer is allocated on the stream that first writes it ----------------------------
def _fresh_sizes():
    """Bytes of what pass 2 of a budgeted round allocates, and of D, by allocation."""
    from fedn_amd import robust
    c = _case()
    ring, outs = [], []
    for dt in c.layout.groups:
        n = c.layout.group_elems[dt]
        step = min(n, max(robust.SLICE_ALIGN, SLICE // dt.itemsize // robust.SLICE_ALIGN * robust.SLICE_ALIGN))
        row = -(-step // robust.SLICE_ALIGN) * robust.SLICE_ALIGN
        nbuf = 2 if n > step else 1
        ring.append(nbuf * c.rows[2] * row * dt.itemsize)          # nbuf x selected host-side updates x row x itemsize
        outs.append(step * br.rr.out_dtype(dt).itemsize)
    return {"pass-2-ring": ring, "pass-2-outs": outs, "D": [K * K * 8]}


# with the ring in play a pass's first launch waits for the copy stream's first refill, and so for whatever
# is queued on that stream: D is also run with every update in HBM, where no launch does
FRESH_CASES = [(a, w, True) for a in ("pass-2-ring", "pass-2-outs", "D") for w in ("compute", "copy")]
FRESH_CASES.append(("D", "copy", False))


@pytest.mark.parametrize("alloc,where,budgeted", FRESH_CASES,
                         ids=[f"{a}-{w}" if b else f"{a}-{w}-in-hbm" for a, w, b in FRESH_CASES])
def test_fresh_hbm_after_queued_work(alloc, where, budgeted, monkeypatch):
    """As the stream suite's: a long run of folds is queued on one of the pipeline's two streams, then
    zero-fills of blocks of exactly the size the pipeline allocates in pass 2 (the four-row ring, the
    result blocks) or for D, and the blocks are freed with their fills still queued. The late round that
    follows must give the oracle's model: a buffer taken from the other stream's pool than the one that
    first writes it would be zeroed under the round. (The poison knob stays off: its poisoner would take
    same-size blocks out of the very pool prepared here.)"""
    sizes = _fresh_sizes()[alloc]
    what = f"fresh {alloc} after queued work on the {where} stream" + ("" if budgeted else ", every update in HBM")
    torch.cuda.synchronize()
    torch.cuda.empty_cache()             # no other free block of these sizes in the pool
    copy, compute = side_by_side_streams()
    with torch.cuda.stream(compute):
        spin_ms = require_side_by_side(copy, compute)
        late = LateLaunches()
        pipe = _pipeline(copy, late, _budget(budgeted))
        assert pipe.host_side == (HOST_SIDE if budgeted else 0)
        with torch.cuda.stream(copy if where == "copy" else compute):
            keep = busy_then_zero_fills(sorted(set(sizes)))
        with late.patched(monkeypatch):
            got = _reduce(pipe)
        late.require_late(spin_ms, what, sliced=budgeted)
        _check_oracle(*got, what)
        torch.cuda.synchronize()
        del keep
