"""The robust pipeline's stream order (fedn_amd/robust.py) under LATE LAUNCHES and buffer reuse.

The plug-ins' own budget tests drive the ring with an idle compute stream: every launch has finished long
before the host refills its buffer, so a missing ``copy.wait_event(consumed[b])``, a ring freed without
``record_stream`` or a missing closing synchronise would pass by timing. Here every launch of the
pipeline is delayed by a device spin on the compute stream (tests/late_streams.py) and the pipeline's
copy stream is one that really runs beside it, so the host and the copy stream run ahead of every kernel:
a refill that does not wait lands under a launch that still reads the buffer, a ring freed early is
handed out again (and, with FEDN_AMD_POISON_REUSE on, filled with NaN) while launches are queued, and
pinned results read without the closing synchronise are not there yet. Both preconditions are asserted
in every late test: (a) the copy stream runs ahead of the spinning compute stream, (b) inside a sliced
walk the launch before had not completed when the host entered the next one.

Expected values are the oracles' (robust_ref, krum_ref, geomed_ref, cclip_ref); the late round's bits
are also those of an undelayed round."""
import functools
import gc
import types

import numpy as np
import pytest
import torch

import krum_ref as kr
import robust_ref as rr
from golden_io import assert_lists_identical
from late_streams import (DEV, LATE_OPS, SPIN_CYCLES, LateLaunches, busy_then_zero_fills, late_pipeline, poison_knob,
                          require_side_by_side, side_by_side_streams)
from robust_checks import check_cclip_chain, check_geomed_chain, same_bits
from test_gpu_cclip import _round_updates as _cclip_updates
from test_gpu_cclip import _tau
from test_gpu_krum import _round_updates, _selection

pytestmark = pytest.mark.gpu

K = 6
# three dtype groups; the f32 group's tensors straddle the slice bounds
SPEC = [((300, 200), np.float32), ((77,), np.int64), ((1001,), np.float32), ((), np.float32), ((513,), np.float16)]
SLICE = 16384            # robust.SLICE_BYTES here: the f32 group (61002 elements) takes 15 slices of 4096
HOST_SIDE = 4            # a budget of two updates: two sit in HBM, four go through the ring
FRACTION, NU, ITERATIONS = 0.2, 1e-6, 3
PLUGIN = {"trimmedmean": "trimmed", "median": "trimmed", "krum": "krum", "multikrum": "krum", "geomedian": "geomed",
          "centeredclip": "cclip"}


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
    """The round's data and everything the oracles say about it that does not depend on the device's
    own coefficients: computed once, read only."""
    from fedn_amd.layout import Layout
    c = types.SimpleNamespace()
    c.ups, c.hostile = _round_updates(0, K, SPEC)
    c.cups, _, c.center = _cclip_updates(0, K, SPEC)
    c.center64 = [a.astype(np.float64) if a.dtype.kind == "i" else a for a in c.center]
    c.tau = _tau(SPEC)
    c.f = kr.byzantine_count(FRACTION, K)
    c.trims = sorted({0, 1, rr.median_trim(K)})
    c.trim = {t: rr.combine(c.ups, t) for t in c.trims}
    c.ms = [1, K - c.f]
    c.sel = {m: _selection(c.ups, m, f"m={m}")[1] for m in c.ms}
    assert c.sel == {m: kr.select(kr.model_distances(c.ups).tolist(), c.f, m) for m in c.ms}
    c.krum = {m: kr.combine(c.ups, c.sel[m]) for m in c.ms}
    c.layout = Layout.of(c.ups[0])
    return c


def _updates(rule):
    return _case().cups if rule == "cclip" else _case().ups


def _budget(budgeted):
    from fedn_amd.budget import HbmBudget
    return HbmBudget(limit=(K - HOST_SIDE if budgeted else K) * _case().layout.nbytes)


def _pipeline(rule, copy, late, budget):
    ups = _updates(rule)
    pipe = late_pipeline(copy, late)(DEV, ups[0], tag=0, budget=budget)
    for k, u in enumerate(ups[1:], 1):
        pipe.add(u, tag=k)
    assert copy is None or pipe.copy is copy
    return pipe


@pytest.fixture(scope="module", autouse=True)
def _warm():
    """One undelayed budgeted round of every rule before the first late one: the kernels' code objects are
    loaded and the pools hold their first blocks, so no launch of a late round pays a first-use cost of
    milliseconds on the host — precondition (b) compares the spin with the host's steady work per slice."""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from fedn_amd import _abi, robust
    _abi.load()
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(robust, "SLICE_BYTES", SLICE)
        for rule in ("trimmed", "krum", "geomed", "cclip"):
            pipe = _pipeline(rule, None, None, _budget(True))
            _check_oracle(rule, *_reduce(pipe, rule), f"{rule}, undelayed")
            pipe.release()
        # Bulyan's window kernel (test_ops_on_a_late_side_stream; its late rounds are test_gpu_bulyan_streams.py's):
        # at K = 6 its f is 0, the window is every value and the model the plain mean
        pipe = _pipeline("trimmed", None, None, _budget(True))
        assert_lists_identical(pipe.bulyan(0), _case().trim[0], "bulyan at f = 0, undelayed")
        pipe.release()
    torch.cuda.synchronize()


def _scrub_pinned():
    """Pinned blocks of the sizes the results take, filled with 0xFF and returned to torch's host pool: a
    result read before its D2H landed shows as NaN / -1, not as an earlier round's (equal) bits."""
    c = _case()
    sizes = {c.layout.group_elems[dt] * rr.out_dtype(dt).itemsize for dt in c.layout.groups}
    blocks = [torch.empty(n, dtype=torch.uint8, pin_memory=True) for n in sizes for _ in range(4)]
    for b in blocks:
        b.fill_(0xFF)
    del blocks


def _reduce(pipe, rule, center="native"):
    """The rule on ``pipe``: ``(models, state)`` — the models by trim / by m / [the one], and what the
    pipeline keeps of the round (the chain checks read it as they read a plug-in)."""
    c = _case()
    _scrub_pinned()
    state = types.SimpleNamespace(selected={})
    if rule == "trimmed":
        models = {t: pipe.result(t) for t in c.trims}
    elif rule == "krum":
        models = {}
        for m in c.ms:
            models[m] = pipe.select_mean(c.f, m)
            state.selected[m] = list(pipe.selected)
    elif rule == "geomed":
        models = {0: pipe.geometric_median(ITERATIONS, NU)}
        state.weights = pipe.weights
    else:
        models = {0: pipe.centered_clip(c.center64 if center == "f64" else c.center, ITERATIONS, c.tau)}
        state.coefficients = pipe.coefficients
    state.trace, state.excluded, state.distances = list(pipe.trace), list(pipe.excluded), pipe.distances
    return models, state


def _check_oracle(rule, models, state, what, center="native"):
    c = _case()
    if rule == "trimmed":
        for t in c.trims:
            assert_lists_identical(models[t], c.trim[t], f"{what}: trim {t}")
    elif rule == "krum":
        for m in c.ms:
            assert state.selected[m] == c.sel[m], f"{what}: m={m}: selected {state.selected[m]}, the oracle {c.sel[m]}"
            assert_lists_identical(models[m], c.krum[m], f"{what}: m={m}")
    elif rule == "geomed":
        check_geomed_chain(c.ups, state, models[0], ITERATIONS, NU, what)
    else:
        check_cclip_chain(c.cups, c.center64 if center == "f64" else c.center, state, models[0], ITERATIONS, c.tau, what)


def _check_same_bits(rule, late, plain, what):
    """The kernels promise the same bits for the same inputs: a late round is an undelayed round."""
    (lm, ls), (pm, ps) = late, plain
    assert lm.keys() == pm.keys()
    for key in lm:
        assert_lists_identical(lm[key], pm[key], f"{what}: late vs undelayed, {key}")
    assert ls.selected == ps.selected
    assert len(ls.trace) == len(ps.trace)
    for t, ((lc, ld), (pc, pd)) in enumerate(zip(ls.trace, ps.trace)):
        same_bits(np.asarray(lc), np.asarray(pc), f"{what}: late vs undelayed, coefficients of pass {t}")
        same_bits(np.asarray(ld), np.asarray(pd), f"{what}: late vs undelayed, d of pass {t}")


def _no_nan(models, what):
    for key, model in models.items():
        for i, a in enumerate(model):
            assert not np.isnan(a).any(), f"{what}: NaN in tensor {i} of model {key}: poison reached the result"


def _collected(budget, what):
    gc.collect()
    assert budget.used(DEV) == 0, f"{what}: the round's reservations went back to the budget"


# ---- late rounds at pipeline level -----------------------------------------------------------------
CASES = [("trimmed", "native"), ("krum", "native"), ("geomed", "native"), ("cclip", "native"), ("cclip", "f64")]


@pytest.mark.parametrize("rule,center", CASES, ids=[r if c == "native" else f"{r}-{c}-centre" for r, c in CASES])
def test_late_round_through_the_ring(rule, center, monkeypatch):
    """Four of six updates on the host, every launch late, the poison knob on: ~15 slices of the f32
    group refill both ring buffers many times while the launches that read them are still queued."""
    what = f"{rule} through the ring"
    copy, compute = side_by_side_streams()
    with torch.cuda.stream(compute), poison_knob() as reuse:
        spin_ms = require_side_by_side(copy, compute)
        watched = reuse.stats()["watched"]
        late, budget = LateLaunches(), _budget(True)
        with late.patched(monkeypatch):
            pipe = _pipeline(rule, copy, late, budget)
            assert pipe.host_side == HOST_SIDE
            got = _reduce(pipe, rule, center)
        late.require_late(spin_ms, what)
        reuse.drain()
        assert reuse.stats()["watched"] > watched, "the staged updates and the ring are watched"
        _no_nan(got[0], what)
        _check_oracle(rule, *got, what, center)
        pipe.release()
        del pipe
        _collected(budget, what)
        plain_budget = _budget(True)
        plain = _pipeline(rule, copy, None, plain_budget)
        _check_same_bits(rule, got, _reduce(plain, rule, center), what)
        plain.release()
        del plain
        _collected(plain_budget, what)


@pytest.mark.parametrize("rule,center", CASES, ids=[r if c == "native" else f"{r}-{c}-centre" for r, c in CASES])
def test_late_round_in_hbm(rule, center, monkeypatch):
    """Every update in HBM: one late launch per dtype group, so the results reach the pinned host buffers
    only once the spins are over — the closing synchronise of ``result`` and ``select_mean`` and the D2H
    behind the launches are what the host's read relies on. (The two iterated rules launch once per slice
    of a group here too, on the updates in place, and end their last pass with a synchronising read of d:
    their closing synchronise finds the stream drained but for the centre's D2H.)"""
    what = f"{rule} in HBM"
    copy, compute = side_by_side_streams()
    with torch.cuda.stream(compute):
        spin_ms = require_side_by_side(copy, compute)
        late, budget = LateLaunches(), _budget(False)
        with late.patched(monkeypatch):
            pipe = _pipeline(rule, copy, late, budget)
            assert pipe.host_side == 0
            got = _reduce(pipe, rule, center)
        late.require_late(spin_ms, what, sliced=False)
        assert {c["name"] for c in late.calls} <= set(LATE_OPS)
        _check_oracle(rule, *got, what, center)
        plain = _pipeline(rule, copy, None, _budget(False))
        _check_same_bits(rule, got, _reduce(plain, rule, center), what)


def test_copy_stream_late_instead():
    """The other way round: the copy stream is late (a spin queued on it ahead of the first refill) and the
    launches are on time. A launch that did not wait for its slice's H2D would read an empty ring."""
    what = "late copy stream"
    copy, compute = side_by_side_streams()
    with torch.cuda.stream(compute), poison_knob():
        require_side_by_side(compute, copy, what="the compute stream")
        pipe = _pipeline("trimmed", copy, None, _budget(True))
        with torch.cuda.stream(copy):
            torch.cuda._sleep(SPIN_CYCLES)
        model = pipe.result(1)
        assert_lists_identical(model, _case().trim[1], what)
        with torch.cuda.stream(copy):
            torch.cuda._sleep(SPIN_CYCLES)
        model = pipe.geometric_median(1, NU)
        check_geomed_chain(_case().ups, pipe, model, 1, NU, what)


# ---- late plug-in rounds ----------------------------------------------------------------------------
def _run_round(agg_name, budget, agg=None, uh=None):
    from fedn_amd.aggregators import get_aggregator
    from fedn_amd.updatehandler import MemoryUpdateHandler
    c = _case()
    rule = PLUGIN[agg_name]
    uh = uh or MemoryUpdateHandler()
    gid = uh.put_global_model(c.center) if rule == "cclip" else "global"
    if agg is None:
        agg = get_aggregator(agg_name, uh)
        agg.device, agg.hbm_budget = torch.device(DEV), budget
    parameters = {"trimmed": {"trim_fraction": 0.2} if agg_name == "trimmedmean" else None,
                  "krum": {"byzantine_fraction": FRACTION},
                  "geomed": {"iterations": ITERATIONS, "nu": NU},
                  "cclip": {"iterations": ITERATIONS, "tau": c.tau}}[rule]
    mus = [uh.submit(u, 10 + k, model_id=gid) for k, u in enumerate(_updates(rule))]
    model, data = agg.combine_models(helper=None, parameters=parameters)
    return model, data, uh, mus, agg, gid


def _check_plugin(agg_name, agg, model, what):
    from fedn_amd.robust import trim_count
    c = _case()
    rule = PLUGIN[agg_name]
    if rule == "trimmed":
        t = rr.median_trim(K) if agg_name == "median" else trim_count(0.2, K)
        assert t in c.trims
        assert_lists_identical(model, c.trim[t], what)
    elif rule == "krum":
        m = 1 if agg_name == "krum" else K - c.f
        assert agg.selected == c.sel[m], f"{what}: selected {agg.selected}, the oracle {c.sel[m]}"
        assert_lists_identical(model, c.krum[m], what)
    elif rule == "geomed":
        check_geomed_chain(c.ups, agg, model, ITERATIONS, NU, what)
    else:
        check_cclip_chain(c.cups, c.center, agg, model, ITERATIONS, c.tau, what)


@pytest.mark.parametrize("agg_name", list(PLUGIN))
def test_late_plugin_round(agg_name, monkeypatch):
    """One budgeted round of each plug-in on the late pipeline, the poison knob on."""
    from fedn_amd.aggregators import trimmedmean
    what = f"{agg_name} plug-in, late"
    copy, compute = side_by_side_streams()
    with torch.cuda.stream(compute), poison_knob() as reuse:
        spin_ms = require_side_by_side(copy, compute)
        watched = reuse.stats()["watched"]
        late, budget = LateLaunches(), _budget(True)
        monkeypatch.setattr(trimmedmean, "RobustPipeline", late_pipeline(copy, late))
        with late.patched(monkeypatch):
            model, data, uh, _, agg, gid = _run_round(agg_name, budget)
        late.require_late(spin_ms, what)
        assert agg.host_side == HOST_SIDE and data["nr_aggregated_models"] == K
        reuse.drain()
        assert reuse.stats()["watched"] > watched
        _no_nan({0: model}, what)
        _check_plugin(agg_name, agg, model, what)
        assert set(uh.store.models) <= {gid}, "every update is deleted once the result exists"
        _collected(budget, what)


@pytest.mark.parametrize("agg_name", ["median", "multikrum", "geomedian", "centeredclip"])
def test_failed_launch_at_a_later_slice(agg_name, monkeypatch):
    """The injected ``FedAggError`` is raised at the third launch of the sliced f32 walk, under late
    launches with the knob on, while the launches before it are still queued on the ring: the round is
    ``(None, data)``, every update stays in storage, the budget is returned, and the same aggregator's
    next round — late as well — is exact against the oracle."""
    from fedn_amd.aggregators import trimmedmean
    what = f"{agg_name}, a launch failing at slice 2"
    copy, compute = side_by_side_streams()
    with torch.cuda.stream(compute), poison_knob():
        spin_ms = require_side_by_side(copy, compute)
        late, budget = LateLaunches(fail_at=2), _budget(True)
        monkeypatch.setattr(trimmedmean, "RobustPipeline", late_pipeline(copy, late))
        with late.patched(monkeypatch):
            model, data, uh, mus, agg, gid = _run_round(agg_name, budget)
            assert late.failed == 1 and len(late.calls) == 2 and late.walk == 1, "the third launch of the first walk"
            print(f"{what}: {late.pending_at_failure} of 2 launches were still queued when the third failed")
            if late.pending_at_failure < 1:
                pytest.fail(f"precondition: {what}: no launch was still queued when the third failed")
            assert model is None and data["nr_aggregated_models"] == 0
            assert uh.model_updates.qsize() == 0
            assert set(uh.store.models) - {gid} == {mu.model_update_id for mu in mus}, "every update stays in storage"
            _collected(budget, what)
            late.fail_at = None
            model, data, uh, _, _, _ = _run_round(agg_name, budget, agg=agg, uh=uh)
        late.require_late(spin_ms, what)
        assert data["nr_aggregated_models"] == K
        _no_nan({0: model}, what)
        _check_plugin(agg_name, agg, model, f"{what}: the round after")
        _collected(budget, what)


# ---- fresh HBM: a buffer is allocated on the stream that first writes it ----------------------------
def _fresh_sizes():
    """Bytes of what a budgeted round allocates, by allocation."""
    from fedn_amd import robust
    c = _case()
    ring, outs, centre = [], [], []
    for dt in c.layout.groups:
        n = c.layout.group_elems[dt]
        step = min(n, max(robust.SLICE_ALIGN, SLICE // dt.itemsize // robust.SLICE_ALIGN * robust.SLICE_ALIGN))
        row = -(-step // robust.SLICE_ALIGN) * robust.SLICE_ALIGN
        nbuf = 2 if n > step else 1
        ring.append(nbuf * HOST_SIDE * row * dt.itemsize)          # nbuf x host-side updates x row x itemsize
        outs.append(step * rr.out_dtype(dt).itemsize)
        centre.append(n * rr.out_dtype(dt).itemsize)
    return {"ring": ("trimmed", ring), "staged": ("trimmed", [c.layout.nbytes]), "outs": ("trimmed", outs),
            "outs-of-the-mean": ("geomed", outs), "centre": ("cclip", centre), "dist": ("geomed", [K * 8]),
            "dist-of-the-clip": ("cclip", [K * 8]), "D": ("krum", [K * K * 8])}


FRESH = ["ring", "staged", "outs", "outs-of-the-mean", "centre", "dist", "dist-of-the-clip", "D"]
# with the ring in play a pass's first launch waits for the copy stream's first refill, and so for whatever
# is queued on that stream: the accumulators are also run with every update in HBM, where no launch does
IN_HBM = ["dist", "dist-of-the-clip", "D"]
FRESH_CASES = [(a, w, True) for a in FRESH for w in ("compute", "copy")] + [(a, "copy", False) for a in IN_HBM]


@pytest.mark.parametrize("alloc,where,budgeted", FRESH_CASES,
                         ids=[f"{a}-{w}" if b else f"{a}-{w}-in-hbm" for a, w, b in FRESH_CASES])
def test_fresh_hbm_after_queued_work(alloc, where, budgeted, monkeypatch):
    """As tests/test_gpu_stream_order.py: a long run of folds is queued on one of the pipeline's two
    streams, then zero-fills of blocks of exactly the size the pipeline allocates next, and the blocks are
    freed with their fills still queued. The late round that follows must give the oracle's model: a
    buffer taken from the other stream's pool than the one that first writes it would be zeroed under
    the round. (The poison knob stays off: its poisoner would take same-size blocks out of the very pool
    prepared here.)"""
    rule, sizes = _fresh_sizes()[alloc]
    what = f"fresh {alloc} after queued work on the {where} stream" + ("" if budgeted else ", every update in HBM")
    torch.cuda.synchronize()
    torch.cuda.empty_cache()             # no other free block of these sizes in the pool
    copy, compute = side_by_side_streams()
    with torch.cuda.stream(compute):
        spin_ms = require_side_by_side(copy, compute)
        late, pipe = LateLaunches(), None
        if alloc != "staged":                # (staging synchronises the copy stream: it comes first)
            pipe = _pipeline(rule, copy, late, _budget(budgeted))
        with torch.cuda.stream(copy if where == "copy" else compute):
            keep = busy_then_zero_fills(sorted(set(sizes)))
        with late.patched(monkeypatch):
            pipe = pipe or _pipeline(rule, copy, late, _budget(budgeted))
            assert pipe.host_side == (HOST_SIDE if budgeted else 0)
            got = _reduce(pipe, rule)
        late.require_late(spin_ms, what, sliced=budgeted)
        _check_oracle(rule, *got, what)
        torch.cuda.synchronize()
        del keep


# ---- ops level: stream= ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LATE_OPS)
def test_ops_on_a_late_side_stream(name):
    """Each of the five ops with ``stream=`` a side stream that spins first, against the same call on the
    current stream: the same bits; the outputs still hold their sentinel and the event behind the op is
    still pending when a marker on the current stream has completed (the op neither ran on nor waited for
    the current stream); and blocks of the op's scratch size (``fa_*_work``) churned on the current stream
    before the side stream is synchronised do not change the result (the scratch is the side stream's)."""
    from fedn_amd import _abi, ops
    lib = _abi.load()
    P = 65539
    rng = np.random.default_rng(LATE_OPS.index(name))
    side, cur = side_by_side_streams()
    with torch.cuda.stream(cur):
        require_side_by_side(cur, side, what="the current stream")
        ups = torch.from_numpy((rng.standard_normal(P) + 0.05 * rng.standard_normal((K, P))).astype(np.float32)).to(DEV)
        views = [ups[k] for k in range(K)]
        centre = torch.from_numpy(rng.standard_normal(P).astype(np.float32)).to(DEV)
        coef = rng.uniform(0.05, 1.0, K).tolist()

        def outputs():
            shapes = {"trimmed_mean": [(P, torch.float32)], "median_window_mean": [(P, torch.float32)],
                      "pairwise_sqdist": [(K * K, torch.float64)],
                      "weighted_mean_sqdist": [(P, torch.float32), (K, torch.float64)],
                      "centered_clip_step": [(P, torch.float32), (K, torch.float64)]}[name]
            return [torch.full((n,), -7.0, dtype=dt, device=DEV) for n, dt in shapes]

        def call(outs, stream):
            if name == "trimmed_mean":
                ops.trimmed_mean(outs[0], views, 1, stream=stream)
            elif name == "median_window_mean":
                ops.median_window_mean(outs[0], views, 4, stream=stream)
            elif name == "pairwise_sqdist":
                ops.pairwise_sqdist(views, out=outs[0].view(K, K), stream=stream)
            elif name == "weighted_mean_sqdist":
                ops.weighted_mean_sqdist(views, coef, out=outs[0], dist=outs[1], stream=stream)
            else:
                ops.centered_clip_step(views, centre, coef, out=outs[0], dist=outs[1], stream=stream)

        work = {"trimmed_mean": 0, "median_window_mean": 0, "pairwise_sqdist": int(lib.fa_pairwise_sqdist_work(K, P)),
                "weighted_mean_sqdist": int(lib.fa_wmean_sqdist_work(K, P)),
                "centered_clip_step": int(lib.fa_centered_clip_work(K, P))}[name]
        want = outputs()
        call(want, None)
        want = [t.cpu().numpy() for t in want]
        cur.synchronize()                                    # the inputs are there for any stream
        with torch.cuda.stream(side):
            got = outputs()
            filled = torch.cuda.Event()
            filled.record(side)
            torch.cuda._sleep(SPIN_CYCLES)
            call(got, side)
            after = torch.cuda.Event()
            after.record(side)
        cur.wait_event(filled)
        seen = [t.clone() for t in got]                      # on the current stream, while the side stream spins
        churn = [torch.full((max(1, work),), float("nan"), dtype=torch.float64, device=DEV) for _ in range(8)]
        del churn
        marker = torch.cuda.Event()
        marker.record(cur)
        marker.synchronize()
        pending = not after.query()
        side.synchronize()
        assert pending, f"{name}: the op on the side stream was over when the current stream's marker completed"
        for t in seen:
            assert bool((t == -7).all()), f"{name}: an output was written before the side stream's spin ended"
        print(f"{name}: scratch {work} float64 values")
        for i, (g, w) in enumerate(zip(got, want)):
            same_bits(g.cpu().numpy(), w, f"{name}: output {i} on the late side stream")
