"""Seeded random rounds through the seven robust plug-ins vs their oracles (tests/robust_ref.py,
krum_ref.py, bulyan_ref.py, geomed_ref.py, cclip_ref.py): the cases of tests/robust_fuzz_cases.py — random
layouts over five dtypes, K = 1-24 and the forced 1 / 2 / 3 / 4 / 33 / 64, random parameters, a random
``robust.SLICE_BYTES`` (1-16 slices of the largest dtype group, down to one SLICE_ALIGN per slice) and a
random HBM budget — each through three routes:

  host    updates submitted as arrays, the aggregator's budget admits the case's first j of them to HBM,
          the rest are walked slice by slice through the ring;
  staged  ``StagingUpdateHandler`` stages every update on arrival: one launch per dtype group;
  mixed   each update is staged on arrival or submitted as host arrays, as the case's bit vector says, and
          the aggregator's budget is 0: ``StagedModel``s and host updates interleaved in FIFO order (the
          handlers allow it: an update that did not arrive through the staging handler is loaded from the
          wrapped one).

Bars: the order statistics and the selected means bit for bit, selections equal (their precondition is the
case's, settled on the CPU), Bulyan's scores within ``_score_rtol``, the geometric median and centred
clipping by their pass-by-pass chains; every update counted and deleted, the budget returned. Extended
runs: FEDN_AMD_FUZZ_BASE / FEDN_AMD_FUZZ_SCALE as in tests/test_gpu_fuzz.py."""
import functools
import gc
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import bulyan_ref as br
import krum_ref as kr
import robust_checks
import robust_fuzz_cases as fc
import robust_ref as rr
from golden_io import assert_lists_identical
from test_gpu_bulyan import _score_rtol
from test_gpu_fuzz import _seeds

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROUTES = ["staged", "host", "mixed"]
SEEDS = _seeds(fc.DEFAULT_SEEDS)
_MODELS = {}                       # (rule, seed, route) -> the round's model, for test_routes_agree
_WORST = {"score": (0.0, 0.0), "cases": {}}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from fedn_amd import _abi
    _abi.load()
    yield
    torch.cuda.synchronize()
    _MODELS.clear()
    print(f"\nrobust fuzz: cases per (rule, route) {_WORST['cases']}; worst relative score error "
          f"{_WORST['score'][0]:.3e} (its bound {_WORST['score'][1]:.3e})")


@functools.lru_cache(maxsize=None)
def _case(rule, seed):
    """The case and what its oracle says, computed once for the three routes and read only."""
    c = fc.case(rule, seed)
    c.want = c.want_sel = c.want_order = c.want_scores = None
    if rule in ("trimmedmean", "median"):
        c.want = rr.combine(c.ups, c.trim)
    elif rule in ("krum", "multikrum"):
        c.want_sel = kr.select(c.D.tolist(), c.f, 1 if rule == "krum" else c.K - c.f)
        c.want = kr.combine(c.ups, c.want_sel)
    elif rule == "bulyan":
        c.want_sel, c.want_order, c.want_scores = br.select(c.D.tolist(), c.f)
        c.want, sel2 = br.combine(c.ups, c.f)
        assert sel2 == c.want_sel
    return c


def _run(c, route, monkeypatch, parameters=None):
    """One round of case ``c`` through ``route``: (model, data, update handler, aggregator, budget, gid)."""
    from fedn_amd import robust
    from fedn_amd.aggregators import get_aggregator
    from fedn_amd.budget import HbmBudget
    from fedn_amd.ingest import StagingUpdateHandler
    from fedn_amd.layout import Layout
    from fedn_amd.updatehandler import MemoryUpdateHandler
    monkeypatch.setattr(robust, "SLICE_BYTES", c.slice_bytes)
    uh = MemoryUpdateHandler()
    gid = uh.put_global_model(c.center) if c.center is not None else "global"
    st = StagingUpdateHandler(uh, helper=None, device=DEV, workers=2) if route != "host" else None
    budget = None
    if route == "host":
        budget = HbmBudget(limit=c.budget_updates * Layout.of(c.ups[0]).nbytes)
    elif route == "mixed":
        budget = HbmBudget(limit=0)
    try:
        agg = get_aggregator(c.rule, st or uh)
        agg.device, agg.hbm_budget = torch.device(DEV), budget
        for k, u in enumerate(c.ups):
            staged = route == "staged" or (route == "mixed" and c.staged_bits[k])
            uh.submit(u, 10 + k, model_id=gid, via=st if staged else None)
        model, data = agg.combine_models(helper=None, parameters=c.parameters if parameters is None else parameters)
    finally:
        if st is not None:
            st.close()
    return model, data, uh, agg, budget, gid


def _check_rule(c, agg, model, what):
    rule = c.rule
    if rule in ("trimmedmean", "median"):
        assert_lists_identical(model, c.want, what)
    elif rule in ("krum", "multikrum"):
        assert agg.selected == c.want_sel, (what, agg.selected, c.want_sel)
        assert len(agg.scores) == c.K, what
        assert_lists_identical(model, c.want, what)
    elif rule == "bulyan":
        assert agg.selected == c.want_sel and agg.pick_order == c.want_order, (what, agg.selected, agg.pick_order)
        got, ref = np.asarray(agg.scores, dtype=np.float64), np.asarray(c.want_scores, dtype=np.float64)
        assert got.shape == ref.shape, what
        rtol = _score_rtol(c.ups)
        err = np.abs(got - ref)
        worst = float((err / np.where(ref > 0, ref, 1.0)).max())
        print(f"{what}: worst relative score error {worst:.3e} (bound {rtol:.3e})")
        if worst > _WORST["score"][0]:
            _WORST["score"] = (worst, rtol)
        assert (err <= rtol * ref).all(), (what, agg.scores, c.want_scores)
        assert_lists_identical(model, c.want, what)
    elif rule == "geomedian":
        robust_checks.check_geomed_chain(c.ups, agg, model, c.iterations, c.nu, what)
    else:
        robust_checks.check_cclip_chain(c.ups, c.center, agg, model, c.iterations, c.tau, what)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("rule", fc.RULES)
def test_fuzz_round(rule, seed, route, monkeypatch):
    c = _case(rule, seed)
    what = f"{route}: {fc.describe(c)}"
    print(what)
    model, data, uh, agg, budget, gid = _run(c, route, monkeypatch)
    assert model is not None, f"{what}: the round failed"
    assert data["nr_aggregated_models"] == c.K, what
    assert [a.dtype for a in model] == [fc.out_dtype(d) for _, d in c.spec], what
    assert [a.shape for a in model] == [tuple(s) for s, _ in c.spec], what
    _check_rule(c, agg, model, what)
    assert uh.model_updates.qsize() == 0, f"{what}: the queue is drained"
    assert set(uh.store.models) == ({gid} if c.center is not None else set()), \
        f"{what}: every update is deleted once the result exists (the global model stays)"
    host_side = {"host": c.K - c.budget_updates, "staged": 0, "mixed": c.staged_bits.count(False)}[route]
    assert agg.host_side == host_side, (what, agg.host_side, host_side)
    del agg
    gc.collect()
    if budget is not None:
        assert budget.used(DEV) == 0, f"{what}: the round's reservations went back to the budget"
    _MODELS[(rule, seed, route)] = model
    key = f"{rule}/{route}"
    _WORST["cases"][key] = _WORST["cases"].get(key, 0) + 1


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("rule", fc.RULES)
def test_routes_agree(rule, seed, monkeypatch):
    """Per case, the host and the mixed round's models equal the staged round's bit for bit: the ring
    must not change a bit. (The models are test_fuzz_round's; a route that has not run yet is run here.)

    For the five rules whose values do not depend on the distances' last bits this held from the start.
    The first run found it broken for the two iterated ones (geomedian seeds 0, 8, 14, 17, 19, 23,
    centeredclip seeds 2, 8, 10, 12, 14, 15, 18, 19: models apart by relative 1e-16 to 1e-11): with every
    update in HBM a pass summed a group's squared distances in one launch, with updates on the host slice
    by slice, d differed in its last bits and the next pass's weights inherited that. The iterated rules'
    passes now walk the slice bounds wherever the updates sit (``RobustPipeline._distance_pass``); these
    seeds are the regression cases."""
    c = _case(rule, seed)
    models = {}
    for route in ROUTES:
        models[route] = _MODELS.get((rule, seed, route))
        if models[route] is None:
            models[route] = _run(c, route, monkeypatch)[0]
    for route in ("host", "mixed"):
        assert_lists_identical(models[route], models["staged"], f"{route} vs staged: {fc.describe(c)}")


# the seeds at which the iterated rules' models depended on where the updates sat (test_routes_agree): kept
# whatever FEDN_AMD_FUZZ_BASE says
ROUTE_REGRESSIONS = ([("geomedian", s) for s in (0, 8, 14, 17, 19, 23)] +
                     [("centeredclip", s) for s in (2, 8, 10, 12, 14, 15, 18, 19)])


@pytest.mark.parametrize("rule,seed", ROUTE_REGRESSIONS)
def test_iterated_rules_do_not_depend_on_where_updates_sit(rule, seed, monkeypatch):
    """The named regression cases of test_routes_agree: every pass's distances — the trace, not only the
    model — have the same bits on the three routes."""
    c = _case(rule, seed)
    assert c.iterations >= 1
    runs = {route: _run(c, route, monkeypatch) for route in ROUTES}
    for route in ("host", "mixed"):
        what = f"{route} vs staged: {fc.describe(c)}"
        assert_lists_identical(runs[route][0], runs["staged"][0], what)
        for t, ((w, d), (w0, d0)) in enumerate(zip(runs[route][3].trace, runs["staged"][3].trace)):
            robust_checks.same_bits(np.asarray(w), np.asarray(w0), f"{what}: pass {t} weights")
            assert np.array_equal(np.isnan(d), np.isnan(d0)), f"{what}: pass {t} d"
            robust_checks.same_bits(np.where(np.isnan(d), 0.0, d), np.where(np.isnan(d0), 0.0, d0), f"{what}: pass {t} d")


# ---- a model of empty tensors only ---------------------------------------------------------------------
EMPTY_SPEC = [((0,), np.float32), ((3, 0), np.int32)]


@pytest.mark.parametrize("rule", fc.RULES)
def test_model_of_empty_tensors(rule, monkeypatch):
    """K = 5 on ``[(0,), (3, 0)]``: no kernel is launched, every distance is exactly 0, the selection is by
    FIFO index ([0] for Krum, [0, 1, 2, 3] for Multi-Krum at the default fraction, ``bulyan_select`` of an
    all-zero D for Bulyan), and the model is empty arrays of the output dtypes with every update counted."""
    from fedn_amd import ops, robust
    K = 5
    launches = []
    for name in ("trimmed_mean", "median_window_mean", "pairwise_sqdist", "weighted_mean_sqdist", "centered_clip_step"):
        def counted(*a, _f=getattr(ops, name), _n=name, **kw):
            launches.append(_n)
            return _f(*a, **kw)
        monkeypatch.setattr(ops, name, counted)
    c = SimpleNamespace(rule=rule, K=K, spec=EMPTY_SPEC, slice_bytes=robust.SLICE_BYTES, budget_updates=K,
                           ups=[[np.zeros(s, dtype=d) for s, d in EMPTY_SPEC] for _ in range(K)],
                           center=[np.zeros(s, dtype=d) for s, d in EMPTY_SPEC] if rule == "centeredclip" else None,
                           parameters={"tau": 1.0} if rule == "centeredclip" else None, staged_bits=[False] * K)
    model, data, uh, agg, _, gid = _run(c, "host", monkeypatch)
    assert model is not None and data["nr_aggregated_models"] == K
    assert not launches, f"{rule}: launched {launches}"
    assert_lists_identical(model, [np.zeros((0,), dtype=np.float32), np.zeros((3, 0), dtype=np.float64)], rule)
    if rule == "krum":
        assert agg.selected == [0] and np.array_equal(agg.scores, np.zeros(K))
    elif rule == "multikrum":
        assert agg.selected == [0, 1, 2, 3] and np.array_equal(agg.scores, np.zeros(K))
    elif rule == "bulyan":
        sel, order, scores = robust.bulyan_select(np.zeros((K, K)), robust.bulyan_f(0.2, K))
        assert (agg.selected, agg.pick_order, list(agg.scores)) == (sel, order, scores)
        assert order == list(range(K)) and scores == [0.0] * K
    elif rule in ("geomedian", "centeredclip"):
        assert len(agg.trace) == 4 and agg.excluded == []
        assert all(np.array_equal(d, np.zeros(K)) and not np.signbit(d).any() for _, d in agg.trace)
        assert np.array_equal(agg.distances, np.zeros(K))
        if rule == "geomedian":                                 # (the host rules of an all-zero d: equal shares)
            assert np.array_equal(agg.weights, robust.weiszfeld_weights(np.zeros(K), 1e-6))
        else:
            assert np.array_equal(agg.coefficients, np.full(K, 1.0 / K))
    assert uh.model_updates.qsize() == 0
    assert set(uh.store.models) == ({gid} if rule == "centeredclip" else set())
