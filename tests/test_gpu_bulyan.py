"""Bulyan on the GPU: ``fa_median_window_mean`` (kernel ``k_median_window``) through
``ops.median_window_mean``, ``robust.RobustPipeline.bulyan`` and the ``bulyan`` plug-in, against the oracle
tests/bulyan_ref.py: bit for bit at every dtype, K, window length, alignment and tail, the same bits on
every call, selections equal."""
import functools

import numpy as np
import pytest
import torch

import bulyan_ref as br
import krum_ref as kr
from golden_io import assert_lists_identical
from robust_fuzz_cases import bulyan_gap, round_updates, selection_bound

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KS = [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64]        # every KP, K = KP, K = KP + 1, padding at its most
PS = [1, 5, 257, 4099]
ROW = 4160                                                 # >= 1 + max(PS); rows of a (K, ROW) matrix stay 16-B aligned
DTYPES = ["f32", "f64", "f16", "bf16", "i32", "i64"]
NP_DT = {"f32": np.float32, "f64": np.float64, "f16": np.float16, "bf16": np.float32, "i32": np.int32, "i64": np.int64}
TORCH_DT = {"f32": torch.float32, "f64": torch.float64, "f16": torch.float16, "bf16": torch.bfloat16,
            "i32": torch.int32, "i64": torch.int64}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from fedn_amd import _abi
    _abi.load()
    yield
    torch.cuda.synchronize()


def _bf16_exact(x):
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def _keeps(K):
    fmax = (K - 3) // 4 if K >= 3 else 0
    return sorted({1, 2, K - 2, K - 1, K, K - 2 * fmax} & set(range(1, K + 1)))


def _plant(S, c, name, rng):
    """Planted columns from column ``c`` on; returns the next free column."""
    K = S.shape[0]
    dt = S.dtype
    half, third = K // 2, max(1, K // 3)
    cols = []
    cols.append(np.full(K, S[0, c]))                                           # all values equal
    dup = S[:, c + 1].copy()
    dup[np.argsort(dup)[K // 4:K // 4 + half + 1]] = np.sort(dup)[K // 2]      # a run of duplicates around the median
    cols.append(dup)
    two = S[:, c + 2].copy()
    two[rng.permutation(K)[:half]] = two[0]                                    # two runs of duplicates
    cols.append(two)
    if dt.kind == "f":
        z = np.where(rng.random(K) < 0.5, -0.0, 0.0)                           # -0 and +0 mixed
        cols.append(z)
        z2 = S[:, c + 3].copy()
        z2[rng.permutation(K)[:half + 1]] = -0.0
        z2[rng.permutation(K)[:third]] = 0.0
        cols.append(z2)
        for lo, hi in ((1, 0), (0, 1), (1, 1), (half + 1, 0), (0, half + 1)):  # +-inf: a few, a majority
            v = S[:, c + 4].copy()
            p = rng.permutation(K)
            v[p[:lo]] = -np.inf
            v[p[lo:lo + hi]] = np.inf
            cols.append(v)
        for n in (min(third, (K - 1) // 2), half + 1, K):                      # NaNs: a minority, a majority, all
            v = S[:, c + 5].copy()
            v[rng.permutation(K)[:n]] = np.nan
            cols.append(v)
        v = S[:, c + 6].copy()
        v[rng.permutation(K)[:third]] = np.nan
        v[rng.permutation(K)[:third]] = np.inf
        cols.append(v)
        if name == "f16":                                                      # an f32 mean that rounds in the conversion
            cols.append(1.0 + rng.integers(0, 7, K) * 2.0 ** -10)
            cols.append(np.full(K, 65504.0))                                   # the f32 sum is past f16's range, the mean is not
            cols.append(rng.choice([6.0e-8, 1.2e-7, 6.1e-5], K))               # subnormal results
    else:
        info = np.iinfo(dt)
        v = S[:, c + 3].copy()
        v[rng.permutation(K)[:third]] = info.min
        v[rng.permutation(K)[:third]] = info.max
        cols.append(v)
        if name == "i64":                                                      # not exact in float64
            cols.append(2 ** 53 + 2 * rng.integers(1, 500, K) + 1)
            cols.append(-(2 ** 53) - rng.integers(1, 1000, K))
            cols.append((2 ** 62 + rng.integers(1, 1000, K)) * rng.choice([-1, 1], K))
    for i, v in enumerate(cols):
        S[:, c + i] = np.asarray(v).astype(dt)
    return c + len(cols)


def _data(rng, name, K):
    """K updates that are close to each other, as in federated learning — a base plus small noise — with
    the planted columns at the start (P = 1, 5 see some), past one lane's strip and at the ragged end."""
    dt = np.dtype(NP_DT[name])
    x = rng.standard_normal(ROW) + 0.05 * rng.standard_normal((K, ROW))
    if dt.kind == "i":
        x = np.round(x * (2.0 ** 20 if name == "i32" else 2.0 ** 40))
    S = np.ascontiguousarray(x.astype(dt))
    for c in (0, 40, 230, 4070):
        end = _plant(S, c, name, rng)
        assert end <= c + 27
    return _bf16_exact(S) if name == "bf16" else S


def _upload(S, name):
    t = torch.from_numpy(np.ascontiguousarray(S)).to(DEV)
    return t.to(torch.bfloat16) if name == "bf16" else t       # exact: the values are bf16's


def _assert_bits(got, want, what):
    assert_lists_identical([got], [want], what)


# ---- ops level ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", DTYPES)
def test_ops_median_window_mean(name, K):
    """Every window length of interest at every size, on 16-B aligned buffers (the vector path with its
    ragged tail) and on buffers one element past a 16-B boundary (E = 1), bit for bit against the oracle;
    keep = K against ops.trimmed_mean on the same buffers; two calls give the same bits."""
    from fedn_amd import ops
    rng = np.random.default_rng(1000 * DTYPES.index(name) + K)
    S = _data(rng, name, K)
    dev = _upload(S, name)
    odt = ops.order_mean_dtype(TORCH_DT[name])
    s = br.rr.sorted_values(S)                                 # sorted once for every keep
    for keep in _keeps(K):
        want = br.window_mean_of_sorted(s, keep)
        for P in PS:
            for off in (0, 1):
                views = [dev[k, off:off + P] for k in range(K)]
                assert all((v.data_ptr() % 16 != 0) == bool(off) for v in views)
                out = torch.empty(P, dtype=odt, device=DEV)
                assert ops.median_window_mean(out, views, keep) is out
                assert ops.last_kernel() == "k_median_window"
                got = out.cpu().numpy()
                _assert_bits(got, want[off:off + P], f"{name} K={K} keep={keep} P={P} off={off}")
                again = torch.empty(P, dtype=odt, device=DEV)
                ops.median_window_mean(again, views, keep)
                assert torch.equal(again.view(torch.uint8), out.view(torch.uint8)), "two calls differ"
                if keep == K:
                    tm = torch.empty(P, dtype=odt, device=DEV)
                    ops.trimmed_mean(tm, views, 0)
                    assert torch.equal(tm.view(torch.uint8), out.view(torch.uint8)), "keep = K is the trimmed mean at trim 0"


@pytest.mark.parametrize("K", [3, 4, 5, 8, 9, 16, 17, 32, 33, 64])       # K = KP and K = KP / 2 + 1 of every KP
@pytest.mark.parametrize("name", ["f32", "f64", "i64"])
def test_ops_every_window_length(name, K):
    """``window_start`` dispatches on the runtime ``keep`` to one separately compiled block per window
    length: EVERY keep in 1..K runs once on the device — for the 32-bit key with the f32 accumulator, the
    64-bit key, and the integer key with the f64 accumulator — over the first 261 columns (the planted
    columns at 0, 40 and 230, the vector path with a ragged tail), bit for bit against the oracle."""
    from fedn_amd import ops
    P, pitch = 261, 264                                        # rows of the result stay 16-B aligned
    S = _data(np.random.default_rng(50_000 + 1000 * DTYPES.index(name) + K), name, K)
    dev = _upload(S, name)
    views = [dev[k, :P] for k in range(K)]
    assert not any(v.data_ptr() % 16 for v in views)
    odt = ops.order_mean_dtype(TORCH_DT[name])
    out = torch.full((K, pitch), -5.0, dtype=odt, device=DEV)
    for keep in range(1, K + 1):
        ops.median_window_mean(out[keep - 1, :P], views, keep)
        assert ops.last_kernel() == "k_median_window"
    got = out.cpu().numpy()
    assert (got[:, P:] == -5).all(), "nothing past the P elements is written"
    s = br.rr.sorted_values(S[:, :P])                          # sorted once for every keep
    for keep in range(1, K + 1):
        _assert_bits(got[keep - 1, :P], br.window_mean_of_sorted(s, keep), f"{name} K={K} keep={keep}")


@pytest.mark.parametrize("name", ["f32", "f64", "i32"])
def test_nothing_outside_the_window_is_written(name):
    from fedn_amd import ops
    K, keep, guard = 9, 5, 64
    S = _data(np.random.default_rng(3), name, K)
    dev = _upload(S, name)
    odt = ops.order_mean_dtype(TORCH_DT[name])
    want = br.window_mean(S, keep)
    for P in (5, 257, 4099):
        for off in (0, 1):
            buf = torch.full((guard + off + P + guard,), -5.0, dtype=odt, device=DEV)
            ops.median_window_mean(buf[guard + off:guard + off + P], [dev[k, :P] for k in range(K)], keep)
            o = buf.cpu().numpy()
            assert (o[:guard + off] == -5).all() and (o[guard + off + P:] == -5).all(), (name, P, off)
            _assert_bits(o[guard + off:guard + off + P], want[:P], f"{name} P={P} off={off}")
    assert torch.equal(dev.view(torch.uint8), _upload(S, name).view(torch.uint8)), "the updates are read only"


def test_ops_refuses_bad_arguments():
    from fedn_amd import _abi, ops
    x = torch.zeros(8, device=DEV)
    out = torch.zeros(8, device=DEV)
    with pytest.raises(ValueError):
        ops.median_window_mean(out, [], 1)
    with pytest.raises(ValueError):
        ops.median_window_mean(out, [x] * 65, 1)
    with pytest.raises(ValueError):
        ops.median_window_mean(out, [x, torch.zeros(9, device=DEV)], 1)                       # lengths differ
    with pytest.raises(TypeError):
        ops.median_window_mean(out, [x, torch.zeros(8, dtype=torch.float64, device=DEV)], 1)  # dtypes differ
    for keep in (0, 3, -1):
        with pytest.raises(_abi.FedAggError) as e:
            ops.median_window_mean(out, [x, x], keep)
        assert e.value.status == _abi.FA_EINVAL
    with pytest.raises(_abi.FedAggError) as e:
        ops.median_window_mean(torch.zeros(8, dtype=torch.float64, device=DEV), [x, x], 1)    # not f32's output dtype
    assert e.value.status == _abi.FA_EDTYPE


# ---- rounds ------------------------------------------------------------------------------------------
SPEC = [((300, 50), np.float32), ((77,), np.int64), ((0,), np.float32), ((1001,), np.float64), ((), np.float32),
        ((513,), np.float16)]


def _round_updates(seed, K, f, spec):
    """K updates of the model ``spec``, f of them hostile: the generator the robust rules' tests share
    (tests/robust_fuzz_cases.round_updates). Returns (updates, hostile indices)."""
    return round_updates(seed, K, f, spec)


def _selection(ups, f, what):
    """The oracle's selection from the oracle's distances, after asserting the precondition in float64 on
    the CPU: at EVERY iteration the relative gap between the smallest score and the next one is at least
    10 x the distance bound, so the kernel's rounding cannot change a pick. One exact tie is structural
    and skipped over: late iterations have nn = 1, a score is then the nearest neighbour's distance, and
    two mutual nearest neighbours hold the SAME entry of the exactly symmetric D — equal on the device as
    here, whatever its rounding, and broken by the FIFO index in both (tests/robust_fuzz_cases.bulyan_gap,
    which the fuzz shares)."""
    D = kr.model_distances(ups)
    bound = selection_bound(ups)
    worst = bulyan_gap(D, f)
    print(f"{what}: smallest score gap {worst:.3e}, needed {bound:.2e}")
    assert worst >= bound, f"{what}: precondition — score gap {worst:.3e} below {bound:.2e}: pick another seed"
    return br.select(D.tolist(), f)


def _score_rtol(ups):
    """The bound of a pick's score against the oracle's: every entry of a dtype group's D is within
    ``ops.sqdist_rtol`` of exact arithmetic, and a score — like the sums over dtype groups and slices under
    it — adds non-negative terms, so the largest of the relative bounds carries over; 2**-45 covers the
    float64 additions themselves (fewer than 2**8 of them, 2**-53 each)."""
    from fedn_amd import ops
    return max(ops.sqdist_rtol(np.asarray(a).dtype, np.asarray(a).size) for a in ups[0]) + 2.0 ** -45


# seeds whose score gaps pass _selection's precondition: found on the CPU with the oracle alone
PIPE_SEEDS = {7: 0, 11: 0, 23: 0}
PLUGIN_SEEDS = {7: 0, 10: 0, 17: 0, 64: 1}                    # (K = 64: seed 0's gap is 4.5e-4, below the 6.13e-4 needed)
BUDGET_SEED = 1                                               # K = 11 on RING_SPEC
# three dtype groups, the f32 group's tensors straddling the slice bounds (test_gpu_robust_streams.py's model)
RING_SPEC = [((300, 200), np.float32), ((77,), np.int64), ((1001,), np.float32), ((), np.float32), ((513,), np.float16)]


@pytest.mark.parametrize("K", [7, 11, 23])
def test_pipeline_hbm_and_ring(K, monkeypatch):
    """The largest legal f. Every update in HBM (one launch per dtype group), then the same round with a
    zero budget: every update stays on the host and both passes walk the groups slice by slice through the
    ring (the f32 group takes four slices). Same selection, same bits, the oracle's."""
    from fedn_amd import robust
    from fedn_amd.budget import HbmBudget
    f = (K - 3) // 4
    ups, hostile = _round_updates(PIPE_SEEDS[K], K, f, SPEC)
    want_sel, want_order, want_scores = _selection(ups, f, f"pipeline K={K}")
    want, sel2 = br.combine(ups, f)
    assert sel2 == want_sel and len(want_sel) == K - 2 * f
    score_rtol = _score_rtol(ups)
    monkeypatch.setattr(robust, "SLICE_BYTES", 16384)
    models = []
    for limit, host_side in ((None, 0), (0, K)):
        pipe = robust.RobustPipeline(DEV, ups[0], budget=HbmBudget(limit=limit) if limit is not None else None)
        try:
            for u in ups[1:]:
                pipe.add(u)
            assert pipe.host_side == host_side
            model = pipe.bulyan(f)
            assert pipe.selected == want_sel and pipe.pick_order == want_order, (pipe.selected, pipe.pick_order)
            got_scores, ref_scores = np.asarray(pipe.scores, dtype=np.float64), np.asarray(want_scores)
            worst = float((np.abs(got_scores - ref_scores) / ref_scores).max())
            print(f"K={K} host_side={host_side}: worst relative score error {worst:.3e} (bound {score_rtol:.3e})")
            assert (np.abs(got_scores - ref_scores) <= score_rtol * ref_scores).all(), (pipe.scores, want_scores)
        finally:
            pipe.release()
        assert_lists_identical(model, want, f"K={K} host_side={host_side} vs oracle")
        models.append(model)
    assert_lists_identical(models[0], models[1], "HBM vs ring")
    assert [a.dtype for a in models[0]] == [np.dtype(d) for d in (np.float32, np.float64, np.float32, np.float64,
                                                                np.float32, np.float16)]
    assert models[0][2].shape == (0,)


def test_pipeline_refuses_bad_f():
    from fedn_amd import robust
    ups, _ = _round_updates(0, 7, 0, [((33,), np.float32)])
    pipe = robust.RobustPipeline(DEV, ups[0])
    try:
        for u in ups[1:]:
            pipe.add(u)
        for f in (-1, 2):                                      # 7 < 4 * 2 + 3
            with pytest.raises(ValueError):
                pipe.bulyan(f)
        model = pipe.bulyan(0)                                 # f = 0: everyone, the plain mean
        assert pipe.selected == list(range(7))
        assert_lists_identical(model, br.rr.combine(ups, 0), "f = 0")
    finally:
        pipe.release()


def _run_round(ups, parameters=None, delete_models=True, staged=False, budget=None, agg=None, uh=None):
    from fedn_amd.aggregators import get_aggregator
    from fedn_amd.ingest import StagingUpdateHandler
    from fedn_amd.updatehandler import MemoryUpdateHandler
    uh = uh or MemoryUpdateHandler()
    st = StagingUpdateHandler(uh, helper=None, device=DEV, workers=2) if staged else None
    try:
        if agg is None:
            agg = get_aggregator("bulyan", st or uh)
            agg.device, agg.hbm_budget = torch.device(DEV), budget
        mus = [uh.submit(u, 10 + k, via=st) for k, u in enumerate(ups)]
        model, data = agg.combine_models(helper=None, delete_models=delete_models, parameters=parameters)
    finally:
        if st is not None:
            st.close()
    return model, data, uh, mus, agg


def _attack_round():
    """K = 11, f = 2: nine honest clients, client 3 at 1e30 everywhere, client 8 all NaN."""
    spec = [((4099,), np.float32), ((257,), np.float64)]
    ups, _ = _round_updates(1, 11, 0, spec)
    for i, (s, dt) in enumerate(spec):
        ups[3][i] = np.full(s, 1e30, dtype=dt)
        ups[8][i] = np.full(s, np.nan, dtype=dt)
    return ups, [3, 8]


def test_plugin_attack_round():
    ups, hostile = _attack_round()
    f = br.byzantine_count(0.2, 11)
    assert f == 2
    want_sel, want_order, _ = _selection(ups, f, "attack round")
    want, _ = br.combine(ups, f)
    honest = [k for k in range(11) if k not in hostile]
    for i, w in enumerate(want):                               # a property of this input: checked on the oracle first
        H = np.stack([ups[k][i] for k in honest])
        assert np.isfinite(w).all() and (w >= H.min(axis=0)).all() and (w <= H.max(axis=0)).all()
    assert not set(want_sel) & set(hostile)
    model, data, uh, _, agg = _run_round(ups, {"byzantine_fraction": 0.2})
    assert data["nr_aggregated_models"] == 11
    for key in ("time_model_load", "time_model_aggregation", "time_h2d", "time_kernel", "time_pack", "time_d2h"):
        assert key in data
    assert agg.selected == want_sel and agg.pick_order == want_order and len(agg.scores) == 7
    assert not set(agg.selected) & set(hostile), "no hostile client is selected"
    assert_lists_identical(model, want, "attack round")
    assert all(np.isfinite(a).all() for a in model)
    assert uh.model_updates.qsize() == 0 and not uh.store.models, "every update is deleted once the result exists"


def test_plugin_default_fraction_and_kept_models():
    """No parameters: byzantine_fraction = 0.2; delete_models = False keeps every update in storage."""
    ups, hostile = _attack_round()
    want, want_sel = br.combine(ups, 2)
    model, data, uh, mus, agg = _run_round(ups, None, delete_models=False)
    assert data["nr_aggregated_models"] == 11 and agg.selected == want_sel
    assert_lists_identical(model, want, "default fraction")
    assert set(uh.store.models) == {mu.model_update_id for mu in mus}


TIMING_KEYS = ("time_model_load", "time_model_aggregation", "time_h2d", "time_kernel", "time_pack", "time_d2h")


@functools.lru_cache(maxsize=None)
def _plugin_case(K):
    """The K-client round on the mixed SPEC at byzantine_fraction 0.2 and what the oracle says about it:
    computed once for the host and the staged round, read only. For f = 0 the selection precondition is
    not asked: its gap is structurally 0 there (the last two remaining clients' scores are the same entry
    of D), and every client is selected whatever the order."""
    f = br.byzantine_count(0.2, K)
    ups, hostile = _round_updates(PLUGIN_SEEDS.get(K, 0), K, f, SPEC)
    if f == 0:
        return ups, f, None, None, br.rr.combine(ups, 0)
    want_sel, want_order, _ = _selection(ups, f, f"plug-in K={K}")
    want, sel2 = br.combine(ups, f)
    assert sel2 == want_sel and len(want_sel) == K - 2 * f and len(hostile) == f
    return ups, f, want_sel, want_order, want


@pytest.mark.parametrize("staged", [False, True], ids=["host", "staged"])
@pytest.mark.parametrize("K", [1, 2, 3, 7, 10, 17, 64])
def test_plugin_round(K, staged):
    """The plug-in on the mixed model, updates from the host and staged on arrival (StagingUpdateHandler),
    from the rounds where Bulyan is the plain mean (f = 0) to K = 64 with f = 12."""
    ups, f, want_sel, want_order, want = _plugin_case(K)
    assert f == {1: 0, 2: 0, 3: 0, 7: 1, 10: 1, 17: 3, 64: 12}[K]
    model, data, uh, _, agg = _run_round(ups, {"byzantine_fraction": 0.2}, staged=staged)
    assert data["nr_aggregated_models"] == K
    for key in TIMING_KEYS:
        assert key in data
    if f:
        assert agg.selected == want_sel and agg.pick_order == want_order, (agg.selected, agg.pick_order)
    else:
        assert agg.selected == list(range(K)) and sorted(agg.pick_order) == agg.selected
    assert len(agg.scores) == K - 2 * f
    assert_lists_identical(model, want, f"bulyan plug-in K={K} f={f}")
    if K == 1:
        assert_lists_identical(model, [a.astype(br.rr.out_dtype(a.dtype)) for a in ups[0]], "K = 1: the update itself")
    assert uh.model_updates.qsize() == 0 and not uh.store.models, "every update is deleted once the result exists"


def test_budget_keeps_updates_on_the_host(monkeypatch):
    """A budget of 3 updates with K = 11, f = 2: eight stay on the host and both passes walk them slice by
    slice through the ring — pass 1 with eight rows, pass 2 with the selected ones' only. The selection
    drops an update that sits in HBM (a precondition, asserted on the oracle's selection). Same selection
    and same model as with everything in HBM."""
    import gc

    from fedn_amd import robust
    from fedn_amd.budget import HbmBudget
    from fedn_amd.layout import Layout
    K, f, in_hbm = 11, 2, 3
    assert br.byzantine_count(0.2, K) == f
    ups, hostile = _round_updates(BUDGET_SEED, K, f, RING_SPEC)
    want_sel, want_order, _ = _selection(ups, f, "bulyan budget")
    want, _ = br.combine(ups, f)
    rejected = sorted(set(range(K)) - set(want_sel))
    print(f"bulyan budget: hostile {hostile}, selected {want_sel}, rejected {rejected}")
    assert any(k < in_hbm for k in rejected) and any(k < in_hbm for k in want_sel), "precondition: HBM side"
    assert any(k >= in_hbm for k in rejected) and any(k >= in_hbm for k in want_sel), "precondition: host side"
    free, data0, _, _, agg0 = _run_round(ups)
    assert agg0.host_side == 0 and data0["nr_aggregated_models"] == K and agg0.selected == want_sel
    monkeypatch.setattr(robust, "SLICE_BYTES", 16384)
    budget = HbmBudget(limit=in_hbm * Layout.of(ups[0]).nbytes)
    model, data, uh, _, agg = _run_round(ups, budget=budget)
    assert agg.host_side == K - in_hbm == 8 and data["nr_aggregated_models"] == K, "every update is counted"
    assert agg.selected == want_sel and agg.pick_order == want_order and not set(agg.selected) & set(hostile)
    assert_lists_identical(model, free, "budgeted vs unbudgeted")
    assert_lists_identical(model, want, "budgeted vs oracle")
    assert not uh.store.models
    del agg, agg0
    gc.collect()
    assert budget.used(DEV) == 0, "the round's reservations went back to the budget"


@pytest.mark.parametrize("staged", [False, True], ids=["host", "staged"])
def test_layout_mismatch_is_skipped_and_kept(staged):
    """K = 8 with one update of another shape: the round is the oracle's over the other seven (f = 1), the
    selection's indices count the admitted updates, and only the mismatching update stays in storage."""
    ups, f, want_sel, want_order, want = _plugin_case(7)          # (asserts _selection's precondition on the 7)
    assert f == 1
    odd = [a.copy() for a in ups[0]]
    odd[0] = np.zeros((5, 3), dtype=np.float32)                   # not this round's layout
    queue = ups[:3] + [odd] + ups[3:]
    model, data, uh, mus, agg = _run_round(queue, staged=staged)
    assert data["nr_aggregated_models"] == 7
    assert agg.selected == want_sel and agg.pick_order == want_order, "indices count the admitted updates"
    assert_lists_identical(model, want, "bulyan without the mismatching update")
    assert set(uh.store.models) == {mus[3].model_update_id}, "the skipped update stays in storage"


def test_too_few_finite_scores_keeps_every_update():
    """K = 7, f = 1: theta = 5 picks, but three clients hold NaNs — no remaining client has K - f - 2 = 4
    finite neighbours: (None, data), nothing deleted."""
    ups, _ = _round_updates(5, 7, 0, [((257,), np.float32)])
    for k in (0, 3, 5):
        ups[k][0][7] = np.nan
    with pytest.raises(ValueError):
        br.select(kr.model_distances(ups).tolist(), 1)
    model, data, uh, mus, agg = _run_round(ups, {"byzantine_fraction": 0.2})
    assert model is None and data["nr_aggregated_models"] == 0 and agg.selected is None
    assert uh.model_updates.qsize() == 0
    assert set(uh.store.models) == {mu.model_update_id for mu in mus}


def test_more_than_64_updates_refused():
    ups, _ = _round_updates(12, 65, 0, [((33,), np.float32)])
    model, data, uh, mus, _ = _run_round(ups)
    assert model is None and data["nr_aggregated_models"] == 0
    assert uh.model_updates.qsize() == 0
    assert set(uh.store.models) == {m.model_update_id for m in mus}, "nothing is deleted"
