"""Robust aggregation on the GPU: ``fa_trimmed_mean`` (kernel ``k_order_mean``) through
``ops.trimmed_mean`` / ``ops.median``, ``robust.RobustPipeline`` and the ``trimmedmean`` / ``median``
plug-ins, bit for bit (values and dtype, NaN by position) against the oracle tests/robust_ref.py."""
import numpy as np
import pytest
import torch

import robust_ref as rr
from golden_io import assert_lists_identical

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KS = [1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32, 33, 63, 64]   # every KP, K = KP, K = KP +- 1, padding at its most
PS = [1, 5, 257, 4099, 65539]
ROW = 65600                  # row length of the test matrix: a multiple of 64, so every row is 16-B aligned
DTYPES = ["f32", "f64", "f16", "bf16", "i32", "i64"]
NP_DT = {"f32": np.float32, "f64": np.float64, "f16": np.float16, "bf16": np.float32, "i32": np.int32, "i64": np.int64}
UINT = {2: np.uint16, 4: np.uint32, 8: np.uint64}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from fedn_amd import _abi
    _abi.load()


def _bf16_exact(x):
    """float32 values that bfloat16 holds exactly (the low 16 bits cleared)."""
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def _upload(S, name):
    t = torch.from_numpy(np.ascontiguousarray(S)).to(DEV)
    return t.to(torch.bfloat16) if name == "bf16" else t      # exact: the values are bf16's


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaN positions differ at {np.argwhere(gn != wn)[:4].tolist()}"
    u = UINT[got.dtype.itemsize]
    bad = (got.view(u) != want.view(u)) & ~gn
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {got.size} differ bitwise, first at "
                           f"{int(np.argwhere(bad)[0][0])}: {got[bad][0]!r} vs {want[bad][0]!r}")


def _random(rng, name, K, n):
    """Mixed magnitudes with ties; in the first quarter of the columns also +-0, +-inf and NaNs."""
    dt = np.dtype(NP_DT[name])
    if dt.kind == "i":
        info = np.iinfo(dt)
        x = rng.integers(info.min, info.max, (K, n), dtype=dt, endpoint=True)
        small = rng.integers(-4, 5, (K, n)).astype(dt)
        x = np.where(rng.random((1, n)) < 0.3, small, x)
        if name == "i64":                                   # not exact in float64: converted with one rounding
            x[:, : n // 8] = (2 ** 53 + rng.integers(1, 1000, (K, n // 8))) * rng.choice([-1, 1], (K, n // 8))
        return np.ascontiguousarray(x)
    span = {"f16": 3, "bf16": 15, "f32": 15, "f64": 150}[name]
    x = np.round(rng.standard_normal((K, n)), 2) * 10.0 ** rng.integers(-span, span, (K, n))
    x = x.astype(dt)
    q = n // 4
    if q:
        pick = rng.random((K, q))
        spec = x[:, :q]
        for lo, hi, v in ((0.00, 0.04, 0.0), (0.04, 0.08, -0.0), (0.08, 0.10, np.inf), (0.10, 0.12, -np.inf),
                          (0.12, 0.14, np.nan)):
            spec[(pick >= lo) & (pick < hi)] = v
    return _bf16_exact(x) if name == "bf16" else np.ascontiguousarray(x)


def _out_torch(name):
    from fedn_amd import ops
    return ops.order_mean_dtype({"bf16": torch.bfloat16}.get(name) or ops.torch_dtype(NP_DT[name]))


def _trims(K):
    return sorted({0, K // 4, (K - 1) // 2})


# ---- ops level -----------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", DTYPES)
def test_ops_trimmed_mean_matrix(name, K):
    from fedn_amd import ops
    rng = np.random.default_rng(1000 * DTYPES.index(name) + K)
    S = _random(rng, name, K, ROW)
    s = rr.sorted_values(S)                                  # the oracle's sort, once for every P and t
    dev = _upload(S, name)
    out = torch.empty(ROW, dtype=_out_torch(name), device=DEV)
    for off in (0, 1):                                       # 1: no 16-B alignment, the scalar path
        for P in PS:
            views = [dev[k, off:off + P] for k in range(K)]
            for t in _trims(K):
                out.zero_()
                o = out[off:off + P]
                ops.trimmed_mean(o, views, t)
                _same(o.cpu().numpy(), rr.mean_of_sorted(s[:, off:off + P], t), f"{name} K={K} P={P} t={t} off={off}")
                assert ops.last_kernel() == "k_order_mean"
            ops.median(out[off:off + P], views)
            _same(out[off:off + P].cpu().numpy(), rr.mean_of_sorted(s[:, off:off + P], rr.median_trim(K)),
                  f"{name} K={K} P={P} median off={off}")


def test_ops_writes_nothing_past_P():
    from fedn_amd import ops
    for name, P in (("f32", 4099), ("f64", 257), ("i32", 5), ("f16", 4099)):
        S = _random(np.random.default_rng(3), name, 5, 8192)
        dev = _upload(S, name)
        for off in (0, 1):
            out = torch.full((8192,), 7.0, dtype=_out_torch(name), device=DEV)
            ops.trimmed_mean(out[off:off + P], [dev[k, off:off + P] for k in range(5)], 1)
            o = out.cpu().numpy()
            assert (o[:off] == 7).all() and (o[off + P:] == 7).all(), (name, off)


def test_ops_refuses_bad_arguments():
    from fedn_amd import ops
    x = torch.zeros(8, device=DEV)
    with pytest.raises(ValueError):
        ops.trimmed_mean(torch.empty(8, device=DEV), [], 0)
    with pytest.raises(ValueError):
        ops.trimmed_mean(torch.empty(8, device=DEV), [x] * 65, 0)
    with pytest.raises(ops.FedAggError):
        ops.trimmed_mean(torch.empty(8, device=DEV), [x, x], 1)                      # 2 * trim == K
    with pytest.raises(ops.FedAggError):
        ops.trimmed_mean(torch.empty(8, dtype=torch.float64, device=DEV), [x, x], 0)  # (F32, F64)


# ---- specials ------------------------------------------------------------------------------------
def _nan_bits(name, negative):
    """A NaN with a payload, of either sign, as the dtype's bits."""
    return {"f32": (0x7FC10000, 0xFFC50000), "bf16": (0x7FC10000, 0xFFC50000), "f16": (0x7E01, 0xFE05),
            "f64": (0x7FF8000000000001, 0xFFF8000000000005)}[name][int(negative)]


def _special_columns(rng, name, K):
    dt = np.dtype(NP_DT[name])
    cols = []
    if dt.kind == "i":
        info = np.iinfo(dt)
        for v in (0, -1, info.max, info.min):
            cols.append([v] * K)
        for m in range(K + 1):
            cols.append([info.max] * m + [info.min] * (K - m))
            cols.append([info.max] * m + [int(v) for v in rng.integers(-3, 4, K - m)])
        if name == "i64":
            cols.append([2 ** 53 + 1 + 2 * k for k in range(K)])
            cols.append([(-1) ** k * (2 ** 62 + 2 ** 9 * k + 1) for k in range(K)])
        S = np.array(cols, dtype=dt).T
    else:
        big = {"f32": 3e38, "bf16": 3e38, "f16": 6e4, "f64": 1.7e308}[name]
        tiny = {"f32": 1e-45, "bf16": 9.2e-41, "f16": 6e-8, "f64": 5e-324}[name]
        fin = lambda n: [float(v) for v in np.round(rng.standard_normal(n), 1)]      # noqa: E731
        for v in (1.5, 0.0, -0.0, np.inf, -np.inf, np.nan, tiny, -tiny, big):
            cols.append([v] * K)                                                      # all equal
        for m in range(K + 1):
            cols.append([-0.0] * m + [0.0] * (K - m))                                 # kept runs of only -0
            cols.append([np.inf] * m + fin(K - m))
            cols.append([-np.inf] * m + fin(K - m))
            cols.append([np.nan] * m + fin(K - m))                                    # fewer than / exactly / more than t
            cols.append([big] * m + [-big] * (K - m))                                 # the kept sum overflows
            cols.append([tiny * (k + 1) * (-1) ** k for k in range(m)] + [0.0] * (K - m))   # denormals
            if 2 * m <= K:
                cols.append([-np.inf] * m + [np.inf] * m + fin(K - 2 * m))
                cols.append([-1.0] * m + [-0.0] * (K - 2 * m) + [1.0] * m)
        S = np.array(cols, dtype=np.float64).T.astype(dt)
        if name == "bf16":
            S = _bf16_exact(S)
        u = S.view(UINT[dt.itemsize])
        nan = np.argwhere(np.isnan(S))
        for i, (r, c) in enumerate(nan):                     # payloads, and every other one negative
            u[r, c] = _nan_bits(name, i % 2)
    for c in range(S.shape[1]):                              # the clients' order must not matter
        S[:, c] = S[rng.permutation(K), c]
    return np.ascontiguousarray(S)


@pytest.mark.parametrize("K", [2, 5, 8, 33])
@pytest.mark.parametrize("name", DTYPES)
def test_ops_specials(name, K):
    from fedn_amd import ops
    rng = np.random.default_rng(77 + K)
    S = _special_columns(rng, name, K)
    total = -(-(S.shape[1] + 1) // 64) * 64                  # rows 16-B aligned, one spare column for off = 1
    S = np.ascontiguousarray(S[:, np.arange(total) % S.shape[1]])
    n = total - 1
    s = rr.sorted_values(S)
    dev = _upload(S, name)
    out = torch.empty(S.shape[1], dtype=_out_torch(name), device=DEV)
    for off in (0, 1):
        views = [dev[k, off:off + n] for k in range(K)]
        for t in sorted({0, min(1, (K - 1) // 2), K // 4, (K - 1) // 2}):
            ops.trimmed_mean(out[off:off + n], views, t)
            _same(out[off:off + n].cpu().numpy(), rr.mean_of_sorted(s[:, off:off + n], t), f"{name} K={K} t={t} off={off}")


@pytest.mark.parametrize("name", ["f32", "f64", "f16", "bf16"])
def test_pads_do_not_leak(name):
    """K = 33 pads 31 of the 64 key slots: with every real value +inf (or NaN) a pad that reached a
    kept slot would show."""
    from fedn_amd import ops
    K, P = 33, 257
    out = torch.empty(P + 1, dtype=_out_torch(name), device=DEV)
    for v, check in ((np.inf, lambda o: np.isposinf(o).all()), (np.nan, lambda o: np.isnan(o).all())):
        S = np.full((K, 320), v, dtype=NP_DT[name])
        dev = _upload(S, name)
        for off in (0, 1):
            for t in (0, 8, 16):
                out.zero_()
                ops.trimmed_mean(out[off:off + P], [dev[k, off:off + P] for k in range(K)], t)
                o = out[off:off + P].cpu().numpy()
                assert check(o), (name, v, t, off, o[:4])
                _same(o, rr.trimmed_mean(S[:, off:off + P], t), f"{name} all {v} t={t}")


# ---- plug-in rounds --------------------------------------------------------------------------------
MNIST = [((64, 784), np.float32), ((64,), np.float32), ((32, 64), np.float32), ((32,), np.float32),
         ((10, 32), np.float32), ((10,), np.float32)]
ODD = [((), np.float32), ((0,), np.float32), ((3, 5), np.float32), ((7,), np.int64), ((0, 4), np.int64),
       ((129,), np.float32), ((0,), np.float64), ((), np.int64)]
MODELS = {"mnist": MNIST, "odd": ODD}


def _clients(rng, spec, K):
    base = [rng.standard_normal(s) for s, _ in spec]
    ups = []
    for k in range(K):
        u = []
        for b, (s, dt) in zip(base, spec):
            if np.dtype(dt).kind == "i":
                u.append(np.asarray(rng.integers(0, 1000, s), dtype=dt).reshape(s))
            else:
                u.append(np.asarray(b + 0.01 * rng.standard_normal(s), dtype=dt).reshape(s))
        ups.append(u)
    if K >= 3:                                   # a hostile client: huge values, an inf and a NaN
        for a in ups[K // 2]:
            if a.size and a.dtype.kind == "f":
                a.reshape(-1)[:] = 1e30
                a.reshape(-1)[0] = np.inf
                a.reshape(-1)[-1] = np.nan
    return ups


def _run_round(agg_name, ups, staged, parameters=None, budget=None, agg=None, uh=None):
    from fedn_amd.aggregators import get_aggregator
    from fedn_amd.ingest import StagingUpdateHandler
    from fedn_amd.updatehandler import MemoryUpdateHandler
    uh = uh or MemoryUpdateHandler()
    st = StagingUpdateHandler(uh, helper=None, device=DEV, workers=2) if staged else None
    try:
        if agg is None:
            agg = get_aggregator(agg_name, st or uh)
            agg.device, agg.hbm_budget = torch.device(DEV), budget
        mus = [uh.submit(u, 10 + k, via=st) for k, u in enumerate(ups)]
        model, data = agg.combine_models(helper=None, parameters=parameters)
    finally:
        if st is not None:
            st.close()
    return model, data, uh, mus, agg


def _want(agg_name, ups, fraction=0.1):
    from fedn_amd.robust import trim_count
    K = len(ups)
    return rr.combine(ups, rr.median_trim(K) if agg_name == "median" else trim_count(fraction, K))


@pytest.mark.parametrize("staged", [False, True], ids=["host", "staged"])
@pytest.mark.parametrize("K", [1, 2, 7, 64])
@pytest.mark.parametrize("model_name", ["mnist", "odd"])
@pytest.mark.parametrize("agg_name", ["trimmedmean", "median"])
def test_plugin_round(agg_name, model_name, K, staged):
    rng = np.random.default_rng(K + 100 * staged)
    ups = _clients(rng, MODELS[model_name], K)
    params = {"trim_fraction": 0.25} if agg_name == "trimmedmean" else None
    model, data, uh, _, _ = _run_round(agg_name, ups, staged, params)
    assert data["nr_aggregated_models"] == K
    for key in ("time_model_load", "time_model_aggregation", "time_h2d", "time_kernel", "time_pack", "time_d2h"):
        assert key in data
    assert_lists_identical(model, _want(agg_name, ups, 0.25), f"{agg_name} {model_name} K={K}")
    assert uh.model_updates.qsize() == 0 and not uh.store.models, "every update is deleted once the result exists"


def test_trimmedmean_default_fraction_and_robustness():
    """The default trim_fraction (0.1) at K = 10 drops one value at each end: the hostile client's inf,
    1e30 and NaN do not reach the model."""
    ups = _clients(np.random.default_rng(5), MNIST, 10)
    model, data, _, _, _ = _run_round("trimmedmean", ups, False)
    assert data["nr_aggregated_models"] == 10
    assert_lists_identical(model, _want("trimmedmean", ups, 0.1), "default fraction")
    assert all(np.isfinite(m).all() and np.abs(m).max() < 10 for m in model)


@pytest.mark.parametrize("staged", [False, True], ids=["host", "staged"])
def test_layout_mismatch_is_skipped_and_kept(staged):
    rng = np.random.default_rng(11)
    ups = _clients(rng, ODD, 6)
    ups[3][2] = np.zeros((5, 3), dtype=np.float32)          # another shape: not this round's layout
    model, data, uh, mus, _ = _run_round("median", ups, staged)
    rest = [u for k, u in enumerate(ups) if k != 3]
    assert data["nr_aggregated_models"] == 5
    assert_lists_identical(model, _want("median", rest), "median without the mismatching update")
    assert set(uh.store.models) == {mus[3].model_update_id}, "the skipped update stays in storage"


def test_more_than_64_updates_refused():
    ups = _clients(np.random.default_rng(12), [((33,), np.float32)], 65)
    model, data, uh, mus, _ = _run_round("trimmedmean", ups, False)
    assert model is None and data["nr_aggregated_models"] == 0
    assert uh.model_updates.qsize() == 0
    assert set(uh.store.models) == {m.model_update_id for m in mus}, "nothing is deleted"


@pytest.mark.parametrize("agg_name", ["trimmedmean", "median"])
def test_budget_keeps_updates_on_the_host(agg_name, monkeypatch):
    """A budget of 3 updates with K = 12: nine stay on the host and are reduced slice by slice through
    the ring, identically to the unbudgeted round."""
    from fedn_amd import robust
    from fedn_amd.budget import HbmBudget
    from fedn_amd.layout import Layout
    spec = [((300, 200), np.float32), ((77,), np.int64), ((1001,), np.float32), ((), np.float32)]
    ups = _clients(np.random.default_rng(13), spec, 12)
    free, data0, _, _, agg0 = _run_round(agg_name, ups, False)
    assert agg0.host_side == 0 and data0["nr_aggregated_models"] == 12
    monkeypatch.setattr(robust, "SLICE_BYTES", 16384)
    budget = HbmBudget(limit=3 * Layout.of(ups[0]).nbytes)
    model, data, uh, _, agg = _run_round(agg_name, ups, False, budget=budget)
    assert agg.host_side == 9 and data["nr_aggregated_models"] == 12, "every update is counted"
    assert_lists_identical(model, free, "budgeted vs unbudgeted")
    assert_lists_identical(model, _want(agg_name, ups), "budgeted vs oracle")
    assert not uh.store.models
    del agg, agg0
    import gc
    gc.collect()
    assert budget.used(DEV) == 0, "the round's reservations went back to the budget"


def test_failed_launch_keeps_every_update(monkeypatch):
    """A launch that fails (injected at the wrapper, as test_gpu_batch_faults.py does): the round is
    (None, data), the updates stay in storage, and the aggregator's next round is exact."""
    from fedn_amd import _abi, ops
    ups = _clients(np.random.default_rng(14), ODD, 7)
    calls = []

    def boom(*a, **kw):
        calls.append(1)
        raise _abi.FedAggError(_abi.FA_EHIP, "trimmed_mean: injected failure")

    with monkeypatch.context() as m:
        m.setattr(ops, "trimmed_mean", boom)
        model, data, uh, mus, agg = _run_round("median", ups, False)
    assert calls and model is None and data["nr_aggregated_models"] == 0
    assert uh.model_updates.qsize() == 0
    assert set(uh.store.models) == {mu.model_update_id for mu in mus}, "every update stays in storage"
    ups2 = _clients(np.random.default_rng(15), ODD, 4)
    model, data, uh, mus2, _ = _run_round("median", ups2, False, agg=agg, uh=uh)
    assert data["nr_aggregated_models"] == 4
    assert_lists_identical(model, _want("median", ups2), "the round after a failed launch")
    assert set(uh.store.models) == {mu.model_update_id for mu in mus}
