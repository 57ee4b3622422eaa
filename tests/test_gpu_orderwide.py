"""The wide trimmed mean / median on the GPU: ``fa_order_mean_wide`` (kernel ``k_order_wide``)
through ``ops.trimmed_mean_wide`` / ``ops.median_wide``, ``RobustPipeline.result_wide`` and the
``trimmedmean_wide`` / ``median_wide`` plug-ins, bit for bit (values, dtype, NaN by position) against the oracle
tests/robust_ref.py. Data, upload and comparison are tests/test_gpu_robust.py's."""
import numpy as np
import pytest
import torch

import robust_ref as rr
from golden_io import assert_lists_identical
from test_gpu_robust import DEV, DTYPES, _clients, _gpu, _out_torch, _random, _run_round, _same, _trims, _upload  # noqa: F401

pytestmark = pytest.mark.gpu

# both sides of the old cap; every KP at K = KP, KP / 2 + 1 and KP - 1: padding at its most
KS = [1, 64, 65, 127, 128, 129, 256, 257, 512, 513, 1023, 1024]
PS = [1, 5, 257, 4099]       # with the tiles of 8 .. 64: one short tile, whole tiles plus one and plus three
ROW = 4160                   # row length of the test matrix: a multiple of 64, so every row is 16-B aligned
MIXED = [((300, 20), np.float32), ((77,), np.int64), ((), np.float32), ((0, 4), np.float32), ((1001,), np.float32)]


def _tile(name, K):
    from fedn_amd import ops
    return ops.order_wide_tile(torch.bfloat16 if name == "bf16" else np.dtype(_NP(name)), K)


def _NP(name):
    from test_gpu_robust import NP_DT
    return NP_DT[name]


# ---- ops level -----------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", DTYPES)
def test_ops_wide_matrix(name, K):
    from fedn_amd import ops
    rng = np.random.default_rng(5000 + 1000 * DTYPES.index(name) + K)
    S = _random(rng, name, K, ROW)
    s = rr.sorted_values(S)                                  # the oracle's sort, once for every P and t
    dev = _upload(S, name)
    out = torch.empty(ROW, dtype=_out_torch(name), device=DEV)
    C = _tile(name, K)
    assert 8 <= C <= 64
    for off in (0, 1):                                       # 1: no 16-B alignment, the element-wise loads
        for P in PS + [2 * C - 1]:                           # ... and a whole tile followed by a tile minus one
            views = [dev[k, off:off + P] for k in range(K)]
            o = out[off:off + P]
            for t in _trims(K):
                out.zero_()
                ops.trimmed_mean_wide(o, views, t)
                _same(o.cpu().numpy(), rr.mean_of_sorted(s[:, off:off + P], t), f"{name} K={K} P={P} t={t} off={off}")
                assert ops.last_kernel() == "k_order_wide"
            ops.median_wide(o, views)
            _same(o.cpu().numpy(), rr.mean_of_sorted(s[:, off:off + P], rr.median_trim(K)), f"{name} K={K} P={P} median")


@pytest.mark.parametrize("K", [1, 2, 33, 64])
@pytest.mark.parametrize("name", DTYPES)
def test_wide_equals_the_register_network(name, K):
    """At K <= 64 both kernels serve the call: the same bits, and each reports itself."""
    from fedn_amd import ops
    P = 4099
    dev = _upload(_random(np.random.default_rng(K), name, K, ROW), name)
    a, b = (torch.empty(P, dtype=_out_torch(name), device=DEV) for _ in range(2))
    views = [dev[k, :P] for k in range(K)]
    for t in _trims(K):
        ops.trimmed_mean(a, views, t)
        assert ops.last_kernel() == "k_order_mean"
        ops.trimmed_mean_wide(b, views, t)
        assert ops.last_kernel() == "k_order_wide"
        _same(b.cpu().numpy(), a.cpu().numpy(), f"{name} K={K} t={t}")


@pytest.mark.parametrize("name,K", [("f32", 65), ("f64", 200), ("i32", 513), ("f16", 1024)])
def test_ops_wide_writes_nothing_outside_out(name, K):
    from fedn_amd import ops
    dev = _upload(_random(np.random.default_rng(3), name, K, 4160), name)
    C = _tile(name, K)
    for P in (5, C, 2 * C - 1, 4099):
        for off in (0, 1, C):
            out = torch.full((4160,), 7.0, dtype=_out_torch(name), device=DEV)
            ops.trimmed_mean_wide(out[off:off + P], [dev[k, off:off + P] for k in range(K)], K // 4)
            o = out.cpu().numpy()
            assert (o[:off] == 7).all() and (o[off + P:] == 7).all(), (name, K, P, off)


def test_ops_wide_is_deterministic_and_refuses_bad_arguments():
    from fedn_amd import ops
    K, P = 300, 4099
    dev = _upload(_random(np.random.default_rng(9), "f32", K, ROW), "f32")
    views = [dev[k, :P] for k in range(K)]
    a, b = torch.empty(P, device=DEV), torch.empty(P, device=DEV)
    ops.trimmed_mean_wide(a, views, 30)
    ops.trimmed_mean_wide(b, views, 30)
    _same(b.cpu().numpy(), a.cpu().numpy(), "two calls")
    with pytest.raises(ValueError, match="1..1024 updates, got 1025"):
        ops.trimmed_mean_wide(a, [views[0]] * 1025, 0)
    with pytest.raises(ValueError):
        ops.trimmed_mean_wide(a, [], 0)
    with pytest.raises(ops.FedAggError):
        ops.trimmed_mean_wide(a, views, 150)                                         # 2 * trim == K
    with pytest.raises(ops.FedAggError):
        ops.trimmed_mean_wide(torch.empty(P, dtype=torch.float64, device=DEV), views, 0)   # (F32, F64)


# ---- pipeline --------------------------------------------------------------------------------------
def _pipe(ups, budget=None):
    from fedn_amd import robust
    pipe = robust.RobustPipeline(DEV, ups[0], tag=0, budget=budget)
    for k, u in enumerate(ups[1:], 1):
        pipe.add(u, tag=k)
    return pipe


@pytest.mark.parametrize("K", [65, 200])
def test_pipeline_result_wide(K, monkeypatch):
    """Every update in HBM, then under a budget of 3 updates with small slices: the oracle's bits both times,
    and the ring within result()'s worst case."""
    from fedn_amd import ops, robust
    from fedn_amd.budget import HbmBudget
    from fedn_amd.layout import Layout
    ups = _clients(np.random.default_rng(20 + K), MIXED, K)
    t = K // 4
    want = rr.combine(ups, t)
    pipe = _pipe(ups)
    assert pipe.host_side == 0
    free = pipe.result_wide(t)
    assert ops.last_kernel() == "k_order_wide"
    assert_lists_identical(free, want, f"K={K} in HBM")
    assert_lists_identical(pipe.result_wide(rr.median_trim(K)), rr.combine(ups, rr.median_trim(K)), f"K={K} median")
    with pytest.raises(ValueError, match=f"leaves nothing of {K}"):
        pipe.result_wide((K + 1) // 2)
    pipe.release()
    monkeypatch.setattr(robust, "SLICE_BYTES", 16384)
    rings = []
    watch = robust.reuse.watch
    monkeypatch.setattr(robust.reuse, "watch", lambda t, s: rings.append(t.numel() * t.element_size()) or watch(t, s))
    pipe = _pipe(ups, HbmBudget(limit=3 * Layout.of(ups[0]).nbytes))
    assert pipe.host_side == K - 3
    assert_lists_identical(pipe.result_wide(t), free, f"K={K}: updates on the host")
    assert rings and max(rings) <= 2 * 64 * 16384, rings
    pipe.release()


def test_pipeline_result_wide_is_result_up_to_64():
    from fedn_amd import ops
    ups = _clients(np.random.default_rng(31), MIXED, 12)
    pipe = _pipe(ups)
    got = pipe.result_wide(3)
    assert ops.last_kernel() == "k_order_mean"
    assert_lists_identical(got, pipe.result(3), "K=12")
    pipe.release()


# ---- plug-ins --------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [65, 129])
@pytest.mark.parametrize("agg_name", ["trimmedmean_wide", "median_wide"])
def test_plugin_round(agg_name, K):
    from fedn_amd.robust import trim_count
    ups = _clients(np.random.default_rng(K), MIXED, K)
    params = {"trim_fraction": 0.25} if agg_name == "trimmedmean_wide" else None
    model, data, uh, _, agg = _run_round(agg_name, ups, False, params)
    assert agg.name == agg_name and data["nr_aggregated_models"] == K
    t = trim_count(0.25, K) if params else rr.median_trim(K)
    assert_lists_identical(model, rr.combine(ups, t), f"{agg_name} K={K}")
    assert uh.model_updates.qsize() == 0 and not uh.store.models, "every update is deleted once the result exists"


@pytest.mark.parametrize("agg_name", ["trimmedmean_wide", "median_wide"])
def test_plugin_refuses_past_max_updates(agg_name, monkeypatch):
    import importlib
    mod = importlib.import_module(f"fedn_amd.aggregators.{agg_name}")
    monkeypatch.setattr(mod.Aggregator, "max_updates", 70)
    ups = _clients(np.random.default_rng(12), [((33,), np.float32)], 71)
    model, data, uh, mus, _ = _run_round(agg_name, ups, False)
    assert model is None and data["nr_aggregated_models"] == 0
    assert uh.model_updates.qsize() == 0
    assert set(uh.store.models) == {m.model_update_id for m in mus}, "nothing is deleted"
