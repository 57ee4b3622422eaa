"""The wide mean around median on the GPU: ``fa_median_window_mean_wide`` (kernel
``k_window_wide``) through ``ops.median_window_mean_wide``, ``RobustPipeline.mean_around_median`` and the ``meamed``
plug-in, bit for bit (values, dtype, NaN by position) against the oracle tests/bulyan_ref.py. Data, upload and
comparison are tests/test_gpu_robust.py's."""
import numpy as np
import pytest
import torch

import bulyan_ref as br
import robust_ref as rr
from golden_io import assert_lists_identical
from test_gpu_robust import (DEV, DTYPES, NP_DT, _clients, _gpu, _out_torch, _random, _run_round, _same,  # noqa: F401
                             _special_columns, _upload)

pytestmark = pytest.mark.gpu

KS = [1, 2, 64, 65, 128, 129, 200, 257, 513, 1000, 1024]     # both parities; every KP, with and without pad slots
THIN = [1, 65, 200, 257, 1024]                                # every KP and both parities for the other dtypes
MIXED = [((300, 20), np.float32), ((77,), np.int64), ((), np.float32), ((0, 4), np.float32), ((1001,), np.float32)]


def _keeps(K):
    return sorted({min(max(k, 1), K) for k in (1, 2, K // 2 + 1, K - 1, K)})


def _tile(name, K):
    from fedn_amd import ops
    return ops.order_wide_tile(torch.bfloat16 if name == "bf16" else np.dtype(NP_DT[name]), K)


def _row(n):
    return -(-(n + 1) // 64) * 64                             # rows 16-byte aligned, one spare column for off = 1


def _check(name, S, Ps, off=0):
    """The op over columns off .. off + P of S for every P and keep, against the oracle (one sort, one walk a keep).
    The output is a slice of a buffer of sevens: nothing outside the slice may change."""
    from fedn_amd import ops
    K = S.shape[0]
    s = rr.sorted_values(S)
    dev = _upload(S, name)
    for keep in _keeps(K):
        want = br.window_mean_of_sorted(s, keep)
        for P in Ps:
            out = torch.full((S.shape[1],), 7.0, dtype=_out_torch(name), device=DEV)
            ops.median_window_mean_wide(out[off:off + P], [dev[k, off:off + P] for k in range(K)], keep)
            assert ops.last_kernel() == "k_window_wide"
            o = out.cpu().numpy()
            _same(o[off:off + P], want[off:off + P], f"{name} K={K} keep={keep} P={P} off={off}")
            assert (o[:off] == 7).all() and (o[off + P:] == 7).all(), (name, K, keep, P, off)


@pytest.mark.parametrize("name,K", [("f32", K) for K in KS] + [(n, K) for n in DTYPES[1:] for K in THIN])
def test_ops_window_wide_matrix(name, K):
    C = _tile(name, K)
    Ps = [1, C - 1, C, C + 1, 3 * C + 5]
    _check(name, _random(np.random.default_rng(7000 + 1000 * DTYPES.index(name) + K), name, K, _row(Ps[-1])), Ps)


def test_ops_window_wide_unaligned_updates():
    """Every update one element past a 16-byte boundary: the element-wise load."""
    P = 3 * _tile("f16", 200) + 5
    _check("f16", _random(np.random.default_rng(41), "f16", 200, _row(P)), [P], off=1)


@pytest.mark.parametrize("name,K", [("f32", 70), ("f64", 129), ("bf16", 70)])
def test_ops_window_wide_specials(name, K):
    """NaNs in some and in all clients, +-inf, +-0, all-equal columns (test_gpu_robust's), and a column whose
    upper neighbour and lowest value are equally far from the median at keep = K - 1: the lower window stays."""
    rng = np.random.default_rng(90 + K)
    S = _special_columns(rng, name, K)
    tie = (np.arange(K) - (K - 1) / 2).astype(S.dtype)[rng.permutation(K)]
    S = np.concatenate([S, tie[:, None]], axis=1)
    n = S.shape[1]
    _check(name, np.ascontiguousarray(S[:, np.arange(_row(n)) % n]), [n])


@pytest.mark.parametrize("K", [1, 33, 64])
@pytest.mark.parametrize("name", DTYPES)
def test_wide_equals_the_register_network(name, K):
    """At K <= 64 both kernels serve the call: the same bits, and each reports itself."""
    from fedn_amd import ops
    P = 257
    dev = _upload(_random(np.random.default_rng(K), name, K, _row(P)), name)
    a, b = (torch.empty(P, dtype=_out_torch(name), device=DEV) for _ in range(2))
    views = [dev[k, :P] for k in range(K)]
    for keep in _keeps(K):
        ops.median_window_mean(a, views, keep)
        assert ops.last_kernel() == "k_median_window"
        ops.median_window_mean_wide(b, views, keep)
        assert ops.last_kernel() == "k_window_wide"
        _same(b.cpu().numpy(), a.cpu().numpy(), f"{name} K={K} keep={keep}")


def _want(ups, keep):
    return [br.window_mean(np.stack([np.asarray(u[i]) for u in ups]), keep) for i in range(len(ups[0]))]


@pytest.mark.parametrize("K", [70, 130])
def test_pipeline_mean_around_median(K, monkeypatch):
    """Every update in HBM, then under a budget of 3 updates with small slices: the oracle's bits both times."""
    from fedn_amd import ops, robust
    from fedn_amd.budget import HbmBudget
    from fedn_amd.layout import Layout
    from test_gpu_orderwide import _pipe
    ups = _clients(np.random.default_rng(60 + K), MIXED, K)
    keep = robust.meamed_keep(0.2, K)
    pipe = _pipe(ups)
    assert pipe.host_side == 0
    free = pipe.mean_around_median(keep)
    assert ops.last_kernel() == "k_window_wide"
    assert_lists_identical(free, _want(ups, keep), f"K={K} in HBM")
    for bad in (0, K + 1):
        with pytest.raises(ValueError, match=f"outside 1..{K}"):
            pipe.mean_around_median(bad)
    pipe.release()
    monkeypatch.setattr(robust, "SLICE_BYTES", 16384)
    pipe = _pipe(ups, HbmBudget(limit=3 * Layout.of(ups[0]).nbytes))
    assert pipe.host_side == K - 3
    assert_lists_identical(pipe.mean_around_median(keep), free, f"K={K}: updates on the host")
    pipe.release()


@pytest.mark.parametrize("K,spec", [(12, MIXED), (70, MIXED), (1024, [((33,), np.float32)])], ids=["12", "70", "1024"])
def test_plugin_round(K, spec):
    from fedn_amd.robust import meamed_keep
    ups = _clients(np.random.default_rng(K), spec, K)
    model, data, uh, _, agg = _run_round("meamed", ups, False, {"byzantine_fraction": 0.3})
    assert agg.name == "meamed" and data["nr_aggregated_models"] == K
    assert_lists_identical(model, _want(ups, meamed_keep(0.3, K)), f"meamed K={K}")
    assert uh.model_updates.qsize() == 0 and not uh.store.models, "every update is deleted once the result exists"


def test_plugin_refuses_past_max_updates(monkeypatch):
    from fedn_amd.aggregators import meamed
    monkeypatch.setattr(meamed.Aggregator, "max_updates", 70)
    ups = _clients(np.random.default_rng(12), [((33,), np.float32)], 71)
    model, data, uh, mus, _ = _run_round("meamed", ups, False)
    assert model is None and data["nr_aggregated_models"] == 0
    assert uh.model_updates.qsize() == 0
    assert set(uh.store.models) == {m.model_update_id for m in mus}, "nothing is deleted"
