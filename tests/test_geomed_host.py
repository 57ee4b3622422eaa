"""Host side of the geometric-median rule: the C ABI's argument validation of ``fa_weighted_mean_sqdist``,
``robust.weiszfeld_weights`` against a plain-Python loop, the oracle tests/geomed_ref.py against the
existing oracles, and the plug-in's parameter validation. No device is touched: every library call here
returns before any HIP call."""
import ctypes
import math

import numpy as np
import pytest

import geomed_ref as gr
import krum_ref as kr
import robust_ref as rr
from fedn_amd import _abi
from fedn_amd.robust import weiszfeld_weights

SIX = [_abi.FA_F32, _abi.FA_F64, _abi.FA_F16, _abi.FA_BF16, _abi.FA_I32, _abi.FA_I64]
OUT_OF = {_abi.FA_F32: _abi.FA_F32, _abi.FA_F64: _abi.FA_F64, _abi.FA_F16: _abi.FA_F16, _abi.FA_BF16: _abi.FA_F32,
          _abi.FA_I32: _abi.FA_F64, _abi.FA_I64: _abi.FA_F64}


# ---- C ABI -------------------------------------------------------------------------------------
def test_library_exports_fa_weighted_mean_sqdist():
    lib, probe = _abi.load(), _abi.load_probe()
    for name in ("fa_weighted_mean_sqdist", "fa_wmean_sqdist_work"):
        assert name in _abi.EXPORTS and hasattr(lib, name) and hasattr(probe, name)
    # the launch geometry is a measurement entry point: the probe library's alone
    assert "fa_wmean_sqdist_geometry" in _abi.PROBE_EXPORTS and hasattr(probe, "fa_wmean_sqdist_geometry")
    assert "fa_wmean_sqdist_geometry" not in _abi.EXPORTS
    assert lib.fa_abi_version() == _abi.ABI_VERSION >= 11


def _call(out=48, od=None, dist=16, ups=True, ud=_abi.FA_F32, beta="uniform", K=4, P=10, acc=0, work=4096, null_at=None):
    """Fake pointers: the call must return before it touches any of them."""
    n = max(1, min(K, 80))
    ptrs = [64 + 16 * k for k in range(n)]
    if null_at is not None:
        ptrs[null_at] = 0
    if isinstance(beta, str):
        beta = [1.0 / n] * n
    od = OUT_OF.get(ud, _abi.FA_F32) if od is None else od
    return _abi.load().fa_weighted_mean_sqdist(out, od, dist, _abi.ptr_array(ptrs) if ups else None, ud,
                                               _abi.double_array(beta) if beta is not None else None, K, P, acc, work, None)


@pytest.mark.parametrize("kw", [dict(dist=None), dict(beta=None), dict(ups=False), dict(work=None), dict(null_at=2),
                                dict(K=0), dict(K=65), dict(K=-1), dict(P=-1),
                                dict(beta=[0.5, -0.25, 0.5, 0.25]), dict(beta=[0.5, float("nan"), 0.5, 0.25]),
                                dict(beta=[0.5, float("inf"), 0.5, 0.25]), dict(beta=[0.0] * 4),
                                dict(beta=[1e-60, 0.0, 1e-50, 0.0]), dict(beta=[1e39, 0.0, 0.0, 0.0])],
                         ids=["null_dist", "null_beta", "null_updates", "null_work", "null_client", "K0", "K65", "K_neg",
                              "P_neg", "beta_negative", "beta_nan", "beta_inf", "beta_all_zero", "beta_all_zero_in_f32",
                              "beta_inf_in_f32"])
def test_argument_errors(kw):
    assert _call(**kw) == _abi.FA_EINVAL
    assert _abi.load().fa_last_error().decode()


def test_weights_are_judged_in_the_compute_type():
    """1e-60 is zero as a float32 and a weight as a float64: refused for the f32 family only (here with
    accumulate and P = 0, so the accepted call launches nothing)."""
    beta = [1e-60, 0.0, 1e-50, 0.0]
    for ud in (_abi.FA_F32, _abi.FA_F16, _abi.FA_BF16):
        assert _call(ud=ud, beta=beta, P=0, acc=1) == _abi.FA_EINVAL
    for ud in (_abi.FA_F64, _abi.FA_I32, _abi.FA_I64):
        assert _call(ud=ud, beta=beta, P=0, acc=1) == _abi.FA_OK


@pytest.mark.parametrize("ud", [_abi.FA_I8, _abi.FA_I16, _abi.FA_U8, _abi.FA_U16, _abi.FA_U32, _abi.FA_U64, _abi.FA_NONE, 99])
def test_dtype_errors(ud):
    assert _call(ud=ud) == _abi.FA_EDTYPE
    assert _abi.load().fa_last_error().decode()
    assert _call(ud=ud, K=65) == _abi.FA_EINVAL, "the argument checks come first"


@pytest.mark.parametrize("ud", SIX)
def test_output_dtype_is_the_tables(ud):
    for od in SIX + [_abi.FA_I8, _abi.FA_NONE]:
        want = _abi.FA_OK if od == OUT_OF[ud] else _abi.FA_EDTYPE
        assert _call(ud=ud, od=od, P=0, acc=1) == want, (ud, od)
        assert _call(ud=ud, od=od, out=None, P=0, acc=1) == want, "a NULL out still names its dtype"


@pytest.mark.parametrize("ud", SIX)
def test_nothing_to_add_is_ok(ud):
    """P = 0 with accumulate = 1 adds nothing: FA_OK with no launch. (With accumulate = 0 the zeros are
    written by a launch: tests/test_gpu_geomed.py.)"""
    for K in (1, 2, 5, 64):
        assert _call(ud=ud, K=K, P=0, acc=1) == _abi.FA_OK
    assert _call(ud=ud, K=3, P=0, acc=1, null_at=1) == _abi.FA_OK, "an empty buffer may be a null pointer"
    assert _call(ud=ud, K=3, P=0, acc=1, out=None) == _abi.FA_OK


def test_work_size_and_geometry():
    lib, geo = _abi.load(), _abi.load_probe()
    for K in (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64):
        te32, te64, r, wg, ft32, ft64 = (ctypes.c_int() for _ in range(6))
        assert geo.fa_wmean_sqdist_geometry(_abi.FA_F16, K, ctypes.byref(te32), ctypes.byref(r), ctypes.byref(wg),
                                            ctypes.byref(ft32)) == 0
        assert geo.fa_wmean_sqdist_geometry(_abi.FA_I32, K, ctypes.byref(te64), None, None, ctypes.byref(ft64)) == 0
        assert 8 <= te64.value <= te32.value and te32.value % 8 == 0 and te64.value % 8 == 0
        assert 1 <= r.value <= _abi.PAIR_CHAIN_TERMS and wg.value >= 1
        kp = next(v for v in (8, 16, 32, 64) if K <= v)
        covered = 256 // (kp // min(kp, 16))                 # elements the 256 lanes cover at a time
        for te, ft in ((te32.value, ft32.value), (te64.value, ft64.value)):
            per_tile = -(-te // covered)                     # terms a lane's chain gains per tile, at most
            assert ft >= 1 and ft * per_tile <= r.value, "a chain never exceeds the bound's R"
        assert lib.fa_wmean_sqdist_work(K, 0) == 1
        sizes = [lib.fa_wmean_sqdist_work(K, P) for P in (1, te64.value, te64.value + 1, 10 ** 6, 10 ** 9, 10 ** 11)]
        assert sizes == sorted(sizes) and sizes[0] >= K
        big = ctypes.c_int()
        assert geo.fa_wmean_sqdist_geometry(_abi.FA_F64, K, None, None, ctypes.byref(big), None) == 0
        assert wg.value <= big.value and sizes[-1] == sizes[-2] == big.value * 64, "the grid, and so the scratch, is capped"
    assert lib.fa_wmean_sqdist_work(0, 10) == 0 and lib.fa_wmean_sqdist_work(65, 10) == 0
    assert lib.fa_wmean_sqdist_work(4, -1) == 0
    assert geo.fa_wmean_sqdist_geometry(_abi.FA_I8, 4, None, None, None, None) == _abi.FA_EDTYPE
    assert geo.fa_wmean_sqdist_geometry(_abi.FA_F32, 65, None, None, None, None) == _abi.FA_EINVAL


# ---- the host rule -------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 3, 8, 33, 64])
def test_weiszfeld_weights_equal_a_plain_loop(K):
    rng = np.random.default_rng(K)
    for trial in range(8):
        d = rng.random(K) * 10.0 ** rng.integers(-12, 6, K)
        if trial % 2 and K > 1:
            d[rng.integers(0, K)] = [np.nan, np.inf, 0.0, -np.inf][trial // 2]
        nu = [1e-6, 1e-3, 2.0, 1e-300][trial % 4]
        got = weiszfeld_weights(d, nu)
        assert got.dtype == np.float64 and got.shape == (K,)
        assert [float(v) for v in got] == gr.weights(d, nu), (K, trial)


def test_weiszfeld_weights_edges():
    w = weiszfeld_weights([4.0, np.nan, 0.0, np.inf, 1e-20], 1e-3)
    raw = [1.0 / 2.0, 0.0, 1.0 / 1e-3, 0.0, 1.0 / 1e-3]        # d = 0 and sqrt(d) < nu give 1 / nu
    total = (((raw[0] + raw[1]) + raw[2]) + raw[3]) + raw[4]
    assert [float(v) for v in w] == [v / total for v in raw]
    assert w[1] == 0.0 and w[3] == 0.0, "a non-finite distance has weight 0"
    assert float(weiszfeld_weights([9.0], 1.0)[0]) == 1.0
    for bad in ([np.nan], [np.inf, np.nan, -np.inf], []):
        with pytest.raises(ValueError):
            weiszfeld_weights(bad, 1e-6)
        if bad:
            with pytest.raises(ValueError):
                gr.weights(bad, 1e-6)


# ---- the oracle against the existing ones ---------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.float64, np.float16])
@pytest.mark.parametrize("K", [1, 2, 4, 8, 16, 32, 64])
def test_wmean_at_one_over_K_is_the_plain_mean(K, dt):
    """K a power of two and beta = 1/K: scaling by 2^-k is exact, so ``(u_0 / K + u_1 / K) + ...`` rounds
    where ``(u_0 + u_1 + ...) / K`` does, and wmean equals the trimmed mean at trim 0 bit for bit. That
    rule adds in ascending order of the values, wmean in client order: the updates are therefore sorted
    along the client axis (ascending values are ascending client indices). Values stay within
    [2^-3, 2^3): no product is subnormal."""
    rng = np.random.default_rng(K)
    mag = 2.0 ** rng.uniform(-3, 3, (K, 3, 50))
    S = np.sort((mag * rng.choice([-1.0, 1.0], mag.shape)).astype(dt), axis=0)
    ups = [[S[k], S[k, 0, :7].copy()] for k in range(K)]
    want = rr.combine(ups, 0)
    got = gr.model_wmean(ups, [1.0 / K] * K)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype == np.dtype(dt) and g.shape == w.shape
        assert np.array_equal(g.view(f"u{g.dtype.itemsize}"), w.view(f"u{w.dtype.itemsize}"))


def test_wmean_by_hand():
    S = np.array([[1.0, -0.0], [np.inf, np.nan], [3.0, 0.0], [2.0 ** -24, 5.0]], dtype=np.float32)
    z = gr.wmean(S, [0.5, 0.0, 0.25, 1.0])
    assert z.dtype == np.float32
    # (0.5 * 1 + 0.25 * 3) + 2^-24 = 1.25 + 2^-24 -> 1.25 in float32; -0 + 0 = +0, + 5
    assert z.tolist() == [1.25, 5.0], "the zero-weight client's inf and NaN never reach z"
    assert np.signbit(gr.wmean(S[:1], [2.0])[1]), "the first product starts the sum: -0 stays -0"
    i = gr.wmean(np.array([[2 ** 53 + 1, 7], [3, 1]], dtype=np.int64), [1.0, 0.5])
    assert i.dtype == np.float64 and i.tolist() == [float(2 ** 53) + 2.0, 7.5]      # converted with one rounding
    h = gr.wmean(np.array([[2049.0], [1.0]], dtype=np.float16), [1.0, 1.0])
    assert h.dtype == np.float16 and float(h[0]) == 2048.0                          # 2049 is 2048 in half: 2049 -> half
    with pytest.raises(ValueError):
        gr.wmean(S, [0.0] * 4)


@pytest.mark.parametrize("dt", [np.float32, np.float16, np.float64, np.int32])
def test_dists_is_row_zero_of_the_pairwise_oracle(dt):
    rng = np.random.default_rng(5)
    S = (rng.standard_normal((5, 300)) * 100).astype(dt)
    z = gr.wmean(S, [0.3, 0.0, 0.2, 0.1, 0.4])
    C = kr.compute_dtype(S.dtype)
    want = kr.sqdist(np.concatenate([z.astype(C)[None], S.astype(C)]))[0, 1:]
    got = gr.dists(S, z)
    assert got.dtype == np.float64 and np.array_equal(got, want)
    pre = gr.dists_prefixes(S, z, [7, 300])
    # a longer prefix continues the shorter one's sum: the same exact value, summed in two pieces
    assert np.array_equal(pre[7], gr.dists(S[:, :7], z[:7])) and np.allclose(pre[300], want, rtol=1e-13, atol=0)


# ---- plug-in: parameter validation before any device work -----------------------------------------
def _queue(K=3):
    from fedn_amd.updatehandler import MemoryUpdateHandler
    uh = MemoryUpdateHandler()
    rng = np.random.default_rng(0)
    for k in range(K):
        uh.submit([rng.standard_normal((4, 3)).astype(np.float32)], 10 + k)
    return uh


@pytest.mark.parametrize("parameters", [{"iterations": -1}, {"iterations": 101}, {"iterations": 3.0}, {"iterations": "3"},
                                        {"iterations": True}, {"nu": 0.0}, {"nu": -1e-6}, {"nu": 1}, {"nu": float("nan")},
                                        {"nu": float("inf")}, {"nu": "1e-6"}, {"iterations": 3, "momentum": 0.9},
                                        {"byzantine_fraction": 0.1}],
                         ids=["it_negative", "it_101", "it_float", "it_str", "it_bool", "nu_zero", "nu_negative", "nu_int",
                              "nu_nan", "nu_inf", "nu_str", "unknown_key", "other_rule_key"])
def test_geomedian_refuses_invalid_parameters(parameters, monkeypatch):
    from fedn_amd import ops
    from fedn_amd.aggregators import get_aggregator

    def no_device_work(*a, **kw):
        raise AssertionError("device work after invalid parameters")

    monkeypatch.setattr(ops, "weighted_mean_sqdist", no_device_work)
    monkeypatch.setattr(ops, "pairwise_sqdist", no_device_work)
    uh = _queue()
    stored = set(uh.store.models)
    agg = get_aggregator("geomedian", uh)
    assert agg.name == "geomedian"
    model, data = agg.combine_models(helper=None, parameters=parameters)
    assert model is None and data["nr_aggregated_models"] == 0
    assert "time_model_load" in data and "time_model_aggregation" in data
    assert uh.model_updates.qsize() == 0, "the queue is drained"
    assert set(uh.store.models) == stored, "nothing is deleted"


def test_geomedian_defaults_and_accepted_values():
    from fedn_amd.aggregators import get_aggregator
    agg = get_aggregator("geomedian", _queue(0))
    assert agg._validate_and_merge_parameters(None) == {"iterations": 3, "nu": 1e-6}
    assert agg._validate_and_merge_parameters({"iterations": 0}) == {"iterations": 0, "nu": 1e-6}
    assert agg._validate_and_merge_parameters({"iterations": 100, "nu": 0.5}) == {"iterations": 100, "nu": 0.5}
    assert math.isclose(agg.default_parameters["nu"], 1e-6)


def test_trimmedmean_refusal_unchanged(caplog):
    """The hook the geometric-median plug-in overrides left the trimmed-mean plug-in's refusal as it was."""
    import logging

    from fedn_amd.aggregators import get_aggregator
    with caplog.at_level(logging.ERROR, logger="fedn"):
        model, _ = get_aggregator("trimmedmean", _queue()).combine_models(helper=None, parameters={"trim_fraction": 0.5})
        model2, _ = get_aggregator("geomedian", _queue()).combine_models(helper=None, parameters={"iterations": 101})
    assert model is None and model2 is None
    assert "Parameter trim_fraction must lie in [0, 0.5), got 0.5" in caplog.text
    assert "Parameter iterations must lie in 0..100, got 101" in caplog.text
