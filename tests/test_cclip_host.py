"""Host side of the centred-clipping rule: the C ABI's argument validation of ``fa_centered_clip_step``,
``robust.clip_coefficients`` against a plain-Python loop, the oracle tests/cclip_ref.py by hand, and the
plug-in's parameter validation. No device is touched: every library call here returns before any HIP
call."""
import ctypes
import math

import numpy as np
import pytest

import cclip_ref as cr
from fedn_amd import _abi
from fedn_amd.robust import clip_coefficients

SIX = [_abi.FA_F32, _abi.FA_F64, _abi.FA_F16, _abi.FA_BF16, _abi.FA_I32, _abi.FA_I64]
OUT_OF = {_abi.FA_F32: _abi.FA_F32, _abi.FA_F64: _abi.FA_F64, _abi.FA_F16: _abi.FA_F16, _abi.FA_BF16: _abi.FA_F32,
          _abi.FA_I32: _abi.FA_F64, _abi.FA_I64: _abi.FA_F64}
OUT_SIZE = {_abi.FA_F32: 4, _abi.FA_F64: 8, _abi.FA_F16: 2}


# ---- C ABI -------------------------------------------------------------------------------------
def test_library_exports_fa_centered_clip_step():
    lib, probe = _abi.load(), _abi.load_probe()
    for name in ("fa_centered_clip_step", "fa_centered_clip_work"):
        assert name in _abi.EXPORTS and hasattr(lib, name) and hasattr(probe, name)
    # the launch geometry is a measurement entry point: the probe library's alone
    assert "fa_centered_clip_geometry" in _abi.PROBE_EXPORTS and hasattr(probe, "fa_centered_clip_geometry")
    assert "fa_centered_clip_geometry" not in _abi.EXPORTS and not hasattr(lib, "fa_centered_clip_geometry")
    assert lib.fa_abi_version() == _abi.ABI_VERSION >= 12


def _call(out=4096, center=8192, od=None, dist=16, ups=True, ud=_abi.FA_F32, coef="uniform", K=4, P=10, acc=0, work=1 << 20,
          null_at=None):
    """Fake pointers: the call must return before it touches any of them."""
    n = max(1, min(K, 80))
    ptrs = [64 + 16 * k for k in range(n)]
    if null_at is not None:
        ptrs[null_at] = 0
    if isinstance(coef, str):
        coef = [1.0 / n] * n
    od = OUT_OF.get(ud, _abi.FA_F32) if od is None else od
    return _abi.load().fa_centered_clip_step(out, center, od, dist, _abi.ptr_array(ptrs) if ups else None, ud,
                                             _abi.double_array(coef) if coef is not None else None, K, P, acc, work, None)


@pytest.mark.parametrize("kw", [dict(dist=None), dict(center=None), dict(coef=None), dict(ups=False), dict(work=None),
                                dict(null_at=2), dict(K=0), dict(K=65), dict(K=-1), dict(P=-1),
                                dict(coef=[0.5, -0.25, 0.5, 0.25]), dict(coef=[0.5, float("nan"), 0.5, 0.25]),
                                dict(coef=[0.5, float("inf"), 0.5, 0.25]), dict(coef=[1e39, 0.0, 0.0, 0.0]),
                                dict(out=8192 + 4, P=10), dict(out=8192 - 36, P=10), dict(out=8192 + 36, P=10)],
                         ids=["null_dist", "null_center", "null_coef", "null_updates", "null_work", "null_client", "K0",
                              "K65", "K_neg", "P_neg", "coef_negative", "coef_nan", "coef_inf", "coef_inf_in_f32",
                              "overlap_by_one", "overlap_from_below", "overlap_last_element"])
def test_argument_errors(kw):
    assert _call(**kw) == _abi.FA_EINVAL
    assert _abi.load().fa_last_error().decode()


def test_coefficients_are_judged_in_the_compute_type():
    """1e39 is inf as a float32 and a coefficient as a float64: refused for the f32 family only (here with
    accumulate and P = 0, so the accepted call launches nothing)."""
    coef = [1e39, 0.0, 0.5, 0.0]
    for ud in (_abi.FA_F32, _abi.FA_F16, _abi.FA_BF16):
        assert _call(ud=ud, coef=coef, P=0, acc=1) == _abi.FA_EINVAL
    for ud in (_abi.FA_F64, _abi.FA_I32, _abi.FA_I64):
        assert _call(ud=ud, coef=coef, P=0, acc=1) == _abi.FA_OK


@pytest.mark.parametrize("ud", SIX)
def test_all_zero_coefficients_are_legal(ud):
    """Unlike fa_weighted_mean_sqdist: every coefficient 0 is the distances-only pass. Not refused up to
    the first HIP call (accumulate with P = 0 launches nothing); one that is 0 only in f32 neither."""
    for K in (1, 4, 64):
        assert _call(ud=ud, K=K, coef=[0.0] * K, P=0, acc=1) == _abi.FA_OK
        assert _call(ud=ud, K=K, coef=[0.0] * K, P=0, acc=1, out=None) == _abi.FA_OK
    assert _call(ud=ud, coef=[1e-60, 0.0, 1e-50, 0.0], P=0, acc=1) == _abi.FA_OK


@pytest.mark.parametrize("ud", SIX)
def test_overlap_is_judged_in_the_output_type(ud):
    """out = center and disjoint buffers pass the check; anything between is FA_EINVAL. The extent is
    P elements of the OUTPUT type. Probed with K = 65, which is refused first, and with P = 0, where nothing
    overlaps and (accumulate) nothing is launched."""
    size = OUT_SIZE[OUT_OF[ud]]
    P = 100
    c = 1 << 16
    for out in (c + size, c + (P - 1) * size, c - size, c - (P - 1) * size):
        assert _call(ud=ud, out=out, center=c, P=P) == _abi.FA_EINVAL, (ud, out - c)
        assert "overlap" in _abi.load().fa_last_error().decode()
        assert _call(ud=ud, out=out, center=c, P=0, acc=1) == _abi.FA_OK
    # in place and disjoint are refused only for what comes later: a null client pointer
    for out in (c, c + P * size, c - P * size, None):
        assert _call(ud=ud, out=out, center=c, P=P, null_at=1) == _abi.FA_EINVAL
        assert "updates[1] is NULL" in _abi.load().fa_last_error().decode(), (ud, out)


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
    written by a launch: tests/test_gpu_cclip.py.)"""
    for K in (1, 2, 5, 64):
        assert _call(ud=ud, K=K, P=0, acc=1) == _abi.FA_OK
    assert _call(ud=ud, K=3, P=0, acc=1, null_at=1) == _abi.FA_OK, "an empty buffer may be a null pointer"
    assert _call(ud=ud, K=3, P=0, acc=1, out=None) == _abi.FA_OK


def _geometry(dt, K):
    te, r, wg, ft = (ctypes.c_int() for _ in range(4))
    assert _abi.load_probe().fa_centered_clip_geometry(dt, K, ctypes.byref(te), ctypes.byref(r), ctypes.byref(wg),
                                                       ctypes.byref(ft)) == 0
    return te.value, r.value, wg.value, ft.value


def test_work_size_and_geometry():
    lib, geo = _abi.load(), _abi.load_probe()
    for K in (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64):
        geoms = {dt: _geometry(dt, K) for dt in SIX}
        kp = next(v for v in (8, 16, 32, 64) if K <= v)
        covered = 256 // (kp // min(kp, 16))                 # elements the 256 lanes cover at a time
        stride = (K + 1) | 1                                 # K clients and the centre, odd
        for dt, (te, r, wg, ft) in geoms.items():
            csize = 4 if dt in (_abi.FA_F32, _abi.FA_F16, _abi.FA_BF16) else 8
            assert 8 <= te <= 512 and te % 8 == 0
            assert te * stride * csize <= 32768, "the tile with the centre's column fits its LDS"
            assert 1 <= r <= _abi.PAIR_CHAIN_TERMS and wg >= 1
            per_tile = -(-te // covered)                     # terms a lane's chain gains per tile, at most
            assert ft >= 1 and ft * per_tile <= r, "a chain never exceeds the bound's R"
        assert geoms[_abi.FA_I32][0] <= geoms[_abi.FA_F16][0]
        # the centre's column costs tile length: never a longer tile than the Weiszfeld pass's
        wte = ctypes.c_int()
        assert geo.fa_wmean_sqdist_geometry(_abi.FA_F32, K, ctypes.byref(wte), None, None, None) == 0
        assert geoms[_abi.FA_F32][0] <= wte.value
        assert lib.fa_centered_clip_work(K, 0) == 1
        te_min = min(g[0] for g in geoms.values())
        Ps = (1, te_min, te_min + 1, 10 ** 6, 10 ** 9, 10 ** 11)
        sizes = [lib.fa_centered_clip_work(K, P) for P in Ps]
        assert sizes == sorted(sizes) and sizes[0] >= K, "monotone in P"
        for P, size in zip(Ps, sizes):                       # enough for every dtype's grid
            for te, _, wg, _ in geoms.values():
                assert size >= min(-(-P // te), wg) * 64
        cap = max(g[2] for g in geoms.values())
        assert sizes[-1] == sizes[-2] == cap * 64, "the grid, and so the scratch, is capped"
    assert lib.fa_centered_clip_work(0, 10) == 0 and lib.fa_centered_clip_work(65, 10) == 0
    assert lib.fa_centered_clip_work(4, -1) == 0
    assert geo.fa_centered_clip_geometry(_abi.FA_I8, 4, None, None, None, None) == _abi.FA_EDTYPE
    assert geo.fa_centered_clip_geometry(_abi.FA_F32, 65, None, None, None, None) == _abi.FA_EINVAL
    assert geo.fa_centered_clip_geometry(_abi.FA_F32, 0, None, None, None, None) == _abi.FA_EINVAL


# ---- the host rule -------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 3, 8, 33, 64])
def test_clip_coefficients_equal_a_plain_loop(K):
    rng = np.random.default_rng(K)
    for trial in range(12):
        d = rng.random(K) * 10.0 ** rng.integers(-12, 6, K)
        if trial % 2 and K > 1:
            d[rng.integers(0, K)] = [np.nan, np.inf, 0.0, -np.inf, -1.0, -0.0][trial // 2]
        tau = [1e-6, 1e-3, 2.0, 1e-300, 30.0, 1e300][trial % 6]
        got = clip_coefficients(d, tau)
        assert got.dtype == np.float64 and got.shape == (K,)
        assert [float(v) for v in got] == cr.coefficients(d, tau), (K, trial)


def test_clip_coefficients_edges():
    tau = 3.0
    below, above = np.nextafter(9.0, 0.0), np.nextafter(9.0, 10.0)
    d = [0.0, below, 9.0, above, 36.0, np.inf, np.nan, -4.0]
    c = clip_coefficients(d, tau)
    assert [float(v) for v in c] == cr.coefficients(d, tau)
    good = 5.0
    assert c[0] == 1.0 / good and c[1] == 1.0 / good and c[2] == 1.0 / good, "at and below tau^2: not clipped"
    assert c[3] == (3.0 / math.sqrt(above)) / good and c[3] <= c[2]
    assert c[4] == 0.5 / good
    assert c[5] == 0.0 and c[6] == 0.0 and c[7] == 0.0, "a non-finite or negative distance has coefficient 0"
    assert [float(v) for v in clip_coefficients([0.0, 0.0, 0.0], 1.0)] == [1.0 / 3.0] * 3 == cr.coefficients([0.0] * 3, 1.0)
    assert float(clip_coefficients([25.0], 1.0)[0]) == 0.2
    assert float(clip_coefficients([-0.0], 1.0)[0]) == 1.0 == cr.coefficients([-0.0], 1.0)[0]
    for bad in ([np.nan], [np.inf, np.nan, -np.inf], [-1.0], []):
        with pytest.raises(ValueError):
            clip_coefficients(bad, 1.0)
        with pytest.raises(ValueError):
            cr.coefficients(bad, 1.0)


# ---- the oracle by hand ------------------------------------------------------------------------------
def test_step_by_hand():
    v = np.array([1.0, 0.0, -0.0, 2.0], dtype=np.float32)
    S = np.array([[3.0, 1.0, -0.0, 2.0], [np.inf, np.nan, 5.0, 7.0], [1.0, 2.0 ** -24, 0.0, 2.0]], dtype=np.float32)
    z = cr.step(S, v, [0.5, 0.0, 1.0])
    assert z.dtype == np.float32
    # 1 + 0.5 * 2 = 2;  (0 + 0.5 * 1) + 2^-24 = 0.5 + 2^-24 -> 0.5 + 2^-24 (exact in float32);  a client at the centre adds 0
    assert z.tolist() == [2.0, 0.5 + 2.0 ** -24, 0.0, 2.0], "the zero-coefficient client's inf and NaN never reach v'"
    same = cr.step(S, v, [0.0, 0.0, 0.0])
    assert np.array_equal(same.view(np.uint32), v.view(np.uint32)), "every coefficient 0: the centre's bits, -0 included"
    one = cr.step(S[2:], np.zeros(4, dtype=np.float32), [1.0])
    assert np.array_equal(one, S[2]), "K = 1 at coef 1 from a centre of zeros is the client"
    i = cr.step(np.array([[2 ** 53 + 1, 7], [3, 1]], dtype=np.int64), np.array([0.0, 1.0]), [1.0, 0.5])
    assert i.dtype == np.float64 and i.tolist() == [float(2 ** 53) + 2.0, 7.0]      # converted with one rounding
    h = cr.step(np.array([[2049.0]], dtype=np.float16), np.array([0.0], dtype=np.float16), [1.0])
    assert h.dtype == np.float16 and float(h[0]) == 2048.0
    with pytest.raises(AssertionError):
        cr.step(np.zeros((1, 2), dtype=np.int32), np.zeros(2, dtype=np.float32), [1.0])   # the centre is not in O


def test_cclip_f64_moves_at_most_tau_over_k():
    """The rule's promise, on the float64 run: a hostile client moves the point by at most tau / K a step."""
    rng = np.random.default_rng(3)
    K, n, tau = 6, 50, 0.5
    center = [np.zeros(n)]
    ups = [[0.01 * rng.standard_normal(n)] for _ in range(K - 1)]
    _, clean = cr.cclip_f64(ups + [[np.zeros(n)]], center, 1, tau)
    trace, hit = cr.cclip_f64(ups + [[1e6 * np.ones(n)]], center, 1, tau)
    assert len(trace) == 2 and not trace[0][0].any()
    assert np.linalg.norm(hit - clean) <= tau / K * (1 + 1e-12)
    trace0, v0 = cr.cclip_f64(ups, center, 0, tau)
    assert len(trace0) == 1 and not v0.any(), "no step: the centre"


# ---- plug-in: parameter validation before any device work -----------------------------------------
def _queue(K=3):
    from fedn_amd.updatehandler import MemoryUpdateHandler
    uh = MemoryUpdateHandler()
    rng = np.random.default_rng(0)
    gid = uh.put_global_model([rng.standard_normal((4, 3)).astype(np.float32)])
    for k in range(K):
        uh.submit([rng.standard_normal((4, 3)).astype(np.float32)], 10 + k, model_id=gid)
    return uh


@pytest.mark.parametrize("parameters", [None, {}, {"iterations": 3}, {"tau": 1.0, "iterations": -1},
                                        {"tau": 1.0, "iterations": 101}, {"tau": 1.0, "iterations": 3.0},
                                        {"tau": 1.0, "iterations": "3"}, {"tau": 1.0, "iterations": True}, {"tau": 0.0},
                                        {"tau": -1.0}, {"tau": 1}, {"tau": float("nan")}, {"tau": float("inf")},
                                        {"tau": "1.0"}, {"tau": 1.0, "momentum": 0.9}, {"tau": 1.0, "nu": 1e-6}],
                         ids=["none", "empty", "tau_missing", "it_negative", "it_101", "it_float", "it_str", "it_bool",
                              "tau_zero", "tau_negative", "tau_int", "tau_nan", "tau_inf", "tau_str", "unknown_key",
                              "other_rule_key"])
def test_centeredclip_refuses_invalid_parameters(parameters, monkeypatch):
    from fedn_amd import ops
    from fedn_amd.aggregators import get_aggregator

    def no_device_work(*a, **kw):
        raise AssertionError("device work after invalid parameters")

    monkeypatch.setattr(ops, "centered_clip_step", no_device_work)
    uh = _queue()
    stored = set(uh.store.models)
    agg = get_aggregator("centeredclip", uh)
    assert agg.name == "centeredclip"
    model, data = agg.combine_models(helper=None, parameters=parameters)
    assert model is None and data["nr_aggregated_models"] == 0
    assert "time_model_load" in data and "time_model_aggregation" in data
    assert uh.model_updates.qsize() == 0, "the queue is drained"
    assert set(uh.store.models) == stored, "nothing is deleted"


def test_centeredclip_defaults_and_accepted_values():
    from fedn_amd.aggregators import get_aggregator
    agg = get_aggregator("centeredclip", _queue(0))
    assert agg._validate_and_merge_parameters({"tau": 2.5}) == {"iterations": 3, "tau": 2.5}
    assert agg._validate_and_merge_parameters({"tau": 1e-9, "iterations": 0}) == {"iterations": 0, "tau": 1e-9}
    assert agg._validate_and_merge_parameters({"iterations": 100, "tau": 0.5}) == {"iterations": 100, "tau": 0.5}
    assert "tau" not in agg.default_parameters, "tau has the model's scale: no default"


def test_other_rules_unchanged_by_the_hook(caplog):
    """The hook the centred-clipping plug-in overrides left the other plug-ins' refusals as they were."""
    import logging

    from fedn_amd.aggregators import get_aggregator
    with caplog.at_level(logging.ERROR, logger="fedn"):
        model, _ = get_aggregator("trimmedmean", _queue()).combine_models(helper=None, parameters={"trim_fraction": 0.5})
        model2, _ = get_aggregator("centeredclip", _queue()).combine_models(helper=None, parameters={"iterations": 2})
    assert model is None and model2 is None
    assert "Parameter trim_fraction must lie in [0, 0.5), got 0.5" in caplog.text
    assert "Parameter tau is required" in caplog.text
