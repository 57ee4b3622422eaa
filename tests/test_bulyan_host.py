"""Host side of Bulyan: the C ABI's argument validation of ``fa_median_window_mean``, the window-start
function of csrc/median_window.h compiled for the CPU against the oracle tests/bulyan_ref.py, the oracle
against itself, the selection ``robust.bulyan_select`` against the brute-force oracle, the Byzantine count,
and the plug-in's parameter validation. No device is touched: every call here returns before any HIP
call."""
import itertools
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import bulyan_ref as br
import krum_ref as kr
import robust_ref as rr
from fedn_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(_abi.FA_F32, _abi.FA_F32), (_abi.FA_F64, _abi.FA_F64), (_abi.FA_F16, _abi.FA_F16), (_abi.FA_BF16, _abi.FA_F32),
         (_abi.FA_I32, _abi.FA_F64), (_abi.FA_I64, _abi.FA_F64)]


# ---- C ABI -------------------------------------------------------------------------------------
def test_library_exports_fa_median_window_mean():
    lib, probe = _abi.load(), _abi.load_probe()
    assert "fa_median_window_mean" in _abi.EXPORTS
    assert hasattr(lib, "fa_median_window_mean") and hasattr(probe, "fa_median_window_mean")
    assert lib.fa_abi_version() == _abi.ABI_VERSION >= 13


def _call(out=16, od=_abi.FA_F32, ups=True, ud=_abi.FA_F32, K=4, keep=2, P=10, null_at=None):
    """Fake pointers: the call must return before it touches any of them."""
    ptrs = [32 + 16 * k for k in range(max(1, min(K, 80)))]
    if null_at is not None:
        ptrs[null_at] = 0
    return _abi.load().fa_median_window_mean(out, od, _abi.ptr_array(ptrs) if ups else None, ud, K, keep, P, None)


@pytest.mark.parametrize("kw", [dict(out=None), dict(ups=False), dict(null_at=2), dict(K=0, keep=1), dict(K=65, keep=1),
                                dict(K=-1, keep=1), dict(keep=0), dict(K=4, keep=5), dict(keep=-1), dict(P=-1)],
                         ids=["null_out", "null_updates", "null_client", "K0", "K65", "K_neg", "keep0", "keep_gt_K",
                              "keep_neg", "P_neg"])
def test_argument_errors(kw):
    assert _call(**kw) == _abi.FA_EINVAL
    assert "fa_median_window_mean" in _abi.load().fa_last_error().decode()


def test_dtype_errors():
    codes = list(range(-1, 12)) + [99]
    bad = [(ud, od) for ud in codes for od in codes if (ud, od) not in PAIRS]
    assert len(bad) == len(codes) ** 2 - 6
    for ud, od in bad:
        assert _call(ud=ud, od=od) == _abi.FA_EDTYPE, (ud, od)
        assert _abi.load().fa_last_error().decode()
        assert _call(ud=ud, od=od, P=0) == _abi.FA_EDTYPE, (ud, od)
    for ud, od in bad[::7]:                                   # the argument checks come first
        assert _call(ud=ud, od=od, K=65) == _abi.FA_EINVAL
        assert _call(ud=ud, od=od, keep=0) == _abi.FA_EINVAL
        assert _call(ud=ud, od=od, P=-1) == _abi.FA_EINVAL
        assert _call(ud=ud, od=od, out=None) == _abi.FA_EINVAL


@pytest.mark.parametrize("ud,od", PAIRS)
def test_empty_is_ok(ud, od):
    for K, keep in [(1, 1), (4, 1), (4, 3), (4, 4), (64, 34), (64, 64)]:
        assert _call(ud=ud, od=od, K=K, keep=keep, P=0) == _abi.FA_OK


# ---- the window-start function (csrc/median_window.h), on the CPU ---------------------------------
WINDOW_PROG = r"""
#include <cstdint>
#include <cstdio>
#include <vector>
#define FA_ORDER_NET_ONLY
#include "order_mean.h"
#include "median_window.h"
struct Ident { template <typename X> X operator()(X x) const { return x; } };
// a group: theta, keep, n, then n medians, then theta rows of n sorted values (column c is one case)
template <typename A, int KP> void run(int theta, int keep, int n, const A* med, const A* s) {
    for (int c = 0; c < n; ++c) {
        A slot[KP];
        for (int j = 0; j < KP; ++j) slot[j] = j < theta ? s[(size_t)j * n + c] : (A)12345;   // padding: never read
        std::printf("%d\n", window_start<A, KP>(slot, theta, keep, med[c], Ident{}));
    }
}
template <typename A> int all(FILE* f) {
    int32_t h[3];
    while (std::fread(h, sizeof(int32_t), 3, f) == 3) {
        const int theta = h[0], keep = h[1], n = h[2];
        std::vector<A> med(n), s((size_t)theta * n);
        if (std::fread(med.data(), sizeof(A), n, f) != (size_t)n) return 2;
        if (std::fread(s.data(), sizeof(A), s.size(), f) != s.size()) return 2;
        if (theta <= 2) run<A, 2>(theta, keep, n, med.data(), s.data());
        else if (theta <= 4) run<A, 4>(theta, keep, n, med.data(), s.data());
        else if (theta <= 8) run<A, 8>(theta, keep, n, med.data(), s.data());
        else if (theta <= 16) run<A, 16>(theta, keep, n, med.data(), s.data());
        else if (theta <= 32) run<A, 32>(theta, keep, n, med.data(), s.data());
        else run<A, 64>(theta, keep, n, med.data(), s.data());
    }
    return 0;
}
int main(int argc, char** argv) {
    FILE* f = std::fopen(argv[2], "rb");
    if (!f) return 3;
    return argv[1][0] == '4' ? all<float>(f) : all<double>(f);
}
"""


@pytest.fixture(scope="module")
def window_exe(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "a C++ compiler is needed (build() needs one too)"
    d = tmp_path_factory.mktemp("window")
    src = d / "window.cpp"
    src.write_text(WINDOW_PROG)
    exe = d / "window"
    subprocess.run([cxx, "-O1", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "fedn_amd", "csrc"), str(src),
                    "-o", str(exe)], check=True)
    return exe


def _exhaustive_groups(dt, alphabet):
    """Every (theta, keep) with theta <= 9: every sorted sequence over ``alphabet`` (given in the rule's
    order) as one column."""
    for theta in range(1, 10):
        cols = np.array(list(itertools.combinations_with_replacement(alphabet, theta)), dtype=dt).T
        for keep in range(1, theta + 1):
            yield cols, keep


def _random_groups(dt, rng):
    for theta in (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64):
        S = (rng.standard_normal((theta, 40)) * 10.0 ** rng.integers(-3, 4, (theta, 40))).astype(dt)
        S[:, 1] = np.round(S[:, 1])                           # ties between differences
        S[:, 2] = 1.5                                         # all equal
        S[: theta // 2, 3] = -0.0
        S[theta // 2:, 3] = 0.0
        S[: theta // 3, 4] = np.nan                           # a minority / a majority of NaNs
        S[: theta // 2 + 1, 5] = np.nan
        S[0, 6], S[-1, 6] = np.inf, -np.inf
        S[: theta // 2 + 1, 7] = np.inf
        s = rr.sorted_values(S)
        fmax = (theta - 3) // 4 if theta >= 3 else 0
        for keep in sorted({1, 2, theta - 2, theta - 1, theta, theta - 2 * fmax} & set(range(1, theta + 1))):
            yield s, keep


def _groups(dt):
    inf, nan = np.inf, np.nan
    yield from _exhaustive_groups(dt, [-2.0, -1.0, 0.0, 1.0, 2.0])
    yield from _exhaustive_groups(dt, [-inf, -1.0, 1.0, inf, nan])
    yield from _exhaustive_groups(dt, [-1.0, -0.0, 0.0, 0.5])
    yield from _random_groups(dt, np.random.default_rng(np.dtype(dt).itemsize))


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_window_start_function_equals_oracle(dt, window_exe, tmp_path):
    """The function the kernel calls, compiled for the CPU on already converted A values, gives the oracle's
    greedy window start; the oracle's counting form agrees with its greedy form on the same cases."""
    want = []
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        for s, keep in _groups(dt):
            a = br.window_start(s, keep)
            assert np.array_equal(a, br.window_start_count(s, keep)), (s.shape[0], keep)
            assert a.min() >= 0 and a.max() <= s.shape[0] - keep
            want.append(a)
            f.write(np.array([s.shape[0], keep, s.shape[1]], dtype=np.int32).tobytes())
            f.write(br.median_acc(s).astype(dt).tobytes())
            f.write(np.ascontiguousarray(s).tobytes())
    r = subprocess.run([str(window_exe), str(np.dtype(dt).itemsize), str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    got = np.array(r.stdout.split(), dtype=np.int64)
    want = np.concatenate(want)
    assert got.shape == want.shape and want.size > 20000
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    assert want.max() > 0 and (want == 0).any()


# ---- the oracle against itself --------------------------------------------------------------------
def _bits_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    nan = np.isnan(a)
    assert np.array_equal(nan, np.isnan(b))
    assert np.array_equal(a[~nan].view(np.uint8), b[~nan].view(np.uint8))


@pytest.mark.parametrize("dt", [np.float32, np.float64, np.float16, np.int32, np.int64], ids=lambda d: np.dtype(d).name)
def test_full_window_is_the_trimmed_mean_at_trim_0(dt):
    rng = np.random.default_rng(11)
    for theta in (1, 2, 3, 7, 16, 33, 64):
        if np.dtype(dt).kind == "i":
            S = rng.integers(-2 ** 40 if dt == np.int64 else -2 ** 30, 2 ** 30, (theta, 50)).astype(dt)
        else:
            S = (rng.standard_normal((theta, 50)) * 10.0 ** rng.integers(-2, 3, (theta, 50))).astype(dt)
            S[0, 0], S[-1, 1], S[0, 2] = np.nan, np.inf, -0.0
        _bits_equal(br.window_mean(S, theta), rr.trimmed_mean(S, 0))
        assert br.window_mean(S, 1).dtype == rr.out_dtype(dt)


@pytest.mark.parametrize("dt", [np.int32, np.int64, np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_window_is_the_closest_values_to_the_median(dt):
    """Small integers, nothing rounds; columns without ties among |s - med|: the window is the brute-force
    set of the ``keep`` values closest to the median, and the result their exact mean."""
    rng = np.random.default_rng(5)
    checked = 0
    for theta in range(1, 18):
        S = rng.integers(-1000, 1000, (theta, 300))
        s = np.sort(S, axis=0)
        med = np.median(s, axis=0)
        dist = np.abs(s - med)
        ok = np.array([len(set(dist[:, c])) == theta and len(set(s[:, c])) == theta for c in range(S.shape[1])])
        s, dist = s[:, ok], dist[:, ok]
        for keep in range(1, theta + 1):
            a = br.window_start(s.astype(dt), keep)
            assert np.array_equal(a, br.window_start_count(s.astype(dt), keep))
            got = br.window_mean(S[:, ok].astype(dt), keep)
            for c in range(s.shape[1]):
                near = sorted(s[np.argsort(dist[:, c])[:keep], c].tolist())
                assert s[a[c]:a[c] + keep, c].tolist() == near, (theta, keep, c)
                assert got[c] == rr.out_dtype(dt).type(sum(near)) / rr.out_dtype(dt).type(keep)
                checked += 1
    assert checked > 5000


def test_window_hand_written():
    f = np.float32
    S = np.array([[0], [1], [2], [10], [11]], dtype=f)                  # med 2: the closest three are 0 1 2
    assert br.window_start(S, 3)[0] == 0 and br.window_mean(S, 3)[0] == f(1)
    S = np.array([[-9], [1], [2], [3], [4]], dtype=f)                   # med 2: 1 2 3
    assert br.window_start(S, 3)[0] == 1 and br.window_mean(S, 3)[0] == f(2)
    S = np.array([[0], [1], [2], [3], [4]], dtype=f)                    # a tie keeps the lower window
    assert br.window_start(S, 3)[0] == 1 and br.window_start(S, 2)[0] == 1 and br.window_start(S, 4)[0] == 0
    S = np.array([[1], [2], [3], [np.nan], [np.nan]], dtype=f)          # med 3; a NaN neighbour stops the walk
    assert br.window_start(S, 2)[0] == 1 and br.window_mean(S, 2)[0] == f(2.5)
    S = np.array([[1], [2], [np.nan], [np.nan], [np.nan]], dtype=f)     # a NaN median: the window stays at 0
    assert br.window_start(S, 2)[0] == 0 and br.window_mean(S, 2)[0] == f(1.5)
    S = np.array([[1], [3], [4], [8]], dtype=np.int64)                  # even theta: med 3.5 is kept in A
    assert br.median_acc(S)[0] == 3.5 and br.window_start(S, 2)[0] == 1 and br.window_mean(S, 2)[0] == 3.5
    S = np.array([[1], [2 ** 53 + 2], [2 ** 53 + 4], [2 ** 62]], dtype=np.int64)
    assert br.window_mean(S, 2).dtype == np.float64 and br.window_mean(S, 2)[0] == float(2 ** 53 + 3) == 2.0 ** 53 + 4


# ---- selection ------------------------------------------------------------------------------------
def _points_matrix(rng, K, ties):
    """D of K random points; with ``ties`` on a small integer grid with duplicated clients, so rows and
    columns repeat and scores tie exactly."""
    if ties:
        X = rng.integers(0, 3, (K, 2)).astype(np.float64)
        for _ in range(K // 3):
            X[rng.integers(0, K)] = X[rng.integers(0, K)]
    else:
        X = rng.standard_normal((K, 5)) * 10.0 ** rng.integers(-2, 3)
    return ((X[:, None, :] - X[None, :, :]) ** 2).sum(axis=2)


def _same_selection(D, f):
    from fedn_amd.robust import bulyan_select
    try:
        want = br.select(D.tolist(), f)
    except ValueError:
        with pytest.raises(ValueError):
            bulyan_select(D, f)
        return None
    sel, order, scores = bulyan_select(D, f)
    assert (sel, order, scores) == want
    theta = D.shape[0] - 2 * f
    assert sel == sorted(order) and len(set(sel)) == theta == len(scores)
    assert all(isinstance(i, int) for i in sel) and all(math.isfinite(v) for v in scores)
    return sel


@pytest.mark.parametrize("K", range(1, 65))
def test_bulyan_select_equals_brute_force(K):
    rng = np.random.default_rng(1000 + K)
    fmax = (K - 3) // 4 if K >= 3 else 0
    fs = sorted({0, 1, fmax} & set(range(fmax + 1))) if K <= 24 else [fmax]
    raised = 0
    for trial in range(4 if K <= 24 else 2):
        D = _points_matrix(rng, K, ties=trial % 2 == 0)
        if trial >= 2:                                        # clients with non-finite distances
            for bad in rng.choice(K, size=min(K, 1 + trial % 2 + K // 16), replace=False):
                D[bad, :] = D[:, bad] = np.nan if trial == 2 else np.inf
                D[bad, bad] = 0.0
        for f in fs:
            sel = _same_selection(D, f)
            raised += sel is None
            if sel is not None and f == 0:
                assert sel == list(range(K)), "f = 0 selects everyone"
            if sel is not None and trial >= 2:
                assert np.isfinite(D[np.ix_(sel, sel)]).all(), "a non-finite client is never selected"
    if K == 1:
        assert raised == 0                                    # (from K = 2 on a non-finite client leaves f = 0 nothing)


def test_bulyan_select_hand_written():
    from fedn_amd.robust import bulyan_select
    assert bulyan_select([[0.0]], 0) == ([0], [0], [0.0])
    # K = 7, f = 1: theta = 5. Clients on a line at 0 1 2 3 4 5 and one at 100.
    x = np.array([0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 100.0])
    D = (x[:, None] - x[None, :]) ** 2
    sel, order, scores = bulyan_select(D, 1)
    assert (sel, order, scores) == br.select(D.tolist(), 1)
    assert 6 not in sel and len(sel) == 5
    assert order[0] == 2 and scores[0] == 1.0 + 1.0 + 4.0 + 4.0     # nn = 4: 2 and 3 tie, the lower index wins
    # duplicated clients: all scores tie at every iteration, the picks go in FIFO order
    D = np.zeros((7, 7))
    assert bulyan_select(D, 1) == ([0, 1, 2, 3, 4], [0, 1, 2, 3, 4], [0.0] * 5)
    # too many non-finite clients: nothing trustworthy is left
    D = (x[:, None] - x[None, :]) ** 2
    for bad in (0, 3, 5):
        D[bad, :] = D[:, bad] = np.nan
    with pytest.raises(ValueError):
        bulyan_select(D, 1)
    with pytest.raises(ValueError):
        br.select(D.tolist(), 1)
    with pytest.raises(ValueError):
        bulyan_select(np.zeros((3, 4)), 0)                    # not square
    with pytest.raises(ValueError):
        bulyan_select(np.zeros((6, 6)), 1)                    # K < 4f + 3


@pytest.mark.parametrize("fraction", [0.0, 0.1, 0.2, 0.24, float(np.nextafter(0.25, 0.0))])
def test_byzantine_count(fraction):
    from fedn_amd.robust import bulyan_f
    for K in range(1, 65):
        f = bulyan_f(fraction, K)
        assert f == br.byzantine_count(fraction, K)
        if K < 3:
            assert f == 0
        else:
            assert f == min(math.floor(fraction * K), (K - 3) // 4) and K >= 4 * f + 3
        theta, beta = K - 2 * f, K - 4 * f
        assert theta >= beta >= (3 if f else 1)
    assert [bulyan_f(0.2, K) for K in (3, 6, 7, 10, 11, 23, 64)] == [0, 0, 1, 1, 2, 4, 12]
    assert [bulyan_f(0.24, K) for K in (7, 11, 15, 64)] == [1, 2, 3, 15]


# ---- plug-in: parameter validation before any device work -----------------------------------------
def _queue(K=3):
    from fedn_amd.updatehandler import MemoryUpdateHandler
    uh = MemoryUpdateHandler()
    rng = np.random.default_rng(0)
    for k in range(K):
        uh.submit([rng.standard_normal((4, 3)).astype(np.float32)], 10 + k)
    return uh


@pytest.mark.parametrize("parameters", [{"byzantine_fraction": 0.25}, {"byzantine_fraction": 0.3}, {"byzantine_fraction": -0.1},
                                        {"byzantine_fraction": float("nan")}, {"byzantine_fraction": 0},
                                        {"byzantine_fraction": "0.1"}, {"byzantine_fraction": 0.1, "momentum": 0.9},
                                        {"trim_fraction": 0.1}],
                         ids=["quarter", "above", "negative", "nan", "int", "str", "unknown_key", "other_rule_key"])
def test_bulyan_refuses_invalid_parameters(parameters, monkeypatch):
    from fedn_amd import ops
    from fedn_amd.aggregators import get_aggregator

    def no_device_work(*a, **kw):
        raise AssertionError("device work after invalid parameters")

    for name in ("pairwise_sqdist", "trimmed_mean", "median_window_mean"):
        monkeypatch.setattr(ops, name, no_device_work)
    uh = _queue()
    stored = set(uh.store.models)
    agg = get_aggregator("bulyan", uh)
    assert agg.name == "bulyan"
    model, data = agg.combine_models(helper=None, parameters=parameters)
    assert model is None and data["nr_aggregated_models"] == 0
    assert "time_model_load" in data and "time_model_aggregation" in data
    assert uh.model_updates.qsize() == 0, "the queue is drained"
    assert set(uh.store.models) == stored, "nothing is deleted"


def test_fraction_bound_is_the_plug_ins_own(caplog):
    import logging

    from fedn_amd.aggregators import get_aggregator
    from fedn_amd.exceptions import InvalidParameterError
    bul, mk = get_aggregator("bulyan", _queue()), get_aggregator("multikrum", _queue())
    assert bul._validate_and_merge_parameters(None) == {"byzantine_fraction": 0.2}
    assert bul._validate_and_merge_parameters({"byzantine_fraction": 0.24}) == {"byzantine_fraction": 0.24}
    assert mk._validate_and_merge_parameters({"byzantine_fraction": 0.3}) == {"byzantine_fraction": 0.3}
    with pytest.raises(InvalidParameterError):
        bul._validate_and_merge_parameters({"byzantine_fraction": 0.3})
    with caplog.at_level(logging.ERROR, logger="fedn"):
        bul.combine_models(helper=None, parameters={"byzantine_fraction": 0.25})
        mk.combine_models(helper=None, parameters={"byzantine_fraction": 0.5})
    assert "Parameter byzantine_fraction must lie in [0, 0.25), got 0.25" in caplog.text
    assert "Parameter byzantine_fraction must lie in [0, 0.5), got 0.5" in caplog.text
