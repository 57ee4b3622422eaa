"""Host side of the robust rules (trimmed mean / median): the C ABI's argument validation, the
plug-ins' parameter validation, the trim count, the sorting network, and the oracle against numpy.
No device is touched: every call here returns before any HIP call."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import robust_ref as rr
from fedn_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- C ABI -------------------------------------------------------------------------------------
def test_library_exports_fa_trimmed_mean():
    lib = _abi.load()
    assert "fa_trimmed_mean" in _abi.EXPORTS and hasattr(lib, "fa_trimmed_mean")
    assert lib.fa_abi_version() == _abi.ABI_VERSION
    assert hasattr(_abi.load_probe(), "fa_trimmed_mean")


def _call(out=16, od=_abi.FA_F32, ups=True, ud=_abi.FA_F32, K=4, trim=1, P=10):
    ptrs = _abi.ptr_array([32 + 16 * k for k in range(max(1, min(K, 80)))]) if ups else None
    return _abi.load().fa_trimmed_mean(out, od, ptrs, ud, K, trim, P, None)


@pytest.mark.parametrize("kw", [dict(out=None), dict(ups=False), dict(K=0), dict(K=65), dict(trim=-1),
                                dict(K=4, trim=2), dict(P=-1)],
                         ids=["null_out", "null_updates", "K0", "K65", "trim_neg", "2trim_eq_K", "P_neg"])
def test_argument_errors(kw):
    assert _call(**kw) == _abi.FA_EINVAL
    assert _abi.load().fa_last_error().decode()


def test_dtype_errors():
    assert _call(ud=_abi.FA_I8, od=_abi.FA_F64) == _abi.FA_EDTYPE
    assert _call(ud=_abi.FA_F32, od=_abi.FA_F64) == _abi.FA_EDTYPE
    assert _abi.load().fa_last_error().decode()


def test_empty_is_ok():
    assert _call(P=0) == _abi.FA_OK
    for ud, od in [(_abi.FA_F64, _abi.FA_F64), (_abi.FA_F16, _abi.FA_F16), (_abi.FA_BF16, _abi.FA_F32),
                   (_abi.FA_I32, _abi.FA_F64), (_abi.FA_I64, _abi.FA_F64)]:
        assert _call(ud=ud, od=od, K=64, trim=31, P=0) == _abi.FA_OK


# ---- plug-ins: parameter validation before any device work --------------------------------------
def _queue(K=3):
    from fedn_amd.updatehandler import MemoryUpdateHandler
    uh = MemoryUpdateHandler()
    rng = np.random.default_rng(0)
    for k in range(K):
        uh.submit([rng.standard_normal((4, 3)).astype(np.float32)], 10 + k)
    return uh


@pytest.mark.parametrize("parameters", [{"trim_fraction": 0.5}, {"trim_fraction": -0.1}, {"trim_fraction": 0},
                                        {"trim_fraction": "0.1"}, {"trim_fraction": 0.1, "momentum": 0.9},
                                        {"trim_fraction": float("nan")}],
                         ids=["half", "negative", "int", "str", "unknown_key", "nan"])
def test_trimmedmean_refuses_invalid_parameters(parameters):
    from fedn_amd.aggregators import get_aggregator
    uh = _queue()
    stored = set(uh.store.models)
    model, data = get_aggregator("trimmedmean", uh).combine_models(helper=None, parameters=parameters)
    assert model is None and data["nr_aggregated_models"] == 0
    assert "time_model_load" in data and "time_model_aggregation" in data
    assert uh.model_updates.qsize() == 0, "the queue is drained"
    assert set(uh.store.models) == stored, "nothing is deleted"


def test_median_takes_no_parameters():
    from fedn_amd.aggregators import get_aggregator
    uh = _queue()
    stored = set(uh.store.models)
    model, data = get_aggregator("median", uh).combine_models(helper=None, parameters={"trim_fraction": 0.1})
    assert model is None and data["nr_aggregated_models"] == 0
    assert uh.model_updates.qsize() == 0 and set(uh.store.models) == stored


def test_several_devices_are_refused(monkeypatch):
    """One device only: with FEDN_AMD_DEVICES naming several, every update is logged and skipped
    before any device work, the round is (None, data) and nothing is deleted."""
    from fedn_amd.aggregators.median import Aggregator
    from fedn_amd.robust import RobustPipeline, UnsupportedRound
    monkeypatch.setenv("FEDN_AMD_DEVICES", "cuda:0,cuda:1")
    with pytest.raises(UnsupportedRound):
        RobustPipeline("cuda:0", [np.zeros(3, dtype=np.float32)])
    uh = _queue()
    stored = set(uh.store.models)
    model, data = Aggregator(uh, device="cuda:0").combine_models(helper=None)
    assert model is None and data["nr_aggregated_models"] == 0
    assert uh.model_updates.qsize() == 0 and set(uh.store.models) == stored


@pytest.mark.parametrize("K", [1, 2, 3, 10, 64])
@pytest.mark.parametrize("f", [0.0, 0.1, 0.25, 0.49])
def test_trim_count(K, f):
    from fedn_amd import ops
    from fedn_amd.robust import trim_count
    t = trim_count(f, K)
    assert t == math.floor(f * K) and K - 2 * t >= 1
    assert ops.median_trim(K) == (K - 1) // 2 == rr.median_trim(K) and K - 2 * ops.median_trim(K) in (1, 2)


def test_trim_count_never_trims_everything():
    from fedn_amd.robust import trim_count
    f = np.nextafter(0.5, 0.0)
    for K in range(1, 65):
        assert K - 2 * trim_count(float(f), K) >= 1


# ---- the comparator network (csrc/order_mean.h), on the CPU ---------------------------------------
NET_PROG = r"""
#include <algorithm>
#include <cstdint>
#include <cstdio>
#define FA_ORDER_NET_ONLY
#include "order_mean.h"
static uint64_t s = 88172645463325252ull;
static uint64_t rnd() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
template <int N> int check() {
    const uint64_t cases = N <= 16 ? (1ull << N) : 60000;     // 0-1 principle: exhaustive up to N = 16
    for (uint64_t c = 0; c < cases; ++c) {
        const uint64_t bits = N <= 16 ? c : rnd();
        uint32_t k[N];
        int ones = 0;
        for (int i = 0; i < N; ++i) ones += (k[i] = (bits >> i) & 1);
        order_sort<uint32_t, N>(k);
        for (int i = 0; i < N; ++i) if (k[i] != (uint32_t)(i >= N - ones)) return N;
    }
    for (int c = 0; c < 4000; ++c) {                          // 64-bit keys, with and without ties
        uint64_t k[N], r[N];
        for (int i = 0; i < N; ++i) k[i] = r[i] = (c & 1) ? rnd() % 5 : rnd();
        order_sort<uint64_t, N>(k);
        std::sort(r, r + N);
        for (int i = 0; i < N; ++i) if (k[i] != r[i]) return 1000 + N;
    }
    return 0;
}
int main() {
    const int rc[] = {check<2>(), check<4>(), check<8>(), check<16>(), check<32>(), check<64>()};
    for (int r : rc) if (r) { std::printf("failed %d\n", r); return 1; }
    std::printf("ok\n");
    return 0;
}
"""


def test_sorting_network_sorts(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "a C++ compiler is needed (build() needs one too)"
    src = tmp_path / "net.cpp"
    src.write_text(NET_PROG)
    exe = tmp_path / "net"
    subprocess.run([cxx, "-O1", "-std=c++17", "-I", os.path.join(ROOT, "fedn_amd", "csrc"), str(src), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok"), (r.returncode, r.stdout, r.stderr)


# ---- the oracle against numpy --------------------------------------------------------------------
def _bits_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    nan = np.isnan(a)
    assert np.array_equal(nan, np.isnan(b))
    assert np.array_equal(a[~nan].view(np.uint8), b[~nan].view(np.uint8))


def _data(rng, dt, K, P=37):
    """Mixed-magnitude values without +-0 ties (numpy leaves their order to its sort). P > 1: numpy
    sums the K rows one after the other, as the rule does (a single column it may sum pairwise)."""
    dt = np.dtype(dt)
    if dt.kind == "i":
        lim = 2 ** (8 * dt.itemsize - 2)
        return rng.integers(-lim, lim, (K, P)).astype(dt)
    span = {2: 3, 4: 20, 8: 200}[dt.itemsize]
    x = (rng.standard_normal((K, P)) * 10.0 ** rng.integers(-span, span, (K, P))).astype(dt)
    x[x == 0] = dt.type(1)
    return x


@pytest.mark.parametrize("dt", [np.float32, np.float64, np.float16, np.int32, np.int64], ids=lambda d: np.dtype(d).name)
def test_oracle_equals_numpy(dt):
    rng = np.random.default_rng(np.dtype(dt).itemsize * 7 + (np.dtype(dt).kind == "i"))
    for K in range(1, 65):
        S = _data(rng, dt, K)
        for t in sorted({0, K // 4, (K - 1) // 2}):
            _bits_equal(rr.trimmed_mean(S, t), np.sort(S, axis=0)[t:K - t].mean(axis=0))
        _bits_equal(rr.median(S), np.median(S, axis=0))


@pytest.mark.parametrize("dt", [np.float32, np.float64, np.float16], ids=lambda d: np.dtype(d).name)
def test_oracle_order_rules(dt):
    z, nz, one, inf, nan = (dt(v) for v in (0.0, -0.0, 1.0, np.inf, np.nan))
    # -0 sorts before +0
    s = rr.sorted_values(np.array([[z], [nz], [z], [nz]], dtype=dt))
    assert np.signbit(s[:, 0]).tolist() == [True, True, False, False]
    # a kept run of only -0 gives -0 (the sum starts from the first kept value, not from +0)
    S = np.array([[z], [nz], [-one], [nz], [one], [nz]], dtype=dt)       # sorted: -1 -0 -0 -0 +0 1
    r = rr.trimmed_mean(S, 1)                                             # keeps -0 -0 -0 +0 -> +0
    assert r[0] == 0 and not np.signbit(r[0])
    S = np.array([[nz], [nz], [-one], [nz], [one], [z], [z]], dtype=dt)   # sorted: -1 -0 -0 -0 +0 +0 1
    r = rr.trimmed_mean(S, 1)[0], rr.trimmed_mean(S, 2)[0], rr.median(S)[0]
    assert [bool(np.signbit(v)) for v in r] == [False, False, True] and all(v == 0 for v in r)
    S = np.array([[nz], [-one], [nz], [one]], dtype=dt)                   # median of -1 -0 -0 1: (-0 + -0) / 2
    assert np.signbit(rr.median(S)[0]) and rr.median(S)[0] == 0
    # NaNs (either sign, any payload) sort after +inf and are equal
    negnan = np.array([nan]).view({2: np.uint16, 4: np.uint32, 8: np.uint64}[np.dtype(dt).itemsize])
    negnan = (negnan | negnan.dtype.type(1 << (8 * np.dtype(dt).itemsize - 1)) | negnan.dtype.type(5)).view(dt)[0]
    S = np.array([[nan], [inf], [negnan], [-inf], [one]], dtype=dt)
    s = rr.sorted_values(S)[:, 0]
    assert s[0] == -inf and s[1] == one and s[2] == inf and np.isnan(s[3]) and np.isnan(s[4])
    assert rr.trimmed_mean(S, 2)[0] == inf                               # 2 NaNs, trim 2: none kept
    assert np.isnan(rr.trimmed_mean(S, 1)[0])                            # one NaN kept -> NaN
    assert rr.trimmed_mean(S, 0).dtype == np.dtype(dt)


def test_oracle_integer_rules():
    big = np.array([[2 ** 63 - 1], [-2 ** 63], [2 ** 53 + 1], [0], [-1]], dtype=np.int64)
    s = rr.sorted_values(big)[:, 0]
    assert s.tolist() == [-2 ** 63, -1, 0, 2 ** 53 + 1, 2 ** 63 - 1]
    r = rr.trimmed_mean(big, 0)
    want = ((((np.float64(-2 ** 63) + np.float64(-1)) + np.float64(0)) + np.float64(2 ** 53 + 1)) +
            np.float64(2 ** 63 - 1)) / np.float64(5)
    assert r.dtype == np.float64 and r[0] == want
    assert rr.median(np.array([[3], [1], [2]], dtype=np.int32)).dtype == np.float64
