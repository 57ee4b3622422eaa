"""Host side of the DP-FedAvg noise: the numpy restatement tests/dpnoise_ref.py against
Philox4x32-10's known answers, the kernel's own generator (fedn_amd/csrc/dp_noise.h compiled for the CPU)
against the restatement, the C ABI's argument validation of ``fa_gaussian_noise``, the restatement's
statistics, and the plug-in's parameter validation. No device is touched: every library call here returns
before any HIP call."""
import logging
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import dpnoise_ref as dr
from fedn_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x0123456789ABCDEF
I63 = (1 << 63) - 1


# ---- the definition ------------------------------------------------------------------------------
KNOWN = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
         ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
         ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
          "d16cfe09 94fdcceb 5001e420 24126ea1")]


@pytest.mark.parametrize("ctr,key,want", KNOWN, ids=["zeros", "ones", "pi"])
def test_known_answers(ctr, key, want):
    got = dr.philox4x32_10(ctr, key)
    assert " ".join(f"{int(w):08x}" for w in got) == want


def test_bits_place_index_stream_round_and_seed():
    """``bits`` is Philox at ctr = (lo(i), hi(i), stream, round), key = (lo(seed), hi(seed))."""
    i, seed = 0x85A308D3243F6A88, 0x299F31D0A4093822
    got = dr.bits(seed, 0x13198A2E, 0x03707344, [i])
    assert " ".join(f"{int(w[0]):08x}" for w in got) == KNOWN[2][2]


def test_uniforms_are_exact_and_in_range():
    full, zero = np.array([0xFFFFFFFF], dtype=np.uint32), np.array([0], dtype=np.uint32)
    u1, u2 = dr.uniforms((full, full, full, full))
    assert u1[0] == 1.0 and u2[0] == 1.0 - 2.0 ** -53
    u1, u2 = dr.uniforms((zero, zero, zero, zero))
    assert u1[0] == 2.0 ** -53 and u2[0] == 0.0
    assert float(dr.radius(np.float64(2.0 ** -53))) < dr.Z_MAX, "|z| <= 8.58"
    u1, u2 = dr.uniforms((np.array([1 << 5]), np.array([3 << 6]), np.array([5 << 5 | 31]), np.array([63])))
    assert u1[0] == (2 ** 26 + 3 + 1) * 2.0 ** -53 and u2[0] == (5 * 2 ** 26) * 2.0 ** -53
    assert dr.TWO_PI == 2.0 * math.pi


def test_apply_rounds_once():
    """float16 straight from float64: 1 + 2^-11 + 2^-30 lies above the midpoint of 1 and 1 + 2^-10 and
    rounds up; through float32 (which drops the 2^-30) it would be a tie and round down to even."""
    z = np.array([2.0 ** -11 + 2.0 ** -30])
    x = np.array([1.0], dtype=np.float16)
    assert float(dr.apply(x, 1.0, z, np.float16)[0]) == 1.0 + 2.0 ** -10
    assert float((x.astype(np.float64) + z).astype(np.float32).astype(np.float16)[0]) == 1.0
    assert dr.apply(None, 1.0, z, np.float64)[0] == z[0]
    assert dr.apply(None, 3.0, z, np.float32).dtype == np.float32


# ---- the kernel's generator, compiled for the CPU ------------------------------------------------
GEN_PROG = r"""
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#define FA_DP_NOISE_GEN_ONLY
#include "dp_noise.h"
// stdin: lines of "seed stream round index" (decimal); stdout: the four words and the two uniforms (hex floats)
int main() {
    uint64_t seed, i;
    uint32_t stream, round;
    while (std::scanf("%" SCNu64 " %" SCNu32 " %" SCNu32 " %" SCNu64, &seed, &stream, &round, &i) == 4) {
        uint32_t x[4];
        dp_noise_bits(x, seed, stream, round, i);
        std::printf("%08x %08x %08x %08x %a %a\n", x[0], x[1], x[2], x[3], dp_uniform_open0(x[0], x[1]),
                    dp_uniform_open1(x[2], x[3]));
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def gen_exe(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "a C++ compiler is needed (build() needs one too)"
    d = tmp_path_factory.mktemp("dpnoise")
    src = d / "gen.cpp"
    src.write_text(GEN_PROG)
    exe = d / "gen"
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-ffp-contract=off", "-I", os.path.join(ROOT, "fedn_amd", "csrc"),
                    str(src), "-o", str(exe)], check=True)
    return exe


def test_header_generator_equals_restatement(gen_exe):
    """dp_noise.h's generator and uniform conversions, compiled for the host: the restatement's bits and
    uniforms exactly, at the indices where the counter's words change and across seeds, streams and rounds."""
    indices = [0, 1, (1 << 32) - 1, 1 << 32, I63]
    seeds = [0, 1, SEED, (1 << 64) - 1, 0xFFFFFFFF00000000]
    cases = [(s, st, r, i) for s in seeds for st, r in [(0, 0), (1, 0), (0, 1), (7, 0xFFFFFFFF), (0xFFFFFFFF, 3)]
             for i in indices]
    cases += [(0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF)]       # the second known answer
    text = "".join(f"{s} {st} {r} {i}\n" for s, st, r, i in cases)
    out = subprocess.run([str(gen_exe)], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    assert len(out) == len(cases) + 1
    assert out[len(cases) - 1].split()[:4] == KNOWN[1][2].split()
    for (s, st, r, i), line in zip(cases, out):
        f = line.split()
        x = dr.bits(s, st, r, np.array([i], dtype=np.uint64))
        assert [int(w, 16) for w in f[:4]] == [int(w[0]) for w in x], (s, st, r, i)
        u1, u2 = dr.uniforms(x)
        assert float.fromhex(f[4]) == u1[0] and float.fromhex(f[5]) == u2[0], (s, st, r, i)
        assert 0.0 < u1[0] <= 1.0 and 0.0 <= u2[0] < 1.0


# ---- statistics of the restatement ---------------------------------------------------------------
def test_restatement_statistics():
    """2^20 deviates at the issue's seed against N(0, 1): |mean| < 4 / sqrt(n), |std - 1| < 4 / sqrt(2n) (four
    standard errors of each estimate), Kolmogorov-Smirnov D sqrt(n) < 1.63 (the 1 % point)."""
    n = 1 << 20
    z, u1 = dr.deviates(SEED, 0, 0, np.arange(n))
    mean, std, ks = dr.statistics(z)
    print(f"restatement: mean {mean:.3e}, std {std:.5f}, KS D*sqrt(n) {ks:.3f}, max |z| {np.abs(z).max():.3f}")
    assert abs(mean) < 4.0 / math.sqrt(n)
    assert abs(std - 1.0) < 4.0 / math.sqrt(2.0 * n)
    assert ks < 1.63
    assert np.abs(z).max() <= dr.Z_MAX and np.isfinite(z).all()


# ---- C ABI ---------------------------------------------------------------------------------------
def test_library_exports_fa_gaussian_noise():
    lib, probe = _abi.load(), _abi.load_probe()
    assert "fa_gaussian_noise" in _abi.EXPORTS and hasattr(lib, "fa_gaussian_noise") and hasattr(probe, "fa_gaussian_noise")
    assert lib.fa_abi_version() == _abi.ABI_VERSION >= 14


def _call(out=4096, x="out", dtype=_abi.FA_F32, sigma=1.0, seed=SEED, stream_id=0, round_id=0, offset=0, P=10):
    """Fake pointers: the call must return before it touches any of them."""
    x = out if isinstance(x, str) else x
    return _abi.load().fa_gaussian_noise(out, x, dtype, sigma, seed, stream_id, round_id, offset, P, None)


@pytest.mark.parametrize("kw", [dict(out=None, x=None), dict(P=-1), dict(offset=-1), dict(offset=I63 - 9),
                                dict(offset=I63, P=1), dict(sigma=-1.0), dict(sigma=-1e-300), dict(sigma=float("nan")),
                                dict(sigma=float("inf")), dict(x=4096 + 4), dict(x=4096 - 36), dict(x=4096 + 36),
                                dict(dtype=_abi.FA_F64, x=4096 + 72), dict(dtype=_abi.FA_F16, x=4096 - 18)],
                         ids=["null_out", "P_neg", "offset_neg", "offset_plus_P_overflows", "offset_max", "sigma_negative",
                              "sigma_tiny_negative", "sigma_nan", "sigma_inf", "overlap_by_one", "overlap_from_below",
                              "overlap_last_element", "overlap_f64", "overlap_f16"])
def test_argument_errors(kw):
    assert _call(**kw) == _abi.FA_EINVAL
    assert _abi.load().fa_last_error().decode()


@pytest.mark.parametrize("dtype", [_abi.FA_BF16, _abi.FA_I32, _abi.FA_I64, _abi.FA_I8, _abi.FA_U64, _abi.FA_NONE, 99])
def test_dtype_errors(dtype):
    assert _call(dtype=dtype) == _abi.FA_EDTYPE
    assert _abi.load().fa_last_error().decode()
    assert _call(dtype=dtype, P=0) == _abi.FA_EDTYPE
    assert _call(dtype=dtype, P=-1) == _abi.FA_EINVAL, "the argument checks come first"


@pytest.mark.parametrize("dtype", [_abi.FA_F32, _abi.FA_F64, _abi.FA_F16])
def test_empty_is_ok(dtype):
    """P = 0 launches nothing; the extremes of every other argument are accepted on the way."""
    assert _call(dtype=dtype, P=0) == _abi.FA_OK
    assert _call(dtype=dtype, P=0, out=None, x=None) == _abi.FA_OK
    assert _call(dtype=dtype, P=0, offset=I63, seed=(1 << 64) - 1, stream_id=0xFFFFFFFF, round_id=0xFFFFFFFF) == _abi.FA_OK
    assert _call(dtype=dtype, P=0, sigma=0.0) == _abi.FA_OK
    assert _call(dtype=dtype, P=0, x=4096 + 4) == _abi.FA_OK, "nothing overlaps at P = 0"


# ---- plug-in: parameter validation before any device work -----------------------------------------
def _queue(K=3):
    from fedn_amd.updatehandler import MemoryUpdateHandler
    uh = MemoryUpdateHandler()
    rng = np.random.default_rng(0)
    gid = uh.put_global_model([rng.standard_normal((4, 3)).astype(np.float32)])
    for k in range(K):
        uh.submit([rng.standard_normal((4, 3)).astype(np.float32)], 10 + k, model_id=gid)
    return uh


OK = {"clip": 1.0, "noise_multiplier": 1.0}
BAD = {"none": None, "empty": {}, "clip_missing": {"noise_multiplier": 1.0}, "noise_missing": {"clip": 1.0},
       "clip_zero": {**OK, "clip": 0.0}, "clip_negative": {**OK, "clip": -1.0}, "clip_int": {**OK, "clip": 1},
       "clip_nan": {**OK, "clip": float("nan")}, "clip_inf": {**OK, "clip": float("inf")}, "clip_str": {**OK, "clip": "1.0"},
       "noise_negative": {**OK, "noise_multiplier": -0.5}, "noise_int": {**OK, "noise_multiplier": 1},
       "noise_nan": {**OK, "noise_multiplier": float("nan")}, "noise_inf": {**OK, "noise_multiplier": float("inf")},
       "seed_bool": {**OK, "seed": True}, "seed_negative": {**OK, "seed": -1}, "seed_2_64": {**OK, "seed": 1 << 64},
       "seed_float": {**OK, "seed": 1.0}, "seed_str": {**OK, "seed": "7"}, "unknown_key": {**OK, "momentum": 0.9},
       "other_rule_key": {**OK, "tau": 1.0}, "other_rule_key_2": {**OK, "iterations": 1}}


@pytest.mark.parametrize("name", list(BAD))
def test_dpfedavg_refuses_invalid_parameters(name, monkeypatch):
    from fedn_amd import ops
    from fedn_amd.aggregators import get_aggregator

    def no_device_work(*a, **kw):
        raise AssertionError("device work after invalid parameters")

    monkeypatch.setattr(ops, "centered_clip_step", no_device_work)
    monkeypatch.setattr(ops, "gaussian_noise", no_device_work)
    uh = _queue()
    stored = set(uh.store.models)
    agg = get_aggregator("dpfedavg", uh)
    assert agg.name == "dpfedavg"
    model, data = agg.combine_models(helper=None, parameters=BAD[name])
    assert model is None and data["nr_aggregated_models"] == 0
    assert "time_model_load" in data and "time_model_aggregation" in data
    assert uh.model_updates.qsize() == 0, "the queue is drained"
    assert set(uh.store.models) == stored, "nothing is deleted"
    assert agg.round_id == 1, "a refused round still uses up its noise stream"


def test_dpfedavg_accepted_values_and_seed(caplog):
    from fedn_amd.aggregators import get_aggregator
    agg = get_aggregator("dpfedavg", _queue(0))
    assert agg.default_parameters == {}, "clip and noise_multiplier have no default"
    assert agg._validate_and_merge_parameters({"clip": 2.5, "noise_multiplier": 0.0}) == {"clip": 2.5, "noise_multiplier": 0.0}
    for seed in (0, 1, (1 << 64) - 1):
        assert agg._validate_and_merge_parameters({**OK, "seed": seed}) == {**OK, "seed": seed}
    with caplog.at_level(logging.DEBUG, logger="fedn"):
        drawn = agg._session_seed(None)
        assert isinstance(drawn, int) and 0 <= drawn < 1 << 64 and agg._session_seed(None) == drawn, "drawn once"
        assert get_aggregator("dpfedavg", _queue(0))._session_seed(None) != drawn, "64 random bits per instance"
        assert "seed" not in caplog.text and str(drawn) not in caplog.text, "a drawn seed is never logged"
        assert agg._session_seed(1234567) == 1234567 and agg._session_seed(1234567) == 1234567
    warnings = [r for r in caplog.records if r.levelno == logging.WARNING]
    assert len(warnings) == 1 and "seed" in warnings[0].getMessage() and "1234567" not in caplog.text


def test_round_id_counts_every_call():
    from fedn_amd.aggregators import get_aggregator
    agg = get_aggregator("dpfedavg", _queue(0))
    for n in range(1, 4):
        model, _ = agg.combine_models(helper=None, parameters=OK)          # an empty queue: (None, data)
        assert model is None and agg.round_id == n
