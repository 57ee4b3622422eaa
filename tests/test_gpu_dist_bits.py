"""The two fused distance kernels' sums, bit for bit: ``k_wmean_dist`` (``ops.weighted_mean_sqdist``) and
``k_cclip_dist`` (``ops.centered_clip_step``) promise the same bits for the same inputs on any device, but the
other suites hold the distances ``d`` to ``ops.sqdist_rtol`` only. tests/golden/dist_bits.json holds the sha256
of ``d`` (stored and with ``store=False``) and of ``z`` / ``v'`` as the library gives them on the MI355X: any
change to the order of a chain, a flush or the partials — a shared body for the two kernels, say (DESIGN.md
§3.10) — shows here.

Cases: the six dtypes x K in (3, 9, 17, 33, 64) — every KP — at P = TE - 1 (one ragged tile) and 3 TE + 5
(several workgroups, a ragged last tile), and for (f16, 33), (bf16, 33) and (i32, 33) the size at which every
workgroup flushes its chains in mid-kernel. ``python tests/test_gpu_dist_bits.py --record [FILE]`` rewrites
the fixture (or FILE) from whichever library ``FEDN_AMD_LIB`` names.
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dist_bits.json")
DTYPES = ["f32", "f64", "f16", "bf16", "i32", "i64"]
KS = [3, 9, 17, 33, 64]
MID_FLUSH = [("f16", 33), ("bf16", 33), ("i32", 33)]
NP_DT = {"f32": np.float32, "f64": np.float64, "f16": np.float16, "bf16": np.float32, "i32": np.int32, "i64": np.int64}
NP_OUT = {"f32": np.float32, "f64": np.float64, "f16": np.float16, "bf16": np.float32, "i32": np.float64, "i64": np.float64}
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
    torch.cuda.empty_cache()                                   # the mid-flush cases hold a few hundred MB


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def _bf16_exact(x):
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def _data(name, K, n):
    """K updates of n elements close to each other — a base plus small noise — a centre in the output type
    and K coefficients in (0, 1], one of them exactly 0, from a seed of (dtype, K); every value is exact in
    the dtype it is uploaded in. Returns device tensors and the coefficient list."""
    rng = np.random.default_rng(7919 * DTYPES.index(name) + K)
    dt = np.dtype(NP_DT[name])
    coef = rng.uniform(0.05, 1.0, K)
    coef[int(rng.integers(0, K))] = 0.0
    wide = np.float64 if name == "f64" else np.float32          # (float32 draws: the mid-flush sizes are millions)
    base = rng.standard_normal(n, dtype=wide)
    x = base + wide(0.05) * rng.standard_normal((K, n), dtype=wide)
    v = base + wide(0.02) * rng.standard_normal(n, dtype=wide)
    if dt.kind == "i":
        scale = 2.0 ** 20 if name == "i32" else 2.0 ** 40
        x = np.round(x.astype(np.float64) * scale).astype(dt)
        v = np.round(v.astype(np.float64) * scale)             # float64: the output type
        if name == "i64":                                      # not exact in float64: converted with one rounding
            q = max(1, n // 8)
            x[:, :q] += 2 ** 53 + 1
            v[:q] += 2.0 ** 53
    else:
        x = _bf16_exact(x) if name == "bf16" else x.astype(dt)
        v = v.astype(NP_OUT[name])
    ups = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    if name == "bf16":
        ups = ups.to(torch.bfloat16)                           # exact: the values are bf16's
    return ups, torch.from_numpy(np.ascontiguousarray(v)).to(DEV), coef.tolist()


def _sha(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def _sizes(te, grid, flush_tiles, mid):
    if mid:
        return {"midflush": grid * te * (flush_tiles + 1) + te // 2 + 3}
    return {"ragged": te - 1, "tiles": 3 * te + 5}


def _hashes(name, K, mid):
    """{"<op>/<size>": {"P", "point", "d", "d_nostore"}} of both ops at this (dtype, K)."""
    from fedn_amd import ops
    geom = {"wmean": ops.wmean_geometry(TORCH_DT[name], K), "cclip": ops.cclip_geometry(TORCH_DT[name], K)}
    sizes = {op: _sizes(te, grid, ft, mid) for op, (te, _, grid, ft) in geom.items()}
    n = -(-max(max(s.values()) for s in sizes.values()) // 64) * 64      # rows stay 16-B aligned
    ups, cen, coef = _data(name, K, n)
    got = {}
    for op in ("wmean", "cclip"):
        for size, P in sizes[op].items():
            views = [ups[k, :P] for k in range(K)]
            if op == "wmean":
                z, d = ops.weighted_mean_sqdist(views, coef)
                none, dn = ops.weighted_mean_sqdist(views, coef, store=False)
            else:
                z, d = ops.centered_clip_step(views, cen[:P], coef)
                none, dn = ops.centered_clip_step(views, cen[:P], coef, store=False)
            assert none is None and ops.last_kernel() == ("k_wmean_dist" if op == "wmean" else "k_cclip_dist")
            got[f"{op}/{size}"] = {"P": P, "point": _sha(z), "d": _sha(d), "d_nostore": _sha(dn)}
    return got


def _check(recorded, name, K, mid):
    key = f"{name}/K{K}/{'mid' if mid else 'small'}"
    got = _hashes(name, K, mid)
    want = recorded[key]
    assert sorted(got) == sorted(want), key
    for case in got:
        for field in ("P", "point", "d", "d_nostore"):
            assert got[case][field] == want[case][field], f"{key} {case}: {field} differs from the recorded library's"


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", DTYPES)
def test_bits_of_small_sizes(recorded, name, K):
    _check(recorded, name, K, False)


@pytest.mark.parametrize("name,K", MID_FLUSH)
def test_bits_across_a_mid_kernel_flush(recorded, name, K):
    _check(recorded, name, K, True)


def _record(path):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from fedn_amd import _abi
    out = {f"{name}/K{K}/small": _hashes(name, K, False) for name in DTYPES for K in KS}
    out.update({f"{name}/K{K}/mid": _hashes(name, K, True) for name, K in MID_FLUSH})
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(out)} cases from {_abi.lib_path()} -> {path}")


if __name__ == "__main__":
    if sys.argv[1:2] != ["--record"] or len(sys.argv) > 3:
        sys.exit("usage: python tests/test_gpu_dist_bits.py --record [FILE]")
    _record(sys.argv[2] if len(sys.argv) == 3 else FIXTURE)
