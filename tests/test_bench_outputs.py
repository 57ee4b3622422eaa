"""bench.py's plain run and ``--dump-outputs``: a plain run prints the headline line alone (no side
field, nothing that takes a run of its own), ``--steps`` sets the timed steps, and the dumped
aggregate is what the timed fold computed on the seeded inputs (bit-for-bit the oracle's)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402

SIDE_FIELDS = ("gather_to_host", "access_pattern", "configs1", "achievable", "host_resident", "fedopt_waves", "fedopt",
               "configs0")


def test_dump_whole_array_below_the_limit(tmp_path):
    x = torch.arange(1000, dtype=torch.float64).reshape(10, 100)
    bench.dump_outputs(str(tmp_path / "d"), {"aggregate": x})
    got = np.load(tmp_path / "d" / "aggregate.npy")
    assert got.dtype == np.float32 and np.array_equal(got, np.arange(1000, dtype=np.float32))


def test_dump_sample_is_fixed_and_keeps_both_ends(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 1000)
    monkeypatch.setattr(bench, "DUMP_EDGE", 100)
    x = torch.arange(5003, dtype=torch.float32)
    bench.dump_outputs(str(tmp_path / "a"), {"aggregate": x})
    bench.dump_outputs(str(tmp_path / "b"), {"aggregate": x.clone()})
    a, b = np.load(tmp_path / "a" / "aggregate.npy"), np.load(tmp_path / "b" / "aggregate.npy")
    assert a.dtype == np.float32 and a.shape == (1000,) and np.array_equal(a, b)
    assert np.array_equal(a[:100], np.arange(100)) and np.array_equal(a[-100:], np.arange(4903, 5003))
    mid = a[100:-100]                                   # the values are their own positions
    assert np.all(np.diff(mid) >= 0) and mid.min() >= 100 and mid.max() < 4903
    assert len(np.unique(mid)) > 600                    # drawn over the whole middle, not one stretch


def test_default_dump_stays_under_64_mb():
    assert bench.DUMP_MAX_ELEMS * 4 + 128 <= 64 * 1000 * 1000 and 2 * bench.DUMP_EDGE < bench.DUMP_MAX_ELEMS


def _run_main(monkeypatch, capsys, *args):
    monkeypatch.setattr(sys, "argv", ["bench.py", *args])
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_plain_run_line_and_dump(tmp_path, monkeypatch, capsys, dtype):
    from oracle import numpy_ref as ref
    K, P, seed = 5, 1_000_003, 3
    out = _run_main(monkeypatch, capsys, "--gpus", "1", "--steps", "3", "--warmup", "1", "--clients", str(K),
                    "--params", str(P), "--seed", str(seed), "--dtype", dtype, "--dump-outputs", str(tmp_path))
    assert out["metric"] == bench.METRIC and out["unit"] == "params/s" and out["higher_is_better"] is True
    assert out["dtype"] == dtype and out["steps"] == 3 and out["warmup"] == 1 and out["full"] is False
    assert out["ms_per_step"] > 0 and out["value"] == pytest.approx(K * P / (out["ms_per_step"] / 1e3), rel=1e-9)
    assert out["cpu_baseline"] is None and not [f for f in SIDE_FIELDS if f in out]
    got = np.load(tmp_path / "aggregate.npy")
    assert got.dtype == np.float32 and got.shape == (P,)
    dev = torch.device("cuda", 0)
    ups = [u.float().cpu().numpy() for u in bench.make_updates(K, P, dtype, dev, seed)]
    ns = [int(v) for v in np.random.default_rng(seed).integers(1, 5001, K)]
    want = ref.fedavg_flat(ups, ns)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
