"""The DP-FedAvg noise on MI355X: fa_gaussian_noise (k_gaussian_noise) over --params float32 parameters
(default 100 M) in place, against two references on the same box. One JSON line.

  noise_ms        one in-place launch (HIP events; median, min and max of --reps timed calls after --warm
                  warm-up calls); noise_Gelem_s the elements and noise_GBps the 8 P bytes it reads and
                  writes over the median
  copy_ms         ops.stream_copy of the same bytes (4 P read, 4 P written), its calls alternating with the
                  noise launches: what the memory system allows an elementwise pass of this size
  noise_vs_copy   noise_ms / copy_ms: how far the generator (ten Philox rounds, a float64 log, sqrt and cos
                  per element) is from memory-bound
  host_ms         the host alternative: numpy ``Generator.standard_normal(P)`` (float64, as a caller that
                  wants the float64 sum would draw it) — host_draw_ms — plus its upload from pageable
                  memory — host_h2d_ms — by the host's clock around a closing synchronise; median of
                  --host-reps
  host_vs_noise   host_ms / noise_ms
  same_bits       two launches from the same input give identical bits
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fedn_amd import _abi, ops  # noqa: E402


def _stats(ms):
    ms = sorted(ms)
    return ms[len(ms) // 2], ms[0], ms[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--params", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    a = ap.parse_args()
    _abi.use_probe()                                 # stream_copy is a measurement entry point; the kernels are the same
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    P = a.params
    x0 = torch.randn(P, generator=torch.Generator(device=dev).manual_seed(0), device=dev)
    x, y = torch.empty(P, device=dev), torch.empty(P, device=dev)
    kw = dict(sigma=0.01, seed=0x0123456789ABCDEF, stream_id=0, round_id=1)
    calls = {"noise": lambda: ops.gaussian_noise(x, x, **kw), "copy": lambda: ops.stream_copy(y, x)}
    for fn in calls.values():
        for _ in range(a.warm):
            x.copy_(x0)
            fn()
    ev = {name: [] for name in calls}
    kept = []
    for _ in range(a.reps):                          # alternating: drift hits both alike
        for name, fn in calls.items():
            x.copy_(x0)                              # the in-place launch starts from the same model every time
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            ev[name].append((s, e))
            if name == "noise" and len(kept) < 2:
                kept.append(x.clone())
    torch.cuda.synchronize()
    rec = {"P": P, "dtype": "float32", "reps": a.reps, "kernel": "k_gaussian_noise"}
    med = {}
    for name in calls:
        med[name], lo, hi = _stats([s.elapsed_time(e) for s, e in ev[name]])
        rec[f"{name}_ms"], rec[f"{name}_ms_min"], rec[f"{name}_ms_max"] = med[name], lo, hi
        rec[f"{name}_GBps"] = 8 * P / med[name] / 1e6
    rec["noise_Gelem_s"] = P / med["noise"] / 1e6
    rec["noise_vs_copy"] = med["noise"] / med["copy"]
    rec["same_bits"] = bool(len(kept) == 2 and torch.equal(kept[0], kept[1]))
    moved = (kept[0] - x0).double()
    rec["noise_std_over_sigma"] = float(moved.std()) / kw["sigma"]       # ~1 up to float32 rounding of the sum

    rng = np.random.default_rng(0)
    draw, h2d = [], []
    dst = torch.empty(P, dtype=torch.float64, device=dev)
    for _ in range(a.host_reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        z = rng.standard_normal(P)
        t1 = time.perf_counter()
        dst.copy_(torch.from_numpy(z))
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        draw.append(1e3 * (t1 - t0))
        h2d.append(1e3 * (t2 - t1))
    rec["host_draw_ms"], rec["host_h2d_ms"] = _stats(draw)[0], _stats(h2d)[0]
    rec["host_ms"] = rec["host_draw_ms"] + rec["host_h2d_ms"]
    rec["host_vs_noise"] = rec["host_ms"] / med["noise"]
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
