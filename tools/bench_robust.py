"""Robust aggregation rules on MI355X: fa_trimmed_mean (k_order_mean), device-resident fp32 updates.
One JSON line per K.

For K in --clients (default 8, 16, 32, 64) over --params fp32 parameters (default 100 M):
  median_ms / trimmed_ms   one ops.median / ops.trimmed_mean(trim = floor(0.1 K)) call (HIP events;
                           median, min and max of --reps timed calls after --warm warm-up calls)
  *_GBps                   the algorithmic bytes 4 P (K + 1) over the median time
  fold_ms / fold_GBps      the FedAvg fold (ops.fedavg_fold, init) timed in the same process on the
                           same buffers, its calls alternating with the robust ones: the same bytes read
  *_vs_fold                fold_ms / rule ms (1.0 = the rule runs at the fold's rate)
  numpy_median_s           np.median over the K updates' first --numpy-params elements on the host,
                           scaled to --params (the numpy server function the rule replaces)
  bit_exact                the device median of that slice equals numpy's, bit for bit
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
    ap.add_argument("--clients", default="8,16,32,64")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--numpy-params", type=int, default=1_000_000)
    a = ap.parse_args()
    _abi.load()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    Ks = [int(k) for k in a.clients.split(",")]
    P = a.params
    g = torch.Generator(device=dev).manual_seed(0)
    ups = [torch.randn(P, generator=g, device=dev) for _ in range(max(Ks))]
    out = torch.empty(P, device=dev)
    agg = torch.empty(P, device=dev)
    rng = np.random.default_rng(0)
    for K in Ks:
        u = ups[:K]
        n = [int(v) for v in rng.integers(1, 5001, K)]
        N = [float(v) for v in np.cumsum(n)]
        t10 = int(np.floor(0.1 * K))
        calls = {"median": lambda: ops.median(out, u), "trimmed": lambda: ops.trimmed_mean(out, u, t10),
                 "fold": lambda: ops.fedavg_fold(agg, u, n, N, True)}
        for fn in calls.values():
            for _ in range(a.warm):
                fn()
        kernel = {}
        for name, fn in calls.items():
            fn()
            kernel[name] = ops.last_kernel()
        ev = {name: [] for name in calls}
        for _ in range(a.reps):                      # alternating: drift hits every rule alike
            for name, fn in calls.items():
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                fn()
                e.record()
                ev[name].append((s, e))
        torch.cuda.synchronize()
        by = 4 * P * (K + 1)
        rec = {"K": K, "P": P, "bytes": by, "trim_0.1": t10, "reps": a.reps, "kernels": kernel}
        med = {}
        for name in calls:
            med[name], lo, hi = _stats([s.elapsed_time(e) for s, e in ev[name]])
            rec[f"{name}_ms"], rec[f"{name}_ms_min"], rec[f"{name}_ms_max"] = med[name], lo, hi
            rec[f"{name}_GBps"] = by / med[name] / 1e6
        rec["median_vs_fold"] = med["fold"] / med["median"]
        rec["trimmed_vs_fold"] = med["fold"] / med["trimmed"]
        m = min(P, a.numpy_params)
        ops.median(out[:m], [x[:m] for x in u])
        got = out[:m].cpu().numpy()
        S = np.stack([x[:m].cpu().numpy() for x in u])
        t0 = time.perf_counter()
        want = np.median(S, axis=0)
        dt = time.perf_counter() - t0
        rec["numpy_median_s"] = dt * P / m
        rec["numpy_slice"] = m
        rec["bit_exact"] = bool(got.dtype == want.dtype and np.array_equal(got.view(np.uint32), want.view(np.uint32)))
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
