"""Bulyan on MI355X: fa_median_window_mean (k_median_window), device-resident fp32 updates.
One JSON line per K, then one per full round.

For K in --clients (default 8, 16, 32, 64) over --params fp32 parameters (default 100 M), with
keep = K - 2 * ((K - 3) // 4) (all K buffers play the selected ones):
  window_ms            one ops.median_window_mean call (HIP events; median, min and max of --reps timed
                       calls after --warm warm-up calls)
  trimmed_ms           ops.trimmed_mean at the trim that keeps as many values, (K - keep) / 2, timed in the
                       same process on the same buffers, its calls alternating with the window calls: the
                       kernel this one grew from, reading the same bytes
  *_GBps               the algorithmic bytes 4 P (K + 1) over the median time
  window_vs_trimmed    trimmed_ms / window_ms (1.0 = the window kernel runs at the trimmed mean's rate)
  same_bits            two window calls' results are identical
For K in --round-clients (default 8, 16) over --round-params parameters (default 10 M): the whole
``RobustPipeline.bulyan`` round (distance pass, iterated selection, window mean over the selected, D2H)
against ``select_mean`` (Multi-Krum) on the SAME held updates, alternating: wall milliseconds, median
[min - max] of --reps rounds.
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
from fedn_amd import _abi, ops, robust  # noqa: E402


def _stats(ms):
    ms = sorted(ms)
    return ms[len(ms) // 2], ms[0], ms[-1]


def full_round(K, P, dev, reps, warm):
    rng = np.random.default_rng(K)
    base = rng.standard_normal(P, dtype=np.float32)
    pipe = None
    for k in range(K):
        noise = rng.standard_normal(P, dtype=np.float32)
        noise *= np.float32(0.05 * (1 + 0.25 * k))
        noise += base
        if pipe is None:
            pipe = robust.RobustPipeline(dev, [noise])
        else:
            pipe.add([noise])
    fb, fk = robust.bulyan_f(0.25, K), robust.krum_f(0.2, K)
    calls = {"bulyan": lambda: pipe.bulyan(fb), "multikrum": lambda: pipe.select_mean(fk, K - fk)}
    wall = {name: [] for name in calls}
    try:
        for i in range(warm + reps):
            for name, fn in calls.items():               # alternating: drift hits both alike
                t0 = time.perf_counter()
                fn()
                if i >= warm:
                    wall[name].append((time.perf_counter() - t0) * 1e3)
        rec = {"round": "bulyan vs multikrum", "K": K, "P": P, "f_bulyan": fb, "f_multikrum": fk, "reps": reps,
               "host_side": pipe.host_side, "selected": pipe.selected}
    finally:
        pipe.release()
    for name in calls:
        rec[f"{name}_ms"], rec[f"{name}_ms_min"], rec[f"{name}_ms_max"] = _stats(wall[name])
    rec["bulyan_vs_multikrum"] = rec["bulyan_ms"] / rec["multikrum_ms"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--params", type=int, default=100_000_000)
    ap.add_argument("--clients", default="8,16,32,64")
    ap.add_argument("--round-clients", default="8,16")
    ap.add_argument("--round-params", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warm", type=int, default=3)
    a = ap.parse_args()
    _abi.load()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    Ks = [int(k) for k in a.clients.split(",") if k]
    P = a.params
    g = torch.Generator(device=dev).manual_seed(0)
    ups = [torch.randn(P, generator=g, device=dev) for _ in range(max(Ks, default=0))]
    out = torch.empty(P, device=dev)
    ref = torch.empty(P, device=dev)
    for K in Ks:
        u = ups[:K]
        keep = K - 2 * ((K - 3) // 4)
        trim = (K - keep) // 2
        calls = {"window": lambda: ops.median_window_mean(out, u, keep), "trimmed": lambda: ops.trimmed_mean(ref, u, trim)}
        kernel = {}
        for name, fn in calls.items():
            for _ in range(a.warm):
                fn()
            kernel[name] = ops.last_kernel()
        ev = {name: [] for name in calls}
        for _ in range(a.reps):                          # alternating: drift hits both alike
            for name, fn in calls.items():
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                fn()
                e.record()
                ev[name].append((s, e))
        torch.cuda.synchronize()
        by = 4 * P * (K + 1)
        rec = {"K": K, "keep": keep, "trim": trim, "P": P, "bytes": by, "reps": a.reps, "kernels": kernel}
        med = {}
        for name in calls:
            med[name], lo, hi = _stats([s.elapsed_time(e) for s, e in ev[name]])
            rec[f"{name}_ms"], rec[f"{name}_ms_min"], rec[f"{name}_ms_max"] = med[name], lo, hi
            rec[f"{name}_GBps"] = by / med[name] / 1e6
        rec["window_vs_trimmed"] = med["trimmed"] / med["window"]
        first = out.clone()
        ops.median_window_mean(out, u, keep)
        rec["same_bits"] = bool(torch.equal(first.view(torch.int32), out.view(torch.int32)))
        del first
        print(json.dumps(rec), flush=True)
    del ups, out, ref
    torch.cuda.empty_cache()
    for K in [int(k) for k in a.round_clients.split(",") if k]:
        print(json.dumps(full_round(K, a.round_params, dev, a.reps, a.warm)), flush=True)


if __name__ == "__main__":
    main()
