"""Geometric median on MI355X: fa_weighted_mean_sqdist (k_wmean_dist), device-resident fp32 updates.
One JSON line per K, then one per full round.

For K in --clients (default 8, 16, 32, 64) over --params fp32 parameters (default 100 M):
  pass_ms / nostore_ms one fused Weiszfeld pass (ops.weighted_mean_sqdist into preallocated buffers) with
                       and without the store of the mean (HIP events; median, min and max of --reps
                       timed calls after --warm warm-up calls)
  pass_GBps            the bytes read, 4 P K, over the median time (nostore_GBps likewise)
  fold_ms / fold_GBps  the FedAvg fold (ops.fedavg_fold, init) timed in the same process on the same
                       buffers, its calls alternating with the passes: the same bytes read
  pass_vs_fold         pass_ms / fold_ms (1.0 = a Weiszfeld step costs one fold); nostore_vs_fold likewise
  same_bits            two of the timed calls' means and distances are identical
For K in --round-clients (default 8, 16): a full ``geomedian`` round through the plug-in from host arrays
(load, H2D, 1 + iterations fused passes, D2H): wall seconds and the plug-in's own timing keys.
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


def full_round(K, P, dev):
    from fedn_amd.aggregators import get_aggregator
    from fedn_amd.updatehandler import MemoryUpdateHandler
    rng = np.random.default_rng(K)
    base = rng.standard_normal(P, dtype=np.float32)
    uh = MemoryUpdateHandler()
    for k in range(K):
        noise = rng.standard_normal(P, dtype=np.float32)
        noise *= np.float32(0.05 * (1 + 0.25 * k))
        noise += base
        uh.submit([noise], 100 + k)
    agg = get_aggregator("geomedian", uh)
    agg.device = dev
    t0 = time.perf_counter()
    model, data = agg.combine_models(helper=None)
    wall = time.perf_counter() - t0
    rec = {"round": "geomedian", "K": K, "P": P, "wall_s": wall, "passes": len(agg.trace or []),
           "weights": [float(w) for w in (agg.weights if agg.weights is not None else [])], "host_side": agg.host_side,
           "ok": model is not None}
    rec.update({k: float(v) for k, v in data.items()})
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--params", type=int, default=100_000_000)
    ap.add_argument("--clients", default="8,16,32,64")
    ap.add_argument("--round-clients", default="8,16")
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
    agg = torch.empty(P, device=dev)
    z = torch.empty(P, device=dev)
    rng = np.random.default_rng(0)
    for K in Ks:
        u = ups[:K]
        n = [int(v) for v in rng.integers(1, 5001, K)]
        N = [float(v) for v in np.cumsum(n)]
        beta = rng.uniform(0.5, 1.5, K)
        beta = (beta / beta.sum()).tolist()
        d = torch.empty(K, dtype=torch.float64, device=dev)
        calls = {"pass": lambda: ops.weighted_mean_sqdist(u, beta, out=z, dist=d),
                 "nostore": lambda: ops.weighted_mean_sqdist(u, beta, dist=d, store=False),
                 "fold": lambda: ops.fedavg_fold(agg, u, n, N, True)}
        for fn in calls.values():
            for _ in range(a.warm):
                fn()
        kernel = {}
        for name, fn in calls.items():
            fn()
            kernel[name] = ops.last_kernel()
        ev = {name: [] for name in calls}
        kept = []
        for _ in range(a.reps):                      # alternating: drift hits all alike
            for name, fn in calls.items():
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                fn()
                e.record()
                ev[name].append((s, e))
                if name == "pass" and len(kept) < 2:
                    kept.append((z[:1 << 20].clone(), d.clone()))
        torch.cuda.synchronize()
        by = 4 * P * K
        rec = {"K": K, "P": P, "bytes": by, "reps": a.reps, "kernels": kernel}
        med = {}
        for name in calls:
            med[name], lo, hi = _stats([s.elapsed_time(e) for s, e in ev[name]])
            rec[f"{name}_ms"], rec[f"{name}_ms_min"], rec[f"{name}_ms_max"] = med[name], lo, hi
            rec[f"{name}_GBps"] = by / med[name] / 1e6
        rec["pass_vs_fold"] = med["pass"] / med["fold"]
        rec["nostore_vs_fold"] = med["nostore"] / med["fold"]
        rec["same_bits"] = bool(len(kept) == 2 and torch.equal(kept[0][0], kept[1][0]) and torch.equal(kept[0][1], kept[1][1]))
        print(json.dumps(rec), flush=True)
    del ups, agg, z
    torch.cuda.empty_cache()
    for K in [int(k) for k in a.round_clients.split(",") if k]:
        print(json.dumps(full_round(K, P, dev)), flush=True)


if __name__ == "__main__":
    main()
