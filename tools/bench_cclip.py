"""Centred clipping on MI355X: fa_centered_clip_step (k_cclip_dist), device-resident updates of --dtype
(f32 by default; bf16, f16, f64). One JSON line per K.

For K in --clients (default 8, 16, 32, 64) over --params parameters (default 100 M); B is the updates'
element size and O the centre's / output's (ops.order_mean_dtype):
  clip_ms / nostore_ms  one clip pass in place (ops.centered_clip_step with out = the centre, which is put
                        back before every call, outside the timed span) and one with out = NULL, the
                        distances-only pass (HIP events; median, min and max of --reps timed calls after
                        --warm warm-up calls)
  clip_GBps             the bytes read, P (B K + O), over the median time (nostore_GBps likewise)
  wmean_ms / fold_ms    the Weiszfeld pass (ops.weighted_mean_sqdist, with its store) and the FedAvg fold
                        (ops.fedavg_fold, init) timed in the same process on the same buffers, their calls
                        alternating with the clip passes; their GB/s over the B P K bytes they read
  yardstick_ms          wmean_ms x (B K + O) / (B K) — the clip pass reads that much more and writes the same —
                        and yardstick_ms_max, the Weiszfeld pass's slowest call scaled alike
  clip_vs_yardstick     clip_ms / yardstick_ms; within_spread: clip_ms <= yardstick_ms_max
  same_bits             two of the timed in-place calls' new points and distances are identical
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fedn_amd import _abi, ops  # noqa: E402


DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "f64": torch.float64}


def _stats(ms):
    ms = sorted(ms)
    return ms[len(ms) // 2], ms[0], ms[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--params", type=int, default=100_000_000)
    ap.add_argument("--clients", default="8,16,32,64")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--dtype", choices=sorted(DTYPES), default="f32")
    a = ap.parse_args()
    _abi.load()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    Ks = [int(k) for k in a.clients.split(",") if k]
    P = a.params
    g = torch.Generator(device=dev).manual_seed(0)
    upd_dt = DTYPES[a.dtype]
    out_dt = ops.order_mean_dtype(upd_dt)
    B, O = upd_dt.itemsize, out_dt.itemsize
    ups = [torch.randn(P, generator=g, device=dev).to(upd_dt) for _ in range(max(Ks, default=0))]
    center0 = torch.randn(P, generator=g, device=dev).to(out_dt)
    cen = torch.empty(P, dtype=out_dt, device=dev)
    agg = torch.empty(P, dtype=out_dt, device=dev)
    z = torch.empty(P, dtype=out_dt, device=dev)
    rng = np.random.default_rng(0)
    for K in Ks:
        u = ups[:K]
        n = [int(v) for v in rng.integers(1, 5001, K)]
        N = [float(v) for v in np.cumsum(n)]
        beta = rng.uniform(0.5, 1.5, K)
        beta = (beta / beta.sum()).tolist()
        coef = (rng.uniform(0.2, 1.0, K) / K).tolist()       # clipped clients: lambda < 1
        d = torch.empty(K, dtype=torch.float64, device=dev)
        calls = {"clip": lambda: ops.centered_clip_step(u, cen, coef, out=cen, dist=d),
                 "nostore": lambda: ops.centered_clip_step(u, cen, coef, dist=d, store=False),
                 "wmean": lambda: ops.weighted_mean_sqdist(u, beta, out=z, dist=d),
                 "fold": lambda: ops.fedavg_fold(agg, u, n, N, True)}
        for fn in calls.values():
            for _ in range(a.warm):
                cen.copy_(center0)
                fn()
        kernel = {}
        for name, fn in calls.items():
            cen.copy_(center0)
            fn()
            kernel[name] = ops.last_kernel()
        ev = {name: [] for name in calls}
        kept = []
        for _ in range(a.reps):                      # alternating: drift hits all alike
            for name, fn in calls.items():
                cen.copy_(center0)                   # the in-place pass starts from the same centre every time
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                fn()
                e.record()
                ev[name].append((s, e))
                if name == "clip" and len(kept) < 2:
                    kept.append((cen[:1 << 20].clone(), cen[-(1 << 20):].clone(), d.clone()))
        torch.cuda.synchronize()
        rec = {"dtype": a.dtype, "K": K, "P": P, "bytes_clip": P * (B * K + O), "bytes_wmean": B * P * K, "reps": a.reps,
               "kernels": kernel}
        med, hi = {}, {}
        for name in calls:
            by = rec["bytes_clip"] if name in ("clip", "nostore") else rec["bytes_wmean"]
            med[name], lo, hi[name] = _stats([s.elapsed_time(e) for s, e in ev[name]])
            rec[f"{name}_ms"], rec[f"{name}_ms_min"], rec[f"{name}_ms_max"] = med[name], lo, hi[name]
            rec[f"{name}_GBps"] = by / med[name] / 1e6
        scale = rec["bytes_clip"] / rec["bytes_wmean"]
        rec["yardstick_ms"], rec["yardstick_ms_max"] = med["wmean"] * scale, hi["wmean"] * scale
        rec["clip_vs_yardstick"] = med["clip"] / rec["yardstick_ms"]
        rec["within_spread"] = bool(med["clip"] <= rec["yardstick_ms_max"])
        rec["clip_vs_fold"] = med["clip"] / med["fold"]
        rec["same_bits"] = bool(len(kept) == 2 and all(torch.equal(x, y) for x, y in zip(kept[0], kept[1])))
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
