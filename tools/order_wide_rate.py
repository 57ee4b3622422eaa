"""The wide trimmed mean / median on MI355X: fa_order_mean_wide (k_order_wide), device-resident updates, one
launch of K updates over the largest P that --gib of update bytes hold, for K in --clients (default 128, 256,
512, 1024) and float32 and bfloat16 updates, against two yardsticks on the same box and the same buffer. One
JSON line per (dtype, K).

  median_ms, trim_ms   one ops.median_wide / ops.trimmed_mean_wide(trim = K // 10) launch (HIP events; median, min
                 and max of --reps timed calls after --warm warm-up calls, the four kinds of call alternating);
                 *_GBps: the algorithmic bytes P (K isz + osz) over the median time
  mean64_ms      (a) ops.median of 64 updates over the same bytes (k_order_mean, the register network), so the
                 two sorts compare per byte: wide_vs_mean64 is the ratio of the GB/s
  fold_ms        (b) ops.fedavg_fold of the same K updates (the HBM-bound fold, chunks of 64 clients)
  floor_ms       the algorithmic bytes over 8.0 TB/s
  same_bits      two median_wide launches agree
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fedn_amd import _abi, ops  # noqa: E402

PEAK_TBPS = 8.0


def _stats(ms):
    ms = sorted(ms)
    return ms[len(ms) // 2], ms[0], ms[-1]


def rate(a, dev, buf, dt, K):
    isz = buf.element_size()
    osz = 4
    P = buf.numel() // K // 64 * 64                          # every row 16-byte aligned
    P64 = buf.numel() // 64 // 64 * 64
    ups = [buf[k * P:(k + 1) * P] for k in range(K)]
    ups64 = [buf[k * P64:(k + 1) * P64] for k in range(64)]
    out, out2 = torch.empty(P, device=dev), torch.empty(P, device=dev)
    out64, agg = torch.empty(P64, device=dev), torch.empty(P, device=dev)
    n = [100.0] * K
    N = [100.0 * (k + 1) for k in range(K)]
    calls = {"median": lambda: ops.median_wide(out, ups),
             "trim": lambda: ops.trimmed_mean_wide(out2, ups, K // 10),
             "mean64": lambda: ops.median(out64, ups64),
             "fold": lambda: ops.fedavg_fold(agg, ups, n, N, True)}
    kernel = {}
    for name, fn in calls.items():
        for _ in range(a.warm):
            fn()
        kernel[name] = ops.last_kernel()
    ev = {name: [] for name in calls}
    kept = []
    for _ in range(a.reps):                                  # alternating: drift hits all alike
        for name, fn in calls.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            ev[name].append((s, e))
            if name == "median" and len(kept) < 2:
                kept.append(out.clone())
    torch.cuda.synchronize()
    nbytes = {"median": P * (K * isz + osz), "trim": P * (K * isz + osz), "mean64": P64 * (64 * isz + osz),
              "fold": P * (K * isz + osz)}
    rec = {"dtype": dt, "K": K, "P": P, "tile": ops.order_wide_tile(buf.dtype, K), "bytes": nbytes["median"], "reps": a.reps,
           "kernels": kernel}
    for name in calls:
        med, lo, hi = _stats([s.elapsed_time(e) for s, e in ev[name]])
        rec[f"{name}_ms"], rec[f"{name}_ms_min"], rec[f"{name}_ms_max"] = med, lo, hi
        rec[f"{name}_GBps"] = nbytes[name] / med / 1e6
    rec["floor_ms"] = nbytes["median"] / (PEAK_TBPS * 1e12) * 1e3
    rec["wide_vs_mean64"] = rec["median_GBps"] / rec["mean64_GBps"]
    rec["wide_vs_fold"] = rec["median_ms"] / rec["fold_ms"]
    rec["wide_vs_floor"] = rec["median_ms"] / rec["floor_ms"]
    rec["same_bits"] = bool(torch.equal(kept[0].view(torch.int32), kept[1].view(torch.int32)))
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=8.0, help="bytes of the K updates together")
    ap.add_argument("--clients", type=int, nargs="+", default=[128, 256, 512, 1024])
    ap.add_argument("--dtypes", nargs="+", default=["float32", "bfloat16"])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warm", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    _abi.load()
    for dt in a.dtypes:
        tdt = getattr(torch, dt)
        buf = torch.empty(int(a.gib * 2 ** 30) // tdt.itemsize, dtype=tdt, device=dev)
        g = torch.Generator(device=dev).manual_seed(0)
        for lo in range(0, buf.numel(), 1 << 28):            # (normal_ of the whole buffer would need its float copy)
            buf[lo:lo + (1 << 28)].normal_(generator=g)
        for K in a.clients:
            rate(a, dev, buf, dt, K)
        del buf
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
