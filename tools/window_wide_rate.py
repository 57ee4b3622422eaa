"""The wide mean around median on MI355X: fa_median_window_mean_wide (k_window_wide) against the wide median
(k_order_wide), which shares its load and sort, on the same box and the same buffer: device-resident updates,
one launch of K updates over the largest P that --gib of update bytes hold, for K in --clients (default 128, 256,
512, 1024) and float32 and bfloat16 updates — the bytes of tools/order_wide_rate.py. One JSON line per (dtype, K).

  median_ms      one ops.median_wide launch: the yardstick (the sort, then one or two keys a coordinate)
  meamed_ms      one ops.median_window_mean_wide launch at keep = K - floor(0.2 K), the plug-in's default
  half_ms        the same at keep = K // 2 + 1: the most window starts to count, the shortest sum
                 (HIP events; median, min and max of --reps timed calls after --warm warm-up calls, the three
                 kinds of call alternating); *_GBps: the algorithmic bytes P (K isz + osz) over the median time
  meamed_vs_median, half_vs_median   the ratios of the times
  same_bits      two meamed launches agree
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fedn_amd import _abi, ops  # noqa: E402


def _stats(ms):
    ms = sorted(ms)
    return ms[len(ms) // 2], ms[0], ms[-1]


def rate(a, dev, buf, dt, K):
    P = buf.numel() // K // 64 * 64                          # every row 16-byte aligned
    ups = [buf[k * P:(k + 1) * P] for k in range(K)]
    outs = {name: torch.empty(P, device=dev) for name in ("median", "meamed", "half")}
    calls = {"median": lambda: ops.median_wide(outs["median"], ups),
             "meamed": lambda: ops.median_window_mean_wide(outs["meamed"], ups, K - K // 5),
             "half": lambda: ops.median_window_mean_wide(outs["half"], ups, K // 2 + 1)}
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
            if name == "meamed" and len(kept) < 2:
                kept.append(outs["meamed"].clone())
    torch.cuda.synchronize()
    nbytes = P * (K * buf.element_size() + 4)
    rec = {"dtype": dt, "K": K, "P": P, "tile": ops.order_wide_tile(buf.dtype, K), "bytes": nbytes, "reps": a.reps,
           "kernels": kernel}
    for name in calls:
        med, lo, hi = _stats([s.elapsed_time(e) for s, e in ev[name]])
        rec[f"{name}_ms"], rec[f"{name}_ms_min"], rec[f"{name}_ms_max"] = med, lo, hi
        rec[f"{name}_GBps"] = nbytes / med / 1e6
    rec["meamed_vs_median"] = rec["meamed_ms"] / rec["median_ms"]
    rec["half_vs_median"] = rec["half_ms"] / rec["median_ms"]
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
