"""The chunked clipping fold on MI355X: fa_clip_fold (k_clip_fold), device-resident fp32 updates, one launch of
--clients (default 64) clients over --params parameters (default 100 M), no carry, against three yardsticks
on the same box and buffers. Then one end-to-end ``dp_clipped_mean`` of --round-clients (default 256) updates
of --round-params (default 25 M) parameters held in HBM. One JSON line each.

  fold_ms       one ops.clip_fold launch, out of place (HIP events; median, min and max of --reps timed calls
                after --warm warm-up calls, the three kinds of call alternating); fold_GBps: the algorithmic
                bytes 4 P (K + 2) over the median
  copy_ms       (a) ops.stream_copy whose read plus written bytes are those 4 P (K + 2)
  fused_ms      (b) ops.centered_clip_step with its store on the same inputs: the LDS-tiled kernel that also
                takes the K distances
  floor_ms      (c) the algorithmic bytes over 8.0 TB/s
  fold_vs_copy, fold_vs_fused, fold_vs_floor   ratios of the medians
  same_bits     the fold's v' equals the fused kernel's, and two fold launches agree

  round:  pass0_ms / pass1_ms   the kernel time (HIP events around every launch) of the distances-only pass and
                of the moving pass (fold launches + distance launches) of one dp_clipped_mean, noise off;
                fused_bytes_pass: what one fused pass of the <= 64 path reads and writes, 4 P (K + 2);
                pass1_vs_fused_bytes_GBps: those bytes over pass1_ms (the chunked pass itself moves
                moved_bytes_pass1: every update twice, the centre and the carries)
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

PEAK_TBPS = 8.0


def _stats(ms):
    ms = sorted(ms)
    return ms[len(ms) // 2], ms[0], ms[-1]


def launch_rate(a, dev):
    K, P = a.clients, a.params
    g = torch.Generator(device=dev).manual_seed(0)
    base = torch.randn(P, generator=g, device=dev)
    ups = [base + 0.05 * torch.randn(P, generator=g, device=dev) for _ in range(K)]
    cen = base + 0.02 * torch.randn(P, generator=g, device=dev)
    del base
    out, out2 = torch.empty(P, device=dev), torch.empty(P, device=dev)
    d = torch.empty(K, dtype=torch.float64, device=dev)
    nbytes = 4 * P * (K + 2)
    src = torch.empty(nbytes // 2 // 4, device=dev).normal_(generator=g)
    dst = torch.empty_like(src)
    coef = (np.random.default_rng(0).uniform(0.2, 1.0, K) / K).tolist()        # clipped clients: lambda < 1
    calls = {"fold": lambda: ops.clip_fold(ups, cen, coef, out=out),
             "copy": lambda: ops.stream_copy(dst, src),
             "fused": lambda: ops.centered_clip_step(ups, cen, coef, out=out2, dist=d)}
    kernel = {}
    for name, fn in calls.items():
        for _ in range(a.warm):
            fn()
        kernel[name] = ops.last_kernel() if name != "copy" else "stream_copy"
    ev = {name: [] for name in calls}
    kept = []
    for _ in range(a.reps):                          # alternating: drift hits all alike
        for name, fn in calls.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            ev[name].append((s, e))
            if name == "fold" and len(kept) < 2:
                kept.append(out.clone())
    torch.cuda.synchronize()
    rec = {"what": "launch", "K": K, "P": P, "dtype": "float32", "bytes": nbytes, "reps": a.reps, "kernels": kernel}
    med = {}
    for name in calls:
        med[name], lo, hi = _stats([s.elapsed_time(e) for s, e in ev[name]])
        rec[f"{name}_ms"], rec[f"{name}_ms_min"], rec[f"{name}_ms_max"] = med[name], lo, hi
        rec[f"{name}_GBps"] = nbytes / med[name] / 1e6
    rec["floor_ms"] = nbytes / (PEAK_TBPS * 1e12) * 1e3
    rec["fold_vs_copy"] = med["fold"] / med["copy"]
    rec["fold_vs_fused"] = med["fold"] / med["fused"]
    rec["fold_vs_floor"] = med["fold"] / rec["floor_ms"]
    rec["same_bits"] = bool(torch.equal(kept[0], kept[1]) and torch.equal(kept[0], out2))
    print(json.dumps(rec), flush=True)


def round_rate(a, dev):
    K, P = a.round_clients, a.round_params
    rng = np.random.default_rng(1)
    base = rng.standard_normal(P).astype(np.float32)
    noise = [rng.standard_normal(P).astype(np.float32) for _ in range(4)]
    center = [base]
    tic = time.perf_counter()
    pipe = None
    for k in range(K):                               # distinct updates from four noise draws at graded scales
        u = [base + np.float32(0.02 + 0.001 * k) * noise[k % 4]]
        if pipe is None:
            pipe = robust.RobustPipeline(dev, u, tag=0)
        else:
            pipe.add(u, tag=k)
    stage_s = time.perf_counter() - tic
    clip = float(0.05 * np.sqrt(P))                  # clips the upper half of the scales
    pipe.dp_clipped_mean(center, clip, 0.0, 1, 0)    # warm: code objects, pools
    t0 = pipe.timings()["time_kernel"]
    pipe.centered_clip(center, 0, clip)              # pass 0 alone
    t1 = pipe.timings()["time_kernel"]
    tic = time.perf_counter()
    pipe.dp_clipped_mean(center, clip, 0.0, 1, 0)    # pass 0 and the moving pass
    wall = time.perf_counter() - tic
    t2 = pipe.timings()["time_kernel"]
    pass0, both = 1e3 * (t1 - t0), 1e3 * (t2 - t1)
    chunks = -(-K // ops.MAX_ORDER_K)
    fused = 4 * P * (K + 2)
    rec = {"what": "round", "K": K, "P": P, "dtype": "float32", "host_side": pipe.host_side, "clipped": pipe.clipped,
           "stage_s": stage_s, "round_wall_ms": 1e3 * wall, "pass0_ms": pass0, "pass1_ms": both - pass0,
           "fused_bytes_pass": fused, "moved_bytes_pass1": 4 * P * (2 * K + 2 * chunks + 2 * (chunks - 1) + 1),
           "pass0_GBps": 4 * P * (K + chunks) / pass0 / 1e6,
           "pass1_vs_fused_bytes_GBps": fused / (both - pass0) / 1e6}
    rec["pass1_moved_GBps"] = rec["moved_bytes_pass1"] / (both - pass0) / 1e6
    pipe.release()
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--params", type=int, default=100_000_000)
    ap.add_argument("--clients", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--round-params", type=int, default=25_000_000)
    ap.add_argument("--round-clients", type=int, default=256)
    ap.add_argument("--skip-round", action="store_true")
    a = ap.parse_args()
    _abi.use_probe()                                 # stream_copy is a measurement entry point; the kernels are the same
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    launch_rate(a, dev)
    torch.cuda.empty_cache()
    if not a.skip_round:
        round_rate(a, dev)


if __name__ == "__main__":
    main()
