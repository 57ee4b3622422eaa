"""The parked fold's tile height and load policy (fa_tune AVG_PARK_HEIGHT / _LOADPOL, probe library;
fedavg_park_body in fedavg_kernels.h), one process, 64 x 100 M fp32 device-resident:

 1. height {1, 2, 4} x slots x load policy {0, nt, sc1, sc1 nt} at one workgroup per CU and ring 2,
    period 0.7 of that grid's round (a round carries HEIGHT times the bytes), windows 8 % and 4 %;
 2. the two best again at two workgroups per CU and (where instantiated) at ring 3;
 3. in the same loop, as reference points: the product's kernel at the product's own window (while
    the product ships height 1 / policy 0, the parent's shipped point), the no-store traversal
    (fa_stream_sum, SUM_NOSTORE) and a one-buffer streaming read (fa_stream_read, 4 GiB);
 4. the best setting against the product's kernel at K = 48 and 32, and at K = 64 on the smallest
    model the pipelined geometry takes (160 MiB per client).

Every point is compared bit for bit with the window-less mode-0 fold of the same inputs. Interleaved
repeats, each the median of 5 launches; a point's figure is the median over the repeats. One JSON
line per section.

  python tools/park_height_sweep.py [--reps 5] [--params 100000000]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fedn_amd import _abi, ops  # noqa: E402
from tools.window_probe import median_ms  # noqa: E402

TILE_BYTES = 16384
OFF = dict(avg_win_period=0, avg_win_w=0, avg_win_mode=0, grid=0, avg_park_depth=0, avg_park_slots=0, avg_park_height=0,
           avg_park_loadpol=0)
POLS = {0: "default", 1: "nt", 2: "sc1", 3: "sc1_nt"}


def period_of(K, cus, grid, height):
    """0.7 of the time one round of the grid's workgroups streams its tall tiles at 6.4 TB/s, in 10-ns ticks."""
    round_bytes = grid * cus * height * TILE_BYTES * (K + 1)
    return int(0.7 * round_bytes / 6.4e12 * 1e8)


class Point:
    """(depth, height, slots, pol, grid, window share): a generalised parked launch; None = the product's."""

    def __init__(self, K, cus, depth, height, slots, pol, grid=1, share=0.08):
        self.key = (depth, height, slots, pol, grid, share)
        self.period = period_of(K, cus, grid, height)
        self.knobs = dict(avg_win_period=self.period, avg_win_w=max(1, int(share * self.period)), avg_win_mode=3, grid=grid,
                          avg_park_depth=depth, avg_park_slots=slots, avg_park_height=height, avg_park_loadpol=pol)
        self.name = f"d{depth}_h{height}_s{slots}_{POLS[pol]}_g{grid}_w{int(share * 100)}"


def measure(fn, agg, ref, points, reps, extra=()):
    """{name: {ms, bit_exact, ...}} of the points, the product's kernel ("product") and `extra`
    [(name, setup, fn, teardown)], interleaved."""
    exact = {}
    for p in points:
        ops.tune(**p.knobs)
        agg.zero_()
        fn()
        torch.cuda.synchronize()
        assert ops.last_kernel() == "k_fedavg_pipe_win", (p.name, ops.last_kernel())
        exact[p.name] = bool(torch.equal(agg.view(torch.int32), ref.view(torch.int32)))
    ops.tune(**OFF)
    agg.zero_()
    fn()
    torch.cuda.synchronize()
    exact["product"] = bool(torch.equal(agg.view(torch.int32), ref.view(torch.int32)))
    res = {}
    for _ in range(reps):
        ops.tune(**OFF)
        fn()
        res.setdefault("product", []).append(median_ms(fn))
        for p in points:
            ops.tune(**p.knobs)
            fn()
            res.setdefault(p.name, []).append(median_ms(fn))
        ops.tune(**OFF)
        for name, setup, efn, teardown in extra:
            setup()
            efn()
            res.setdefault(name, []).append(median_ms(efn))
            teardown()
    ops.tune(**OFF)
    out = {}
    for name, v in res.items():
        out[name] = {"ms": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
        if name in exact:
            out[name]["bit_exact"] = exact[name]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--params", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    _abi.use_probe()
    dev = torch.device("cuda", 0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    P, K = a.params, 64
    g = torch.Generator(device=dev).manual_seed(5)
    base = torch.randn(P, generator=g, device=dev)
    ups = [torch.randn(P, generator=g, device=dev).mul_(0.01).add_(base) for _ in range(K)]
    del base
    one = torch.empty(1 << 30, dtype=torch.float32, device=dev).normal_(generator=g)      # the one-buffer read: 4 GiB
    sink = ops.stream_read_sink(one)
    agg = torch.empty(P, device=dev)

    def workload(K, n):
        ns = [int(v) for v in np.random.default_rng(K).integers(1, 5001, K)]
        Ns = [int(v) for v in np.cumsum(ns)]
        view = [u[:n] for u in ups[:K]]
        out = agg[:n]
        fn = lambda: ops.fedavg_fold(out, view, ns, Ns, True)  # noqa: E731
        ops.tune(**OFF)
        ops.tune(avg_win_period=-1)                           # no window, mode 0: the reference bits
        fn()
        torch.cuda.synchronize()
        ref = out.clone()
        ops.tune(**OFF)
        return fn, out, ref, view

    fn, out, ref, view = workload(K, P)
    alg = K * P * 4 + P * 4
    extra = [("nostore", lambda: ops.tune(sum_nostore=1), lambda: ops.stream_sum(out, view), lambda: ops.tune(sum_nostore=0)),
             ("one_buffer_read", lambda: None, lambda: ops.stream_read(one, sink), lambda: None)]
    shapes = [(1, 1), (1, 2), (2, 1), (2, 2), (4, 1)]
    points = [Point(K, cus, 2, h, s, pol, 1, share) for h, s in shapes for pol in POLS for share in (0.08, 0.04)]
    r1 = measure(fn, out, ref, points, a.reps, extra)
    read_tbps = one.numel() * 4 / r1["one_buffer_read"]["ms"] / 1e9
    r1["one_buffer_read"]["tbps"] = round(read_tbps, 3)
    r1["one_buffer_read"]["ms_for_alg_bytes"] = round(alg / read_tbps / 1e9, 4)
    print(json.dumps({"section": "height x slots x policy, 1 per CU, ring 2", "clients": K, "params": P, "cus": cus,
                      "alg_bytes": alg, "points": r1}), flush=True)
    ranked = sorted(points, key=lambda p: r1[p.name]["ms"])
    best = []
    for p in ranked:                                          # the two best (depth, height, slots, pol), whatever their window
        if p.key[:4] not in [b.key[:4] for b in best]:
            best.append(p)
        if len(best) == 2:
            break
    ring3 = {(1, 1), (1, 2), (1, 4), (2, 1), (2, 2)}          # (height, slots) instantiated at ring 3, policy 0
    again = list(best)
    for b in best:
        d, h, s, pol, _, share = b.key
        again.append(Point(K, cus, d, h, s, pol, 2, share))
        if pol == 0 and (h, s) in ring3:
            again.append(Point(K, cus, 3, h, s, pol, 1, share))
    r2 = measure(fn, out, ref, again, a.reps)
    print(json.dumps({"section": "the two best at 2 per CU and at ring 3", "clients": K, "params": P, "points": r2}), flush=True)
    d, h, s, pol, _, share = best[0].key
    for K2, n in ((48, P), (32, P), (64, (160 << 20) // 4)):
        fn2, out2, ref2, _ = workload(K2, n)
        r3 = measure(fn2, out2, ref2, [Point(K2, cus, d, h, s, pol, 1, share), Point(K2, cus, 2, 1, 2, 0, 1, 0.08)], a.reps)
        print(json.dumps({"section": "the best setting elsewhere", "clients": K2, "params": n, "points": r3}), flush=True)


if __name__ == "__main__":
    main()
