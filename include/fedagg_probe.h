/*
 * fedagg_probe.h — measurement and tuning entry points of `libfedagg_probe.so`.
 *
 * NOT part of the drop-in boundary: the product library `libfedagg.so` exports only
 * include/fedagg.h, built with the measured-best launch settings as compile-time constants
 * (no mutable or process-global state). `libfedagg_probe.so` is the same source compiled with
 * -DFEDAGG_PROBES: it exports everything fedagg.h declares PLUS the knobs and probe kernels
 * below, which tools/ (microbench, PMC probes, A/B runs) and the division tests use to measure
 * alternatives. Knob settings are process-global (atomics) within the probe library only.
 */
#ifndef FEDAGG_PROBE_H
#define FEDAGG_PROBE_H

#include "fedagg.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Measurement helpers (not part of the reference interface): achievable-peak
 * reference kernels for the roofline section of bench.py.
 *   fa_stream_copy  dst[i] = src[i], 16 B per lane
 *   fa_stream_read  reads `bytes` and writes one 16-B word per workgroup to `sink`
 *                   (sink must hold >= 16 * fa_stream_read_blocks(bytes) bytes)
 */
int fa_stream_copy(void* dst, const void* src, int64_t bytes, void* stream);
/* out[i] = sum_k bufs[k][i] (fp32, K <= 64) with exactly the traversal of the FedAvg fold
 * kernel but one add per element: the access-pattern ceiling of fa_fedavg_fold.        */
int fa_stream_sum(float* out, const float* const* bufs, int K, int64_t P, void* stream);
/* The launch geometry of fa_pairwise_sqdist for (upd_dtype, K): the tile length TE (elements a
 * workgroup stages at a time), R (= FA_PAIR_CHAIN_TERMS), the largest grid, and the tiles a workgroup
 * walks between two flushes of its chains — what tools and tests need to put sizes on the kernel's
 * edges; none of it is part of the product ABI. Any output pointer may be NULL. FA_EINVAL for K
 * outside 1..64, FA_EDTYPE for a dtype outside the six of fa_pairwise_sqdist.                  */
int fa_pairwise_sqdist_geometry(int upd_dtype, int K, int* tile_elems, int* chain_terms, int* max_workgroups,
                                int* flush_tiles);
/* The same four numbers for fa_weighted_mean_sqdist: the tile length, the longest chain its kernel sums in
 * the compute type (<= FA_PAIR_CHAIN_TERMS), the largest grid and the tiles between two flushes. Same
 * status codes.                                                                                      */
int fa_wmean_sqdist_geometry(int upd_dtype, int K, int* tile_elems, int* chain_terms, int* max_workgroups,
                             int* flush_tiles);
/* And for fa_centered_clip_step, whose tile holds one more column (the centre's). Same status codes. */
int fa_centered_clip_geometry(int upd_dtype, int K, int* tile_elems, int* chain_terms, int* max_workgroups,
                              int* flush_tiles);

/* The knobs of fa_tune (process-global; measurement and tuning only). Every setting computes the
 * reference's bits except OPT_MIX and OPT_WIN_PERIOD > 0 without OPT_WIN_PROD, which run access-
 * pattern probes. fa_tune answers FA_EINVAL for an unknown knob or a value outside the ranges below.
 *
 * Launch geometry of the fp32 / bf16 -> fp32 FedAvg fold (the sweep of tools/microbench.py):
 *   STRIPS x UNROLL x NT: see probe_fedavg_geometry in csrc/probes.h for the instantiated
 *   combinations; any other runs 1 strip x 8 clients ahead.                                    */
enum fa_tune_knob {
    FA_TUNE_STRIPS = 0 /* 16-B strips per lane: 1 | 2 | 4 (default) | 8 | 16 */,
    FA_TUNE_UNROLL = 1 /* clients loaded before folding: 1 | 2 | 4 | 8 | 16 (k_fedavg), or 0 (default) =
                          the pipelined kernel k_fedavg_pipe */,
    FA_TUNE_NT = 2 /* non-temporal loads of the client buffers (0 default | 1) */,
    FA_TUNE_FASTDIV = 3 /* fp32 t/N via the exact RN64(1/N) product (1, default) or IEEE division (0);
                           both are correctly rounded */,
    FA_TUNE_LANETAB = 4 /* pipelined kernel reads the client table from registers via v_readlane (1) or
                           by scalar loads (0, default) */,
    FA_TUNE_GRID = 5 /* pipelined kernel: 0 (default) = one tile per workgroup, n <= 64 = a persistent
                        grid of n workgroups per CU sweeping the tiles; with AVG_WIN_MODE 3 (always a
                        persistent grid): 0 = its own 1 per CU, n = n per CU */,
    FA_TUNE_READ = 6 /* fa_stream_read loads per lane: 4 | 8 | 16 (default) */,
    FA_TUNE_BLOCK = 7 /* pipelined kernel workgroup size 256 (default) | 512 | 1024 */,
    FA_TUNE_SUM_NOSTORE = 8 /* fa_stream_sum: 1 = skip the store (reads + adds only) */,
    FA_TUNE_NT_STORE = 9 /* aggregate stores of the 4-strip pipelined kernel and fa_stream_sum: 0 plain,
                            1 non-temporal (default), 2 write-through (sc1) */,
    FA_TUNE_FASTDIV64 = 10 /* fp64 t/N via RN64(1/N) + two exact Markstein corrections (1, default) or
                              IEEE division (0); both correctly rounded */,
    FA_TUNE_NARROW = 11 /* bf16 -> f32 FedAvg: 1 (default) = the product's 8-B client strips / 16-B
                           aggregate strips (4 elements, 8 strips per lane: every wave store one
                           contiguous 1 KiB), 0 = 16-B client strips (8 elements, 4 per lane) */,
    FA_TUNE_AUTO_GEOM = 12 /* 1 (default) = with the default geometry knobs, the product's size-dependent
                              choice (pipelined kernel only for client buffers >= 160 MiB, else 1 strip
                              x 4/8 clients ahead); 0 = the knobs as set, at every size */,
    FA_TUNE_OPT_MIX = 13 /* FedOpt FIRST|FINAL, fp32 updates over an fp32 / fp64 model: 1 = k_fedopt_c's
                            exact loads and stores with one add per value instead of the arithmetic
                            (k_fedopt_mix; results are NOT the reference's; a ragged last 2048-element
                            tile is skipped) */,
    FA_TUNE_OPT_WIN_PERIOD = 14 /* FedOpt store window, in 10-ns ticks of the 100 MHz reference clock
                                   (64 .. 2^24): stores are issued only while clock mod period <
                                   OPT_WIN_W. Without OPT_WIN_PROD: k_fedopt_mix's pattern, windowed
                                   (k_fedopt_mixw; fp64 m out). With it: see OPT_WIN_PROD.
                                   0 (default) = the product's own window, -1 = none */,
    FA_TUNE_OPT_WIN_W = 15 /* the store window in 10-ns ticks */,
    FA_TUNE_OPT_WIN_MODE = 16 /* k_fedopt_mixw: 0 gate the stores only; 1 also start a tile's reads
                                 outside the window; 2 also every client batch's reads */,
    FA_TUNE_AVG_WIN_PERIOD = 17 /* FedAvg fp32 k_fedavg_pipe (the headline instantiation), its store
                                   window: 0 (default) = the product's own (avg_store_window), -1 =
                                   none, > 0 = this period with AVG_WIN_W / _MODE, also on the
                                   continuation launches of K > 64 */,
    FA_TUNE_AVG_WIN_W = 18,
    FA_TUNE_AVG_WIN_MODE = 19 /* 0 gate the stores only; 1 also start a tile's reads outside the window;
                                 2 also every client pair's reads; 3 "parked" (fp32 updates, first
                                 launches only; elsewhere it is mode 0): a persistent grid whose
                                 workgroups park a finished tile in LDS, read on, and store it when
                                 the window opens */,
    FA_TUNE_OPT_WIN_PROD = 20 /* 1: OPT_WIN_PERIOD / _W apply to the product step (k_fedopt_cw, bit-
                                 identical; a first or middle launch of a multi-launch round runs
                                 k_fedopt_cwp) instead of the pattern probe (0, default) */,
    FA_TUNE_AVG_PARK_DEPTH = 21 /* AVG_WIN_MODE 3: client buffers in the load ring, 2 | 3 | 4 (the loads of
                                   that many minus one stream positions stay in flight behind a
                                   consume); 0 (default) = the product's. With either of the two set,
                                   the launch is k_fedavg_park's (a knob left at 0: 2 buffers, 1 slot) */,
    FA_TUNE_AVG_PARK_SLOTS = 22 /* AVG_WIN_MODE 3: parked tiles per workgroup, 1 | 2 | 4 (16 KiB of LDS
                                   each); 0 (default) = the product's */,
    FA_TUNE_AVG_PARK_HEIGHT = 23 /* AVG_WIN_MODE 3: consecutive 16 KiB tiles of the model a workgroup reads
                                    from one client before it moves to the next client (a "tall" tile; a
                                    parked tile is that many times 16 KiB of LDS), 1 | 2 | 4; 0 (default)
                                    = the product's. Instantiated: ring 2 at (height, slots) = (2, 1),
                                    (2, 2), (4, 1); ring 3 at height 2 with 1 | 2 slots; a combination
                                    that is not instantiated launches nothing (fa_last_kernel says so) */,
    FA_TUNE_AVG_PARK_LOADPOL = 24 /* AVG_WIN_MODE 3: cache policy of the ring's buffer loads, 0 default |
                                     1 nt | 2 sc1 | 3 sc1 nt (ring 2, up to 2 slots at height 1) */
};
int fa_tune(int knob, int value);
int64_t fa_stream_read_blocks(int64_t bytes);
int fa_stream_read(const void* src, int64_t bytes, void* sink, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FEDAGG_PROBE_H */
