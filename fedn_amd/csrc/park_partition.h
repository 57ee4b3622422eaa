// park_partition.h — how the parked fold (fedavg_park_body, fedavg_kernels.h) divides a model of P
// elements among its workgroups: one definition for the kernel, its launcher (fedavg_launch.h) and
// the CPU test (tests/test_park_partition_host.py, which compiles this file alone for the host).
//
// A small tile is `tile` elements (16 KiB of a client), a tall tile `height` consecutive small
// tiles. Whole tall tiles go through the load ring: workgroup b of a grid of G takes tall tiles b,
// b + G, ... Behind them lie up to height - 1 whole small tiles and at most one ragged tile; these
// "tail tiles" go through k_fedavg_tail, tail tile j to workgroup (ntall + j) mod G — the workgroups
// that come next in the ring's own order, distinct while there are at least as many as tail tiles.
#ifndef FEDAGG_PARK_PARTITION_H
#define FEDAGG_PARK_PARTITION_H

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FA_HD __host__ __device__ inline
#else
#define FA_HD inline
#endif

struct ParkPartition {
    int64_t ntall;   // whole tall tiles: elements [0, ntall * height * tile)
    int nleft;       // whole small tiles behind them, 0 .. height - 1
    int ragged;      // elements of the ragged tile behind those, 0 .. tile - 1
    FA_HD int ntail() const { return nleft + (ragged ? 1 : 0); }
    // what the grid is sized by: at most one workgroup per tall or tail tile
    FA_HD int64_t units() const { return ntall + ntail(); }
};

FA_HD ParkPartition park_partition(int64_t P, int64_t tile, int height) {
    const int64_t nsmall = P / tile;
    return {nsmall / height, (int)(nsmall % height), (int)(P % tile)};
}

// tall tiles of workgroup `wg`: wg, wg + grid, ... below ntall
FA_HD int64_t park_ring_tiles(const ParkPartition& p, int64_t grid, int64_t wg) {
    return wg < p.ntall ? (p.ntall - wg + grid - 1) / grid : 0;
}

// the workgroup that folds tail tile j (small tile ntall * height + j of the model)
FA_HD int64_t park_tail_owner(const ParkPartition& p, int64_t grid, int j) { return (p.ntall + j) % grid; }

#undef FA_HD
#endif  // FEDAGG_PARK_PARTITION_H
