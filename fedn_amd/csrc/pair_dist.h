// pair_dist.h — pairwise squared distances of K client buffers (fa_pairwise_sqdist, kernel k_pair_sqdist).
//
// Included by fedagg.hip inside its anonymous namespace (it uses fold_rules.h's element types, host_common.h's
// fill_ptrs and for_kp, and that file's error plumbing). D[i][j] = sum_p (C(u_i[p]) - C(u_j[p]))^2 in the
// compute type C of the dtype family: f32 for f32 / f16 / bf16 (widened exactly), f64 for f64 / i32 / i64 (one
// rounding). DESIGN.md §3.8 has the definition, the error bound and the resource table.
//
// Shape: a workgroup stages a tile of TE elements x KP clients in LDS, converted to C, element-major
// (one padded row of KP values per element). A lane owns one B x B block (bi <= bj) of the client-pair
// matrix and every G-th element of the tile: per element it reads its B + B values with wide LDS reads
// and runs one subtract and one fused multiply-add per pair into B*B chains in C. Before a chain could
// exceed kPairChain terms the workgroup flushes: the chains go through LDS to owner threads, which add
// the G lanes' totals of a slot to the workgroup's f64 partial in a fixed order. Each workgroup writes
// its partial to `work`; k_pair_finish sums the workgroups' partials in index order, writes (or adds
// to) D's upper triangle and mirrors it. Nothing here depends on timing: same inputs, same bits.
//
// The next tile's global loads are issued before the current tile is computed and parked in registers.
// A tile that lies wholly inside [0, P) behind 16-byte-aligned pointers is fetched with 16-byte loads;
// otherwise element by element, zeros past P (a zero in every client adds exactly 0 to every chain) —
// the element-to-chain map is the same, so are the bits.

constexpr int kPairChain = FA_PAIR_CHAIN_TERMS;   // R (fedagg.h): terms one chain in C sums before it is flushed to f64
constexpr int kPairGrid = 512;          // workgroups at most: two per CU of a 256-CU part, all resident at every
                                        // register count below (a constant: the partition must not depend on the device)
constexpr int kPairTileBytes = 32768;   // LDS of the tile (half of it for C = f64: fewer parked loads, the
                                        // registers go to the f64 chains); the flush stages the chains in the same bytes
static_assert(kPairChain <= 1024, "the error bound (R + 4) * 2^-24 is stated for R <= 1024");

template <typename C, int KP>
struct PairGeom {
    static constexpr int KPV = KP;
    static constexpr int TB = sizeof(C) == 8 ? kPairTileBytes / 2 : kPairTileBytes;
    static constexpr int B = KP < 8 ? KP : 8;                 // a lane's block of the pair matrix: B x B
    static constexpr int NBK = KP / B;
    static constexpr int NB = NBK * (NBK + 1) / 2;            // blocks of the upper triangle, diagonal included
    static constexpr int G = kBlock / NB;                     // lanes per block: lane (g, blk) takes elements g, g + G, ...
    static constexpr int SLOTS = B * B;
    static constexpr int S = KP + 16 / (int)sizeof(C);        // row stride in values: one 16-B access of padding
    static constexpr int TE = TB / (S * (int)sizeof(C)) / 8 * 8;   // elements per tile, a multiple of 8
    static constexpr int PER_TILE = (TE + G - 1) / G;         // terms a chain gains per tile, at most
    static constexpr int SC0 = TB / (kBlock * (int)sizeof(C));
    static constexpr int SC = SLOTS < SC0 ? SLOTS : SC0;      // slots staged per flush pass
    static constexpr int EVMIN = sizeof(C) == 4 ? 4 : 2;      // fewest elements in 16 bytes (f32 / f64)
    static constexpr int NI = (KP * (TE / EVMIN) + kBlock - 1) / kBlock;       // 16-B items a lane parks per tile
    static constexpr int KW = KP < 16 ? KP : 16;              // clients across adjacent lanes of a load
    static constexpr int PART = SLOTS * NB;                   // doubles of one workgroup's partial
    static constexpr int AL = B * (int)sizeof(C) < 16 ? B * (int)sizeof(C) : 16;
    static_assert(G >= 1 && TE >= 8 && PER_TILE <= kPairChain, "tile geometry");
    static_assert(SLOTS % SC == 0 && kBlock * SC * (int)sizeof(C) <= TB, "flush staging");
    static_assert(TE * S * (int)sizeof(C) <= TB && (S * (int)sizeof(C)) % AL == 0, "tile rows");
    static_assert(kBlock % KW == 0, "a lane keeps its client column");
};

struct PairTable {
    const void* ptr[kMaxK];
};

__device__ __forceinline__ float pair_cvt(float v, float) { return v; }
__device__ __forceinline__ float pair_cvt(f16 v, float) { return f16_to_f32(v.bits); }
__device__ __forceinline__ float pair_cvt(bf16 v, float) { return bf16_to_f32(v.bits); }
__device__ __forceinline__ double pair_cvt(double v, double) { return v; }
__device__ __forceinline__ double pair_cvt(int32_t v, double) { return (double)v; }
__device__ __forceinline__ double pair_cvt(int64_t v, double) { return (double)v; }
__device__ __forceinline__ float pair_fma(float d, float a) { return __builtin_fmaf(d, d, a); }
__device__ __forceinline__ double pair_fma(double d, double a) { return __builtin_fma(d, d, a); }

template <typename T>
union PairItem {
    uint4 v;
    T e[16 / sizeof(T)];
};

// 16 bytes of client buffer `base` from element i0 on: one load where allowed, else element loads, zeros past P
template <typename T>
__device__ __forceinline__ uint4 pair_load(const void* base, int64_t i0, int64_t P, bool vec) {
    constexpr int EV = 16 / (int)sizeof(T);
    const T* p = static_cast<const T*>(base) + i0;
    if (vec && i0 + EV <= P) return *reinterpret_cast<const uint4*>(p);
    PairItem<T> u;
    u.v = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
    for (int q = 0; q < EV; ++q)
        if (i0 + q < P) u.e[q] = p[q];
    return u.v;
}

// the item's elements, converted, into one column of EV consecutive tile rows
template <typename T, typename C>
__device__ __forceinline__ void pair_put(uint4 raw, C* dst, int S) {
    constexpr int EV = 16 / (int)sizeof(T);
    PairItem<T> u;
    u.v = raw;
#pragma unroll
    for (int q = 0; q < EV; ++q) dst[q * S] = pair_cvt(u.e[q], C{});
}

template <typename C>
__device__ __forceinline__ uint4 pair_load_dt(int dtype, const void* base, int64_t i0, int64_t P, bool vec) {
    if (sizeof(C) == 4) {
        if (dtype == FA_F32) return pair_load<float>(base, i0, P, vec);
        if (dtype == FA_F16) return pair_load<f16>(base, i0, P, vec);
        return pair_load<bf16>(base, i0, P, vec);
    }
    if (dtype == FA_F64) return pair_load<double>(base, i0, P, vec);
    if (dtype == FA_I32) return pair_load<int32_t>(base, i0, P, vec);
    return pair_load<int64_t>(base, i0, P, vec);
}

template <typename C, int N, int AL>
__device__ __forceinline__ void pair_read(const C* p, C (&v)[N]) {
    __builtin_memcpy(v, __builtin_assume_aligned(p, AL), N * sizeof(C));
}

// The chains of every lane -> the workgroup's f64 partial, in a fixed order: SC slots at a time, lane t
// stages slot s at stage[s][t]; the owner thread of (slot, block) adds the G lanes' values g = 0, 1, ...
// in f64 and the total to acc64. Every thread of the workgroup calls it (barriers inside).
template <int KP, typename C, int NS>
__device__ __forceinline__ void pair_flush(C (&acc)[NS], C* stage, double* acc64, int t, bool active) {
    using GM = PairGeom<C, KP>;
    static_assert(NS == GM::SLOTS, "one chain per slot");
    __syncthreads();                                  // the tile's reads are over: its bytes are the stage now
#pragma unroll
    for (int h = 0; h < GM::SLOTS; h += GM::SC) {
        if (active) {
#pragma unroll
            for (int s = 0; s < GM::SC; ++s) stage[s * kBlock + t] = acc[h + s];
        }
        __syncthreads();
        for (int o = t; o < GM::SC * GM::NB; o += kBlock) {
            const int s = o / GM::NB, blk = o % GM::NB;
            double sum = 0.0;
            for (int g = 0; g < GM::G; ++g) sum += (double)stage[s * kBlock + g * GM::NB + blk];
            acc64[(h + s) * GM::NB + blk] += sum;
        }
        __syncthreads();
    }
#pragma unroll
    for (int s = 0; s < GM::SLOTS; ++s) acc[s] = C(0);
}

template <typename C, int KP>
__global__ void __launch_bounds__(kBlock)
k_pair_sqdist(double* __restrict__ work, const PairTable tab, const int K, const int dtype, const int64_t P,
              const int vec) {
    using GM = PairGeom<C, KP>;
    __shared__ __attribute__((aligned(16))) unsigned char smem[GM::TB];
    __shared__ double acc64[GM::PART];
    C* tile = reinterpret_cast<C*>(smem);
    const int t = threadIdx.x;
    const int g = t / GM::NB, blk = t % GM::NB;
    const bool active = g < GM::G;
    int bi = 0, bj = blk;                              // block blk of the upper triangle, rows first
    while (bj >= GM::NBK - bi) {
        bj -= GM::NBK - bi;
        ++bi;
    }
    bj += bi;
    for (int o = t; o < GM::PART; o += kBlock) acc64[o] = 0.0;

    const int ev = dtype == FA_F16 || dtype == FA_BF16 ? 8 : (dtype == FA_F32 || dtype == FA_I32 ? 4 : 2);
    const int CH = GM::TE / ev;                        // 16-B items per client and tile
    const int total = KP * CH;
    const int64_t ntiles = (P + GM::TE - 1) / GM::TE;
    const int klow = t % GM::KW;

    // The client pointers, in LDS (a lane indexes them by a client number that is not a constant). A
    // lane's 16-B items are the same (client, byte offset in the tile) in every tile: packed once. An
    // item past the table or of a padded client reads client 0 at offset 0 and is zeroed.
    __shared__ const char* sptr[KP];
    if (t < KP) sptr[t] = static_cast<const char*>(tab.ptr[t < K ? t : 0]);
    const int sz = 16 / ev;                            // bytes per element
    unsigned item[GM::NI];                             // client << 24 | byte offset
    unsigned live = 0;
#pragma unroll
    for (int n = 0; n < GM::NI; ++n) {
        const int it = t + n * kBlock;
        const int r = it / GM::KW;
        const int k = (r / CH) * GM::KW + klow, c = r % CH;
        const bool ok = it < total && k < K;
        item[n] = ok ? (unsigned)k << 24 | (unsigned)(16 * c) : 0u;
        live |= ok ? 1u << n : 0u;
    }
    __syncthreads();

    uint4 pre[GM::NI];
    auto fetch = [&](int64_t ti) {
        const int64_t e0 = ti * GM::TE;
        if (vec && e0 + GM::TE <= P) {                 // (uniform) the whole tile: unconditional 16-B loads
#pragma unroll
            for (int n = 0; n < GM::NI; ++n)
                pre[n] = *reinterpret_cast<const uint4*>(sptr[item[n] >> 24] + (item[n] & 0xFFFFFFu) + e0 * sz);
#pragma unroll
            for (int n = 0; n < GM::NI; ++n)
                if (!(live >> n & 1u)) pre[n] = make_uint4(0u, 0u, 0u, 0u);
            return;
        }
#pragma unroll
        for (int n = 0; n < GM::NI; ++n) {
            pre[n] = make_uint4(0u, 0u, 0u, 0u);
            if (live >> n & 1u)
                pre[n] = pair_load_dt<C>(dtype, sptr[item[n] >> 24], e0 + (int64_t)(item[n] & 0xFFFFFFu) / sz, P, false);
        }
    };
    auto put = [&](auto tag) {                         // the parked items, converted, into the tile
        using T = decltype(tag);
#pragma unroll
        for (int n = 0; n < GM::NI; ++n) {
            const int it = t + n * kBlock;
            if (it < total) {
                const int r = it / GM::KW;
                const int k = (r / CH) * GM::KW + klow, c = r % CH;
                pair_put<T, C>(pre[n], tile + (c * ev) * GM::S + k, GM::S);      // clients K.. are zeros
            }
        }
    };

    C acc[GM::SLOTS];
#pragma unroll
    for (int s = 0; s < GM::SLOTS; ++s) acc[s] = C(0);
    int cnt = 0;
    int64_t ti = blockIdx.x;
    if (ti < ntiles) fetch(ti);
    for (; ti < ntiles; ti += gridDim.x) {
        __syncthreads();                               // the previous tile (or the flush) is read
        if constexpr (sizeof(C) == 4) {
            if (dtype == FA_F32) put(float{});
            else if (dtype == FA_F16) put(f16{});
            else put(bf16{});
        } else {
            if (dtype == FA_F64) put(double{});
            else if (dtype == FA_I32) put(int32_t{});
            else put(int64_t{});
        }
        __syncthreads();
        if (ti + gridDim.x < ntiles) fetch(ti + gridDim.x);
        if (active) {
            for (int e = g; e < GM::TE; e += GM::G) {
                const C* row = tile + e * GM::S;
                C a[GM::B], b[GM::B];
                pair_read<C, GM::B, GM::AL>(row + bi * GM::B, a);
                pair_read<C, GM::B, GM::AL>(row + bj * GM::B, b);
#pragma unroll
                for (int i = 0; i < GM::B; ++i)
#pragma unroll
                    for (int j = 0; j < GM::B; ++j) acc[i * GM::B + j] = pair_fma(a[i] - b[j], acc[i * GM::B + j]);
            }
        }
        cnt += GM::PER_TILE;
        if (cnt + GM::PER_TILE > kPairChain) {         // the same count in every lane: a uniform branch
            pair_flush<KP>(acc, tile, acc64, t, active);
            cnt = 0;
        }
    }
    pair_flush<KP>(acc, tile, acc64, t, active);
    for (int o = t; o < GM::PART; o += kBlock) work[(int64_t)blockIdx.x * GM::PART + o] = acc64[o];
}

// D's upper triangle from the nwg partials, in workgroup order, mirrored; the diagonal is 0
template <int KP>
__global__ void __launch_bounds__(kBlock)
k_pair_finish(double* __restrict__ D, const double* __restrict__ work, const int K, const int nwg,
              const int accumulate) {
    using GM = PairGeom<float, KP>;                    // B, NBK, NB, PART do not depend on C
    const int idx = blockIdx.x * kBlock + threadIdx.x;
    if (idx >= K * K) return;
    const int i = idx / K, j = idx % K;
    if (i == j) {
        if (!accumulate) D[idx] = 0.0;
        return;
    }
    if (i > j) return;
    const int bi = i / GM::B, bj = j / GM::B;
    const int blk = bi * GM::NBK - bi * (bi - 1) / 2 + (bj - bi);
    const int o = ((i % GM::B) * GM::B + (j % GM::B)) * GM::NB + blk;
    double sum = 0.0;
#pragma unroll 8
    for (int w = 0; w < nwg; ++w) sum += work[(int64_t)w * GM::PART + o];
    if (accumulate) {
        D[i * K + j] += sum;
        D[j * K + i] += sum;
    } else {
        D[i * K + j] = sum;
        D[j * K + i] = sum;
    }
}

// the compute family of an update dtype: 32 (f32 / f16 / bf16), 64 (f64 / i32 / i64), 0 for any other dtype
inline int pair_family(int dtype) {
    if (dtype == FA_F32 || dtype == FA_F16 || dtype == FA_BF16) return 32;
    return dtype == FA_F64 || dtype == FA_I32 || dtype == FA_I64 ? 64 : 0;
}

// f(PairGeom-carrying tag) for the (family, KP) of (dtype, K)
template <typename C, typename F>
int pair_for_kp(int K, F&& f) {
    return for_kp<2>(K, [&](auto kp) -> int { return f(PairGeom<C, decltype(kp)::value>{}); });
}

inline int64_t pair_workgroups(int64_t P, int TE) {
    return std::min<int64_t>((P + TE - 1) / TE, kPairGrid);
}

template <typename C>
int launch_pair_sqdist(double* D, const void* const* ups, int dtype, int K, int64_t P, int accumulate, double* work,
                       hipStream_t st) {
    PairTable tab;
    const bool vec = fill_ptrs(tab.ptr, ups, K);
    g_kernel = "k_pair_sqdist";
    return pair_for_kp<C>(K, [&](auto gm) -> int {
        using GM = decltype(gm);
        constexpr int KP = GM::KPV;
        const int nwg = K > 1 ? (int)pair_workgroups(P, GM::TE) : 0;
        if (nwg > 0)
            hipLaunchKernelGGL((k_pair_sqdist<C, KP>), dim3((unsigned)nwg), dim3(kBlock), 0, st, work, tab, K, dtype, P,
                               (int)vec);
        hipLaunchKernelGGL((k_pair_finish<KP>), dim3((unsigned)((K * K + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, D,
                           work, K, nwg, accumulate);
        return check_launch("fa_pairwise_sqdist: kernel launch");
    });
}
