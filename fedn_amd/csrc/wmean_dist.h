// wmean_dist.h — weighted mean of K client buffers and the K squared distances to it, in one pass
// (fa_weighted_mean_sqdist, kernel k_wmean_dist): one smoothed Weiszfeld step of the geometric median.
//
// Included by fedagg.hip inside its anonymous namespace, after pair_dist.h (it uses that file's
// conversions, 16-byte loads and fused multiply-add, fold_rules.h's element types, host_common.h's for_dtype,
// for_kp, fill_ptrs and order_out_dtype, and fedagg.hip's error plumbing). Its host side — geometry, table
// builder, the finishing launch and the step entry points' argument checks — also serves cclip.h's kernel; the
// two kernels' bodies stay two copies (DESIGN.md §3.10 has the two attempts at one and their figures).
// With C the compute type of the dtype family (f32 for f32 / f16 / bf16, f64 for f64 / i32 / i64) and
// b_k = C(beta[k]):
//     z[p] = O(((b_a C(u_a[p]) + b_b C(u_b[p])) + ...))   over the clients with b_k != 0, in index order,
//     d[k] = sum_p (C(u_k[p]) - C(z[p]))^2                  for every k,
// every product, add and difference rounded once, the squares summed by FMA in chains of at most
// kWmChain terms in C, the chain totals in f64. DESIGN.md §3.9 has the definition and the resource table.
//
// Shape: a workgroup stages a tile of TE elements x K clients in LDS, converted to C, element-major (one
// row of K values per element, odd row stride KS = K | 1: lanes that walk rows hit distinct banks). K is
// padded to KP in {8, 16, 32, 64} and SPLIT = KP / 16 (1 below 32) lanes share an element: each folds
// the whole row into z with ONE running accumulator (the same z in all of them; lane 0 of the element
// stores it), then takes its own CK = KP / SPLIT <= 16 clients of the row a second time from LDS for one
// subtract and one FMA each into CK chains in registers. Every loop over clients is unrolled, so chains
// and weights are indexed by constants; a weight of 0 and a padded client are dropped by a select on a
// bit mask, not a branch (a padded client's column is the next row's data: read, never used). Few chains
// a lane keep the registers at four waves a SIMD, which this kernel lives on: it has no loads in flight
// while it computes, the other workgroups of the CU have. Every flush_tiles tiles the chains go through
// LDS: TPC threads a client add SEG lanes' totals each in lane order in f64, then one thread a client adds
// those sums in order to the workgroup's partial. Each workgroup writes its K partials to `work`;
// k_wmean_finish sums the workgroups' partials in index order and writes (or adds to) dist. Nothing
// depends on timing or on the device: same inputs, same bits.
//
// An item (16 bytes of one client) that lies inside [0, P) behind 16-byte-aligned pointers is one 16-byte
// load, otherwise element loads, zeros past P; the tile in LDS is the same either way, so are the bits.

constexpr int kWmChain = 32;            // terms one chain in C sums before it is flushed to f64 (<= R of fedagg.h)
constexpr int kWmTileBytes = 32768;     // LDS of the tile
constexpr int kWmTileMax = 512;         // elements of a tile at most
constexpr int kWmChains = 16;           // chains a lane keeps at most (CK)
constexpr int kWmItems = kWmTileBytes / 16 / kBlock;      // 16-B items a lane fetches per tile, at most
static_assert(kWmChain <= FA_PAIR_CHAIN_TERMS, "the error bound is stated for chains of at most R terms");

constexpr int wm_kp(int K) { return K <= 8 ? 8 : (K <= 16 ? 16 : (K <= 32 ? 32 : 64)); }
constexpr int wm_ck(int KP) { return KP < kWmChains ? KP : kWmChains; }

struct WmGeom {
    int TE;      // elements per tile, a multiple of 8 (a tile starts on a 16-B boundary in every dtype)
    int KS;      // row stride in values
    int FT;      // tiles between two flushes
    int GRID;    // workgroups at most: `waves` a CU of a 256-CU part, all resident (a constant: the
                 // partition must not depend on the device)
};

// `cols`: columns of the tile, K (k_wmean_dist) or K + 1 (k_cclip_dist, cclip.h: the centre's)
inline WmGeom wm_geom(int K, int csize, int waves, int cols) {
    WmGeom g;
    const int KP = wm_kp(K);
    g.KS = cols | 1;
    const int te = kWmTileBytes / (g.KS * csize);
    g.TE = (te < kWmTileMax ? te : kWmTileMax) / 8 * 8;
    const int sl = kBlock / (KP / wm_ck(KP));          // elements the lanes cover at a time
    g.FT = kWmChain / ((g.TE + sl - 1) / sl);
    g.GRID = 256 * waves;
    return g;
}

template <typename C>
struct WmTable {
    const void* ptr[kMaxK];
    C b[kMaxK];                          // C(beta[k])
};

// T: update dtype; C: compute type; O: output storage type (ops.order_mean_dtype's table)
// WAVES: waves a SIMD the registers are held to (unpacking the 16-byte items of the narrow types takes more
// registers), and so workgroups a CU: the grid cap counts on it
template <typename T> struct WmTraits { using C = float; using O = float; static constexpr int WAVES = 4; };
template <> struct WmTraits<bf16> { using C = float; using O = float; static constexpr int WAVES = 3; };
template <> struct WmTraits<f16> { using C = float; using O = f16; static constexpr int WAVES = 3; };
template <> struct WmTraits<double> { using C = double; using O = double; static constexpr int WAVES = 4; };
template <> struct WmTraits<int32_t> { using C = double; using O = double; static constexpr int WAVES = 3; };
template <> struct WmTraits<int64_t> { using C = double; using O = double; static constexpr int WAVES = 4; };

template <typename T> constexpr int wm_waves(int KP) {
    return std::is_same<T, f16>::value && KP >= 32 ? 2 : WmTraits<T>::WAVES;
}

template <typename O, typename C> __device__ __forceinline__ O wm_out(C v) { return v; }
template <> __device__ __forceinline__ f16 wm_out<f16, float>(float v) { return f16{f32_to_f16(v)}; }
__device__ __forceinline__ float wm_back(float v) { return v; }
__device__ __forceinline__ double wm_back(double v) { return v; }
__device__ __forceinline__ float wm_back(f16 v) { return f16_to_f32(v.bits); }

// `live`: bit k set for every client after the first with a nonzero weight (the first, kfirst, starts the sum)
template <typename T, int KP, int CK>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(wm_waves<T>(KP), wm_waves<T>(KP))))
k_wmean_dist(typename WmTraits<T>::O* __restrict__ out, double* __restrict__ work,
             const WmTable<typename WmTraits<T>::C> tab, const int K, const int kfirst, const unsigned long long live,
             const int64_t P, const int TE, const int KS, const int flush_tiles, const int vec) {
    using C = typename WmTraits<T>::C;
    using O = typename WmTraits<T>::O;
    constexpr int EV = 16 / (int)sizeof(T);
    constexpr int TB = kWmTileBytes;
    constexpr int NI = kWmItems;
    __shared__ __attribute__((aligned(16))) unsigned char smem[TB + 512];   // (+ 64 values: a padded client of the last row)
    __shared__ const void* sptr[kMaxK];                // a lane indexes them by a client number that is not uniform
    C* tile = reinterpret_cast<C*>(smem);
    const int t = threadIdx.x;
    if (t < K) sptr[t] = tab.ptr[t];

    // A lane's 16-B items are the same (client, chunk of the tile) in every tile: found once.
    const int CH = TE / EV;                            // 16-B items per client and tile
    const int total = K * CH;                          // <= NI * kBlock: the tile holds them converted
    unsigned item[NI];                                 // client << 16 | chunk
#pragma unroll
    for (int n = 0; n < NI; ++n) {
        const int it = t + n * kBlock;
        const int k = it / CH;
        item[n] = it < total ? (unsigned)k << 16 | (unsigned)(it - k * CH) : 0xFFFFFFFFu;
    }
    __syncthreads();

    uint4 pre[NI];                                     // a tile's items between their loads and the tile
    auto fetch = [&](int64_t ti) {
        const int64_t e0 = ti * TE;
#pragma unroll
        for (int n = 0; n < NI; ++n) {
            pre[n] = make_uint4(0u, 0u, 0u, 0u);
            if (item[n] != 0xFFFFFFFFu)
                pre[n] = pair_load<T>(sptr[item[n] >> 16], e0 + (int64_t)(item[n] & 0xFFFFu) * EV, P, vec != 0);
        }
    };
    auto put = [&]() {                                 // the items, converted, into the tile
#pragma unroll
        for (int n = 0; n < NI; ++n) {
            if (item[n] != 0xFFFFFFFFu) {
                PairItem<T> u;
                u.v = pre[n];
                C* dst = tile + (int)(item[n] & 0xFFFFu) * EV * KS + (int)(item[n] >> 16);
#pragma unroll
                for (int q = 0; q < EV; ++q) dst[q * KS] = pair_cvt(u.e[q], C{});
            }
        }
    };

    // lane t: element slot t / SPLIT (+ j * SL), clients sub * CK .. sub * CK + CK - 1 of its chains
    constexpr int SPLIT = KP / CK;                     // lanes an element
    constexpr int SL = kBlock / SPLIT;                 // elements the lanes cover at a time
    constexpr int FK = CK < 16 ? CK : 16;              // chains of a lane per flush pass
    constexpr int NC = SPLIT * FK;                     // clients per flush pass
    constexpr int TPC = kBlock / NC;                   // threads a client in the flush
    constexpr int SEG = SL / TPC;                      // lanes' totals a thread adds
    static_assert(KP % CK == 0 && CK % FK == 0 && kBlock % NC == 0 && SL % TPC == 0, "flush geometry");
    static_assert(NC * SL * (int)sizeof(double) <= TB, "the flush stages its pass in the tile");
    const int sub = t % SPLIT, slot = t / SPLIT;
    __shared__ double part64[kMaxK];                   // the workgroup's f64 partials
    __shared__ double stage2[kBlock];
    if (t < kMaxK) part64[t] = 0.0;
    C chain[CK];
#pragma unroll
    for (int i = 0; i < CK; ++i) chain[i] = C(0);
    auto flush = [&]() {                               // every thread calls it, between two tiles (barriers inside)
        double* stage = reinterpret_cast<double*>(smem);          // [client of the pass][slot]
#pragma unroll
        for (int ih = 0; ih < CK; ih += FK) {
#pragma unroll
            for (int i = 0; i < FK; ++i) stage[(sub * FK + i) * SL + slot] = (double)chain[ih + i];
            __syncthreads();
            {
                const int c = t / TPC, j = t % TPC;    // TPC threads a client, SEG slots each, in slot order
                double sum = 0.0;
#pragma unroll
                for (int i = 0; i < SEG; ++i) sum += stage[c * SL + j * SEG + i];
                stage2[t] = sum;
            }
            __syncthreads();
            if (t < NC) {
                const int k = (t / FK) * CK + ih + t % FK;
                double sum = 0.0;
#pragma unroll
                for (int j = 0; j < TPC; ++j) sum += stage2[t * TPC + j];
                if (k < K) part64[k] += sum;
            }
            __syncthreads();
        }
#pragma unroll
        for (int i = 0; i < CK; ++i) chain[i] = C(0);
    };

    const int64_t ntiles = (P + TE - 1) / TE;
    const C bfirst = tab.b[kfirst];
    int walked = 0;
    int64_t ti = blockIdx.x;
    for (; ti < ntiles; ti += gridDim.x) {
        fetch(ti);
        put();
        __syncthreads();
        const int64_t e0 = ti * TE;
        const int n = P - e0 < TE ? (int)(P - e0) : TE;
        for (int e = slot; e < n; e += SL) {
            const C* row = tile + e * KS;
            C acc = bfirst * row[kfirst];
#pragma unroll
            for (int k = 1; k < KP; ++k) {             // (k >= K reads the next row's values: never selected)
                const C p = tab.b[k] * row[k];
                const C s = acc + p;
                acc = (live >> k & 1ull) ? s : acc;    // a client with weight 0 is no part of z
            }
            const O z = wm_out<O, C>(acc);
            if (out && sub == 0) out[e0 + e] = z;
            const C zc = wm_back(z);
            const C* mine = row + sub * CK;
#pragma unroll
            for (int i = 0; i < CK; ++i) {
                const C d = mine[i] - zc;
                chain[i] = pair_fma(d, chain[i]);      // (a client >= K: a chain nobody reads)
            }
        }
        __syncthreads();                               // the tile is read
        if (++walked == flush_tiles) {                 // the same count in every lane: a uniform branch
            flush();
            walked = 0;
        }
    }
    flush();
    if (t < K) work[(int64_t)blockIdx.x * kMaxK + t] = part64[t];
}

// dist[k] from the nwg partials, in workgroup order
__global__ void __launch_bounds__(kMaxK)
k_wmean_finish(double* __restrict__ dist, const double* __restrict__ work, const int K, const int nwg,
               const int accumulate) {
    const int k = threadIdx.x;
    if (k >= K) return;
    double sum = 0.0;
#pragma unroll 8
    for (int w = 0; w < nwg; ++w) sum += work[(int64_t)w * kMaxK + k];
    dist[k] = accumulate ? dist[k] + sum : sum;
}

// the geometry of (dtype, K) at `cols` tile columns; dtype is one of the six
inline WmGeom wm_geom_dt(int dtype, int K, int cols) {
    return for_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return wm_geom(K, (int)sizeof(typename WmTraits<T>::C), wm_waves<T>(wm_kp(K)), cols);
    });
}

inline int64_t wm_workgroups(int64_t P, const WmGeom& gm) {
    return std::min<int64_t>((P + gm.TE - 1) / gm.TE, gm.GRID);
}

// The table of a launch from the update pointers and the coefficients already cast to C (bc[k] is C(beta[k])
// held in a double: the cast back is exact). Returns vec (every update 16-byte aligned) and live: bit k for
// every client with a nonzero coefficient — with skip_first, but for the first of them (k_wmean_dist starts its
// sum with that client; k_cclip_dist starts with the centre).
struct WmLive {
    bool vec;
    unsigned long long live;
};

template <typename C>
WmLive wm_fill_table(WmTable<C>& tab, const void* const* ups, const double* bc, int K, bool skip_first) {
    WmLive r{fill_ptrs(tab.ptr, ups, K), 0};
    for (int k = 0; k < kMaxK; ++k) {
        tab.b[k] = k < K ? (C)bc[k] : C(0);
        if (k >= K || bc[k] == 0.0) continue;
        if (skip_first) skip_first = false;
        else r.live |= 1ull << k;
    }
    return r;
}

// the launch that follows either distance kernel: dist[k] from the nwg partials; `who` names the failed launch
inline int wm_finish(double* dist, double* work, int K, int nwg, int accumulate, hipStream_t st, const char* who) {
    hipLaunchKernelGGL(k_wmean_finish, dim3(1), dim3(kMaxK), 0, st, dist, work, K, nwg, accumulate);
    return check_launch(who);
}

// The argument checks of the two step entry points, reported in `who`'s name: `ptrs` (every pointer the entry
// point needs is there), K, P, the dtype family, the output dtype that goes with the updates' (`gives`: what the
// updates do to it, for the message), and the K coefficients `coef` (called `cname`): each finite and >= 0, cast
// to the compute type once into cc[k], where it must still be finite.
inline int wm_check_step(const char* who, const char* cname, const char* gives, bool ptrs, int out_dtype, int upd_dtype,
                         const double* coef, int K, int64_t P, double* cc) {
    if (!ptrs) return fail(FA_EINVAL, "%s: null pointer argument", who);
    if (K < 1 || K > kMaxK) return fail(FA_EINVAL, "%s: K=%d outside 1..%d", who, K, kMaxK);
    if (P < 0) return fail(FA_EINVAL, "%s: negative size (P=%lld)", who, (long long)P);
    const int fam = pair_family(upd_dtype);
    if (!fam) return fail(FA_EDTYPE, "%s: unsupported dtype %d", who, upd_dtype);
    const int want = order_out_dtype(upd_dtype);
    if (out_dtype != want)
        return fail(FA_EDTYPE, "%s: updates of dtype %d %s of dtype %d, not %d", who, upd_dtype, gives, want, out_dtype);
    for (int k = 0; k < K; ++k) {
        if (!(coef[k] >= 0.0) || std::isinf(coef[k]))
            return fail(FA_EINVAL, "%s: %s[%d]=%g is negative or not finite", who, cname, k, coef[k]);
        cc[k] = fam == 32 ? (double)(float)coef[k] : coef[k];
        if (std::isinf(cc[k]))
            return fail(FA_EINVAL, "%s: %s[%d]=%g is not finite in the compute type", who, cname, k, coef[k]);
    }
    return FA_OK;
}

template <typename T>
int launch_wmean_dist(void* out, double* dist, const void* const* ups, const double* bc, int kfirst, int K, int64_t P,
                      int accumulate, double* work, hipStream_t st) {
    using C = typename WmTraits<T>::C;
    using O = typename WmTraits<T>::O;
    WmTable<C> tab;
    const WmLive tl = wm_fill_table(tab, ups, bc, K, true);
    const WmGeom gm = wm_geom(K, (int)sizeof(C), wm_waves<T>(wm_kp(K)), K);
    const int nwg = (int)wm_workgroups(P, gm);
    g_kernel = "k_wmean_dist";
    if (nwg > 0)
        for_kp<8>(wm_kp(K), [&](auto kp) {                     // KP is the geometry's own wm_kp(K)
            constexpr int KP = decltype(kp)::value;
            hipLaunchKernelGGL((k_wmean_dist<T, KP, wm_ck(KP)>), dim3((unsigned)nwg), dim3(kBlock), 0, st,
                               static_cast<O*>(out), work, tab, K, kfirst, tl.live, P, gm.TE, gm.KS, gm.FT, (int)tl.vec);
        });
    return wm_finish(dist, work, K, nwg, accumulate, st, "fa_weighted_mean_sqdist: kernel launch");
}
