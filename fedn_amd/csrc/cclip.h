// cclip.h — one centred-clipping step: the centre v moved by the clipped differences of K client buffers to
// it, and the K squared distances to the new point, in one pass (fa_centered_clip_step, kernel k_cclip_dist).
//
// Included by fedagg.hip inside its anonymous namespace, after wmean_dist.h: it is that file's kernel
// "with one extra client". This file holds the kernel and its launcher alone; from wmean_dist.h it takes the
// tile constants (kWm*), wm_kp / wm_ck / wm_waves, WmTraits, WmTable, wm_out / wm_back, and the whole host
// side: WmGeom and wm_geom at K + 1 tile columns, wm_workgroups, wm_fill_table and wm_finish
// (k_wmean_finish); the dispatch on KP is host_common.h's for_kp. With C the compute type and O the output type
// of the dtype family (WmTraits) and c_k = C(coef[k]):
//     v'[p] = O((C(v[p]) + c_a (C(u_a[p]) - C(v[p]))) + c_b (C(u_b[p]) - C(v[p])) + ...)
//                                                         over the clients with c_k != 0, in index order,
//     d[k]  = sum_p (C(u_k[p]) - C(v'[p]))^2               for every k,
// every difference, product and add rounded once, the squares summed as in k_wmean_dist. DESIGN.md §3.10 has
// the definition and the resource table.
//
// Shape: k_wmean_dist's, with the centre's tile staged as column K of the LDS tile (row stride
// KS = (K + 1) | 1). The centre's 16-byte items follow the clients' in the lanes' item list (a tile of K + 1
// columns holds them all) and are fetched with them; where O != T they hold another number of elements and
// convert differently, which one compare per item tells. For bf16 updates that second path costs the
// registers of a wave, so there lane t < TE / 4 fetches item t of the centre behind the clients' items
// instead. Either way the centre's tile is in LDS before the barrier: every read of a tile's centre
// precedes every store of v' to it, and tiles are disjoint across workgroups and across a workgroup's
// steps, so out may be the centre itself. Nothing depends on timing, on the device or on a pointer's
// alignment.

__device__ __forceinline__ float cc_center(float v, float) { return v; }
__device__ __forceinline__ float cc_center(f16 v, float) { return f16_to_f32(v.bits); }
__device__ __forceinline__ double cc_center(double v, double) { return v; }

// `live`: bit k set for every client with a nonzero coefficient
template <typename T, int KP, int CK>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(wm_waves<T>(KP), wm_waves<T>(KP))))
k_cclip_dist(typename WmTraits<T>::O* out, const typename WmTraits<T>::O* center, double* __restrict__ work,
             const WmTable<typename WmTraits<T>::C> tab, const int K, const unsigned long long live, const int64_t P,
             const int TE, const int KS, const int flush_tiles, const int vec, const int cvec) {
    using C = typename WmTraits<T>::C;
    using O = typename WmTraits<T>::O;
    constexpr int EV = 16 / (int)sizeof(T);
    constexpr int EVO = 16 / (int)sizeof(O);
    constexpr int TB = kWmTileBytes;
    constexpr int NI = kWmItems;
    constexpr bool SAME = std::is_same<T, O>::value;   // the centre is one more client column, item for item
    constexpr bool LATE = std::is_same<T, bf16>::value;   // its items are fetched behind the clients' (registers)
    static_assert(!LATE || kWmTileMax / EVO <= kBlock, "a late centre: one item a lane");
    __shared__ __attribute__((aligned(16))) unsigned char smem[TB + 512];   // (+ 64 values: a padded client of the last row)
    __shared__ const void* sptr[kMaxK + 1];            // a lane indexes them by a column number that is not uniform
    C* tile = reinterpret_cast<C*>(smem);
    const int t = threadIdx.x;
    if (t < K) sptr[t] = tab.ptr[t];
    if (t == K) sptr[t] = center;

    // A lane's 16-B items are the same (column, chunk of the tile) in every tile: found once. Column K is
    // the centre's, in items of EVO elements.
    const int CH = TE / EV;                            // 16-B items per client and tile
    const int CHO = TE / EVO;                          // ... of the centre
    const int nclient = K * CH;
    const int total = nclient + (LATE ? 0 : CHO);      // <= NI * kBlock: the tile holds them converted
    unsigned item[NI];                                 // column << 16 | chunk
#pragma unroll
    for (int n = 0; n < NI; ++n) {
        const int it = t + n * kBlock;
        const int k = it < nclient ? it / CH : K;
        item[n] = it < total ? (unsigned)k << 16 | (unsigned)(it - k * CH) : 0xFFFFFFFFu;
    }
    __syncthreads();

    uint4 pre[NI];                                     // a tile's items between their loads and the tile
    auto fetch = [&](int64_t ti) {
        const int64_t e0 = ti * TE;
#pragma unroll
        for (int n = 0; n < NI; ++n) {
            pre[n] = make_uint4(0u, 0u, 0u, 0u);
            if (item[n] != 0xFFFFFFFFu) {
                const int k = (int)(item[n] >> 16), c = (int)(item[n] & 0xFFFFu);
                if (SAME || LATE || k != K) pre[n] = pair_load<T>(sptr[k], e0 + (int64_t)c * EV, P, (k == K ? cvec : vec) != 0);
                else pre[n] = pair_load<O>(sptr[K], e0 + (int64_t)c * EVO, P, cvec != 0);
            }
        }
    };
    auto put = [&](int64_t ti) {                       // the items, converted, into the tile
#pragma unroll
        for (int n = 0; n < NI; ++n) {
            if (item[n] != 0xFFFFFFFFu) {
                const int k = (int)(item[n] >> 16), c = (int)(item[n] & 0xFFFFu);
                if (SAME || LATE || k != K) {
                    PairItem<T> u;
                    u.v = pre[n];
                    C* dst = tile + c * EV * KS + k;
#pragma unroll
                    for (int q = 0; q < EV; ++q) dst[q * KS] = pair_cvt(u.e[q], C{});
                } else {
                    PairItem<O> u;
                    u.v = pre[n];
                    C* dst = tile + c * EVO * KS + K;
#pragma unroll
                    for (int q = 0; q < EVO; ++q) dst[q * KS] = cc_center(u.e[q], C{});
                }
            }
        }
        if (LATE && t < CHO) {
            PairItem<O> u;
            u.v = pair_load<O>(center, ti * TE + (int64_t)t * EVO, P, cvec != 0);
            C* dst = tile + t * EVO * KS + K;
#pragma unroll
            for (int q = 0; q < EVO; ++q) dst[q * KS] = cc_center(u.e[q], C{});
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
    int walked = 0;
    int64_t ti = blockIdx.x;
    for (; ti < ntiles; ti += gridDim.x) {
        fetch(ti);
        put(ti);
        __syncthreads();                               // the centre's tile is read: stores to it may follow
        const int64_t e0 = ti * TE;
        const int n = P - e0 < TE ? (int)(P - e0) : TE;
        for (int e = slot; e < n; e += SL) {
            const C* row = tile + e * KS;
            const C vc = row[K];
            C acc = vc;
#pragma unroll
            for (int k = 0; k < KP; ++k) {             // (k >= K reads the centre or the next row: never selected)
                const C dl = row[k] - vc;
                const C p = tab.b[k] * dl;
                const C s = acc + p;
                acc = (live >> k & 1ull) ? s : acc;    // a client with coefficient 0 is no part of v'
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

template <typename T>
int launch_cclip_dist(void* out, const void* center, double* dist, const void* const* ups, const double* cc, int K,
                      int64_t P, int accumulate, double* work, hipStream_t st) {
    using C = typename WmTraits<T>::C;
    using O = typename WmTraits<T>::O;
    WmTable<C> tab;
    const WmLive tl = wm_fill_table(tab, ups, cc, K, false);
    const WmGeom gm = wm_geom(K, (int)sizeof(C), wm_waves<T>(wm_kp(K)), K + 1);
    const int nwg = (int)wm_workgroups(P, gm);
    const bool cvec = aligned16(center);
    g_kernel = "k_cclip_dist";
    if (nwg > 0)
        for_kp<8>(wm_kp(K), [&](auto kp) {                     // KP is the geometry's own wm_kp(K)
            constexpr int KP = decltype(kp)::value;
            hipLaunchKernelGGL((k_cclip_dist<T, KP, wm_ck(KP)>), dim3((unsigned)nwg), dim3(kBlock), 0, st,
                               static_cast<O*>(out), static_cast<const O*>(center), work, tab, K, tl.live, P, gm.TE, gm.KS,
                               gm.FT, (int)tl.vec, (int)cvec);
        });
    return wm_finish(dist, work, K, nwg, accumulate, st, "fa_centered_clip_step: kernel launch");
}
