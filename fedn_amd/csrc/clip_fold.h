// clip_fold.h — the centred-clipping fold of up to kMaxK client buffers into a running accumulator
// (fa_clip_fold, kernel k_clip_fold): what moves the centre of a round of MORE than kMaxK clients, one launch
// per chunk of the clients, the accumulator carried between the launches in the compute type.
//
// Included by fedagg.hip inside its anonymous namespace, after cclip.h: from wmean_dist.h it takes WmTraits,
// WmTable, wm_out and wm_check_step, from cclip.h cc_center, from pair_dist.h PairItem and pair_cvt. With C the
// compute type and O the output type of the dtype family, v the centre in O and c_k = C(coef[k]), per element
//     acc = carry_in[p] (C) where a carry comes in, else C(v[p])
//     acc = acc + c_k (C(u_k[p]) - C(v[p]))            over the launch's clients with c_k != 0, in index order
//     carry_out[p] = acc (C),   out[p] = O(acc)         whichever is given
// the difference, the product and the add each rounded once (no FMA: -ffp-contract=off). A chain of launches
// over consecutive chunks of a round — the first without carry_in, the last with out — gives k_cclip_dist's v'
// and tests/cclip_ref.py::step bit for bit wherever it is cut: the carry holds acc exactly and the differences
// are always taken to the centre the round started from. DESIGN.md §3.13 has the definition and the
// resource table.
//
// Shape: a streaming fold like k_fedavg. The host compacts the table to the live clients (c_k != 0: a client
// with coefficient 0 is never read). A lane owns ITEMS of EV = 16 / sizeof(T) elements: it keeps acc and C(v) of
// its item in registers, loads the clients' 16-byte items kClipAhead at a time before it folds any of them, and
// stores the item with 16-byte stores. The centre (O) and the carries (C) of an item are EV elements too, so
// one or two 16-byte items each (bf16 / f16 / i32: two). No LDS, no atomic, nothing crosses lanes. An item
// behind a pointer off 16-byte alignment, and the ragged last item, go element by element through the same
// clip_fold_term: the same bits. A lane reads its item of the centre and of carry_in before it stores the same
// elements and items are disjoint across lanes, so out may be the centre and carry_out may be carry_in.

constexpr int kClipAhead = 8;            // clients' items a lane loads before it folds them
constexpr int kClipMaxBlocks = 2048;     // the grid's bound: 8 workgroups a CU (grid-stride beyond)

template <typename C>
__device__ __forceinline__ C clip_fold_term(C acc, C c, C u, C vc) {
    const C dl = u - vc;
    const C p = c * dl;
    return acc + p;
}

// `tab`: the launch's live clients, compacted (pointer, C(c_k)); L of them (0: nothing to fold)
template <typename T>
__global__ void __launch_bounds__(kBlock)
k_clip_fold(typename WmTraits<T>::O* out, typename WmTraits<T>::C* carry_out, const typename WmTraits<T>::C* carry_in,
            const typename WmTraits<T>::O* center, const WmTable<typename WmTraits<T>::C> tab, const int L,
            const int64_t P, const int vec) {
    using C = typename WmTraits<T>::C;
    using O = typename WmTraits<T>::O;
    constexpr int EV = 16 / (int)sizeof(T);            // elements of an item
    constexpr int EVO = 16 / (int)sizeof(O), NO = EV / EVO;     // the centre's / out's 16-byte items of one item
    constexpr int EVC = 16 / (int)sizeof(C), NC = EV / EVC;     // the carries'
    constexpr int U = kClipAhead;
    static_assert(NO >= 1 && NC >= 1 && NO * EVO == EV && NC * EVC == EV, "an item is whole 16-byte items of O and of C");
    const int64_t items = (P + EV - 1) / EV;
    for (int64_t it = (int64_t)blockIdx.x * kBlock + threadIdx.x; it < items; it += (int64_t)gridDim.x * kBlock) {
        const int64_t i0 = it * EV;
        if (vec && i0 + EV <= P) {
            C vc[EV], acc[EV];
            {
                PairItem<O> cv[NO];
#pragma unroll
                for (int j = 0; j < NO; ++j) cv[j].v = *reinterpret_cast<const uint4*>(center + i0 + j * EVO);
#pragma unroll
                for (int e = 0; e < EV; ++e) vc[e] = cc_center(cv[e / EVO].e[e % EVO], C{});
            }
            if (carry_in) {
                PairItem<C> ci[NC];
#pragma unroll
                for (int j = 0; j < NC; ++j) ci[j].v = *reinterpret_cast<const uint4*>(carry_in + i0 + j * EVC);
#pragma unroll
                for (int e = 0; e < EV; ++e) acc[e] = ci[e / EVC].e[e % EVC];
            } else {
#pragma unroll
                for (int e = 0; e < EV; ++e) acc[e] = vc[e];
            }
            int k = 0;
            for (; k + U <= L; k += U) {
                PairItem<T> y[U];
#pragma unroll
                for (int u = 0; u < U; ++u)
                    y[u].v = *reinterpret_cast<const uint4*>(static_cast<const T*>(tab.ptr[k + u]) + i0);
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const C c = tab.b[k + u];
#pragma unroll
                    for (int e = 0; e < EV; ++e) acc[e] = clip_fold_term(acc[e], c, pair_cvt(y[u].e[e], C{}), vc[e]);
                }
            }
            for (; k < L; ++k) {
                PairItem<T> y;
                y.v = *reinterpret_cast<const uint4*>(static_cast<const T*>(tab.ptr[k]) + i0);
                const C c = tab.b[k];
#pragma unroll
                for (int e = 0; e < EV; ++e) acc[e] = clip_fold_term(acc[e], c, pair_cvt(y.e[e], C{}), vc[e]);
            }
            if (carry_out) {
                PairItem<C> co[NC];
#pragma unroll
                for (int e = 0; e < EV; ++e) co[e / EVC].e[e % EVC] = acc[e];
#pragma unroll
                for (int j = 0; j < NC; ++j) *reinterpret_cast<uint4*>(carry_out + i0 + j * EVC) = co[j].v;
            }
            if (out) {
                PairItem<O> ov[NO];
#pragma unroll
                for (int e = 0; e < EV; ++e) ov[e / EVO].e[e % EVO] = wm_out<O, C>(acc[e]);
#pragma unroll
                for (int j = 0; j < NO; ++j) *reinterpret_cast<uint4*>(out + i0 + j * EVO) = ov[j].v;
            }
        } else {
            const int n = P - i0 < EV ? (int)(P - i0) : EV;    // within [0, P)
            for (int q = 0; q < n; ++q) {
                const C vc = cc_center(center[i0 + q], C{});
                C acc = carry_in ? carry_in[i0 + q] : vc;
                for (int k = 0; k < L; ++k)
                    acc = clip_fold_term(acc, tab.b[k], pair_cvt(static_cast<const T*>(tab.ptr[k])[i0 + q], C{}), vc);
                if (carry_out) carry_out[i0 + q] = acc;
                if (out) out[i0 + q] = wm_out<O, C>(acc);
            }
        }
    }
}

// true when [a, a + na) and [b, b + nb) share a byte
inline bool clip_fold_overlap(const void* a, uintptr_t na, const void* b, uintptr_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + nb && y < x + na;
}

// The aliasing rule of fa_clip_fold at P > 0, every pointer that is given non-null: carry_in == carry_out and
// out == center exactly are the two legal aliases; any other overlap among out, the carries and the centre,
// and any overlap of one of those four with an update, is refused. (Two updates may overlap: both are only
// read, as in every other entry point.)
inline int clip_fold_check_overlap(const void* out, const void* carry_out, const void* carry_in, const void* center,
                                   const void* const* ups, int K, int64_t P, size_t osize, size_t csize, size_t tsize) {
    struct Span {
        const void* p;
        uintptr_t n;
        const char* name;
    };
    const Span s[4] = {{out, (uintptr_t)P * osize, "out"},
                       {carry_out, (uintptr_t)P * csize, "carry_out"},
                       {carry_in, (uintptr_t)P * csize, "carry_in"},
                       {center, (uintptr_t)P * osize, "center"}};
    for (int i = 0; i < 4; ++i) {
        if (!s[i].p) continue;
        for (int j = i + 1; j < 4; ++j) {
            if (!s[j].p) continue;
            const bool alias = (i == 0 && j == 3) || (i == 1 && j == 2);     // out / center, carry_out / carry_in
            if (alias && s[i].p == s[j].p) continue;
            if (clip_fold_overlap(s[i].p, s[i].n, s[j].p, s[j].n))
                return fail(FA_EINVAL, "fa_clip_fold: %s and %s overlap%s", s[i].name, s[j].name,
                            alias ? " without being the same buffer" : "");
        }
        for (int k = 0; k < K; ++k)
            if (ups[k] && clip_fold_overlap(s[i].p, s[i].n, ups[k], (uintptr_t)P * tsize))
                return fail(FA_EINVAL, "fa_clip_fold: %s and updates[%d] overlap", s[i].name, k);
    }
    return FA_OK;
}

template <typename T>
int launch_clip_fold(void* out, void* carry_out, const void* carry_in, const void* center, const void* const* ups,
                     const double* cc, int K, int64_t P, hipStream_t st) {
    using C = typename WmTraits<T>::C;
    using O = typename WmTraits<T>::O;
    constexpr int EV = 16 / (int)sizeof(T);
    WmTable<C> tab;
    int L = 0;
    bool vec = aligned16(center) && (!out || aligned16(out)) && (!carry_out || aligned16(carry_out)) &&
               (!carry_in || aligned16(carry_in));
    for (int k = 0; k < K; ++k) {
        if (cc[k] == 0.0) continue;                          // never read
        tab.ptr[L] = ups[k];
        tab.b[L] = (C)cc[k];
        vec = vec && aligned16(ups[k]);
        ++L;
    }
    for (int k = L; k < kMaxK; ++k) {
        tab.ptr[k] = nullptr;
        tab.b[k] = C(0);
    }
    const int64_t items = (P + EV - 1) / EV;
    const dim3 grid((unsigned)std::min<int64_t>((items + kBlock - 1) / kBlock, kClipMaxBlocks));
    g_kernel = "k_clip_fold";
    hipLaunchKernelGGL((k_clip_fold<T>), grid, dim3(kBlock), 0, st, static_cast<O*>(out), static_cast<C*>(carry_out),
                       static_cast<const C*>(carry_in), static_cast<const O*>(center), tab, L, P, (int)vec);
    return check_launch("fa_clip_fold: kernel launch");
}
