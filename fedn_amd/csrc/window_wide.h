// window_wide.h — coordinate-wise mean of the `keep` values closest to the median over 1 .. 1024 client buffers
// (fa_median_window_mean_wide): "mean around median" (Xie, Koyejo and Gupta, 2018), and Bulyan's second stage at
// cohorts past 64.
//
// Included by fedagg.hip inside its anonymous namespace, after order_wide.h and median_window.h. The rule is
// median_window.h's bit for bit: the keys and their order, med kept in the accumulator type A,
// the window start a = #{ j in [0, K - keep) : (A(s[j + keep]) - med) < (med - A(s[j])) } through that header's
// window_moves, the ascending sum from s[a], one IEEE division by keep, order_out. The tile geometry, the
// wavefront's sort and the launch path are order_wide.h's (WideGeom, wide_sort, wide_store_block,
// launch_wide_kernel); the transposing load is k_order_wide's, written again here: as a function shared by the two
// kernels it changed the instruction schedule of k_order_wide, whose measured rates stand. The epilogue is this
// file's. DESIGN.md §3.15 has the resource table and the rates.
//
// One workgroup (4 wavefronts) takes a tile of C consecutive coordinates:
//   1. transposing load, as k_order_wide;
//   2. a wavefront a column: sort, blocked store — and then THE SAME WAVEFRONT finds the column's window. Every
//      lane reads med's slots (K - 1) / 2 and K / 2 (one LDS broadcast each); the lanes stride over j, each with
//      the predicate of (col[j], col[j + keep]); a ballot and a population count add the 64 predicates of a step
//      to the wavefront-uniform count (an integer: the order is free). Lane 0 leaves a in the first of the 16
//      spare bytes behind the column's KP slots. The pad slots K .. KP - 1 are never read: j + keep < K;
//   3. sum: lane c of the first wavefront walks column c from s[a] over keep slots in A (the ascending sum is
//      serial by definition), divides once and stores out[i0 + c].
//
// LDS ordering in step 2. The predicate loads of a lane read slots that OTHER lanes of its wavefront stored. No
// workgroup barrier stands between them — the wavefronts walk different numbers of columns in a short last tile,
// and nothing of a column is shared between wavefronts before step 3 — but a wavefront-scope release/acquire
// fence pair around a wave barrier does: the loop is uniform over the wavefront (c depends on the wavefront's
// number only), so all 64 lanes have issued the blocked store when any of them issues a predicate load; a
// wavefront's LDS instructions are executed in the order they were issued; and the fences keep the compiler from
// moving a load above the store or from reusing what it knew of the column before the sort. The __syncthreads()
// before step 3 orders the sorted column and a for the lane of the first wavefront that sums.

// KP / 2 < K <= KP (K <= 128 at KP = 128), 1 <= keep <= K. vec: every update is 16-byte aligned. Dynamic LDS:
// WideGeom::LDS bytes.
template <typename T, int KP>
__global__ void __launch_bounds__(kBlock)
k_window_wide(typename OrderTraits<T>::O* __restrict__ out, const void* const* __restrict__ tab, const int K,
              const int keep, const int64_t P, const int vec) {
    using TR = OrderTraits<T>;
    using G = WideGeom<T, KP>;
    using KEY = typename TR::KEY;
    using A = typename TR::A;
    using O = typename TR::O;
    constexpr int C = G::C, R = G::R, STRIDE = G::STRIDE;
    extern __shared__ uint64_t wide_lds[];
    KEY* const lds = reinterpret_cast<KEY*>(wide_lds);

    const int tid = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * C;
    const int ncols = P - i0 >= C ? C : (int)(P - i0);

    // 1. transposing load
    if (vec && ncols == C) {
        constexpr int EPC = 16 / (int)sizeof(T);         // elements a 16-byte chunk
        constexpr int CH = C / EPC;                      // chunks a segment
        const int total = K * CH;
        for (int base = tid; base < total; base += kBlock * kWideLoads) {
            T y[kWideLoads][EPC];
#pragma unroll
            for (int u = 0; u < kWideLoads; ++u) {
                const int idx = base + u * kBlock;
                if (idx < total)
                    strip_load<T, EPC, true>(static_cast<const T*>(tab[idx / CH]) + i0 + (idx % CH) * EPC, y[u]);
            }
#pragma unroll
            for (int u = 0; u < kWideLoads; ++u) {
                const int idx = base + u * kBlock;
                if (idx < total) {
                    KEY* col = lds + (idx % CH) * EPC * STRIDE + idx / CH;
#pragma unroll
                    for (int e = 0; e < EPC; ++e) col[e * STRIDE] = TR::key(y[u][e]);
                }
            }
        }
    } else {
        const int total = K * C;
        for (int base = tid; base < total; base += kBlock * kWideLoads) {
            T y[kWideLoads];
#pragma unroll
            for (int u = 0; u < kWideLoads; ++u) {
                const int idx = base + u * kBlock;
                if (idx < total && idx % C < ncols) y[u] = static_cast<const T*>(tab[idx / C])[i0 + idx % C];
            }
#pragma unroll
            for (int u = 0; u < kWideLoads; ++u) {
                const int idx = base + u * kBlock;
                if (idx < total && idx % C < ncols) lds[(idx % C) * STRIDE + idx / C] = TR::key(y[u]);
            }
        }
    }
    const int npad = KP - K;                             // padding: never before a real value
    for (int idx = tid; idx < npad * C; idx += kBlock) lds[(idx / npad) * STRIDE + K + idx % npad] = (KEY)~(KEY)0;
    __syncthreads();

    // 2. one wavefront a column: the sort, then the window start
    const int lane = tid & 63;
    const int m0 = (K - 1) / 2, m1 = K / 2;              // the median's slots
    const int nj = K - keep;                             // window starts the walk may move past
    for (int c = tid >> 6; c < ncols; c += kBlock / 64) {
        KEY* const col = lds + c * STRIDE;
        KEY key[R];
#pragma unroll
        for (int r = 0; r < R; ++r) key[r] = col[r * 64 + lane];
        wide_sort<KEY, R>(key, lane);
        wide_store_block<KEY, R>(col + lane * R, key);   // (the wavefront's loads of this column are all done)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const A med = m0 == m1 ? TR::val(col[m0]) : (TR::val(col[m0]) + TR::val(col[m1])) / (A)2;
        int a = 0;
        for (int j0 = 0; j0 < nj; j0 += 64) {            // uniform over the wavefront: the ballot sees all 64 lanes
            const int j = j0 + lane;
            const bool moves = j < nj && window_moves<A>(TR::val(col[j]), TR::val(col[j + keep]), med) != 0;
            a += __popcll(__ballot(moves));
        }
        if (lane == 0) col[KP] = (KEY)a;                 // the first spare slot of the column
    }
    __syncthreads();

    // 3. the ascending sum of the window's slots, one lane a coordinate
    if (tid < ncols) {
        const KEY* const col = lds + tid * STRIDE;
        const KEY* const s = col + (int)col[KP];         // a <= K - keep: s[keep - 1] is a real slot
        A acc = TR::val(s[0]);
#pragma unroll 8
        for (int j = 1; j < keep; ++j) acc = acc + TR::val(s[j]);
        out[i0 + tid] = order_out<A, O>(acc / (A)keep);
    }
}

template <typename T>
int launch_window_wide(void* out, const void* const* ups, int K, int keep, int64_t P, void* work, hipStream_t st) {
    return launch_wide_kernel<T>("fa_median_window_mean_wide", "k_window_wide", out, ups, K, keep, P, work, st,
                                 [](auto kp) { return k_window_wide<T, decltype(kp)::value>; });
}
