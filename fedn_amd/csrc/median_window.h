// median_window.h — coordinate-wise mean of the `keep` values closest to the median over K client buffers
// (fa_median_window_mean), Bulyan's second stage.
//
// Included by fedagg.hip inside its anonymous namespace, after order_mean.h: the keys, the comparator
// network, OrderTraits, OrderTable, order_vec_elems, the launch path (launch_sort_kernel) and the strip loads /
// stores are that header's. With
// FA_ORDER_NET_ONLY defined only the window-start functions are compiled, by any C++17 compiler (after
// order_mean.h under the same guard, for FA_ORDER_HD): tests/test_bulyan_host.py checks them against the
// oracle on the CPU.
//
// Per element: the K values are sorted as in order_mean.h; med is the median of the sorted values kept in
// the accumulator type A (one add and one division for an even K); the window start a is the number of
// j in [0, K - keep) with (A(s[j + keep]) - med) < (med - A(s[j])) — the greedy walk "move the window up
// while its upper neighbour is closer to the median than its lowest value" in counting form: the predicate
// is monotone in j; the kept slots s[a] .. s[a + keep - 1] are summed in ascending order starting FROM
// s[a], divided by keep with an IEEE division and rounded once to the output type. DESIGN.md §3.11 has
// the definition and the register table.
//
// s[j + keep] with a runtime keep would index the key registers dynamically (scratch). Instead keep, which
// is uniform over the launch, is dispatched on: window_start() branches to the one block in which every
// slot pair (j, j + KEEP) is a compile-time constant. That costs code size (KP (KP - 1) / 2 pair bodies
// per instantiation), not registers: one block runs per launch.

// 1 when the window moves past slot j: its upper neighbour `hi` = A(s[j + keep]) is closer to the median
// than its lowest value `lo` = A(s[j]). Each difference is rounded once in A; strict, so a tie keeps the
// lower window; false when anything is a NaN.
template <typename A>
FA_ORDER_HD int window_moves(A lo, A hi, A med) {
    return (hi - med) < (med - lo) ? 1 : 0;
}

// The window start of the K sorted slots s[0 .. K - 1] (K <= KP) at the compile-time window length KEEP:
// every slot index is a constant once the loop is unrolled. val(slot) gives the slot's value in A.
template <typename A, int KP, int KEEP, typename SLOT, typename VAL>
FA_ORDER_HD int window_start_at(const SLOT (&s)[KP], int K, A med, VAL val) {
    int a = 0;
#pragma unroll
    for (int j = 0; j + KEEP < KP; ++j)
        if (j + KEEP < K) a += window_moves<A>(val(s[j]), val(s[j + KEEP]), med);
    return a;
}

// The window start at the runtime window length keep (1 <= keep <= K): a chain of uniform branches to
// window_start_at<KEEP>. keep == KP (then K == KP) leaves nothing to move past: 0.
template <typename A, int KP, int KEEP = 1, typename SLOT, typename VAL>
FA_ORDER_HD int window_start(const SLOT (&s)[KP], int K, int keep, A med, VAL val) {
    if constexpr (KEEP >= KP) {
        return 0;
    } else {
        if (keep == KEEP) return window_start_at<A, KP, KEEP>(s, K, med, val);
        return window_start<A, KP, KEEP + 1>(s, K, keep, med, val);
    }
}

#ifndef FA_ORDER_NET_ONLY

template <typename T> struct OrderVal {          // key slot -> accumulator value
    __device__ __forceinline__ typename OrderTraits<T>::A operator()(typename OrderTraits<T>::KEY k) const {
        return OrderTraits<T>::val(k);
    }
};

// Element EI of a lane's E: sort, median, window start, windowed sum. The elements are walked by template
// recursion (window_elements), not by a loop: whatever the body's size, every index of y[][] and r[] is a
// compile-time constant.
template <typename T, int KP, int E, int EI>
__device__ __forceinline__ void window_element(const T (&y)[KP][E], typename OrderTraits<T>::O (&r)[E], const int K,
                                               const int keep) {
    using TR = OrderTraits<T>;
    using KEY = typename TR::KEY;
    using A = typename TR::A;
    using O = typename TR::O;
    const int m0 = (K - 1) / 2, m1 = K / 2;      // the median's slots, both in [KP / 4, KP / 2]
    KEY key[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) key[k] = (k < KP / 2 || k < K) ? TR::key(y[k][EI]) : (KEY) ~(KEY)0;
    order_sort<KEY, KP>(key);
    KEY k0 = key[KP / 4], k1 = key[KP / 4];
#pragma unroll
    for (int j = KP / 4 + 1; j <= KP / 2; ++j) {
        k0 = j == m0 ? key[j] : k0;
        k1 = j == m1 ? key[j] : k1;
    }
    const A med = m0 == m1 ? TR::val(k0) : (TR::val(k0) + TR::val(k1)) / (A)2;
    const int a = window_start<A, KP>(key, K, keep, med, OrderVal<T>{});
    const int hi = a + keep;                     // kept slots: a <= j < hi, per lane
    A acc = TR::val(key[0]);                     // a == 0; a later slot replaces it otherwise
#pragma unroll
    for (int j = 1; j < KP; ++j) {
        const A v = TR::val(key[j]);
        acc = j == a ? v : ((j > a && j < hi) ? acc + v : acc);
    }
    r[EI] = order_out<A, O>(acc / (A)keep);
}

template <typename T, int KP, int E, int EI = 0>
__device__ __forceinline__ void window_elements(const T (&y)[KP][E], typename OrderTraits<T>::O (&r)[E], const int K,
                                                const int keep) {
    if constexpr (EI < E) {
        window_element<T, KP, E, EI>(y, r, K, keep);
        window_elements<T, KP, E, EI + 1>(y, r, K, keep);
    }
}

// One lane: E consecutive elements, KP key slots each, as k_order_mean (KP / 2 < K <= KP, or K = 1 with
// KP = 2). All of a lane's K loads are issued before the first compare.
template <typename T, int KP, int E>
__global__ void __launch_bounds__(kBlock)
k_median_window(typename OrderTraits<T>::O* __restrict__ out, const OrderTable tab, const int K, const int keep,
                const int64_t P) {
    using O = typename OrderTraits<T>::O;
    const int64_t i0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * E;
    if (i0 >= P) return;
    const bool full = P - i0 >= E;
    const int rem = full ? E : (int)(P - i0);

    T y[KP][E];
    if (full) {
#pragma unroll
        for (int k = 0; k < KP; ++k)
            if (k < KP / 2 || k < K) strip_load<T, E, false>(static_cast<const T*>(tab.ptr[k]) + i0, y[k]);
    } else {
#pragma unroll
        for (int k = 0; k < KP; ++k)
            if (k < KP / 2 || k < K) {
                const T* yp = static_cast<const T*>(tab.ptr[k]) + i0;
#pragma unroll
                for (int e = 0; e < E; ++e) y[k][e] = e < rem ? yp[e] : T{};
            }
    }

    O r[E];
    window_elements<T, KP, E>(y, r, K, keep);
    if (full) strip_store<O, E, 0>(out + i0, r);
    else
        for (int e = 0; e < rem; ++e) out[i0 + e] = r[e];
}

template <typename T>
int launch_median_window(void* out, const void* const* ups, int K, int keep, int64_t P, hipStream_t st) {
    auto launch = [&](auto kp, auto e, dim3 grid, auto* o, const OrderTable& tab) {      // E is k_order_mean's (§3.11)
        g_kernel = "k_median_window";
        hipLaunchKernelGGL((k_median_window<T, decltype(kp)::value, decltype(e)::value>), grid, dim3(kBlock), 0, st, o, tab,
                           K, keep, P);
    };
    return launch_sort_kernel<T>("fa_median_window_mean", out, ups, K, P, launch);
}

#endif  // FA_ORDER_NET_ONLY
