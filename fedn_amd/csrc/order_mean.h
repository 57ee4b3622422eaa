// order_mean.h — coordinate-wise trimmed mean / median over K client buffers (fa_trimmed_mean).
//
// Included by fedagg.hip inside its anonymous namespace (it uses fold_rules.h's element types and strip
// loads / stores, host_common.h's grid_for, fill_ptrs and for_kp, and that file's error plumbing). Its launch
// path, launch_sort_kernel, also serves median_window.h's kernel. With FA_ORDER_NET_ONLY defined only the
// comparator network is compiled, by any C++17 compiler: tests/test_robust_host.py checks it with the 0-1
// principle.
//
// Per element: the K values become unsigned keys whose integer order is the rule's total order
// (-0 before +0, every NaN after +inf, all NaNs equal), the keys are sorted by a fully unrolled
// comparator network on registers (nothing is shared between lanes: no LDS, no cross-lane op), and the
// kept slots s[t] .. s[K-t-1] are summed in ascending order starting FROM s[t] (each add rounded once,
// no FMA: the file is built with -ffp-contract=off), divided by K - 2t with an IEEE division and
// rounded once to the output type. DESIGN.md §3.7 has the definition and the register table.

#ifndef FA_ORDER_HD
#ifdef __HIPCC__
#define FA_ORDER_HD __host__ __device__ __forceinline__
#else
#define FA_ORDER_HD inline
#endif
#endif

// compare-exchange: lo to slot a, hi to slot b (a < b). 32-bit keys: v_min_u32 / v_max_u32; 64-bit
// keys: one compare and four selects.
template <typename KEY>
FA_ORDER_HD void order_ce(KEY& a, KEY& b) {
    const KEY lo = b < a ? b : a;
    const KEY hi = b < a ? a : b;
    a = lo;
    b = hi;
}

// Batcher's odd-even merge sort of N = 2^LOG keys, ascending. Every index is a compile-time constant
// once the loops are unrolled, so k[] stays in registers. N = 2, 4, 8, 16, 32, 64: 1, 5, 19, 63,
// 191, 543 comparators.
template <typename KEY, int N>
FA_ORDER_HD void order_sort(KEY (&k)[N]) {
    static_assert(N >= 2 && (N & (N - 1)) == 0, "N must be a power of two");
#pragma unroll
    for (int p = 1; p < N; p *= 2) {
#pragma unroll
        for (int d = p; d >= 1; d /= 2) {
#pragma unroll
            for (int j = d % p; j + d < N; j += 2 * d) {
#pragma unroll
                for (int i = 0; i < d; ++i) {
                    const int a = i + j, b = i + j + d;
                    if (b < N && a / (2 * p) == b / (2 * p)) order_ce(k[a], k[b]);
                }
            }
        }
    }
}

#ifndef FA_ORDER_NET_ONLY

// ----------------------------------------------------------------------------
// keys: value -> unsigned key (order-preserving), key -> accumulator value
// ----------------------------------------------------------------------------
constexpr uint32_t kKeyPad32 = 0xFFFFFFFFu;              // padding: never before a real value
constexpr uint64_t kKeyPad64 = 0xFFFFFFFFFFFFFFFFull;

__device__ __forceinline__ uint32_t f32_key(float x) {
    const uint32_t u = __float_as_uint(x);
    const uint32_t k = u ^ ((uint32_t)((int32_t)u >> 31) | 0x80000000u);   // negative: ~u; else u | sign
    return x != x ? kKeyPad32 - 1 : k;                                      // every NaN: one key after +inf
}
__device__ __forceinline__ float f32_unkey(uint32_t k) {
    return __uint_as_float(k ^ (~(uint32_t)((int32_t)k >> 31) | 0x80000000u));   // max - 1 -> 0x7FFFFFFE, a NaN
}
__device__ __forceinline__ uint64_t f64_key(double x) {
    const uint64_t u = (uint64_t)__double_as_longlong(x);
    const uint64_t k = u ^ ((uint64_t)((int64_t)u >> 63) | 0x8000000000000000ull);
    return x != x ? kKeyPad64 - 1 : k;
}
__device__ __forceinline__ double f64_unkey(uint64_t k) {
    return __longlong_as_double((long long)(k ^ (~(uint64_t)((int64_t)k >> 63) | 0x8000000000000000ull)));
}

// T: update dtype; KEY: 32- or 64-bit network; A: accumulator; O: output storage type
template <typename T> struct OrderTraits;
template <> struct OrderTraits<float> {
    using KEY = uint32_t; using A = float; using O = float;
    static __device__ __forceinline__ KEY key(float v) { return f32_key(v); }
    static __device__ __forceinline__ A val(KEY k) { return f32_unkey(k); }
};
template <> struct OrderTraits<f16> {        // widened exactly to f32; the mean rounded once to half
    using KEY = uint32_t; using A = float; using O = f16;
    static __device__ __forceinline__ KEY key(f16 v) { return f32_key(f16_to_f32(v.bits)); }
    static __device__ __forceinline__ A val(KEY k) { return f32_unkey(k); }
};
template <> struct OrderTraits<bf16> {       // the fp32 rule on exact upcasts
    using KEY = uint32_t; using A = float; using O = float;
    static __device__ __forceinline__ KEY key(bf16 v) { return f32_key(bf16_to_f32(v.bits)); }
    static __device__ __forceinline__ A val(KEY k) { return f32_unkey(k); }
};
template <> struct OrderTraits<double> {
    using KEY = uint64_t; using A = double; using O = double;
    static __device__ __forceinline__ KEY key(double v) { return f64_key(v); }
    static __device__ __forceinline__ A val(KEY k) { return f64_unkey(k); }
};
template <> struct OrderTraits<int32_t> {    // integers: float64 mean (numpy), each kept value converted once
    using KEY = uint32_t; using A = double; using O = double;
    static __device__ __forceinline__ KEY key(int32_t v) { return (uint32_t)v ^ 0x80000000u; }
    static __device__ __forceinline__ A val(KEY k) { return (double)(int32_t)(k ^ 0x80000000u); }
};
template <> struct OrderTraits<int64_t> {
    using KEY = uint64_t; using A = double; using O = double;
    static __device__ __forceinline__ KEY key(int64_t v) { return (uint64_t)v ^ 0x8000000000000000ull; }
    static __device__ __forceinline__ A val(KEY k) { return (double)(int64_t)(k ^ 0x8000000000000000ull); }
};

template <typename A, typename O> __device__ __forceinline__ O order_out(A r) { return static_cast<O>(r); }
template <> __device__ __forceinline__ f16 order_out<float, f16>(float r) { return f16{f32_to_f16(r)}; }

struct OrderTable {
    const void* ptr[kMaxK];
};

// One lane: E consecutive elements, KP key slots each (KP / 2 < K <= KP, or K = 1 with KP = 2: the
// first KP / 2 clients always exist). All of a lane's K loads are issued before the first compare.
template <typename T, int KP, int E>
__global__ void __launch_bounds__(kBlock)
k_order_mean(typename OrderTraits<T>::O* __restrict__ out, const OrderTable tab, const int K, const int trim,
             const int64_t P) {
    using TR = OrderTraits<T>;
    using KEY = typename TR::KEY;
    using A = typename TR::A;
    using O = typename TR::O;
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

    const int hi = K - trim;                     // kept slots: trim <= j < hi
    const A cnt = (A)(K - 2 * trim);
    O r[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        KEY key[KP];
#pragma unroll
        for (int k = 0; k < KP; ++k) key[k] = (k < KP / 2 || k < K) ? TR::key(y[k][e]) : (KEY)~(KEY)0;
        order_sort<KEY, KP>(key);
        A acc = TR::val(key[0]);                 // trim == 0; a later slot replaces it otherwise
#pragma unroll
        for (int j = 1; j < KP; ++j) {
            const A v = TR::val(key[j]);
            acc = j == trim ? v : ((j > trim && j < hi) ? acc + v : acc);
        }
        r[e] = order_out<A, O>(acc / cnt);
    }
    if (full) strip_store<O, E, 0>(out + i0, r);
    else
        for (int e = 0; e < rem; ++e) out[i0 + e] = r[e];
}

// elements per lane on the vector path: registers decide (DESIGN.md §3.7 has the compiler's table)
template <typename KEY, int KP> constexpr int order_vec_elems() {
    if (sizeof(KEY) == 4) return KP <= 16 ? 4 : (KP == 32 ? 2 : 1);
    return KP <= 16 ? 2 : 1;
}

// The launch path of the two sort kernels, k_order_mean and median_window.h's k_median_window, reported in the
// entry point `who`'s name: the bound on P, the client table, the padded client count KP and the elements a
// lane, E (order_vec_elems when out and every update are 16-byte aligned, else 1).
// launch(kp, e, grid, out, tab) launches the <T, KP, E> instantiation; kp and e are std::integral_constant tags.
template <typename T, typename LAUNCH>
int launch_sort_kernel(const char* who, void* out, const void* const* ups, int K, int64_t P, LAUNCH&& launch) {
    // grid = ceil(P / E / 256) workgroups must fit the 32-bit grid dimension
    if (P > (int64_t)0x7FFFFFFF * kBlock) return fail(FA_EINVAL, "%s: P=%lld is too large", who, (long long)P);
    OrderTable tab;
    const bool vec = fill_ptrs(tab.ptr, ups, K) && aligned16(out);
    auto* o = static_cast<typename OrderTraits<T>::O*>(out);
    for_kp<2>(K, [&](auto kp) {
        constexpr int EV = order_vec_elems<typename OrderTraits<T>::KEY, decltype(kp)::value>();
        if (vec && EV > 1) launch(kp, std::integral_constant<int, EV>{}, dim3((unsigned)grid_for(P, EV)), o, tab);
        else launch(kp, std::integral_constant<int, 1>{}, dim3((unsigned)grid_for(P, 1)), o, tab);
    });
    char what[64];
    std::snprintf(what, sizeof(what), "%s: kernel launch", who);
    return check_launch(what);
}

template <typename T>
int launch_order_mean(void* out, const void* const* ups, int K, int trim, int64_t P, hipStream_t st) {
    auto launch = [&](auto kp, auto e, dim3 grid, auto* o, const OrderTable& tab) {
        g_kernel = "k_order_mean";
        hipLaunchKernelGGL((k_order_mean<T, decltype(kp)::value, decltype(e)::value>), grid, dim3(kBlock), 0, st, o, tab, K,
                           trim, P);
    };
    return launch_sort_kernel<T>("fa_trimmed_mean", out, ups, K, P, launch);
}

#endif  // FA_ORDER_NET_ONLY
