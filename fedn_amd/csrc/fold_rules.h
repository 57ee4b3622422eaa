// fold_rules.h — what every fold kernel is built from: the element types, the arithmetic numpy performs
// for each dtype (CF32 / CF64 / CF16, the server-function rules CWSUM / CRUN), 16-byte strip loads and
// stores, the client table of a launch, and the clock test of the chip-wide store windows.
// Included by fedagg.hip inside its anonymous namespace, first of the family headers; it uses only
// that file's constants (kMaxK). DESIGN.md §3.2 / §3.2b have the division arguments, §3.3 the windows.

// ----------------------------------------------------------------------------
// element types and exact conversions
// ----------------------------------------------------------------------------
struct bf16 { uint16_t bits; };
struct f16 { uint16_t bits; };

__device__ __forceinline__ float bf16_to_f32(uint16_t b) { return __uint_as_float(static_cast<uint32_t>(b) << 16); }
__device__ __forceinline__ float f16_to_f32(uint16_t b) {
    __half h;
    __builtin_memcpy(&h, &b, 2);
    return __half2float(h);
}
__device__ __forceinline__ uint16_t f32_to_f16(float f) {
    __half h = __float2half_rn(f);
    uint16_t b;
    __builtin_memcpy(&b, &h, 2);
    return b;
}

// ----------------------------------------------------------------------------
// compute policies: the arithmetic numpy performs for each dtype
// ----------------------------------------------------------------------------
struct CF32 {            // float32 ufunc loops
    using V = float;     // register type
    using S = float;     // scalar (n, N) type
    using T = float;     // storage type (FedOpt's pseudo-gradient workspace)
    __device__ static __forceinline__ V fold(V x, V y, S n, S N, double r) {
        V t[1] = {x}, yy[1] = {y};
        fold_strip<1>(t, yy, n, N, r);
        return t[0];
    }
    // One client step over E elements: x <- x + (n*(y-x))/N.
    // t/N is correctly rounded. N is the same for every element of a client step, so
    // the host supplies r = RN64(1/N) and the quotient is RN32(RN64(t * r)): its
    // relative error is < 2^-52, while t/N (t, N binary32, N's odd part < 2^24) is
    // never closer than 2^-49 (relative) to a binary32 rounding midpoint in the normal
    // range, so the final rounding lands where IEEE division does (DESIGN.md has the
    // argument; tests/test_gpu_divide.py checks every binary32 t exhaustively).
    // r == 0 (host: N == 0, |N| >= 2^28, or fa_tune) selects IEEE division; lanes with
    // 0 < |t| < 2^-98 (a subnormal quotient is possible) redo it with IEEE division.
    template <int E>
    __device__ static __forceinline__ void fold_strip(V (&x)[E], const V (&y)[E], S n, S N, double r) {
        V t[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            t[e] = y[e] - x[e];
            t[e] = n * t[e];
        }
        if (r != 0.0) {
            V q[E];
            bool small = false;   // |t| < 2^-98, zeros included: one compare per element
#pragma unroll
            for (int e = 0; e < E; ++e) {
                q[e] = (float)((double)t[e] * r);
                small |= __builtin_fabsf(t[e]) < 0x1p-98f;
            }
            if (__builtin_expect(small, 0)) {
                // zero lanes already hold the right signed zero (t*r); only nonzero tiny t divide
#pragma unroll
                for (int e = 0; e < E; ++e)
                    if (__builtin_fabsf(t[e]) < 0x1p-98f && t[e] != 0.0f) q[e] = t[e] / N;
            }
#pragma unroll
            for (int e = 0; e < E; ++e) x[e] = x[e] + q[e];
        } else {
#pragma unroll
            for (int e = 0; e < E; ++e) x[e] = x[e] + t[e] / N;
        }
    }
};
struct CF64 {            // float64 ufunc loops
    using V = double;
    using S = double;
    using T = double;
    // RN64(t/N) without a division when the host supplies r = RN64(1/N) (r == 0: IEEE
    // division). q0 = RN(t*r) is within 1.5 ulp of z = t/N; one Markstein step
    // q1 = RN(q0 + RN(t - q0*N)*r) makes it faithful (the error left is ~2^-52 of q0's);
    // for a faithful q the remainder t - q*N is exact (FMA), and q2 = RN(q1 + (t - q1*N)*r)
    // lands within |z - q1|*|N*r - 1| < 2^-53.x ulp of z, which is closer than z can be to a
    // rounding midpoint without being one (|z - mid| >= ulp/(2*N') with N' < 2^53 N's odd
    // significand; z is never exactly a midpoint), so q2 = RN(z). DESIGN.md §3.2b has the
    // argument. The bounds |t| in [2^-600, 2^600] (host: |N| in [2^-60, 2^60]) keep every
    // intermediate and remainder normal; other lanes (0, tiny, huge, inf, NaN) divide.
    __device__ static __forceinline__ V div(V t, S N, double r) {
        if (r != 0.0) {
            const double a = __builtin_fabs(t);
            if (a >= 0x1p-600 && a <= 0x1p600) {
                double q = t * r;
                double e = __builtin_fma(-q, N, t);
                q = __builtin_fma(e, r, q);
                e = __builtin_fma(-q, N, t);
                return __builtin_fma(e, r, q);
            }
            if (a == 0.0) return t * r;   // signed zero: sign(t) * sign(N), as t / N
        }
        return t / N;
    }
    __device__ static __forceinline__ V fold(V x, V y, S n, S N, double r) {
        V t = y - x;
        t = n * t;
        t = div(t, N, r);
        return x + t;
    }
};
struct CF16 {            // numpy half loops: op in float, round to half after every op
    using V = float;     // holds a value exactly representable in f16
    using S = float;     // n, N pre-rounded to f16 on the host
    using T = f16;
    __device__ static __forceinline__ V rh(float a) { return f16_to_f32(f32_to_f16(a)); }
    __device__ static __forceinline__ V fold(V x, V y, S n, S N, double) {
        V t = rh(y - x);
        // n and t are halves, so the half product rounds the exact product once, as rh(n * t) would; written as
        // a half multiply because the float one is compiled to a mixed-precision fma with a +0 addend, which
        // turns a product of -0 (a negative or zero n) into +0
        t = (float)((_Float16)n * (_Float16)t);
        t = rh(t / N);
        return rh(x + t);
    }
};

// Server-function aggregation rules, the two the reference ships as
// examples of user `aggregate` / `incremental_aggregate` code (hooks.py:109-143):
//
// CWSUM — examples/server-functions/server_functions.py:58-67
//     weighted_sum[i] += client_parameters[i] * num_examples
//   the product is taken in the update dtype Y (python scalar w is weak: cast to Y), the sum
//   in promote(acc, Y), the result stored back in the accumulator dtype X (in-place +=).
template <typename Y, typename X>
struct CWSUM {
    static constexpr bool kF32 = std::is_same<Y, float>::value && std::is_same<X, float>::value;
    using V = typename std::conditional<kF32, float, double>::type;
    using S = double;
    __device__ static __forceinline__ V fold(V x, V y, S w, S, double) {
        V s;
        if constexpr (std::is_same<Y, float>::value) {
            const float p = (float)y * (float)w;     // y holds an exact f32 value
            s = x + (V)p;
        } else {
            s = x + y * w;                           // f64 product, f64 sum
        }
        if constexpr (std::is_same<X, float>::value && std::is_same<V, double>::value)
            return (double)(float)s;                 // += into an f32 accumulator rounds every step
        else
            return s;
    }
};

// CRUN — examples/server-functions/sf_incremental_aggregation.py:36-37
//     g = (g * (T - n) + m * n) / T       (T = running total including this client)
//   g and m share the dtype T_; every python scalar is cast to it (numpy weak scalars) and each
//   operation rounds in it: RN(RN(RN(g*a) + RN(m*b)) / T). The client table carries
//   b = n in n[], T in N[] and a = T - n in r[].
template <typename T_>
struct CRUN {
    using V = T_;
    using S = double;
    __device__ static __forceinline__ V fold(V x, V y, S b, S T, double a) {
        const V u = x * (V)a;
        const V w = y * (V)b;
        const V s = u + w;
        return s / (V)T;
    }
};

template <class CP> struct is_nostore : std::false_type {};   // true for a measurement rule only (probes.h)

// element-wise client step for policies without a strip-level shortcut
template <class CP, int E>
__device__ __forceinline__ void fold_strip(typename CP::V (&x)[E], const typename CP::V (&y)[E], typename CP::S n,
                                           typename CP::S N, double r) {
    if constexpr (std::is_same<CP, CF32>::value) {
        CP::template fold_strip<E>(x, y, n, N, r);
    } else {
#pragma unroll
        for (int e = 0; e < E; ++e) x[e] = CP::fold(x[e], y[e], n, N, r);
    }
}

// load one element of storage type T, widened to the compute register type V
template <typename T, typename V> __device__ __forceinline__ V widen(T v) { return static_cast<V>(v); }
template <> __device__ __forceinline__ float widen<bf16, float>(bf16 v) { return bf16_to_f32(v.bits); }
template <> __device__ __forceinline__ double widen<bf16, double>(bf16 v) { return (double)bf16_to_f32(v.bits); }
template <> __device__ __forceinline__ float widen<f16, float>(f16 v) { return f16_to_f32(v.bits); }
template <> __device__ __forceinline__ double widen<f16, double>(f16 v) { return (double)f16_to_f32(v.bits); }

template <typename T, typename V> __device__ __forceinline__ T narrow(V v) { return static_cast<T>(v); }
template <> __device__ __forceinline__ f16 narrow<f16, float>(float v) { return f16{f32_to_f16(v)}; }

// ----------------------------------------------------------------------------
// 16-byte strip loads/stores (E elements of T). NT = non-temporal (read-once data)
// ----------------------------------------------------------------------------
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

template <typename T, int E, bool NT>
__device__ __forceinline__ void strip_load(const T* __restrict__ p, T (&r)[E]) {
    constexpr int bytes = E * (int)sizeof(T);
    if constexpr (bytes % 16 == 0) {
        const u32x4* q = reinterpret_cast<const u32x4*>(p);
#pragma unroll
        for (int j = 0; j < bytes / 16; ++j) {
            u32x4 w = NT ? __builtin_nontemporal_load(q + j) : q[j];
            __builtin_memcpy(reinterpret_cast<char*>(r) + 16 * j, &w, 16);
        }
    } else if constexpr (bytes == 8) {          // one dwordx2 (8-B aligned: the caller's contract)
        const u32x2* q = reinterpret_cast<const u32x2*>(p);
        u32x2 w = NT ? __builtin_nontemporal_load(q) : *q;
        __builtin_memcpy(reinterpret_cast<char*>(r), &w, 8);
    } else if constexpr (bytes == 4) {          // one dword (4-B aligned)
        const unsigned int* q = reinterpret_cast<const unsigned int*>(p);
        unsigned int w = NT ? __builtin_nontemporal_load(q) : *q;
        __builtin_memcpy(reinterpret_cast<char*>(r), &w, 4);
    } else {
#pragma unroll
        for (int e = 0; e < E; ++e) r[e] = p[e];
    }
}

// SM (store mode): 0 plain (write-back in L2), 1 non-temporal, 2 write-through (`sc1`,
// MI355X_MICROARCH.md "stores of each flavour": the line leaves L2 as the store issues)
template <typename T, int E, int SM = 0>
__device__ __forceinline__ void strip_store(T* __restrict__ p, const T (&r)[E]) {
    constexpr int bytes = E * (int)sizeof(T);
    if constexpr (bytes == 8 && SM == 0) {
        u32x2 w;
        __builtin_memcpy(&w, reinterpret_cast<const char*>(r), 8);
        *reinterpret_cast<u32x2*>(p) = w;
    } else if constexpr (bytes == 8 && SM == 1) {
        u32x2 w;
        __builtin_memcpy(&w, reinterpret_cast<const char*>(r), 8);
        __builtin_nontemporal_store(w, reinterpret_cast<u32x2*>(p));
    } else if constexpr (bytes % 16 == 0) {
        u32x4* q = reinterpret_cast<u32x4*>(p);
#pragma unroll
        for (int j = 0; j < bytes / 16; ++j) {
            u32x4 w;
            __builtin_memcpy(&w, reinterpret_cast<const char*>(r) + 16 * j, 16);
            if constexpr (SM == 1) __builtin_nontemporal_store(w, q + j);
            else if constexpr (SM == 2) asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(q + j), "v"(w) : "memory");
            else q[j] = w;
        }
    } else {
#pragma unroll
        for (int e = 0; e < E; ++e) p[e] = r[e];
    }
}

// the client table of one launch (kernarg; filled by fill_table, host_common.h)
template <typename S>
struct ClientTable {
    const void* ptr[kMaxK];
    S n[kMaxK];
    S N[kMaxK];
    double r[kMaxK];   // RN64(1/N) for CF32's division shortcut, 0 = use IEEE division
};

// Chip-wide store windows (probe kernels: fa_tune OPT_WIN_* / AVG_WIN_*). Every wave reads the GPU's
// 100 MHz reference clock (s_memrealtime: one counter for all XCDs) and stores only while
// clock mod period < win_w, reads (optionally) only outside that window: the DRAM then sees
// read-only stretches and write bursts instead of writes interleaved everywhere, with no grid
// barrier. A wait gives up after 2^18 polls, far past one period, should the clock stand still.
// (the clock's low 32 bits: one irregular period every 43 s where they wrap; the remainder by a
// power-of-two period is a mask, otherwise a multiply-high by floor(2^32 / period) and one correction)
[[maybe_unused]] __device__ __forceinline__ bool in_write_window(uint32_t period, uint32_t win_w) {
    const uint32_t t = (uint32_t)__builtin_amdgcn_s_memrealtime();
    uint32_t r;
    if ((period & (period - 1)) == 0) {
        r = t & (period - 1);
    } else {
        const uint32_t recip = 0xFFFFFFFFu / period;   // uniform: the compiler keeps it out of the poll loop
        r = t - __umulhi(t, recip) * period;
        if (r >= period) r -= period;
    }
    return r < win_w;
}
// (a wait gives up after 2^18 polls, far past one period, should the clock ever stand still)
[[maybe_unused]] __device__ __forceinline__ void wait_write_window(uint32_t period, uint32_t win_w) {
    for (int n = 0; n < (1 << 18) && !in_write_window(period, win_w); ++n) __builtin_amdgcn_s_sleep(1);
}
[[maybe_unused]] __device__ __forceinline__ void wait_read_window(uint32_t period, uint32_t win_w) {
    for (int n = 0; n < (1 << 18) && in_write_window(period, win_w); ++n) __builtin_amdgcn_s_sleep(1);
}

// A launch's window as the host hands it to the kernel, in 10-ns ticks ({0, 0}: none). The rules that
// size them are opt_store_window (fedopt_launch.h) and avg_store_window (fedavg_launch.h).
struct StoreWindow {
    uint32_t period = 0, w = 0;
};
struct AvgWindow {
    uint32_t period = 0, w = 0;
    int mode = 0;
};
