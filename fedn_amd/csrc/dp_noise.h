// dp_noise.h — Gaussian noise for central DP-FedAvg: one N(0,1) deviate per element from a counter-based
// generator, added to a buffer (fa_gaussian_noise, kernel k_gaussian_noise).
//
// Included by fedagg.hip inside its anonymous namespace, after host_common.h (f16 and its conversions are
// fold_rules.h's, aligned16 and the error plumbing that file's and fedagg.hip's). With FA_DP_NOISE_GEN_ONLY
// defined only the generator and the two uniform conversions are compiled, by any C++17 compiler:
// tests/test_dpnoise_host.py checks them against the numpy restatement tests/dpnoise_ref.py.
//
// The deviate of element i is a pure function of (seed, stream_id, round_id, i) — DESIGN.md §3.12:
//     (x0, x1, x2, x3) = Philox4x32-10(ctr = (lo32(i), hi32(i), stream_id, round_id), key = (lo32(seed), hi32(seed)))
//     u1 = ((x0 >> 5) * 2^26 + (x1 >> 6) + 1) * 2^-53      in (0, 1]
//     u2 = ((x2 >> 5) * 2^26 + (x3 >> 6)) * 2^-53          in [0, 1)
//     z  = sqrt(-2 * log(u1)) * cos(TWO_PI * u2)           in float64, every operation rounded once
//     out[j] = O(double(x[j]) + sigma * z(offset + j))     product and sum rounded once in float64, one
//                                                          conversion to O (float16 straight from float64)
// One Philox block per element and no sine branch: an element's value depends on nothing but its index,
// so the bits are the same for every grid, slice bound, offset and pointer alignment. The file is built
// with -ffp-contract=off: neither sigma * z + x nor the Box-Muller product is fused.

#ifndef FA_DP_HD
#ifdef __HIPCC__
#define FA_DP_HD __host__ __device__ __forceinline__
#else
#define FA_DP_HD inline
#endif
#endif

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;     // multipliers on ctr[0], ctr[2]
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;     // key increments (Weyl sequence)

// Philox4x32-10 (Salmon, Moraes, Dror and Shaw, SC'11): c[] in, c[] out
FA_DP_HD void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)kPhiloxM0 * c[0], p1 = (uint64_t)kPhiloxM1 * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[0] = n0;
        c[1] = (uint32_t)p1;
        c[2] = n2;
        c[3] = (uint32_t)p0;
        k0 += kPhiloxW0;
        k1 += kPhiloxW1;
    }
}

// the block of element i
FA_DP_HD void dp_noise_bits(uint32_t (&x)[4], uint64_t seed, uint32_t stream_id, uint32_t round_id, uint64_t i) {
    x[0] = (uint32_t)i;
    x[1] = (uint32_t)(i >> 32);
    x[2] = stream_id;
    x[3] = round_id;
    philox4x32_10(x, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// 53 bits of two words as a float64 in (0, 1] / [0, 1): the integer is below 2^53 + 1, so it and the
// product with 2^-53 are exact
FA_DP_HD double dp_uniform_open0(uint32_t a, uint32_t b) {     // (0, 1]: log never sees 0
    return (double)((((uint64_t)(a >> 5) << 26) | (uint64_t)(b >> 6)) + 1u) * 0x1p-53;
}
FA_DP_HD double dp_uniform_open1(uint32_t a, uint32_t b) {     // [0, 1)
    return (double)(((uint64_t)(a >> 5) << 26) | (uint64_t)(b >> 6)) * 0x1p-53;
}

#ifndef FA_DP_NOISE_GEN_ONLY

constexpr double kDpTwoPi = 6.283185307179586;                 // the float64 nearest 2 pi (0x401921FB54442D18)
constexpr int kDpMaxBlocks = 2048;                             // the grid's bound: 8 workgroups a CU

__device__ __forceinline__ double dp_deviate(uint64_t seed, uint32_t stream_id, uint32_t round_id, uint64_t i) {
    uint32_t x[4];
    dp_noise_bits(x, seed, stream_id, round_id, i);
    const double u1 = dp_uniform_open0(x[0], x[1]), u2 = dp_uniform_open1(x[2], x[3]);
    const double l = ::log(u1);
    const double m = -2.0 * l;
    const double r = __builtin_sqrt(m);
    const double a = kDpTwoPi * u2;
    const double c = ::cos(a);
    return r * c;
}

// float64 -> float16 bits, ONE round-to-nearest-even (numpy's astype: never through float32, whose
// rounding first moves about one value in 8192 across a float16 midpoint). A NaN keeps its sign and the
// top bits of its payload, as numpy's conversion does.
__device__ __forceinline__ uint16_t dp_f64_to_f16(double d) {
    const uint64_t b = (uint64_t)__double_as_longlong(d);
    const uint16_t sign = (uint16_t)((b >> 48) & 0x8000u);
    const uint64_t a = b & 0x7FFFFFFFFFFFFFFFull;
    const int e = (int)(a >> 52);                              // biased by 1023
    const uint64_t frac = a & 0x000FFFFFFFFFFFFFull;
    if (e == 0x7FF) {                                          // inf, NaN
        if (frac == 0) return sign | 0x7C00u;
        const uint16_t h = (uint16_t)(0x7C00u + (frac >> 42));
        return sign | (h == 0x7C00u ? 0x7C01u : h);
    }
    if (e >= 1039) return sign | 0x7C00u;                      // |d| >= 2^16
    if (e < 998) return sign;                                  // |d| < 2^-25: below half the smallest subnormal
    uint64_t h, rem, half;
    if (e >= 1009) {                                           // a normal float16 (before rounding)
        h = ((uint64_t)(e - 1008) << 10) | (frac >> 42);
        rem = frac & ((1ull << 42) - 1);
        half = 1ull << 41;
    } else {                                                   // a subnormal one: units of 2^-24
        const int shift = 1009 - e + 42;                       // 43 .. 53
        const uint64_t sig = frac | (1ull << 52);
        h = sig >> shift;
        rem = sig & ((1ull << shift) - 1);
        half = 1ull << (shift - 1);
    }
    if (rem > half || (rem == half && (h & 1))) ++h;           // a carry runs into the exponent: up to inf
    return sign | (uint16_t)h;
}

template <typename T> struct DpIo;                             // element type <-> float64
template <> struct DpIo<float> {
    static __device__ __forceinline__ double in(float v) { return (double)v; }
    static __device__ __forceinline__ float out(double v) { return (float)v; }
};
template <> struct DpIo<double> {
    static __device__ __forceinline__ double in(double v) { return v; }
    static __device__ __forceinline__ double out(double v) { return v; }
};
template <> struct DpIo<f16> {
    static __device__ __forceinline__ double in(f16 v) { return (double)f16_to_f32(v.bits); }
    static __device__ __forceinline__ f16 out(double v) { return f16{dp_f64_to_f16(v)}; }
};

template <typename T>
__device__ __forceinline__ T dp_apply(T xv, bool have_x, double sigma, double z) {
    const double base = have_x ? DpIo<T>::in(xv) : 0.0;
    const double n = sigma * z;
    const double s = base + n;
    return DpIo<T>::out(s);
}

// One lane, one 16-byte item of `out` at a time (VEC: out and x are 16-byte aligned) or one element
// (otherwise); a grid-stride loop over the items. The last item of the vector path may be short: its
// elements are loaded and stored one by one. x == out is the normal use: a lane reads its item of x
// before it stores the same bytes of out, and items are disjoint.
template <typename T, bool VEC>
__global__ void __launch_bounds__(kBlock)
k_gaussian_noise(T* out, const T* x, const double sigma, const uint64_t seed, const uint32_t stream_id,
                 const uint32_t round_id, const uint64_t offset, const int64_t P) {
    constexpr int EV = VEC ? 16 / (int)sizeof(T) : 1;
    union Item {
        uint4 v;
        T e[16 / sizeof(T)];
    };
    const int64_t items = (P + EV - 1) / EV;
    for (int64_t it = (int64_t)blockIdx.x * kBlock + threadIdx.x; it < items; it += (int64_t)gridDim.x * kBlock) {
        const int64_t j0 = it * EV;
        if (VEC && j0 + EV <= P) {
            Item u;
            u.v = make_uint4(0u, 0u, 0u, 0u);
            if (x) u.v = *reinterpret_cast<const uint4*>(x + j0);
#pragma unroll
            for (int q = 0; q < EV; ++q)
                u.e[q] = dp_apply<T>(u.e[q], x != nullptr, sigma, dp_deviate(seed, stream_id, round_id, offset + (uint64_t)(j0 + q)));
            *reinterpret_cast<uint4*>(out + j0) = u.v;
        } else {
            const int n = P - j0 < EV ? (int)(P - j0) : EV;    // within [0, P)
            for (int q = 0; q < n; ++q) {
                const T xv = x ? x[j0 + q] : T{};
                out[j0 + q] = dp_apply<T>(xv, x != nullptr, sigma, dp_deviate(seed, stream_id, round_id, offset + (uint64_t)(j0 + q)));
            }
        }
    }
}

template <typename T>
int launch_gaussian_noise(void* out, const void* x, double sigma, uint64_t seed, uint32_t stream_id, uint32_t round_id,
                          int64_t offset, int64_t P, hipStream_t st) {
    const bool vec = aligned16(out) && (!x || aligned16(x));
    const int EV = vec ? 16 / (int)sizeof(T) : 1;
    const int64_t items = (P + EV - 1) / EV;
    const dim3 grid((unsigned)std::min<int64_t>((items + kBlock - 1) / kBlock, kDpMaxBlocks));
    g_kernel = "k_gaussian_noise";
    if (vec)
        hipLaunchKernelGGL((k_gaussian_noise<T, true>), grid, dim3(kBlock), 0, st, static_cast<T*>(out),
                           static_cast<const T*>(x), sigma, seed, stream_id, round_id, (uint64_t)offset, P);
    else
        hipLaunchKernelGGL((k_gaussian_noise<T, false>), grid, dim3(kBlock), 0, st, static_cast<T*>(out),
                           static_cast<const T*>(x), sigma, seed, stream_id, round_id, (uint64_t)offset, P);
    return check_launch("fa_gaussian_noise: kernel launch");
}

#endif  // FA_DP_NOISE_GEN_ONLY
