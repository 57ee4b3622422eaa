// helper_kernels.h — the numpyhelper primitives as elementwise kernels (k_elementwise, k_axpby_half,
// k_ipow, k_ifold, k_nfold), the 1-norm (k_abssum_partial, k_colabssum, k_final_reduce) and the
// broadcasting conversion of the per-tensor path (k_cast): fa_elementwise, fa_norm1, fa_cast.
// Included by fedagg.hip inside its anonymous namespace, after fold_rules.h (the element types and
// `widen`). DESIGN.md §3.6 describes the cast, §3.6b the numpy contract of the primitives.

// ----------------------------------------------------------------------------
// numpyhelper primitives (numpyhelper.py:34-142) as elementwise kernels, numpy rounding:
// every product/quotient in its operand's dtype (python floats are weak scalars), the
// final combination in the promoted dtype.
// ----------------------------------------------------------------------------
template <typename T> __device__ __forceinline__ T as_t(double v) { return (T)v; }

// numpyhelper.add / subtract on float16 arrays: x*a + y*b with the python scalars cast to half and
// every op rounded to half (numpy's half loops compute in float and round: the float product of two
// halves is exact and the float sum is wide enough, 24 >= 2*11+2, so each is the IEEE half op). Written
// in half arithmetic on purpose: for rh(float(x) * ah) the compiler emitted a mixed-precision fma with a
// +0 addend, which turns a product of -0 into +0, and (-0)*a + (-0)*b came out +0.
__device__ __forceinline__ _Float16 f16_value(f16 v) {
    _Float16 h;
    __builtin_memcpy(&h, &v.bits, 2);
    return h;
}
__global__ void __launch_bounds__(kBlock) k_axpby_half(f16* __restrict__ out, const f16* __restrict__ x,
                                                       const f16* __restrict__ y, float ah, float bh, int64_t P) {
    const _Float16 a = (_Float16)ah, b = (_Float16)bh;          // halves already (to_half_value): exact
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < P; i += (int64_t)gridDim.x * kBlock) {
        const _Float16 xa = f16_value(x[i]) * a;
        const _Float16 yb = f16_value(y[i]) * b;
        const _Float16 r = xa + yb;
        __builtin_memcpy(&out[i].bits, &r, 2);
    }
}

template <typename TX, typename TY, typename TO>
__global__ void __launch_bounds__(kBlock)
k_elementwise(int op, TO* __restrict__ out, const TX* __restrict__ x, const TY* __restrict__ y, double a, double b,
              int64_t P) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < P; i += (int64_t)gridDim.x * kBlock) {
        TO r;
        switch (op) {
            case FA_EW_AXPBY: {                                   // x*a + y*b   (numpyhelper.add)
                const TX xa = x[i] * as_t<TX>(a);
                const TY yb = y[i] * as_t<TY>(b);
                r = (TO)xa + (TO)yb;
                break;
            }
            case FA_EW_MUL:                                       // numpyhelper.multiply
                r = y ? (TO)x[i] * (TO)y[i] : (TO)(x[i] * as_t<TX>(a));
                break;
            case FA_EW_DIV:                                       // numpyhelper.divide
                r = y ? (TO)x[i] / (TO)y[i] : (TO)(x[i] / as_t<TX>(a));
                break;
            case FA_EW_SQRT:                                      // numpyhelper.sqrt
                r = (TO)__builtin_sqrt((double)x[i]);
                if constexpr (std::is_same<TX, float>::value) r = (TO)__builtin_sqrtf(x[i]);
                break;
            case FA_EW_SQUARE:                                    // numpyhelper.power(m, 2)
                r = (TO)(x[i] * x[i]);
                break;
            case FA_EW_SIGN: {                                    // numpyhelper.sign
                const TX v = x[i];
                r = v > (TX)0 ? (TO)1 : (v < (TX)0 ? (TO)-1 : (v == (TX)0 ? (TO)0 : (TO)v));
                break;
            }
            case FA_EW_POW:                                       // numpyhelper.power(m, a), float a
                if constexpr (std::is_same<TX, float>::value) r = (TO)(float)::pow((double)x[i], a);
                else r = (TO)::pow((double)x[i], a);
                break;
            default:                                              // FA_EW_FILL: np.ones(shape) * a
                r = (TO)(1.0 * a);
                break;
        }
        out[i] = r;
    }
}

// numpyhelper.power on an integer array with a non-negative python int exponent: numpy's
// exponentiation by squaring in the array's integer type (wrapping products).
template <typename T>
__global__ void __launch_bounds__(kBlock) k_ipow(T* __restrict__ out, const T* __restrict__ x, uint64_t e, int64_t P) {
    // products in uint64 (no signed overflow, no promotion of 8/16-bit operands to int): x**e mod
    // 2**64 taken mod 2**bits(T) is numpy's wrapped result in T
    using U = typename std::make_unsigned<T>::type;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < P; i += (int64_t)gridDim.x * kBlock) {
        uint64_t base = (uint64_t)(U)x[i], r = 1;
        for (uint64_t k = e; k; k >>= 1) {
            if (k & 1) r *= base;
            base *= base;
        }
        out[i] = (T)(U)r;
    }
}

// numpyhelper.increment_average (numpyhelper.py:32) on integer arrays folded with a python-float
// num_examples: numpy subtracts in the integer dtype (wrapping), multiplies the difference by the
// float n in float64, divides by N in float64 and adds x in float64 — each op rounded once.
// Any integer width: the difference is taken in the same-width unsigned type (no signed overflow)
// and wrapped back to T.
template <typename T>
__global__ void __launch_bounds__(kBlock) k_ifold(double* __restrict__ out, const T* __restrict__ x,
                                                  const T* __restrict__ y, double n, double N, int64_t P) {
    using U = typename std::make_unsigned<T>::type;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < P; i += (int64_t)gridDim.x * kBlock) {
        const T d = (T)(U)((U)y[i] - (U)x[i]);
        double t = (double)d * n;
        t = t / N;
        out[i] = (double)x[i] + t;
    }
}

// The same fold with a python-INT num_examples (numpy's weak int scalar takes the array's dtype):
// difference AND product wrap in T (computed in a >= 32-bit unsigned type, so no signed overflow
// and no int promotion surprises for 8/16-bit T), then true_divide by N in float64 and add x.
template <typename T>
__global__ void __launch_bounds__(kBlock) k_nfold(double* __restrict__ out, const T* __restrict__ x,
                                                  const T* __restrict__ y, T n, double N, int64_t P) {
    using U = typename std::make_unsigned<T>::type;
    using W = typename std::conditional<(sizeof(T) < 8), uint32_t, uint64_t>::type;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < P; i += (int64_t)gridDim.x * kBlock) {
        const W d = (W)(U)((W)(U)y[i] - (W)(U)x[i]);
        const T p = (T)(U)(d * (W)(U)n);
        out[i] = (double)x[i] + (double)p / N;
    }
}

// numpyhelper.norm (numpyhelper.py:106-117): np.linalg.norm(x, 1) of one tensor, accumulated in f64
// with a fixed (deterministic) order. Vector: sum |x|, grid-stride partials per block then one
// block sums the partials. Matrix (rows x cols, C order): column sums of |x| (one lane per
// column, rows in order), then the max over columns (NaN propagates, as numpy's max).
constexpr int kNormBlocks = 1024;
template <typename T>
__global__ void __launch_bounds__(kBlock) k_abssum_partial(const T* __restrict__ x, int64_t P, double* __restrict__ work) {
    __shared__ double red[kBlock];
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < P; i += (int64_t)gridDim.x * kBlock)
        acc += __builtin_fabs((double)x[i]);
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) work[blockIdx.x] = red[0];
}
template <typename T>
__global__ void __launch_bounds__(kBlock) k_colabssum(const T* __restrict__ x, int64_t rows, int64_t cols,
                                                      double* __restrict__ work) {
    for (int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x; c < cols; c += (int64_t)gridDim.x * kBlock) {
        double acc = 0.0;
        for (int64_t r = 0; r < rows; ++r) acc += __builtin_fabs((double)x[r * cols + c]);
        work[c] = acc;
    }
}
__global__ void __launch_bounds__(kBlock) k_final_reduce(const double* __restrict__ work, int64_t n, int is_max,
                                                         double* __restrict__ out) {
    __shared__ double red[kBlock];
    double acc = is_max ? -__builtin_inf() : 0.0;
    for (int64_t i = threadIdx.x; i < n; i += kBlock) {
        const double v = work[i];
        acc = is_max ? (acc != acc ? acc : (v != v || v > acc ? v : acc)) : acc + v;   // NaN wins, as numpy max
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            const double a = red[threadIdx.x], b = red[threadIdx.x + w];
            red[threadIdx.x] = is_max ? (a != a ? a : (b != b || b > a ? b : a)) : a + b;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (n == 0 && is_max) ? 0.0 : red[0];
}

// ----------------------------------------------------------------------------
// broadcast + widening conversion (fa_cast): numpy's implicit operand preparation when a
// client update differs from the running model in dtype or broadcastable shape. Only the
// per-tensor path (fedn_amd/mixed.py) uses it; the uniform-round kernels above never do.
// ----------------------------------------------------------------------------
constexpr int kCastMaxDim = 8;
struct CastGeom {
    int64_t shape[kCastMaxDim];    // out shape (C order)
    int64_t stride[kCastMaxDim];   // element strides of `in` per out dimension (0 = broadcast)
    int ndim;
};

template <typename TI, typename TO, bool BC>
__global__ void __launch_bounds__(kBlock)
k_cast(TO* __restrict__ out, const TI* __restrict__ in, const CastGeom g, const int64_t P) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < P; i += (int64_t)gridDim.x * kBlock) {
        int64_t j = i;
        if constexpr (BC) {
            int64_t rem = i;
            j = 0;
            for (int d = g.ndim - 1; d >= 0; --d) {
                const int64_t q = rem / g.shape[d];
                j += (rem - q * g.shape[d]) * g.stride[d];
                rem = q;
            }
        }
        if constexpr (std::is_same<TO, f16>::value && std::is_integral<TI>::value)
            out[i] = f16{f32_to_f16((float)in[j])};          // int8 / uint8 only: exact in half
        else if constexpr (std::is_same<TO, f16>::value && std::is_same<TI, float>::value)
            out[i] = f16{f32_to_f16(in[j])};                 // narrowing: round to nearest even (astype)
        else if constexpr (std::is_same<TO, float>::value && std::is_same<TI, double>::value)
            out[i] = (float)in[j];                           // narrowing: round to nearest even (astype)
        else
            out[i] = widen<TI, TO>(in[j]);
    }
}

// host side of fa_elementwise / fa_norm1: the grid of the grid-stride kernels above, the integer dtypes
dim3 elementwise_grid(int64_t P) { return dim3((unsigned)std::min<int64_t>((P + kBlock - 1) / kBlock, 8192)); }

// f(T{}) for the element type T of integer dtype `dt`; any other dtype fails with `fmt`, which takes dt
template <class F>
int for_int_dtype(int dt, F&& f, const char* fmt) {
    switch (dt) {
        case FA_I8: return f(int8_t{});
        case FA_I16: return f(int16_t{});
        case FA_I32: return f(int32_t{});
        case FA_I64: return f(int64_t{});
        case FA_U8: return f(uint8_t{});
        case FA_U16: return f(uint16_t{});
        case FA_U32: return f(uint32_t{});
        case FA_U64: return f(uint64_t{});
        default: return fail(FA_EDTYPE, fmt, dt);
    }
}
