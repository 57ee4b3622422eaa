// order_wide.h — coordinate-wise trimmed mean / median over 1 .. 1024 client buffers (fa_order_mean_wide).
//
// Included by fedagg.hip inside its anonymous namespace, after order_mean.h: the keys, OrderTraits, order_ce,
// order_sort, order_out and the strip loads are that file's and fold_rules.h's, and the rule is order_mean.h's
// bit for bit; only the sort is new. k_order_mean keeps a coordinate's KP keys in one lane's
// registers, which ends at 64. Here a WAVEFRONT owns a coordinate: each lane holds R = KP / 64 keys, and a
// bitonic merge sort runs its in-lane stages as compile-time comparators on registers and its cross-lane stages
// as wavefront shuffles. DESIGN.md §3.14 has the split, the LDS layout, the resource table and the rates.
//
// One workgroup (4 wavefronts) takes a tile of C consecutive coordinates:
//   1. transposing load: each client's C-element segment is read coalesced (16-byte loads when every update
//      is 16-byte aligned and the tile is full, element-wise otherwise), turned into keys and stored to LDS
//      column by coordinate: key (coordinate c, client k) at c * STRIDE + k. Slots K .. KP-1 take the pad key;
//   2. sort: wavefront w sorts columns w, w + 4, ...: it reads the column striped (lane l: slots l, l + 64,
//      ...; the order the keys arrive in does not matter), sorts, and writes it back blocked (lane l: sorted
//      positions l * R .. l * R + R - 1) with 16-byte stores. STRIDE = KP + 16 bytes keeps every column
//      16-byte aligned and the transposing stores of step 1 at two lanes a bank, the least 64 lanes can do;
//   3. sum: lane c of the first wavefront walks column c from s[trim] to s[K - trim - 1] in the accumulator
//      type (the ascending sum is serial by definition), divides once and stores out[i0 + c].
// Nothing is written past P: the last tile loads, sorts and stores its P - i0 columns only.

constexpr int kMaxWideK = 1024;          // clients of one fa_order_mean_wide call
constexpr int kWideFill = 256;           // pointers one k_fill_ptrs launch carries in its kernarg (2 KiB)
constexpr int kWideTileBytes = 32 << 10; // LDS of a tile's keys where the 64-byte segment rule leaves a choice
constexpr int kWideLoads = 4;            // segment loads a lane issues before it stores the first key

// ----------------------------------------------------------------------------
// the client table in device memory: 1024 pointers do not fit a kernarg
// ----------------------------------------------------------------------------
struct WidePtrChunk {
    const void* ptr[kWideFill];
};

// dst[i] = chunk.ptr[i], i < n: the chunk travels by value in the kernarg, so the host array it came from
// may be gone when the kernel runs; the table is written in stream order ahead of the kernel that reads it.
__global__ void __launch_bounds__(kWideFill)
k_fill_ptrs(const void** __restrict__ dst, const WidePtrChunk chunk, const int n) {
    const int i = threadIdx.x;
    if (i < n) dst[i] = chunk.ptr[i];
}

// ----------------------------------------------------------------------------
// geometry of one instantiation
// ----------------------------------------------------------------------------
template <typename T, int KP>
struct WideGeom {
    using KEY = typename OrderTraits<T>::KEY;
    static_assert(KP >= 128 && KP <= kMaxWideK && (KP & (KP - 1)) == 0, "KP is 128, 256, 512 or 1024");
    static constexpr int R = KP / 64;                                   // keys a lane
    static constexpr int CMIN = 64 / (int)sizeof(T);                    // a client's segment: 64 bytes at least
    static constexpr int CFIT = kWideTileBytes / (KP * (int)sizeof(KEY));
    static constexpr int C = CFIT < CMIN ? CMIN : (CFIT > 64 ? 64 : CFIT);   // coordinates a tile (<= 64: one wavefront sums)
    static constexpr int STRIDE = KP + 16 / (int)sizeof(KEY);           // keys from one column to the next
    static constexpr size_t LDS = (size_t)C * STRIDE * sizeof(KEY);
    static_assert(C % (kBlock / 64) == 0 && C * (int)sizeof(T) % 16 == 0, "whole 16-byte chunks, columns for every wavefront");
};

// ----------------------------------------------------------------------------
// the sort of one column by one wavefront
// ----------------------------------------------------------------------------
template <typename KEY>
__device__ __forceinline__ KEY wide_lane_xor(KEY v, int mask) {
    if constexpr (sizeof(KEY) == 4) {
        return (KEY)__shfl_xor((unsigned int)v, mask, 64);
    } else {
        const unsigned int lo = __shfl_xor((unsigned int)v, mask, 64);
        const unsigned int hi = __shfl_xor((unsigned int)(v >> 32), mask, 64);
        return ((KEY)hi << 32) | lo;
    }
}

// the lower lane of a cross-lane comparator keeps the smaller key, the upper lane the larger one
template <typename KEY>
__device__ __forceinline__ KEY wide_keep(KEY mine, KEY other, bool lower) {
    const KEY lo = other < mine ? other : mine;
    const KEY hi = other < mine ? mine : other;
    return lower ? lo : hi;
}

// Ascending sort of the KP = 64 * R keys of a wavefront; position i = lane * R + r afterwards. order_sort
// sorts each lane's R keys; then sorted runs of k / 2 are merged into runs of k, k = 2R .. KP, by the
// all-ascending form of the bitonic merge: position i against k - 1 - i within its run of k (lane ^ (k / R - 1),
// register R - 1 - r), then half-cleaners at distance j = k / 4 .. 1 — across lanes (lane ^ (j / R), the same
// register) while j >= R, between registers below.
template <typename KEY, int R>
__device__ __forceinline__ void wide_sort(KEY (&key)[R], const int lane) {
    constexpr int KP = 64 * R;
    order_sort<KEY, R>(key);
#pragma unroll
    for (int k = 2 * R; k <= KP; k *= 2) {
        {
            const bool lower = (lane & (k / (2 * R))) == 0;
            KEY o[R];
#pragma unroll
            for (int r = 0; r < R; ++r) o[r] = wide_lane_xor(key[R - 1 - r], k / R - 1);
#pragma unroll
            for (int r = 0; r < R; ++r) key[r] = wide_keep(key[r], o[r], lower);
        }
#pragma unroll
        for (int j = k / 4; j >= R; j /= 2) {
            const bool lower = (lane & (j / R)) == 0;
#pragma unroll
            for (int r = 0; r < R; ++r) key[r] = wide_keep(key[r], wide_lane_xor(key[r], j / R), lower);
        }
#pragma unroll
        for (int j = R / 2; j >= 1; j /= 2) {
#pragma unroll
            for (int r = 0; r < R; ++r)
                if ((r & j) == 0) order_ce(key[r], key[r | j]);
        }
    }
}

// a lane's R sorted keys to its block of the column: 16-byte stores (8 bytes for two 32-bit keys)
template <typename KEY, int R>
__device__ __forceinline__ void wide_store_block(KEY* __restrict__ p, const KEY (&key)[R]) {
    constexpr int bytes = R * (int)sizeof(KEY);
    if constexpr (bytes % 16 == 0) {
#pragma unroll
        for (int j = 0; j < bytes / 16; ++j) {
            u32x4 w;
            __builtin_memcpy(&w, reinterpret_cast<const char*>(key) + 16 * j, 16);
            reinterpret_cast<u32x4*>(p)[j] = w;
        }
    } else {
        static_assert(bytes == 8, "two 32-bit keys");
        u32x2 w;
        __builtin_memcpy(&w, reinterpret_cast<const char*>(key), 8);
        *reinterpret_cast<u32x2*>(p) = w;
    }
}

// ----------------------------------------------------------------------------
// the kernel
// ----------------------------------------------------------------------------
// KP / 2 < K <= KP (K <= 128 at KP = 128). vec: every update is 16-byte aligned. Dynamic LDS: WideGeom::LDS bytes.
template <typename T, int KP>
__global__ void __launch_bounds__(kBlock)
k_order_wide(typename OrderTraits<T>::O* __restrict__ out, const void* const* __restrict__ tab, const int K,
             const int trim, const int64_t P, const int vec) {
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

    // 2. one wavefront a column
    const int lane = tid & 63;
    for (int c = tid >> 6; c < ncols; c += kBlock / 64) {
        KEY* const col = lds + c * STRIDE;
        KEY key[R];
#pragma unroll
        for (int r = 0; r < R; ++r) key[r] = col[r * 64 + lane];
        wide_sort<KEY, R>(key, lane);
        wide_store_block<KEY, R>(col + lane * R, key);   // (the wavefront's loads of this column are all done)
    }
    __syncthreads();

    // 3. the ascending sum of the kept slots, one lane a coordinate
    if (tid < ncols) {
        const KEY* const col = lds + tid * STRIDE;
        const int hi = K - trim;                         // kept slots: trim <= j < hi
        A acc = TR::val(col[trim]);
#pragma unroll 8
        for (int j = trim + 1; j < hi; ++j) acc = acc + TR::val(col[j]);
        out[i0 + tid] = order_out<A, O>(acc / (A)(K - 2 * trim));
    }
}

// f(std::integral_constant<int, KP>{}) for the padded client count of K: 128 up to K = 128, then the power
// of two with KP / 2 < K <= KP
template <typename F>
auto for_wide_kp(int K, F&& f) {
    if (K <= 128) return f(std::integral_constant<int, 128>{});
    if (K <= 256) return f(std::integral_constant<int, 256>{});
    if (K <= 512) return f(std::integral_constant<int, 512>{});
    return f(std::integral_constant<int, 1024>{});
}

// The device's LDS limit for one workgroup, and the kernel's dynamic-LDS attribute raised to `bytes`
// (needed past 64 KiB). Asked at every launch: the process may drive several devices. Reported in `who`'s name.
template <typename KERNEL>
int wide_raise_lds(const char* who, KERNEL kernel, size_t bytes) {
    int dev = 0, limit = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, dev);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(FA_EHIP, "%s: LDS limit query: %s", who, hipGetErrorString(e));
    }
    if ((size_t)limit < bytes)
        return fail(FA_EHIP, "%s: the tile needs %zu bytes of LDS, the device gives a workgroup %d", who, bytes, limit);
    if (bytes > (64u << 10)) {
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(FA_EHIP, "%s: raising the dynamic LDS limit to %zu: %s", who, bytes, hipGetErrorString(e));
        }
    }
    return FA_OK;
}

// The launch path of the two wide kernels, k_order_wide and window_wide.h's k_window_wide, reported in the entry
// point `who`'s name: the bound on P, the LDS limit, the client table written to `work` in stream order, the
// padded client count KP. pick(kp) gives the <T, KP> instantiation (kp a std::integral_constant tag), `name`
// what fa_last_kernel reports, `count` the rule's own argument (trim or keep).
template <typename T, typename PICK>
int launch_wide_kernel(const char* who, const char* name, void* out, const void* const* ups, int K, int count, int64_t P,
                       void* work, hipStream_t st, PICK&& pick) {
    return for_wide_kp(K, [&](auto kp) -> int {
        using G = WideGeom<T, decltype(kp)::value>;
        // grid = ceil(P / C) workgroups must fit the 32-bit grid dimension
        if (P > (int64_t)0x7FFFFFFF * G::C) return fail(FA_EINVAL, "%s: P=%lld is too large", who, (long long)P);
        auto kernel = pick(kp);
        if (const int rc = wide_raise_lds(who, kernel, G::LDS)) return rc;
        const void** tab = static_cast<const void**>(work);
        bool vec = true;
        for (int k0 = 0; k0 < K; k0 += kWideFill) {
            WidePtrChunk chunk;
            const int n = std::min(kWideFill, K - k0);
            for (int j = 0; j < kWideFill; ++j) {
                chunk.ptr[j] = j < n ? ups[k0 + j] : nullptr;
                if (j < n) vec = vec && aligned16(ups[k0 + j]);
            }
            hipLaunchKernelGGL(k_fill_ptrs, dim3(1), dim3(kWideFill), 0, st, tab + k0, chunk, n);
        }
        g_kernel = name;
        hipLaunchKernelGGL(kernel, dim3((unsigned)((P + G::C - 1) / G::C)), dim3(kBlock), G::LDS, st,
                           static_cast<typename OrderTraits<T>::O*>(out), tab, K, count, P, (int)vec);
        char what[64];
        std::snprintf(what, sizeof(what), "%s: kernel launch", who);
        return check_launch(what);
    });
}

template <typename T>
int launch_order_wide(void* out, const void* const* ups, int K, int trim, int64_t P, void* work, hipStream_t st) {
    return launch_wide_kernel<T>("fa_order_mean_wide", "k_order_wide", out, ups, K, trim, P, work, st,
                                 [](auto kp) { return k_order_wide<T, decltype(kp)::value>; });
}
