// host_common.h — host code that more than one kernel family's launch path uses: filling a launch's
// client table (the fold's, and the robust kernels' table of pointers), the device's size (CUs, resident
// workgroups of a kernel), the robust entry points' dispatch by update dtype and by padded client count, the
// output dtype that goes with an update dtype, and the argument checks and device mappings that several entry
// points share.
//
// Included by fedagg.hip inside its anonymous namespace, after the kernel headers and probes.h: it uses
// ClientTable (fold_rules.h), the cfg_* getters (probes.h) and that file's error plumbing.

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// numpy's conversion of a python int to float16 (round-to-nearest-even), kept in f32
// a python float / int as numpy's float16 weak scalar: ONE round-to-nearest-even from double (held in
// an f32; every half is exact in f32)
float to_half_value(double v) { return (float)(_Float16)v; }

// Clients k0 .. k0 + cnt of a round into one launch's table. half: numpy casts the python n, N to the
// half dtype (CF16), so the table carries them pre-rounded.
template <typename S>
void fill_table(ClientTable<S>& t, const void* const* ptrs, const double* n, const double* N, int k0, int cnt,
                bool half = false) {
    for (int j = 0; j < cnt; ++j) {
        t.ptr[j] = ptrs[k0 + j];
        t.n[j] = half ? (S)to_half_value(n[k0 + j]) : (S)n[k0 + j];
        t.N[j] = half ? (S)to_half_value(N[k0 + j]) : (S)N[k0 + j];
        if constexpr (std::is_same<S, double>::value) {
            // CF64's division shortcut: r = RN64(1/N) for 2^-60 <= |N| <= 2^60 (CWSUM ignores r,
            // CRUN overwrites it)
            const double Nd = N[k0 + j], a = std::fabs(Nd);
            t.r[j] = (cfg_fastdiv64() && a >= 0x1p-60 && a <= 0x1p60) ? 1.0 / Nd : 0.0;
        } else {
            // reciprocal for CF32's division shortcut: only for N that keep every normal-range
            // quotient normal (|N| < 2^28) and only when enabled
            const float Nf = (float)N[k0 + j];
            t.r[j] = (cfg_fastdiv() && Nf != 0.0f && std::fabs(Nf) < 0x1p28f) ? 1.0 / (double)Nf : 0.0;
        }
    }
    for (int j = cnt; j < kMaxK; ++j) {
        t.ptr[j] = nullptr;
        t.n[j] = 0;
        t.N[j] = 0;
        t.r[j] = 0.0;
    }
}

// The K update pointers of a robust launch into its table's kMaxK entries (PairTable, OrderTable, WmTable:
// nullptr past K); true when every one of the K is 16-byte aligned.
bool fill_ptrs(const void* (&ptr)[kMaxK], const void* const* ups, int K) {
    bool vec = true;
    for (int k = 0; k < kMaxK; ++k) {
        ptr[k] = k < K ? ups[k] : nullptr;
        if (k < K) vec = vec && aligned16(ups[k]);
    }
    return vec;
}

int64_t grid_for(int64_t P, int E) {
    const int64_t strips = (P + E - 1) / E;
    return (strips + kBlock - 1) / kBlock;
}

int device_cus() {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        cus = 256;
    return cus > 0 ? cus : 256;
}

// Resident workgroups of KERNEL per CU at BLK lanes and no dynamic LDS (0: the query failed); asked
// once per instantiation.
template <auto KERNEL, int BLK>
int resident_blocks() {
    static std::atomic<int> blocks_per_cu{-1};
    int nb = blocks_per_cu.load(std::memory_order_relaxed);
    if (nb < 0) {
        nb = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, KERNEL, BLK, 0) != hipSuccess) nb = 0;
        blocks_per_cu.store(nb, std::memory_order_relaxed);
    }
    return nb;
}

// f(T{}) with the element type T of `dtype`, one of the six the robust kernels take (the caller has checked it)
template <typename F>
auto for_dtype(int dtype, F&& f) {
    switch (dtype) {
        case FA_F32: return f(float{});
        case FA_F16: return f(f16{});
        case FA_BF16: return f(bf16{});
        case FA_F64: return f(double{});
        case FA_I32: return f(int32_t{});
        default: return f(int64_t{});
    }
}

// f(std::integral_constant<int, KP>{}) for the padded client count of K: the power of two KP <= 64 with
// KP / 2 < K <= KP, and MIN (2 or 8) for fewer clients. No KP below MIN is instantiated.
template <int MIN, typename F>
auto for_kp(int K, F&& f) {
    static_assert(MIN == 2 || MIN == 8, "the sort and pairwise kernels start at 2, the fused distance kernels at 8");
    if constexpr (MIN == 2) {
        if (K <= 2) return f(std::integral_constant<int, 2>{});
        if (K <= 4) return f(std::integral_constant<int, 4>{});
    }
    if (K <= 8) return f(std::integral_constant<int, 8>{});
    if (K <= 16) return f(std::integral_constant<int, 16>{});
    if (K <= 32) return f(std::integral_constant<int, 32>{});
    return f(std::integral_constant<int, 64>{});
}

// The output dtype that goes with updates of `upd_dtype` in the robust rules (ops.order_mean_dtype): the float
// dtype itself, f32 for bf16, f64 for the integers; -1 for a dtype that is none of the six.
int order_out_dtype(int upd_dtype) {
    switch (upd_dtype) {
        case FA_F32: case FA_BF16: return FA_F32;
        case FA_F16: return FA_F16;
        case FA_F64: case FA_I32: case FA_I64: return FA_F64;
        default: return -1;
    }
}

// the first null among a round's K update pointers, reported in `who`'s name
int check_updates(const char* who, const void* const* updates, int K) {
    for (int k = 0; k < K; ++k)
        if (!updates[k]) return fail(FA_EINVAL, "%s: updates[%d] is NULL", who, k);
    return FA_OK;
}

// The argument checks of the two sort entry points (fa_trimmed_mean, fa_median_window_mean), reported in
// `who`'s name, in two halves: the entry point's own bound on its count (trim, keep) is refused between them,
// after a bad K and before a bad P, as it always was.
int check_sort_ptrs(const char* who, const void* out, const void* const* updates, int K) {
    if (!out || !updates) return fail(FA_EINVAL, "%s: null pointer argument", who);
    if (K < 1 || K > kMaxK) return fail(FA_EINVAL, "%s: K=%d outside 1..%d", who, K, kMaxK);
    return FA_OK;
}

int check_sort_size(const char* who, int out_dtype, int upd_dtype, int64_t P) {
    if (P < 0) return fail(FA_EINVAL, "%s: negative size (P=%lld)", who, (long long)P);
    const int want = order_out_dtype(upd_dtype);
    if (want < 0 || out_dtype != want)
        return fail(FA_EDTYPE, "%s: unsupported dtype pair (update %d, output %d)", who, upd_dtype, out_dtype);
    return FA_OK;
}

// A host-mapped round (fa_*_host): the device mappings of its K page-locked update buffers into dev[].
// `e` is the status of the mappings the caller made first (its model buffers); a failure of any of them
// is reported here.
int map_host_updates(const char* who, hipError_t e, const void* const* updates, int K, const void** dev) {
    for (int k = 0; e == hipSuccess && k < K; ++k) {
        void* d = nullptr;
        if (!updates[k]) return fail(FA_EINVAL, "%s: updates[%d] is NULL", who, k);
        e = hipHostGetDevicePointer(&d, const_cast<void*>(updates[k]), 0);
        dev[k] = d;
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(FA_EINVAL, "%s: %s (not page-locked host memory?)", who, hipGetErrorString(e));
    }
    return FA_OK;
}

// ... and its end: the launch's status, or the wait for the model to be on the host
int wait_host_round(const char* who, int rc, void* stream) {
    if (rc != FA_OK) return rc;
    const hipError_t e = hipStreamSynchronize(static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(FA_EHIP, "%s: hipStreamSynchronize: %s", who, hipGetErrorString(e));
    return FA_OK;
}
