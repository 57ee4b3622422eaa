// host_common.h — host code that more than one kernel family's launch path uses: filling a launch's
// client table, the device's size (CUs, resident workgroups of a kernel), the robust entry points' dispatch
// by update dtype, and the argument checks and device mappings that several entry points share.
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

// the first null among a round's K update pointers, reported in `who`'s name
int check_updates(const char* who, const void* const* updates, int K) {
    for (int k = 0; k < K; ++k)
        if (!updates[k]) return fail(FA_EINVAL, "%s: updates[%d] is NULL", who, k);
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
