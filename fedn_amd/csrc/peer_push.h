// peer_push.h — stores into the peers' copies of the model for the parameter-sliced all-gather: the
// fold that pushes its result (k_fedavg_push, fa_fedavg_fold_push), the push of a folded piece (k_push,
// k_push_tail, fa_push), and the system-scope release that follows either (k_release, launch_release).
// Included by fedagg.hip inside its anonymous namespace, after fold_rules.h and fedavg_kernels.h: the
// pushing fold is k_fedavg's arithmetic (strip_start, fold_strip, the client table), and the release
// reports through that file's error plumbing. DESIGN.md §5 describes the engines.

// Destinations a piece is pushed to besides its own buffer (the peers' model buffers, IPC-mapped
// or in-process): fa_push and the fused fold + push (fa_fedavg_fold_push).
constexpr int kPushMax = 16;
struct PushTable {
    u32x4* dst[kPushMax];
};

// k_fedavg with the all-gather fused in (fa_fedavg_fold_push; sharded.P2PAllGather engine "fused"):
// every finished strip is stored to this rank's own copy of the model AND to each peer's copy — the
// same vector stores a copy kernel would issue, straight from the registers that hold the result, so
// a round needs no second pass over the piece and no second launch. fp32 updates and aggregate,
// 16-B aligned buffers, one strip per lane; the fold arithmetic and order are k_fedavg's.
template <int U, bool INIT>
__global__ void __launch_bounds__(kBlock)
k_fedavg_push(float* __restrict__ agg, const ClientTable<CF32::S> tab, const int K, const int64_t P, PushTable t,
              const int nd) {
    using V = CF32::V;
    constexpr int E = 4;
    const int64_t strip = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t i0 = strip * E;
    if (i0 + E <= P) {
        V x[E];
        int k = strip_start<float, float, CF32, E, INIT, false, false>(x, agg, tab, i0, E);
        for (; k + U <= K; k += U) {
            float y[U][E];
#pragma unroll
            for (int u = 0; u < U; ++u) strip_load<float, E, false>(static_cast<const float*>(tab.ptr[k + u]) + i0, y[u]);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                V yv[E];
#pragma unroll
                for (int e = 0; e < E; ++e) yv[e] = widen<float, V>(y[u][e]);
                fold_strip<CF32, E>(x, yv, tab.n[k + u], tab.N[k + u], tab.r[k + u]);
            }
        }
        for (; k < K; ++k) {
            float y[E];
            strip_load<float, E, false>(static_cast<const float*>(tab.ptr[k]) + i0, y);
            V yv[E];
#pragma unroll
            for (int e = 0; e < E; ++e) yv[e] = widen<float, V>(y[e]);
            fold_strip<CF32, E>(x, yv, tab.n[k], tab.N[k], tab.r[k]);
        }
        float xo[E];
#pragma unroll
        for (int e = 0; e < E; ++e) xo[e] = narrow<float, V>(x[e]);
        u32x4 w;
        __builtin_memcpy(&w, xo, 16);
        __builtin_nontemporal_store(w, reinterpret_cast<u32x4*>(agg + i0));
        for (int d = 0; d < nd; ++d) __builtin_nontemporal_store(w, t.dst[d] + strip);
    } else if (i0 < P) {                                       // the ragged last strip
        const int rem = (int)(P - i0);
        V x[E];
        int k = strip_start<float, float, CF32, E, INIT, false, false>(x, agg, tab, i0, rem);
        for (; k < K; ++k) {
            const float* yp = static_cast<const float*>(tab.ptr[k]) + i0;
            for (int e = 0; e < rem; ++e) x[e] = CF32::fold(x[e], widen<float, V>(yp[e]), tab.n[k], tab.N[k], tab.r[k]);
        }
        for (int e = 0; e < rem; ++e) {
            const float v = narrow<float, V>(x[e]);
            agg[i0 + e] = v;
            for (int d = 0; d < nd; ++d) reinterpret_cast<float*>(t.dst[d])[i0 + e] = v;
        }
    }
}

// A system-scope release on every XCD after a grid that stored into other GPUs' memory
// (k_fedavg_push, k_push): the stores still held in an XCD's L2 are written back before anything
// later on the stream (the fence the ranks exchange). A release inside every wave of a large grid
// would write the L2s back hundreds of thousands of times, so a separate grid of kReleaseBlocks
// single-wave workgroups releases instead — but HIP does not promise which XCDs a grid's workgroups
// land on, so each workgroup reads the XCD it runs on (HW_REG_XCC_ID) and ORs it into the caller's
// release record (FA_REL_*, include/fedagg.h). The launch's last workgroup to arrive (an acq_rel
// arrival counter: it sees every other workgroup's bit) compares the number of distinct XCDs covered
// with the device's XCD count and counts a miss; the record is read by the caller at its next synchronisation
// (sharded.P2PAllGather.check_release), which fails the session on any miss. The mask and the
// arrival counter are reset by that last workgroup, so the next launch on the stream starts clean.
constexpr int kReleaseBlocks = 64;
constexpr unsigned kXccIdReg = (3u << 11) | 20u;   // s_getreg operand: HW_REG_XCC_ID, offset 0, 4 bits

__global__ void __launch_bounds__(64) k_release(unsigned* __restrict__ rec, unsigned expect) {
    if (threadIdx.x != 0) return;
    __threadfence_system();
    if (rec == nullptr) return;
    const unsigned xcc = __builtin_amdgcn_s_getreg(kXccIdReg) & 15u;
    __hip_atomic_fetch_or(rec + FA_REL_MASK, 1u << xcc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned before = __hip_atomic_fetch_add(rec + FA_REL_ARRIVED, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (before + 1 != gridDim.x) return;
    const unsigned seen = __hip_atomic_exchange(rec + FA_REL_MASK, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(rec + FA_REL_ARRIVED, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_or(rec + FA_REL_SEEN, seen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(rec + FA_REL_LAUNCHES, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(rec + FA_REL_EXPECT, expect, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // distinct XCDs seen vs the device's count (a partition mode may number its XCDs by their
    // physical index rather than 0 .. n - 1: the mask is reported, the count is what is checked)
    if (__builtin_popcount(seen) < __builtin_popcount(expect))
        __hip_atomic_fetch_add(rec + FA_REL_MISSES, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// XCDs of the current device (1 in a partition mode that exposes one XCD per device)
int device_xccs(int dev, int* n) {
    int v = 0;
    hipError_t e = hipDeviceGetAttribute(&v, hipDeviceAttributeNumberOfXccs, dev);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(FA_EHIP, "hipDeviceGetAttribute(NumberOfXccs, %d): %s", dev, hipGetErrorString(e));
    }
    if (v < 1 || v > 16) return fail(FA_EHIP, "device %d reports %d XCDs", dev, v);
    *n = v;
    return FA_OK;
}

int launch_release(hipStream_t st, unsigned* rec) {
    unsigned expect = 0;
    if (rec) {
        int dev = 0, nx = 0;
        (void)hipGetDevice(&dev);
        const int rc = device_xccs(dev, &nx);
        if (rc) return rc;
        expect = (nx >= 32) ? ~0u : ((1u << nx) - 1u);
    }
    hipLaunchKernelGGL(k_release, dim3(kReleaseBlocks), dim3(64), 0, st, rec, expect);
    return check_launch("release after peer stores");
}

// ----------------------------------------------------------------------------
// k_push: one folded piece to every peer's copy of the model (fa_push; sharded.P2PAllGather's
// "kernel" engine). Each lane loads a 16-B word of the piece ONCE and stores it to every
// destination: the piece crosses each peer's own xGMI link once, all links at once, and local HBM
// is read once instead of once per DMA copy. The stores are plain vector stores (non-temporal:
// nothing here is read back by this GPU); k_release after the grid makes them visible to the peers
// before the stream's next operation (the fence the ranks exchange).
// ----------------------------------------------------------------------------
constexpr int kPushWords = 4;                    // 16-B words per lane per iteration (64 B in flight)

__global__ void __launch_bounds__(kBlock) k_push(PushTable t, int nd, const u32x4* __restrict__ src, int64_t n16) {
    const int64_t stride = (int64_t)gridDim.x * kBlock * kPushWords;
    for (int64_t base = (int64_t)blockIdx.x * kBlock * kPushWords + threadIdx.x; base < n16; base += stride) {
        u32x4 v[kPushWords];
#pragma unroll
        for (int j = 0; j < kPushWords; ++j) {
            const int64_t i = base + (int64_t)j * kBlock;
            if (i < n16) v[j] = __builtin_nontemporal_load(src + i);
        }
        for (int d = 0; d < nd; ++d) {
            u32x4* __restrict__ o = t.dst[d];
#pragma unroll
            for (int j = 0; j < kPushWords; ++j) {
                const int64_t i = base + (int64_t)j * kBlock;
                if (i < n16) __builtin_nontemporal_store(v[j], o + i);
            }
        }
    }
}

// the < 16 B tail of a piece whose length is not a multiple of 16 (one lane per byte)
__global__ void k_push_tail(PushTable t, int nd, const uint8_t* __restrict__ src, int64_t off, int rem) {
    const int b = threadIdx.x;
    if (b < rem)
        for (int d = 0; d < nd; ++d) reinterpret_cast<uint8_t*>(t.dst[d])[off + b] = src[off + b];
}
