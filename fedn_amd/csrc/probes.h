// probes.h — everything that exists only in the probe build (-DFEDAGG_PROBES -> libfedagg_probe.so;
// tools/ and the division tests): the measurement rules CADD / CADDNW, the probe kernels (k_fedopt_cwp,
// k_fedopt_mix, k_fedopt_mixw, k_stream_copy, k_stream_read), the fa_tune knob block g_cfg with its
// cfg_* getters, and the probe_* hooks through which the knobs reach the launch functions. The product
// build gets the #else branch at the end instead: the getters as constants, the hooks as stubs that
// change nothing, so no launch function needs a conditional of its own. The probe build's entry
// points (fa_tune, ...) are in probes_abi.h.
//
// Included by fedagg.hip inside its anonymous namespace, after every kernel header (the probe kernels
// are variants of theirs) and before host_common.h and the launch headers, which call the getters and
// hooks. DESIGN.md §3.5 lists the measurement kernels; include/fedagg_probe.h numbers the knobs.

#ifdef FEDAGG_PROBES

// ----------------------------------------------------------------------------
// measurement rules and kernels
// ----------------------------------------------------------------------------
struct CADD {            // measurement only: x <- x + y (same traversal as the fold, minimal VALU)
    using V = float;
    using S = float;
    __device__ static __forceinline__ V fold(V x, V y, S, S, double) { return x + y; }
};
struct CADDNW : CADD {};  // measurement only: CADD whose store is skipped (never-true data test)
template <> struct is_nostore<CADDNW> : std::true_type {};

// store-window probe on a wave of a multi-launch round (staging.FedOptPipeline: the first or a middle
// launch, pg written back to the workspace; fa_tune OPT_WIN_PERIOD > 0 with OPT_WIN_PROD = 1):
// k_fedopt_c's bits. Null for the product: 8 bf16 updates over fp64 pg, 250 M params, every period
// 400-2500 ticks slower than no window (first +7...+76 %, middle +1...+34 %;
// profiles/r05_wave_window.log) — the 20-25 % write share of the FedAvg bf16 K = 8 case.
template <typename Y, typename OLD, class PG, bool FIRST, bool NT>
__global__ void __launch_bounds__(kBlock)
k_fedopt_cwp(const OptBuffers b, const OptScalars s, const ClientTable<typename PG::S> tab, const int K, const int64_t P,
             const uint32_t period, const uint32_t win_w) {
    fedopt_c_body<Y, OLD, PG, FIRST, false, NT, 1, 4, kUnroll / 2, false, true>(b, s, tab, K, P, period, win_w);
}

// access-pattern probe (FA_TUNE_OPT_MIX): exactly k_fedopt_c's loads and stores for a FIRST|FINAL
// launch — the element map (4 pairs per lane), clients loaded 4 at a time then the K % 4 remainder,
// the state after the fold, non-temporal stores of v / out / m — with the arithmetic cut to one
// add per value: the ceiling of the kernel's HBM traffic pattern alone. Whole wave tiles only.
template <typename Y, typename OLD, typename S, bool NT>
__global__ void __launch_bounds__(kBlock)
k_fedopt_mix(const OptBuffers b, const ClientTable<S> tab, const int K, const int64_t P) {
    constexpr int NH = 4, H = 2, E = 2 * NH, U = kUnroll / 2;
    constexpr int64_t T = 128 * NH;
    const int64_t base = ((int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * T;
    if (base + T > P) return;
    const int64_t i0 = base + 2 * (threadIdx.x & 63);
    auto at = [i0](int h) { return i0 + (int64_t)h * 128; };
    double acc[E];
    {
        OLD old[E];
#pragma unroll
        for (int h = 0; h < NH; ++h) strip_load<OLD, H, false>(static_cast<const OLD*>(b.old) + at(h), *reinterpret_cast<OLD(*)[H]>(&old[h * H]));
#pragma unroll
        for (int e = 0; e < E; ++e) acc[e] = (double)widen<OLD, double>(old[e]);
    }
    auto add_client = [&](int k, Y (&y)[E]) {
        const Y* yp = static_cast<const Y*>(tab.ptr[k]);
#pragma unroll
        for (int h = 0; h < NH; ++h) strip_load<Y, H, NT>(yp + at(h), *reinterpret_cast<Y(*)[H]>(&y[h * H]));
    };
    int k = 0;
    {
        Y y[E];
        add_client(0, y);
#pragma unroll
        for (int e = 0; e < E; ++e) acc[e] += (double)widen<Y, double>(y[e]);
        k = 1;
    }
    for (; k + U <= K; k += U) {
        Y y[U][E];
#pragma unroll
        for (int u = 0; u < U; ++u) add_client(k + u, y[u]);
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int e = 0; e < E; ++e) acc[e] += (double)widen<Y, double>(y[u][e]);
    }
    for (; k < K; ++k) {
        Y y[E];
        add_client(k, y);
#pragma unroll
        for (int e = 0; e < E; ++e) acc[e] += (double)widen<Y, double>(y[e]);
    }
#pragma unroll
    for (int h = 0; h < NH; ++h) {
        double mi[H] = {}, vv[H] = {};
        opt_load_state<H>(b, OptScalars{}, at(h), H, mi, vv);
        double m[H], v[H], o[H];
#pragma unroll
        for (int e = 0; e < H; ++e) {
            m[e] = mi[e] + acc[h * H + e];
            v[e] = vv[e] + acc[h * H + e];
            o[e] = acc[h * H + e];
        }
        strip_store<double, H, 1>(static_cast<double*>(b.v_out) + at(h), v);
        strip_store<double, H, 1>(static_cast<double*>(b.out) + at(h), o);
        if (b.m_out_f64) strip_store<double, H, 1>(static_cast<double*>(b.m_out) + at(h), m);
        else {
            float mf[H];
#pragma unroll
            for (int e = 0; e < H; ++e) mf[e] = (float)m[e];
            strip_store<float, H, 1>(static_cast<float*>(b.m_out) + at(h), mf);
        }
    }
}

// clock-windowed store probe (FA_TUNE_OPT_WIN_*): k_fedopt_mix's access pattern with the whole chip's
// stores confined to a common time window. Every wave reads the GPU's 100 MHz reference clock
// (s_memrealtime, one counter for all XCDs) and issues its v / out / m stores only while
// clock mod period < win_w, and (mode >= 1) starts a tile's reads, or (mode 2) each client batch's
// reads, only outside that window — so the DRAM sees read-only stretches and write bursts instead of
// 36 streams with 14 % writes interleaved everywhere, without a grid barrier. Waits are bounded by
// one period; results are k_fedopt_mix's.
template <typename Y, typename OLD, typename S, bool NT>
__global__ void __launch_bounds__(kBlock)
k_fedopt_mixw(const OptBuffers b, const ClientTable<S> tab, const int K, const int64_t P, const uint32_t period,
              const uint32_t win_w, const int mode) {
    constexpr int NH = 4, H = 2, E = 2 * NH, U = kUnroll / 2;
    constexpr int64_t T = 128 * NH;
    const int64_t base = ((int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * T;
    if (base + T > P) return;
    const int64_t i0 = base + 2 * (threadIdx.x & 63);
    auto at = [i0](int h) { return i0 + (int64_t)h * 128; };
    if (mode >= 1) wait_read_window(period, win_w);
    double acc[E];
    {
        OLD old[E];
#pragma unroll
        for (int h = 0; h < NH; ++h) strip_load<OLD, H, false>(static_cast<const OLD*>(b.old) + at(h), *reinterpret_cast<OLD(*)[H]>(&old[h * H]));
#pragma unroll
        for (int e = 0; e < E; ++e) acc[e] = (double)widen<OLD, double>(old[e]);
    }
    auto add_client = [&](int k, Y (&y)[E]) {
        const Y* yp = static_cast<const Y*>(tab.ptr[k]);
#pragma unroll
        for (int h = 0; h < NH; ++h) strip_load<Y, H, NT>(yp + at(h), *reinterpret_cast<Y(*)[H]>(&y[h * H]));
    };
    int k = 0;
    {
        Y y[E];
        add_client(0, y);
#pragma unroll
        for (int e = 0; e < E; ++e) acc[e] += (double)widen<Y, double>(y[e]);
        k = 1;
    }
    for (; k + U <= K; k += U) {
        if (mode >= 2) wait_read_window(period, win_w);
        Y y[U][E];
#pragma unroll
        for (int u = 0; u < U; ++u) add_client(k + u, y[u]);
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int e = 0; e < E; ++e) acc[e] += (double)widen<Y, double>(y[u][e]);
    }
    for (; k < K; ++k) {
        Y y[E];
        add_client(k, y);
#pragma unroll
        for (int e = 0; e < E; ++e) acc[e] += (double)widen<Y, double>(y[e]);
    }
    double mo[E], vo[E];
#pragma unroll
    for (int h = 0; h < NH; ++h) {
        double mi[H] = {}, vv[H] = {};
        opt_load_state<H>(b, OptScalars{}, at(h), H, mi, vv);
#pragma unroll
        for (int e = 0; e < H; ++e) {
            mo[h * H + e] = mi[e] + acc[h * H + e];
            vo[h * H + e] = vv[e] + acc[h * H + e];
        }
    }
    wait_write_window(period, win_w);
#pragma unroll
    for (int h = 0; h < NH; ++h) {
        strip_store<double, H, 1>(static_cast<double*>(b.v_out) + at(h), *reinterpret_cast<double(*)[H]>(&vo[h * H]));
        strip_store<double, H, 1>(static_cast<double*>(b.out) + at(h), *reinterpret_cast<double(*)[H]>(&acc[h * H]));
        strip_store<double, H, 1>(static_cast<double*>(b.m_out) + at(h), *reinterpret_cast<double(*)[H]>(&mo[h * H]));
    }
}

// the stream probes (fa_stream_copy / fa_stream_read)
__global__ void __launch_bounds__(kBlock) k_stream_copy(u32x4* __restrict__ dst, const u32x4* __restrict__ src, int64_t n16) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n16) dst[i] = __builtin_nontemporal_load(src + i);
}

constexpr int kReadPerLane = 16;
template <int RPL>
__global__ void __launch_bounds__(kBlock) k_stream_read(const u32x4* __restrict__ src, int64_t n16, u32x4* __restrict__ sink) {
    const int64_t base = (int64_t)blockIdx.x * kBlock * RPL + threadIdx.x;
    u32x4 acc = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < RPL; ++j) {
        const int64_t i = base + (int64_t)j * kBlock;
        if (i < n16) acc ^= __builtin_nontemporal_load(src + i);
    }
    // one 16-B word per block keeps the loads alive; the bandwidth probe needs no exact reduction
    __shared__ u32x4 red[kBlock];
    red[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        u32x4 r = red[0];
        for (int t = 1; t < kBlock; ++t) r ^= red[t];
        sink[blockIdx.x] = r;
    }
}

// Launch configuration. The product library (libfedagg.so) is built with the measured-best
// settings as compile-time constants: nothing in it is mutable or process-global. The probe
// build (-DFEDAGG_PROBES -> libfedagg_probe.so, tools/ and the division tests only) adds the
// fa_tune knobs that produced those measurements (profiles/r01_microbench.md).
struct FedAvgCfg {
    std::atomic<int> strips{4}, unroll{0}, lanetab{0}, grid_per_cu{0}, read_per_lane{16}, block_log{8},
        sum_nostore{0}, nt_store{1}, nt{0}, fastdiv{1}, fastdiv64{1}, narrow{1}, auto_geom{1}, opt_mix{0},
        opt_win_period{0}, opt_win_w{0}, opt_win_mode{0}, opt_win_prod{0}, avg_win_period{0}, avg_win_w{0},
        avg_win_mode{0}, avg_park_depth{0}, avg_park_slots{0}, avg_park_height{0}, avg_park_loadpol{0};
};
FedAvgCfg g_cfg;
int cfg_fastdiv() { return g_cfg.fastdiv.load(std::memory_order_relaxed); }
int cfg_fastdiv64() { return g_cfg.fastdiv64.load(std::memory_order_relaxed); }
int cfg_grid_per_cu() { return g_cfg.grid_per_cu.load(std::memory_order_relaxed); }

// what the hooks below dispatch to in fedavg_launch.h, which follows
template <auto KERNEL, int BLK>
int64_t avg_park_grid(int64_t ntiles, int per_cu);
template <typename Y, typename X, class CP, int E, int S, bool NT, bool LT, int BLK, int NTS, int MAP>
void launch_fedavg_pipe(X* a, const ClientTable<typename CP::S>& tab, int cnt, int64_t P, bool first, bool int_first,
                        hipStream_t st);
template <typename Y, typename X, class CP, int E, int S, int U, bool NT>
void launch_fedavg_geom(X* a, const ClientTable<typename CP::S>& tab, int cnt, int64_t P, bool first, bool int_first,
                        hipStream_t st);
template <typename Y, typename X, class CP, int E>
void launch_fedavg_small(X* a, const ClientTable<typename CP::S>& tab, int cnt, int64_t P, bool first, bool int_first,
                         hipStream_t st);
template <typename Y>
inline bool pipe_pays(int64_t P);

// ----------------------------------------------------------------------------
// probe overrides (libfedagg_probe.so only): everything the fa_tune knobs change in the launch functions
// (fedavg_launch.h, fedopt_launch.h). Each hook leaves the product's choice alone while its knobs are at their defaults.
// ----------------------------------------------------------------------------

// AVG_WIN_PERIOD / _W / _MODE on a first fold launch: -1 = no window, > 0 = this one
void probe_avg_window(AvgWindow& w, int& mode) {
    const int period = g_cfg.avg_win_period;
    if (period < 0) w = AvgWindow{};
    else if (period > 0) {
        w = AvgWindow{(uint32_t)period, (uint32_t)g_cfg.avg_win_w.load()};
        mode = g_cfg.avg_win_mode.load();
    }
}

// AVG_PARK_DEPTH / _SLOTS / _HEIGHT / _LOADPOL on a parked launch: all 0 = the product's kernel
// (false); otherwise the generalised one (k_fedavg_park; a knob left at 0 is 2 buffers / 1 slot /
// height 1 / the default policy), GRID n = n workgroups per CU. Instantiated: the nine (DEPTH, SLOTS)
// at height 1 and the default policy; ring 2 at (HEIGHT, SLOTS) = (1, 1), (1, 2), (2, 1), (2, 2),
// (4, 1) at every policy; ring 3 at height 2, 1 and 2 slots. Anything else launches nothing and
// reports "k_fedavg_park (not instantiated)" as the kernel family. The launcher reports the
// product's family for a launch: one fold, one name.
template <typename Y, typename X, class CP, int E, int S, int BLK, int NTS>
bool probe_fedavg_park(X* a, const ClientTable<typename CP::S>& tab, int cnt, int64_t P, uint32_t period, uint32_t win_w,
                       hipStream_t st) {
    const int depth = g_cfg.avg_park_depth, slots = g_cfg.avg_park_slots, height = g_cfg.avg_park_height;
    const int pol = g_cfg.avg_park_loadpol;
    if (!depth && !slots && !height && !pol) return false;
    constexpr int64_t kTile = (int64_t)BLK * S * E;
    switch ((depth ? depth : 2) * 1000 + (height ? height : 1) * 100 + (slots ? slots : 1) * 10 + pol) {
#define FA_PARK(D_, H_, S_, P_) \
    case D_ * 1000 + H_ * 100 + S_ * 10 + P_: { \
        constexpr auto kernel = k_fedavg_park<Y, X, CP, E, S, BLK, NTS, D_, S_, H_, P_>; \
        const dim3 pgrid((unsigned)avg_park_grid<kernel, BLK>(park_partition(P, kTile, H_).units(), cfg_grid_per_cu())); \
        hipLaunchKernelGGL(kernel, pgrid, dim3(BLK), 0, st, a, tab, cnt, P, period, win_w); \
        break; \
    }
#define FA_PARK_POLS(D_, H_, S_) FA_PARK(D_, H_, S_, 0) FA_PARK(D_, H_, S_, 1) FA_PARK(D_, H_, S_, 2) FA_PARK(D_, H_, S_, 3)
        FA_PARK_POLS(2, 1, 1) FA_PARK_POLS(2, 1, 2) FA_PARK_POLS(2, 2, 1) FA_PARK_POLS(2, 2, 2) FA_PARK_POLS(2, 4, 1)
        FA_PARK(2, 1, 4, 0) FA_PARK(3, 1, 1, 0) FA_PARK(3, 1, 2, 0) FA_PARK(3, 1, 4, 0) FA_PARK(4, 1, 1, 0) FA_PARK(4, 1, 2, 0) FA_PARK(4, 1, 4, 0)
        FA_PARK(3, 2, 1, 0) FA_PARK(3, 2, 2, 0)
#undef FA_PARK_POLS
#undef FA_PARK
        default:                                         // nothing runs: no other kernel stands in for a missing one
            g_kernel = "k_fedavg_park (not instantiated)";
            return true;
    }
    g_kernel = "k_fedavg_pipe_win";
    return true;
}

// AVG_WIN_PERIOD > 0 on a continuation launch (K > 64) of the fp32 fold: windowed too, which the
// product never does (k_fedavg_pipe_win's INIT = false instantiation)
template <typename Y, typename X, class CP, int E, int S, bool NT, bool LT, int BLK, int NTS, int MAP>
bool probe_avg_window_cont(X* a, const ClientTable<typename CP::S>& tab, int cnt, int64_t P, bool first, bool int_first,
                           dim3 grid, hipStream_t st) {
    if constexpr (std::is_same<CP, CF32>::value && std::is_same<X, float>::value && S * E * (int)sizeof(Y) == 64 &&
                  BLK == kBlock && MAP == 0 && !LT && !NT && NTS == 1) {
        if (g_cfg.avg_win_period > 0 && g_cfg.avg_win_mode != 3 && !int_first && !first) {   // (mode 3: first launches only)
            const uint32_t wl = (uint32_t)g_cfg.avg_win_period.load(), ww = (uint32_t)g_cfg.avg_win_w.load();
            g_kernel = "k_fedavg_pipe_win";
            hipLaunchKernelGGL((k_fedavg_pipe_win<Y, X, CP, E, S, false, false, NT, LT, BLK, NTS, MAP>), grid, dim3(BLK), 0, st, a, tab,
                               cnt, P, wl, ww, g_cfg.avg_win_mode.load());
            return true;
        }
    }
    return false;
}

// The FedAvg geometry sweep (STRIPS, UNROLL, NT, LANETAB, BLOCK, NT_STORE, NARROW, AUTO_GEOM) of the
// fp32 / bf16 -> fp32 fold: false while every one of these knobs is at its default (the caller then
// makes the product's choice, launch_fedavg_default); otherwise launches the instantiated geometry,
// or 1 x 8 for a combination that is not instantiated. GRID is no part of this: launch_fedavg_pipe
// applies it to whichever pipelined geometry is chosen, the product's included.
template <typename Y, typename X, class CP, int E>
bool probe_fedavg_geometry(X* a, const ClientTable<typename CP::S>& tab, int cnt, int64_t P, bool first, bool int_first,
                           hipStream_t st) {
    const int block_log = g_cfg.block_log, strips = g_cfg.strips, unroll = g_cfg.unroll, nt = g_cfg.nt;
    const int lanetab = g_cfg.lanetab, nt_store = g_cfg.nt_store;
    const int key = (block_log == 9 ? 20000 : block_log == 10 ? 30000 : 0) + lanetab * 10000 + strips * 100 +
                    unroll * 2 + nt;
    constexpr bool narrowable = sizeof(Y) < sizeof(X) && E % 2 == 0;
    if (key == 4 * 100 + 0 && nt_store == 1) {
        if (g_cfg.auto_geom && (g_cfg.narrow || !narrowable)) return false;   // every knob at its default
        // NARROW 0 keeps the size rule; AUTO_GEOM 0 forces the pipelined kernel at every size
        if (g_cfg.auto_geom && !pipe_pays<Y>(P)) {
            launch_fedavg_small<Y, X, CP, E>(a, tab, cnt, P, first, int_first, st);
            return true;
        }
        if constexpr (narrowable) {
            if (g_cfg.narrow) {
                launch_fedavg_pipe<Y, X, CP, E / 2, 8, false, false, kBlock, 1, 0>(a, tab, cnt, P, first, int_first, st);
                return true;
            }
        }
    }
    switch (key) {
#define FA_GEOM(S_, U_, NT_) \
    case S_ * 100 + U_ * 2 + NT_: launch_fedavg_geom<Y, X, CP, E, S_, U_, NT_>(a, tab, cnt, P, first, int_first, st); return true;
#define FA_PIPE(KEY_, S_, NT_, LT_, BLK_) \
    case KEY_: launch_fedavg_pipe<Y, X, CP, E, S_, NT_, LT_, BLK_, 0, 0>(a, tab, cnt, P, first, int_first, st); return true;
        FA_GEOM(1, 4, 0) FA_GEOM(1, 8, 0) FA_GEOM(1, 16, 0) FA_GEOM(2, 4, 0) FA_GEOM(2, 8, 0) FA_GEOM(2, 16, 0)
        FA_GEOM(4, 1, 0) FA_GEOM(4, 2, 0) FA_GEOM(4, 4, 0) FA_GEOM(8, 1, 0) FA_GEOM(8, 2, 0) FA_GEOM(16, 1, 0)
        FA_GEOM(1, 8, 1) FA_GEOM(4, 2, 1) FA_GEOM(8, 1, 1)
        FA_PIPE(2 * 100 + 0, 2, false, false, kBlock)
        case 4 * 100 + 0:
            if (nt_store == 1) launch_fedavg_pipe<Y, X, CP, E, 4, false, false, kBlock, 1, 0>(a, tab, cnt, P, first, int_first, st);
            else if (nt_store == 2) launch_fedavg_pipe<Y, X, CP, E, 4, false, false, kBlock, 2, 0>(a, tab, cnt, P, first, int_first, st);
            else launch_fedavg_pipe<Y, X, CP, E, 4, false, false, kBlock, 0, 0>(a, tab, cnt, P, first, int_first, st);
            return true;
        FA_PIPE(8 * 100 + 0, 8, false, false, kBlock)
        FA_PIPE(4 * 100 + 1, 4, true, false, kBlock)
        FA_PIPE(20000 + 4 * 100 + 0, 4, false, false, 512)
        FA_PIPE(30000 + 4 * 100 + 0, 4, false, false, 1024)
        FA_PIPE(20000 + 8 * 100 + 0, 8, false, false, 512)
        FA_PIPE(30000 + 2 * 100 + 0, 2, false, false, 1024)
        FA_PIPE(10000 + 2 * 100 + 0, 2, false, true, kBlock)
        FA_PIPE(10000 + 4 * 100 + 0, 4, false, true, kBlock)
        FA_PIPE(10000 + 8 * 100 + 0, 8, false, true, kBlock)
#undef FA_PIPE
#undef FA_GEOM
        default: break;
    }
    launch_fedavg_geom<Y, X, CP, E, 1, kUnroll, false>(a, tab, cnt, P, first, int_first, st);
    return true;
}

// FedOpt launches of the vector path (E = 4) that replace the product step: the access-pattern
// probes of a FIRST | FINAL launch (OPT_MIX, and OPT_WIN_PERIOD > 0 without OPT_WIN_PROD:
// k_fedopt_mixw) — instantiated for the configs[3] shapes only, fp32 updates over an fp32 or fp64
// model — and the store window on a first or middle launch of a multi-launch round (OPT_WIN_PERIOD
// > 0 with OPT_WIN_PROD: k_fedopt_cwp, every dtype). True: launched, or refused, with the status in rc.
template <typename Y, typename OLD, class PG, bool NT>
bool probe_fedopt_launch(const OptBuffers& b, const OptScalars& s, const ClientTable<typename PG::S>& tab, int cnt, int64_t P,
                         bool first, bool final_, dim3 g4, hipStream_t st, int& rc) {
    constexpr bool probe_combo = std::is_same<Y, float>::value && (std::is_same<OLD, float>::value || std::is_same<OLD, double>::value);
    const int period = g_cfg.opt_win_period, prod = g_cfg.opt_win_prod;
    if constexpr (probe_combo) {                         // (g4: a ragged last tile is skipped)
        if (first && final_ && period > 0 && !prod) {
            if (b.m_out_f64 != 1) {
                rc = fail(FA_EINVAL, "fa_tune OPT_WIN probe: fp64 m out");
                return true;
            }
            hipLaunchKernelGGL((k_fedopt_mixw<Y, OLD, typename PG::S, NT>), g4, dim3(kBlock), 0, st, b, tab, cnt, P, (uint32_t)period,
                               (uint32_t)g_cfg.opt_win_w.load(), g_cfg.opt_win_mode.load());
            rc = check_launch("fa_fedopt_step: kernel launch");
            return true;
        }
        if (first && final_ && g_cfg.opt_mix) {
            hipLaunchKernelGGL((k_fedopt_mix<Y, OLD, typename PG::S, NT>), g4, dim3(kBlock), 0, st, b, tab, cnt, P);
            rc = check_launch("fa_fedopt_step: kernel launch");
            return true;
        }
    }
    if (!final_ && period > 0 && prod) {
        const uint32_t w = (uint32_t)g_cfg.opt_win_w.load();
        if (first)
            hipLaunchKernelGGL((k_fedopt_cwp<Y, OLD, PG, true, NT>), g4, dim3(kBlock), 0, st, b, s, tab, cnt, P, (uint32_t)period, w);
        else
            hipLaunchKernelGGL((k_fedopt_cwp<Y, OLD, PG, false, NT>), g4, dim3(kBlock), 0, st, b, s, tab, cnt, P, (uint32_t)period, w);
        rc = check_launch("fa_fedopt_step: kernel launch");
        return true;
    }
    return false;
}

// OPT_WIN_PERIOD on the product's single-launch step (k_fedopt_cw): -1 = no window, > 0 with
// OPT_WIN_PROD = this one
void probe_opt_window(StoreWindow& sw) {
    const int period = g_cfg.opt_win_period;
    if (period < 0) sw = StoreWindow{};
    else if (period > 0 && g_cfg.opt_win_prod) sw = StoreWindow{(uint32_t)period, (uint32_t)g_cfg.opt_win_w.load()};
}

#else  // the product: its measured-best settings as constants, and hooks that leave every choice alone

constexpr int cfg_fastdiv() { return 1; }     // fp32 t/N via the exact RN64(1/N) product
constexpr int cfg_fastdiv64() { return 1; }   // fp64 t/N via RN64(1/N) + two exact corrections (§3.2b)
constexpr int cfg_grid_per_cu() { return 0; } // one 16-KiB-per-client tile per workgroup

inline void probe_avg_window(AvgWindow&, int&) {}
inline void probe_opt_window(StoreWindow&) {}
template <typename Y, typename X, class CP, int E, int S, int BLK, int NTS, class... A>
constexpr bool probe_fedavg_park(A&&...) { return false; }
template <typename Y, typename X, class CP, int E, int S, bool NT, bool LT, int BLK, int NTS, int MAP, class... A>
constexpr bool probe_avg_window_cont(A&&...) { return false; }
template <typename Y, typename X, class CP, int E, class... A>
constexpr bool probe_fedavg_geometry(A&&...) { return false; }
template <typename Y, typename OLD, class PG, bool NT, class... A>
constexpr bool probe_fedopt_launch(A&&...) { return false; }

#endif
