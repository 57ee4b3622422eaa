// fedavg_launch.h — launch policy of the FedAvg fold: the store window and the parked grid of a first
// launch (avg_store_window, avg_park_grid), the geometry by model size (launch_fedavg_small / _pipe /
// _default / _vec) and the chunking of K > 64 clients (launch_fedavg), which fa_fedavg_fold,
// fa_weighted_sum and fa_running_mean dispatch to.
//
// Included by fedagg.hip inside its anonymous namespace, after fedavg_kernels.h, probes.h (the cfg_*
// getters and probe_* hooks: constants and inert stubs in the product) and host_common.h. DESIGN.md
// §3.2 and §4 have the measurements behind each choice.

// Mode 3 (parked stores, fedavg_park_body) is instantiated for the fp32 geometry's first launch
template <typename Y, typename X, class CP, int E, int S, bool NT, bool LT, int BLK, int NTS, int MAP>
constexpr bool avg_park_geometry = std::is_same<CP, CF32>::value && std::is_same<X, float>::value &&
                                   std::is_same<Y, float>::value && S * E == 16 && BLK == kBlock && MAP == 0 && !LT && !NT;

// Its grid: kAvgParkPerCu workgroups per CU where the occupancy query allows them (per_cu > 0: that
// many instead), at most one per tall or tail tile (ParkPartition::units). Its waves never idle and keep the ring's loads in flight
// behind every consume, and more tile streams than that needs only crowd the memory system: at
// 64 x 100 M and 2 ring buffers, 1 per CU -0.9...-1.4 % against the round-7 kernel at its own 2 per
// CU, 2 per CU +1.4...+1.7 %, 3 per CU +4 % and more; 3 or 4 ring buffers +1.7...+6 % at every
// grid (profiles/r08_ring_sweep.log; the round-7 kernel, whose address arithmetic drained its ring
// before every load: profiles/r07_park_sweep.log). With tall tiles and nt loads, 2 per CU is still
// +2 % (profiles/r09_height_sweep.log).
constexpr int kAvgParkPerCu = 1;
template <auto KERNEL, int BLK>
int64_t avg_park_grid(int64_t ntiles, int per_cu) {
    const int nb = per_cu > 0 ? per_cu : std::min(std::max(resident_blocks<KERNEL, BLK>(), 1), kAvgParkPerCu);
    return std::max<int64_t>(1, std::min<int64_t>(ntiles, (int64_t)nb * device_cus()));
}

// One parked launch of the product's kernel (the PARK instantiation of k_fedavg_pipe_win).
template <typename Y, typename X, class CP, int E, int S, bool NT, bool LT, int BLK, int NTS, int MAP>
void launch_fedavg_park(X* a, const ClientTable<typename CP::S>& tab, int cnt, int64_t P, uint32_t period, uint32_t win_w,
                        int per_cu, hipStream_t st) {
    constexpr int64_t kTile = (int64_t)BLK * S * E;
    constexpr auto kernel = k_fedavg_pipe_win<Y, X, CP, E, S, true, false, NT, LT, BLK, NTS, MAP, true>;
    const dim3 pgrid((unsigned)avg_park_grid<kernel, BLK>(park_partition(P, kTile, kAvgParkHeight).units(), per_cu));
    g_kernel = "k_fedavg_pipe_win";
    hipLaunchKernelGGL(kernel, pgrid, dim3(BLK), 0, st, a, tab, cnt, P, period, win_w, 3);
}

// The store window of a first FedAvg launch (k_fedavg_pipe_win), in 10-ns ticks of the reference
// clock: period 0.45 of the time one round of resident workgroups streams its tiles at 6.4 TB/s,
// window 15 % — measured (profiles/r05_fedavg_window.log, 100 M fp32, bit-exact, two boxes) at
// K = 64: 0.24-0.47 round -5...-7 %, 0.6 round and longer +2...+22 %; K = 8: 0.34-0.42 round -6 %,
// 0.64 round 0 %; bf16 updates at K = 64 -5 %, at K = 8 (a 20 % write share) +4 %. {0, 0}: no window
// (write shares over 15 %, models under 2^24 elements, periods under 500 ticks).
template <typename Y, typename X, class CP, int E, int S, bool NT, bool LT, int BLK, int NTS, int MAP>
AvgWindow avg_store_window(int K, int64_t P) {
    if (P < ((int64_t)1 << 24) || K < 2) return {};
    const int nb = resident_blocks<k_fedavg_pipe_win<Y, X, CP, E, S, true, false, NT, LT, BLK, NTS, MAP>, BLK>();
    if (nb <= 0) return {};
    if ((double)sizeof(X) / ((double)K * sizeof(Y) + sizeof(X)) > 0.15) return {};
    const double round_bytes = (double)nb * device_cus() * BLK * S * E * ((double)K * sizeof(Y) + sizeof(X));
    const double period = 0.45 * round_bytes / 6.4e12 * 1e8;
    if (period < 500 || period > 20000) return {};
    AvgWindow w;
    w.period = (uint32_t)period;
    w.w = (uint32_t)(0.15 * period);
    // Parked stores (mode 3), where a wait for the window costs no reading: from 32 fp32 clients (a
    // write share <= 3 %), kAvgParkDepth ring buffers, kAvgParkSlots parked tiles, period 0.7 of the
    // round of ITS resident workgroups, window 8 % — measured (profiles/r08_ring_sweep.log, 100 M
    // fp32, every point bit-exact) at K = 64: -1.1 % against the round-7 kernel's 2 per CU at the same
    // period and window rule (1 slot -0.9 %; 4 slots at 2.8 rounds and a 4 % window -1.4 %: both
    // within the session's noise of this one), K = 48 -1.6 %, K = 32 -2.6 % against mode 0 above.
    // K = 16 0 %, K = 8 +4 % with the round-7 kernel (profiles/r07_park_sweep.log): those keep mode 0.
    // Tall tiles and non-temporal ring loads (kAvgParkHeight 2, kAvgParkLoadPol nt; the period is that
    // of a round of tall tiles) — measured (profiles/r09_height_sweep.log, one process, every point
    // bit-exact) at K = 64 x 100 M against height 1 / default policy / 2 slots: nt alone -7.0 %, height
    // 2 alone -0.6 %, both -9.9 % (1 or 2 slots, nt or sc1 nt: within 0.2 % of each other; sc1 alone
    // 0 %; height 4 nt -9.4 %, without nt +4.7 %; a 4 % window +2...+7 % on the 8 % one; 2 workgroups
    // per CU +2 % on 1). Height 2, 1 slot, sc1 nt at K = 48 -9.5 %, K = 32 -4.7 %, and at the smallest
    // pipelined model (160 MiB per client, K = 64, 5 tall tiles per workgroup) -9.4 %: no K or size at
    // which height 1 wins, so there is no gate. 2 slots rather than 1: the same at the 8 % window and
    // 4.7 % faster at the 4 % one, where a wave meets a closed window more often. The gain depends on
    // the box: on two others the same setting was -4.1 and -5.0 % (nt alone -2.4 and -3.2 %), and plain
    // bench.py against the parent commit -3.6 % at K = 64, -4.5 % at K = 48, -4.4 % at K = 32, -4.6 % at
    // 160 MiB per client (profiles/r09_height_pairs.log).
    if constexpr (avg_park_geometry<Y, X, CP, E, S, NT, LT, BLK, NTS, MAP>) {
        const double pperiod = 0.7 * period / 0.45 * kAvgParkPerCu / nb * kAvgParkHeight;   // a round of tall tiles
        if (K >= 32 && pperiod >= 500 && pperiod <= 20000) {
            w.period = (uint32_t)pperiod;
            w.w = (uint32_t)(0.08 * pperiod);
            w.mode = 3;
        }
    }
    return w;
}

template <typename Y, typename X, class CP, int E, int S, int U, bool NT>
void launch_fedavg_geom(X* a, const ClientTable<typename CP::S>& tab, int cnt, int64_t P, bool first, bool int_first,
                        hipStream_t st) {
    g_kernel = "k_fedavg";
    const int64_t strips = (P + E - 1) / E;
    const dim3 grid((unsigned)((strips + (int64_t)kBlock * S - 1) / ((int64_t)kBlock * S)));
    if (first && int_first) {
        if constexpr (std::is_integral<Y>::value)
            hipLaunchKernelGGL((k_fedavg<Y, X, CP, E, S, U, true, true, NT>), grid, dim3(kBlock), 0, st, a, tab, cnt, P);
    } else if (first)
        hipLaunchKernelGGL((k_fedavg<Y, X, CP, E, S, U, true, false, NT>), grid, dim3(kBlock), 0, st, a, tab, cnt, P);
    else
        hipLaunchKernelGGL((k_fedavg<Y, X, CP, E, S, U, false, false, NT>), grid, dim3(kBlock), 0, st, a, tab, cnt, P);
}

// Launch geometry by model size (profiles/r02_tile_probe.log). Every workgroup folds all K
// clients over one tile, so the grid must be many times the ~1,024 resident workgroups or its
// last partial wave decides the time. The pipelined 4-strip kernel (16 KiB of each client per
// tile) is the fastest once each client buffer is >= kPipeMinClientBytes (>= 10 K tiles: 0.74-0.75
// of peak at 64 x 100 M fp32 and bf16); below that, one 16-B strip per lane with 4 (fp32) or 8
// (narrower types, or K <= 8) clients loaded ahead — 4 KiB tiles — holds 0.65-0.80 where the
// 4-strip tiles drop to 0.25-0.55 (bf16 10 M: 0.27 -> 0.65; fp32 3 M x 64: 0.45 -> 0.67).
constexpr int64_t kPipeMinClientBytes = 160ll << 20;

template <typename Y>
inline bool pipe_pays(int64_t P) { return P * (int64_t)sizeof(Y) >= kPipeMinClientBytes; }

template <class CP> struct is_sf_rule : std::false_type {};
template <typename Y, typename X> struct is_sf_rule<CWSUM<Y, X>> : std::true_type {};
template <typename T_> struct is_sf_rule<CRUN<T_>> : std::true_type {};

template <typename Y, typename X, class CP, int E>
void launch_fedavg_small(X* a, const ClientTable<typename CP::S>& tab, int cnt, int64_t P, bool first, bool int_first,
                         hipStream_t st) {
    if (sizeof(Y) < 4 || cnt <= 8) launch_fedavg_geom<Y, X, CP, E, 1, 8, false>(a, tab, cnt, P, first, int_first, st);
    else launch_fedavg_geom<Y, X, CP, E, 1, 4, false>(a, tab, cnt, P, first, int_first, st);
}

template <typename Y, typename X, class CP, int E, int S, bool NT, bool LT, int BLK, int NTS, int MAP>
void launch_fedavg_pipe(X* a, const ClientTable<typename CP::S>& tab, int cnt, int64_t P, bool first, bool int_first,
                        hipStream_t st) {
    g_kernel = "k_fedavg_pipe";
    const int64_t strips = (P + E - 1) / E;
    int64_t ntiles = (strips + (int64_t)BLK * S - 1) / ((int64_t)BLK * S);
    if (cfg_grid_per_cu() > 0) {
        if constexpr (MAP != 0) return launch_fedavg_pipe<Y, X, CP, E, S, NT, LT, BLK, NTS, 0>(a, tab, cnt, P, first, int_first, st);
        ntiles = std::min<int64_t>(ntiles, (int64_t)cfg_grid_per_cu() * device_cus());
    }
    const dim3 grid((unsigned)ntiles);
    // the fp32 fold with a first launch (the BASELINE workload's shape): its stores in the chip-wide
    // window; other dtypes / continuation launches were not measured with one
    if constexpr (std::is_same<CP, CF32>::value && std::is_same<X, float>::value &&
                  ((std::is_same<Y, float>::value && S * E == 16) || (std::is_same<Y, bf16>::value && S * E == 32)) &&
                  BLK == kBlock && MAP == 0 && !LT && !NT && NTS == 1) {
        if (first && !int_first) {
            AvgWindow w = avg_store_window<Y, X, CP, E, S, NT, LT, BLK, NTS, MAP>(cnt, P);
            int wm = w.mode;
            probe_avg_window(w, wm);
            // mode 3 (parked stores): its own grid, the resident workgroups (fa_tune GRID n: n per CU)
            if constexpr (avg_park_geometry<Y, X, CP, E, S, NT, LT, BLK, NTS, MAP>) {
                if (w.period && wm == 3) {
                    if (probe_fedavg_park<Y, X, CP, E, S, BLK, NTS>(a, tab, cnt, P, w.period, w.w, st)) return;
                    launch_fedavg_park<Y, X, CP, E, S, NT, LT, BLK, NTS, MAP>(a, tab, cnt, P, w.period, w.w, cfg_grid_per_cu(), st);
                    return;
                }
            }
            if (wm == 3) wm = 0;                         // not instantiated for this geometry
            if (w.period && cfg_grid_per_cu() == 0) {
                g_kernel = "k_fedavg_pipe_win";
                hipLaunchKernelGGL((k_fedavg_pipe_win<Y, X, CP, E, S, true, false, NT, LT, BLK, NTS, MAP>), grid, dim3(BLK), 0, st, a,
                                   tab, cnt, P, w.period, w.w, wm);
                return;
            }
        }
    }
    if (probe_avg_window_cont<Y, X, CP, E, S, NT, LT, BLK, NTS, MAP>(a, tab, cnt, P, first, int_first, grid, st)) return;
    if (first && int_first) {
        if constexpr (std::is_integral<Y>::value)
            hipLaunchKernelGGL((k_fedavg_pipe<Y, X, CP, E, S, true, true, NT, LT, BLK, NTS, MAP>), grid, dim3(BLK), 0, st, a, tab, cnt, P);
    } else if (first)
        hipLaunchKernelGGL((k_fedavg_pipe<Y, X, CP, E, S, true, false, NT, LT, BLK, NTS, MAP>), grid, dim3(BLK), 0, st, a, tab, cnt, P);
    else
        hipLaunchKernelGGL((k_fedavg_pipe<Y, X, CP, E, S, false, false, NT, LT, BLK, NTS, MAP>), grid, dim3(BLK), 0, st, a, tab, cnt, P);
}

// The product's geometry for the fp32 hot path (fp32 / bf16 updates into an fp32 aggregate), both builds.
template <typename Y, typename X, class CP, int E>
void launch_fedavg_default(X* a, const ClientTable<typename CP::S>& tab, int cnt, int64_t P, bool first, bool int_first,
                           hipStream_t st) {
    if (!pipe_pays<Y>(P)) return launch_fedavg_small<Y, X, CP, E>(a, tab, cnt, P, first, int_first, st);
    // measured best on MI355X (profiles/r01_microbench.md): 4 x 16-B strips per lane, the next
    // client's strips in flight (pipelined), cached loads, non-temporal aggregate stores.
    // bf16 clients: strips of 4 elements (8-B loads, 16-B f32 stores), 8 per lane, so every wave
    // store is one contiguous 1 KiB — +3.5 % at K = 64, +7 % at K = 8 (profiles/r02_narrow_probe.log)
    if constexpr (sizeof(Y) < sizeof(X) && E % 2 == 0)
        return launch_fedavg_pipe<Y, X, CP, E / 2, 8, false, false, kBlock, 1, 0>(a, tab, cnt, P, first, int_first, st);
    else
        return launch_fedavg_pipe<Y, X, CP, E, 4, false, false, kBlock, 1, 0>(a, tab, cnt, P, first, int_first, st);
}

// The tunable geometries (probe build) are instantiated for the fp32 hot path only; other dtypes use the default.
template <typename Y, typename X, class CP, int E>
void launch_fedavg_vec(X* a, const ClientTable<typename CP::S>& tab, int cnt, int64_t P, bool first, bool int_first,
                       hipStream_t st) {
    constexpr bool tunable = (std::is_same<Y, float>::value || std::is_same<Y, bf16>::value) && std::is_same<X, float>::value &&
                             std::is_same<CP, CF32>::value;
    if constexpr (is_sf_rule<CP>::value) {
        if (!pipe_pays<Y>(P)) return launch_fedavg_small<Y, X, CP, E>(a, tab, cnt, P, first, int_first, st);
        launch_fedavg_pipe<Y, X, CP, E, 4, false, false, kBlock, 0, 0>(a, tab, cnt, P, first, int_first, st);
        return;
    }
    if constexpr (tunable) {
        if (probe_fedavg_geometry<Y, X, CP, E>(a, tab, cnt, P, first, int_first, st)) return;
        return launch_fedavg_default<Y, X, CP, E>(a, tab, cnt, P, first, int_first, st);
    }
    launch_fedavg_geom<Y, X, CP, E, 1, kUnroll, false>(a, tab, cnt, P, first, int_first, st);
}

template <typename Y, typename X, class CP>
int launch_fedavg(void* agg, const void* const* ups, const double* n, const double* N, int K, int64_t P,
                  int init, bool int_first, hipStream_t st) {
    constexpr int E16 = 16 / (int)sizeof(Y) > 0 ? 16 / (int)sizeof(Y) : 1;
    bool vec = aligned16(agg);
    for (int k = 0; k < K && vec; ++k) vec = aligned16(ups[k]);
    using S = typename CP::S;
    ClientTable<S> tab;
    int k0 = 0;
    bool first = init != 0;
    X* a = static_cast<X*>(agg);
    while (k0 < K) {
        const int cnt = (K - k0) < kMaxK ? (K - k0) : kMaxK;
        fill_table<S>(tab, ups, n, N, k0, cnt, std::is_same<CP, CF16>::value);
        if (vec) launch_fedavg_vec<Y, X, CP, E16>(a, tab, cnt, P, first, int_first, st);
        else launch_fedavg_geom<Y, X, CP, 1, 1, kUnroll, false>(a, tab, cnt, P, first, int_first, st);
        int rc = check_launch("fa_fedavg_fold: kernel launch");
        if (rc) return rc;
        first = false;
        k0 += cnt;
    }
    return FA_OK;
}
