// fedopt_launch.h — launch policy of the FedOpt step: the store window of a single-launch step
// (opt_store_window), the kernel for one launch (launch_fedopt_one) and the chunking of K > 64 clients
// (launch_fedopt), which fa_fedopt_step_ex dispatches to by dtype pair.
//
// Included by fedagg.hip inside its anonymous namespace, after fedopt_kernels.h, probes.h (the probe_*
// hooks: inert in the product) and host_common.h. DESIGN.md §3.3 has the measurements behind each choice.

// The chip-wide store window of a single-launch FedOpt step (k_fedopt_cw), in 10-ns ticks of the
// reference clock, from the time one round of resident waves takes to stream its tiles at 6.4 TB/s
// (periods past ~1.5 rounds leave waves waiting for their window: 1.3-2x slower). Measured
// (profiles/r05_fedopt_window_product.log, 350 M params, every variant bit-exact):
//  - a launch that reads no optimizer state (a session's first round): period 0.65 round, window the
//    write share + 15 % of it: -8...-11 % at K = 32-64, -4...-5 % at K = 16;
//  - one that reads m and v (the steady state): period 0.35 round, window 15 %: -4...-9 % at K = 32,
//    -8...-10 % at K = 48 and 64 — but slower at K = 16 at every period tried, so only K >= 32.
// {0, 0}: no window — under 8 clients (under 32 with state), models under 2^24 elements, write
// shares over 25 %.
template <typename Y, typename OLD, class PG, bool NT>
StoreWindow opt_store_window(const OptBuffers& b, int K, int64_t P) {
    const bool state = b.m_in_f64 >= 0 || b.v_in;
    if (K < (state ? 32 : 8) || P < ((int64_t)1 << 24)) return {};
    const int nb = resident_blocks<k_fedopt_cw<Y, OLD, PG, NT>, kBlock>();
    if (nb <= 0) return {};
    const double waves = (double)nb * (kBlock / 64) * device_cus();
    const double m_in = b.m_in_f64 == 1 ? 8 : b.m_in_f64 == 0 ? 4 : b.m_in_f64 < 0 ? 0 : 2;
    const double m_out = b.m_out_f64 == 1 ? 8 : b.m_out_f64 == 0 ? 4 : 2;
    const double rd = (double)K * sizeof(Y) + sizeof(OLD) + m_in + (b.v_in ? (b.v_in_f32 ? 4 : 8) : 0);
    const double wr = (b.out_f32 ? 4 : 8) + (b.v_out_f32 ? 4 : 8) + m_out;
    const double frac = wr / (rd + wr);
    if (frac > 0.25) return {};
    const double period = (state ? 0.35 : 0.65) * waves * 512.0 * (rd + wr) / 6.4e12 * 1e8;
    if (period < 1000 || period > 20000) return {};
    StoreWindow sw;
    sw.period = (uint32_t)period;
    sw.w = (uint32_t)(period * (state ? 0.15 : std::min(0.30, std::max(0.08, 1.15 * frac))));
    return sw;
}

template <typename Y, typename OLD, class PG, int E, bool NT>
int launch_fedopt_one(const OptBuffers& b, const OptScalars& s, const ClientTable<typename PG::S>& tab, int cnt,
                      int64_t P, bool first, bool final_, hipStream_t st) {
    g_kernel = E == 4 ? "k_fedopt_c" : "k_fedopt";
    const dim3 grid((unsigned)grid_for(P, E));
    if constexpr (E == 4) {
        // wave-coalesced element map, 4 pairs per lane (512-element wave tiles), non-temporal state /
        // model stores: +3-6 % over the per-lane strip map on configs[3], bit-identical
        // (profiles/r02_fedopt_coal_*.log); every vector-path update dtype (bf16 /
        // fp16 updates: one dword per pair)
        const dim3 g4((unsigned)((P + 4 * 512 - 1) / (4 * 512)));
        int prc = FA_OK;
        if (probe_fedopt_launch<Y, OLD, PG, NT>(b, s, tab, cnt, P, first, final_, g4, st, prc)) return prc;
        if (first && final_) {
            StoreWindow sw = opt_store_window<Y, OLD, PG, NT>(b, cnt, P);
            probe_opt_window(sw);
            if (sw.period) {
                g_kernel = "k_fedopt_cw";
                hipLaunchKernelGGL((k_fedopt_cw<Y, OLD, PG, NT>), g4, dim3(kBlock), 0, st, b, s, tab, cnt, P, sw.period, sw.w);
                return check_launch("fa_fedopt_step: kernel launch");
            }
        }
        if (first && final_) hipLaunchKernelGGL((k_fedopt_c<Y, OLD, PG, true, true, NT, 1, 4>), g4, dim3(kBlock), 0, st, b, s, tab, cnt, P);
        else if (first) hipLaunchKernelGGL((k_fedopt_c<Y, OLD, PG, true, false, NT, 1, 4>), g4, dim3(kBlock), 0, st, b, s, tab, cnt, P);
        else if (final_) hipLaunchKernelGGL((k_fedopt_c<Y, OLD, PG, false, true, NT, 1, 4>), g4, dim3(kBlock), 0, st, b, s, tab, cnt, P);
        else hipLaunchKernelGGL((k_fedopt_c<Y, OLD, PG, false, false, NT, 1, 4>), g4, dim3(kBlock), 0, st, b, s, tab, cnt, P);
    } else {
        if (first && final_) hipLaunchKernelGGL((k_fedopt<Y, OLD, PG, E, true, true, NT>), grid, dim3(kBlock), 0, st, b, s, tab, cnt, P);
        else if (first) hipLaunchKernelGGL((k_fedopt<Y, OLD, PG, E, true, false, NT>), grid, dim3(kBlock), 0, st, b, s, tab, cnt, P);
        else if (final_) hipLaunchKernelGGL((k_fedopt<Y, OLD, PG, E, false, true, NT>), grid, dim3(kBlock), 0, st, b, s, tab, cnt, P);
        else hipLaunchKernelGGL((k_fedopt<Y, OLD, PG, E, false, false, NT>), grid, dim3(kBlock), 0, st, b, s, tab, cnt, P);
    }
    return check_launch("fa_fedopt_step: kernel launch");
}

template <typename Y, typename OLD, class PG>
int launch_fedopt(const OptBuffers& b, const OptScalars& s, const void* const* ups, const double* n, const double* N,
                  int K, int64_t P, int flags, hipStream_t st) {
    bool vec = aligned16(b.old) && aligned16(b.pg) && aligned16(b.m_in) && aligned16(b.m_out) && aligned16(b.v_in) &&
               aligned16(b.v_out) && aligned16(b.out);
    for (int k = 0; k < K && vec; ++k) vec = aligned16(ups[k]);
    using S = typename PG::S;
    ClientTable<S> tab;
    bool first = (flags & FA_PG_FIRST) != 0;
    const bool final_all = (flags & FA_PG_FINAL) != 0;
    int k0 = 0;
    do {
        const int cnt = (K - k0) < kMaxK ? (K - k0) : kMaxK;
        fill_table<S>(tab, ups, n, N, k0, cnt, std::is_same<PG, CF16>::value);
        const bool last = k0 + cnt >= K;
        const bool fin = last && final_all;
        int rc = vec ? launch_fedopt_one<Y, OLD, PG, 4, true>(b, s, tab, cnt, P, first, fin, st)
                     : launch_fedopt_one<Y, OLD, PG, 1, false>(b, s, tab, cnt, P, first, fin, st);
        if (rc) return rc;
        first = false;
        k0 += cnt;
    } while (k0 < K);
    return FA_OK;
}
