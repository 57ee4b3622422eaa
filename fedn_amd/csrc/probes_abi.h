// probes_abi.h — the entry points of the probe build only (include/fedagg_probe.h): the geometry
// queries of the robust kernels, fa_tune, and the stream probes fa_stream_sum / _copy / _read.
//
// Included by fedagg.hip inside its extern "C" block, in the probe build alone. It uses g_cfg and the
// probe kernels (probes.h), launch_fedavg_pipe (fedavg_launch.h), fill_table (host_common.h) and the
// geometry tables of pair_dist.h and wmean_dist.h (cclip.h's kernel uses the latter's). DESIGN.md §3.5 describes the stream probes.

int fa_pairwise_sqdist_geometry(int upd_dtype, int K, int* tile_elems, int* chain_terms, int* max_workgroups,
                                int* flush_tiles) {
    g_err[0] = 0;
    if (K < 1 || K > kMaxK) return fail(FA_EINVAL, "fa_pairwise_sqdist_geometry: K=%d outside 1..%d", K, kMaxK);
    if (!pair_family(upd_dtype)) return fail(FA_EDTYPE, "fa_pairwise_sqdist_geometry: unsupported dtype %d", upd_dtype);
    int te = 0, ft = 0;
    auto get = [&](auto gm) -> int {
        te = decltype(gm)::TE;
        ft = kPairChain / decltype(gm)::PER_TILE;
        return FA_OK;
    };
    if (pair_family(upd_dtype) == 64) pair_for_kp<double>(K, get);
    else pair_for_kp<float>(K, get);
    if (tile_elems) *tile_elems = te;
    if (chain_terms) *chain_terms = kPairChain;
    if (max_workgroups) *max_workgroups = kPairGrid;
    if (flush_tiles) *flush_tiles = ft;
    return FA_OK;
}

// the two fused-pass kernels' geometry at `cols` tile columns, in `who`'s name
static int wm_geometry(const char* who, int upd_dtype, int K, int cols, int* tile_elems, int* chain_terms,
                       int* max_workgroups, int* flush_tiles) {
    g_err[0] = 0;
    if (K < 1 || K > kMaxK) return fail(FA_EINVAL, "%s: K=%d outside 1..%d", who, K, kMaxK);
    if (!pair_family(upd_dtype)) return fail(FA_EDTYPE, "%s: unsupported dtype %d", who, upd_dtype);
    const WmGeom gm = wm_geom_dt(upd_dtype, K, cols);
    if (tile_elems) *tile_elems = gm.TE;
    if (chain_terms) *chain_terms = kWmChain;
    if (max_workgroups) *max_workgroups = gm.GRID;
    if (flush_tiles) *flush_tiles = gm.FT;
    return FA_OK;
}

int fa_wmean_sqdist_geometry(int upd_dtype, int K, int* tile_elems, int* chain_terms, int* max_workgroups,
                             int* flush_tiles) {
    return wm_geometry("fa_wmean_sqdist_geometry", upd_dtype, K, K, tile_elems, chain_terms, max_workgroups, flush_tiles);
}

int fa_centered_clip_geometry(int upd_dtype, int K, int* tile_elems, int* chain_terms, int* max_workgroups,
                              int* flush_tiles) {
    return wm_geometry("fa_centered_clip_geometry", upd_dtype, K, K + 1, tile_elems, chain_terms, max_workgroups,
                       flush_tiles);
}

int fa_tune(int knob, int value) {
    g_err[0] = 0;
    // one knob: v into its field where `ok`, else FA_EINVAL with the knob's range
    auto set = [](std::atomic<int>& field, int v, bool ok = true, const char* range = "") -> int {
        if (!ok) return fail(FA_EINVAL, "fa_tune: %s", range);
        field = v;
        return FA_OK;
    };
    auto among = [value](std::initializer_list<int> vs) { return std::find(vs.begin(), vs.end(), value) != vs.end(); };
    const int flag = value ? 1 : 0;
    const bool period_ok = value == 0 || value == -1 || (value >= 64 && value <= (1 << 24));
    const char* period = "store-window period 64 .. 2^24 ticks of 10 ns (0 = the product's own, -1 = none)";
    switch (knob) {
        case FA_TUNE_STRIPS: return set(g_cfg.strips, value, among({1, 2, 4, 8, 16}), "strips must be 1, 2, 4, 8 or 16");
        case FA_TUNE_UNROLL:
            return set(g_cfg.unroll, value, among({0, 1, 2, 4, 8, 16}), "unroll must be 0 (pipelined), 1, 2, 4, 8 or 16");
        case FA_TUNE_NT: return set(g_cfg.nt, flag);
        case FA_TUNE_SUM_NOSTORE: return set(g_cfg.sum_nostore, flag);
        case FA_TUNE_NT_STORE: return set(g_cfg.nt_store, value, value >= 0 && value <= 2, "store mode 0 (plain), 1 (nt) or 2 (sc1)");
        case FA_TUNE_BLOCK:
            return set(g_cfg.block_log, value == 256 ? 8 : value == 512 ? 9 : 10, among({256, 512, 1024}), "block 256, 512 or 1024");
        case FA_TUNE_READ: return set(g_cfg.read_per_lane, value, among({4, 8, 16}), "read probe depth 4, 8 or 16");
        case FA_TUNE_GRID: return set(g_cfg.grid_per_cu, value, value >= 0 && value <= 64, "grid blocks per CU must be 0..64");
        case FA_TUNE_LANETAB: return set(g_cfg.lanetab, flag);
        case FA_TUNE_FASTDIV: return set(g_cfg.fastdiv, flag);
        case FA_TUNE_FASTDIV64: return set(g_cfg.fastdiv64, flag);
        case FA_TUNE_NARROW: return set(g_cfg.narrow, flag);
        case FA_TUNE_AUTO_GEOM: return set(g_cfg.auto_geom, flag);
        case FA_TUNE_OPT_MIX: return set(g_cfg.opt_mix, flag);
        case FA_TUNE_OPT_WIN_PERIOD: return set(g_cfg.opt_win_period, value, period_ok, period);
        case FA_TUNE_OPT_WIN_W: return set(g_cfg.opt_win_w, value, value >= 0, "store-window length in ticks >= 0");
        case FA_TUNE_OPT_WIN_MODE: return set(g_cfg.opt_win_mode, value, value >= 0 && value <= 2, "store-window mode 0, 1 or 2");
        case FA_TUNE_OPT_WIN_PROD:
            return set(g_cfg.opt_win_prod, value, among({0, 1}), "OPT_WIN_PROD 0 (pattern probe) or 1 (k_fedopt_cw)");
        case FA_TUNE_AVG_WIN_PERIOD: return set(g_cfg.avg_win_period, value, period_ok, period);
        case FA_TUNE_AVG_WIN_W: return set(g_cfg.avg_win_w, value, value >= 0, "store-window length in ticks >= 0");
        case FA_TUNE_AVG_WIN_MODE:
            return set(g_cfg.avg_win_mode, value, value >= 0 && value <= 3, "store-window mode 0, 1, 2 or 3 (parked)");
        case FA_TUNE_AVG_PARK_DEPTH:
            return set(g_cfg.avg_park_depth, value, among({0, 2, 3, 4}), "parked ring depth 2, 3 or 4 (0 = the product's)");
        case FA_TUNE_AVG_PARK_SLOTS:
            return set(g_cfg.avg_park_slots, value, among({0, 1, 2, 4}), "parked tiles per workgroup 1, 2 or 4 (0 = the product's)");
        case FA_TUNE_AVG_PARK_HEIGHT:
            return set(g_cfg.avg_park_height, value, among({0, 1, 2, 4}), "parked tile height 1, 2 or 4 (0 = the product's)");
        case FA_TUNE_AVG_PARK_LOADPOL:
            return set(g_cfg.avg_park_loadpol, value, value >= 0 && value <= 3, "ring load policy 0 (default), 1 (nt), 2 (sc1) or 3 (sc1 nt)");
        default: return fail(FA_EINVAL, "fa_tune: unknown knob %d", knob);
    }
}

int fa_stream_sum(float* out, const float* const* bufs, int K, int64_t P, void* stream) {
    g_err[0] = 0;
    if (K < 1 || K > kMaxK || P < 0 || !out || !bufs) return fail(FA_EINVAL, "fa_stream_sum: bad arguments");
    bool vec = aligned16(out);
    for (int k = 0; k < K; ++k) vec = vec && bufs[k] && aligned16(bufs[k]);
    if (!vec) return fail(FA_EINVAL, "fa_stream_sum: buffers must be 16-B aligned");
    ClientTable<float> tab;
    std::vector<double> ones(K, 1.0);
    fill_table<float>(tab, reinterpret_cast<const void* const*>(bufs), ones.data(), ones.data(), 0, K);
    if (g_cfg.sum_nostore)
        launch_fedavg_pipe<float, float, CADDNW, 4, 4, false, false, kBlock, 0, 0>(out, tab, K, P, true, false, static_cast<hipStream_t>(stream));
    else if (g_cfg.nt_store == 1)
        launch_fedavg_pipe<float, float, CADD, 4, 4, false, false, kBlock, 1, 0>(out, tab, K, P, true, false, static_cast<hipStream_t>(stream));
    else if (g_cfg.nt_store == 2)
        launch_fedavg_pipe<float, float, CADD, 4, 4, false, false, kBlock, 2, 0>(out, tab, K, P, true, false, static_cast<hipStream_t>(stream));
    else
        launch_fedavg_pipe<float, float, CADD, 4, 4, false, false, kBlock, 0, 0>(out, tab, K, P, true, false, static_cast<hipStream_t>(stream));
    return check_launch("fa_stream_sum");
}

int fa_stream_copy(void* dst, const void* src, int64_t bytes, void* stream) {
    g_err[0] = 0;
    if (bytes < 0 || (bytes & 15) || !aligned16(dst) || !aligned16(src))
        return fail(FA_EINVAL, "fa_stream_copy: bytes must be a multiple of 16 and buffers 16-B aligned");
    const int64_t n16 = bytes / 16;
    if (!n16) return FA_OK;
    hipLaunchKernelGGL(k_stream_copy, dim3((unsigned)((n16 + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                       static_cast<hipStream_t>(stream), static_cast<u32x4*>(dst), static_cast<const u32x4*>(src), n16);
    return check_launch("fa_stream_copy");
}

int64_t fa_stream_read_blocks(int64_t bytes) {
    const int64_t n16 = bytes / 16;
    const int64_t per = (int64_t)kBlock * kReadPerLane;
    return (n16 + per - 1) / per;
}

int fa_stream_read(const void* src, int64_t bytes, void* sink, void* stream) {
    g_err[0] = 0;
    if (bytes < 0 || (bytes & 15) || !aligned16(src) || !aligned16(sink))
        return fail(FA_EINVAL, "fa_stream_read: bytes must be a multiple of 16 and buffers 16-B aligned");
    const int64_t blocks = fa_stream_read_blocks(bytes);
    if (!blocks) return FA_OK;
    const int64_t n16 = bytes / 16;
    const dim3 blk(kBlock);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const u32x4* s4 = static_cast<const u32x4*>(src);
    u32x4* k4 = static_cast<u32x4*>(sink);
    // loads in flight per lane (fa_tune FA_TUNE_READ: 4, 8 or 16)
    switch (g_cfg.read_per_lane) {
        case 4: hipLaunchKernelGGL(k_stream_read<4>, dim3((unsigned)((n16 + kBlock * 4 - 1) / (kBlock * 4))), blk, 0, st, s4, n16, k4); break;
        case 8: hipLaunchKernelGGL(k_stream_read<8>, dim3((unsigned)((n16 + kBlock * 8 - 1) / (kBlock * 8))), blk, 0, st, s4, n16, k4); break;
        default: hipLaunchKernelGGL(k_stream_read<16>, dim3((unsigned)blocks), blk, 0, st, s4, n16, k4); break;
    }
    return check_launch("fa_stream_read");
}
