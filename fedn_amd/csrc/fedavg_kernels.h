// fedavg_kernels.h — the FedAvg fold x <- x + (n_k*(y_k - x))/N_k over K client buffers, device code:
// k_fedavg (U clients loaded ahead), k_fedavg_pipe (the next client in flight), k_fedavg_pipe_win (stores
// inside the chip-wide window, parked in LDS in mode 3) and k_fedavg_park (the parked fold at any depth).
// Included by fedagg.hip inside its anonymous namespace, after fold_rules.h, whose rules, strips, client
// table and window clock it uses. DESIGN.md §3.2 describes the fold, §3.3 the windows, §4 the tile order;
// fedavg_launch.h chooses among these kernels.

// Start one strip's running value. INIT: x := updates[0] (the `model = model_next`
// alias, fedavg.py:65-66); else x := agg (continuing a chunked / streamed fold).
// INT_FIRST: integer updates; the first fold runs in integer arithmetic (numpy int
// subtract + multiply wrap), then true_divide to f64 (numpyhelper.py:32 on int arrays).
// Returns the first client index still to fold.
template <typename Y, typename X, class CP, int E, bool INIT, bool INT_FIRST, bool NT>
__device__ __forceinline__ int strip_start(typename CP::V (&x)[E], const X* __restrict__ agg,
                                           const ClientTable<typename CP::S>& tab, int64_t i0, int rem) {
    using V = typename CP::V;
    if constexpr (INIT) {
        const Y* y0p = static_cast<const Y*>(tab.ptr[0]) + i0;
        Y y0[E];
        if (rem == E) strip_load<Y, E, NT>(y0p, y0);
        else {
#pragma unroll
            for (int e = 0; e < E; ++e) y0[e] = e < rem ? y0p[e] : Y{};
        }
        if constexpr (INT_FIRST) {
            const Y* y1p = static_cast<const Y*>(tab.ptr[1]) + i0;   // K >= 2 guaranteed by the host
            using U = typename std::make_unsigned<Y>::type;
            const U n1 = (U)(int64_t)tab.n[1];
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const Y y1 = e < rem ? y1p[e] : Y{};
                U t = (U)y1 - (U)y0[e];   // wrapping subtract
                t = n1 * t;               // wrapping multiply
                x[e] = (double)y0[e] + (double)(Y)t / (double)tab.N[1];
            }
            return 2;
        } else {
#pragma unroll
            for (int e = 0; e < E; ++e) x[e] = widen<Y, V>(y0[e]);
            return 1;
        }
    } else {
        X xa[E];
        if (rem == E) strip_load<X, E, false>(agg + i0, xa);
        else {
#pragma unroll
            for (int e = 0; e < E; ++e) xa[e] = e < rem ? agg[i0 + e] : X{};
        }
#pragma unroll
        for (int e = 0; e < E; ++e) x[e] = widen<X, V>(xa[e]);
        return 0;
    }
}

// The grid's last block: its strips may be ragged or past the end of the buffers.
template <typename Y, typename X, class CP, int E, int S, bool INIT, bool INT_FIRST, int BLK = kBlock>
__device__ __forceinline__ void k_fedavg_tail(X* __restrict__ agg, const ClientTable<typename CP::S>& tab, const int K,
                                           const int64_t P, const int64_t strip0) {
    using V = typename CP::V;
    for (int s = 0; s < S; ++s) {
        const int64_t i0 = (strip0 + s * BLK) * E;
        if (i0 >= P) break;
        const int rem = (P - i0) < E ? (int)(P - i0) : E;
        V x[E];
        int k = strip_start<Y, X, CP, E, INIT, INT_FIRST, false>(x, agg, tab, i0, rem);
        for (; k < K; ++k) {
            const Y* yp = static_cast<const Y*>(tab.ptr[k]) + i0;
            const typename CP::S n = tab.n[k], N = tab.N[k];
            const double r = tab.r[k];
            for (int e = 0; e < rem; ++e) x[e] = CP::fold(x[e], widen<Y, V>(yp[e]), n, N, r);
        }
        for (int e = 0; e < rem; ++e) agg[i0 + e] = narrow<X, V>(x[e]);
    }
}

// One lane owns S strips of E elements (strip s at lane + s*kBlock within the block's
// span, so every wave instruction stays a contiguous 1 KiB). U clients' strips are
// loaded before any of them is folded, so a lane keeps U*S 16-B loads in flight.
template <typename Y, typename X, class CP, int E, int S, int U, bool INIT, bool INT_FIRST, bool NT>
__global__ void __launch_bounds__(kBlock)
k_fedavg(X* __restrict__ agg, const ClientTable<typename CP::S> tab, const int K, const int64_t P) {
    using V = typename CP::V;
    using Sc = typename CP::S;
    const int64_t strip0 = (int64_t)blockIdx.x * (kBlock * S) + threadIdx.x;
    if ((strip0 + (int64_t)(S - 1) * kBlock) * E + E <= P) {
        V x[S][E];
        int k = 0;
#pragma unroll
        for (int s = 0; s < S; ++s)
            k = strip_start<Y, X, CP, E, INIT, INT_FIRST, NT>(x[s], agg, tab, (strip0 + s * kBlock) * E, E);
        for (; k + U <= K; k += U) {
            Y y[U][S][E];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const Y* yp = static_cast<const Y*>(tab.ptr[k + u]);
#pragma unroll
                for (int s = 0; s < S; ++s) strip_load<Y, E, NT>(yp + (strip0 + s * kBlock) * E, y[u][s]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const Sc n = tab.n[k + u], N = tab.N[k + u];
                const double r = tab.r[k + u];
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    V yv[E];
#pragma unroll
                    for (int e = 0; e < E; ++e) yv[e] = widen<Y, V>(y[u][s][e]);
                    fold_strip<CP, E>(x[s], yv, n, N, r);
                }
            }
        }
        for (; k < K; ++k) {
            const Y* yp = static_cast<const Y*>(tab.ptr[k]);
            Y y[S][E];
#pragma unroll
            for (int s = 0; s < S; ++s) strip_load<Y, E, NT>(yp + (strip0 + s * kBlock) * E, y[s]);
            const Sc n = tab.n[k], N = tab.N[k];
            const double r = tab.r[k];
#pragma unroll
            for (int s = 0; s < S; ++s) {
                V yv[E];
#pragma unroll
                for (int e = 0; e < E; ++e) yv[e] = widen<Y, V>(y[s][e]);
                fold_strip<CP, E>(x[s], yv, n, N, r);
            }
        }
#pragma unroll
        for (int s = 0; s < S; ++s) {
            X xo[E];
#pragma unroll
            for (int e = 0; e < E; ++e) xo[e] = narrow<X, V>(x[s][e]);
            strip_store<X, E>(agg + (strip0 + s * kBlock) * E, xo);
        }
    } else {
        k_fedavg_tail<Y, X, CP, E, S, INIT, INT_FIRST>(agg, tab, K, P, strip0);
    }
}

// Software-pipelined variant: while client k's S strips are folded, client k+1's are
// already in flight (two register buffers, explicit ping-pong), so a lane never waits
// for a whole batch to drain before issuing the next.
// Client-table access from registers: lane j of every wave holds client j's pointer,
// n, N and r (K <= 64 = wave size), and a client step reads them with v_readlane
// (uniform index -> SGPR) instead of a scalar-memory load + lgkmcnt wait.
template <class CP>
struct LaneTable {
    uint64_t p;
    typename CP::S n, N;
    double r;
    __device__ __forceinline__ explicit LaneTable(const ClientTable<typename CP::S>& tab) {
        const int lane = threadIdx.x & 63;
        p = reinterpret_cast<uint64_t>(tab.ptr[lane]);
        n = tab.n[lane];
        N = tab.N[lane];
        r = tab.r[lane];
    }
    template <typename T>
    __device__ __forceinline__ static T rl(T v, int k) {
        static_assert(sizeof(T) == 4 || sizeof(T) == 8, "readlane of 4/8-byte values");
        if constexpr (sizeof(T) == 4) {
            int i;
            __builtin_memcpy(&i, &v, 4);
            i = __builtin_amdgcn_readlane(i, k);
            __builtin_memcpy(&v, &i, 4);
            return v;
        } else {
            int i[2];
            __builtin_memcpy(i, &v, 8);
            i[0] = __builtin_amdgcn_readlane(i[0], k);
            i[1] = __builtin_amdgcn_readlane(i[1], k);
            __builtin_memcpy(&v, i, 8);
            return v;
        }
    }
};

// Workgroup -> tile order for the one-tile-per-workgroup grid. Only MAP 0 is instantiated.
// Workgroups are dealt round-robin to the 8 XCDs, so with MAP 0 consecutive tiles run on
// different XCDs. MAP = R > 0 gives each XCD runs of R consecutive tiles (groups of 8R tiles,
// XCD x taking tiles [xR, xR + R) of each group): a bijection on the first whole groups and
// the identity on the rest. (Runs of 2...32 measured within 1 % of identity, one contiguous
// eighth of the model per XCD 0.5-4 % slower: DESIGN.md §4.)
template <int MAP>
__device__ __forceinline__ int64_t map_tile(int64_t t, int64_t ntiles) {
    if constexpr (MAP > 0) {
        const int64_t g = ntiles / (8 * MAP);
        if (t < 8 * MAP * g) {
            const int64_t j = t / 8;
            t = (j / MAP) * (8 * MAP) + (t % 8) * MAP + (j % MAP);
        }
    }
    return t;
}

template <typename Y, typename X, class CP, int E, int S, bool INIT, bool INT_FIRST, bool NT, bool LT, int BLK, int NTS,
          int MAP, bool WIN = false>
__device__ __forceinline__ void fedavg_pipe_body(X* __restrict__ agg, const ClientTable<typename CP::S>& tab, const int K,
                                                 const int64_t P, const uint32_t period = 0, const uint32_t win_w = 0,
                                                 const int win_mode = 0) {
    using V = typename CP::V;
    const LaneTable<CP> lt(tab);
    const int64_t ntiles = ((P + E - 1) / E + (int64_t)BLK * S - 1) / ((int64_t)BLK * S);
    // one tile per block (gridDim == ntiles), or a persistent grid sweeping tiles in grid
    // order so the tiles read concurrently from one client buffer are adjacent
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int64_t tile = map_tile<MAP>(t, ntiles);
        const int64_t strip0 = tile * (BLK * S) + threadIdx.x;
        if ((strip0 + (int64_t)(S - 1) * BLK) * E + E > P) {
            k_fedavg_tail<Y, X, CP, E, S, INIT, INT_FIRST, BLK>(agg, tab, K, P, strip0);
            continue;
        }
        if constexpr (WIN) {
            if (win_mode >= 1) wait_read_window(period, win_w);
        }
        V x[S][E];
        int k = 0;
#pragma unroll
        for (int s = 0; s < S; ++s)
            k = strip_start<Y, X, CP, E, INIT, INT_FIRST, NT>(x[s], agg, tab, (strip0 + s * BLK) * E, E);
        auto load = [&](int kk, Y (&y)[S][E]) {
            const Y* yp = LT ? reinterpret_cast<const Y*>(LaneTable<CP>::rl(lt.p, kk)) : static_cast<const Y*>(tab.ptr[kk]);
#pragma unroll
            for (int s = 0; s < S; ++s) strip_load<Y, E, NT>(yp + (strip0 + s * BLK) * E, y[s]);
        };
        auto fold = [&](int kk, const Y (&y)[S][E]) {
            const typename CP::S n = LT ? LaneTable<CP>::rl(lt.n, kk) : tab.n[kk];
            const typename CP::S N = LT ? LaneTable<CP>::rl(lt.N, kk) : tab.N[kk];
            const double r = LT ? LaneTable<CP>::rl(lt.r, kk) : tab.r[kk];
#pragma unroll
            for (int s = 0; s < S; ++s) {
                V yv[E];
#pragma unroll
                for (int e = 0; e < E; ++e) yv[e] = widen<Y, V>(y[s][e]);
                fold_strip<CP, E>(x[s], yv, n, N, r);
            }
        };
        Y a[S][E], b[S][E];
        if (k < K) load(k, a);
        while (k + 1 < K) {
            if constexpr (WIN) {
                if (win_mode >= 2) wait_read_window(period, win_w);
            }
            load(k + 1, b);
            fold(k, a);
            if (k + 2 < K) load(k + 2, a);
            fold(k + 1, b);
            k += 2;
        }
        if (k < K) fold(k, a);
        if constexpr (WIN) wait_write_window(period, win_w);
#pragma unroll
        for (int s = 0; s < S; ++s) {
            X xo[E];
#pragma unroll
            for (int e = 0; e < E; ++e) xo[e] = narrow<X, V>(x[s][e]);
            if constexpr (is_nostore<CP>::value) {
                if (__float_as_uint(x[s][0]) != 0xFFFFFFFFu) continue;   // keeps loads + adds live
            }
            strip_store<X, E, NTS>(agg + (strip0 + s * BLK) * E, xo);
        }
    }
}

template <typename Y, typename X, class CP, int E, int S, bool INIT, bool INT_FIRST, bool NT, bool LT, int BLK = kBlock,
          int NTS = 0, int MAP = 0>
__global__ void __launch_bounds__(BLK)
k_fedavg_pipe(X* __restrict__ agg, const ClientTable<typename CP::S> tab, const int K, const int64_t P) {
    fedavg_pipe_body<Y, X, CP, E, S, INIT, INT_FIRST, NT, LT, BLK, NTS, MAP>(agg, tab, K, P);
}

// The ring depth, the parked tiles per workgroup, the tile height and the ring's load policy (1: nt)
// the product ships (avg_store_window has the measurements).
constexpr int kAvgParkDepth = 2, kAvgParkSlots = 2, kAvgParkHeight = 2, kAvgParkLoadPol = 1;

// The cache-policy operand (aux) of the ring's buffer loads for load policy POL (fa_tune
// AVG_PARK_LOADPOL): 0 default, 1 nt, 2 sc1, 3 sc1 nt. The bits are the compiler's gfx940-family
// encoding of a buffer instruction's policy (bit 1: slc, printed nt; bit 4: scc, printed sc1; bit 0,
// glc, printed sc0, stays clear) — read off the disassembly of the four instantiations, DESIGN §3.2.
constexpr int park_load_aux(int pol) { return ((pol & 1) ? 2 : 0) | ((pol & 2) ? 16 : 0); }

constexpr int park_lcm(int a, int b) {
    int m = a;
    while (m % b) m += a;
    return m;
}
template <int... Is, class F>
__device__ __forceinline__ void park_static_for(std::integer_sequence<int, Is...>, F&& f) {
    (f(std::integral_constant<int, Is>{}), ...);
}

// Store-window mode 3, "parked" (a first launch, INIT): no workgroup idles for the
// window. The grid is the resident workgroups, each sweeping tiles blockIdx.x + i * gridDim.x. A
// finished tile's results are parked in LDS (each lane its own 16-B pieces, piece s of lane l at
// [s * BLK + l] of a slot's small tile) and the workgroup goes straight on to its next tile. Four
// compile-time parameters (fa_tune AVG_PARK_DEPTH / _SLOTS / _HEIGHT / _LOADPOL): DEPTH client
// buffers in the load ring, SLOTS parked tiles per workgroup, HEIGHT consecutive 16 KiB tiles of the
// model in one "tall" tile, and the cache policy POL of the ring's loads (park_load_aux).
// The sweep is one stream of (tall tile, client, piece) positions, the piece advancing first, then
// the client, then the tile: a workgroup reads HEIGHT * 16 KiB of one client in a row, and the
// positions a wave has in flight are mostly neighbours in one client's buffer. A position is 16 KiB
// of one client whatever HEIGHT is. Buffer i holds stream position i mod DEPTH, the running values
// x[p] belong to piece p = i mod HEIGHT, and the step that consumes a position first issues the
// loads of the position DEPTH - 1 ahead into the buffer the step before it consumed. The load cursor
// (lt, lk) runs ahead of the consume cursor (t, k) across tile boundaries, over several tiles where
// K * HEIGHT < DEPTH. What keeps the loads in flight:
//  - the loop is counted (the workgroup's positions are known up front) and unrolled lcm(DEPTH,
//    HEIGHT) times, so buffer and piece indices are static and the loop has one exit; the remainder
//    of the stream and the last DEPTH - 1 steps, which load nothing, are copies of their own behind
//    it. (With an exit in every step, the compiler's common exit block is also a path back to the
//    loop's head on which a step's buffer is the newest load, and every wait is sized for that.)
//  - a strip is one buffer load: the position's base in a scalar descriptor, the strip in the scalar
//    offset, the lane's offset in a loop-invariant register. (Address registers are taken from the
//    buffer about to be loaded, and computing them waits for all but one load in flight.)
// A tall tile is parked piece by piece while its last client is consumed, and counts as parked with
// its last piece. Parked tiles are stored oldest first: all of them when a poll of the clock, once
// per client pair, finds the window open, the oldest behind the bounded wait when a tile is about to
// be parked with no slot free, the rest at the end of the sweep. Each wave keeps the FIFO for itself:
// `oldest` (a tall-tile number, -1 = none; the others follow gridDim.x apart), its slot `head`, and
// `count`. A lane reads back only what it wrote, so there is still no barrier. Arithmetic, element
// order per lane, store addresses and store flavour are mode 0's. What is no whole tall tile — up to
// HEIGHT - 1 whole 16 KiB tiles and the ragged one — goes through k_fedavg_tail, all the lanes of
// the workgroup park_partition.h names (the same arithmetic per element).
template <typename Y, typename X, class CP, int E, int S, int BLK, int NTS, int DEPTH, int SLOTS, int HEIGHT = 1, int POL = 0>
__device__ __forceinline__ void fedavg_park_body(X* __restrict__ agg, const ClientTable<typename CP::S>& tab, const int K,
                                                 const int64_t P, const uint32_t period, const uint32_t win_w) {
    using V = typename CP::V;
    static_assert(E * sizeof(X) == 16 && E * sizeof(Y) == 16, "one 16-B piece per strip");
    static_assert(DEPTH >= 2 && DEPTH <= 4, "a ring of 2, 3 or 4 client buffers");
    static_assert(HEIGHT == 1 || HEIGHT == 2 || HEIGHT == 4, "tall tiles of 1, 2 or 4 tiles");
    static_assert((SLOTS == 1 || SLOTS == 2 || SLOTS == 4) && SLOTS * HEIGHT * S * BLK * 16 <= 65536,
                  "1, 2 or 4 slots of static LDS");
    static_assert(POL >= 0 && POL <= 3, "load policy 0 (default), 1 (nt), 2 (sc1) or 3 (sc1 nt)");
    __shared__ u32x4 park[SLOTS][HEIGHT][S * BLK];
    constexpr int64_t kTile = (int64_t)BLK * S * E;
    constexpr int U = park_lcm(DEPTH, HEIGHT);                           // the loop's unroll: buffer and piece both static
    const ParkPartition part = park_partition(P, kTile, HEIGHT);
    // this workgroup's whole tall tiles and stream positions
    const int64_t mine = park_ring_tiles(part, gridDim.x, blockIdx.x), npos = mine * K * HEIGHT;
    V x[HEIGHT][S][E];
    Y buf[DEPTH][S][E];
    int64_t t = blockIdx.x, lt = t, oldest = -1;                         // the tile in hand, the last one loaded from, the FIFO
    int k = 0, lk = 0, head = 0, count = 0;
    const uint32_t lane_y = threadIdx.x * (uint32_t)(E * sizeof(Y)), lane_x = threadIdx.x * (uint32_t)(E * sizeof(X));
    // piece `piece` of client kk in tall tile tt < ntall: a whole 16 KiB tile, inside the client's buffer
    auto load = [&](int64_t tt, int kk, int piece, Y (&y)[S][E]) {
        char* base = const_cast<char*>(static_cast<const char*>(tab.ptr[kk])) + (tt * HEIGHT + piece) * (kTile * (int64_t)sizeof(Y));
        const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(base, 0, (int)(kTile * sizeof(Y)), 0x00020000);
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const u32x4 w = __builtin_amdgcn_raw_buffer_load_b128(rsrc, lane_y, s * BLK * E * (int)sizeof(Y), park_load_aux(POL));
            __builtin_memcpy(y[s], &w, 16);
        }
    };
    auto next = [&](int64_t& tt, int& kk) {                              // the client after (tt, kk)
        if (++kk == K) {
            kk = 0;
            tt += gridDim.x;
        }
    };
    auto flush = [&]() {                                                 // the oldest parked tile
        char* base = reinterpret_cast<char*>(agg) + oldest * (HEIGHT * kTile * (int64_t)sizeof(X));
#pragma unroll
        for (int p = 0; p < HEIGHT; ++p)
#pragma unroll
            for (int s = 0; s < S; ++s) {
                X xo[E];
                const u32x4 w = park[head][p][s * BLK + threadIdx.x];
                __builtin_memcpy(xo, &w, 16);
                strip_store<X, E, NTS>(reinterpret_cast<X*>(base + (int64_t)(p * S + s) * BLK * E * sizeof(X) + lane_x), xo);
            }
        head = (head + 1) % SLOTS;
        oldest = --count ? oldest + gridDim.x : -1;
    };
    // one step of the consume cursor: `cur` holds piece PC of client k of tall tile t
    auto consume = [&](auto pc, const Y (&cur)[S][E]) {
        constexpr int PC = decltype(pc)::value;
        if (k == 0) {                                                    // x := updates[0] (strip_start's INIT)
#pragma unroll
            for (int s = 0; s < S; ++s)
#pragma unroll
                for (int e = 0; e < E; ++e) x[PC][s][e] = widen<Y, V>(cur[s][e]);
        } else {
            const typename CP::S n = tab.n[k], N = tab.N[k];
            const double r = tab.r[k];
#pragma unroll
            for (int s = 0; s < S; ++s) {
                V yv[E];
#pragma unroll
                for (int e = 0; e < E; ++e) yv[e] = widen<Y, V>(cur[s][e]);
                fold_strip<CP, E>(x[PC][s], yv, n, N, r);
            }
        }
        if (k == K - 1) {                                                // the piece is finished: park it
            if constexpr (PC == 0) {
                if (count == SLOTS) {                                    // no slot free
                    wait_write_window(period, win_w);
                    flush();
                }
            }
            const int slot = (head + count) % SLOTS;
#pragma unroll
            for (int s = 0; s < S; ++s) {
                X xo[E];
#pragma unroll
                for (int e = 0; e < E; ++e) xo[e] = narrow<X, V>(x[PC][s][e]);
                u32x4 w;
                __builtin_memcpy(&w, xo, 16);
                park[slot][PC][s * BLK + threadIdx.x] = w;
            }
            if constexpr (PC == HEIGHT - 1) {
                if (count++ == 0) oldest = t;
            }
        } else if (PC == HEIGHT - 1 && (k & 1) && count > 0 && in_write_window(period, win_w)) {
            do flush();
            while (count > 0);
        }
        if constexpr (PC == HEIGHT - 1) next(t, k);
    };
    // the load cursor moves on to a position whose piece is LP, and loads it into buf[B]
    auto fetch = [&](auto lp, auto b) {
        constexpr int LP = decltype(lp)::value;
        if constexpr (LP == 0) next(lt, lk);
        load(lt, lk, LP, buf[decltype(b)::value]);
    };
    // step J of the unrolled ring: the load DEPTH - 1 positions ahead is issued before position J is consumed
    auto step = [&](auto jx) {
        constexpr int J = decltype(jx)::value;
        fetch(std::integral_constant<int, (J + DEPTH - 1) % HEIGHT>{}, std::integral_constant<int, (J + DEPTH - 1) % DEPTH>{});
        consume(std::integral_constant<int, J % HEIGHT>{}, buf[J % DEPTH]);
    };
    // the last DEPTH - 1 positions, all loaded, from position J on
    auto drain = [&](auto jx) {
        constexpr int J = decltype(jx)::value;
        park_static_for(std::make_integer_sequence<int, DEPTH - 1>{}, [&](auto d) {
            constexpr int Q = J + decltype(d)::value;
            consume(std::integral_constant<int, Q % HEIGHT>{}, buf[Q % DEPTH]);
        });
    };
    // the remainder behind the loop: `rem` < U more steps, then the drain
    auto finish = [&](auto self, auto jx, int rem) -> void {
        constexpr int J = decltype(jx)::value;
        if constexpr (J == U - 1) {
            drain(jx);
        } else {
            if (rem == J) {
                drain(jx);
            } else {
                step(jx);
                self(self, std::integral_constant<int, J + 1>{}, rem);
            }
        }
    };
    using I0 = std::integral_constant<int, 0>;
    if (npos >= DEPTH - 1) {
        load(t, 0, 0, buf[0]);                                           // DEPTH - 1 positions before the first consume
        park_static_for(std::make_integer_sequence<int, DEPTH - 2>{}, [&](auto d) {
            constexpr int Q = decltype(d)::value + 1;
            fetch(std::integral_constant<int, Q % HEIGHT>{}, std::integral_constant<int, Q>{});
        });
        const int64_t nstep = npos - (DEPTH - 1);                        // steps that load
        for (int64_t i = nstep / U; i > 0; --i) park_static_for(std::make_integer_sequence<int, U>{}, step);
        finish(finish, I0{}, (int)(nstep % U));
    } else if (npos > 0) {                                               // a stream shorter than the ring: 1 or 2 positions
        load(t, 0, 0, buf[0]);
        if (npos > 1) fetch(std::integral_constant<int, 1 % HEIGHT>{}, std::integral_constant<int, 1>{});
        consume(I0{}, buf[0]);
        if (npos > 1) consume(std::integral_constant<int, 1 % HEIGHT>{}, buf[1]);
    }
    while (count > 0) flush();
    for (int j = 0; j < part.ntail(); ++j)
        if (park_tail_owner(part, gridDim.x, j) == blockIdx.x)
            k_fedavg_tail<Y, X, CP, E, S, true, false, BLK>(agg, tab, K, P, (part.ntall * HEIGHT + j) * (BLK * S) + threadIdx.x);
}

// The parked fold at any (DEPTH, SLOTS, HEIGHT, POL), for the probe library: a kernel template of its
// own, so that the window kernels keep their names (profiles/pmc_traffic.json is keyed on them). The
// launcher reports k_fedavg_pipe_win's family for it.
template <typename Y, typename X, class CP, int E, int S, int BLK, int NTS, int DEPTH, int SLOTS, int HEIGHT = 1, int POL = 0>
__global__ void __launch_bounds__(BLK)
k_fedavg_park(X* __restrict__ agg, const ClientTable<typename CP::S> tab, const int K, const int64_t P, const uint32_t period,
              const uint32_t win_w) {
    fedavg_park_body<Y, X, CP, E, S, BLK, NTS, DEPTH, SLOTS, HEIGHT, POL>(agg, tab, K, P, period, win_w);
}

// The same fold with every wave's stores inside a chip-wide window of the GPU's 100 MHz clock
// (avg_store_window): bit-identical, the stores bunched into common bursts.
// PARK: mode 3, whose LDS no other instantiation carries.
template <typename Y, typename X, class CP, int E, int S, bool INIT, bool INT_FIRST, bool NT, bool LT, int BLK, int NTS,
          int MAP, bool PARK = false>
__global__ void __launch_bounds__(BLK)
k_fedavg_pipe_win(X* __restrict__ agg, const ClientTable<typename CP::S> tab, const int K, const int64_t P,
                  const uint32_t period, const uint32_t win_w, const int win_mode) {
    if constexpr (PARK) {
        static_assert(INIT && !INT_FIRST && !NT && !LT && MAP == 0, "parked stores: first launches of the product geometry");
        fedavg_park_body<Y, X, CP, E, S, BLK, NTS, kAvgParkDepth, kAvgParkSlots, kAvgParkHeight, kAvgParkLoadPol>(agg, tab, K, P, period, win_w);
    } else {
        fedavg_pipe_body<Y, X, CP, E, S, INIT, INT_FIRST, NT, LT, BLK, NTS, MAP, true>(agg, tab, K, P, period, win_w, win_mode);
    }
}
