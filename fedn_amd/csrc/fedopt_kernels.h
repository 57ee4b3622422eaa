// fedopt_kernels.h — the FedOpt step, device code: the pseudo-gradient fold (the running mean of
// y_k - old) and the Adam / Yogi / AdaGrad server step over (old, m, v), fused. k_fedopt (per-lane
// strips, any alignment), k_fedopt_c (the wave-coalesced element map) and k_fedopt_cw (its stores
// inside the chip-wide window).
// Included by fedagg.hip inside its anonymous namespace, after fold_rules.h, whose rules, strips, client
// table and window clock it uses. DESIGN.md §3.3 describes it (§3.3c the fp32-state mode);
// fedopt_launch.h chooses among these kernels.

struct OptScalars {
    // python-float constants exactly as fedopt.py computes them
    double lr, b1, b2, tau, tau2, c1, c2, nc2;   // c1 = 1-b1, c2 = 1-b2, nc2 = -(1-b2)
    float b1f, c1f, c2f;                         // the same cast to f32 (numpy weak-scalar rule)
    float b1h, c1h, c2h;                         // ... and to f16 (held in f32): float16 state / pg
    int opt;
};

struct OptBuffers {
    const void* old;
    void* pg;
    const void* m_in;
    void* m_out;
    const void* v_in;
    void* v_out;
    void* out;
    int m_in_f64;    // 0: f32, 1: f64, -1: None
    int m_out_f64;
    // storage dtype of v and the new model (fa_fedopt_step_ex): 0 = f64 (the reference's), 1 = f32
    // (the fp32-state mode: same f64 arithmetic, rounded once to f32 on store, widened exactly on load)
    int v_in_f32;
    int v_out_f32;
    int out_f32;
};

// multiply an array element held as PG by a python float constant (numpy weak scalar)
template <class PG> __device__ __forceinline__ double mul_pg(double a, double c, float cf, float ch);
template <> __device__ __forceinline__ double mul_pg<CF32>(double a, double, float cf, float) { return (double)((float)a * cf); }
template <> __device__ __forceinline__ double mul_pg<CF64>(double a, double c, float, float) { return a * c; }
template <> __device__ __forceinline__ double mul_pg<CF16>(double a, double, float, float ch) {
    return (double)CF16::rh((float)a * ch);
}

// numpyhelper.subtract(next, old) = next*1.0 + old*(-1.0) (numpyhelper.py:44-56) and power(pg, 2)
// (:94-104) in the pseudo-gradient's dtype: float16 rounds every op to half, as numpy's half loops
template <class PG> __device__ __forceinline__ typename PG::V pg_sub(typename PG::V y, typename PG::V o) { return y - o; }
template <> __device__ __forceinline__ float pg_sub<CF16>(float y, float o) { return CF16::rh(y - o); }
template <class PG> __device__ __forceinline__ typename PG::V pg_sq(typename PG::V v) { return (typename PG::V)(v * v); }
template <> __device__ __forceinline__ float pg_sq<CF16>(float v) { return CF16::rh(v * v); }

__device__ __forceinline__ double np_sign(double d) {
    // numpy sign: 1 / -1 / 0 (for +-0), NaN propagates
    return d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : (d == 0.0 ? 0.0 : d));
}

// The server state of one strip: m_in (as exact f64 values; f32 state is widened exactly) and
// v_in (or tau**2 when v is None, fedopt.py:170-171). rem < E: ragged strip.
template <int E, bool SNT = false>
__device__ __forceinline__ void opt_load_state(const OptBuffers& b, const OptScalars& s, int64_t i0, int rem,
                                               double (&mi)[E], double (&v)[E]) {
    const bool full = rem == E;
    if (b.m_in_f64 == 0) {
        float mf[E];
        const float* mp = static_cast<const float*>(b.m_in) + i0;
        if (full) strip_load<float, E, SNT>(mp, mf);
        else
            for (int e = 0; e < E; ++e) mf[e] = e < rem ? mp[e] : 0.f;
#pragma unroll
        for (int e = 0; e < E; ++e) mi[e] = (double)mf[e];
    } else if (b.m_in_f64 == 1) {
        const double* mp = static_cast<const double*>(b.m_in) + i0;
        if (full) strip_load<double, E, SNT>(mp, mi);
        else
            for (int e = 0; e < E; ++e) mi[e] = e < rem ? mp[e] : 0.0;
    } else if (b.m_in_f64 == 2) {                // float16 m (a float16 session's first rounds)
        f16 mh[E];
        const f16* mp = static_cast<const f16*>(b.m_in) + i0;
        if (full) strip_load<f16, E, SNT>(mp, mh);
        else
            for (int e = 0; e < E; ++e) mh[e] = e < rem ? mp[e] : f16{0};
#pragma unroll
        for (int e = 0; e < E; ++e) mi[e] = (double)f16_to_f32(mh[e].bits);
    }
    if (b.v_in && b.v_in_f32) {
        float vf[E];
        const float* vp = static_cast<const float*>(b.v_in) + i0;
        if (full) strip_load<float, E, SNT>(vp, vf);
        else
            for (int e = 0; e < E; ++e) vf[e] = e < rem ? vp[e] : 0.f;
#pragma unroll
        for (int e = 0; e < E; ++e) v[e] = (double)vf[e];
    } else if (b.v_in) {
        const double* vp = static_cast<const double*>(b.v_in) + i0;
        if (full) strip_load<double, E, SNT>(vp, v);
        else
            for (int e = 0; e < E; ++e) v[e] = e < rem ? vp[e] : 0.0;
    } else {
#pragma unroll
        for (int e = 0; e < E; ++e) v[e] = s.tau2;
    }
}

// The server step for one strip of E elements (fedopt.py:151-258), from the folded
// pseudo-gradient pg, the widened old model ov (OLD -> V is exact or the same conversion
// numpy's `old * 1.0` makes, so (double)ov == old as numpy sees it) and the state loaded by
// opt_load_state (mi, v; v is updated in place). rem < E: ragged strip.
template <class PG, int E, bool NOST = false, int OSM = 0>
__device__ __forceinline__ void opt_apply(const OptBuffers& b, const OptScalars& s, const typename PG::V (&pg)[E],
                                          const typename PG::V (&ov)[E], const double (&mi)[E], double (&v)[E],
                                          int64_t i0, int rem) {
    using V = typename PG::V;
    constexpr bool PG32 = std::is_same<PG, CF32>::value;
    const bool full = rem == E;
    // ---- m (fedopt.py:173-176 and the two twins)
    constexpr bool PG64 = std::is_same<PG, CF64>::value;
    double m[E];
    if (b.m_in_f64 < 0) {
#pragma unroll
        for (int e = 0; e < E; ++e) m[e] = mul_pg<PG>((double)pg[e], s.c1, s.c1f, s.c1h);
    } else {
        // m*beta1 in m's dtype, pg*(1-beta1) in pg's dtype, their sum in the promoted dtype
        // (f16 < f32 < f64); each operand is exact in its dtype, so the float sum rounds once
        if (b.m_in_f64 == 1) {                     // f64 m: an f64 sum
#pragma unroll
            for (int e = 0; e < E; ++e) m[e] = mi[e] * s.b1 + mul_pg<PG>((double)pg[e], s.c1, s.c1f, s.c1h);
        } else if (b.m_in_f64 == 0) {              // f32 m (mi is an exact f32)
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const float a = (float)mi[e] * s.b1f;
                const double pm = mul_pg<PG>((double)pg[e], s.c1, s.c1f, s.c1h);
                if constexpr (PG64) m[e] = (double)a + pm;          // f32 + f64
                else m[e] = (double)(a + (float)pm);                // f32 + f32 (or f16) in f32
            }
        } else {                                   // f16 m (a float16 session's first rounds)
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const float a = CF16::rh((float)mi[e] * s.b1h);
                const double pm = mul_pg<PG>((double)pg[e], s.c1, s.c1f, s.c1h);
                if constexpr (PG64) m[e] = (double)a + pm;
                else if constexpr (PG32) m[e] = (double)(a + (float)pm);
                else m[e] = (double)CF16::rh(a + (float)pm);
            }
        }
    }
    // ---- v (fedopt.py:178-179 / 214-217 / 251-252)
    double o[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const V pv = pg[e];
        const double p = (double)pg_sq<PG>(pv);   // power(pg, 2) in the pg dtype
        if (s.opt == FA_ADAM) {
            v[e] = v[e] * s.b2 + mul_pg<PG>(p, s.c2, s.c2f, s.c2h);
        } else if (s.opt == FA_YOGI) {
            const double sg = np_sign(v[e] - p);
            v[e] = v[e] + (sg * p) * s.nc2;
        } else {
            v[e] = v[e] + p;
        }
        const double sv = __builtin_sqrt(v[e]) + s.tau;
        const double t = m[e] / sv;
        o[e] = (double)ov[e] + t * s.lr;
    }
    // ---- stores
    if constexpr (NOST) {   // probe build: stores skipped behind a never-true data test (reads + math live)
        if (__double_as_longlong(o[0]) != 0x7FF4DEADBEEF0001LL) return;
    }
    if (full) {
        if (b.v_out_f32) {
            float vf[E];
#pragma unroll
            for (int e = 0; e < E; ++e) vf[e] = (float)v[e];
            strip_store<float, E, OSM>(static_cast<float*>(b.v_out) + i0, vf);
        } else {
            strip_store<double, E, OSM>(static_cast<double*>(b.v_out) + i0, v);
        }
        if (b.out_f32) {
            float of[E];
#pragma unroll
            for (int e = 0; e < E; ++e) of[e] = (float)o[e];
            strip_store<float, E, OSM>(static_cast<float*>(b.out) + i0, of);
        } else {
            strip_store<double, E, OSM>(static_cast<double*>(b.out) + i0, o);
        }
        if (b.m_out_f64 == 1) strip_store<double, E, OSM>(static_cast<double*>(b.m_out) + i0, m);
        else if (b.m_out_f64 == 0) {
            float mf[E];
#pragma unroll
            for (int e = 0; e < E; ++e) mf[e] = (float)m[e];
            strip_store<float, E, OSM>(static_cast<float*>(b.m_out) + i0, mf);
        } else {                                  // f16 m: every value is already a half
            f16 mh[E];
#pragma unroll
            for (int e = 0; e < E; ++e) mh[e] = f16{f32_to_f16((float)m[e])};
            strip_store<f16, E, 0>(static_cast<f16*>(b.m_out) + i0, mh);
        }
    } else {
        for (int e = 0; e < rem; ++e) {
            if (b.v_out_f32) static_cast<float*>(b.v_out)[i0 + e] = (float)v[e];
            else static_cast<double*>(b.v_out)[i0 + e] = v[e];
            if (b.out_f32) static_cast<float*>(b.out)[i0 + e] = (float)o[e];
            else static_cast<double*>(b.out)[i0 + e] = o[e];
            if (b.m_out_f64 == 1) static_cast<double*>(b.m_out)[i0 + e] = m[e];
            else if (b.m_out_f64 == 0) static_cast<float*>(b.m_out)[i0 + e] = (float)m[e];
            else static_cast<f16*>(b.m_out)[i0 + e] = f16{f32_to_f16((float)m[e])};
        }
    }
}

template <class PG, int E, bool NOST = false, int OSM = 0>
__device__ __forceinline__ void opt_final(const OptBuffers& b, const OptScalars& s, const typename PG::V (&pg)[E],
                                          const typename PG::V (&ov)[E], int64_t i0, int rem) {
    double mi[E], v[E];
    opt_load_state<E>(b, s, i0, rem, mi, v);
    opt_apply<PG, E, NOST, OSM>(b, s, pg, ov, mi, v, i0, rem);
}

// One lane's strip of E elements at i0 < P, clients batched kUnroll/2 at a time. (A
// k_fedavg_pipe-style traversal — 2 or 4 strips per lane, next client in flight — measured
// within noise of this one on configs[3]: profiles/r01_fedopt_ab.log)
template <typename Y, typename OLD, class PG, int E, bool FIRST, bool FINAL, bool NT, bool NOST = false, int OSM = 0>
__device__ __forceinline__ void fedopt_strip(const OptBuffers& b, const OptScalars& s,
                                             const ClientTable<typename PG::S>& tab, const int K, const int64_t P,
                                             const int64_t i0) {
    using V = typename PG::V;   // float or double
    const int rem = (P - i0) < E ? (int)(P - i0) : E;
    const bool full = rem == E;

    OLD old[E];
    const OLD* oldp = static_cast<const OLD*>(b.old) + i0;
    if (full) strip_load<OLD, E, false>(oldp, old);
    else {
#pragma unroll
        for (int e = 0; e < E; ++e) old[e] = e < rem ? oldp[e] : OLD{};
    }
    V ov[E];
#pragma unroll
    for (int e = 0; e < E; ++e) ov[e] = widen<OLD, V>(old[e]);

    // ---- pseudo-gradient: pg = y0 - old ; pg = pg + (n*((y_k - old) - pg))/N (fedopt.py:89-94)
    V pg[E];
    int k = 0;
    if constexpr (FIRST) {
        Y y[E];
        const Y* yp = static_cast<const Y*>(tab.ptr[0]) + i0;
        if (full) strip_load<Y, E, NT>(yp, y);
        else {
#pragma unroll
            for (int e = 0; e < E; ++e) y[e] = e < rem ? yp[e] : Y{};
        }
#pragma unroll
        for (int e = 0; e < E; ++e) pg[e] = pg_sub<PG>(widen<Y, V>(y[e]), ov[e]);
        k = 1;
    } else {
        using T = typename PG::T;                 // the workspace holds pg in its own dtype
        const T* pgp = static_cast<const T*>(b.pg) + i0;
        if (full) {
            T t[E];
            strip_load<T, E, false>(pgp, t);
#pragma unroll
            for (int e = 0; e < E; ++e) pg[e] = widen<T, V>(t[e]);
        } else {
#pragma unroll
            for (int e = 0; e < E; ++e) pg[e] = e < rem ? widen<T, V>(pgp[e]) : V{};
        }
    }
    if (full) {
        for (; k + kUnroll / 2 <= K; k += kUnroll / 2) {
            Y y[kUnroll / 2][E];
#pragma unroll
            for (int u = 0; u < kUnroll / 2; ++u)
                strip_load<Y, E, NT>(static_cast<const Y*>(tab.ptr[k + u]) + i0, y[u]);
#pragma unroll
            for (int u = 0; u < kUnroll / 2; ++u) {
                const typename PG::S n = tab.n[k + u], N = tab.N[k + u];
                const double r = tab.r[k + u];
                V d[E];
#pragma unroll
                for (int e = 0; e < E; ++e) d[e] = pg_sub<PG>(widen<Y, V>(y[u][e]), ov[e]);   // subtract(next, old)
                fold_strip<PG, E>(pg, d, n, N, r);
            }
        }
    }
    for (; k < K; ++k) {
        const Y* yp = static_cast<const Y*>(tab.ptr[k]) + i0;
        const typename PG::S n = tab.n[k], N = tab.N[k];
        const double r = tab.r[k];
#pragma unroll
        for (int e = 0; e < E; ++e)
            if (e < rem) pg[e] = PG::fold(pg[e], pg_sub<PG>(widen<Y, V>(yp[e]), ov[e]), n, N, r);
    }

    if constexpr (!FINAL) {
        using T = typename PG::T;
        T* pgp = static_cast<T*>(b.pg) + i0;
        T t[E];
#pragma unroll
        for (int e = 0; e < E; ++e) t[e] = narrow<T, V>(pg[e]);
        if (full) strip_store<T, E>(pgp, t);
        else
            for (int e = 0; e < rem; ++e) pgp[e] = t[e];
        return;
    } else {
        opt_final<PG, E, NOST, OSM>(b, s, pg, ov, i0, rem);
    }
}

// The same lane work with a wave-coalesced element map: lane L of a wave tile of 128*NH elements
// owns the pairs {2L, 2L+1} + 128 j, j < NH, so every 8-byte stream (old, m, v, pg, out) moves one
// contiguous 1 KiB per wave instruction (full 128-B lines, no half-line stores) and the client loads
// are contiguous 512-B dwordx2 wave instructions. Whole wave tiles only.
// H: elements per lane per strip — 2 (pairs; the only value instantiated) or 4 (quads at lane
// stride 4: 2-byte client loads become dwordx2, 8-byte streams two dwordx4 per strip; a null result).
template <typename Y, typename OLD, class PG, bool FIRST, bool FINAL, bool NT, int OSM = 0, int NH = 2,
          int U = kUnroll / 2, bool WIN = false, int H = 2>
__device__ __forceinline__ void fedopt_strip_split(const OptBuffers& b, const OptScalars& s,
                                                   const ClientTable<typename PG::S>& tab, const int K,
                                                   const int64_t i0, const uint32_t period = 0,
                                                   const uint32_t win_w = 0) {
    using V = typename PG::V;
    constexpr int E = H * NH;
    auto half = [](auto& a, int h) -> auto& {
        using T = std::remove_reference_t<decltype(a[0])>;
        return *reinterpret_cast<T(*)[H]>(&a[h * H]);
    };
    auto at = [i0](int h) { return i0 + (int64_t)h * 64 * H; };
    OLD old[E];
#pragma unroll
    for (int h = 0; h < NH; ++h) strip_load<OLD, H, false>(static_cast<const OLD*>(b.old) + at(h), half(old, h));
    V ov[E];
#pragma unroll
    for (int e = 0; e < E; ++e) ov[e] = widen<OLD, V>(old[e]);
    V pg[E];
    int k = 0;
    if constexpr (FIRST) {
        Y y[E];
        const Y* yp = static_cast<const Y*>(tab.ptr[0]);
#pragma unroll
        for (int h = 0; h < NH; ++h) strip_load<Y, H, NT>(yp + at(h), half(y, h));
#pragma unroll
        for (int e = 0; e < E; ++e) pg[e] = pg_sub<PG>(widen<Y, V>(y[e]), ov[e]);
        k = 1;
    } else {
        using T = typename PG::T;                 // the workspace holds pg in its own dtype
        T t[E];
#pragma unroll
        for (int h = 0; h < NH; ++h) strip_load<T, H, false>(static_cast<const T*>(b.pg) + at(h), half(t, h));
#pragma unroll
        for (int e = 0; e < E; ++e) pg[e] = widen<T, V>(t[e]);
    }
    for (; k + U <= K; k += U) {
        Y y[U][E];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const Y* yp = static_cast<const Y*>(tab.ptr[k + u]);
#pragma unroll
            for (int h = 0; h < NH; ++h) strip_load<Y, H, NT>(yp + at(h), half(y[u], h));
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            V d[E];
#pragma unroll
            for (int e = 0; e < E; ++e) d[e] = pg_sub<PG>(widen<Y, V>(y[u][e]), ov[e]);
            fold_strip<PG, E>(pg, d, tab.n[k + u], tab.N[k + u], tab.r[k + u]);
        }
    }
    for (; k < K; ++k) {
        const Y* yp = static_cast<const Y*>(tab.ptr[k]);
        Y y[E];
#pragma unroll
        for (int h = 0; h < NH; ++h) strip_load<Y, H, NT>(yp + at(h), half(y, h));
        V d[E];
#pragma unroll
        for (int e = 0; e < E; ++e) d[e] = pg_sub<PG>(widen<Y, V>(y[e]), ov[e]);
        fold_strip<PG, E>(pg, d, tab.n[k], tab.N[k], tab.r[k]);
    }
    if constexpr (!FINAL) {
        using T = typename PG::T;
        T t[E];
#pragma unroll
        for (int e = 0; e < E; ++e) t[e] = narrow<T, V>(pg[e]);
        if constexpr (WIN) wait_write_window(period, win_w);
#pragma unroll
        for (int h = 0; h < NH; ++h) strip_store<T, H>(static_cast<T*>(b.pg) + at(h), half(t, h));
    } else {
        double mi[E], vv[E];
#pragma unroll
        for (int h = 0; h < NH; ++h) opt_load_state<H>(b, s, at(h), H, half(mi, h), half(vv, h));
        if constexpr (WIN) wait_write_window(period, win_w);   // the state loads land meanwhile
#pragma unroll
        for (int h = 0; h < NH; ++h)
            opt_apply<PG, H, false, OSM>(b, s, half(pg, h), half(ov, h), half(mi, h), half(vv, h), at(h), H);
    }
}

template <typename Y, typename OLD, class PG, bool FIRST, bool FINAL, bool NT, int OSM, int NH, int U, bool MV = false,
          bool WIN = false>
__device__ __forceinline__ void fedopt_c_body(const OptBuffers& b, const OptScalars& s, const ClientTable<typename PG::S>& tab,
                                              const int K, const int64_t P, const uint32_t period = 0,
                                              const uint32_t win_w = 0) {
    constexpr int64_t T = 128 * NH;                                     // elements per wave tile
    const int64_t base = ((int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * T;
    const int lane = threadIdx.x & 63;
    if constexpr (MV) {
        // layout probe (never instantiated now): fp64 m and v interleaved per wave tile in one buffer
        // ([m of tile w | v of tile w] at 2wT), read from m_in and written to m_out; whole tiles only
        if (base + T > P) return;
        OptBuffers bb = b;
        bb.m_in = static_cast<const double*>(b.m_in) + base;
        bb.v_in = static_cast<const double*>(b.m_in) + base + T;
        bb.m_out = static_cast<double*>(b.m_out) + base;
        bb.v_out = static_cast<double*>(b.m_out) + base + T;
        fedopt_strip_split<Y, OLD, PG, FIRST, FINAL, NT, OSM, NH, U>(bb, s, tab, K, base + 2 * lane);
        return;
    }
    if (base + T <= P) {
        fedopt_strip_split<Y, OLD, PG, FIRST, FINAL, NT, OSM, NH, U, WIN>(b, s, tab, K, base + 2 * lane, period, win_w);
    } else {                                      // the ragged last tile: the per-lane strip map
#pragma unroll
        for (int j = 0; j < NH / 2; ++j) {
            const int64_t i0 = base + j * 256 + 4 * lane;
            if (i0 < P) fedopt_strip<Y, OLD, PG, 4, FIRST, FINAL, NT, false, OSM>(b, s, tab, K, P, i0);
        }
    }
}

template <typename Y, typename OLD, class PG, bool FIRST, bool FINAL, bool NT, int OSM = 0, int NH = 2,
          int U = kUnroll / 2>
__global__ void __launch_bounds__(kBlock)
k_fedopt_c(const OptBuffers b, const OptScalars s, const ClientTable<typename PG::S> tab, const int K, const int64_t P) {
    fedopt_c_body<Y, OLD, PG, FIRST, FINAL, NT, OSM, NH, U>(b, s, tab, K, P);
}

// The same single-launch step (all K clients, FIRST | FINAL) with every wave's v / out / m stores
// issued inside a chip-wide window of the GPU's 100 MHz reference clock (clock mod period < win_w;
// opt_store_window sizes both from the launch's bytes per round of resident waves). Reads continue
// throughout; the stores of all waves bunch into common bursts instead of interleaving with 36
// read streams everywhere — fewer DRAM read/write turnarounds (profiles/r05_fedopt_window.log).
// Arithmetic and element map are k_fedopt_c's: bit-identical results.
template <typename Y, typename OLD, class PG, bool NT>
__global__ void __launch_bounds__(kBlock)
k_fedopt_cw(const OptBuffers b, const OptScalars s, const ClientTable<typename PG::S> tab, const int K, const int64_t P,
            const uint32_t period, const uint32_t win_w) {
    fedopt_c_body<Y, OLD, PG, true, true, NT, 1, 4, kUnroll / 2, false, true>(b, s, tab, K, P, period, win_w);
}

template <typename Y, typename OLD, class PG, int E, bool FIRST, bool FINAL, bool NT, bool NOST = false, int OSM = 0>
__global__ void __launch_bounds__(kBlock)
k_fedopt(const OptBuffers b, const OptScalars s, const ClientTable<typename PG::S> tab, const int K, const int64_t P) {
    const int64_t i0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * E;
    if (i0 < P) fedopt_strip<Y, OLD, PG, E, FIRST, FINAL, NT, NOST, OSM>(b, s, tab, K, P, i0);
}
