// fedagg.hip — gfx950 (MI355X) kernels + C ABI for FEDn's combiner-side aggregation.
//
// The hot path is an elementwise, HBM-bound recurrence over K client buffers:
//   FedAvg  (numpyhelper.py:32, fedavg.py:47-71):   x <- x + (n_k*(y_k - x))/N_k
//   FedOpt  (fedopt.py:74-118):  pg <- running mean of (y_k - old), then one
//           Adam/Yogi/AdaGrad server step (fedopt.py:151-258) over (old, m, v).
// Every output element depends only on the same element of the inputs, and the
// client order is fixed by FEDn's FIFO queue, so parallelism is across elements:
// one lane owns a 16-byte strip of elements, keeps the running aggregate in
// registers for all K clients (no LDS round trip: nothing is shared between
// lanes), issues the K strip loads U at a time so every wave has U x 1 KiB in
// flight, and stores once. Bit-exact parity with numpy requires replaying the
// op order with IEEE rounding at every step: this file is compiled with
// -ffp-contract=off and relies on hipcc's correctly rounded f32/f64 `/` and
// f64 sqrt (checked against the golden fixtures).
//
// Client tables (pointer, n_k, N_k) travel in the kernarg segment (<= 64 clients
// per launch, ~1.5 KiB): they are read by scalar loads, need no H2D copy and keep
// launches graph-capturable. K > 64 is chunked by the host code (launch_fedavg, launch_fedopt); the
// chunks continue from the stored aggregate, which replays the same recurrence exactly.

#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <algorithm>
#include <atomic>
#include <cstring>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/fedagg.h"
#ifdef FEDAGG_PROBES
#include "../../include/fedagg_probe.h"
#endif

namespace {

// ----------------------------------------------------------------------------
// error plumbing
// ----------------------------------------------------------------------------
thread_local char g_err[512] = "";
// the kernel family the calling thread's last fold / FedOpt launch used (fa_last_kernel): a diagnostic
// like g_err, so a benchmark names the kernel that ran, not one it infers
thread_local const char* g_kernel = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(FA_EHIP, "%s: %s", what, hipGetErrorString(e));
    return FA_OK;
}

constexpr int kMaxK = 64;     // clients per launch (kernarg table)
constexpr int kBlock = 256;   // 4 waves
constexpr int kUnroll = 8;    // client strips in flight per lane

size_t dt_size(int dt) {
    switch (dt) {
        case FA_F32: return 4;
        case FA_F64: return 8;
        case FA_BF16: return 2;
        case FA_F16: return 2;
        case FA_I32: return 4;
        case FA_I64: return 8;
        default: return 0;
    }
}

// The kernel families and their launch policy, one header each, in dependency order
#include "fold_rules.h"      // element types, numpy's arithmetic per dtype, 16-B strips, the client table
#include "park_partition.h"   // the parked fold's split of a model into ring tiles and tail tiles (kernel, launcher, CPU test)
#include "fedavg_kernels.h"   // k_fedavg, k_fedavg_pipe, k_fedavg_pipe_win (the parked fold included)
#include "fedopt_kernels.h"   // k_fedopt, k_fedopt_c, k_fedopt_cw
#include "helper_kernels.h"   // numpyhelper primitives, the 1-norm, k_cast
#include "peer_push.h"        // k_fedavg_push, k_push, k_release
#include "probes.h"           // probe build: measurement kernels, knobs and launch hooks; product: inert stubs
#include "host_common.h"      // client-table fill, occupancy, host-mapped rounds
#include "fedavg_launch.h"    // store window, parked grid, geometry by size, launch_fedavg
#include "fedopt_launch.h"    // store window, launch_fedopt
#include "order_mean.h"       // coordinate-wise trimmed mean / median (k_order_mean, fa_trimmed_mean)
#include "median_window.h"    // mean of the values closest to the median, Bulyan (k_median_window, fa_median_window_mean)
#include "pair_dist.h"        // pairwise squared distances for Krum / Multi-Krum (k_pair_sqdist, fa_pairwise_sqdist)
#include "wmean_dist.h"       // weighted mean and the K squared distances to it (k_wmean_dist, fa_weighted_mean_sqdist)
#include "cclip.h"            // one centred-clipping step and the K squared distances to it (k_cclip_dist, fa_centered_clip_step)
#include "clip_fold.h"        // the clipping fold carried across chunks of more than 64 clients (k_clip_fold, fa_clip_fold)
#include "dp_noise.h"         // Philox Gaussian noise added to a buffer, DP-FedAvg (k_gaussian_noise, fa_gaussian_noise)

}  // namespace

// ============================================================================
// C ABI
// ============================================================================
extern "C" {

int fa_abi_version(void) { return FA_ABI_VERSION; }

const char* fa_last_error(void) { return g_err; }
const char* fa_last_kernel(void) { return g_kernel; }

int fa_promote(int a, int b) {
    auto fl = [](int d) { return d == FA_BF16 ? FA_F32 : d; };
    if (a == FA_NONE) return fl(b);
    if (b == FA_NONE) return fl(a);
    a = fl(a);
    b = fl(b);
    if (a == b) return a;
    if (a == FA_F64 || b == FA_F64) return FA_F64;
    if ((a == FA_F32 && b == FA_F16) || (a == FA_F16 && b == FA_F32)) return FA_F32;
    return FA_NONE;
}

int fa_fedavg_fold(void* agg, int agg_dtype, const void* const* updates, int upd_dtype, const double* n, const double* N,
                   int K, int64_t P, int init, void* stream) {
    g_err[0] = 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (P < 0 || K < 0) return fail(FA_EINVAL, "fa_fedavg_fold: negative size (P=%lld, K=%d)", (long long)P, K);
    if (init && K < 1) return fail(FA_EINVAL, "fa_fedavg_fold: init requires K >= 1");
    if (K == 0 || P == 0) return FA_OK;
    if (!agg || !updates || !n || !N) return fail(FA_EINVAL, "fa_fedavg_fold: null pointer argument");
    if (const int rc = check_updates("fa_fedavg_fold", updates, K)) return rc;
    if (init && K == 1) {
        if (agg_dtype != upd_dtype) return fail(FA_EDTYPE, "fa_fedavg_fold: K=1 init is a copy; dtypes must match");
        hipError_t e = hipMemcpyAsync(agg, updates[0], (size_t)P * dt_size(upd_dtype), hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) return fail(FA_EHIP, "fa_fedavg_fold: hipMemcpyAsync: %s", hipGetErrorString(e));
        return FA_OK;
    }
    const bool int_first = init && (upd_dtype == FA_I64 || upd_dtype == FA_I32);
    // the first fold of integer updates multiplies in the integer dtype: numpy does that for an int
    // num_examples only (a float one multiplies in float64: fa_elementwise FA_EW_IFOLD)
    if (int_first && !(n[1] == std::floor(n[1]) && std::fabs(n[1]) < 0x1p63))
        return fail(FA_EINVAL, "fa_fedavg_fold: integer updates need an integral n[1] (got %g); a float "
                               "num_examples folds through fa_elementwise(FA_EW_IFOLD)", n[1]);
    // ... and in the update dtype: numpy refuses a python int outside it (OverflowError), it never wraps one
    if (int_first && upd_dtype == FA_I32 && !(n[1] >= -0x1p31 && n[1] < 0x1p31))
        return fail(FA_EINVAL, "fa_fedavg_fold: int32 updates need an n[1] within int32 (got %.17g); numpy "
                               "refuses that product (OverflowError)", n[1]);
    if (upd_dtype == FA_F32 && agg_dtype == FA_F32) return launch_fedavg<float, float, CF32>(agg, updates, n, N, K, P, init, false, st);
    if (upd_dtype == FA_BF16 && agg_dtype == FA_F32) return launch_fedavg<bf16, float, CF32>(agg, updates, n, N, K, P, init, false, st);
    if (upd_dtype == FA_F16 && agg_dtype == FA_F16) return launch_fedavg<f16, f16, CF16>(agg, updates, n, N, K, P, init, false, st);
    if (upd_dtype == FA_F64 && agg_dtype == FA_F64) return launch_fedavg<double, double, CF64>(agg, updates, n, N, K, P, init, false, st);
    if (upd_dtype == FA_F32 && agg_dtype == FA_F64) return launch_fedavg<float, double, CF64>(agg, updates, n, N, K, P, init, false, st);
    if (upd_dtype == FA_I64 && agg_dtype == FA_F64) return launch_fedavg<int64_t, double, CF64>(agg, updates, n, N, K, P, init, int_first, st);
    if (upd_dtype == FA_I32 && agg_dtype == FA_F64) return launch_fedavg<int32_t, double, CF64>(agg, updates, n, N, K, P, init, int_first, st);
    return fail(FA_EDTYPE, "fa_fedavg_fold: unsupported dtype pair (update %d, aggregate %d)", upd_dtype, agg_dtype);
}

// A small model's whole round in one call: the fold reads the packed updates and writes the model
// straight in page-locked host memory, through their device mappings, and the call returns with the
// model on the host. For mnist-sized models the copies, events and extra launches of the device path
// cost more than the bytes (configs[0]); the kernel and client table are fa_fedavg_fold's, so the bits
// are too.
int fa_fedavg_fold_host(void* agg, int agg_dtype, const void* const* updates, int upd_dtype, const double* n,
                        const double* N, int K, int64_t P, int init, void* stream) {
    g_err[0] = 0;
    if (P < 0 || K < 0) return fail(FA_EINVAL, "fa_fedavg_fold_host: negative size (P=%lld, K=%d)", (long long)P, K);
    if (K > kMaxK) return fail(FA_EINVAL, "fa_fedavg_fold_host: K=%d exceeds one launch (%d)", K, kMaxK);
    if (K == 0 || P == 0) return FA_OK;
    if (!agg || !updates) return fail(FA_EINVAL, "fa_fedavg_fold_host: null pointer argument");
    void* dev_agg = nullptr;
    const void* dev_upd[kMaxK];
    const hipError_t e = hipHostGetDevicePointer(&dev_agg, agg, 0);
    if (const int rc = map_host_updates("fa_fedavg_fold_host", e, updates, K, dev_upd)) return rc;
    return wait_host_round("fa_fedavg_fold_host",
                           fa_fedavg_fold(dev_agg, agg_dtype, dev_upd, upd_dtype, n, N, K, P, init, stream), stream);
}

int fa_weighted_sum(void* acc, int acc_dtype, const void* const* updates, int upd_dtype, const double* w, int K,
                    int64_t P, void* stream) {
    g_err[0] = 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (P < 0 || K < 0) return fail(FA_EINVAL, "fa_weighted_sum: negative size (P=%lld, K=%d)", (long long)P, K);
    if (K == 0 || P == 0) return FA_OK;
    if (!acc || !updates || !w) return fail(FA_EINVAL, "fa_weighted_sum: null pointer argument");
    if (const int rc = check_updates("fa_weighted_sum", updates, K)) return rc;
    // the client table's N is unused by the rule; pass w so fill_table reads valid memory
    if (upd_dtype == FA_F32 && acc_dtype == FA_F32) return launch_fedavg<float, float, CWSUM<float, float>>(acc, updates, w, w, K, P, 0, false, st);
    if (upd_dtype == FA_F32 && acc_dtype == FA_F64) return launch_fedavg<float, double, CWSUM<float, double>>(acc, updates, w, w, K, P, 0, false, st);
    if (upd_dtype == FA_F64 && acc_dtype == FA_F64) return launch_fedavg<double, double, CWSUM<double, double>>(acc, updates, w, w, K, P, 0, false, st);
    if (upd_dtype == FA_F64 && acc_dtype == FA_F32) return launch_fedavg<double, float, CWSUM<double, float>>(acc, updates, w, w, K, P, 0, false, st);
    return fail(FA_EDTYPE, "fa_weighted_sum: unsupported dtype pair (update %d, accumulator %d)", upd_dtype, acc_dtype);
}

int fa_running_mean(void* g, int dtype, const void* m, double a, double b, double T, int64_t P, void* stream) {
    g_err[0] = 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (P < 0) return fail(FA_EINVAL, "fa_running_mean: negative size");
    if (P == 0) return FA_OK;
    if (!g || !m) return fail(FA_EINVAL, "fa_running_mean: null pointer argument");
    const void* ups[1] = {m};
    const double bb[1] = {b}, TT[1] = {T};
    auto run = [&](auto tag) -> int {
        using T_ = decltype(tag);
        using CP = CRUN<T_>;
        constexpr int E = 16 / (int)sizeof(T_);
        ClientTable<double> tab;
        fill_table<double>(tab, ups, bb, TT, 0, 1);
        tab.r[0] = a;                                        // a = T - n rides in r[]
        T_* x = static_cast<T_*>(g);
        if (aligned16(g) && aligned16(m)) launch_fedavg_vec<T_, T_, CP, E>(x, tab, 1, P, false, false, st);
        else launch_fedavg_geom<T_, T_, CP, 1, 1, kUnroll, false>(x, tab, 1, P, false, false, st);
        return check_launch("fa_running_mean: kernel launch");
    };
    if (dtype == FA_F32) return run(float{});
    if (dtype == FA_F64) return run(double{});
    return fail(FA_EDTYPE, "fa_running_mean: unsupported dtype %d", dtype);
}

int fa_fedopt_step(const void* old, int old_dtype, const void* const* updates, int upd_dtype, const double* n,
                   const double* N, int K, void* pg, int flags, const void* m_in, int m_in_dtype, void* m_out,
                   const double* v_in, double* v_out, double* out, int serveropt, double lr, double beta1,
                   double beta2, double tau, int64_t P, void* stream) {
    // the reference's dtype flow: m as numpy promotes it, v and the model float64
    int pg_dt = (upd_dtype == FA_I32 || upd_dtype == FA_I64) ? FA_F64 : fa_promote(upd_dtype, old_dtype);
    const int m_out_dt = fa_promote(m_in ? m_in_dtype : FA_NONE, pg_dt);
    return fa_fedopt_step_ex(old, old_dtype, updates, upd_dtype, n, N, K, pg, flags, m_in, m_in_dtype, m_out,
                             m_out_dt, v_in, FA_F64, v_out, out, FA_F64, serveropt, lr, beta1, beta2, tau, P, stream);
}

int fa_fedopt_step_ex(const void* old, int old_dtype, const void* const* updates, int upd_dtype, const double* n,
                      const double* N, int K, void* pg, int flags, const void* m_in, int m_in_dtype, void* m_out,
                      int m_out_dtype, const void* v_in, int v_in_dtype, void* v_out, void* out, int state_dtype,
                      int serveropt, double lr, double beta1, double beta2, double tau, int64_t P, void* stream) {
    g_err[0] = 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (P < 0 || K < 0) return fail(FA_EINVAL, "fa_fedopt_step: negative size");
    if (P == 0) return FA_OK;
    const bool first = flags & FA_PG_FIRST, final_ = flags & FA_PG_FINAL;
    if (first && K < 1) return fail(FA_EINVAL, "fa_fedopt_step: FA_PG_FIRST requires K >= 1");
    if (!old) return fail(FA_EINVAL, "fa_fedopt_step: old is NULL");
    if (K > 0 && (!updates || !n || !N)) return fail(FA_EINVAL, "fa_fedopt_step: null client table");
    if (const int rc = check_updates("fa_fedopt_step", updates, K)) return rc;
    if ((!first || !final_ || K > kMaxK) && !pg) return fail(FA_EINVAL, "fa_fedopt_step: pg workspace required");
    if (final_ && (!m_out || !v_out || !out)) return fail(FA_EINVAL, "fa_fedopt_step: null output buffer");
    if (serveropt < FA_ADAM || serveropt > FA_ADAGRAD) return fail(FA_EINVAL, "fa_fedopt_step: unsupported serveropt %d", serveropt);
    auto is_int = [](int d) { return d == FA_I32 || d == FA_I64; };
    if (old_dtype != FA_F32 && old_dtype != FA_F64 && old_dtype != FA_F16 && !is_int(old_dtype))
        return fail(FA_EDTYPE, "fa_fedopt_step: old dtype %d", old_dtype);
    if (upd_dtype != FA_F32 && upd_dtype != FA_F64 && upd_dtype != FA_BF16 && upd_dtype != FA_F16 && !is_int(upd_dtype))
        return fail(FA_EDTYPE, "fa_fedopt_step: update dtype %d", upd_dtype);
    if (is_int(old_dtype) && !is_int(upd_dtype))
        return fail(FA_EDTYPE, "fa_fedopt_step: integer global model with float updates is unsupported");
    // integer tensors: subtract = next*1.0 + old*(-1.0) turns them into float64 (numpy: int * python float)
    const int pg_dt = is_int(upd_dtype) ? FA_F64 : fa_promote(upd_dtype, old_dtype);
    if (m_in && m_in_dtype != FA_F32 && m_in_dtype != FA_F64 && m_in_dtype != FA_F16)
        return fail(FA_EDTYPE, "fa_fedopt_step: m dtype %d", m_in_dtype);
    if (!m_in) m_in_dtype = FA_NONE;
    if (state_dtype != FA_F64 && state_dtype != FA_F32)
        return fail(FA_EDTYPE, "fa_fedopt_step_ex: state dtype %d (F64: the reference's, F32: fp32 state)", state_dtype);
    if (v_in && v_in_dtype != FA_F64 && v_in_dtype != FA_F32)
        return fail(FA_EDTYPE, "fa_fedopt_step_ex: v dtype %d", v_in_dtype);
    // m as numpy promotes it; in the fp32-state mode m may instead be stored as f32 (rounded once)
    const int m_np = fa_promote(m_in_dtype, pg_dt);
    const int m_out_dt = m_out_dtype;
    if (final_ && m_out_dt != m_np && !(state_dtype == FA_F32 && m_out_dt == FA_F32))
        return fail(FA_EDTYPE, "fa_fedopt_step_ex: m_out dtype %d (numpy gives %d%s)", m_out_dt, m_np,
                    state_dtype == FA_F32 ? "; F32 in the fp32-state mode" : "");
    auto mcode = [](int d) { return d == FA_NONE ? -1 : d == FA_F64 ? 1 : d == FA_F16 ? 2 : 0; };

    OptBuffers b{old, pg, m_in, m_out, v_in, v_out, out, mcode(m_in_dtype), mcode(final_ ? m_out_dt : m_np),
                 v_in && v_in_dtype == FA_F32, state_dtype == FA_F32, state_dtype == FA_F32};
    OptScalars s;
    s.lr = lr;
    s.b1 = beta1;
    s.b2 = beta2;
    s.tau = tau;
    s.tau2 = std::pow(tau, 2.0);   // math.pow(tau, 2)
    s.c1 = 1.0 - beta1;
    s.c2 = 1.0 - beta2;
    s.nc2 = -(1.0 - beta2);
    s.b1f = (float)beta1;
    s.c1f = (float)s.c1;
    // fedopt adam: p*(1-beta2); p has the pg dtype
    s.c2f = (float)s.c2;
    s.b1h = to_half_value(beta1);
    s.c1h = to_half_value(s.c1);
    s.c2h = to_half_value(s.c2);
    s.opt = serveropt;

    if (upd_dtype == FA_F32 && old_dtype == FA_F32) return launch_fedopt<float, float, CF32>(b, s, updates, n, N, K, P, flags, st);
    if (upd_dtype == FA_BF16 && old_dtype == FA_F32) return launch_fedopt<bf16, float, CF32>(b, s, updates, n, N, K, P, flags, st);
    if (upd_dtype == FA_F32 && old_dtype == FA_F64) return launch_fedopt<float, double, CF64>(b, s, updates, n, N, K, P, flags, st);
    if (upd_dtype == FA_F64 && old_dtype == FA_F64) return launch_fedopt<double, double, CF64>(b, s, updates, n, N, K, P, flags, st);
    if (upd_dtype == FA_BF16 && old_dtype == FA_F64) return launch_fedopt<bf16, double, CF64>(b, s, updates, n, N, K, P, flags, st);
    if (upd_dtype == FA_F64 && old_dtype == FA_F32) return launch_fedopt<double, float, CF64>(b, s, updates, n, N, K, P, flags, st);
    // float16 sessions (numpy's half loops for the pseudo-gradient while it is float16)
    if (upd_dtype == FA_F16 && old_dtype == FA_F16) return launch_fedopt<f16, f16, CF16>(b, s, updates, n, N, K, P, flags, st);
    if (upd_dtype == FA_F16 && old_dtype == FA_F32) return launch_fedopt<f16, float, CF32>(b, s, updates, n, N, K, P, flags, st);
    if (upd_dtype == FA_F16 && old_dtype == FA_F64) return launch_fedopt<f16, double, CF64>(b, s, updates, n, N, K, P, flags, st);
    if (upd_dtype == FA_F32 && old_dtype == FA_F16) return launch_fedopt<float, f16, CF32>(b, s, updates, n, N, K, P, flags, st);
    if (upd_dtype == FA_F64 && old_dtype == FA_F16) return launch_fedopt<double, f16, CF64>(b, s, updates, n, N, K, P, flags, st);
    if (upd_dtype == FA_I64 && old_dtype == FA_I64) return launch_fedopt<int64_t, int64_t, CF64>(b, s, updates, n, N, K, P, flags, st);
    if (upd_dtype == FA_I64 && old_dtype == FA_F64) return launch_fedopt<int64_t, double, CF64>(b, s, updates, n, N, K, P, flags, st);
    if (upd_dtype == FA_I64 && old_dtype == FA_F32) return launch_fedopt<int64_t, float, CF64>(b, s, updates, n, N, K, P, flags, st);
    if (upd_dtype == FA_I32 && old_dtype == FA_I32) return launch_fedopt<int32_t, int32_t, CF64>(b, s, updates, n, N, K, P, flags, st);
    if (upd_dtype == FA_I32 && old_dtype == FA_F64) return launch_fedopt<int32_t, double, CF64>(b, s, updates, n, N, K, P, flags, st);
    if (upd_dtype == FA_I32 && old_dtype == FA_F32) return launch_fedopt<int32_t, float, CF64>(b, s, updates, n, N, K, P, flags, st);
    return fail(FA_EDTYPE, "fa_fedopt_step: unsupported dtype pair (update %d, old %d)", upd_dtype, old_dtype);
}

// A small model's whole FedOpt round in one call (the FedOpt form of fa_fedavg_fold_host): the global
// model, the packed updates and the new model in page-locked host memory, read and written through
// their device mappings; m / v in HBM. One FIRST | FINAL launch (the pseudo-gradient in registers,
// then the server step), then the stream wait.
int fa_fedopt_step_host(const void* old, int old_dtype, const void* const* updates, int upd_dtype, const double* n,
                        const double* N, int K, const void* m_in, int m_in_dtype, void* m_out, int m_out_dtype,
                        const void* v_in, int v_in_dtype, void* v_out, void* out, int state_dtype, int serveropt,
                        double lr, double beta1, double beta2, double tau, int64_t P, void* stream) {
    g_err[0] = 0;
    if (P < 0 || K < 1 || K > kMaxK)
        return fail(FA_EINVAL, "fa_fedopt_step_host: 1 <= K <= %d updates in one launch (K=%d, P=%lld)", kMaxK, K,
                    (long long)P);
    if (P == 0) return FA_OK;
    if (!old || !updates || !out) return fail(FA_EINVAL, "fa_fedopt_step_host: null pointer argument");
    void* dev_old = nullptr;
    void* dev_out = nullptr;
    const void* dev_upd[kMaxK];
    hipError_t e = hipHostGetDevicePointer(&dev_old, const_cast<void*>(old), 0);
    if (e == hipSuccess) e = hipHostGetDevicePointer(&dev_out, out, 0);
    if (const int rc = map_host_updates("fa_fedopt_step_host", e, updates, K, dev_upd)) return rc;
    const int rc = fa_fedopt_step_ex(dev_old, old_dtype, dev_upd, upd_dtype, n, N, K, nullptr, FA_PG_FIRST | FA_PG_FINAL,
                                     m_in, m_in_dtype, m_out, m_out_dtype, v_in, v_in_dtype, v_out, dev_out, state_dtype,
                                     serveropt, lr, beta1, beta2, tau, P, stream);
    return wait_host_round("fa_fedopt_step_host", rc, stream);
}

int fa_elementwise(int op, void* out, int out_dtype, const void* x, int x_dtype, const void* y, int y_dtype,
                   double a, double b, int64_t P, void* stream) {
    g_err[0] = 0;
    if (P < 0 || !out || (op != FA_EW_FILL && !x)) return fail(FA_EINVAL, "fa_elementwise: bad arguments");
    if (op < FA_EW_AXPBY || op > FA_EW_NFOLD) return fail(FA_EINVAL, "fa_elementwise: unknown op %d", op);
    if (op == FA_EW_AXPBY && !y) return fail(FA_EINVAL, "fa_elementwise: AXPBY needs y");
    if (P == 0) return FA_OK;
    const dim3 grid = elementwise_grid(P);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (op == FA_EW_IPOW) {
        if (out_dtype != x_dtype)
            return fail(FA_EDTYPE, "fa_elementwise: IPOW returns its input's dtype");
        if (!(a >= 0.0) || a != std::floor(a) || a > 0x1p63)
            return fail(FA_EINVAL, "fa_elementwise: IPOW exponent must be a non-negative integer");
        auto run = [&](auto tag) -> int {
            using T = decltype(tag);
            hipLaunchKernelGGL(k_ipow<T>, grid, dim3(kBlock), 0, st, static_cast<T*>(out), static_cast<const T*>(x),
                               (uint64_t)a, P);
            return check_launch("fa_elementwise");
        };
        return for_int_dtype(x_dtype, run, "fa_elementwise: IPOW takes an integer array, got dtype %d");
    }
    if (op == FA_EW_IFOLD || op == FA_EW_NFOLD) {
        if (!y || out_dtype != FA_F64 || x_dtype != y_dtype)
            return fail(FA_EDTYPE, "fa_elementwise: IFOLD / NFOLD take two arrays of one integer dtype and return float64");
        if (op == FA_EW_NFOLD && !(std::fabs(a) < 0x1p53 && a == std::floor(a)))
            return fail(FA_EINVAL, "fa_elementwise: NFOLD num_examples must be an integer below 2^53 in magnitude");
        auto run = [&](auto tag) -> int {
            using T = decltype(tag);
            using U = typename std::make_unsigned<T>::type;
            if (op == FA_EW_IFOLD)
                hipLaunchKernelGGL(k_ifold<T>, grid, dim3(kBlock), 0, st, static_cast<double*>(out),
                                   static_cast<const T*>(x), static_cast<const T*>(y), a, b, P);
            else
                hipLaunchKernelGGL(k_nfold<T>, grid, dim3(kBlock), 0, st, static_cast<double*>(out),
                                   static_cast<const T*>(x), static_cast<const T*>(y), (T)(U)(int64_t)a, b, P);
            return check_launch("fa_elementwise");
        };
        return for_int_dtype(x_dtype, run, "fa_elementwise: IFOLD / NFOLD need an integer dtype, got %d");
    }
    if (op == FA_EW_AXPBY && x_dtype == FA_F16 && y_dtype == FA_F16 && out_dtype == FA_F16) {
        hipLaunchKernelGGL(k_axpby_half, grid, dim3(kBlock), 0, st, static_cast<f16*>(out),
                           static_cast<const f16*>(x), static_cast<const f16*>(y), to_half_value(a), to_half_value(b), P);
        return check_launch("fa_elementwise");
    }
    auto isf = [](int d) { return d == FA_F32 || d == FA_F64; };
    if (op == FA_EW_FILL) x_dtype = out_dtype;
    if (!y) y_dtype = x_dtype;
    if (!isf(out_dtype) || !isf(x_dtype) || !isf(y_dtype)) return fail(FA_EDTYPE, "fa_elementwise: f32/f64 only");
    const int want = (op == FA_EW_FILL) ? out_dtype
                     : (op == FA_EW_AXPBY || ((op == FA_EW_MUL || op == FA_EW_DIV) && y)) ? fa_promote(x_dtype, y_dtype)
                     : x_dtype;
    if (out_dtype != want) return fail(FA_EDTYPE, "fa_elementwise: output dtype must be %d", want);
    // np.power(x32, a): the python float is a weak scalar, so numpy raises to float32(a)
    if (op == FA_EW_POW && x_dtype == FA_F32) a = (double)(float)a;
#define FA_EW(TX, TY, TO) \
    hipLaunchKernelGGL((k_elementwise<TX, TY, TO>), grid, dim3(kBlock), 0, st, op, static_cast<TO*>(out), \
                       static_cast<const TX*>(x), static_cast<const TY*>(y), a, b, P)
    const bool x32 = x_dtype == FA_F32, y32 = y_dtype == FA_F32, o32 = out_dtype == FA_F32;
    if (x32 && y32 && o32) FA_EW(float, float, float);
    else if (x32 && y32) FA_EW(float, float, double);
    else if (x32) FA_EW(float, double, double);
    else if (y32) FA_EW(double, float, double);
    else FA_EW(double, double, double);
#undef FA_EW
    return check_launch("fa_elementwise");
}

int64_t fa_norm1_work(int64_t rows, int64_t cols, int matrix) {
    return matrix ? std::max<int64_t>(cols, 1) : kNormBlocks;
}

int fa_norm1(double* out, const void* x, int dtype, int64_t rows, int64_t cols, int matrix, double* work,
             void* stream) {
    g_err[0] = 0;
    if (!out || !work || rows < 0 || cols < 0 || (rows * cols > 0 && !x)) return fail(FA_EINVAL, "fa_norm1: bad arguments");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t P = rows * cols;
    auto run = [&](auto tag) -> int {
        using T = decltype(tag);
        const T* xp = static_cast<const T*>(x);
        if (matrix) {
            if (cols > 0)
                hipLaunchKernelGGL(k_colabssum<T>, dim3((unsigned)std::min<int64_t>((cols + kBlock - 1) / kBlock, 4096)),
                                   dim3(kBlock), 0, st, xp, rows, cols, work);
            hipLaunchKernelGGL(k_final_reduce, dim3(1), dim3(kBlock), 0, st, work, cols, 1, out);
        } else {
            hipLaunchKernelGGL(k_abssum_partial<T>, dim3(kNormBlocks), dim3(kBlock), 0, st, xp, P, work);
            hipLaunchKernelGGL(k_final_reduce, dim3(1), dim3(kBlock), 0, st, work, (int64_t)kNormBlocks, 0, out);
        }
        return check_launch("fa_norm1");
    };
    if (dtype == FA_F32) return run(float{});
    if (dtype == FA_F64) return run(double{});
    return for_int_dtype(dtype, run, "fa_norm1: dtype %d");
}

int fa_cast(void* out, int out_dtype, const void* in, int in_dtype, int ndim, const int64_t* out_shape,
            const int64_t* in_strides, void* stream) {
    g_err[0] = 0;
    if (!out_shape || !in_strides) return fail(FA_EINVAL, "fa_cast: null shape or strides");
    if (ndim < 1 || ndim > kCastMaxDim) return fail(FA_EINVAL, "fa_cast: ndim must be 1..%d, got %d", kCastMaxDim, ndim);
    CastGeom g;
    g.ndim = ndim;
    int64_t P = 1, cstride = 1;
    bool bc = false;
    for (int d = ndim - 1; d >= 0; --d) {
        if (out_shape[d] < 0) return fail(FA_EINVAL, "fa_cast: negative dimension");
        g.shape[d] = out_shape[d];
        g.stride[d] = in_strides[d];
        if (out_shape[d] != 1 && in_strides[d] != cstride) bc = true;   // not the contiguous identity map
        cstride *= out_shape[d];
    }
    for (int d = 0; d < ndim; ++d) P *= out_shape[d];
    if (P == 0) return FA_OK;
    if (!out || !in) return fail(FA_EINVAL, "fa_cast: null buffer");
    const dim3 grid((unsigned)std::min<int64_t>((P + kBlock - 1) / kBlock, 16384));
    hipStream_t st = static_cast<hipStream_t>(stream);
#define FA_CAST(DI, TI, DO, TO)                                                                                     \
    if (in_dtype == DI && out_dtype == DO) {                                                                        \
        if (bc) hipLaunchKernelGGL((k_cast<TI, TO, true>), grid, dim3(kBlock), 0, st, static_cast<TO*>(out),        \
                                   static_cast<const TI*>(in), g, P);                                                \
        else hipLaunchKernelGGL((k_cast<TI, TO, false>), grid, dim3(kBlock), 0, st, static_cast<TO*>(out),          \
                                static_cast<const TI*>(in), g, P);                                                   \
        return check_launch("fa_cast");                                                                             \
    }
    FA_CAST(FA_F32, float, FA_F32, float)
    FA_CAST(FA_F64, double, FA_F64, double)
    FA_CAST(FA_F32, float, FA_F16, f16)      // narrowing float casts (numpy astype: round to nearest even):
    FA_CAST(FA_F64, double, FA_F32, float)   // the result of a float16 / float32 helper op computed wider
    FA_CAST(FA_F16, f16, FA_F16, f16)
    FA_CAST(FA_BF16, bf16, FA_BF16, bf16)
    FA_CAST(FA_I32, int32_t, FA_I32, int32_t)
    FA_CAST(FA_I64, int64_t, FA_I64, int64_t)
    FA_CAST(FA_F16, f16, FA_F32, float)
    FA_CAST(FA_F16, f16, FA_F64, double)
    FA_CAST(FA_BF16, bf16, FA_F32, float)
    FA_CAST(FA_BF16, bf16, FA_F64, double)
    FA_CAST(FA_F32, float, FA_F64, double)
    FA_CAST(FA_I32, int32_t, FA_I64, int64_t)
    FA_CAST(FA_I32, int32_t, FA_F64, double)
    FA_CAST(FA_I64, int64_t, FA_F64, double)
    // narrow / unsigned integers: identity (broadcast) and numpy's safe widenings
    FA_CAST(FA_I8, int8_t, FA_I8, int8_t)
    FA_CAST(FA_I8, int8_t, FA_I16, int16_t)
    FA_CAST(FA_I8, int8_t, FA_I32, int32_t)
    FA_CAST(FA_I8, int8_t, FA_I64, int64_t)
    FA_CAST(FA_I8, int8_t, FA_F16, f16)
    FA_CAST(FA_I8, int8_t, FA_F32, float)
    FA_CAST(FA_I8, int8_t, FA_F64, double)
    FA_CAST(FA_U8, uint8_t, FA_U8, uint8_t)
    FA_CAST(FA_U8, uint8_t, FA_I16, int16_t)
    FA_CAST(FA_U8, uint8_t, FA_U16, uint16_t)
    FA_CAST(FA_U8, uint8_t, FA_I32, int32_t)
    FA_CAST(FA_U8, uint8_t, FA_U32, uint32_t)
    FA_CAST(FA_U8, uint8_t, FA_I64, int64_t)
    FA_CAST(FA_U8, uint8_t, FA_U64, uint64_t)
    FA_CAST(FA_U8, uint8_t, FA_F16, f16)
    FA_CAST(FA_U8, uint8_t, FA_F32, float)
    FA_CAST(FA_U8, uint8_t, FA_F64, double)
    FA_CAST(FA_I16, int16_t, FA_I16, int16_t)
    FA_CAST(FA_I16, int16_t, FA_I32, int32_t)
    FA_CAST(FA_I16, int16_t, FA_I64, int64_t)
    FA_CAST(FA_I16, int16_t, FA_F32, float)
    FA_CAST(FA_I16, int16_t, FA_F64, double)
    FA_CAST(FA_U16, uint16_t, FA_U16, uint16_t)
    FA_CAST(FA_U16, uint16_t, FA_I32, int32_t)
    FA_CAST(FA_U16, uint16_t, FA_U32, uint32_t)
    FA_CAST(FA_U16, uint16_t, FA_I64, int64_t)
    FA_CAST(FA_U16, uint16_t, FA_U64, uint64_t)
    FA_CAST(FA_U16, uint16_t, FA_F32, float)
    FA_CAST(FA_U16, uint16_t, FA_F64, double)
    FA_CAST(FA_U32, uint32_t, FA_U32, uint32_t)
    FA_CAST(FA_U32, uint32_t, FA_I64, int64_t)
    FA_CAST(FA_U32, uint32_t, FA_U64, uint64_t)
    FA_CAST(FA_U32, uint32_t, FA_F64, double)
    FA_CAST(FA_U64, uint64_t, FA_U64, uint64_t)
    FA_CAST(FA_U64, uint64_t, FA_F64, double)
#undef FA_CAST
    return fail(FA_EDTYPE, "fa_cast: unsupported conversion %d -> %d", in_dtype, out_dtype);
}

// ----------------------------------------------------------------------------
// peer transport of the parameter-sliced all-gather (sharded.P2PAllGather,
// multidev.allgather_devices): IPC mappings of the peers' model buffers and DMA copies into them
// ----------------------------------------------------------------------------
static_assert(sizeof(hipIpcMemHandle_t) <= FA_IPC_HANDLE_BYTES, "IPC handle size");

int fa_ipc_get_handle(const void* dptr, void* handle, uint64_t* offset) {
    g_err[0] = 0;
    if (!dptr || !handle || !offset) return fail(FA_EINVAL, "fa_ipc_get_handle: null argument");
    // a handle names a whole allocation (a caching allocator hands out pieces of one): export the
    // allocation's base and the piece's offset in it
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    hipError_t e = hipMemGetAddressRange(&base, &size, const_cast<void*>(dptr));
    if (e != hipSuccess) return fail(FA_EHIP, "fa_ipc_get_handle: hipMemGetAddressRange: %s", hipGetErrorString(e));
    hipIpcMemHandle_t h;
    e = hipIpcGetMemHandle(&h, base);
    if (e != hipSuccess) return fail(FA_EHIP, "fa_ipc_get_handle: hipIpcGetMemHandle: %s", hipGetErrorString(e));
    std::memset(handle, 0, FA_IPC_HANDLE_BYTES);
    std::memcpy(handle, &h, sizeof(h));
    *offset = (uint64_t)(static_cast<const char*>(dptr) - static_cast<const char*>(base));
    return FA_OK;
}

int fa_ipc_open(const void* handle, uint64_t offset, void** base, void** dptr) {
    g_err[0] = 0;
    if (!handle || !base || !dptr) return fail(FA_EINVAL, "fa_ipc_open: null argument");
    hipIpcMemHandle_t h;
    std::memcpy(&h, handle, sizeof(h));
    void* b = nullptr;
    hipError_t e = hipIpcOpenMemHandle(&b, h, hipIpcMemLazyEnablePeerAccess);
    if (e != hipSuccess) return fail(FA_EHIP, "fa_ipc_open: hipIpcOpenMemHandle: %s", hipGetErrorString(e));
    *base = b;
    *dptr = static_cast<char*>(b) + offset;
    return FA_OK;
}

int fa_ipc_close(void* base) {
    g_err[0] = 0;
    if (!base) return FA_OK;
    hipError_t e = hipIpcCloseMemHandle(base);
    if (e != hipSuccess) return fail(FA_EHIP, "fa_ipc_close: %s", hipGetErrorString(e));
    return FA_OK;
}

int fa_copy_async(void* dst, const void* src, int64_t bytes, void* stream) {
    g_err[0] = 0;
    if (bytes < 0 || (bytes > 0 && (!dst || !src))) return fail(FA_EINVAL, "fa_copy_async: bad arguments");
    if (bytes == 0) return FA_OK;
    hipError_t e = hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDefault, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(FA_EHIP, "fa_copy_async: %s", hipGetErrorString(e));
    return FA_OK;
}

int fa_fedavg_fold_push(float* agg, const void* const* updates, const double* n, const double* N, int K, int64_t P,
                        int init, void* const* dsts, int ndst, uint32_t* release_rec, void* stream) {
    g_err[0] = 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (P < 0 || K < 0 || ndst < 0 || ndst > kPushMax)
        return fail(FA_EINVAL, "fa_fedavg_fold_push: bad sizes (P=%lld, K=%d, ndst=%d <= %d)", (long long)P, K, ndst,
                    kPushMax);
    if (init && K < 1) return fail(FA_EINVAL, "fa_fedavg_fold_push: init requires K >= 1");
    if (K == 0 || P == 0) return FA_OK;
    if (!agg || !updates || !n || !N || (ndst > 0 && !dsts)) return fail(FA_EINVAL, "fa_fedavg_fold_push: null pointer argument");
    if (!aligned16(agg)) return fail(FA_EINVAL, "fa_fedavg_fold_push: agg not 16-B aligned");
    PushTable t{};
    for (int d = 0; d < ndst; ++d) {
        if (!dsts[d] || !aligned16(dsts[d])) return fail(FA_EINVAL, "fa_fedavg_fold_push: destination %d null or not 16-B aligned", d);
        t.dst[d] = static_cast<u32x4*>(dsts[d]);
    }
    for (int k = 0; k < K; ++k)
        if (!updates[k] || !aligned16(updates[k])) return fail(FA_EINVAL, "fa_fedavg_fold_push: updates[%d] null or not 16-B aligned", k);
    // clients beyond one kernarg table fold first (plain launches); the last table's launch pushes
    const int last0 = ((K - 1) / kMaxK) * kMaxK;
    if (last0 > 0) {
        const int rc = fa_fedavg_fold(agg, FA_F32, updates, FA_F32, n, N, last0, P, init, stream);
        if (rc) return rc;
    }
    ClientTable<CF32::S> tab;
    const int cnt = K - last0;
    fill_table<CF32::S>(tab, updates, n, N, last0, cnt);
    const bool first = init && last0 == 0;
    const dim3 grid((unsigned)((P + 4 * (int64_t)kBlock - 1) / (4 * (int64_t)kBlock)));
    if (cnt <= 8) {
        if (first) hipLaunchKernelGGL((k_fedavg_push<8, true>), grid, dim3(kBlock), 0, st, agg, tab, cnt, P, t, ndst);
        else hipLaunchKernelGGL((k_fedavg_push<8, false>), grid, dim3(kBlock), 0, st, agg, tab, cnt, P, t, ndst);
    } else {
        if (first) hipLaunchKernelGGL((k_fedavg_push<4, true>), grid, dim3(kBlock), 0, st, agg, tab, cnt, P, t, ndst);
        else hipLaunchKernelGGL((k_fedavg_push<4, false>), grid, dim3(kBlock), 0, st, agg, tab, cnt, P, t, ndst);
    }
    const int rc = check_launch("fa_fedavg_fold_push: kernel launch");
    return rc ? rc : (ndst > 0 ? launch_release(st, release_rec) : FA_OK);
}

int fa_push(void* const* dsts, int ndst, const void* src, int64_t bytes, uint32_t* release_rec, void* stream) {
    g_err[0] = 0;
    if (ndst < 0 || ndst > kPushMax || bytes < 0 || (bytes > 0 && (!src || (ndst > 0 && !dsts))))
        return fail(FA_EINVAL, "fa_push: bad arguments (at most %d destinations)", kPushMax);
    if (bytes == 0 || ndst == 0) return FA_OK;
    PushTable t{};
    for (int d = 0; d < ndst; ++d) {
        if (!dsts[d]) return fail(FA_EINVAL, "fa_push: destination %d is null", d);
        if (reinterpret_cast<uintptr_t>(dsts[d]) % 16) return fail(FA_EINVAL, "fa_push: destination %d not 16-B aligned", d);
        t.dst[d] = static_cast<u32x4*>(dsts[d]);
    }
    if (reinterpret_cast<uintptr_t>(src) % 16) return fail(FA_EINVAL, "fa_push: source not 16-B aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t n16 = bytes / 16;
    const int rem = (int)(bytes % 16);
    if (n16 > 0) {
        // link-bound, not HBM-bound: a few hundred workgroups keep every link's writes in flight and
        // leave most of the chip to the fold running beside it
        const int64_t need = (n16 + (int64_t)kBlock * kPushWords - 1) / ((int64_t)kBlock * kPushWords);
        const int grid = (int)std::min<int64_t>(need, 512);
        hipLaunchKernelGGL(k_push, dim3(grid), dim3(kBlock), 0, st, t, ndst, static_cast<const u32x4*>(src), n16);
    }
    if (rem > 0)
        hipLaunchKernelGGL(k_push_tail, dim3(1), dim3(64), 0, st, t, ndst, static_cast<const uint8_t*>(src), n16 * 16,
                           rem);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(FA_EHIP, "fa_push: %s", hipGetErrorString(e));
    return launch_release(st, release_rec);
}

int fa_device_xccs(int dev, int* n) {
    g_err[0] = 0;
    if (!n) return fail(FA_EINVAL, "fa_device_xccs: null argument");
    return device_xccs(dev, n);
}

int fa_host_device_ptr(const void* host, void** dptr) {
    g_err[0] = 0;
    if (!host || !dptr) return fail(FA_EINVAL, "fa_host_device_ptr: null argument");
    void* d = nullptr;
    hipError_t e = hipHostGetDevicePointer(&d, const_cast<void*>(host), 0);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(FA_EHIP, "fa_host_device_ptr: %s (not page-locked host memory?)", hipGetErrorString(e));
    }
    *dptr = d;
    return FA_OK;
}

int fa_host_register(void* p, int64_t bytes) {
    g_err[0] = 0;
    if (!p || bytes <= 0) return fail(FA_EINVAL, "fa_host_register: bad arguments");
    hipError_t e = hipHostRegister(p, (size_t)bytes, hipHostRegisterPortable);
    if (e != hipSuccess) return fail(FA_EHIP, "fa_host_register: %s", hipGetErrorString(e));
    return FA_OK;
}

int fa_host_unregister(void* p) {
    g_err[0] = 0;
    if (!p) return FA_OK;
    hipError_t e = hipHostUnregister(p);
    if (e != hipSuccess) return fail(FA_EHIP, "fa_host_unregister: %s", hipGetErrorString(e));
    return FA_OK;
}

int fa_peer_enable(int dev, int peer) {
    g_err[0] = 0;
    if (dev == peer) return FA_OK;
    int can = 0;
    hipError_t e = hipDeviceCanAccessPeer(&can, dev, peer);
    if (e != hipSuccess) return fail(FA_EHIP, "fa_peer_enable: hipDeviceCanAccessPeer: %s", hipGetErrorString(e));
    if (!can) return fail(FA_EHIP, "fa_peer_enable: device %d cannot access device %d", dev, peer);
    int cur = 0;
    (void)hipGetDevice(&cur);
    e = hipSetDevice(dev);
    if (e == hipSuccess) e = hipDeviceEnablePeerAccess(peer, 0);
    (void)hipSetDevice(cur);
    if (e == hipErrorPeerAccessAlreadyEnabled) {
        (void)hipGetLastError();
        return FA_OK;
    }
    if (e != hipSuccess) return fail(FA_EHIP, "fa_peer_enable(%d -> %d): %s", dev, peer, hipGetErrorString(e));
    return FA_OK;
}

int fa_trimmed_mean(void* out, int out_dtype, const void* const* updates, int upd_dtype, int K, int trim, int64_t P,
                    void* stream) {
    g_err[0] = 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (const int rc = check_sort_ptrs("fa_trimmed_mean", out, updates, K)) return rc;
    if (trim < 0 || 2 * trim >= K) return fail(FA_EINVAL, "fa_trimmed_mean: trim=%d leaves nothing of K=%d", trim, K);
    if (const int rc = check_sort_size("fa_trimmed_mean", out_dtype, upd_dtype, P)) return rc;
    if (P == 0) return FA_OK;
    if (const int rc = check_updates("fa_trimmed_mean", updates, K)) return rc;
    return for_dtype(upd_dtype, [&](auto t) { return launch_order_mean<decltype(t)>(out, updates, K, trim, P, st); });
}

int fa_median_window_mean(void* out, int out_dtype, const void* const* updates, int upd_dtype, int K, int keep,
                          int64_t P, void* stream) {
    g_err[0] = 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (const int rc = check_sort_ptrs("fa_median_window_mean", out, updates, K)) return rc;
    if (keep < 1 || keep > K) return fail(FA_EINVAL, "fa_median_window_mean: keep=%d outside 1..K=%d", keep, K);
    if (const int rc = check_sort_size("fa_median_window_mean", out_dtype, upd_dtype, P)) return rc;
    if (P == 0) return FA_OK;
    if (const int rc = check_updates("fa_median_window_mean", updates, K)) return rc;
    return for_dtype(upd_dtype,
                     [&](auto t) { return launch_median_window<decltype(t)>(out, updates, K, keep, P, st); });
}

int64_t fa_pairwise_sqdist_work(int K, int64_t P) {
    if (K < 1 || K > kMaxK || P < 0) return 0;
    int64_t n = 0;
    pair_for_kp<double>(K, [&](auto gm) -> int {        // the f64 family's tile is the smaller one: most workgroups
        using GM = decltype(gm);
        n = pair_workgroups(P, GM::TE) * GM::PART;
        return FA_OK;
    });
    return std::max<int64_t>(n, 1);
}

int fa_pairwise_sqdist(double* D, const void* const* updates, int upd_dtype, int K, int64_t P, int accumulate,
                       double* work, void* stream) {
    g_err[0] = 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!D || !updates || !work) return fail(FA_EINVAL, "fa_pairwise_sqdist: null pointer argument");
    if (K < 1 || K > kMaxK) return fail(FA_EINVAL, "fa_pairwise_sqdist: K=%d outside 1..%d", K, kMaxK);
    if (P < 0) return fail(FA_EINVAL, "fa_pairwise_sqdist: negative size (P=%lld)", (long long)P);
    const int fam = pair_family(upd_dtype);
    if (!fam) return fail(FA_EDTYPE, "fa_pairwise_sqdist: unsupported dtype %d", upd_dtype);
    if (P > 0)                                               // (an empty buffer may be a null pointer)
        if (const int rc = check_updates("fa_pairwise_sqdist", updates, K)) return rc;
    if (accumulate && (P == 0 || K == 1)) return FA_OK;      // nothing to add: no launch
    if (fam == 32) return launch_pair_sqdist<float>(D, updates, upd_dtype, K, P, accumulate, work, st);
    return launch_pair_sqdist<double>(D, updates, upd_dtype, K, P, accumulate, work, st);
}


int64_t fa_wmean_sqdist_work(int K, int64_t P) {
    if (K < 1 || K > kMaxK || P < 0) return 0;
    // f64 updates: the smallest tile and the largest grid, so the most workgroups; kMaxK doubles per workgroup
    return std::max<int64_t>(wm_workgroups(P, wm_geom_dt(FA_F64, K, K)) * kMaxK, 1);
}

int fa_weighted_mean_sqdist(void* out, int out_dtype, double* dist, const void* const* updates, int upd_dtype,
                            const double* beta, int K, int64_t P, int accumulate, double* work, void* stream) {
    g_err[0] = 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    double bc[kMaxK];
    if (const int rc = wm_check_step("fa_weighted_mean_sqdist", "beta", "give a mean", dist && beta && updates && work,
                                     out_dtype, upd_dtype, beta, K, P, bc))
        return rc;
    int kfirst = 0;
    while (kfirst < K && bc[kfirst] == 0.0) ++kfirst;
    if (kfirst == K) return fail(FA_EINVAL, "fa_weighted_mean_sqdist: every weight is zero in the compute type");
    if (P > 0)                                               // (an empty buffer may be a null pointer)
        if (const int rc = check_updates("fa_weighted_mean_sqdist", updates, K)) return rc;
    if (accumulate && P == 0) return FA_OK;                  // nothing to add: no launch
    return for_dtype(upd_dtype, [&](auto t) {
        return launch_wmean_dist<decltype(t)>(out, dist, updates, bc, kfirst, K, P, accumulate, work, st);
    });
}

int64_t fa_centered_clip_work(int K, int64_t P) {
    if (K < 1 || K > kMaxK || P < 0) return 0;
    // f64 updates again: of the six dtypes they have the smallest tile (8-byte values) and the largest grid
    // (four waves a SIMD at every K), so no other dtype has more workgroups at any (K, P)
    return std::max<int64_t>(wm_workgroups(P, wm_geom_dt(FA_F64, K, K + 1)) * kMaxK, 1);
}

int fa_centered_clip_step(void* out, const void* center, int out_dtype, double* dist, const void* const* updates,
                          int upd_dtype, const double* coef, int K, int64_t P, int accumulate, double* work, void* stream) {
    g_err[0] = 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    double cc[kMaxK];
    if (const int rc = wm_check_step("fa_centered_clip_step", "coef", "move a centre",
                                     dist && center && coef && updates && work, out_dtype, upd_dtype, coef, K, P, cc))
        return rc;
    if (out && out != center && P > 0) {                     // in place or disjoint, nothing between
        const uintptr_t a = reinterpret_cast<uintptr_t>(out), b = reinterpret_cast<uintptr_t>(center);
        const uintptr_t len = (uintptr_t)P * dt_size(out_dtype);
        if (a < b + len && b < a + len)
            return fail(FA_EINVAL, "fa_centered_clip_step: out and center overlap without being the same buffer");
    }
    if (P > 0)                                               // (an empty buffer may be a null pointer)
        if (const int rc = check_updates("fa_centered_clip_step", updates, K)) return rc;
    if (accumulate && P == 0) return FA_OK;                  // nothing to add: no launch
    return for_dtype(upd_dtype, [&](auto t) {
        return launch_cclip_dist<decltype(t)>(out, center, dist, updates, cc, K, P, accumulate, work, st);
    });
}

int fa_clip_fold(void* out, int out_dtype, void* carry_out, const void* carry_in, const void* center,
                 const void* const* updates, int upd_dtype, const double* coef, int K, int64_t P, void* stream) {
    g_err[0] = 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    double cc[kMaxK];
    if (const int rc = wm_check_step("fa_clip_fold", "coef", "move a centre", (out || carry_out) && center && coef && updates,
                                     out_dtype, upd_dtype, coef, K, P, cc))
        return rc;
    if (P == 0) return FA_OK;                                // (an empty buffer may be a null pointer)
    const size_t csize = pair_family(upd_dtype) == 32 ? 4 : 8;
    if (const int rc = clip_fold_check_overlap(out, carry_out, carry_in, center, updates, K, P, dt_size(out_dtype), csize,
                                               dt_size(upd_dtype)))
        return rc;
    if (const int rc = check_updates("fa_clip_fold", updates, K)) return rc;
    return for_dtype(upd_dtype, [&](auto t) {
        return launch_clip_fold<decltype(t)>(out, carry_out, carry_in, center, updates, cc, K, P, st);
    });
}

int fa_gaussian_noise(void* out, const void* x, int dtype, double sigma, uint64_t seed, uint32_t stream_id,
                      uint32_t round_id, int64_t offset, int64_t P, void* stream) {
    g_err[0] = 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (P < 0 || offset < 0) return fail(FA_EINVAL, "fa_gaussian_noise: negative size or offset (P=%lld, offset=%lld)",
                                         (long long)P, (long long)offset);
    if (offset > INT64_MAX - P)
        return fail(FA_EINVAL, "fa_gaussian_noise: offset + P passes 2^63 - 1 (offset=%lld, P=%lld)", (long long)offset,
                    (long long)P);
    if (!out && P > 0) return fail(FA_EINVAL, "fa_gaussian_noise: out is NULL");
    if (!(sigma >= 0.0) || !std::isfinite(sigma))
        return fail(FA_EINVAL, "fa_gaussian_noise: sigma must be finite and >= 0 (got %g)", sigma);
    if (dtype != FA_F32 && dtype != FA_F64 && dtype != FA_F16)
        return fail(FA_EDTYPE, "fa_gaussian_noise: dtype %d (float32, float64 or float16)", dtype);
    if (x && x != out && P > 0) {                            // in place or disjoint, nothing between
        const uintptr_t a = reinterpret_cast<uintptr_t>(out), b = reinterpret_cast<uintptr_t>(x);
        const uintptr_t len = (uintptr_t)P * dt_size(dtype);
        if (a < b + len && b < a + len)
            return fail(FA_EINVAL, "fa_gaussian_noise: out and x overlap without being the same buffer");
    }
    if (P == 0) return FA_OK;
    if (dtype == FA_F32) return launch_gaussian_noise<float>(out, x, sigma, seed, stream_id, round_id, offset, P, st);
    if (dtype == FA_F64) return launch_gaussian_noise<double>(out, x, sigma, seed, stream_id, round_id, offset, P, st);
    return launch_gaussian_noise<f16>(out, x, sigma, seed, stream_id, round_id, offset, P, st);
}

#ifdef FEDAGG_PROBES
#include "probes_abi.h"       // fa_tune, fa_stream_*, the *_geometry queries (include/fedagg_probe.h)
#endif

}  // extern "C"
