// Stand-alone host program: the two step entry points' validation (and the helpers under it) under
// AddressSanitizer + UBSan, host code only. Bad arguments, P = 0, the *_work sizes and the geometry queries.
// It needs no GPU (nothing it checks reaches a kernel; the two P = 0 launches report "no device") and is not
// part of the build or the tests. From tools/:
//     hipcc -O1 -g -std=c++17 -ffp-contract=off -Wall --offload-arch=gfx950 -DFEDAGG_PROBES \
//         -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -Xarch_host -fno-omit-frame-pointer -o /tmp/step_checks asan_step_checks.hip
//     ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 /tmp/step_checks
// profiles/r21_distbody_asan_host.log is its output (r18_bulyan_asan_host.log: before fa_trimmed_mean's refusals
// and the pointer-table fill; r17_hostfold_asan_host.log: before fa_median_window_mean).
#include "../fedn_amd/csrc/fedagg.hip"

#include <cstdlib>

static int g_bad = 0;

static void expect(const char* what, int rc, int want_rc, const char* want_text) {
    const char* err = fa_last_error();
    const bool ok = rc == want_rc && (!want_text || std::strstr(err, want_text));
    std::printf("%s %-46s rc=%d  \"%s\"\n", ok ? "ok  " : "FAIL", what, rc, err);
    if (!ok) ++g_bad;
}

int main() {
    // heap buffers of exactly the sizes the entry points may read: an over-read is a report
    const int K = 5;
    double* beta = (double*)std::malloc(K * sizeof(double));
    const void** ups = (const void**)std::malloc(K * sizeof(void*));
    double* dist = (double*)std::malloc(K * sizeof(double));
    double* work = (double*)std::malloc(64 * sizeof(double));
    float* buf = (float*)std::malloc(5 * 64 * sizeof(float));
    for (int k = 0; k < K; ++k) {
        beta[k] = 0.2;
        ups[k] = buf + 64 * k;
    }
    float* out = buf;
    expect("wmean null dist", fa_weighted_mean_sqdist(out, FA_F32, nullptr, ups, FA_F32, beta, K, 64, 0, work, nullptr),
           FA_EINVAL, "fa_weighted_mean_sqdist: null pointer argument");
    expect("wmean null beta", fa_weighted_mean_sqdist(out, FA_F32, dist, ups, FA_F32, nullptr, K, 64, 0, work, nullptr),
           FA_EINVAL, "fa_weighted_mean_sqdist: null pointer argument");
    expect("wmean K=0", fa_weighted_mean_sqdist(out, FA_F32, dist, ups, FA_F32, beta, 0, 64, 0, work, nullptr), FA_EINVAL,
           "fa_weighted_mean_sqdist: K=0 outside 1..64");
    expect("wmean K=65", fa_weighted_mean_sqdist(out, FA_F32, dist, ups, FA_F32, beta, 65, 64, 0, work, nullptr), FA_EINVAL,
           "fa_weighted_mean_sqdist: K=65 outside 1..64");
    expect("wmean P<0", fa_weighted_mean_sqdist(out, FA_F32, dist, ups, FA_F32, beta, K, -1, 0, work, nullptr), FA_EINVAL,
           "fa_weighted_mean_sqdist: negative size (P=-1)");
    expect("wmean dtype 99", fa_weighted_mean_sqdist(out, FA_F32, dist, ups, 99, beta, K, 64, 0, work, nullptr), FA_EDTYPE,
           "fa_weighted_mean_sqdist: unsupported dtype 99");
    {
        char want[160];
        std::snprintf(want, sizeof(want), "fa_weighted_mean_sqdist: updates of dtype %d give a mean of dtype %d, not %d",
                      FA_F16, FA_F16, FA_F32);
        expect("wmean out dtype", fa_weighted_mean_sqdist(out, FA_F32, dist, ups, FA_F16, beta, K, 64, 0, work, nullptr),
               FA_EDTYPE, want);
        std::snprintf(want, sizeof(want), "fa_centered_clip_step: updates of dtype %d move a centre of dtype %d, not %d",
                      FA_I32, FA_F64, FA_F32);
        expect("cclip out dtype",
               fa_centered_clip_step(out, out, FA_F32, dist, ups, FA_I32, beta, K, 64, 0, work, nullptr), FA_EDTYPE, want);
    }
    beta[3] = -1.0;
    expect("wmean negative", fa_weighted_mean_sqdist(out, FA_F32, dist, ups, FA_F32, beta, K, 64, 0, work, nullptr), FA_EINVAL,
           "fa_weighted_mean_sqdist: beta[3]=-1 is negative or not finite");
    expect("cclip negative", fa_centered_clip_step(out, out, FA_F32, dist, ups, FA_F32, beta, K, 64, 0, work, nullptr),
           FA_EINVAL, "fa_centered_clip_step: coef[3]=-1 is negative or not finite");
    beta[3] = std::nan("");
    expect("wmean nan", fa_weighted_mean_sqdist(out, FA_F32, dist, ups, FA_F32, beta, K, 64, 0, work, nullptr), FA_EINVAL,
           "fa_weighted_mean_sqdist: beta[3]=nan is negative or not finite");
    beta[3] = INFINITY;
    expect("cclip inf", fa_centered_clip_step(out, out, FA_F32, dist, ups, FA_F32, beta, K, 64, 0, work, nullptr), FA_EINVAL,
           "fa_centered_clip_step: coef[3]=inf is negative or not finite");
    beta[3] = 1e300;
    expect("wmean 1e300 in f32", fa_weighted_mean_sqdist(out, FA_F32, dist, ups, FA_BF16, beta, K, 64, 0, work, nullptr),
           FA_EINVAL, "fa_weighted_mean_sqdist: beta[3]=1e+300 is not finite in the compute type");
    expect("cclip 1e300 in f32", fa_centered_clip_step(out, out, FA_F16, dist, ups, FA_F16, beta, K, 64, 0, work, nullptr),
           FA_EINVAL, "fa_centered_clip_step: coef[3]=1e+300 is not finite in the compute type");
    for (int k = 0; k < K; ++k) beta[k] = k == 2 ? 1e-300 : 0.0;          // zero in f32, not in f64
    expect("wmean all zero in f32", fa_weighted_mean_sqdist(out, FA_F32, dist, ups, FA_F32, beta, K, 64, 0, work, nullptr),
           FA_EINVAL, "fa_weighted_mean_sqdist: every weight is zero in the compute type");
    expect("cclip all zero, accumulate, P=0",
           fa_centered_clip_step(nullptr, out, FA_F32, dist, ups, FA_F32, beta, K, 0, 1, work, nullptr), FA_OK, nullptr);
    for (int k = 0; k < K; ++k) beta[k] = 0.2;
    expect("cclip null center", fa_centered_clip_step(out, nullptr, FA_F32, dist, ups, FA_F32, beta, K, 64, 0, work, nullptr),
           FA_EINVAL, "fa_centered_clip_step: null pointer argument");
    expect("cclip overlap", fa_centered_clip_step(out + 8, out, FA_F32, dist, ups, FA_F32, beta, K, 64, 0, work, nullptr),
           FA_EINVAL, "fa_centered_clip_step: out and center overlap without being the same buffer");
    ups[4] = nullptr;
    expect("wmean updates[4] null", fa_weighted_mean_sqdist(out, FA_F32, dist, ups, FA_F32, beta, K, 64, 0, work, nullptr),
           FA_EINVAL, "fa_weighted_mean_sqdist: updates[4] is NULL");
    expect("cclip updates[4] null", fa_centered_clip_step(out, out, FA_F32, dist, ups, FA_F32, beta, K, 64, 0, work, nullptr),
           FA_EINVAL, "fa_centered_clip_step: updates[4] is NULL");
    expect("wmean accumulate, P=0 (null updates pass)",
           fa_weighted_mean_sqdist(nullptr, FA_F64, dist, ups, FA_I64, beta, K, 0, 1, work, nullptr), FA_OK, nullptr);
    // the two sort entry points share one check (check_sort_ptrs, check_sort_size): every refusal under both names
    expect("trimmed mean P=0", fa_trimmed_mean(out, FA_F32, ups, FA_BF16, K, 1, 0, nullptr), FA_OK, nullptr);
    expect("trimmed mean null out", fa_trimmed_mean(nullptr, FA_F32, ups, FA_F32, K, 1, 64, nullptr), FA_EINVAL,
           "fa_trimmed_mean: null pointer argument");
    expect("trimmed mean null updates", fa_trimmed_mean(out, FA_F32, nullptr, FA_F32, K, 1, 64, nullptr), FA_EINVAL,
           "fa_trimmed_mean: null pointer argument");
    expect("trimmed mean K=0", fa_trimmed_mean(out, FA_F32, ups, FA_F32, 0, 0, 64, nullptr), FA_EINVAL,
           "fa_trimmed_mean: K=0 outside 1..64");
    expect("trimmed mean K=65", fa_trimmed_mean(out, FA_F32, ups, FA_F32, 65, 1, 64, nullptr), FA_EINVAL,
           "fa_trimmed_mean: K=65 outside 1..64");
    expect("trimmed mean trim=-1", fa_trimmed_mean(out, FA_F32, ups, FA_F32, K, -1, 64, nullptr), FA_EINVAL,
           "fa_trimmed_mean: trim=-1 leaves nothing of K=5");
    expect("trimmed mean 2 trim > K", fa_trimmed_mean(out, FA_F32, ups, FA_F32, K, 3, 64, nullptr), FA_EINVAL,
           "fa_trimmed_mean: trim=3 leaves nothing of K=5");
    expect("trimmed mean P<0", fa_trimmed_mean(out, FA_F32, ups, FA_F32, K, 1, -1, nullptr), FA_EINVAL,
           "fa_trimmed_mean: negative size (P=-1)");
    expect("trimmed mean dtype pair", fa_trimmed_mean(out, FA_F64, ups, FA_F32, K, 1, 64, nullptr), FA_EDTYPE,
           "fa_trimmed_mean: unsupported dtype pair (update 0, output 1)");
    expect("trimmed mean dtype 99 / -1", fa_trimmed_mean(out, -1, ups, 99, K, 1, 64, nullptr), FA_EDTYPE,
           "fa_trimmed_mean: unsupported dtype pair (update 99, output -1)");
    expect("trimmed mean updates[4] null", fa_trimmed_mean(out, FA_F32, ups, FA_F32, K, 1, 64, nullptr), FA_EINVAL,
           "fa_trimmed_mean: updates[4] is NULL");
    expect("median window null out", fa_median_window_mean(nullptr, FA_F32, ups, FA_F32, K, 3, 64, nullptr), FA_EINVAL,
           "fa_median_window_mean: null pointer argument");
    expect("median window null updates", fa_median_window_mean(out, FA_F32, nullptr, FA_F32, K, 3, 64, nullptr), FA_EINVAL,
           "fa_median_window_mean: null pointer argument");
    expect("median window K=0", fa_median_window_mean(out, FA_F32, ups, FA_F32, 0, 1, 64, nullptr), FA_EINVAL,
           "fa_median_window_mean: K=0 outside 1..64");
    expect("median window K=65", fa_median_window_mean(out, FA_F32, ups, FA_F32, 65, 1, 64, nullptr), FA_EINVAL,
           "fa_median_window_mean: K=65 outside 1..64");
    expect("median window keep=0", fa_median_window_mean(out, FA_F32, ups, FA_F32, K, 0, 64, nullptr), FA_EINVAL,
           "fa_median_window_mean: keep=0 outside 1..K=5");
    expect("median window keep=K+1", fa_median_window_mean(out, FA_F32, ups, FA_F32, K, K + 1, 64, nullptr), FA_EINVAL,
           "fa_median_window_mean: keep=6 outside 1..K=5");
    expect("median window P<0", fa_median_window_mean(out, FA_F32, ups, FA_F32, K, 3, -1, nullptr), FA_EINVAL,
           "fa_median_window_mean: negative size (P=-1)");
    expect("median window dtype pair", fa_median_window_mean(out, FA_F64, ups, FA_F32, K, 3, 64, nullptr), FA_EDTYPE,
           "fa_median_window_mean: unsupported dtype pair (update 0, output 1)");
    expect("median window updates[4] null", fa_median_window_mean(out, FA_F32, ups, FA_F32, K, 3, 64, nullptr), FA_EINVAL,
           "fa_median_window_mean: updates[4] is NULL");
    expect("median window P=0", fa_median_window_mean(out, FA_F64, ups, FA_I64, K, K, 0, nullptr), FA_OK, nullptr);
    // P = 0 without accumulate reaches the launchers (table builder, geometry, nwg = 0); with no device the
    // finish launch reports a HIP error: either status is fine, a sanitizer report is not
    int rc = fa_weighted_mean_sqdist(nullptr, FA_F32, dist, ups, FA_F32, beta, K, 0, 0, work, nullptr);
    std::printf("     wmean P=0, no accumulate: rc=%d \"%s\"\n", rc, fa_last_error());
    rc = fa_centered_clip_step(nullptr, out, FA_F64, dist, ups, FA_F64, beta, K, 0, 0, work, nullptr);
    std::printf("     cclip P=0, no accumulate: rc=%d \"%s\"\n", rc, fa_last_error());

    // the table builder on exactly-sized heap arrays, both mask kinds
    {
        WmTable<float> tab;
        double bc[5] = {0.0, 0.5, 0.0, 0.25, 0.25};
        const WmLive a = wm_fill_table(tab, ups, bc, K, true), b = wm_fill_table(tab, ups, bc, K, false);
        const bool ok = a.live == 0x18ull && b.live == 0x1Aull && a.vec && tab.ptr[5] == nullptr && tab.b[3] == 0.25f;
        std::printf("%s table builder: live (first skipped) %#llx, live %#llx\n", ok ? "ok  " : "FAIL", a.live, b.live);
        if (!ok) ++g_bad;
    }
    // the pointer-table fill on exactly-sized heap arrays: K entries read, kMaxK written
    {
        const void** five = (const void**)std::malloc(K * sizeof(void*));
        PairTable* pt = (PairTable*)std::malloc(sizeof(PairTable));
        for (int k = 0; k < K; ++k) five[k] = buf + 64 * k;
        const bool all = fill_ptrs(pt->ptr, five, K);
        five[2] = buf + 1;
        const bool odd = fill_ptrs(pt->ptr, five, K);
        const bool none = fill_ptrs(pt->ptr, five, 0);
        const bool ok = all == ((reinterpret_cast<uintptr_t>(buf) & 15u) == 0) && !odd && none && pt->ptr[0] == nullptr &&
                        pt->ptr[kMaxK - 1] == nullptr;
        std::printf("%s pointer-table fill: aligned %d, one odd pointer %d, K = 0 %d\n", ok ? "ok  " : "FAIL", (int)all,
                    (int)odd, (int)none);
        if (!ok) ++g_bad;
        std::free(five);
        std::free(pt);
    }
    // work sizes: the f64 geometry is the largest of the six at every (K, P) tried
    {
        int64_t worst = 0;
        for (int k = 1; k <= 64; ++k)
            for (const int64_t P : {(int64_t)0, (int64_t)1, (int64_t)63, (int64_t)512, (int64_t)99999, (int64_t)1 << 20,
                                    (int64_t)1 << 31, ((int64_t)1 << 40) + 7}) {
                for (const int cols : {k, k + 1}) {
                    int64_t n = 0;
                    for (const int dt : {FA_F32, FA_F16, FA_BF16, FA_F64, FA_I32, FA_I64})
                        n = std::max(n, wm_workgroups(P, wm_geom_dt(dt, k, cols)));
                    const int64_t got = cols == k ? fa_wmean_sqdist_work(k, P) : fa_centered_clip_work(k, P);
                    if (got != std::max<int64_t>(n * kMaxK, 1)) {
                        ++g_bad;
                        std::printf("FAIL work size K=%d P=%lld cols=%d: %lld\n", k, (long long)P, cols, (long long)got);
                    }
                    worst = std::max(worst, got);
                }
            }
        std::printf("ok   work sizes equal the maximum over the six dtypes for K = 1..64 x 8 sizes (largest %lld)\n",
                    (long long)worst);
    }
    int te = 0, r = 0, wg = 0, ft = 0;
    expect("wmean geometry K=0", fa_wmean_sqdist_geometry(FA_F32, 0, &te, &r, &wg, &ft), FA_EINVAL,
           "fa_wmean_sqdist_geometry: K=0 outside 1..64");
    expect("cclip geometry dtype", fa_centered_clip_geometry(99, 8, &te, &r, &wg, &ft), FA_EDTYPE,
           "fa_centered_clip_geometry: unsupported dtype 99");
    expect("cclip geometry", fa_centered_clip_geometry(FA_F16, 33, &te, nullptr, &wg, nullptr), FA_OK, nullptr);
    std::printf("     cclip geometry f16 K=33: TE=%d GRID=%d\n", te, wg);
    std::free(beta);
    std::free(ups);
    std::free(dist);
    std::free(work);
    std::free(buf);
    std::printf("%s\n", g_bad ? "RESULT: FAILED" : "RESULT: all checks passed, no sanitizer report");
    return g_bad ? 1 : 0;
}
