/*
 * fedagg.h — C ABI of the MI355X (gfx950) aggregation library `libfedagg.so`.
 *
 * This is the drop-in boundary for FEDn's combiner-side aggregation hot path
 * (SURVEY.md §8(b)). Every entry point takes plain pointers, sizes and a
 * hipStream_t passed as `void*`; no torch or numpy types cross it. Buffers are
 * owned by the caller (device memory, e.g. PyTorch-ROCm tensors); the library
 * allocates nothing persistent. Every function returns 0 on success or a
 * positive FA_E* status; `fa_last_error()` then holds a message (thread-local).
 *
 * Reference interfaces each entry point replaces (paths relative to the FEDn
 * checkout, v0.33.0):
 *   fa_fedavg_fold   numpyhelper.Helper.increment_average
 *                    fedn/utils/helpers/plugins/numpyhelper.py:18-32, applied in
 *                    queue order by fedavg.Aggregator.combine_models
 *                    fedn/network/combiner/aggregators/fedavg.py:47-71, and by
 *                    Control.reduce fedn/network/controller/control.py:678-682
 *   fa_fedopt_step   the pseudo-gradient loop + server optimizer of
 *                    fedopt.Aggregator.combine_models
 *                    fedn/network/combiner/aggregators/fedopt.py:74-118 with
 *                    serveropt_adam   fedopt.py:151-185
 *                    serveropt_yogi   fedopt.py:187-223
 *                    serveropt_adagrad fedopt.py:225-258
 *                    and the helper primitives numpyhelper.py:34-142 they call.
 *
 * Numerics contract: results are bit-identical to the numpy reference for the
 * dtypes it defines (IEEE-754 op-by-op replay of the same expression order, no
 * FMA contraction, correctly rounded division and square root). bf16 inputs have
 * no numpy counterpart: they are defined as the fp32 path on the exactly
 * upcast values.
 */
#ifndef FEDAGG_H
#define FEDAGG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FA_ABI_VERSION 15

/* element type codes */
enum fa_dtype {
    FA_NONE = -1, /* "array is None" (FedOpt state before the first round) */
    FA_F32 = 0,
    FA_F64 = 1,
    FA_BF16 = 2,
    FA_F16 = 3,
    FA_I32 = 4,
    FA_I64 = 5,
    /* narrow / unsigned integers: accepted by fa_cast and the FA_EW_IFOLD / FA_EW_NFOLD folds only
       (models with such tensors are aggregated by the per-tensor path, fedn_amd/mixed.py) */
    FA_I8 = 6,
    FA_I16 = 7,
    FA_U8 = 8,
    FA_U16 = 9,
    FA_U32 = 10,
    FA_U64 = 11
};

/* status codes */
enum fa_status {
    FA_OK = 0,
    FA_EINVAL = 1,  /* bad argument (null pointer, negative size, K out of range) */
    FA_EDTYPE = 2,  /* unsupported dtype combination */
    FA_EHIP = 3     /* a HIP runtime call or kernel launch failed */
};

/* server optimizers, fedopt.py:141-145 */
enum fa_serveropt { FA_ADAM = 0, FA_YOGI = 1, FA_ADAGRAD = 2 };

/* fa_fedopt_step flags */
#define FA_PG_FIRST 1 /* pseudo-gradient starts from updates[0] - old (fedopt.py:89-91); else read from pg */
#define FA_PG_FINAL 2 /* apply the server step and write m_out, v_out, out; else write pg   */

int fa_abi_version(void);
const char* fa_last_error(void);
/* ABI 8: the kernel family the calling thread's last fold / FedOpt launch ran ("k_fedavg",
 * "k_fedavg_pipe", "k_fedavg_pipe_win", "k_fedopt", "k_fedopt_c", "k_fedopt_cw"; "" before any), so a
 * benchmark reports the kernel that ran — e.g. whether the store window was used — not a guess.
 * fa_weighted_sum and fa_running_mean run the fold's kernels with their own arithmetic and report
 * them too: "k_fedavg" (a pointer not 16-B aligned, or a client buffer below 160 MiB) or
 * "k_fedavg_pipe" (at and above it). */
const char* fa_last_kernel(void);

/*
 * FedAvg incremental weighted fold (numpyhelper.py:32):
 *     x <- x + (n_k * (y_k - x)) / N_k        for k in queue order
 *
 * agg      device buffer, P elements of agg_dtype (the running model)
 * updates  HOST array of K DEVICE pointers, each P elements of upd_dtype
 * n, N     HOST arrays of K doubles: num_examples of update k and the running
 *          total including it (fedavg.py:62), exact integers
 * init     1: agg := updates[0] (the `model = model_next` alias, fedavg.py:65-66),
 *             then fold k = 1..K-1;  0: fold k = 0..K-1 into the existing agg
 * stream   hipStream_t (NULL = default stream)
 *
 * dtype pairs (upd, agg) and the compute type numpy would use:
 *   (F32,F32)->f32  (BF16,F32)->f32  (F16,F16)->f16  (F64,F64)->f64
 *   (F32,F64)->f64  (I64,F64)/(I32,F64)->int then f64 (numpy true_divide)
 * With init=1 and K=1 the result is a plain copy and agg_dtype must equal upd_dtype.
 * Integer updates with init=1: n[1] must be integral (numpy multiplies the first integer difference
 * in the integer dtype only for an int num_examples; see FA_EW_IFOLD for a float one) and fit the
 * update dtype (I32: -2^31 <= n[1] < 2^31; numpy raises OverflowError for a python int outside the
 * dtype instead of wrapping it). Either violation is FA_EINVAL, and nothing is written.
 */
int fa_fedavg_fold(void* agg, int agg_dtype,
                   const void* const* updates, int upd_dtype,
                   const double* n, const double* N, int K,
                   int64_t P, int init, void* stream);

/*
 * fa_fedavg_fold_host (ABI 8): fa_fedavg_fold for a small model whose round never leaves the host
 * (configs[0]: FEDn's mnist-pytorch example, fedavg.py:47-83 over 52,650 parameters). agg and every
 * updates[k] are PAGE-LOCKED HOST addresses (e.g. the pinned arena the updates were packed into and a
 * pinned result block); the kernel reads and writes them over PCIe through their device mappings
 * (hipHostGetDevicePointer), and the call returns once `stream` has drained, with the model in agg.
 * No H2D / D2H copy and no event: the round's GPU work is one launch and one wait. Same kernel,
 * client table and dtype pairs as fa_fedavg_fold, so the same bits. K <= 64 (one launch).
 * FA_EINVAL for memory that is not page-locked.
 */
int fa_fedavg_fold_host(void* agg, int agg_dtype, const void* const* updates, int upd_dtype,
                        const double* n, const double* N, int K, int64_t P, int init, void* stream);

/*
 * fa_fedopt_step_host (ABI 8): the FedOpt round of a small model in one call — fa_fedopt_step_ex with
 * flags FA_PG_FIRST | FA_PG_FINAL and no pg workspace, where `old`, every updates[k] and `out` are
 * PAGE-LOCKED HOST addresses (the global model and the updates packed into a pinned arena, a pinned
 * result block), mapped inside; m_in / m_out / v_in / v_out are device buffers as in
 * fa_fedopt_step_ex (the session's state stays in HBM). Returns once `stream` has drained. 1 <= K <= 64.
 */
int fa_fedopt_step_host(const void* old, int old_dtype, const void* const* updates, int upd_dtype,
                        const double* n, const double* N, int K,
                        const void* m_in, int m_in_dtype, void* m_out, int m_out_dtype,
                        const void* v_in, int v_in_dtype, void* v_out, void* out, int state_dtype,
                        int serveropt, double lr, double beta1, double beta2, double tau, int64_t P, void* stream);

/*
 * FedOpt (fedopt.py:74-118, 151-258), fused: pseudo-gradient running mean over the
 * K updates followed (FA_PG_FINAL) by one Adam / Yogi / AdaGrad server step.
 *
 * old       device, P elements of old_dtype (F32 | F64 | F16 | I32 | I64): the global model the
 *           clients trained from (fedopt.py:90)
 * updates   HOST array of K DEVICE pointers (F32 | BF16 | F16 | F64 | I32 | I64); a float16
 *           pseudo-gradient (F16 updates over an F16 model) is computed with numpy's half loops
 *           (every op rounded to half, python scalars cast to half); integer tensors
 *           (e.g. BatchNorm counters) become float64 exactly as numpy's int * 1.0 does.
 *           upd_dtype is required even when K = 0: it fixes the pg dtype.
 * n, N      HOST arrays of K doubles (num_examples, running total)
 * pg        device workspace, P elements of pg dtype = promote(upd, old) (F64 for integer
 *           updates); read when
 *           !FA_PG_FIRST, written when !FA_PG_FINAL (and used internally when
 *           K exceeds one launch); may be NULL when FIRST|FINAL and K <= 64
 * m_in      device, P elements of m_in_dtype (F16 | F32 | F64), or NULL with m_in_dtype = FA_NONE
 * m_out     device, dtype promote(m_in, pg) (pg dtype when m is None); may alias m_in
 *           when the dtypes are equal
 * v_in      device f64, or NULL (v is None -> ones * tau**2, fedopt.py:170-171)
 * v_out     device f64; may alias v_in
 * out       device f64 (the new global model, fedopt.py:183)
 * serveropt FA_ADAM | FA_YOGI | FA_ADAGRAD; lr, beta1, beta2, tau as in fedopt.py:53-59
 */
int fa_fedopt_step(const void* old, int old_dtype,
                   const void* const* updates, int upd_dtype,
                   const double* n, const double* N, int K,
                   void* pg, int flags,
                   const void* m_in, int m_in_dtype, void* m_out,
                   const double* v_in, double* v_out, double* out,
                   int serveropt, double lr, double beta1, double beta2, double tau,
                   int64_t P, void* stream);

/*
 * fa_fedopt_step with the storage dtypes of the server state explicit: the reference's flow
 * (state_dtype F64; m_out_dtype = numpy's promote(m_in, pg)) or the fp32-STATE mode (state_dtype
 * F32): v_out and out are float32 and m_out may be F32. Same arithmetic as the reference step on the
 * values it is given (f64 server step, numpy's dtype rules for m and the pseudo-gradient); each
 * stored value is the f64 result rounded once to f32, and f32 state is widened exactly on load.
 * HBM bytes per round in that mode with fp32 updates, old, m, v: P*(4K + 24) instead of
 * P*(4K + 48) (plug-in fedn_amd.aggregators.fedopt_f32state).
 * v_in_dtype: F64 or F32 (either mode may read either: a session can switch).
 */
int fa_fedopt_step_ex(const void* old, int old_dtype,
                      const void* const* updates, int upd_dtype,
                      const double* n, const double* N, int K,
                      void* pg, int flags,
                      const void* m_in, int m_in_dtype, void* m_out, int m_out_dtype,
                      const void* v_in, int v_in_dtype, void* v_out, void* out, int state_dtype,
                      int serveropt, double lr, double beta1, double beta2, double tau,
                      int64_t P, void* stream);

/*
 * Server-function aggregation rules (hooks.py:109-143): the two formulas the reference ships
 * as examples of user aggregation code, on device buffers with numpy's rounding.
 *
 * fa_weighted_sum replaces the loop of examples/server-functions/server_functions.py:58-67
 *     for each client k in order:  acc[i] += updates[k][i] * w[k]
 *   the product in the update dtype (w is a weak python scalar), the sum in
 *   promote(acc, update), stored in the accumulator dtype. acc is read (start from zeros for
 *   the example's np.zeros_like). The final `/ total_weight` is fa_elementwise(FA_EW_DIV).
 *   acc_dtype, upd_dtype in {F32, F64}; w: HOST array of K doubles; any K (chunked by 64).
 *
 * fa_running_mean replaces examples/server-functions/sf_incremental_aggregation.py:36-37
 *     g[i] = (g[i] * a + m[i] * b) / T      with a = T - n, b = n, T = running total
 *   in place, g and m of the same dtype (F32 or F64); every scalar cast to that dtype.
 */
int fa_weighted_sum(void* acc, int acc_dtype, const void* const* updates, int upd_dtype,
                    const double* w, int K, int64_t P, void* stream);
int fa_running_mean(void* g, int dtype, const void* m, double a, double b, double T,
                    int64_t P, void* stream);

/*
 * numpyhelper primitives (numpyhelper.py:34-142) on device buffers, numpy rounding (python
 * scalars a, b are weak: x*a is computed in x's dtype, then promoted). F32 / F64, and AXPBY on
 * three F16 arrays (numpy's half loops: a, b cast to half, every op rounded to half).
 *   FA_EW_AXPBY   out = x*a + y*b                 numpyhelper.add / subtract (b -> -b)
 *   FA_EW_MUL     out = x*y, or x*a if y == NULL   numpyhelper.multiply
 *   FA_EW_DIV     out = x/y, or x/a if y == NULL   numpyhelper.divide
 *   FA_EW_SQRT    out = sqrt(x)                    numpyhelper.sqrt
 *   FA_EW_SQUARE  out = x*x                        numpyhelper.power(m, 2)
 *   FA_EW_SIGN    out = sign(x) (+-1, 0, NaN)      numpyhelper.sign
 *   FA_EW_FILL    out = 1.0*a (x unused)           numpyhelper.ones
 *   FA_EW_POW     out = x**a (float a)             numpyhelper.power(m, a) = np.power(x, a). a is a weak
 *                                                  scalar: an f32 x is raised to (float)a, as numpy
 *                                                  does, computed as RN_f32(pow((double)x, (float)a))
 *                                                  with the f64 pow; an f64 x to a itself. C99 Annex F
 *                                                  special cases, bit for bit. (numpy's own float power
 *                                                  is its host libm's / SIMD library's: not
 *                                                  bit-reproducible across hosts; parity: 1e-6
 *                                                  relative, f64 1e-15)
 *   FA_EW_IPOW    out = x**a, x any integer dtype (I8..I64, U8..U64), a a non-negative integer:
 *                 exponentiation by squaring with wrapping products, out_dtype = x_dtype (numpy's
 *                 integer power)
 *   FA_EW_IFOLD   out = x + ((y - x)*a)/b, x and y of one integer dtype (I8..I64, U8..U64), out
 *                 F64: numpyhelper.increment_average (numpyhelper.py:32) on integer arrays with a
 *                 python-float num_examples a and total b — the difference wraps in the integer
 *                 dtype, then float64 multiply, divide and add, each rounded once
 *   FA_EW_NFOLD   out = x + T((y - x)*a)/b, x and y of one integer dtype T (I8, I16, U8, U16, U32,
 *                 U64, I32, I64), out F64: the same fold with a python-INT num_examples a (integral,
 *                 |a| < 2^53; numpy refuses an a outside T's range, and so must the caller) —
 *                 difference and product wrap in T, then the float64 divide by b and add
 * out_dtype must be the numpy result dtype of the op.
 * out may be exactly x or exactly y when it has that operand's dtype (each element is read before
 * it is written, by the same lane: `acc /= total`, `x = x*a + y*b`); a partial overlap is not allowed.
 */
enum fa_ew_op { FA_EW_AXPBY = 0, FA_EW_MUL = 1, FA_EW_DIV = 2, FA_EW_SQRT = 3, FA_EW_SQUARE = 4, FA_EW_SIGN = 5,
                FA_EW_FILL = 6, FA_EW_POW = 7, FA_EW_IPOW = 8, FA_EW_IFOLD = 9,
                FA_EW_NFOLD = 10 };
int fa_elementwise(int op, void* out, int out_dtype, const void* x, int x_dtype, const void* y, int y_dtype,
                   double a, double b, int64_t P, void* stream);

/*
 * numpyhelper.norm (numpyhelper.py:106-117) for one tensor: np.linalg.norm(x, 1), i.e. sum |x| of a
 * vector (matrix = 0; rows*cols elements) or the max column sum of |x| of a C-order rows x cols
 * matrix (matrix = 1). x: F32 | F64 | any integer dtype (numpy: astype(float) first). Accumulated in
 * f64 in a fixed order (numpy sums f32
 * pairwise in f32: parity 1e-6 relative). out: DEVICE double (written on `stream`); work: DEVICE
 * scratch of fa_norm1_work(rows, cols, matrix) doubles.
 */
int64_t fa_norm1_work(int64_t rows, int64_t cols, int matrix);
int fa_norm1(double* out, const void* x, int dtype, int64_t rows, int64_t cols, int matrix, double* work,
             void* stream);

/* dtype promotion used by the two entry points above (numpy result_type for the
 * pairs this library supports; bf16 promotes as f32). Returns FA_NONE if unsupported. */
int fa_promote(int a, int b);

/*
 * Broadcast + widening conversion, the implicit step numpy takes before a binary ufunc whose
 * operands differ in dtype or (broadcastable) shape — e.g. numpyhelper.py:32 folding a float64
 * client into a float32 model, an int64 model with a float32 client, or a (1,) tensor against
 * (n,). Used by the per-tensor path of the plug-ins (fedn_amd/mixed.py) when client updates
 * differ from the running model (fedavg.py:68, fedopt.py:91-94, control.py:682).
 *
 *   out[i] = convert(in[j(i)])      i over the ndim-dimensional C-order index space out_shape,
 *                                   j(i) = sum_d i_d * in_strides[d] (element strides; 0 along
 *                                   broadcast dimensions)
 * Conversions (numpy's casting of the value): identity for every dtype; F16/BF16 -> F32/F64 and
 * F32 -> F64 (exact); I32 -> I64 (exact); I32/I64 -> F64 (round to nearest even); I8 / I16 / U8 /
 * U16 / U32 / U64 to every integer or float dtype numpy casts them to safely (U64 -> F64 rounds to
 * nearest even, the rest are exact); and two narrowing float casts, F32 -> F16 and F64 -> F32, rounded
 * to nearest even as numpy's astype (the result of a helper op computed in a wider float: a single
 * correctly rounded op then rounded again equals the op rounded once, since 24 >= 2*11+2 and
 * 53 >= 2*24+2). Other narrowing conversions are refused (FA_EDTYPE). 1 <= ndim <= 8; out is contiguous.
 */
int fa_cast(void* out, int out_dtype, const void* in, int in_dtype, int ndim, const int64_t* out_shape,
            const int64_t* in_strides, void* stream);

/*
 * Peer transport of the parameter-sliced all-gather ("prefer ... direct (all 7
 * links)"; the gathered model's consumer is roundhandler.py:465-468). Replaces the transport of
 * RCCL's ncclAllGather for fedn_amd/sharded.py P2PAllGather (one process per GPU) and
 * fedn_amd/multidev.py allgather_devices (one process, several GPUs): every rank copies its folded
 * slice straight into each peer's model buffer, one copy stream per peer (one xGMI link each).
 *
 * fa_ipc_get_handle  FA_IPC_HANDLE_BYTES of handle for the allocation that holds dptr, and dptr's
 *                    byte offset in it (a caching allocator hands out pieces of one allocation)
 * fa_ipc_open        map another process's handle: *base = the mapping (pass it to fa_ipc_close),
 *                    *dptr = base + offset
 * fa_ipc_close       unmap a mapping fa_ipc_open returned
 * fa_copy_async      bytes from src to dst on stream; any two device pointers of this process
 *                    (IPC mappings and other devices' buffers included): the DMA engines move them
 * fa_push            bytes from src to each of ndst (<= 16) destinations on stream, by a kernel: the
 *                    source is read once and every destination (IPC mappings of the peers' model
 *                    buffers, or in-process peers' buffers) written by vector stores — each over its
 *                    own link, all at once; 16-B aligned pointers. The alternative to one
 *                    fa_copy_async per peer that the all-gather picks between (sharded.P2PAllGather;
 *                    replaces the all-gather consumed at roundhandler.py:465-468)
 * fa_fedavg_fold_push  fa_fedavg_fold (fp32 updates, fp32 aggregate, 16-B aligned buffers) whose kernel
 *                    also stores every finished element to each of ndst (<= 16) destinations: the
 *                    fold and the all-gather push in ONE pass (sharded.P2PAllGather engine "fused";
 *                    the peers' buffers IPC-mapped or in-process). agg is this rank's own copy.
 *   release_rec      (fa_push, fa_fedavg_fold_push; ABI 7) after a grid that stored into peers, a
 *                    release grid writes every XCD's L2 back at system scope. HIP does not promise
 *                    which XCDs a grid's workgroups run on, so each release workgroup records its
 *                    XCD (HW_REG_XCC_ID) in release_rec: FA_RELEASE_WORDS uint32 of caller-owned
 *                    DEVICE memory, zeroed once before the first call and then passed to every call
 *                    on one stream. Per release launch, the last workgroup compares the number of
 *                    distinct XCDs covered with the device's XCD count (IDs are counted, not matched
 *                    against 0 .. n - 1: a partition mode may report physical indices) and
 *                    increments FA_REL_MISSES on a gap; FA_REL_LAUNCHES counts the launches checked,
 *                    FA_REL_SEEN is the union of the XCDs seen and FA_REL_EXPECT the mask
 *                    (1 << n) - 1 of the device's XCD count. The caller reads the record at a
 *                    synchronisation point and must treat MISSES > 0 as a failed exchange. NULL:
 *                    release without the record (in-process peers behind a device synchronize).
 * fa_device_xccs     *n = the number of XCDs (each with its own L2) of device dev
 * fa_peer_enable     let device dev read / write device peer's memory directly (in-process);
 *                    already enabled is not an error
 * fa_host_register   page-lock host memory the caller mapped (the node's shared host model that
 *                    every rank D2H's its slice into: sharded.HostGather), so DMA reaches it directly;
 * fa_host_unregister undo it before the caller unmaps
 * fa_host_device_ptr the device address of page-locked host memory (hipHostGetDevicePointer): a
 *                    small round's fold reads its clients from the pinned arena and writes the
 *                    model into the caller's pinned block over PCIe, with no H2D / D2H copy
 *                    (staging.FedAvgPipeline.result); an error for pageable memory
 */
#define FA_IPC_HANDLE_BYTES 64
#define FA_RELEASE_WORDS 8
enum fa_release_word { FA_REL_MASK = 0, FA_REL_ARRIVED = 1, FA_REL_LAUNCHES = 2, FA_REL_MISSES = 3, FA_REL_SEEN = 4,
                       FA_REL_EXPECT = 5 };
int fa_ipc_get_handle(const void* dptr, void* handle, uint64_t* offset);
int fa_ipc_open(const void* handle, uint64_t offset, void** base, void** dptr);
int fa_ipc_close(void* base);
int fa_copy_async(void* dst, const void* src, int64_t bytes, void* stream);
int fa_push(void* const* dsts, int ndst, const void* src, int64_t bytes, uint32_t* release_rec, void* stream);
int fa_fedavg_fold_push(float* agg, const void* const* updates, const double* n, const double* N, int K, int64_t P,
                        int init, void* const* dsts, int ndst, uint32_t* release_rec, void* stream);
int fa_device_xccs(int dev, int* n);
int fa_peer_enable(int dev, int peer);
int fa_host_register(void* p, int64_t bytes);
int fa_host_unregister(void* p);
int fa_host_device_ptr(const void* host, void** dptr);

/*
 * fa_trimmed_mean (ABI 9): coordinate-wise trimmed mean of K client updates (Yin et al., 2018), the
 * median included — a robust, UNWEIGHTED rule: one client cannot move a parameter past the others'.
 * Per element, the K values of upd_dtype are put in the total order "by value, -0 before +0, every
 * NaN (either sign, any payload) after +inf, all NaNs equal"; of the ascending sequence s the values
 * s[trim] .. s[K-trim-1] are kept, and
 *     out = (((A(s[trim]) + A(s[trim+1])) + ...) + A(s[K-trim-1])) / A(K - 2*trim)
 * with every add rounded once in the accumulator type A (the sum starts from the first kept value, not
 * from zero: a kept run of -0 gives -0), an IEEE division, and one rounding to out_dtype. A NaN among
 * the kept values gives NaN. This equals numpy's np.sort(S, axis=0)[trim:K-trim].mean(axis=0) bit for
 * bit, and with trim = (K-1)/2 np.median(S, axis=0) (numpy leaves the order of -0 / +0 ties open).
 *
 * (upd, out) pairs and A:  (F32,F32) f32   (F64,F64) f64   (F16,F16) f32   (BF16,F32) f32 on exact
 * upcasts   (I32,F64) / (I64,F64) f64, each kept value converted with one rounding.
 *
 * updates  HOST array of K DEVICE pointers, each P elements of upd_dtype; 1 <= K <= 64
 * trim     0 <= trim and 2*trim < K;  the median is trim = (K - 1) / 2
 * FA_EINVAL: a null pointer, K or trim out of range, P < 0; FA_EDTYPE: any other dtype pair; FA_OK
 * for P = 0 — all before any HIP call. fa_last_kernel reports "k_order_mean".
 */
int fa_trimmed_mean(void* out, int out_dtype, const void* const* updates, int upd_dtype,
                    int K, int trim, int64_t P, void* stream);

/*
 * fa_pairwise_sqdist (ABI 10): the K x K matrix of squared Euclidean distances between K client updates,
 * the input of Krum / Multi-Krum (Blanchard et al., 2017) and of any rule that selects whole updates.
 * With C the compute type of upd_dtype — f32 for F32 / F16 / BF16 (each value widened exactly), f64 for
 * F64 / I32 / I64 (each value converted with one rounding) —
 *     D[i][j] = sum_p (C(u_i[p]) - C(u_j[p]))^2      for i != j,      D[i][i] = 0 exactly.
 * Each difference is rounded once in C; the squares are summed in C (fused multiply-add) in chains of at
 * most R = FA_PAIR_CHAIN_TERMS terms (a compile-time constant of the library); the chain totals
 * are summed in f64. Every term is non-negative, so against exact arithmetic on the converted values the
 * relative error of an entry is at most (R + 4) * 2^-24 for C = f32 and (P + 4) * 2^-53 for C = f64.
 * D is exactly symmetric: the upper triangle is computed and mirrored. A non-finite input value makes the
 * entries of its client inf or NaN; that is not an error.
 *
 * Deterministic: the partition of the elements into chains and partial sums depends only on (K, P,
 * upd_dtype), the partials are combined in a fixed order and there is no floating-point atomic — the
 * same inputs give the same bits on every call, whether or not the client pointers are 16-byte aligned.
 *
 * D        DEVICE buffer of K x K doubles, row-major
 * updates  HOST array of K DEVICE pointers, each P elements of upd_dtype; 1 <= K <= 64
 * accumulate  0: D is written; 1: the call's distances are added to D in f64 (D[i][j] += d, D[j][i] += d)
 *          — a model's dtype groups or slices summed into one D without a host round trip
 * work     DEVICE scratch of fa_pairwise_sqdist_work(K, P) doubles (>= 1; enough for every dtype)
 * FA_EINVAL: a null pointer (an entry of updates included, when P > 0), K outside 1..64, P < 0; FA_EDTYPE: a dtype
 * outside the six above — all before any HIP call. P = 0 and K = 1 are FA_OK: with accumulate = 0 the
 * zeros (the single 0) are still written by a launch; with accumulate = 1 there is nothing to add and
 * nothing is launched. fa_last_kernel reports "k_pair_sqdist".
 */
#define FA_PAIR_CHAIN_TERMS 1024 /* R: the longest chain summed in the compute type */
int64_t fa_pairwise_sqdist_work(int K, int64_t P);
int fa_pairwise_sqdist(double* D, const void* const* updates, int upd_dtype, int K, int64_t P, int accumulate,
                       double* work, void* stream);

/*
 * fa_weighted_mean_sqdist (ABI 11): a weighted mean of K client updates and the K squared distances of
 * the updates to it, in ONE pass over the updates — one smoothed Weiszfeld step of the geometric median
 * (RFA: Pillutla, Kakade and Harchaoui). With C the compute type of upd_dtype as for fa_pairwise_sqdist
 * and b_k = C(beta[k]) (each cast once), per element over the clients with b_k != 0 in index order
 *     acc = b C(u)  for the first,  acc = acc + b C(u)  for the others,      z = acc rounded once to out_dtype,
 * every product and every add rounded once in C (no FMA, no reassociation). A client with b_k = 0 is no
 * part of z: its inf or NaN cannot reach it. Then, for EVERY k (b_k = 0 included),
 *     dist[k] = sum_p (C(u_k[p]) - C(z[p]))^2        with z as stored (or as it would be, out = NULL),
 * by fa_pairwise_sqdist's arithmetic: the difference rounded once, the squares summed by FMA in chains
 * of at most FA_PAIR_CHAIN_TERMS terms in C, the chain totals in f64 — relative error at most
 * (R + 4) * 2^-24 for C = f32 and (P + 4) * 2^-53 for C = f64 against exact arithmetic on C(u), C(z).
 *
 * Deterministic as fa_pairwise_sqdist: the partition into tiles, chains and partials depends only on
 * (K, P, upd_dtype), the grid cap is a constant, partials are combined in a fixed order, there is no
 * floating-point atomic; the same bits on every call, whether or not the pointers are 16-byte aligned.
 *
 * out      DEVICE buffer of P elements of out_dtype, or NULL: z is computed but not stored
 * out_dtype  F32 for F32 / BF16 updates, F16 for F16, F64 for F64 / I32 / I64
 * dist     DEVICE buffer of K doubles
 * updates  HOST array of K DEVICE pointers, each P elements of upd_dtype; 1 <= K <= 64
 * beta     HOST array of K doubles, each finite and >= 0, not all zero in C
 * accumulate  0: dist is written; 1: the call's distances are added to it in f64 (dtype groups, slices)
 * work     DEVICE scratch of fa_wmean_sqdist_work(K, P) doubles (>= 1; enough for every dtype)
 * FA_EINVAL: a null dist, beta, updates or work, a null entry of updates when P > 0, K outside 1..64,
 * P < 0, a beta that is negative or not finite, every C(beta) zero; FA_EDTYPE: a dtype outside the six or
 * an out_dtype that is not the table's — all before any HIP call. P = 0 is FA_OK: with accumulate = 0
 * the K zeros are still written, with accumulate = 1 nothing is launched. A non-finite input value is not
 * an error. fa_last_kernel reports "k_wmean_dist".
 */
int64_t fa_wmean_sqdist_work(int K, int64_t P);
int fa_weighted_mean_sqdist(void* out, int out_dtype, double* dist, const void* const* updates, int upd_dtype,
                            const double* beta, int K, int64_t P, int accumulate, double* work, void* stream);

/*
 * fa_centered_clip_step (ABI 12): one step of centred clipping (Karimireddy, He and Jaggi, "Learning from
 * History for Byzantine Robust Optimization") — the centre v moved by the clipped differences of K client
 * updates to it — and the K squared distances of the updates to the NEW point, in ONE pass over the
 * updates. With C and the output type O of upd_dtype as for fa_weighted_mean_sqdist (O -> C is exact) and
 * c_k = C(coef[k]) (each cast once), per element
 *     acc = C(v),   then over the clients with c_k != 0 in index order:   acc = acc + c_k (C(u_k) - C(v)),
 *     v' = acc rounded once to O,
 * the difference, the product and the add each rounded once in C (no FMA, no reassociation): a client
 * equal to the centre contributes exactly 0, a client with c_k = 0 is no part of v' (its inf or NaN cannot
 * reach it). Every c_k = 0 is legal: v' = O(C(v)), and with out = NULL the call is the distances-only pass
 * that starts the rule. Then, for EVERY k,
 *     dist[k] = sum_p (C(u_k[p]) - C(v'[p]))^2       with v' as stored (or as it would be, out = NULL),
 * by fa_weighted_mean_sqdist's arithmetic and within its error bound. The caller clips:
 * coef[k] = min(1, tau / sqrt(d_k)) / K_good from the distances of the step before.
 *
 * Deterministic as fa_weighted_mean_sqdist: tiles, chains and partials depend only on (K, P, upd_dtype),
 * the grid cap is a constant, no floating-point atomic; the same bits on every call and at every pointer
 * alignment.
 *
 * out      DEVICE buffer of P elements of out_dtype; NULL: v' is computed but not stored; `center` itself:
 *          the step is taken in place (safe by construction: a workgroup reads its tile of the centre
 *          before it stores to it, and tiles are disjoint); any other buffer must not overlap `center`
 * center   DEVICE buffer of P elements of out_dtype
 * out_dtype  F32 for F32 / BF16 updates, F16 for F16, F64 for F64 / I32 / I64
 * dist     DEVICE buffer of K doubles
 * updates  HOST array of K DEVICE pointers, each P elements of upd_dtype; 1 <= K <= 64
 * coef     HOST array of K doubles, each finite and >= 0 (in C too)
 * accumulate  0: dist is written; 1: the call's distances are added to it in f64 (dtype groups, slices)
 * work     DEVICE scratch of fa_centered_clip_work(K, P) doubles (>= 1; enough for every dtype)
 * FA_EINVAL: a null dist, center, coef, updates or work, a null entry of updates when P > 0, K outside
 * 1..64, P < 0, a coef that is negative or not finite (also as a C value), out overlapping center without
 * being equal to it; FA_EDTYPE: a dtype outside the six or an out_dtype that is not the table's — all
 * before any HIP call. P = 0 is FA_OK: with accumulate = 0 the K zeros are still written, with
 * accumulate = 1 nothing is launched. A non-finite input value is not an error. fa_last_kernel reports
 * "k_cclip_dist".
 */
int64_t fa_centered_clip_work(int K, int64_t P);
int fa_centered_clip_step(void* out, const void* center, int out_dtype, double* dist, const void* const* updates,
                          int upd_dtype, const double* coef, int K, int64_t P, int accumulate, double* work,
                          void* stream);

/*
 * fa_median_window_mean (ABI 13): per element, the mean of the `keep` values closest to the median of K
 * client updates — the second stage of Bulyan (El Mhamdi, Guerraoui and Rouault, 2018), which calls it
 * with the theta = K_round - 2f selected updates and keep = theta - 2f. UNWEIGHTED like fa_trimmed_mean,
 * whose total order, dtype pairs, accumulator type A and output rounding it shares. Per element:
 *   1. the K values are sorted in fa_trimmed_mean's total order (-0 before +0, every NaN after +inf, all
 *      NaNs equal): s[0 .. K-1];
 *   2. med is the median KEPT IN A: A(s[(K-1)/2]) for an odd K, (A(s[K/2-1]) + A(s[K/2])) / A(2) for an
 *      even one (one add, one IEEE division, each rounded once; not rounded to out_dtype);
 *   3. the window start: a = 0; while a < K - keep and (A(s[a+keep]) - med) < (med - A(s[a])): a += 1.
 *      Each difference is rounded once in A; the comparison is strict (a tie keeps the lower window) and
 *      false when a NaN is involved (the walk stops). The predicate is monotone in a, so a is also the
 *      number of j in [0, K - keep) for which it holds: the kernel counts;
 *   4. out = (((A(s[a]) + A(s[a+1])) + ...) + A(s[a+keep-1])) / A(keep): ascending, starting from A(s[a]),
 *      every add rounded once, no FMA, one IEEE division, one rounding to out_dtype.
 * With keep = K this is fa_trimmed_mean at trim 0, bit for bit.
 *
 * updates  HOST array of K DEVICE pointers, each P elements of upd_dtype; 1 <= K <= 64
 * keep     the window length, 1 <= keep <= K (K - keep may be odd)
 * FA_EINVAL: a null pointer, K or keep out of range, P < 0; FA_EDTYPE: a dtype pair fa_trimmed_mean does
 * not take; FA_OK for P = 0 — all before any HIP call. fa_last_kernel reports "k_median_window".
 */
int fa_median_window_mean(void* out, int out_dtype, const void* const* updates, int upd_dtype,
                          int K, int keep, int64_t P, void* stream);

/*
 * fa_gaussian_noise (ABI 14): Gaussian noise for central DP-FedAvg (McMahan, Ramage, Talwar and Zhang, 2018),
 * added to a buffer: out[j] = O(double(x[j]) + sigma * z(offset + j)), j in [0, P), with z(i) the N(0,1)
 * deviate that is a pure function of (seed, stream_id, round_id, i) — DESIGN.md §3.12:
 *     (x0, x1, x2, x3) = Philox4x32-10(ctr = (i mod 2^32, i >> 32, stream_id, round_id),
 *                                      key = (seed mod 2^32, seed >> 32))
 *     u1 = ((x0 >> 5) 2^26 + (x1 >> 6) + 1) 2^-53 in (0, 1],   u2 = ((x2 >> 5) 2^26 + (x3 >> 6)) 2^-53 in [0, 1)
 *     z = sqrt(-2 log(u1)) cos(TWO_PI u2) in float64 (TWO_PI the float64 nearest 2 pi), |z| <= 8.58.
 * The product sigma z and the sum are each rounded once in float64 (no FMA) and the result is converted
 * ONCE to the output type; a float16 output is rounded straight from float64. The bits of the uniforms are
 * the definition's; log and cos are the device library's float64 functions (DESIGN.md §3.12 has the
 * measured distance to a correctly rounded z). One block per element: the same bits for every split of
 * [0, P) into calls at their offsets, for every grid and every pointer alignment.
 *
 * out      DEVICE buffer of P elements of dtype (written: exactly out[0 .. P))
 * x        DEVICE buffer of P elements of dtype; `out` itself (in place, the normal use), a buffer that does
 *          not overlap it, or NULL: zeros (out float64, x NULL, sigma 1 gives z itself)
 * dtype    F32, F64 or F16: the output types of the robust rules (bf16 is never one)
 * sigma    the noise's standard deviation, finite and >= 0
 * offset   the index of out[0] in the stream, >= 0, offset + P <= 2^63 - 1
 * FA_EINVAL: a null out with P > 0, P < 0, offset < 0, offset + P past 2^63 - 1, a sigma that is negative
 * or not finite, out overlapping x without being equal to it; FA_EDTYPE: any other dtype — all before any
 * HIP call. P = 0 is FA_OK with no launch. fa_last_kernel reports "k_gaussian_noise".
 */
int fa_gaussian_noise(void* out, const void* x, int dtype, double sigma, uint64_t seed, uint32_t stream_id,
                      uint32_t round_id, int64_t offset, int64_t P, void* stream);

/*
 * fa_clip_fold (ABI 15): the centred-clipping fold of fa_centered_clip_step for rounds of MORE than 64
 * clients — up to 64 clients of a round folded into a running accumulator that is carried between launches
 * in the compute type. With C, O and c_k = C(coef[k]) as for fa_centered_clip_step, per element
 *     acc = carry_in[p] where carry_in is given, else C(center[p]),
 *     then over the call's clients with c_k != 0 in index order:   acc = acc + c_k (C(u_k) - C(center[p])),
 *     carry_out[p] = acc (in C, exact),   out[p] = acc rounded once to O,   whichever is given,
 * the difference, the product and the add each rounded once in C (no FMA, no reassociation). A client with
 * c_k = 0 is never read. The differences are always taken to `center`, which the call does not modify
 * unless out == center. A chain of calls over consecutive chunks of a round's clients in index order — the
 * first without carry_in, the last with out, the ones between with both carries — gives
 * fa_centered_clip_step's v' bit for bit, wherever the chain is cut. No distances: the
 * caller takes them with fa_centered_clip_step at coef = 0 against the new point.
 *
 * out        DEVICE buffer of P elements of out_dtype, or NULL; `center` itself is legal (in place: a lane
 *            reads its elements of the centre before it stores them)
 * out_dtype  F32 for F32 / BF16 updates, F16 for F16, F64 for F64 / I32 / I64 (named also when out is NULL)
 * carry_out  DEVICE buffer of P elements of C (float for F32 / F16 / BF16 updates, else double), or NULL; at
 *            least one of out and carry_out is given
 * carry_in   DEVICE buffer of P elements of C, or NULL; `carry_out` itself is legal
 * center     DEVICE buffer of P elements of out_dtype
 * updates    HOST array of K DEVICE pointers, each P elements of upd_dtype; 1 <= K <= 64
 * coef       HOST array of K doubles, each finite and >= 0 (in C too); all zero is legal (acc passes through)
 * FA_EINVAL: a null center, coef or updates, out and carry_out both null, a null entry of updates when
 * P > 0, K outside 1..64, P < 0, a coef that is negative or not finite (also as a C value), and at P > 0 any
 * overlap among out, the carries and the centre other than the two aliases above, or of one of those four
 * with an update; FA_EDTYPE: a dtype outside the six or an out_dtype that is not the table's — all before
 * any HIP call. P = 0 is FA_OK with no launch. The same bits on every call, for every grid and at every
 * pointer alignment. fa_last_kernel reports "k_clip_fold".
 */
int fa_clip_fold(void* out, int out_dtype, void* carry_out, const void* carry_in, const void* center,
                 const void* const* updates, int upd_dtype, const double* coef, int K, int64_t P, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FEDAGG_H */
