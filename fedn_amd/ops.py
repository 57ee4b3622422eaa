"""Tensor-level entry points over the C ABI (device buffers are PyTorch-ROCm tensors).

These are thin: validate shapes/devices, collect raw pointers, call libfedagg on the
tensors' current HIP stream, raise :class:`FedAggError` on a nonzero status.

dtype rules mirror numpy's for the reference expressions:
see :func:`fold_result_dtype` and :func:`fedopt_dtypes`.
"""
import contextlib
import ctypes

import numpy as np
import torch

from . import _abi
from ._abi import FedAggError  # noqa: F401  (the status exception, re-exported for the pipelines)

_TORCH_TO_FA = {
    torch.float32: _abi.FA_F32,
    torch.float64: _abi.FA_F64,
    torch.bfloat16: _abi.FA_BF16,
    torch.float16: _abi.FA_F16,
    torch.int32: _abi.FA_I32,
    torch.int64: _abi.FA_I64,
    # narrow / unsigned integers: fa_cast and the IFOLD / NFOLD folds only (the per-tensor path)
    torch.int8: _abi.FA_I8,
    torch.int16: _abi.FA_I16,
    torch.uint8: _abi.FA_U8,
    torch.uint16: _abi.FA_U16,
    torch.uint32: _abi.FA_U32,
    torch.uint64: _abi.FA_U64,
}
_FA_TO_TORCH = {v: k for k, v in _TORCH_TO_FA.items()}
_NP_TO_TORCH = {
    np.dtype(np.float32): torch.float32,
    np.dtype(np.float64): torch.float64,
    np.dtype(np.float16): torch.float16,
    np.dtype(np.int32): torch.int32,
    np.dtype(np.int64): torch.int64,
    np.dtype(np.int8): torch.int8,
    np.dtype(np.int16): torch.int16,
    np.dtype(np.uint8): torch.uint8,
    np.dtype(np.uint16): torch.uint16,
    np.dtype(np.uint32): torch.uint32,
    np.dtype(np.uint64): torch.uint64,
    np.dtype(np.bool_): torch.bool,        # staged / returned as is; no kernel takes it (numpy never folds bool)
}
_TORCH_TO_NP = {v: k for k, v in _NP_TO_TORCH.items()}


def fa_dtype(t):
    dt = t.dtype if isinstance(t, torch.Tensor) else t
    if isinstance(dt, np.dtype) or (isinstance(dt, type) and issubclass(dt, np.generic)):
        dt = torch_dtype(dt)
    try:
        return _TORCH_TO_FA[dt]
    except KeyError:
        raise TypeError(f"dtype {dt} is not supported by libfedagg") from None


def torch_dtype(np_dtype):
    try:
        return _NP_TO_TORCH[np.dtype(np_dtype)]
    except KeyError:
        raise TypeError(f"numpy dtype {np_dtype} is not supported by libfedagg") from None


def numpy_dtype(torch_dt):
    if torch_dt == torch.bfloat16:
        raise TypeError("bfloat16 has no numpy dtype")
    return _TORCH_TO_NP[torch_dt]


def fold_result_dtype(agg_dt, upd_dt, nfolds=1):
    """dtype of ``np.add(x, n*(y-x)/N)`` for x: agg_dt, y: upd_dt (torch dtypes).

    bf16 (no numpy counterpart) accumulates in f32. Integer inputs become f64 on the
    first fold (numpy true_divide). ``nfolds == 0`` means "no fold yet" (plain alias).
    """
    if nfolds == 0:
        return upd_dt
    ints = (torch.int32, torch.int64)
    if agg_dt in ints or upd_dt in ints:
        return torch.float64
    if torch.float64 in (agg_dt, upd_dt):
        return torch.float64
    if agg_dt == torch.float16 and upd_dt == torch.float16:
        return torch.float16
    return torch.float32


def _stream_handle(t, stream):
    if stream is None:
        stream = torch.cuda.current_stream(t.device)
    return ctypes_stream(stream)


def ctypes_stream(stream):
    return int(stream.cuda_stream) if stream is not None else 0


def _check_dev(name, t, P, device):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if t.device.type != "cuda":
        raise ValueError(f"{name} must be a device (cuda/hip) tensor, got {t.device}")
    if device is not None and t.device != device:
        raise ValueError(f"{name} is on {t.device}, expected {device}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if t.numel() != P:
        raise ValueError(f"{name} has {t.numel()} elements, expected {P}")


def fedavg_fold(agg, updates, n, N, init, stream=None):
    """FedAvg fold on device (``fa_fedavg_fold``): numpyhelper.py:32 replayed in queue order.

    agg      flat device tensor (running model; written)
    updates  sequence of flat device tensors of the same length
    n, N     per-update num_examples and running totals (python numbers)
    init     True: agg := updates[0] then fold updates[1:]; False: fold all into agg
    """
    lib = _abi.load()
    K = len(updates)
    if len(n) != K or len(N) != K:
        raise ValueError("n and N must have one entry per update")
    P = agg.numel()
    dev = agg.device
    _check_dev("agg", agg, P, None)
    upd_dt = updates[0].dtype if K else agg.dtype
    for i, u in enumerate(updates):
        _check_dev(f"updates[{i}]", u, P, dev)
        if u.dtype != upd_dt:
            raise TypeError("all updates in one fold call must share a dtype")
    # the integer first fold multiplies in the update dtype: numpy's rule for a python int n[1], and for a
    # numpy integer only when the product keeps that dtype (np.int64(3) * int32 is int64: mixed._int_fold_kind)
    if init and K > 1 and upd_dt in (torch.int32, torch.int64) and isinstance(n[1], np.integer) \
            and np.result_type(n[1], numpy_dtype(upd_dt)) != numpy_dtype(upd_dt):
        raise TypeError(f"a {type(n[1]).__name__} num_examples times a {numpy_dtype(upd_dt)} difference is not "
                        f"the integer first fold's product")
    with _on(dev):        # launch on the tensors' device (multi-GPU processes)
        st = _stream_handle(agg, stream)
        rc = lib.fa_fedavg_fold(agg.data_ptr(), fa_dtype(agg), _abi.ptr_array([u.data_ptr() for u in updates]),
                                fa_dtype(upd_dt), _abi.double_array(n), _abi.double_array(N), K, P, int(bool(init)), st)
    _abi.check(rc)
    return agg


def fedavg_fold_ptrs(agg, ptrs, upd_dtype, n, N, init, stream=None):
    """:func:`fedavg_fold` with the client table given as device addresses (ints) of ``agg.numel()``
    elements of ``upd_dtype`` each, on ``agg``'s device: the pipelines' own staging buffers, whose
    extent they guarantee (no per-update tensor view or check)."""
    lib = _abi.load()
    K = len(ptrs)
    if len(n) != K or len(N) != K:
        raise ValueError("n and N must have one entry per update")
    P = agg.numel()
    _check_dev("agg", agg, P, None)
    args = (agg.data_ptr(), fa_dtype(agg), (ctypes.c_void_p * max(1, K))(*ptrs), fa_dtype(upd_dtype),
            (ctypes.c_double * max(1, K))(*n), (ctypes.c_double * max(1, K))(*N), K, P, int(bool(init)))
    if agg.device.index == torch.cuda.current_device():      # the common case: no device switch
        rc = lib.fa_fedavg_fold(*args, _stream_handle(agg, stream))
    else:
        with _on(agg.device):
            rc = lib.fa_fedavg_fold(*args, _stream_handle(agg, stream))
    _abi.check(rc)
    return agg


def weighted_sum(acc, updates, w, stream=None):
    """``acc[i] += updates[k][i] * w[k]`` for k in order (``fa_weighted_sum``): the loop of the
    reference's server-function example aggregate (server_functions.py:58-67), numpy rounding."""
    lib = _abi.load()
    K = len(updates)
    if len(w) != K:
        raise ValueError("w must have one entry per update")
    P = acc.numel()
    dev = acc.device
    _check_dev("acc", acc, P, None)
    upd_dt = updates[0].dtype if K else acc.dtype
    for i, u in enumerate(updates):
        _check_dev(f"updates[{i}]", u, P, dev)
        if u.dtype != upd_dt:
            raise TypeError("all updates in one weighted_sum call must share a dtype")
    with _on(dev):
        st = _stream_handle(acc, stream)
        rc = lib.fa_weighted_sum(acc.data_ptr(), fa_dtype(acc), _abi.ptr_array([u.data_ptr() for u in updates]),
                                 fa_dtype(upd_dt), _abi.double_array(w), K, P, st)
    _abi.check(rc)
    return acc


MAX_ORDER_K = 64      # clients of one fa_trimmed_mean call (the kernarg table; one sorting network)


def order_mean_dtype(upd_dt):
    """dtype of the trimmed mean / median of updates of torch dtype ``upd_dt``: numpy's
    ``np.sort(S, 0)[t:K-t].mean(0)`` dtype — the float dtype itself, float64 for integers — and
    float32 for bf16 (the fp32 rule on exact upcasts)."""
    if upd_dt in (torch.float32, torch.float64, torch.float16):
        return upd_dt
    if upd_dt == torch.bfloat16:
        return torch.float32
    if upd_dt in (torch.int32, torch.int64):
        return torch.float64
    raise TypeError(f"trimmed_mean: dtype {upd_dt} is not supported")


def median_trim(K):
    """The trim count that makes the trimmed mean the median: the middle value of an odd K, the mean
    of the two middle values of an even one."""
    return (K - 1) // 2


def trimmed_mean(out, updates, trim, stream=None):
    """Coordinate-wise trimmed mean on device (``fa_trimmed_mean``): per element, the ``trim``
    smallest and ``trim`` largest of the K updates' values are dropped (-0 before +0, NaNs last) and
    the rest averaged in ascending order — ``np.sort(S, 0)[trim:K-trim].mean(0)`` bit for bit.

    out      flat device tensor of :func:`order_mean_dtype` of the updates' dtype (written)
    updates  1 <= K <= 64 flat device tensors of one dtype and of ``out``'s length
    trim     0 <= trim, 2 * trim < K
    """
    lib = _abi.load()
    K = len(updates)
    if not 1 <= K <= MAX_ORDER_K:
        raise ValueError(f"trimmed_mean takes 1..{MAX_ORDER_K} updates, got {K}")
    P = out.numel()
    dev = out.device
    _check_dev("out", out, P, None)
    upd_dt = updates[0].dtype
    for i, u in enumerate(updates):
        _check_dev(f"updates[{i}]", u, P, dev)
        if u.dtype != upd_dt:
            raise TypeError("all updates in one trimmed_mean call must share a dtype")
    with _on(dev):
        st = _stream_handle(out, stream)
        rc = lib.fa_trimmed_mean(out.data_ptr(), fa_dtype(out), _abi.ptr_array([u.data_ptr() for u in updates]),
                                 fa_dtype(upd_dt), K, int(trim), P, st)
    _abi.check(rc)
    return out


def median_window_mean(out, updates, keep, stream=None):
    """Coordinate-wise mean of the values closest to the median on device (``fa_median_window_mean``,
    Bulyan's second stage): per element, the K updates' values are sorted (-0 before +0, NaNs last), the
    window of ``keep`` consecutive sorted values closest to their median is found (a tie keeps the lower
    window) and averaged in ascending order. ``keep = K`` is :func:`trimmed_mean` at ``trim = 0`` bit for
    bit.

    out      flat device tensor of :func:`order_mean_dtype` of the updates' dtype (written)
    updates  1 <= K <= 64 flat device tensors of one dtype and of ``out``'s length
    keep     1 <= keep <= K
    """
    lib = _abi.load()
    K = len(updates)
    if not 1 <= K <= MAX_ORDER_K:
        raise ValueError(f"median_window_mean takes 1..{MAX_ORDER_K} updates, got {K}")
    P = out.numel()
    dev = out.device
    _check_dev("out", out, P, None)
    upd_dt = updates[0].dtype
    for i, u in enumerate(updates):
        _check_dev(f"updates[{i}]", u, P, dev)
        if u.dtype != upd_dt:
            raise TypeError("all updates in one median_window_mean call must share a dtype")
    with _on(dev):
        st = _stream_handle(out, stream)
        rc = lib.fa_median_window_mean(out.data_ptr(), fa_dtype(out), _abi.ptr_array([u.data_ptr() for u in updates]),
                                       fa_dtype(upd_dt), K, int(keep), P, st)
    _abi.check(rc)
    return out


def median(out, updates, stream=None):
    """Coordinate-wise median on device: :func:`trimmed_mean` with ``trim = (K - 1) // 2``
    (``np.median(S, 0)`` bit for bit)."""
    return trimmed_mean(out, updates, median_trim(len(updates)), stream)


_SQDIST_F32 = (torch.float32, torch.float16, torch.bfloat16)
_SQDIST_F64 = (torch.float64, torch.int32, torch.int64)


def _geometry(entry, dtype, K):
    """The four ints of the probe library's geometry query ``entry`` for K updates of ``dtype``."""
    te, r, wg, ft = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _abi.check(getattr(_abi.load_probe(), entry)(fa_dtype(dtype), int(K), ctypes.byref(te), ctypes.byref(r),
                                                 ctypes.byref(wg), ctypes.byref(ft)))
    return te.value, r.value, wg.value, ft.value


def sqdist_geometry(dtype, K):
    """``(TE, R, max workgroups, tiles per flush)`` of ``fa_pairwise_sqdist`` for K updates of ``dtype``:
    the elements a workgroup stages at a time, the longest chain summed in the compute type, the largest
    grid, and the tiles a workgroup walks before it flushes its chains to f64. A measurement entry point
    (libfedagg_probe.so, the same source as the product library): tools and tests place sizes with it."""
    return _geometry("fa_pairwise_sqdist_geometry", dtype, K)


def sqdist_rtol(dtype, P):
    """Relative error bound of every entry of :func:`pairwise_sqdist` against exact arithmetic on the
    converted values: ``(R + 4) * 2**-24`` for float32 / float16 / bfloat16 updates (chains of at most R
    terms in f32, summed in f64), ``(P + 4) * 2**-53`` for float64 / int32 / int64 ones.
    R is the library's compile-time constant ``FA_PAIR_CHAIN_TERMS`` (include/fedagg.h)."""
    dt = dtype if isinstance(dtype, torch.dtype) else torch_dtype(dtype)
    if dt in _SQDIST_F32:
        return (_abi.PAIR_CHAIN_TERMS + 4) * 2.0 ** -24
    if dt in _SQDIST_F64:
        return (int(P) + 4) * 2.0 ** -53
    raise TypeError(f"pairwise_sqdist: dtype {dt} is not supported")


def _distance_updates(name, updates):
    """The checks the three distance ops make of their updates, in ``name``'s words: 1..64 flat
    contiguous tensors of one supported dtype, one length and one device. Returns ``(K, P, dev, upd_dt)``."""
    K = len(updates)
    if not 1 <= K <= MAX_ORDER_K:
        raise ValueError(f"{name} takes 1..{MAX_ORDER_K} updates, got {K}")
    if not isinstance(updates[0], torch.Tensor):
        raise TypeError("updates[0] must be a torch.Tensor")
    P = updates[0].numel()
    dev = updates[0].device
    upd_dt = updates[0].dtype
    if upd_dt not in _SQDIST_F32 and upd_dt not in _SQDIST_F64:
        raise TypeError(f"{name}: dtype {upd_dt} is not supported")
    for i, u in enumerate(updates):
        _check_dev(f"updates[{i}]", u, P, dev)
        if u.dtype != upd_dt:
            raise TypeError(f"all updates in one {name} call must share a dtype")
    return K, P, dev, upd_dt


def _check_point(name, arg, t, P, dev, upd_dt):
    """``t`` (argument ``arg``) holds a point of the updates' space: P elements of their output dtype."""
    _check_dev(arg, t, P, dev)
    if t.dtype != order_mean_dtype(upd_dt):
        raise TypeError(f"{name}: {arg} must be {order_mean_dtype(upd_dt)} for {upd_dt} updates, got {t.dtype}")


def _check_outputs(name, dev, accumulate, arg, what, sums, n, out=None, P=0, upd_dt=None):
    """The output checks of a distance op: ``out`` where given is a point (:func:`_check_point`); the
    sums ``sums`` (argument ``arg``, "the ``what``" in words) are n float64 values, or None — then there is
    nothing to ``accumulate`` into."""
    if out is not None:
        _check_point(name, "out", out, P, dev, upd_dt)
    if sums is None:
        if accumulate:
            raise ValueError(f"{name}: accumulate needs the {what} to add to ({arg})")
    else:
        _check_dev(arg, sums, n, dev)
        if sums.dtype != torch.float64:
            raise TypeError(f"{name}: {arg} must be float64, got {sums.dtype}")


def _stream_alloc(dev, stream, nwork, sums, shape, out=None, fresh_out=None):
    """The launching stream ``s`` and, allocated under it (scratch and fresh outputs belong to the stream
    that launches: DESIGN.md §3.7): ``out`` where None and wanted (``fresh_out``: its ``(P, dtype)``),
    the float64 ``sums`` of ``shape`` where None, and ``nwork`` doubles of scratch. Returns
    ``(s, out, sums, work)``; called on ``dev``."""
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.stream(s):
        if out is None and fresh_out is not None:
            out = torch.empty(fresh_out[0], dtype=fresh_out[1], device=dev)
        if sums is None:
            sums = torch.empty(shape, dtype=torch.float64, device=dev)
        work = torch.empty(max(1, int(nwork)), dtype=torch.float64, device=dev)
    return s, out, sums, work


def pairwise_sqdist(updates, out=None, accumulate=False, stream=None):
    """Squared Euclidean distances between K updates on device (``fa_pairwise_sqdist``): a K x K
    float64 device tensor, exactly symmetric with a zero diagonal, every entry within
    :func:`sqdist_rtol` of the exact sum, the same bits on every call.

    updates     1 <= K <= 64 flat device tensors of one dtype (float32 / float64 / float16 / bfloat16 /
                int32 / int64) and one length
    out         K x K float64 device tensor (contiguous); allocated when None
    accumulate  add this call's distances to ``out`` instead of writing it (dtype groups, slices)
    """
    lib = _abi.load()
    K, P, dev, upd_dt = _distance_updates("pairwise_sqdist", updates)
    _check_outputs("pairwise_sqdist", dev, accumulate, "out", "matrix", out, K * K)
    with _on(dev):
        s, _, out, work = _stream_alloc(dev, stream, lib.fa_pairwise_sqdist_work(K, P), out, (K, K))
        rc = lib.fa_pairwise_sqdist(out.data_ptr(), _abi.ptr_array([u.data_ptr() for u in updates]), fa_dtype(upd_dt),
                                    K, P, int(bool(accumulate)), work.data_ptr(), ctypes_stream(s))
    _abi.check(rc)
    return out


def wmean_geometry(dtype, K):
    """``(TE, chain, max workgroups, tiles per flush)`` of ``fa_weighted_mean_sqdist`` for K updates of
    ``dtype``: the elements a workgroup stages at a time, the longest chain its kernel sums in the
    compute type (at most R of :func:`sqdist_rtol`), the largest grid, and the tiles a workgroup walks
    between two flushes of its chains to f64. A measurement entry point (libfedagg_probe.so) like
    :func:`sqdist_geometry`."""
    return _geometry("fa_wmean_sqdist_geometry", dtype, K)


def weighted_mean_sqdist(updates, beta, out=None, dist=None, accumulate=False, store=True, stream=None):
    """One smoothed Weiszfeld step on device (``fa_weighted_mean_sqdist``): the weighted mean
    ``z = sum_k beta[k] * u_k`` of K updates — summed in index order in the compute type over the clients
    with a nonzero weight, rounded once to :func:`order_mean_dtype` of the updates' dtype — and the K
    squared distances ``sum_p (u_k[p] - z[p])**2`` of EVERY update to it, each within
    :func:`sqdist_rtol` of the exact sum, in one pass that reads every update once. Returns
    ``(out or None, dist)``; the same bits on every call.

    updates     1 <= K <= 64 flat device tensors of one dtype (float32 / float64 / float16 / bfloat16 /
                int32 / int64) and one length
    beta        K weights, finite and >= 0, not all zero (they need not sum to 1)
    out         flat device tensor for z; allocated when None and ``store``
    dist        K float64 device values; allocated when None
    accumulate  add this call's distances to ``dist`` instead of writing it (dtype groups, slices)
    store       False: z is formed for the distances but not stored (``out`` is left alone; None is returned)
    """
    lib = _abi.load()
    K, P, dev, upd_dt = _distance_updates("weighted_mean_sqdist", updates)
    out_dt = order_mean_dtype(upd_dt)
    beta = [float(b) for b in beta]
    if len(beta) != K:
        raise ValueError(f"weighted_mean_sqdist: {len(beta)} weights for {K} updates")
    _check_outputs("weighted_mean_sqdist", dev, accumulate, "dist", "distances", dist, K, out, P, upd_dt)
    with _on(dev):
        s, out, dist, work = _stream_alloc(dev, stream, lib.fa_wmean_sqdist_work(K, P), dist, K, out,
                                           (P, out_dt) if store else None)
        rc = lib.fa_weighted_mean_sqdist(out.data_ptr() if store else None, fa_dtype(out_dt), dist.data_ptr(),
                                         _abi.ptr_array([u.data_ptr() for u in updates]), fa_dtype(upd_dt),
                                         _abi.double_array(beta), K, P, int(bool(accumulate)), work.data_ptr(),
                                         ctypes_stream(s))
    _abi.check(rc)
    return (out if store else None), dist


def cclip_geometry(dtype, K):
    """``(TE, chain, max workgroups, tiles per flush)`` of ``fa_centered_clip_step`` for K updates of
    ``dtype``, as :func:`wmean_geometry` (its tile holds one more column, the centre's). A measurement
    entry point (libfedagg_probe.so)."""
    return _geometry("fa_centered_clip_geometry", dtype, K)


def centered_clip_step(updates, center, coef, out=None, dist=None, accumulate=False, store=True, stream=None):
    """One centred-clipping step on device (``fa_centered_clip_step``): the new point
    ``v' = v + sum_k coef[k] * (u_k - v)`` — the differences to the centre ``v`` taken first, summed in
    index order in the compute type over the clients with a nonzero coefficient, rounded once to
    :func:`order_mean_dtype` of the updates' dtype — and the K squared distances ``sum_p (u_k[p] - v'[p])**2``
    of EVERY update to it, each within :func:`sqdist_rtol` of the exact sum, in one pass that reads every
    update and the centre once. Returns ``(out or None, dist)``; the same bits on every call.

    updates     1 <= K <= 64 flat device tensors of one dtype (float32 / float64 / float16 / bfloat16 /
                int32 / int64) and one length
    center      flat device tensor of :func:`order_mean_dtype` of the updates' dtype, of the same length
    coef        K coefficients, finite and >= 0; all zero is legal (v' = v: the distances to the centre)
    out         flat device tensor for v': ``center`` itself (in place) or one that does not overlap it;
                allocated when None and ``store``
    dist        K float64 device values; allocated when None
    accumulate  add this call's distances to ``dist`` instead of writing it (dtype groups, slices)
    store       False: v' is formed for the distances but not stored (``out`` is left alone; None is returned)
    """
    lib = _abi.load()
    K, P, dev, upd_dt = _distance_updates("centered_clip_step", updates)
    out_dt = order_mean_dtype(upd_dt)
    _check_point("centered_clip_step", "center", center, P, dev, upd_dt)
    coef = [float(c) for c in coef]
    if len(coef) != K:
        raise ValueError(f"centered_clip_step: {len(coef)} coefficients for {K} updates")
    _check_outputs("centered_clip_step", dev, accumulate, "dist", "distances", dist, K, out, P, upd_dt)
    with _on(dev):
        s, out, dist, work = _stream_alloc(dev, stream, lib.fa_centered_clip_work(K, P), dist, K, out,
                                           (P, out_dt) if store else None)
        # (an empty tensor has no address and the library refuses a null centre: at P = 0 nothing reads it)
        cptr = center.data_ptr() if P else work.data_ptr()
        rc = lib.fa_centered_clip_step((out.data_ptr() or None) if store else None, cptr, fa_dtype(out_dt),
                                       dist.data_ptr(), _abi.ptr_array([u.data_ptr() for u in updates]),
                                       fa_dtype(upd_dt), _abi.double_array(coef), K, P, int(bool(accumulate)),
                                       work.data_ptr(), ctypes_stream(s))
    _abi.check(rc)
    return (out if store else None), dist


MAX_CLIP_K = 1024     # clients of one round of the clipping rules that fold by chunks (clip_fold): 16 launches' tables


def clip_compute_dtype(upd_dt):
    """The compute type of the distance and clipping kernels for updates of torch dtype ``upd_dt``: float32
    for float32 / float16 / bfloat16, float64 for float64 / int32 / int64. A carry of :func:`clip_fold` has it."""
    if upd_dt in _SQDIST_F32:
        return torch.float32
    if upd_dt in _SQDIST_F64:
        return torch.float64
    raise TypeError(f"clip_fold: dtype {upd_dt} is not supported")


def clip_fold(updates, center, coef, out=None, carry_in=None, carry_out=None, stream=None):
    """Up to 64 clients of a centred-clipping step folded into a running accumulator on device
    (``fa_clip_fold``, kernel ``k_clip_fold``): per element ``acc = carry_in`` (else the centre), then
    ``acc = acc + coef[k] * (u_k - center)`` over the clients with a nonzero coefficient in index order, every
    operation rounded once in the compute type; ``carry_out = acc`` and ``out = acc`` rounded once to
    :func:`order_mean_dtype` of the updates' dtype. A chain of calls over consecutive chunks of a round — the
    first without ``carry_in``, the last with ``out`` — is :func:`centered_clip_step`'s new point bit for bit,
    for any number of clients and wherever the chain is cut. Returns ``(out, carry_out)``
    as given; the same bits on every call.

    updates    1 <= K <= 64 flat device tensors of one dtype (float32 / float64 / float16 / bfloat16 /
               int32 / int64) and one length
    center     flat device tensor of :func:`order_mean_dtype` of the updates' dtype, of the same length;
               the differences are taken to it, and it is not modified unless ``out`` is it
    coef       K coefficients, finite and >= 0; a client with coefficient 0 is not read; all zero is legal
    out        None, ``center`` itself (in place) or a tensor like it that overlaps nothing else
    carry_in   None, or the accumulator so far: a flat device tensor of :func:`clip_compute_dtype`
    carry_out  None, ``carry_in`` itself, or a tensor like it that overlaps nothing else; at least one of
               ``out`` and ``carry_out`` is given
    """
    lib = _abi.load()
    K, P, dev, upd_dt = _distance_updates("clip_fold", updates)
    out_dt, c_dt = order_mean_dtype(upd_dt), clip_compute_dtype(upd_dt)
    _check_point("clip_fold", "center", center, P, dev, upd_dt)
    coef = [float(c) for c in coef]
    if len(coef) != K:
        raise ValueError(f"clip_fold: {len(coef)} coefficients for {K} updates")
    if out is None and carry_out is None:
        raise ValueError("clip_fold: one of out and carry_out is needed")
    if out is not None:
        _check_point("clip_fold", "out", out, P, dev, upd_dt)
    for arg, t in (("carry_in", carry_in), ("carry_out", carry_out)):
        if t is not None:
            _check_dev(arg, t, P, dev)
            if t.dtype != c_dt:
                raise TypeError(f"clip_fold: {arg} must be {c_dt} for {upd_dt} updates, got {t.dtype}")
    # the two legal aliases: out is the centre, carry_out is carry_in; any other overlap that involves one of
    # those four buffers is refused (the library checks the same at the pointers' level)
    named = [("out", out), ("carry_out", carry_out), ("carry_in", carry_in), ("center", center)]
    spans = [(n, t.data_ptr(), P * t.element_size()) for n, t in named if t is not None]
    for i, (na, a, la) in enumerate(spans):
        for nb, b, lb in spans[i + 1:]:
            if a == b and (na, nb) in (("out", "center"), ("carry_out", "carry_in")):
                continue
            if a < b + lb and b < a + la:
                raise ValueError(f"clip_fold: {na} and {nb} overlap")
        for k, u in enumerate(updates):
            b, lb = u.data_ptr(), P * u.element_size()
            if a < b + lb and b < a + la:
                raise ValueError(f"clip_fold: {na} and updates[{k}] overlap")
    if P == 0:
        return out, carry_out
    with _on(dev):
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        rc = lib.fa_clip_fold(out.data_ptr() if out is not None else None, fa_dtype(out_dt),
                              carry_out.data_ptr() if carry_out is not None else None,
                              carry_in.data_ptr() if carry_in is not None else None, center.data_ptr(),
                              _abi.ptr_array([u.data_ptr() for u in updates]), fa_dtype(upd_dt),
                              _abi.double_array(coef), K, P, ctypes_stream(s))
    _abi.check(rc)
    return out, carry_out


NOISE_DTYPES = (torch.float32, torch.float64, torch.float16)      # order_mean_dtype's outputs


def gaussian_noise(out, x=None, *, sigma, seed, stream_id=0, round_id=0, offset=0, stream=None):
    """Gaussian noise added to a buffer on device (``fa_gaussian_noise``, kernel ``k_gaussian_noise``):
    ``out[j] = O(double(x[j]) + sigma * z(offset + j))`` with ``z(i)`` the N(0, 1) deviate that is a pure
    function of ``(seed, stream_id, round_id, i)`` (Philox4x32-10 and Box-Muller in float64, DESIGN.md
    §3.12; ``tests/dpnoise_ref.py`` restates it in numpy). The product and the sum are rounded once in
    float64 and the result once to ``out``'s dtype. The same bits on every call, for every split of a
    range into calls at their offsets and at every pointer alignment.

    out        flat device tensor, float32 / float64 / float16 (written)
    x          ``out`` itself (in place, the normal use), a tensor of the same dtype, length and device
               that does not overlap it, or None: zeros
    sigma      the noise's standard deviation, finite and >= 0
    seed       0 .. 2^64 - 1
    stream_id, round_id   0 .. 2^32 - 1: the dtype group and the round of a session
    offset     the index of ``out[0]`` in the stream, >= 0, ``offset + len(out) <= 2^63 - 1``
    """
    lib = _abi.load()
    P = out.numel() if isinstance(out, torch.Tensor) else 0
    _check_dev("out", out, P, None)
    if out.dtype not in NOISE_DTYPES:
        raise TypeError(f"gaussian_noise: out must be float32, float64 or float16, got {out.dtype}")
    if x is not None:
        _check_dev("x", x, P, out.device)
        if x.dtype != out.dtype:
            raise TypeError(f"gaussian_noise: x is {x.dtype}, out is {out.dtype}")
        a, b, nbytes = out.data_ptr(), x.data_ptr(), P * out.element_size()
        if a != b and a < b + nbytes and b < a + nbytes:
            raise ValueError("gaussian_noise: out and x overlap without being the same buffer")
    sigma = float(sigma)
    if not (sigma >= 0.0 and sigma != float("inf")):
        raise ValueError(f"gaussian_noise: sigma must be finite and >= 0, got {sigma}")
    for name, v, bits in (("seed", seed, 64), ("stream_id", stream_id, 32), ("round_id", round_id, 32), ("offset", offset, 63)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) < 1 << bits:
            raise ValueError(f"gaussian_noise: {name} must be an int in 0 .. 2^{bits} - 1, got {v!r}")
    if int(offset) + P > (1 << 63) - 1:
        raise ValueError(f"gaussian_noise: offset + len(out) passes 2^63 - 1 (offset={offset}, {P} elements)")
    if P == 0:
        return out
    with _on(out.device):
        st = _stream_handle(out, stream)
        rc = lib.fa_gaussian_noise(out.data_ptr(), x.data_ptr() if x is not None else None, fa_dtype(out), sigma,
                                   int(seed), int(stream_id), int(round_id), int(offset), P, st)
    _abi.check(rc)
    return out


def running_mean(g, m, a, b, T, stream=None):
    """``g = (g*a + m*b)/T`` in place (``fa_running_mean``): one step of the reference's
    incremental server-function example (sf_incremental_aggregation.py:36-37)."""
    lib = _abi.load()
    P = g.numel()
    _check_dev("g", g, P, None)
    _check_dev("m", m, P, g.device)
    if m.dtype != g.dtype:
        raise TypeError(f"running_mean: model dtype {m.dtype} differs from the running model's {g.dtype}")
    with _on(g.device):
        st = _stream_handle(g, stream)
        rc = lib.fa_running_mean(g.data_ptr(), fa_dtype(g), m.data_ptr(), float(a), float(b), float(T), P, st)
    _abi.check(rc)
    return g


_OPTS = {"adam": _abi.FA_ADAM, "yogi": _abi.FA_YOGI, "adagrad": _abi.FA_ADAGRAD}


def promote(a, b):
    """numpy result dtype for the FedOpt elementwise pairs (torch dtypes; None = absent)."""
    if a is None:
        a, b = b, None
    if b is None:
        return torch.float32 if a == torch.bfloat16 else a
    a = torch.float32 if a == torch.bfloat16 else a
    b = torch.float32 if b == torch.bfloat16 else b
    if a == b:
        return a
    if torch.float64 in (a, b):
        return torch.float64
    return torch.float32


def fedopt_dtypes(upd_dt, old_dt, m_dt):
    """(pg dtype, m_out dtype) for fedopt.py's expressions; v and out are always f64.
    Integer updates: ``next*1.0 + old*(-1.0)`` is float64 in numpy (int array * python float)."""
    pg = torch.float64 if upd_dt in (torch.int32, torch.int64) else promote(upd_dt, old_dt)
    return pg, promote(m_dt, pg)


def fedopt_step(old, updates, n, N, *, first, final, pg=None, m_in=None, m_out=None, v_in=None, v_out=None,
                out=None, serveropt="adam", learning_rate=1e-3, beta1=0.9, beta2=0.99, tau=1e-4, stream=None,
                upd_dtype=None):
    """Fused FedOpt step on device (``fa_fedopt_step``), fedopt.py:74-118 + 151-258.

    ``upd_dtype``: dtype of the round's client updates; required when ``updates`` is empty
    (a server step on an accumulated ``pg``), because it fixes the pseudo-gradient dtype."""
    lib = _abi.load()
    if serveropt not in _OPTS:
        raise ValueError(f"Unsupported server optimizer: {serveropt}")
    K = len(updates)
    P = old.numel()
    dev = old.device
    _check_dev("old", old, P, None)
    if K:
        upd_dt = updates[0].dtype
    elif upd_dtype is not None:
        upd_dt = upd_dtype
    elif pg is not None and pg.dtype == torch.float64 and old.dtype != torch.float64:
        raise ValueError("fedopt_step without updates needs upd_dtype (pg is float64, old is not)")
    else:
        upd_dt = pg.dtype if pg is not None else old.dtype
    for i, u in enumerate(updates):
        _check_dev(f"updates[{i}]", u, P, dev)
        if u.dtype != upd_dt:
            raise TypeError("all updates in one call must share a dtype")
    if pg is not None and pg.dtype != fedopt_dtypes(upd_dt, old.dtype, None)[0]:
        raise TypeError(f"pg must be {fedopt_dtypes(upd_dt, old.dtype, None)[0]} for {upd_dt} updates over a "
                        f"{old.dtype} model")
    for name, t in (("pg", pg), ("m_in", m_in), ("m_out", m_out), ("v_in", v_in), ("v_out", v_out), ("out", out)):
        if t is not None:
            _check_dev(name, t, P, dev)
    if v_in is not None and v_in.dtype not in (torch.float64, torch.float32):
        raise TypeError("v must be float64 (fedopt.py:171: np.ones(...) * tau**2), or float32 (fp32-state mode)")
    # the storage dtype of the server state: out's (float64: the reference's flow; float32: the
    # fp32-state mode, fa_fedopt_step_ex — v and the model stored as f32, m as f32 or numpy's dtype)
    state_dt = out.dtype if out is not None else torch.float64
    if state_dt not in (torch.float64, torch.float32):
        raise TypeError("out must be float64 (the reference's model dtype) or float32 (fp32-state mode)")
    pg_dt, m_np = fedopt_dtypes(upd_dt, old.dtype, None if m_in is None else m_in.dtype)
    if final:
        if m_out is None or v_out is None or out is None:
            raise ValueError("final step needs m_out, v_out and out")
        if v_out.dtype != state_dt:
            raise TypeError(f"v_out must be {state_dt}, like out")
        if m_out.dtype != m_np and not (state_dt == torch.float32 and m_out.dtype == torch.float32):
            raise TypeError(f"output dtypes: m_out {m_np}" + (" or float32" if state_dt == torch.float32 else "") +
                            f", v_out/out {state_dt}")
    flags = (_abi.FA_PG_FIRST if first else 0) | (_abi.FA_PG_FINAL if final else 0)
    ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
    with _on(dev):
        st = _stream_handle(old, stream)
        rc = lib.fa_fedopt_step_ex(
            old.data_ptr(), fa_dtype(old), _abi.ptr_array([u.data_ptr() for u in updates]), fa_dtype(upd_dt),
            _abi.double_array(n), _abi.double_array(N), K, ptr(pg), flags,
            ptr(m_in), _abi.FA_NONE if m_in is None else fa_dtype(m_in), ptr(m_out),
            fa_dtype(m_out) if m_out is not None else fa_dtype(m_np),
            ptr(v_in), _abi.FA_F64 if v_in is None else fa_dtype(v_in), ptr(v_out), ptr(out),
            fa_dtype(state_dt), _OPTS[serveropt], float(learning_rate), float(beta1), float(beta2), float(tau), P, st)
    _abi.check(rc)


def fedopt_step_raw(old_ptr, old_dt, upd_ptrs, upd_dt, n, N, P, *, first, final, pg_ptr=0, m_in=None, m_out=None,
                    v_in=None, v_out=None, out_ptr=0, state_dt=torch.float64, serveropt="adam", learning_rate=1e-3,
                    beta1=0.9, beta2=0.99, tau=1e-4, stream=None, device=None):
    """:func:`fedopt_step` with the global model, the client table, pg and the new model given as
    device addresses of ``P`` elements each — pinned host memory's device addresses included (a
    small round folded zero-copy, staging.FedOptPipeline) — and no tensor view per update; m / v
    are device tensors as in :func:`fedopt_step`. For the pipelines' own buffers, whose extents
    and dtypes they guarantee (the dtype rules are the same; the C ABI checks the pairs)."""
    if serveropt not in _OPTS:
        raise ValueError(f"Unsupported server optimizer: {serveropt}")
    K = len(upd_ptrs)
    if len(n) != K or len(N) != K:
        raise ValueError("fedopt_step_raw: one n and N per update")
    if final and (m_out is None or v_out is None or not out_ptr):
        raise ValueError("final step needs m_out, v_out and out")
    _, m_np = fedopt_dtypes(upd_dt, old_dt, None if m_in is None else m_in.dtype)
    flags = (_abi.FA_PG_FIRST if first else 0) | (_abi.FA_PG_FINAL if final else 0)
    ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
    with _on(device):
        rc = _abi.load().fa_fedopt_step_ex(
            int(old_ptr), fa_dtype(old_dt), _abi.ptr_array([int(u) for u in upd_ptrs]), fa_dtype(upd_dt),
            _abi.double_array(n), _abi.double_array(N), K, int(pg_ptr), flags,
            ptr(m_in), _abi.FA_NONE if m_in is None else fa_dtype(m_in), ptr(m_out),
            fa_dtype(m_out.dtype if m_out is not None else m_np),
            ptr(v_in), _abi.FA_F64 if v_in is None else fa_dtype(v_in), ptr(v_out), int(out_ptr),
            fa_dtype(state_dt), _OPTS[serveropt], float(learning_rate), float(beta1), float(beta2), float(tau), int(P),
            ctypes_stream(stream))
    _abi.check(rc)


def cast_dims(oshape, x):
    """The (extents, strides) ``fa_cast`` walks to broadcast the strided device tensor ``x`` to the
    contiguous shape ``oshape``. Host arithmetic only: raises ValueError where ``x`` does not broadcast to
    ``oshape``, or where more than 8 dimensions remain after merging (the kernel's limit), so a caller can
    refuse such an operand before it launches anything."""
    oshape = tuple(oshape)
    xshape = tuple(x.shape)
    if len(xshape) > len(oshape):
        raise ValueError(f"cast: cannot broadcast {xshape} to {oshape}")
    # right-align x's dims to out's (numpy broadcasting); stride 0 where x has extent 1
    lead = len(oshape) - len(xshape)
    strides = [0] * lead
    for d, (xs, st) in enumerate(zip(xshape, x.stride())):
        os_ = oshape[lead + d]
        if xs == os_:
            strides.append(st if xs != 1 else 0)
        elif xs == 1:
            strides.append(0)
        else:
            raise ValueError(f"cast: cannot broadcast {xshape} to {oshape}")
    # drop extent-1 dims, then merge adjacent dims that are contiguous in both (keeps ndim
    # within the kernel's limit)
    dims = [(s, t) for s, t in zip(oshape, strides) if s != 1] or [(1, 0)]
    ms, mt = [dims[0][0]], [dims[0][1]]
    for s, t in dims[1:]:
        if mt[-1] == t * s:
            ms[-1] *= s
            mt[-1] = t
        else:
            ms.append(s)
            mt.append(t)
    if len(ms) > 8:
        raise ValueError(f"cast: {len(ms)} non-mergeable dimensions (kernel limit 8)")
    return ms, mt


def cast(out, x, stream=None):
    """``out[...] = x`` broadcast to ``out.shape`` and widened to ``out.dtype`` (``fa_cast``):
    numpy's implicit operand preparation for a binary ufunc whose operands differ in dtype or
    broadcastable shape. ``out`` is contiguous; ``x`` any strided device tensor. A shape that does
    not broadcast, or more than 8 non-mergeable dimensions, raise ValueError before any launch."""
    lib = _abi.load()
    if out.device != x.device:
        raise ValueError(f"cast: {x.device} -> {out.device}")
    if not out.is_contiguous():
        raise ValueError("cast: out must be contiguous")
    ms, mt = cast_dims(out.shape, x)
    with _on(out.device):
        st = _stream_handle(out, stream)
        rc = lib.fa_cast(out.data_ptr(), fa_dtype(out), x.data_ptr(), fa_dtype(x), len(ms), _abi.int64_array(ms),
                         _abi.int64_array(mt), st)
    _abi.check(rc)
    return out


def _probe_lib():
    """The measurement entry points exist only in libfedagg_probe.so (include/fedagg_probe.h)."""
    lib = _abi.load()
    if lib is not _abi._probe:
        raise RuntimeError("measurement / tuning entry point: call fedn_amd._abi.use_probe() first "
                           "(libfedagg_probe.so; the product libfedagg.so has no knobs)")
    return lib


def stream_copy(dst, src, stream=None):
    lib = _probe_lib()
    st = _stream_handle(src, stream)
    _abi.check(lib.fa_stream_copy(dst.data_ptr(), src.data_ptr(), src.numel() * src.element_size(), st))


def stream_sum(out, bufs, stream=None):
    """Measurement: out = sum of bufs (fp32) with the FedAvg kernel's traversal."""
    lib = _probe_lib()
    st = _stream_handle(out, stream)
    _abi.check(lib.fa_stream_sum(out.data_ptr(), _abi.ptr_array([b.data_ptr() for b in bufs]), len(bufs),
                                 out.numel(), st))


def stream_read(src, sink, stream=None):
    lib = _probe_lib()
    st = _stream_handle(src, stream)
    _abi.check(lib.fa_stream_read(src.data_ptr(), src.numel() * src.element_size(), sink.data_ptr(), st))


def stream_read_sink(src):
    lib = _probe_lib()
    blocks = lib.fa_stream_read_blocks(src.numel() * src.element_size())
    return torch.empty(max(1, blocks) * 16, dtype=torch.uint8, device=src.device)


# tune(strips=...) names: _abi's FA_TUNE_* constants in lower case without the prefix
_KNOBS = {name[len("FA_TUNE_"):].lower(): value for name, value in vars(_abi).items() if name.startswith("FA_TUNE_")}


def tune(**knobs):
    """Set launch knobs (fa_tune): FedAvg strips, unroll, nt, fastdiv, ...; and fastdiv64 (CF64's division). Results never change (every setting is bit-identical)."""
    lib = _probe_lib()
    for k, v in knobs.items():
        _abi.check(lib.fa_tune(_KNOBS[k], int(v)))


_EW = {"axpby": _abi.FA_EW_AXPBY, "mul": _abi.FA_EW_MUL, "div": _abi.FA_EW_DIV, "sqrt": _abi.FA_EW_SQRT,
       "square": _abi.FA_EW_SQUARE, "sign": _abi.FA_EW_SIGN, "fill": _abi.FA_EW_FILL, "pow": _abi.FA_EW_POW,
       "ipow": _abi.FA_EW_IPOW, "ifold": _abi.FA_EW_IFOLD, "nfold": _abi.FA_EW_NFOLD}


def elementwise(op, out, x=None, y=None, a=0.0, b=0.0, stream=None):
    """numpyhelper primitive on device tensors (``fa_elementwise``); see include/fedagg.h."""
    lib = _abi.load()
    P = out.numel()
    _check_dev("out", out, P, None)
    for name, t in (("x", x), ("y", y)):
        if t is not None:
            _check_dev(name, t, P, out.device)
    if P == 0:                      # an empty tensor: nothing to compute (its buffers may be null)
        for t in (out, x, y):
            if t is not None:
                fa_dtype(t)         # the same dtype refusal as a non-empty call
        if op not in _EW:
            raise ValueError(f"unknown elementwise op {op}")
        return out
    with _on(out.device):
        st = _stream_handle(out, stream)
        rc = lib.fa_elementwise(_EW[op], out.data_ptr(), fa_dtype(out), 0 if x is None else x.data_ptr(),
                                fa_dtype(out) if x is None else fa_dtype(x), 0 if y is None else y.data_ptr(),
                                _abi.FA_NONE if y is None else fa_dtype(y), float(a), float(b), P, st)
    _abi.check(rc)
    return out


def norm1(x, matrix, stream=None):
    """np.linalg.norm(x, 1) of one device tensor (``fa_norm1``): a 0-dim f64 device tensor.
    ``matrix``: x is 2-D (max column sum of |x|), else the sum of |x| over all elements."""
    lib = _abi.load()
    if not x.is_contiguous():
        raise ValueError("norm1: x must be contiguous")
    rows, cols = (x.shape[0], x.shape[1]) if matrix else (1, x.numel())
    work = torch.empty(max(1, int(lib.fa_norm1_work(rows, cols, int(matrix)))), dtype=torch.float64, device=x.device)
    out = torch.empty((), dtype=torch.float64, device=x.device)
    with _on(x.device):
        st = _stream_handle(x, stream)
        rc = lib.fa_norm1(out.data_ptr(), x.data_ptr(), fa_dtype(x), rows, cols, int(matrix), work.data_ptr(), st)
    _abi.check(rc)
    return out


# ---- peer transport of the sliced all-gather (include/fedagg.h fa_ipc_* / fa_copy_async) ----------

def ipc_handle(t):
    """(handle bytes, byte offset) exporting device tensor ``t``'s memory to another process."""
    import ctypes
    lib = _abi.load()
    h = ctypes.create_string_buffer(_abi.IPC_HANDLE_BYTES)
    off = ctypes.c_uint64(0)
    with _on(t.device):
        _abi.check(lib.fa_ipc_get_handle(t.data_ptr(), h, ctypes.byref(off)))
    return h.raw, int(off.value)


def ipc_open(handle, offset, device):
    """Map a peer process's buffer on ``device``: (base, device pointer); unmap with ipc_close(base)."""
    import ctypes
    lib = _abi.load()
    if len(handle) != _abi.IPC_HANDLE_BYTES:
        raise ValueError(f"IPC handle must be {_abi.IPC_HANDLE_BYTES} bytes")
    base, ptr = ctypes.c_void_p(), ctypes.c_void_p()
    with _on(device):
        _abi.check(lib.fa_ipc_open(ctypes.create_string_buffer(handle, len(handle)), int(offset), ctypes.byref(base),
                                   ctypes.byref(ptr)))
    return int(base.value or 0), int(ptr.value or 0)


def ipc_close(base, device):
    lib = _abi.load()
    with _on(device):
        _abi.check(lib.fa_ipc_close(base))


def copy_async(dst_ptr, src, nbytes, stream):
    """``nbytes`` of device tensor ``src`` (from its start) to device address ``dst_ptr`` on ``stream``
    (an IPC mapping of a peer's buffer, or another device's tensor): the DMA engines drive the link."""
    lib = _abi.load()
    if nbytes > src.numel() * src.element_size():
        raise ValueError("copy_async: more bytes than the source holds")
    with _on(src.device):
        _abi.check(lib.fa_copy_async(int(dst_ptr), src.data_ptr(), int(nbytes), ctypes_stream(stream)))


def copy_ptr_async(dst_ptr, src_ptr, nbytes, stream, device):
    """``nbytes`` from address ``src_ptr`` to ``dst_ptr`` (host or device) on ``stream``: one
    hipMemcpyAsync, without a tensor per call."""
    with _on(device):
        _abi.check(_abi.load().fa_copy_async(int(dst_ptr), int(src_ptr), int(nbytes), ctypes_stream(stream)))


def fedavg_fold_push(agg_ptr, ptrs, n, N, P, init, dst_ptrs, stream, device, release_rec=None):
    """The fp32 fold of ``P`` elements into device address ``agg_ptr`` whose kernel also stores the
    result to every address in ``dst_ptrs`` (``fa_fedavg_fold_push``: fold and all-gather push in
    one pass); client table and destinations as device addresses, 16-B aligned. ``release_rec``: a
    :func:`release_record` tensor on ``device`` the release grid records its XCDs in (or None).
    Returns whether a release grid was launched (there were destinations and something to fold)."""
    K = len(ptrs)
    if len(n) != K or len(N) != K:
        raise ValueError("n and N must have one entry per update")
    nd = len(dst_ptrs)
    rec = _release_ptr(release_rec, device)
    with _on(device):
        _abi.check(_abi.load().fa_fedavg_fold_push(
            int(agg_ptr), (ctypes.c_void_p * max(1, K))(*ptrs), (ctypes.c_double * max(1, K))(*n),
            (ctypes.c_double * max(1, K))(*N), K, int(P), int(bool(init)),
            (ctypes.c_void_p * max(1, nd))(*[int(p) for p in dst_ptrs]), nd, rec, ctypes_stream(stream)))
    return K > 0 and P > 0 and nd > 0    # a release grid ran after the peer stores


def push(dst_ptrs, src, nbytes, stream, release_rec=None):
    """``nbytes`` of device tensor ``src`` (from its start) to every device address in ``dst_ptrs``
    on ``stream`` with ONE kernel (``fa_push``): the source is read once, each destination written
    over its own link (IPC mappings of peers' buffers, or other devices' buffers in-process).
    Returns whether a release grid was launched (something was stored)."""
    lib = _abi.load()
    if nbytes > src.numel() * src.element_size():
        raise ValueError("push: more bytes than the source holds")
    n = len(dst_ptrs)
    rec = _release_ptr(release_rec, src.device)
    with _on(src.device):
        _abi.check(lib.fa_push((ctypes.c_void_p * max(1, n))(*[int(p) for p in dst_ptrs]), n, src.data_ptr(),
                               int(nbytes), rec, ctypes_stream(stream)))
    return n > 0 and nbytes > 0          # a release grid ran after the stores (fa_push returns before one
    #                                      when there is nothing to store)


def release_record(device):
    """A zeroed release record (include/fedagg.h FA_RELEASE_WORDS uint32 on ``device``) for the
    release grids of :func:`push` / :func:`fedavg_fold_push` on one stream."""
    return torch.zeros(_abi.RELEASE_WORDS, dtype=torch.int32, device=device)


def _release_ptr(rec, device):
    if rec is None:
        return None
    if (rec.dtype != torch.int32 or rec.numel() < _abi.RELEASE_WORDS or not rec.is_contiguous()
            or rec.device != torch.device(device)):
        raise ValueError(f"release record must be {_abi.RELEASE_WORDS} contiguous int32 on {device}")
    return rec.data_ptr()


def read_release_record(rec):
    """The XCD-coverage record of the release grids (synchronises with its device): launches checked,
    launches that missed an XCD, the XCDs seen (mask) and the device's XCD mask."""
    v = [int(x) & 0xFFFFFFFF for x in rec.cpu().tolist()]
    return {"launches": v[_abi.FA_REL_LAUNCHES], "misses": v[_abi.FA_REL_MISSES], "seen_mask": v[_abi.FA_REL_SEEN],
            "expect_mask": v[_abi.FA_REL_EXPECT], "xcds_seen": bin(v[_abi.FA_REL_SEEN]).count("1")}


def device_xccs(device):
    """XCDs (each with its own L2) of ``device``."""
    out = ctypes.c_int(0)
    idx = torch.device(device).index or 0
    _abi.check(_abi.load().fa_device_xccs(int(idx), ctypes.byref(out)))
    return int(out.value)


_NULL_CTX = contextlib.nullcontext()


def _on(device):
    """``torch.cuda.device(device)`` unless it is already the current device (the per-round and
    per-update copy calls of the pipelines pay the context switch only when they need it)."""
    if device is None:
        return _NULL_CTX
    idx = device.index if isinstance(device, torch.device) else torch.device(device).index
    if idx is None or idx == torch.cuda.current_device():
        return _NULL_CTX
    return torch.cuda.device(device)


def peer_enable(dev, peer):
    """Direct access of device ``dev`` to device ``peer``'s memory (in-process multi-GPU)."""
    _abi.check(_abi.load().fa_peer_enable(int(dev), int(peer)))


def last_kernel():
    """The kernel family the calling thread's last fold / FedOpt launch ran (fa_last_kernel)."""
    v = _abi.load().fa_last_kernel()
    return v.decode() if v else ""


def host_device_ptr(host_ptr, device):
    """Device address of page-locked host memory at ``host_ptr`` (raises for pageable memory)."""
    out = ctypes.c_void_p()
    with _on(device):
        _abi.check(_abi.load().fa_host_device_ptr(int(host_ptr), ctypes.byref(out)))
    return int(out.value or 0)


def fedavg_fold_raw(out_ptr, out_dtype, P, ptrs, upd_dtype, n, N, init, stream, device):
    """:func:`fedavg_fold_ptrs` into ``P`` elements of ``out_dtype`` at device address ``out_ptr``
    (e.g. pinned host memory's device address: the model lands on the host with no D2H copy)."""
    K = len(ptrs)
    if len(n) != K or len(N) != K:
        raise ValueError("n and N must have one entry per update")
    with _on(device):
        _abi.check(_abi.load().fa_fedavg_fold(int(out_ptr), fa_dtype(out_dtype), (ctypes.c_void_p * max(1, K))(*ptrs),
                                              fa_dtype(upd_dtype), (ctypes.c_double * max(1, K))(*n),
                                              (ctypes.c_double * max(1, K))(*N), K, int(P), int(bool(init)),
                                              ctypes_stream(stream)))


def fedavg_fold_host(call, n, N):
    """A small round's whole fold (smallround.py): ``call(n, N)`` runs the native pack wait +
    ``fa_fedavg_fold_host`` + stream wait (``_fastpack.fold_host``) with the client table's ``n`` /
    ``N`` and returns its status; FedAggError on a failed one (the C-ABI wrapper level, as every
    fold op here), CodecError if the pack it waited for failed."""
    if len(n) != len(N):
        raise ValueError("n and N must have one entry per update")
    rc = call(n, N)
    if rc == -1:
        from . import codec
        raise codec.CodecError(f"fnpz_gather_wait: {codec.load_lib().fnpz_last_error().decode(errors='replace')}")
    _abi.check(rc)


def fedopt_step_host(call, n, N, *, first=True, final=True):
    """A small FedOpt round's whole step (smallround.SmallFedOptRound): ``call(n, N)`` runs the native
    pack wait + ``fa_fedopt_step_host`` (FIRST | FINAL) + stream wait with the client table's ``n`` /
    ``N``; FedAggError on a failed one (the state untouched: the step writes the buffers the state
    does not hold), CodecError if a pack failed."""
    if len(n) != len(N):
        raise ValueError("n and N must have one entry per update")
    if not (first and final):
        raise ValueError("fedopt_step_host: the one-call round is a FIRST | FINAL step")
    rc = call(n, N)
    if rc == -1:
        from . import codec
        raise codec.CodecError(f"fnpz_gather_wait: {codec.load_lib().fnpz_last_error().decode(errors='replace')}")
    _abi.check(rc)


def host_register(t):
    """Page-lock the memory of host tensor ``t`` (mapped by the caller, e.g. shared memory)."""
    _abi.check(_abi.load().fa_host_register(t.data_ptr(), t.numel() * t.element_size()))


def host_unregister(t):
    _abi.check(_abi.load().fa_host_unregister(t.data_ptr()))


def host_register_ptr(ptr, nbytes):
    """Page-lock ``nbytes`` of host memory at ``ptr`` in place (e.g. a decoded update's numpy array),
    so DMA reads it directly; undo with :func:`host_unregister_ptr` before the memory is freed."""
    _abi.check(_abi.load().fa_host_register(int(ptr), int(nbytes)))


def host_unregister_ptr(ptr):
    _abi.check(_abi.load().fa_host_unregister(int(ptr)))


_FUSED_OPT = {(torch.float32, torch.float32), (torch.bfloat16, torch.float32), (torch.float32, torch.float64),
              (torch.float64, torch.float64), (torch.bfloat16, torch.float64), (torch.float64, torch.float32),
              (torch.int64, torch.int64), (torch.int64, torch.float64), (torch.int64, torch.float32),
              (torch.int32, torch.int32), (torch.int32, torch.float64), (torch.int32, torch.float32),
              # float16 sessions: a half global model's pseudo-gradient is half (numpy's half loops)
              (torch.float16, torch.float16), (torch.float16, torch.float32), (torch.float16, torch.float64),
              (torch.float32, torch.float16), (torch.float64, torch.float16)}


def fused_fedopt_pair(upd, old):
    """Whether fa_fedopt_step instantiates (update dtype, global-model dtype)."""
    return (upd, old) in _FUSED_OPT


def check_fedopt_dtypes(layout):
    for dt in layout.groups:
        if torch_dtype(dt) not in (torch.float16, torch.float32, torch.float64, torch.int32, torch.int64):
            raise TypeError(f"FedOpt supports float16/float32/float64/int32/int64 updates, got {dt}")
