"""Oracle of the robust rules (coordinate-wise trimmed mean / median), numpy only.

Per element, the K values are put in the total order "by value, -0 before +0, every NaN (either
sign, any payload) after +inf, all NaNs equal" by sorting unsigned integer keys; of the ascending
sequence s the values s[t] .. s[K-t-1] are kept and summed in that order in the accumulator type A,
STARTING from s[t] (so a kept run of -0 gives -0), each add rounded once; the sum is divided by
A(K - 2t) and rounded once to the output type.

    dtype     A        output
    float32   float32  float32
    float64   float64  float64
    float16   float32  float16
    int32/64  float64  float64   (each kept value converted with one rounding)

numpy's own ``np.sort(S, 0)[t:K-t].mean(0)`` / ``np.median(S, 0)`` equal this bit for bit wherever
they are defined (tests/test_robust_host.py); they leave the order of -0 / +0 ties to the sort
algorithm, which is why the oracle sorts keys.
"""
import numpy as np

_UINT = {2: np.uint16, 4: np.uint32, 8: np.uint64}


def acc_dtype(dt):
    dt = np.dtype(dt)
    if dt.kind == "i":
        return np.dtype(np.float64)
    return np.dtype(np.float32) if dt == np.float16 else dt


def out_dtype(dt):
    dt = np.dtype(dt)
    return np.dtype(np.float64) if dt.kind == "i" else dt


def median_trim(K):
    return (K - 1) // 2


def sorted_values(S):
    """``S`` (K, ...) of one dtype, sorted along axis 0 in the rule's total order (NaNs canonical)."""
    S = np.ascontiguousarray(S)
    dt = S.dtype
    U = _UINT[dt.itemsize]
    bits = 8 * dt.itemsize
    sign = U(1 << (bits - 1))
    ones = U((1 << bits) - 1)
    u = S.view(U)
    if dt.kind == "i":
        key = np.sort(u ^ sign, axis=0)
        return (key ^ sign).view(dt)
    if dt.kind != "f":
        raise TypeError(f"no robust rule for dtype {dt}")
    key = np.where((u & sign) != 0, u ^ ones, u ^ sign)
    key = np.where(np.isnan(S), U(ones - U(1)), key).astype(U)    # every NaN: one key after +inf
    key = np.sort(key, axis=0)
    back = np.where((key & sign) != 0, key ^ sign, key ^ ones).astype(U)
    return back.view(dt)                                          # max - 1 maps back to a NaN


def trimmed_mean(S, t):
    """Trimmed mean along axis 0 of ``S`` (K, ...) dropping ``t`` values at each end."""
    S = np.asarray(S)
    K = S.shape[0]
    if t < 0 or K - 2 * t < 1:
        raise ValueError(f"trim={t} leaves nothing of K={K}")
    return mean_of_sorted(sorted_values(S), t)


def mean_of_sorted(s, t):
    """The rule's arithmetic on ``s`` = :func:`sorted_values` of the updates (sorted once, any ``t``)."""
    K = s.shape[0]
    A = acc_dtype(s.dtype)
    with np.errstate(all="ignore"):
        acc = s[t].astype(A)
        for j in range(t + 1, K - t):
            acc = acc + s[j].astype(A)
        r = acc / A.type(K - 2 * t)
        return np.asarray(r, dtype=A).astype(out_dtype(s.dtype))


def median(S):
    S = np.asarray(S)
    return trimmed_mean(S, median_trim(S.shape[0]))


def combine(updates, t):
    """A round: ``updates`` = list of models (lists of arrays of one layout); the model per tensor."""
    return [trimmed_mean(np.stack([np.asarray(u[i]) for u in updates]), t) for i in range(len(updates[0]))]
