"""Oracle of Krum / Multi-Krum (Blanchard et al., 2017) as DESIGN.md §3.8 defines it, numpy and plain
Python only.

Distances. With C the compute type of the updates' dtype (float32 for float32 / float16 / bfloat16, each
value widened exactly; float64 for float64 / int32 / int64, each value converted with one rounding),
``D[i][j] = sum_p (C(u_i[p]) - C(u_j[p]))**2``, ``D[i][i] = 0``. :func:`sqdist` evaluates that sum on the
converted values far more precisely than the kernel may (float64 for the float32 family, longdouble for
the float64 family); the kernel's entries must lie within ``rtol`` of it, relatively:
``(R + 4) * 2**-24`` for C = float32 (chains of at most R terms), ``(P + 4) * 2**-53`` for C = float64.

Selection, on the host in float64. Non-finite entries of D count as +inf;
``nn = max(K - f - 2, min(1, K - 1))``; a client's score is the sum of its ``nn`` smallest distances to
the OTHER clients, sorted ascending and summed in that order; the ``m`` clients with the smallest scores
are selected, ties to the lower index; fewer than ``m`` finite scores is an error.
``f = min(floor(fraction * K), (K - 3) // 2)`` for K >= 3, else 0. Multi-Krum: m = K - f; Krum: m = 1.

Model: the unweighted mean of the selected updates by the §3.7 rule at trim 0 (robust_ref.combine).
"""
import math

import numpy as np

import robust_ref as rr


def compute_dtype(dt):
    dt = np.dtype(dt)
    return np.dtype(np.float32) if dt in (np.dtype(np.float32), np.dtype(np.float16)) else np.dtype(np.float64)


def rtol(dt, P, R):
    return (R + 4) * 2.0 ** -24 if compute_dtype(dt) == np.float32 else (P + 4) * 2.0 ** -53


def sqdist_prefixes(S, Ps):
    """``{P: D of S[:, :P]}`` for every P in ``Ps``, as float64: one pass over the longest prefix
    (bfloat16 data comes as the float32 values it holds exactly). Non-finite inputs give inf / NaN in
    their client's row and column."""
    S = np.asarray(S)
    K = S.shape[0]
    Ps = sorted(set(int(P) for P in Ps))
    C = compute_dtype(S.dtype)
    wide = np.float64 if C == np.float32 else np.longdouble
    X = S[:, :Ps[-1]].astype(C).astype(wide)         # the conversion the kernel makes, then exact widening
    out = {P: np.zeros((K, K), dtype=np.float64) for P in Ps}
    with np.errstate(all="ignore"):
        for i in range(K - 1):
            d = X[i + 1:] - X[i]
            d *= d
            lo, run = 0, np.zeros(K - 1 - i, dtype=wide)
            for P in Ps:                             # the prefixes' sums, each continuing the one before
                run = run + d[:, lo:P].sum(axis=1, dtype=wide)
                out[P][i, i + 1:] = out[P][i + 1:, i] = run.astype(np.float64)
                lo = P
    return out


def sqdist(S):
    """K x K reference distances of ``S`` (K, P) as float64."""
    S = np.asarray(S)
    return sqdist_prefixes(S, [S.shape[1]])[S.shape[1]]


def byzantine_count(fraction, K):
    if K < 3:
        return 0
    return min(math.floor(fraction * K), (K - 3) // 2)


def scores(D, f):
    """Brute force, on Python floats."""
    K = len(D)
    nn = max(K - f - 2, min(1, K - 1))
    out = []
    for i in range(K):
        others = []
        for j in range(K):
            if j != i:
                v = float(D[i][j])
                others.append(v if math.isfinite(v) else math.inf)
        others.sort()
        total = 0.0
        for v in others[:nn]:
            total = total + v
        out.append(total)
    return out


def select(D, f, m):
    """The m selected FIFO indices, ascending; ``ValueError`` if fewer than m scores are finite."""
    sc = scores(D, f)
    if sum(1 for v in sc if math.isfinite(v)) < m:
        raise ValueError("too few finite scores")
    left = list(range(len(sc)))
    picked = []
    for _ in range(m):                               # the smallest remaining score, the lowest index first
        best = left[0]
        for i in left[1:]:
            if sc[i] < sc[best]:
                best = i
        picked.append(best)
        left.remove(best)
    return sorted(picked)


def model_distances(updates):
    """D of a round: ``updates`` = list of models (lists of arrays of one layout); each tensor's
    distances in its own compute type, summed in float64 (as the pipeline sums the dtype groups)."""
    K = len(updates)
    D = np.zeros((K, K), dtype=np.float64)
    with np.errstate(all="ignore"):
        for t in range(len(updates[0])):
            S = np.stack([np.asarray(u[t]).reshape(-1) for u in updates])
            if S.shape[1]:
                D = D + sqdist(S)
    return D


def combine(updates, selected):
    return rr.combine([updates[i] for i in selected], 0)
