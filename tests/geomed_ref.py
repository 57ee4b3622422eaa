"""Oracle of the fused Weiszfeld pass (``fa_weighted_mean_sqdist``) and of the geometric-median rule as
DESIGN.md §3.9 defines them, numpy and plain Python only.

Weighted mean. With C the compute type of the updates' dtype (krum_ref.compute_dtype) and
``b_k = C(beta[k])``, per element over the clients with ``b_k != 0`` in index order: ``acc = b * C(u)`` for
the first, ``acc = acc + b * C(u)`` for the others, every product and add rounded once in C; the result
is rounded once to the output type (robust_ref.out_dtype; bfloat16 data comes as the float32 values it
holds exactly and gives float32). A client with ``b_k = 0`` is no part of the sum.

Distances. ``d[k] = sum_p (C(u_k[p]) - C(z[p]))**2`` for every k: krum_ref.sqdist's arithmetic on the rows
``[z, u_0, ...]`` converted to C, row 0. The kernel's values must lie within krum_ref.rtol of them.

Weights. ``w_k = 1 / max(nu, sqrt(d_k))`` where d_k is finite, else 0, summed in index order, in float64.
"""
import math

import numpy as np

import krum_ref as kr
import robust_ref as rr


def wmean(S, beta):
    """The weighted mean of the rows of ``S`` (K, P) by the definition above."""
    S = np.asarray(S)
    C = kr.compute_dtype(S.dtype)
    acc = None
    with np.errstate(all="ignore"):
        for k in range(S.shape[0]):
            b = C.type(beta[k])
            if b == 0:
                continue
            p = b * S[k].astype(C)
            acc = p if acc is None else acc + p
        if acc is None:
            raise ValueError("every weight is zero")
        return np.asarray(acc, dtype=C).astype(rr.out_dtype(S.dtype))


def dists_prefixes(S, z, Ps):
    """``{P: d of S[:, :P] to z[:P]}`` as float64 arrays of K, one pass over the longest prefix."""
    S, z = np.asarray(S), np.asarray(z)
    Ps = sorted(set(int(P) for P in Ps))
    C = kr.compute_dtype(S.dtype)
    wide = np.float64 if C == np.float32 else np.longdouble
    out = {}
    with np.errstate(all="ignore"):
        d = S[:, :Ps[-1]].astype(C).astype(wide) - z[:Ps[-1]].astype(C).astype(wide)
        d *= d
        lo, run = 0, np.zeros(S.shape[0], dtype=wide)
        for P in Ps:
            run = run + d[:, lo:P].sum(axis=1, dtype=wide)
            out[P] = run.astype(np.float64)
            lo = P
    return out


def dists(S, z):
    S = np.asarray(S)
    return dists_prefixes(S, z, [S.shape[1]])[S.shape[1]]


def weights(d, nu):
    """Plain-Python Weiszfeld weights."""
    w = []
    for v in d:
        v = float(v)
        w.append(1.0 / max(float(nu), math.sqrt(v)) if math.isfinite(v) else 0.0)
    total = 0.0
    for v in w:
        total = total + v
    if total == 0.0:
        raise ValueError("every weight is zero")
    return [v / total for v in w]


def model_wmean(updates, beta):
    """A round: ``updates`` = list of models (lists of arrays of one layout); the weighted mean per tensor."""
    return [wmean(np.stack([np.asarray(u[i]).reshape(-1) for u in updates]), beta).reshape(np.asarray(updates[0][i]).shape)
            for i in range(len(updates[0]))]


def model_dists(updates, beta):
    """The K squared distances of a round's updates to ``model_wmean(updates, beta)``: each tensor's in its
    own compute type, summed in float64."""
    K = len(updates)
    d = np.zeros(K, dtype=np.float64)
    with np.errstate(all="ignore"):
        for i in range(len(updates[0])):
            S = np.stack([np.asarray(u[i]).reshape(-1) for u in updates])
            if S.shape[1]:
                d = d + dists(S, wmean(S, beta))
    return d


def weiszfeld_f64(updates, iterations, nu, excluded=()):
    """A float64 run of the rule on the CPU: ``[(beta_t, d_t)]`` for t = 0 .. iterations and the final
    point as one flat float64 vector. ``excluded`` clients have weight 0 throughout."""
    X = np.stack([np.concatenate([np.asarray(a, dtype=np.float64).reshape(-1) for a in u]) for u in updates])
    K = X.shape[0]
    good = [k for k in range(K) if k not in set(excluded)]
    beta = np.zeros(K)
    beta[good] = 1.0 / len(good)
    trace = []
    with np.errstate(all="ignore"):
        for t in range(iterations + 1):
            if t:
                beta = np.array(weights(trace[-1][1], nu))
            z = (beta[good, None] * X[good]).sum(axis=0)
            d = ((X - z) ** 2).sum(axis=1)
            trace.append((beta, d))
    return trace, z
