"""Oracle of the fused centred-clipping pass (``fa_centered_clip_step``) and of the rule as DESIGN.md
§3.10 defines them, numpy and plain Python only.

Step. With C the compute type of the updates' dtype (krum_ref.compute_dtype), O the output type
(robust_ref.out_dtype; bfloat16 data comes as the float32 values it holds exactly and gives float32),
``v`` the centre in O and ``c_k = C(coef[k])``, per element ``acc = C(v)``, then over the clients with
``c_k != 0`` in index order ``acc = acc + c_k * (C(u_k) - C(v))``: the difference, the product and the add
each rounded once in C; ``v' = O(acc)``. A client with ``c_k = 0`` is no part of the sum; every ``c_k = 0``
gives ``O(C(v))``.

Distances. geomed_ref's: ``d[k] = sum_p (C(u_k[p]) - C(v'[p]))**2`` for every k. The kernel's values must
lie within krum_ref.rtol of them.

Coefficients. ``r = sqrt(d_k)``; ``lambda_k = 1`` where ``r <= tau`` else ``tau / r``, 0 where ``d_k`` is not
finite or negative; ``coef_k = lambda_k / K_good``, in float64.
"""
import math

import numpy as np

import geomed_ref as gr
import krum_ref as kr
import robust_ref as rr

dists = gr.dists
dists_prefixes = gr.dists_prefixes


def step(S, v, coef):
    """The new point from the rows of ``S`` (K, P), the centre ``v`` (P,) in O and K coefficients."""
    S, v = np.asarray(S), np.asarray(v)
    C = kr.compute_dtype(S.dtype)
    O = rr.out_dtype(S.dtype)
    assert v.dtype == O, (v.dtype, O)
    with np.errstate(all="ignore"):
        vc = v.astype(C)
        acc = vc.copy()
        for k in range(S.shape[0]):
            c = C.type(coef[k])
            if c == 0:
                continue
            delta = S[k].astype(C) - vc
            acc = acc + c * delta
        return np.asarray(acc, dtype=C).astype(O)


def coefficients(d, tau):
    """Plain-Python clipping coefficients."""
    tau = float(tau)
    lam, good = [], 0
    for v in d:
        v = float(v)
        if not math.isfinite(v) or v < 0.0:
            lam.append(0.0)
            continue
        r = math.sqrt(v)
        lam.append(1.0 if r <= tau else tau / r)
        good += 1
    if good == 0:
        raise ValueError("no client has a finite distance")
    return [v / float(good) for v in lam]


def _rows(updates, i):
    return np.stack([np.asarray(u[i]).reshape(-1) for u in updates])


def model_center(updates, center):
    """The centre's tensors converted to each tensor's output type."""
    return [np.asarray(c).astype(rr.out_dtype(np.asarray(updates[0][i]).dtype)) for i, c in enumerate(center)]


def model_step(updates, center, coef):
    """A round: ``updates`` = list of models (lists of arrays of one layout), ``center`` one model in the
    output types; the new point per tensor."""
    return [step(_rows(updates, i), np.asarray(center[i]).reshape(-1), coef).reshape(np.asarray(center[i]).shape)
            for i in range(len(center))]


def model_dists(updates, point):
    """The K squared distances of a round's updates to the model ``point`` (output types): each tensor's in
    its own compute type, summed in float64."""
    d = np.zeros(len(updates), dtype=np.float64)
    with np.errstate(all="ignore"):
        for i in range(len(point)):
            S = _rows(updates, i)
            if S.shape[1]:
                d = d + dists(S, np.asarray(point[i]).reshape(-1))
    return d


def cclip_f64(updates, center, iterations, tau):
    """A float64 run of the rule on the CPU: ``[(coef_t, d_t)]`` for t = 0 .. iterations and the final point
    as one flat float64 vector."""
    X = np.stack([np.concatenate([np.asarray(a, dtype=np.float64).reshape(-1) for a in u]) for u in updates])
    v = np.concatenate([np.asarray(a, dtype=np.float64).reshape(-1) for a in center])
    K = X.shape[0]
    trace = []
    with np.errstate(all="ignore"):
        coef = np.zeros(K)
        for t in range(iterations + 1):
            if t:
                coef = np.array(coefficients(trace[-1][1], tau))
                live = coef != 0
                v = v + (coef[live, None] * (X[live] - v)).sum(axis=0)
            d = ((X - v) ** 2).sum(axis=1)
            trace.append((coef, d))
    return trace, v
