"""Oracle of Bulyan (El Mhamdi, Guerraoui and Rouault, 2018) as DESIGN.md §3.11 defines it, numpy and plain
Python only.

Byzantine count. ``f = min(floor(fraction * K), (K - 3) // 4)`` for K >= 3, else 0; ``theta = K - 2f``
updates are selected and ``beta = theta - 2f`` values kept per coordinate.

Selection, on the host in float64 from the K x K squared distances D: ``theta`` times, the Krum scores
(krum_ref.scores, with its ``nn`` on the remaining count) of the remaining clients' sub-matrix are taken,
the client with the smallest one is picked (ties to the lower index; a non-finite smallest score is an
error) and removed.

Per coordinate over the selected updates, with A the accumulator type of robust_ref:
  1. sort in robust_ref's total order: s[0 .. theta-1];
  2. med in A: A(s[(theta-1)/2]) for an odd theta, (A(s[theta/2-1]) + A(s[theta/2])) / A(2) for an even one;
  3. a = 0; while a < theta - beta and (A(s[a+beta]) - med) < (med - A(s[a])): a += 1  (each difference
     rounded once in A; strict; false on a NaN);
  4. out = (((A(s[a]) + A(s[a+1])) + ...) + A(s[a+beta-1])) / A(beta), rounded once to the output type.
"""
import math

import numpy as np

import krum_ref as kr
import robust_ref as rr


def byzantine_count(fraction, K):
    if K < 3:
        return 0
    return min(math.floor(fraction * K), (K - 3) // 4)


def median_acc(s):
    """Step 2 on ``s`` = rr.sorted_values (theta, ...): the median in A."""
    theta = s.shape[0]
    A = rr.acc_dtype(s.dtype)
    with np.errstate(all="ignore"):
        if theta % 2:
            return s[(theta - 1) // 2].astype(A)
        return np.asarray((s[theta // 2 - 1].astype(A) + s[theta // 2].astype(A)) / A.type(2), dtype=A)


def _moves(s, med, j, keep):
    """Step 3's predicate at window start j, per column."""
    A = rr.acc_dtype(s.dtype)
    with np.errstate(all="ignore"):
        return np.asarray(s[j + keep].astype(A) - med, dtype=A) < np.asarray(med - s[j].astype(A), dtype=A)


def window_start(s, keep):
    """Step 3, the greedy walk, column by column: int array of the shape of ``s[0]``."""
    theta = s.shape[0]
    med = median_acc(s)
    a = np.zeros(s.shape[1:], dtype=np.int64)
    walking = np.ones(s.shape[1:], dtype=bool)
    for j in range(theta - keep):
        walking = walking & _moves(s, med, j, keep)          # a column stops at its first false
        a = a + walking
    return a


def window_start_count(s, keep):
    """The counting form: the number of j in [0, theta - keep) for which the predicate holds."""
    theta = s.shape[0]
    med = median_acc(s)
    a = np.zeros(s.shape[1:], dtype=np.int64)
    for j in range(theta - keep):
        a = a + _moves(s, med, j, keep)
    return a


def window_mean_of_sorted(s, keep, a=None):
    theta = s.shape[0]
    if not 1 <= keep <= theta:
        raise ValueError(f"keep={keep} of {theta} values")
    A = rr.acc_dtype(s.dtype)
    a = window_start(s, keep) if a is None else a
    flat = s.reshape(theta, -1)
    idx = a.reshape(1, -1)
    with np.errstate(all="ignore"):
        acc = np.take_along_axis(flat, idx, axis=0)[0].astype(A)
        for j in range(1, keep):
            acc = acc + np.take_along_axis(flat, idx + j, axis=0)[0].astype(A)
        r = acc / A.type(keep)
        return np.asarray(r, dtype=A).astype(rr.out_dtype(s.dtype)).reshape(s.shape[1:])


def window_mean(S, keep):
    """The mean of the ``keep`` values closest to the median along axis 0 of ``S`` (theta, ...)."""
    return window_mean_of_sorted(rr.sorted_values(np.asarray(S)), keep)


def select(D, f):
    """``(selected ascending, pick order, pick scores)``, brute force on Python floats; ``ValueError`` when
    a pick's score is not finite."""
    K = len(D)
    theta = K - 2 * f
    left = list(range(K))
    order, scores = [], []
    for _ in range(theta):
        sub = [[D[i][j] for j in left] for i in left]
        sc = kr.scores(sub, f)
        best = 0
        for i in range(1, len(left)):
            if sc[i] < sc[best]:
                best = i
        if not math.isfinite(sc[best]):
            raise ValueError("no finite score left")
        order.append(left.pop(best))
        scores.append(sc[best])
    return sorted(order), order, scores


def combine(updates, f):
    """A round: ``updates`` = list of models (lists of arrays of one layout); ``(model per tensor,
    selected)`` with distances from krum_ref.model_distances."""
    selected, _, _ = select(kr.model_distances(updates).tolist(), f)
    keep = len(selected) - 2 * f
    model = [window_mean(np.stack([np.asarray(updates[k][i]) for k in selected]), keep)
             for i in range(len(updates[0]))]
    return model, selected
