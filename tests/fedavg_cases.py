"""Shared builders for the FedAvg fold tests (tests/test_fedavg_cases_host.py on the oracle alone,
tests/test_gpu_fedavg_kernels.py on the device): the seven (update, aggregate) dtype pairs of
``fa_fedavg_fold``, the numpy reference of a fold that starts from the first update or continues a stored
aggregate, the clients' num_examples per pair, and the special-value columns. Plain numpy; nothing here
touches a GPU. The scalar helpers are tests/fedopt_cases.py's.

A bf16 update is an f32 array whose low 16 bits are zero, and its reference is the f32 computation on
those exact values (test_fedavg_bf16_defined_as_fp32_on_upcast).
"""
import math
from collections import namedtuple

import numpy as np

from fedopt_cases import (MAXV, NAN_BITS, NP_DT, SUBV, cast, client_ns, is_int, near_midpoints,  # noqa: F401
                          tie_numerators, tile, to_bf16, totals)
from oracle import numpy_ref as ref

# (update, aggregate), in the order of fa_fedavg_fold's dispatch
PAIRS = [("f32", "f32"), ("bf16", "f32"), ("f16", "f16"), ("f64", "f64"), ("f32", "f64"), ("i64", "f64"), ("i32", "f64")]
_SIZE = {"f16": 2, "bf16": 2, "f32": 4, "f64": 8, "i32": 4, "i64": 8}
# elements per 16-byte strip of the update (launch_fedavg's E16)
E_OF = {p: 16 // _SIZE[p[0]] for p in PAIRS}
DTYPES = ["f32", "f64", "bf16", "f16", "i32", "i64"]
# every pair of the library's fold dtypes outside the dispatch (29, among them (f64, f32), (f16, f32), (i64, i64))
REFUSED = [(u, a) for u in DTYPES for a in DTYPES if (u, a) not in PAIRS]
# K = 1 with init is a copy: these pairs have no such copy
NO_COPY = [p for p in PAIRS if p[0] != p[1]]


def kinds(pair):
    """The ns lists a pair takes: integer updates fold their first step in the integer dtype for an int
    num_examples only (a fractional n[1] is refused: tests/test_gpu_ifold.py)."""
    return ("plain", "big") if is_int(pair[0]) else ("plain", "float", "big")


def ns_for(pair, K, kind="plain"):
    """num_examples per client (python numbers): fedopt_cases.client_ns, and on top of it
    f16 "float": n = 1000, 1, 2049 + 2^-20 (one rounding from double gives the half 2050, a rounding
                 through float 2048), 2048, 2049 (the half 2048); the total at client 3 is 5098 + 2^-20 (the
                 half 5100; through float the tie 5098 -> 5096);
    f16 "big":   n = 2048, 1 (the total 2049: the half 2048), 63470 (the total 65519: the half 65504),
                 65519 (finite; the totals are inf from here on), 65520 (inf);
    f64 aggregates "float": n[4] = 2.0**61 (the totals from there on are outside [2^-60, 2^60]: fill_table
                 hands CF64 r = 0);
    integer updates "big": n[1] = 1 000 003 (the first step's product wraps), n[2] makes the total
                 2^53 + 3 (not a double)."""
    u, a = pair
    assert kind in kinds(pair)
    ns = client_ns(K, kind)
    head = {}
    if u == "f16" and kind == "float":
        head = {0: 1000, 1: 1, 2: 2049 + 2.0 ** -20, 3: 2048, 4: 2049}
    elif u == "f16" and kind == "big":
        head = {0: 2048, 1: 1, 2: 63470, 3: 65519, 4: 65520}
    elif a == "f64" and not is_int(u) and kind == "float":
        head = {4: 2.0 ** 61}
    elif is_int(u) and kind == "big":
        head = {1: 1_000_003, 2: 2 ** 53 + 3 - (ns[0] + 1_000_003)}
    for i, v in head.items():
        if i < K:
            ns[i] = v
    assert all(type(n) in (int, float) for n in ns)
    return ns


def start(pair, y0):
    """The model a fold with init starts from (fedavg.py:65-66 aliases the first update):
    same-dtype pairs and bf16 (an f32 array already): the update itself; (f32, f64): the update widened
    exactly (strip_start's ``widen``; tests/test_gpu_parity.py::test_fedavg_f32_updates_into_f64_aggregate
    defines it so); integer pairs: the integer array, so that numpy performs the wrapping first step."""
    u, a = pair
    assert y0.dtype == NP_DT[u]
    if u == "bf16":
        assert not (y0.view(np.uint32) & 0xFFFF).any()
    if pair == ("f32", "f64"):
        return y0.astype(np.float64)
    assert is_int(u) or NP_DT[u] == NP_DT[a]
    return y0


def reference(pair, agg0, ups, ns, Ns):
    """The fold of ``ups`` with the oracle's increment_average, one client at a time: into ``agg0`` (a
    continuation), or with ``agg0 is None`` (init) starting from ``start(pair, ups[0])``. ``ns`` / ``Ns``:
    one entry per update (the first client's are unused with init)."""
    assert len(ups) == len(ns) == len(Ns) and len(ups) >= 1
    with np.errstate(all="ignore"):
        if agg0 is None:
            model, k0 = start(pair, ups[0]), 1
        else:
            assert agg0.dtype == NP_DT[pair[1]]
            model, k0 = agg0, 0
        for k in range(k0, len(ups)):
            assert ups[k].dtype == NP_DT[pair[0]]
            model = ref.increment_average([model], [ups[k]], ns[k], Ns[k])[0]
    assert model.dtype == NP_DT[pair[1]], f"{pair}: the oracle gives {model.dtype}"
    return model


Step = namedtuple("Step", "x d t N q")


def fold_trace(pair, ups, ns):
    """The init fold's intermediates per client k >= 1: Step(x = the model before the step, d = y - x,
    t = n*d, N, q = t/N), each step checked against increment_average; and the final model."""
    out, Ns = [None], totals(ns)
    with np.errstate(all="ignore"):
        x = start(pair, ups[0])
        for k in range(1, len(ups)):
            d = np.subtract(ups[k], x)
            t = np.multiply(ns[k], d)
            q = np.true_divide(t, Ns[k])
            new = np.add(x, q)
            want = ref.increment_average([x], [ups[k]], ns[k], Ns[k])[0]
            assert new.dtype == want.dtype and new.tobytes() == want.tobytes()
            out.append(Step(x, d, t, Ns[k], q))
            x = new
    return out, x


Cols = namedtuple("Cols", "ups ns Ns names")


def special_columns(pair, K, ns_kind="plain", seed=23):
    """One scenario per column: ``ups`` (K rows of the update dtype), the clients' ``ns`` and running
    totals ``Ns``, and the columns' names. Client order is permuted per column except in the columns
    named ``fixed:*``, which are written for the first fold step (client 0 is the model, n[1] = 1 outside
    the integer "big" list, so t = y1 - y0 there).

    Every float pair: ordinary values; x and y of +-0 in the four sign combinations; y == x; inf, -inf and
    NaN (with payloads, both signs) in one client and in all; inf - inf; the largest finite value and the
    smallest subnormal; n*t overflowing.
    f32 aggregates: t on, just above and just below 2^-98, a sweep of tiny t with subnormal quotients, and
    the ties of t/N between f32 subnormals the reciprocal rounds the other way (N1 = 98: "big").
    f64 aggregates: signed-zero t; with f64 updates |t| around 2^-600 and above 2^600, and quotients next
    to a rounding midpoint (narrower updates cannot make such a t at the first step).
    f16: n*t overflowing in half, t/N subnormal in half and vanishing.
    Integer pairs: 0, -1, min, max; y1 - y0 that wraps; n1*(y1 - y0) that wraps ("big"); int64 beyond
    2^53 in y0 and in later clients; 16 777 217-like values."""
    u, a = pair
    rng = np.random.default_rng(seed + 7 * K + 3 * PAIRS.index(pair))
    ns = ns_for(pair, K, ns_kind)
    Ns = totals(ns)
    inf, nan = math.inf, math.nan
    nnan = math.copysign(math.nan, -1.0)
    cols = []

    def add(name, ys):
        ys = list(ys) if isinstance(ys, (list, tuple)) else [ys] * K
        assert len(ys) == K, name
        cols.append((name, ys))

    def first(y0, y1, rest):
        """y0, y1, then ``rest`` (a value, or a function of k) for clients 2..K-1."""
        return [y0, y1][:K] + [rest(k) if callable(rest) else rest for k in range(2, K)]

    N1 = Ns[1]
    if not is_int(u):
        grid = [1.0 + 2.0 ** -6 * ((k % 5) - 2) for k in range(K)]
        add("ordinary", grid)
        for _ in range(7):
            add("ordinary", [float(v) for v in 1.0 + 0.1 * rng.standard_normal(K)])
        for x in (0.0, -0.0):
            for y in (0.0, -0.0):
                add("fixed:zero", first(x, y, y))
                add("fixed:zero", first(x, y, lambda k: -0.0 if k % 2 else 0.0))
        add("zero", [-0.0 if k % 2 else 0.0 for k in range(K)])
        for y in (1.5, -3.0, 0.0, -0.0):
            add("const", y)
        for s in (inf, -inf, nan, nnan):
            add("one-special", [s] + grid[1:])
            add("all-special", s)
        for h in sorted({1, K // 2}):
            add("inf-inf", [inf] * h + [-inf] * (K - h))
        for y in (MAXV[u], -MAXV[u], SUBV[u], -SUBV[u]):
            add("extreme", y)
        ext = [MAXV[u], -MAXV[u], SUBV[u], 0.0, -SUBV[u]]
        add("extreme", [ext[k % 5] for k in range(K)])
        add("overflow", [MAXV[u] * (-1) ** k for k in range(K)])                  # y - x overflows
        add("overflow", [MAXV[u] / 4 * (-1) ** k for k in range(K)])              # y - x is finite, n * t is not
        add("fixed:overflow", first(MAXV[u] / 4, -MAXV[u] / 4, lambda k: MAXV[u] / 4 * (-1) ** k))
        if a == "f32":
            base = 2.0 ** -98
            step = 2.0 ** -23 if u == "f32" else 2.0 ** -7
            for y1 in (base, base * (1 + step), base * (1 - step / 2)):
                for s in (1.0, -1.0):
                    add("fixed:tiny", first(0.0, s * y1, 0.0))
                    add("fixed:tiny", first(-0.0, s * y1, s * y1))
            for s in range(24):
                e = -148 + 2 * s
                add("tiny", [float(rng.uniform(1, 2)) * 2.0 ** e * (-1) ** (k + s) for k in range(K)])
            if u == "f32" and type(N1) is int and N1 % 2 == 0 and N1 & (N1 - 1) and ns[1] == 1:
                for c in tie_numerators(N1):
                    for s in (1.0, -1.0):
                        add("fixed:tie", first(0.0, s * c * (N1 // 2) * 2.0 ** -149, 0.0))
        if a == "f64":
            if u == "f64":
                base = 2.0 ** -600
                for y1 in (base, base * (1 + 2.0 ** -52), base * (1 - 2.0 ** -53)):
                    for s in (1.0, -1.0):
                        add("fixed:tiny", first(0.0, s * y1, 0.0))
                        add("fixed:tiny", first(-0.0, s * y1, s * y1))
                for s in range(24):
                    e = -1070 + 20 * s
                    add("tiny", [float(rng.uniform(1, 2)) * 2.0 ** e * (-1) ** (k + s) for k in range(K)])
                for s in range(8):
                    e = min(590 + 60 * s, 1023)
                    add("huge", [float(rng.uniform(1, 2)) * 2.0 ** e * (-1) ** k for k in range(K)])
                    add("fixed:huge", first(0.0, 1.5 * 2.0 ** e * (-1) ** s, 0.0))
                if ns[1] == 1 and type(N1) is float:
                    for T in near_midpoints(N1):
                        for s in (1.0, -1.0):
                            add("fixed:midpoint", first(0.0, s * float(T), 0.0))
        if u == "f16":
            add("half-nt", [1000.0 * (-1) ** k for k in range(K)])
            add("half-nt", [60000.0 * (-1) ** k for k in range(K)])
            add("fixed:half-nt", first(30000.0, -30000.0, lambda k: 30000.0 * (-1) ** k))
            for y in (2.0 ** -8, 2.0 ** -12, 2.0 ** -16, 2.0 ** -20, 2.0 ** -24):
                add("half-small", [y * (-1) ** k for k in range(K)])
                add("fixed:half-small", first(0.0, y, 0.0))
                add("fixed:half-small", first(-0.0, -y, lambda k: y * (k % 3)))
    else:
        ii = np.iinfo(NP_DT[u])
        mn, mx, bits = int(ii.min), int(ii.max), ii.bits
        IV = [0, -1, mn, mx]
        for _ in range(4):
            add("ordinary", [int(v) for v in rng.integers(-10 ** 6, 10 ** 6, K)])
        for y in IV:
            add("int-extreme", y)
        for j in range(4):
            add("int-extreme", [IV[(k + j) % 4] for k in range(K)])
        for y0, y1 in ((mx, mn), (mn, mx), (mx, -1), (mn, 1), (0, mn), (-1, mx), (mx, -2), (mn // 2, mx), (mn, 0), (-2, mx)):
            add("fixed:wrap-sub", first(y0, y1, lambda k: IV[k % 4]))
        q = 1 << (bits - 3)
        for y0, y1 in ((0, q), (0, -q), (q, -q), (-3 * q, 3 * q), (1, mx // 3 + 7), (5, mx // 1000), (0, 2148), (0, -2147),
                       (7, mx // 1_000_003 + 8), (-7, -(mx // 1_000_003) - 8)):
            add("fixed:wrap-mul", first(y0, y1, lambda k: int(rng.integers(-10 ** 6, 10 ** 6))))
        if u == "i64":
            b53 = 2 ** 53 + 1
            add("fixed:i64-2^53", [b53 + 2 * k for k in range(K)])                 # in y0 and in every later client
            add("fixed:i64-2^53", [-(b53 + 2 * k) for k in range(K)])
            add("fixed:i64-2^53", first(1, 2, lambda k: (b53 + 2 * k) * (-1) ** k))  # in later clients only
            add("i64-2^53", [(b53 + 2 * k) * (-1) ** k for k in range(K)])
            add("i64-2^62", [(2 ** 62 + 2 ** 9 * k + 1) * (-1) ** k for k in range(K)])
            add("fixed:i64-2^62", first(2 ** 62 + 1, -(2 ** 62) - 513, lambda k: 2 ** 62 + 2 ** 9 * k + 1))
        add("int-f32", [16_777_217 + 2 * k for k in range(K)])
        add("int-f32", [-(16_777_217 + 2 * k) for k in range(K)])
    names = [c[0] for c in cols]
    rows = [ys if name.startswith("fixed:") else [ys[j] for j in rng.permutation(K)] for name, ys in cols]
    ups = [cast(u, [r[k] for r in rows]) for k in range(K)]
    return Cols(ups, ns, Ns, names)


def large_total_ties(count=16):
    """(ups, ns) of a K = 2 f32 fold whose total N1 = 49 * 2^30 is beyond CF32's reciprocal range (|N| >= 2^28:
    fill_table hands r = 0): t = y1 = +-49c * 2^-120 with c odd and 2^22 <= 49c < 2^24 is an f32 value of at
    least 2^-98, so no redo covers it, and t / N1 = c * 2^-150 is a tie between two f32 subnormals that
    RN32(RN64(t * RN64(1/N1))) rounds the other way for the c chosen here (RN64(1/49) is far from 1/49).
    Only the IEEE division of the r == 0 arm gets these columns right."""
    N = 49 * 2 ** 30
    c = np.arange((2 ** 22 // 49 + 1) | 1, 2 ** 24 // 49, 2, dtype=np.int64)
    t64 = (49 * c).astype(np.float64) * 2.0 ** -120
    t = t64.astype(np.float32)
    assert (t.astype(np.float64) == t64).all() and (t64 >= 2.0 ** -98).all()
    with np.errstate(all="ignore"):
        fast = (t64 * (1.0 / float(np.float32(N)))).astype(np.float32)
        ieee = t / np.float32(N)
    pick = t[fast != ieee][:count]
    assert len(pick) == count and float(np.float32(N)) == N and (np.abs(ieee) < 2.0 ** -126).all()
    y1 = np.concatenate([pick, -pick]).astype(np.float32)
    return [np.zeros_like(y1), y1], [N - 1, 1]
