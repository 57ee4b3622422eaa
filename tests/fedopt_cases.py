"""Shared builders for the FedOpt step tests (tests/test_fedopt_cases_host.py on the oracle alone,
tests/test_gpu_fedopt_kernels.py on the device): the 17 (update, old) dtype pairs of ``fa_fedopt_step_ex``,
the numpy reference of one step with the server state set directly, the running pseudo-gradient with
its intermediates, and the special-value columns. Plain numpy; nothing here touches a GPU.

A bf16 update is an f32 array whose low 16 bits are zero, and its reference is the f32 computation on
those exact values (test_fedavg_bf16_defined_as_fp32_on_upcast).
"""
import math
from collections import namedtuple

import numpy as np

from oracle import numpy_ref as ref

# (update, old), in the order of fa_fedopt_step_ex's dispatch
PAIRS = [("f32", "f32"), ("bf16", "f32"), ("f32", "f64"), ("f64", "f64"), ("bf16", "f64"), ("f64", "f32"),
         ("f16", "f16"), ("f16", "f32"), ("f16", "f64"), ("f32", "f16"), ("f64", "f16"),
         ("i64", "i64"), ("i64", "f64"), ("i64", "f32"), ("i32", "i32"), ("i32", "f64"), ("i32", "f32")]
OPTS = ["adam", "yogi", "adagrad"]
NP_DT = {"f16": np.float16, "bf16": np.float32, "f32": np.float32, "f64": np.float64, "i32": np.int32, "i64": np.int64}
_RANK = {"f16": 0, "bf16": 1, "f32": 1, "f64": 2}
_BY_RANK = ["f16", "f32", "f64"]
# NaN bit patterns planted into every array (positive, negative): quiet, with a payload
NAN_BITS = {2: (0x7E11, 0xFE25), 4: (0x7FC10000, 0xFFC50000), 8: (0x7FF8200000000000, 0xFFF8A00000000000)}
_UINT = {2: np.uint16, 4: np.uint32, 8: np.uint64}
BF16_MAX = float(np.array([0x7F7F0000], np.uint32).view(np.float32)[0])
MAXV = {"f16": 65504.0, "bf16": BF16_MAX, "f32": float(np.finfo(np.float32).max), "f64": float(np.finfo(np.float64).max)}
SUBV = {"f16": 2.0 ** -24, "bf16": 2.0 ** -133, "f32": 2.0 ** -149, "f64": 5e-324}


def is_int(name):
    return name[0] == "i"


def promote(a, b):
    """numpy's result dtype of two float arrays (bf16 counts as the f32 it is upcast to)."""
    return _BY_RANK[max(_RANK[a], _RANK[b])]


def pg_dtype(pair):
    """The pseudo-gradient's dtype: next*1.0 + old*(-1.0); an integer array times a python float is f64."""
    u, o = pair
    if is_int(u):
        return "f64"
    return promote(u, o)


def m_out_dtype(pair, m_dt):
    return pg_dtype(pair) if m_dt is None else promote(m_dt, pg_dtype(pair))


def to_bf16(a):
    """f32 values rounded to the nearest bf16 (ties to even), held as f32 with the low 16 bits zero."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = a.view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    r = np.where(np.isnan(a), (b.astype(np.uint32) & np.uint32(0xFFFF0000)) | np.uint32(0x00400000), r)
    return r.astype(np.uint32).view(np.float32)


def cast(name, values):
    """``values`` (python numbers or an array) as an array of dtype ``name``, NaNs replaced by the
    payload patterns of NAN_BITS by sign. Integer dtypes take python ints exactly."""
    if is_int(name):
        return np.array([int(v) for v in values], dtype=NP_DT[name])
    with np.errstate(all="ignore"):
        a = np.array(values, dtype=np.float64).astype(NP_DT[name])
        if name == "bf16":
            a = to_bf16(a)
    a = np.ascontiguousarray(a)
    pos, neg = NAN_BITS[a.dtype.itemsize]
    bits = a.view(_UINT[a.dtype.itemsize])
    nan = np.isnan(a)
    sgn = np.signbit(a)
    bits[nan & ~sgn] = pos
    bits[nan & sgn] = neg
    return a


def params(opt, kind):
    """"default": the reference's beta1 / beta2 / lr / tau. "odd": values with no exact f32 or f16 form
    that differ from each other, tau = 0.0 for Adam and AdaGrad (0/0 and m/0), 2^-10 for Yogi (tau^2 is
    then exactly the square of a pseudo-gradient of 2^-10)."""
    if kind == "default":
        return {"serveropt": opt}
    return {"serveropt": opt, "learning_rate": 1e-2, "beta1": 0.7, "beta2": 0.999,
            "tau": 2.0 ** -10 if opt == "yogi" else 0.0}


def client_ns(K, kind="plain"):
    """num_examples per client, python numbers. Client 1 always has n = 1, so that t = d - pg at the
    first fold step (the ``fixed:*`` columns rely on it).
    "float": n[0] is a python float with a full 53-bit significand just below 2^11 (so has the first
             running total N1: RN64(1/N1) is then as far from 1/N1 as it gets), n[2] is 2.75, n[3] is
             1000 (the totals pass 2048: not half values);
    "big":   N1 = 98 (even, and RN64(1/98) is far from 1/98: ties of t/N1 between f32 subnormals exist and
             round differently through the reciprocal), the running total is 16 777 217 at client 2 (not an
             f32 value) and n[4] = 2^28 + 5 (the totals from there on select IEEE division in CF32); in
             half, n and N become inf."""
    rng = np.random.default_rng(K * 31 + len(kind))
    ns = [int(v) for v in rng.integers(1, 500, K)]
    if K > 1:
        ns[1] = 1
    if kind == "float":
        ns[0] = 2044.9858126302304
        if K > 2:
            ns[2] = 2.75
        if K > 3:
            ns[3] = 1000
    elif kind == "big":
        ns[0] = 97
        if K > 2:
            ns[2] = 16_777_119
        if K > 4:
            ns[4] = 2 ** 28 + 5
    assert all(type(n) in (int, float) for n in ns)
    return ns


def tie_numerators(N, count=12):
    """Odd c for which t = c * (N/2) * 2^-149 (an f32 value; t / N = c * 2^-150 is a tie between two f32
    subnormals) rounds differently as RN32(RN64(t * RN64(1/N))) and as the IEEE quotient: the lanes that
    CF32::fold_strip must redo with a division. N even, not a power of two."""
    h = N // 2
    c = np.arange(1, min(2 ** 12, (2 ** 24 - 1) // h), 2, dtype=np.int64)
    t = ((c * h).astype(np.float64) * 2.0 ** -149).astype(np.float32)
    with np.errstate(all="ignore"):
        fast = (t.astype(np.float64) * (1.0 / float(np.float32(N)))).astype(np.float32)
        ieee = t / np.float32(N)
    return [int(x) for x in c[fast != ieee][:count]]


def near_midpoints(N, ds=(1, -1, 3, -3, 5, -5)):
    """Integers T < 2^53 whose quotient T / N lies as close to a binary64 rounding midpoint as a quotient
    of two doubles can: |z - mid| = |d| ulp / (2 N') with N' the odd significand of N (the construction
    of tests/test_fastdiv64.py): T * 2^54 = M * N' - d with M odd, 54 bits."""
    m, _ = math.frexp(N)
    Ni = int(m * 2 ** 53)
    No = Ni >> ((Ni & -Ni).bit_length() - 1)
    inv = pow(No, -1, 2 ** 54)
    out = []
    for d in ds:
        M = (d * inv) % 2 ** 54
        T = (M * No - d) // 2 ** 54
        if M >= 2 ** 53 and T < 2 ** 53:
            out.append(T)
    return out


def totals(ns):
    """The running totals as fedopt.py accumulates them (python arithmetic)."""
    out, t = [], 0
    for n in ns:
        t += n
        out.append(t)
    return out


def reference(pair, old, ups, ns, m, v, params, f32state=False):
    """(out, m, v) of one round from the oracle, with the server state set directly to arrays of the
    requested dtypes. An f32 ``v`` outside the f32-state mode is widened exactly to f64 first, which is
    how that mode defines a stored f32 v (fedopt_combine_f32state does the same)."""
    st = ref.FedOptState()
    st.m = None if m is None else [m]
    if v is None:
        st.v = None
    else:
        st.v = [v] if (f32state or v.dtype == np.float64) else [v.astype(np.float64)]
    fn = ref.fedopt_combine_f32state if f32state else ref.fedopt_combine
    with np.errstate(all="ignore"):
        model, nr = fn(st, [([u], n) for u, n in zip(ups, ns)], [old], params)
    assert model is not None, f"the oracle returned None for {pair} {params}"
    assert nr == len(ups), f"the oracle skipped a client for {pair}: {nr} of {len(ups)}"
    return model[0], st.m[0], st.v[0]


Step = namedtuple("Step", "t N q pg")


def fold_trace(old, ups, ns):
    """The running pseudo-gradient after every client, with the fold's intermediates: a list of
    Step(t = n*(d - pg), N, q = t/N, pg after the step); client 0 has t = q = None. Each step is checked
    against the oracle's increment_average."""
    out, total, pg = [], 0, None
    with np.errstate(all="ignore"):
        for k, (u, n) in enumerate(zip(ups, ns)):
            total += n
            d = ref.subtract([u], [old])[0]
            if k == 0:
                pg = d
                out.append(Step(None, total, None, pg))
                continue
            t = np.multiply(n, np.subtract(d, pg))
            q = np.true_divide(t, total)
            new = np.add(pg, q)
            want = ref.increment_average([pg], [d], n, total)[0]
            assert new.dtype == want.dtype and new.tobytes() == want.tobytes()
            pg = new
            out.append(Step(t, total, q, pg))
    return out


Cols = namedtuple("Cols", "old ups m v ns names")


def special_columns(pair, K, opt, params, ns_kind="float", m_dt=None, seed=11):
    """One scenario per column: ``old`` (C values of the old dtype: row 0), ``ups`` (K rows of the update
    dtype: rows 1..K), the matching ``m`` (dtype ``m_dt``, default the pseudo-gradient's) and ``v``
    (f64) rows, the clients' ``ns`` and the columns' names. Client order is permuted per column except in
    the columns named ``fixed:*``, which are written for n[1] = 1. The columns do not depend on ``opt`` and
    ``params``; the Yogi columns hold v = 2^-20 = tau^2 of params("yogi", "odd"), so that a missing v gives
    the same zero there (asserted).

    Families (float pairs): pg = +-0; tiny t around 2^-98 (f32 pg from f32 / bf16 updates) or 2^-600
    (f64 pg from f64 updates: narrower updates cannot make such a difference), ties of t/N between f32
    subnormals that the reciprocal rounds the other way, f64 quotients next to a rounding midpoint; huge
    f64 t and overflowing n*t; inf / NaN in old, one client, all clients; special m / v; the largest finite and
    smallest subnormal of each dtype; Yogi's v - pg^2 = +0 and around it; half squares that overflow,
    are subnormal or vanish, half n*t that overflows. Integer pairs: 0, -1, min, max; int64 beyond
    2^53 and 2^62; 16 777 217-like updates."""
    u, o = pair
    pg = pg_dtype(pair)
    m_dt = m_dt or pg
    rng = np.random.default_rng(seed + 7 * K)
    ns = client_ns(K, ns_kind)
    inf, nan = math.inf, math.nan
    nnan = math.copysign(math.nan, -1.0)
    tau2 = 2.0 ** -20            # params("yogi", "odd")'s tau^2: a missing v gives the same zero there
    assert opt != "yogi" or params.get("tau") in (None, 2.0 ** -10)
    cols = []
    M_ORD, V_ORD = [0.0, 0.25, -0.5, 1.0], [1e-8, 0.0625, 1.0, 4.0]

    def add(name, old, ys, m=None, v=None):
        ys = list(ys) if isinstance(ys, (list, tuple)) else [ys] * K
        assert len(ys) == K
        i = len(cols)
        cols.append((name, old, ys, M_ORD[i % 4] if m is None else m, V_ORD[(i // 4) % 4] if v is None else v))

    MS = [inf, -inf, nan, nnan, -1.5, 0.0, -0.0, SUBV[m_dt], -MAXV[m_dt]]
    VS = [inf, -inf, nan, -1.0, 0.0, -0.0, 5e-324, 1.7e308, 4.0]
    if not is_int(u):
        grid = [1.0 + 2.0 ** -6 * ((k % 5) - 2) for k in range(K)]
        # pg = +-0
        for old in (1.5, 0.0, -0.0):
            for m, v in ((None, None), (0.0, 0.0), (-1.5, 0.0), (0.0, -0.0)):
                add("zero", old, old, m, v)
        add("zero", 0.0, -0.0)
        add("zero", -0.0, 0.0)
        add("fixed:zero", 0.0, [-0.0 if k % 2 else 0.0 for k in range(K)])       # d - pg = -0: t and t/N are -0
        # tiny t
        bound = {("f32", "f32"): 2.0 ** -98, ("f32", "bf16"): 2.0 ** -98, ("f64", "f64"): 2.0 ** -600}.get((pg, u))
        if bound and K >= 2:
            base = bound                    # n[1] = 1: t = y1 at the first fold step
            step = {"f32": 2.0 ** -23, "bf16": 2.0 ** -7, "f64": 2.0 ** -52}[u]
            for y1 in (base, base * (1 + step), base * (1 - step / 2)):
                for s in (1.0, -1.0):
                    add("fixed:tiny", 0.0, [0.0, s * y1] + [0.0] * (K - 2), v=0.0)
                    add("fixed:tiny", -0.0, [-0.0, s * y1] + [s * y1] * (K - 2))
            lo, st = (-148, 2) if pg == "f32" else (-1070, 20)
            for s in range(24):
                e = lo + st * s
                ys = [float(rng.uniform(1, 2)) * 2.0 ** e * (-1) ** (k + s) for k in range(K)]
                add("tiny", 0.0 if s % 2 == 0 else 1.5 * 2.0 ** e, ys, v=0.0 if s % 3 == 0 else None)
            N1 = totals(ns)[1]
            if pg == "f32" and u == "f32" and N1 % 2 == 0 and N1 & (N1 - 1):
                for c in tie_numerators(N1):
                    for s in (1.0, -1.0):
                        add("fixed:tie", 0.0, [0.0, s * c * (N1 // 2) * 2.0 ** -149] + [0.0] * (K - 2))
            if pg == "f64" and type(N1) is float:
                for T in near_midpoints(N1):
                    for s in (1.0, -1.0):
                        add("fixed:midpoint", 0.0, [0.0, s * float(T)] + [0.0] * (K - 2))
        if pg == "f64" and u == "f64":
            for s in range(8):
                e = 590 + 60 * s
                add("huge", 0.0 if s % 2 else -MAXV[o] if o != "f64" else 2.0 ** e,
                    [float(rng.uniform(1, 2)) * 2.0 ** min(e, 1023) * (-1) ** k for k in range(K)])
        # inf / NaN
        for s in (inf, -inf, nan, nnan):
            add("old-special", s, grid)
            add("one-special", 1.0, [s] + grid[1:])
            add("all-special", 1.0, s)
            add("all-special", s, s)
            add("all-special", -s, s)
        for h in sorted({1, K // 2}):
            add("inf-inf", 1.0, [inf] * h + [-inf] * (K - h))
        # m / v
        for m in MS:
            for v in VS:
                add("mv", 1.0, grid, m, v)
            for v in (0.0, inf, 4.0):
                add("mv-zero-pg", 1.0, 1.0, m, v)
        # extremes of each dtype
        for old in (MAXV[o], -MAXV[o], SUBV[o], -SUBV[o], 0.0):
            for y in (MAXV[u], -MAXV[u], SUBV[u], -SUBV[u]):
                add("extreme", old, y)
        ext = [MAXV[u], -MAXV[u], SUBV[u], 0.0, -SUBV[u]]
        add("extreme", 0.0, [ext[k % 5] for k in range(K)])
        add("extreme", -MAXV[o], [ext[k % 5] for k in range(K)])
        # Yogi: v - pg^2 = +0, just below, just above
        for s in (1.0, -1.0):
            for v in (tau2, tau2 * (1 - 2.0 ** -53), tau2 * (1 + 2.0 ** -52)):
                add("yogi-zero", 0.0, s * math.sqrt(tau2), v=v)
                if u != "bf16":
                    add("yogi-zero", 1.0, 1.0 + s * 2.0 ** -10, v=2.0 ** -20 * (v / tau2))
        # half: squares that overflow / are subnormal / vanish, n*t that overflows
        for y in (255.0, 256.0, 300.0, 2.4e-4, 1e-4, 6e-5, 2.0 ** -24):
            add("half-square", 0.0, y)
            add("half-square", -0.0, -y, v=0.0)
        add("half-nt", 0.0, [1000.0 * (-1) ** k for k in range(K)])
        add("half-nt", 1.0, [60000.0 * (-1) ** k for k in range(K)])
    else:
        ii = np.iinfo(NP_DT[u])
        IV = [0, -1, int(ii.min), int(ii.max)]
        olds = IV if is_int(o) else [0.0, -1.0, 0.5, inf, -inf, nan, nnan, MAXV[o], SUBV[o]]
        for old in olds:
            for y in IV:
                add("int-extreme", old, y)
            add("int-extreme", old, [IV[k % 4] for k in range(K)])
        zero = 0 if is_int(o) else 0.0
        if u == "i64":
            b53 = 2 ** 53 + 1
            add("i64-2^53", b53 if is_int(o) else zero, [b53 + 2 * k for k in range(K)])
            add("i64-2^53", zero, [-(b53 + 2 * k) for k in range(K)])
            add("i64-2^62", zero, [(2 ** 62 + 2 ** 9 * k + 1) * (-1) ** k for k in range(K)])
            if is_int(o):
                add("i64-2^62", 2 ** 62 + 1, [2 ** 62 + 2 ** 9 * k + 1 for k in range(K)])
                add("i64-wrap", int(ii.min), int(ii.max))
                add("i64-wrap", int(ii.max), int(ii.min))
        add("int-f32", 16_777_216 if is_int(o) else 16_777_216.0, [16_777_217 + 2 * k for k in range(K)])
        add("int-f32", zero, [-(16_777_217 + 2 * k) for k in range(K)])
        for m in MS:
            for v in (inf, nan, -1.0, 0.0, 4.0):
                add("mv", zero, [(k % 3) - 1 for k in range(K)], m, v)
        for m, v in ((0.0, 0.0), (-1.5, 0.0)):
            add("zero", 5 if is_int(o) else 5.0, 5, m, v)
        for s in (1, -1):
            for v in (1.0, 1.0 - 2.0 ** -53, 1.0 + 2.0 ** -52):
                add("yogi-zero", zero, s, v=v)
    names = [c[0] for c in cols]
    rows = []
    for name, _, ys, _, _ in cols:
        rows.append(ys if name.startswith("fixed:") else [ys[j] for j in rng.permutation(K)])
    ups = [cast(u, [r[k] for r in rows]) for k in range(K)]
    return Cols(cast(o, [c[1] for c in cols]), ups, cast(m_dt, [c[3] for c in cols]),
                cast("f64", [c[4] for c in cols]), ns, names)


def as_f32(v):
    """An f64 v row as the f32 state stores it (values beyond f32 become inf)."""
    with np.errstate(all="ignore"):
        return v.astype(np.float32)


def tile(a, P):
    """The columns repeated cyclically to P elements."""
    return np.ascontiguousarray(np.resize(a, P))
