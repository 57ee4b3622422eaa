"""The builders of tests/fedavg_cases.py reach the lanes they were written for — shown on the oracle
alone, so that a wrong bound in a builder cannot silently remove a scenario from
tests/test_gpu_fedavg_kernels.py. The fold's intermediates are recomputed in numpy (d = y - x, t = n*d and
the quotient per step) and each lane of the fold rules' special-value code (fold_rules.h: CF32's redo, its
r == 0 division, CF64::div's guard, CF16's rounding of n and N and of every operation, the integer first
step) is asserted to be hit by at least one column; no family of columns may be empty."""
from fractions import Fraction

import numpy as np
import pytest

import fedavg_cases as fa
from oracle import numpy_ref as ref

KS = [2, 5, 65]
_ids = "-".join

FAMILIES = {
    "float": {"ordinary", "fixed:zero", "zero", "const", "one-special", "all-special", "inf-inf", "extreme", "overflow",
              "fixed:overflow"},
    ("f32", "f32"): {"fixed:tiny", "tiny"}, ("bf16", "f32"): {"fixed:tiny", "tiny"},
    ("f64", "f64"): {"fixed:tiny", "tiny", "huge", "fixed:huge", "fixed:midpoint"}, ("f32", "f64"): set(),
    ("f16", "f16"): {"half-nt", "fixed:half-nt", "half-small", "fixed:half-small"},
    "int": {"ordinary", "int-extreme", "fixed:wrap-sub", "fixed:wrap-mul", "int-f32"},
    ("i64", "f64"): {"fixed:i64-2^53", "i64-2^53", "i64-2^62", "fixed:i64-2^62"}, ("i32", "f64"): set(),
}


def _trace(pair, kind="plain", K=5):
    c = fa.special_columns(pair, K, kind)
    tr, final = fa.fold_trace(pair, c.ups, c.ns)
    return c, tr, final


def _cols(c, name):
    return [i for i, n in enumerate(c.names) if n == name]


def test_pairs_are_the_dispatch():
    assert len(fa.PAIRS) == 7 and len(set(fa.PAIRS)) == 7
    assert [fa.E_OF[p] for p in fa.PAIRS] == [4, 8, 8, 2, 4, 2, 4]
    assert len(fa.REFUSED) == 29 and not set(fa.REFUSED) & set(fa.PAIRS)
    assert {("f64", "f32"), ("f16", "f32"), ("i64", "i64")} <= set(fa.REFUSED)
    assert fa.NO_COPY == [("bf16", "f32"), ("f32", "f64"), ("i64", "f64"), ("i32", "f64")]


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("pair", fa.PAIRS, ids=_ids)
def test_no_family_is_empty(pair, K):
    """Every family of the pair has a column under every ns list, the ties under "big" (N1 = 98) and the
    midpoints wherever n[1] = 1; the columns fit into the GPU tests' P with room to repeat."""
    for kind in fa.kinds(pair):
        c = fa.special_columns(pair, K, kind)
        want = set(FAMILIES["int" if fa.is_int(pair[0]) else "float"]) | FAMILIES[pair]
        if pair == ("f32", "f32") and kind == "big":
            want |= {"fixed:tie"}
        if kind != "float":
            want -= {"fixed:midpoint"}                # built for a float N1 with a full significand
        got = set(c.names) - (set() if kind == "big" else {"fixed:tie"})      # (other lists may have an even N1 too)
        assert got == want, (pair, kind, got ^ want)
        assert len(c.ups) == K and len({len(u) for u in c.ups}) == 1 and 30 <= len(c.names) < 1024
        assert all(u.dtype == fa.NP_DT[pair[0]] for u in c.ups)
        out = fa.reference(pair, None, c.ups, c.ns, c.Ns)
        assert out.dtype == fa.NP_DT[pair[1]]


def test_ns_lists():
    h = np.float16
    with np.errstate(all="ignore"):
        f = fa.ns_for(("f16", "f16"), 5, "float")
        Nf = fa.totals(f)
        assert f[1] == 1 and f[4] == 2049 and float(h(f[4])) == 2048.0
        # one rounding from double against a rounding through float: n and N
        assert float(h(f[2])) == 2050.0 and float(h(np.float32(f[2]))) == 2048.0
        assert float(h(Nf[3])) == 5100.0 and float(h(np.float32(Nf[3]))) == 5096.0
        b = fa.ns_for(("f16", "f16"), 5, "big")
        Nb = fa.totals(b)
        assert Nb[1] == 2049 and float(h(Nb[1])) == 2048.0
        assert Nb[2] == 65519 and float(h(Nb[2])) == 65504.0 and np.isinf(h(Nb[3])) and np.isinf(h(b[4]))
        assert b[3] == 65519 and float(h(b[3])) == 65504.0 and b[4] == 65520
        assert float(np.multiply(b[4], np.ones(1, h))[0]) == np.inf          # numpy's own conversion of the python int
    for pair in (("f64", "f64"), ("f32", "f64")):
        n = fa.ns_for(pair, 5, "float")
        assert n[4] == 2.0 ** 61 and fa.totals(n)[4] > 2.0 ** 60 and all(t < 2.0 ** 60 for t in fa.totals(n)[:4])
        assert any(type(x) is float and x != int(x) for x in n)
    for pair in (("f32", "f32"), ("bf16", "f32")):
        t = fa.totals(fa.ns_for(pair, 5, "big"))
        assert t[1] == 98 and any(float(np.float32(x)) != x for x in t) and t[4] >= 2 ** 28
        assert all(abs(float(np.float32(x))) < 2.0 ** 28 for x in t[:4])
        assert all(type(x) is float for x in fa.totals(fa.ns_for(pair, 5, "float")))
    for pair in (("i64", "f64"), ("i32", "f64")):
        for kind in fa.kinds(pair):
            n = fa.ns_for(pair, 5, kind)
            assert all(type(x) is int for x in n) and abs(n[1]) < 2 ** 31
        t = fa.totals(fa.ns_for(pair, 5, "big"))
        assert t[2] == 2 ** 53 + 3 and int(float(t[2])) != t[2]


@pytest.mark.parametrize("pair", fa.PAIRS, ids=_ids)
def test_reference_start_rules_and_fedavg_flat(pair):
    """The start rule of each pair, the result dtype, waves == one call, and agreement with
    ``ref.fedavg_flat`` wherever both are defined (same-dtype float pairs and integer pairs, int n)."""
    u, a = pair
    for kind in fa.kinds(pair):
        c = fa.special_columns(pair, 5, kind)
        s = fa.start(pair, c.ups[0])
        if pair == ("f32", "f64"):
            assert s.dtype == np.float64 and (s.astype(np.float32).tobytes() == c.ups[0].tobytes())
        elif fa.is_int(u):
            assert s is c.ups[0] and s.dtype.kind == "i"
        else:
            assert s is c.ups[0]
        if u == "bf16":
            assert all(not (x.view(np.uint32) & 0xFFFF).any() for x in c.ups)
        whole = fa.reference(pair, None, c.ups, c.ns, c.Ns)
        assert whole.dtype == fa.NP_DT[a]
        part = fa.reference(pair, None, c.ups[:2], c.ns[:2], c.Ns[:2])
        rest = fa.reference(pair, part, c.ups[2:], c.ns[2:], c.Ns[2:])
        assert rest.tobytes() == whole.tobytes()
        if (u == a or fa.is_int(u)) and all(type(n) is int for n in c.ns):
            with np.errstate(all="ignore"):
                flat = ref.fedavg_flat(c.ups, c.ns)
            assert flat.dtype == whole.dtype and flat.tobytes() == whole.tobytes()
    if pair in fa.NO_COPY and not fa.is_int(u):
        c = fa.special_columns(pair, 2)
        assert fa.reference(pair, None, c.ups[:1], c.ns[:1], c.Ns[:1]).dtype == fa.NP_DT[a]
    if fa.is_int(u):                # K = 1 has no f64 result: the refused copy
        c = fa.special_columns(pair, 2)
        with pytest.raises(AssertionError):
            fa.reference(pair, None, c.ups[:1], c.ns[:1], c.Ns[:1])


def _f32_tiny(tr):
    hit = above = False
    for s in tr[1:]:
        assert s.t.dtype == np.float32
        a = np.abs(s.t.astype(np.float64))
        N = float(np.float32(s.N))
        if abs(N) >= 2.0 ** 28:
            continue
        hit |= bool(((a > 0) & (a < 2.0 ** -98) & (a / N < 2.0 ** -126)).any())
        above |= bool(((a > 2.0 ** -98) & (a < 2.0 ** -97)).any())
    return hit, above


@pytest.mark.parametrize("kind", ["plain", "float", "big"])
@pytest.mark.parametrize("pair", [("f32", "f32"), ("bf16", "f32")], ids=_ids)
def test_f32_tiny_lane(pair, kind):
    """0 < |t| < 2^-98 with a subnormal exact quotient while r != 0, t on both sides of the bound and on it."""
    c, tr, _ = _trace(pair, kind)
    assert _f32_tiny(tr) == (True, True)
    t1 = np.abs(tr[1].t[_cols(c, "fixed:tiny")].astype(np.float64))
    assert (t1 == 2.0 ** -98).any() and (t1 > 2.0 ** -98).any() and ((t1 < 2.0 ** -98) & (t1 > 0)).any()


def _ties(c, tr):
    tie = _cols(c, "fixed:tie")
    s = tr[1]
    t = s.t[tie]
    with np.errstate(all="ignore"):
        fast = (t.astype(np.float64) * (1.0 / float(np.float32(s.N)))).astype(np.float32)
    return tie, t, fast, s.q[tie]


@pytest.mark.parametrize("K", KS)
def test_f32_tie_lane(K):
    """RN32(RN64(t * r)) != t / N: without the redo of 0 < |t| < 2^-98 every one of these columns is wrong
    at the first step."""
    c, tr, _ = _trace(("f32", "f32"), "big", K)
    tie, t, fast, q = _ties(c, tr)
    assert len(tie) >= 16 and tr[1].N == 98 and c.ns[1] == 1
    a = np.abs(t.astype(np.float64))
    assert ((a > 0) & (a < 2.0 ** -98)).all()
    assert (fast != q).all() and (np.abs(q) < 2.0 ** -126).all()


def test_bf16_rounding_of_the_f32_columns():
    """The f32 columns passed through to_bf16 (what the pipelined geometry's bf16 run folds): the tiny lane,
    the zeros, inf, NaN, inf - inf and the r == 0 totals survive; the ties do not (a bf16 value is a
    multiple of 2^-133, so t / 98 is never halfway between two f32 subnormals), and f32's largest finite
    value becomes inf."""
    c = fa.special_columns(("f32", "f32"), 5, "big")
    ups = [fa.to_bf16(u) for u in c.ups]
    assert all(not (u.view(np.uint32) & 0xFFFF).any() for u in ups)
    tr, final = fa.fold_trace(("bf16", "f32"), ups, c.ns)
    assert _f32_tiny(tr) == (True, True)
    tie = _cols(c, "fixed:tie")
    t = tr[1].t[tie]
    with np.errstate(all="ignore"):
        fast = (t.astype(np.float64) * (1.0 / 98.0)).astype(np.float32)
    assert len(tie) >= 16 and (fast == tr[1].q[tie]).all()
    ex = _cols(c, "extreme")
    assert np.isinf(ups[0][ex]).any() and (np.abs(c.ups[0][ex]) == fa.MAXV["f32"]).any()
    tt = np.concatenate([s.t for s in tr[1:]])
    assert np.isnan(final).any() and np.isinf(tt).any() and ((tt == 0) & np.signbit(tt)).any()
    assert any(np.isnan(u).any() for u in ups) and float(np.float32(tr[-1].N)) >= 2.0 ** 28


@pytest.mark.parametrize("pair", [p for p in fa.PAIRS if not fa.is_int(p[0])], ids=_ids)
def test_zero_nonfinite_and_overflow_lanes(pair):
    """The four sign combinations of x, y = +-0 at the first step, t of both zero signs, NaN t, inf - inf,
    and n * t overflowing from a finite difference, in every float pair."""
    for kind in fa.kinds(pair):
        c, tr, final = _trace(pair, kind)
        z = _cols(c, "fixed:zero")
        x0, y1 = fa.start(pair, c.ups[0])[z], c.ups[1][z]
        combos = {(bool(np.signbit(x)), bool(np.signbit(y))) for x, y in zip(x0, y1)}
        assert (x0 == 0).all() and (y1 == 0).all() and len(combos) == 4
        t = np.concatenate([s.t for s in tr[1:]])
        d = np.concatenate([s.d for s in tr[1:]])
        assert ((t == 0) & np.signbit(t)).any() and ((t == 0) & ~np.signbit(t)).any() and np.isnan(t).any()
        assert np.isnan(final).any() and any(np.isinf(s.x).any() for s in tr[1:])
        ii = _cols(c, "inf-inf")
        assert any(np.isnan(s.d[ii]).any() and np.isinf(s.x[ii]).any() for s in tr[1:])
        if pair == ("f32", "f64"):                          # an f64 t of f32 values cannot overflow
            assert not (np.isinf(t) & np.isfinite(d)).any()
        elif pair != ("f16", "f16") or kind == "plain":     # (the half lists' n is 1 or overflows by itself)
            assert (np.isinf(t) & np.isfinite(d)).any()
        ex = _cols(c, "extreme")
        vals = np.abs(np.concatenate([u[ex].astype(np.float64) for u in c.ups]))
        assert (vals == fa.MAXV[pair[0]]).any() and (vals == fa.SUBV[pair[0]]).any()


@pytest.mark.parametrize("pair", [p for p in fa.PAIRS if not fa.is_int(p[0])], ids=_ids)
def test_nan_payloads_are_planted(pair):
    c = fa.special_columns(pair, 5)
    size = c.ups[0].dtype.itemsize
    view = {2: np.uint16, 4: np.uint32, 8: np.uint64}[size]
    pos, neg = fa.NAN_BITS[size]
    if pair[0] == "bf16":
        pos, neg = pos & 0xFFFF0000, neg & 0xFFFF0000
    bits = np.concatenate([u[np.isnan(u)].view(view) for u in c.ups])
    assert (bits == pos).any() and (bits == neg).any() and set(bits.tolist()) <= {pos, neg}
    one = _cols(c, "one-special")
    assert any(sum(bool(np.isnan(u[i])) for u in c.ups) == 1 for i in one)
    assert any(all(np.isnan(u[i]) for u in c.ups) for i in _cols(c, "all-special"))


@pytest.mark.parametrize("pair", [("f32", "f32"), ("bf16", "f32")], ids=_ids)
def test_f32_total_lanes(pair):
    """A running total that is not an f32 value, totals >= 2^28 (r == 0: IEEE division) and below, and a
    python-float n and N."""
    c, tr, _ = _trace(pair, "big")
    Ns = [s.N for s in tr[1:]]
    assert 16_777_217 in Ns and float(np.float32(16_777_217)) != 16_777_217
    assert any(float(np.float32(N)) >= 2.0 ** 28 for N in Ns) and any(float(np.float32(N)) < 2.0 ** 28 for N in Ns)
    c, tr, _ = _trace(pair, "float")
    assert all(type(s.N) is float for s in tr[1:]) and any(type(n) is float and n != int(n) for n in c.ns)


def test_f64_guard_lanes():
    """|t| below 2^-600 and above 2^600 (CF64::div's guard), t on the lower bound and on both sides of it,
    n * t overflowing, and r == 0 from a total above 2^60."""
    for kind in ("plain", "float", "big"):
        c, tr, _ = _trace(("f64", "f64"), kind)
        tiny = huge = over = False
        for s in tr[1:]:
            assert s.t.dtype == np.float64
            a = np.abs(s.t)
            tiny |= bool(((a > 0) & (a < 2.0 ** -600)).any())
            huge |= bool(((a > 2.0 ** 600) & np.isfinite(a)).any())
            over |= bool(np.isinf(a).any())
        assert tiny and huge and over
        t1 = np.abs(tr[1].t[_cols(c, "fixed:tiny")])
        assert (t1 == 2.0 ** -600).any() and (t1 > 2.0 ** -600).any() and ((t1 < 2.0 ** -600) & (t1 > 0)).any()
        h1 = np.abs(tr[1].t[_cols(c, "fixed:huge")])
        assert (h1 > 2.0 ** 600).any() and (h1 < 2.0 ** 600).any()
    c, tr, _ = _trace(("f64", "f64"), "float")
    assert tr[4].N > 2.0 ** 60 and tr[3].N < 2.0 ** 60 and np.isfinite(tr[4].q).any() and (tr[4].t != 0).any()
    c, tr, _ = _trace(("f32", "f64"), "float")              # f32 updates: t stays inside the guard
    assert tr[4].N > 2.0 ** 60
    a = np.abs(np.concatenate([s.t for s in tr[1:4]]))
    assert not ((a > 0) & (a < 2.0 ** -600)).any()


@pytest.mark.parametrize("kind", ["float"])
def test_f64_near_midpoint_lane(kind):
    """t / N1 next to a rounding midpoint, inside CF64::div's shortcut range. (An f32 update cannot make
    such a 53-bit t at the first step, so (f32, f64) has no such columns.)"""
    c, tr, _ = _trace(("f64", "f64"), kind)
    mid = _cols(c, "fixed:midpoint")
    s = tr[1]
    assert len(mid) >= 4 and c.ns[1] == 1
    wrong = 0
    for t, q in zip(s.t[mid], s.q[mid]):
        assert 2.0 ** -600 <= abs(t) <= 2.0 ** 600 and q == t / s.N
        ulp = Fraction(float(np.spacing(abs(q))))
        z = Fraction(float(t)) / Fraction(s.N)
        assert abs(abs(z - Fraction(float(q))) - ulp / 2) < ulp * Fraction(1, 2 ** 40)
        wrong += float(t) * (1.0 / s.N) != q
    if kind == "float":
        assert wrong                         # t * RN(1/N1) alone is wrong for some of them


def test_half_lanes():
    h = np.float16
    with np.errstate(all="ignore"):
        c, tr, _ = _trace(("f16", "f16"), "plain")
        nt = _cols(c, "half-nt") + _cols(c, "fixed:half-nt")
        assert any((np.isinf(s.t[nt]) & np.isfinite(s.d[nt])).any() for s in tr[1:])      # n * t overflows in half
        sm = _cols(c, "half-small") + _cols(c, "fixed:half-small")
        q = np.concatenate([s.q[sm] for s in tr[1:]])
        t = np.concatenate([s.t[sm] for s in tr[1:]])
        assert q.dtype == h and ((np.abs(q) > 0) & (np.abs(q) < 2.0 ** -14)).any()         # subnormal quotient
        assert ((q == 0) & (t != 0)).any()                                                 # ... and one that vanishes
        # the "float" list: numpy's n and N are one rounding from double; a rounding through float changes results
        c, tr, final = _trace(("f16", "f16"), "float")
        assert float(h(c.ns[2])) == 2050.0 and float(h(tr[3].N)) == 5100.0
        for k in (2, 3):                   # n through float at client 2, N through float at client 3
            x = tr[k].x
            via_float = x + (h(np.float32(c.ns[k])) * (c.ups[k] - x)) / h(np.float32(tr[k].N))
            ok = np.isfinite(via_float) & np.isfinite(tr[k + 1].x)
            assert via_float.dtype == h and (via_float[ok] != tr[k + 1].x[ok]).any()
        # the "big" list: half n == inf with y == x gives inf * 0, half N == inf
        c, tr, final = _trace(("f16", "f16"), "big")
        assert np.isfinite(h(c.ns[3])) and np.isinf(h(tr[3].N)) and np.isfinite(h(tr[2].N)) and np.isinf(h(c.ns[4]))
        fin = np.isfinite(tr[3].t)
        assert (tr[3].q[fin] == 0).all() and (tr[3].t[fin] != 0).any()                     # finite t / inf N
        const = _cols(c, "const")
        assert (tr[4].d[const] == 0).all() and np.isnan(tr[4].t[const]).all() and np.isnan(final[const]).all()
        ex = _cols(c, "extreme")
        vals = np.abs(np.concatenate([u[ex] for u in c.ups]).astype(np.float64))
        assert (vals == 65504.0).any() and (vals == 2.0 ** -24).any()


@pytest.mark.parametrize("pair", [("i64", "f64"), ("i32", "f64")], ids=_ids)
def test_integer_first_step_lanes(pair):
    """The first step in the integer dtype: a difference and a product that differ from the exact ones, the
    product also where the difference is exact; the dtype's extremes; from the second step on float64."""
    dt = fa.NP_DT[pair[0]]
    ii = np.iinfo(dt)
    for kind in ("plain", "big"):
        c, tr, final = _trace(pair, kind)
        s = tr[1]
        assert s.x.dtype == dt and s.d.dtype == dt and s.t.dtype == dt and s.q.dtype == np.float64
        assert tr[2].x.dtype == np.float64 and tr[2].d.dtype == np.float64 and final.dtype == np.float64
        y0 = [int(v) for v in c.ups[0]]
        y1 = [int(v) for v in c.ups[1]]
        d_exact = [b - a for a, b in zip(y0, y1)]
        ws = _cols(c, "fixed:wrap-sub")
        assert sum(int(s.d[i]) != d_exact[i] for i in ws) >= 4 and any(int(s.d[i]) == d_exact[i] for i in ws)
        n1 = c.ns[1]
        wm = _cols(c, "fixed:wrap-mul")
        wrapped = [i for i in wm if int(s.d[i]) == d_exact[i] and int(s.t[i]) != n1 * d_exact[i]]
        if kind == "big":
            assert n1 > 1 and len(wrapped) >= 4
            # a double multiply instead: (double)n1 * (double)d / N differs from numpy's quotient
            assert any(float(n1) * float(d_exact[i]) / float(s.N) != float(s.q[i]) for i in wrapped)
        else:
            assert n1 == 1 and not wrapped
        allv = {int(v) for u in c.ups for v in u}
        assert {0, -1, int(ii.min), int(ii.max)} <= allv
        if kind == "big":
            assert any(st.N > 2 ** 53 and int(float(st.N)) != st.N for st in tr[1:])


def test_int64_beyond_f64():
    c, tr, _ = _trace(("i64", "f64"), "plain")
    inexact = lambda a: [int(x) for x in a if int(np.float64(x)) != int(x)]   # noqa: E731
    assert any(2 ** 53 < abs(x) < 2 ** 54 for x in inexact(c.ups[0])) and any(abs(x) > 2 ** 62 for x in inexact(c.ups[0]))
    later = [x for u in c.ups[2:] for x in inexact(u)]
    assert any(2 ** 53 < abs(x) < 2 ** 54 for x in later) and any(abs(x) > 2 ** 62 for x in later)
    late_only = [i for i in _cols(c, "fixed:i64-2^53") if abs(int(c.ups[0][i])) < 2 ** 53]
    assert late_only and all(int(np.float64(c.ups[2][i])) != int(c.ups[2][i]) for i in late_only)
    c32 = fa.special_columns(("i32", "f64"), 5)
    assert any(float(np.float32(int(x))) != int(x) for u in c32.ups for x in u if abs(int(x)) < 2 ** 25)
