"""The builders of tests/fedopt_cases.py reach the lanes they were written for — shown on the oracle
alone, so that a wrong bound in a builder cannot silently remove a scenario from
tests/test_gpu_fedopt_kernels.py. The fold's intermediates are recomputed in numpy (t = n*(d - pg) per
step, the quotient, v - pg^2, pg^2 in half) and each lane of the kernels' special-value code is asserted
to be hit by at least one column."""
import numpy as np
import pytest

import fedopt_cases as fc

K = 5


def _trace(pair, kind="float", k=K):
    c = fc.special_columns(pair, k, "yogi", fc.params("yogi", "odd"), ns_kind=kind)
    return c, fc.fold_trace(c.old, c.ups, c.ns)


def test_pairs_are_the_dispatch():
    assert len(fc.PAIRS) == 17 and len(set(fc.PAIRS)) == 17
    assert sum(fc.is_int(u) for u, _ in fc.PAIRS) == 6
    assert {fc.pg_dtype(p) for p in fc.PAIRS} == {"f16", "f32", "f64"}
    assert [p for p in fc.PAIRS if fc.pg_dtype(p) == "f16"] == [("f16", "f16")]


def test_bf16_values_have_zero_low_bits():
    a = fc.cast("bf16", [1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 3.3e38, np.nan, -np.nan, 2.0 ** -133, 1e-45])
    assert not (a.view(np.uint32) & 0xFFFF).any()
    assert a[1] == 1.0 and a[2] == 1.0 + 2.0 ** -6          # ties to even, both ways
    assert np.isnan(a[4]) and np.isnan(a[5]) and np.signbit(a[5]) and not np.signbit(a[4])


@pytest.mark.parametrize("pair", [("f32", "f32"), ("bf16", "f32"), ("f32", "f16")], ids="-".join)
def test_f32_tiny_lane(pair):
    """0 < |t| < 2^-98 with a subnormal exact quotient, and t on both sides of the bound and on it."""
    c, tr = _trace(pair)
    hit = above = False
    for s in tr[1:]:
        assert s.t.dtype == np.float32
        a = np.abs(s.t.astype(np.float64))
        N = float(np.float32(s.N))
        assert abs(N) < 2.0 ** 28                            # the reciprocal lane (r != 0)
        hit |= bool(((a > 0) & (a < 2.0 ** -98) & (a / N < 2.0 ** -126)).any())
        above |= bool(((a > 2.0 ** -98) & (a < 2.0 ** -97)).any())
    assert hit and above
    fixed = [i for i, n in enumerate(c.names) if n == "fixed:tiny"]
    t1 = np.abs(tr[1].t[fixed].astype(np.float64))
    assert (t1 == 2.0 ** -98).any() and (t1 > 2.0 ** -98).any() and ((t1 < 2.0 ** -98) & (t1 > 0)).any()


@pytest.mark.parametrize("pair", [("f32", "f32"), ("f32", "f16")], ids="-".join)
def test_f32_tie_lane(pair):
    """Quotients that are ties between two f32 subnormals and that the reciprocal rounds the other way:
    without the redo of 0 < |t| < 2^-98 every one of these columns is wrong."""
    c, tr = _trace(pair, "big")
    tie = [i for i, n in enumerate(c.names) if n == "fixed:tie"]
    s = tr[1]
    assert len(tie) >= 16 and float(np.float32(s.N)) == 98.0
    t = s.t[tie]
    a = np.abs(t.astype(np.float64))
    assert ((a > 0) & (a < 2.0 ** -98)).all()
    fast = (t.astype(np.float64) * (1.0 / 98.0)).astype(np.float32)
    assert (fast != s.q[tie]).all() and (np.abs(s.q[tie]) < 2.0 ** -126).all()


@pytest.mark.parametrize("pair", [("f64", "f64"), ("f64", "f32"), ("f64", "f16")], ids="-".join)
def test_f64_near_midpoint_lane(pair):
    """t / N1 next to a rounding midpoint, inside CF64::div's shortcut range; t * RN(1/N1) alone is wrong
    for some of them."""
    from fractions import Fraction
    c, tr = _trace(pair, "float")
    mid = [i for i, n in enumerate(c.names) if n == "fixed:midpoint"]
    s = tr[1]
    assert len(mid) >= 4 and type(s.N) is float
    wrong = 0
    for t, q in zip(s.t[mid], s.q[mid]):
        assert 2.0 ** -600 <= abs(t) <= 2.0 ** 600 and q == t / s.N
        ulp = Fraction(float(np.spacing(abs(q))))
        z = Fraction(float(t)) / Fraction(s.N)
        assert abs(abs(z - Fraction(float(q))) - ulp / 2) < ulp * Fraction(1, 2 ** 50)
        wrong += float(t) * (1.0 / s.N) != q
    assert wrong


@pytest.mark.parametrize("pair", [("f64", "f64"), ("f64", "f32"), ("f64", "f16")], ids="-".join)
def test_f64_tiny_and_huge_lanes(pair):
    c, tr = _trace(pair)
    tiny = huge = over = False
    for s in tr[1:]:
        assert s.t.dtype == np.float64
        a = np.abs(s.t)
        tiny |= bool(((a > 0) & (a < 2.0 ** -600)).any())
        huge |= bool(((a > 2.0 ** 600) & np.isfinite(a)).any())
        over |= bool(np.isinf(a).any())
    assert tiny and huge and over
    fixed = [i for i, n in enumerate(c.names) if n == "fixed:tiny"]
    t1 = np.abs(tr[1].t[fixed])
    assert (t1 == 2.0 ** -600).any() and (t1 > 2.0 ** -600).any() and ((t1 < 2.0 ** -600) & (t1 > 0)).any()


@pytest.mark.parametrize("pair", fc.PAIRS, ids="-".join)
def test_zero_and_nonfinite_pseudo_gradients(pair):
    """pg of +0 and -0 (float pairs), NaN and inf lanes, in every pair."""
    c, tr = _trace(pair)
    pg = tr[-1].pg
    assert pg.dtype == fc.NP_DT[fc.pg_dtype(pair)]
    z = pg == 0
    assert (z & ~np.signbit(pg)).any()
    if not fc.is_int(pair[0]):
        p0 = tr[0].pg                  # a fold step turns -0 into +0 (x + q with x = -0 needs q = -0,
        assert ((p0 == 0) & np.signbit(p0)).any()      # i.e. d = -0 and pg = +0), so -0 is client 0's
        assert np.isnan(pg).any() and np.isinf(p0).any()   # d - pg of two infinities is NaN from client 1 on
        t = np.concatenate([s.t for s in tr[1:]])
        assert ((t == 0) & np.signbit(t)).any() and ((t == 0) & ~np.signbit(t)).any() and np.isnan(t).any()


@pytest.mark.parametrize("pair", fc.PAIRS, ids="-".join)
def test_yogi_sign_takes_every_value(pair):
    c, tr = _trace(pair)
    with np.errstate(all="ignore"):
        sq = np.power(tr[-1].pg, 2)
        d = c.v + sq * -1.0
        s = np.sign(d)
    assert sq.dtype == tr[-1].pg.dtype
    for want in (-1.0, 0.0, 1.0):
        assert (s == want).any(), want
    assert np.isnan(s).any()
    yz = [i for i, n in enumerate(c.names) if n == "yogi-zero"]
    assert (d[yz] == 0).any() and (d[yz] > 0).any() and (d[yz] < 0).any()


@pytest.mark.parametrize("kind", ["float", "big"])
def test_half_lanes(kind):
    c, tr = _trace(("f16", "f16"), kind)
    pg = tr[-1].pg
    assert pg.dtype == np.float16
    if kind == "float":
        with np.errstate(all="ignore"):
            sq = np.power(pg, 2)
        nz = (pg != 0) & np.isfinite(pg)
        assert (np.isinf(sq) & nz).any()
        assert ((sq > 0) & (sq < 2.0 ** -14)).any()
        assert ((sq == 0) & nz).any()
        nt = [i for i, n in enumerate(c.names) if n == "half-nt"]      # finite d and pg, n*t overflows half
        assert any(np.isinf(s.t[nt][np.isfinite(p.pg[nt])]).any() for p, s in zip(tr, tr[1:]))
        assert any(float(np.float16(s.N)) != s.N and s.N > 2048 for s in tr)
    else:
        with np.errstate(all="ignore"):
            assert any(np.isinf(np.float16(s.N)) for s in tr)
            assert any(np.isinf(np.asarray(n).astype(np.float16)) for n in c.ns)


def test_scalars():
    f = fc.client_ns(K, "float")
    assert 2.75 in f and any(type(n) is float for n in f) and all(type(n) is float for n in fc.totals(f))
    b = fc.totals(fc.client_ns(K, "big"))
    assert any(t > 2 ** 24 and float(np.float32(t)) != t for t in b)
    assert any(n >= 2 ** 28 for n in fc.client_ns(K, "big")) and b[-1] >= 2 ** 28
    assert all(abs(float(np.float32(t))) < 2.0 ** 28 for t in b[:4])
    for kind in ("default", "odd"):
        p = fc.ref.validate_parameters(fc.params("adam", kind))
        for key in ("beta1", "beta2", "learning_rate"):
            assert float(np.float32(p[key])) != p[key] and float(np.float16(p[key])) != p[key]
        assert p["beta1"] != p["beta2"]
    assert fc.params("adam", "odd")["tau"] == 0.0 and fc.params("adagrad", "odd")["tau"] == 0.0


@pytest.mark.parametrize("pair", [p for p in fc.PAIRS if p[0] == "i64"], ids="-".join)
def test_int64_operands_beyond_f64(pair):
    c, _ = _trace(pair)
    arrs = c.ups + ([c.old] if pair[1] == "i64" else [])
    inexact = [int(x) for a in arrs for x in a if int(np.float64(x)) != int(x)]
    assert any(2 ** 53 < abs(x) < 2 ** 54 for x in inexact) and any(abs(x) > 2 ** 62 for x in inexact)
    if pair[1] == "i64":          # a difference that wraps as int64 and does not as float64
        with np.errstate(all="ignore"):
            wrap = (c.ups[0] - c.old).astype(np.float64) != c.ups[0].astype(np.float64) - c.old.astype(np.float64)
        assert wrap.any()


@pytest.mark.parametrize("pair", [p for p in fc.PAIRS if fc.is_int(p[0]) and p[1] == "f32"], ids="-".join)
def test_int_updates_f32_cannot_hold(pair):
    c, _ = _trace(pair)
    assert any(float(np.float32(int(x))) != int(x) for a in c.ups for x in a if abs(int(x)) < 2 ** 25)


@pytest.mark.parametrize("opt", fc.OPTS)
@pytest.mark.parametrize("pair", fc.PAIRS, ids="-".join)
def test_reference_is_never_none(pair, opt):
    """Every pair x optimizer x parameter set x ns list, K = 2, 5 and 65, with m of every dtype, v absent, f64 and f32,
    and the f32-state mode: the oracle returns a model (reference() asserts it) of the expected dtypes."""
    for k, kind, pk in ((2, "float", "odd"), (2, "big", "default"), (5, "float", "odd"), (5, "big", "default"),
                        (65, "float", "default"), (65, "big", "odd")):
        p = fc.params(opt, pk)
        for m_dt in (None, "f16", "f32", "f64"):
            c = fc.special_columns(pair, k, opt, p, ns_kind=kind, m_dt=m_dt)
            assert len({len(c.old), len(c.m), len(c.v)} | {len(x) for x in c.ups}) == 1 and len(c.ups) == k
            for v in (None, c.v, fc.as_f32(c.v)):
                m = None if m_dt is None else c.m
                out, mo, vo = fc.reference(pair, c.old, c.ups, c.ns, m, v, p)
                assert out.dtype == np.float64 and vo.dtype == np.float64
                assert mo.dtype == fc.NP_DT[fc.m_out_dtype(pair, m_dt)]
            if pair[1] == "f32":
                out, mo, vo = fc.reference(pair, c.old, c.ups, c.ns, c.m if m_dt else None,
                                           fc.as_f32(c.v), p, f32state=True)
                assert out.dtype == mo.dtype == vo.dtype == np.float32
