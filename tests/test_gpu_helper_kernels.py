"""The kernels behind the GPU helper — k_elementwise<TX,TY,TO>, k_axpby_half, k_ipow, k_abssum_partial,
k_colabssum, k_final_reduce, k_cast (fa_elementwise / fa_norm1 / fa_cast) — against numpy itself at the
values and sizes where such kernels go wrong: signed zeros, subnormals, infinities, NaN, products that
overflow or underflow, every float16 / bfloat16 bit pattern, every float32 -> float16 rounding
boundary, sizes on both sides of every grid cap (the second pass of each grid-stride loop), and `out`
aliasing an operand.

The reference is the expression numpyhelper runs (numpyhelper.py:34-142) on the same host arrays under
np.errstate(all="ignore"). Unless a test says otherwise the rule is: numpy's dtype and shape, NaN at
the same positions (payload and sign of a NaN are not defined by numpy), every other element equal bit
for bit, signed zeros included. np.power, never `**`: the operator takes sqrt / reciprocal shortcuts
the ufunc does not."""
import functools
import math

import numpy as np
import pytest
import torch

from fedn_amd import _abi, ops
from fedn_amd._abi import FedAggError
from fedn_amd.helper import Helper

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, F64, F16 = np.float32, np.float64, np.float16
EW_PASS = 8192 * 256          # elements one pass of fa_elementwise's capped grid covers
CAST_PASS = 16384 * 256       # the same for fa_cast
NORM_PASS = 1024 * 256        # k_abssum_partial's stride
COL_PASS = 4096 * 256         # k_colabssum's


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    _abi.load()
    yield
    # buffers of up to 34 MB were cached by this module: hand every block back, so the modules after
    # this one start from an empty pool (as test_gpu_krum does)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ---- plumbing -----------------------------------------------------------------------------------------

def _dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(DEV)      # the shared inputs are read-only


def _ew(op, odt, n, x=None, y=None, a=0.0, b=0.0):
    """ops.elementwise into a fresh flat device tensor of numpy dtype ``odt``; the result as numpy."""
    out = torch.empty(n, dtype=ops.torch_dtype(odt), device=DEV)
    ops.elementwise(op, out, None if x is None else _dev(x), None if y is None else _dev(y), a, b)
    return out.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype}{got.shape} vs {want.dtype}{want.shape}"
    if want.dtype.kind != "f":
        bad = np.flatnonzero(got.ravel() != want.ravel())
    else:
        gn, wn = np.isnan(got).ravel(), np.isnan(want).ravel()
        bad = np.flatnonzero((gn != wn) | (~wn & (_bits(got).ravel() != _bits(want).ravel())))
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {want.size} elements differ, first at {i}: "
                             f"got {got.ravel()[i]!r}, numpy {want.ravel()[i]!r}")


def _ord(a):
    """A monotone integer image of a float array (both zeros at 0): differences are ulp distances."""
    i = np.ascontiguousarray(a).view({4: np.int32, 8: np.int64}[a.dtype.itemsize]).astype(np.int64)
    lo = np.int64(np.iinfo({4: np.int32, 8: np.int64}[a.dtype.itemsize]).min)
    return np.where(i < 0, lo - i, i)


def _ulps(got, want):
    """Largest ulp distance and the number of differing elements (NaN positions must agree)."""
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), "NaN positions differ"
    d = np.abs(_ord(got)[~wn] - _ord(want)[~wn])
    return (int(d.max()) if d.size else 0), int(np.count_nonzero(d))


def _edge(dt):
    """One column of the values float kernels get wrong (about 30 per dtype)."""
    fi = np.finfo(dt)
    big = 64 if dt == F32 else 600
    one = dt(1)
    sub_min, sub_max = fi.smallest_subnormal, np.nextafter(fi.tiny, dt(0))
    v = [0.0, -0.0, np.inf, -np.inf, np.nan, sub_min, -sub_min, sub_max, -sub_max, fi.tiny, -fi.tiny, fi.max, -fi.max,
         1.0, -1.0, np.nextafter(one, dt(2)), np.nextafter(one, dt(0)), 3.0, dt(1) / dt(3), dt(2.0) ** big,
         -(dt(2.0) ** big), dt(2.0) ** -big, -(dt(2.0) ** -big)]
    return np.array(v, dtype=dt)


def _pairs(xdt, ydt):
    """All pairs of the two edge columns: x the column repeated, y the column tiled."""
    cx, cy = _edge(xdt), _edge(ydt)
    return np.repeat(cx, cy.size), np.tile(cy, cx.size)


@functools.lru_cache(maxsize=None)
def _wide(dt, n=65537, seed=11):
    """standard_normal scaled by 10**U(-30, 30) (f32) / 10**U(-200, 200) (f64): the bulk is ordinary
    values of every magnitude, products and quotients of two of them still overflow and underflow."""
    rng = np.random.default_rng(seed + np.dtype(dt).itemsize)
    span = 30 if dt == F32 else 200
    with np.errstate(all="ignore"):
        x = (rng.standard_normal(n) * 10.0 ** rng.uniform(-span, span, n)).astype(dt)
    x.setflags(write=False)
    return x


PAIRS = [(F32, F32), (F32, F64), (F64, F32), (F64, F64)]     # the reachable (x, y) of k_elementwise<TX,TY,TO>
AXPBY_AB = [(0.9, 0.1), (0.99, 1.0 - 0.99), (1.0, -1.0), (1e30, 1e30)]
MUL_A = [0.37, 1 - 0.9, 1e-30, 0.0, -0.0]
DIV_A = [3.1, 0.0, -0.0, math.inf, 1e38, 1e-40]
FILL_A = [1e-8, 0.25, 0.0, -0.0, math.inf]


def _pid(p):
    return "-".join(np.dtype(d).name for d in p) if isinstance(p, tuple) else np.dtype(p).name


# ---- A. k_elementwise at edge values ------------------------------------------------------------------

@pytest.mark.parametrize("ab", AXPBY_AB, ids=str)
@pytest.mark.parametrize("pair", PAIRS, ids=_pid)
def test_edge_axpby(pair, ab):
    """x*a + y*b on all pairs of the edge columns. Each product is rounded in its operand's dtype
    before the sum in the promoted one (x32*1e30 overflows to inf in float32 beside a float64 y);
    (1e30, 1e30) also gives inf - inf = NaN."""
    x, y = _pairs(*pair)
    a, b = ab
    with np.errstate(all="ignore"):
        want = x * a + y * b
    _same(_ew("axpby", want.dtype, x.size, x, y, a, b), want, f"axpby {_pid(pair)} {ab}")


@pytest.mark.parametrize("pair", PAIRS, ids=_pid)
def test_edge_mul_div_by_array(pair):
    """x*y and x/y on all pairs: 0*inf, inf/inf, 0/0, x/±0, overflow, underflow into subnormals."""
    x, y = _pairs(*pair)
    with np.errstate(all="ignore"):
        wm, wd = np.multiply(x, y), np.divide(x, y)
    _same(_ew("mul", wm.dtype, x.size, x, y), wm, f"mul {_pid(pair)}")
    _same(_ew("div", wd.dtype, x.size, x, y), wd, f"div {_pid(pair)}")


@pytest.mark.parametrize("dt", [F32, F64], ids=_pid)
def test_edge_scalar_and_unary(dt):
    """multiply / divide by a weak python scalar (cast to the array's dtype: float32(1e-40) is itself
    subnormal), sqrt (negatives NaN, -0 stays -0, subnormals correctly rounded), x*x, sign (±0 -> +0,
    NaN stays NaN) and ones(shape)*a on the edge column."""
    x = _edge(dt)
    with np.errstate(all="ignore"):
        for a in MUL_A:
            _same(_ew("mul", dt, x.size, x, a=a), np.multiply(x, a), f"{_pid(dt)} * {a!r}")
        for a in DIV_A:
            _same(_ew("div", dt, x.size, x, a=a), np.divide(x, a), f"{_pid(dt)} / {a!r}")
        _same(_ew("sqrt", dt, x.size, x), np.sqrt(x), f"sqrt {_pid(dt)}")
        # x*x is the IEEE product; np.power(x, 2) (what numpyhelper runs) equals it wherever numpy's
        # power is exact, which a libm's pow need not be: the product is the defined part
        _same(_ew("square", dt, x.size, x), np.multiply(x, x), f"square {_pid(dt)}")
        _same(_ew("sign", dt, x.size, x), np.sign(x), f"sign {_pid(dt)}")
        sg = _ew("sign", dt, x.size, x)
        assert not np.signbit(sg[:2]).any() and np.isnan(sg[4]), "sign(±0) = +0, sign(NaN) = NaN"
        for a in FILL_A:
            want = np.ones(x.shape) * a
            _same(_ew("fill", F64, x.size, a=a), want, f"ones * {a!r}")
            if dt == F32:            # the float32 instantiation stores the same value narrowed once
                _same(_ew("fill", F32, x.size, a=a), want.astype(F32), f"ones * {a!r} as float32")


@pytest.mark.parametrize("pair", PAIRS, ids=_pid)
def test_random_every_op(pair):
    """Every op once on 65 537 wide-range random values (more than one block, a ragged tail)."""
    xdt, ydt = pair
    x, y = _wide(xdt), _wide(ydt, seed=12)
    n = x.size
    with np.errstate(all="ignore"):
        for a, b in AXPBY_AB[:2]:
            want = x * a + y * b
            _same(_ew("axpby", want.dtype, n, x, y, a, b), want, f"axpby {_pid(pair)}")
        wm, wd = np.multiply(x, y), np.divide(x, y)
        _same(_ew("mul", wm.dtype, n, x, y), wm, f"mul {_pid(pair)}")
        _same(_ew("div", wd.dtype, n, x, y), wd, f"div {_pid(pair)}")
        if xdt == ydt:
            _same(_ew("mul", xdt, n, x, a=1 - 0.9), np.multiply(x, 1 - 0.9), "mul scalar")
            _same(_ew("div", xdt, n, x, a=3.1), np.divide(x, 3.1), "div scalar")
            _same(_ew("sqrt", xdt, n, x), np.sqrt(x), "sqrt")
            _same(_ew("square", xdt, n, x), np.multiply(x, x), "square")
            _same(_ew("sign", xdt, n, x), np.sign(x), "sign")
            _same(_ew("fill", F64, n, a=1e-8), np.ones(n) * 1e-8, "fill")


# ---- B. k_axpby_half ----------------------------------------------------------------------------------

def _half_edge():
    fi = np.finfo(F16)
    one = F16(1)
    sub_max = np.nextafter(fi.tiny, F16(0))
    v = [0.0, -0.0, np.inf, -np.inf, np.nan, fi.smallest_subnormal, -fi.smallest_subnormal, sub_max, -sub_max,
         fi.tiny, -fi.tiny, 65504.0, -65504.0, 1.0, -1.0, np.nextafter(one, F16(2)), np.nextafter(one, F16(0)),
         2.0 ** 12, 2.0 ** -12]
    return np.array(v, dtype=F16)


HALF_AB = [(0.9, 0.1), (1.0, -1.0), (1 + 2.0 ** -11 + 2.0 ** -30, 1.0), (65520.0, 1.0), (1e-8, 1.0)]


@pytest.mark.parametrize("ab", HALF_AB, ids=str)
def test_half_axpby(ab):
    """x16*a + y16*b in numpy's half loops: a and b become halves with ONE rounding from the python
    float (1 + 2^-11 + 2^-30 is 1.001 as a half, 1.0 had it passed through float32; 65520 is inf;
    1e-8 is 0), each product and the sum rounded to half. All pairs of the half edge column, then
    65 537 random bit patterns. (-0)*a + (-0)*b is -0: the kernel first gave +0 here.)"""
    a, b = ab
    assert F16(1 + 2.0 ** -11 + 2.0 ** -30) != F16(F32(1 + 2.0 ** -11 + 2.0 ** -30))
    c = _half_edge()
    rng = np.random.default_rng(21)
    rx, ry = (rng.integers(0, 1 << 16, 65537, dtype=np.uint16).view(F16) for _ in range(2))
    x = np.concatenate([np.repeat(c, c.size), rx])
    y = np.concatenate([np.tile(c, c.size), ry])
    with np.errstate(all="ignore"):
        want = x * a + y * b
    _same(_ew("axpby", F16, x.size, x, y, a, b), want, f"half axpby {ab}")


# ---- C. power -----------------------------------------------------------------------------------------

POW_A = [0.7, 1 / 3, -0.3, -1.5, 0.5, 3, 2.5]
NPOW = 500_000


@functools.lru_cache(maxsize=None)
def _loguniform(dt):
    rng = np.random.default_rng(31)
    lo, hi = (-37, 38) if dt == F32 else (-300, 300)
    x = (10.0 ** rng.uniform(lo, hi, NPOW)).astype(dt)
    x.setflags(write=False)
    return x


def _close(got, want, rtol, what):
    """The project's relative parity bound on data whose results reach the subnormal range: there the
    format's spacing is fixed (one subnormal step is up to 100 % of the value), so a result below the
    smallest normal may differ by one such step instead."""
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), what
    ok = ~wn
    g, w = got[ok].astype(F64), want[ok].astype(F64)
    inf = np.isinf(w)
    assert np.array_equal(g[inf], w[inf]), what
    err = np.abs(g[~inf] - w[~inf])
    bound = rtol * np.abs(w[~inf]) + float(np.finfo(want.dtype).smallest_subnormal)
    bad = np.flatnonzero(~(err <= bound))
    assert bad.size == 0, f"{what}: {bad.size} elements beyond {rtol}, first got {g[~inf][bad[0]]!r} numpy {w[~inf][bad[0]]!r}"


@pytest.mark.parametrize("a", POW_A, ids=lambda a: f"{a:.4g}")
def test_pow_f32_is_the_rounded_f64_power_of_the_f32_exponent(a):
    """np.power(x32, a) raises to float32(a) (a python float is a weak scalar). The contract is
    got = RN_f32(pow(x, f32(a))); the reference is the host's float64 power of the same operands
    rounded once. 500 000 x log-uniform over [1e-37, 1e38].

    (i) every element within 1 float32 ulp of the reference and (ii) at most 1e-4 of them different at
    all. Derived, not measured: the device's and the host's float64 pow are each within 2^-44 relative
    of exact (512 float64 ulps; OpenCL allows pow 16), so both round to the same float32 or to
    neighbours, and they differ only when a float32 rounding boundary lies inside a window 2^-43 wide
    against a spacing of 2^-24: at most 2^-19 per element.
    With the exponent left a double (before this test) 96 % of the elements differed, by up to 18 ulps;
    measured on an MI355X now: none of the 500 000 differs, for any of the exponents.
    Also numpy's own float32 power (its host SIMD library's) at the project's 1e-6."""
    x = _loguniform(F32)
    got = _ew("pow", F32, x.size, x, a=a)
    with np.errstate(all="ignore"):
        want = np.power(x.astype(F64), float(F32(a))).astype(F32)
        numpy32 = np.power(x, a)
    assert numpy32.dtype == got.dtype == F32
    worst, differ = _ulps(got, want)
    print(f"pow f32 a={a!r}: max {worst} ulp, {differ} of {x.size} differ from RN_f32(pow64(x, f32(a)))")
    assert worst <= 1, f"a={a!r}: {worst} ulps"
    assert differ <= 1e-4 * x.size, f"a={a!r}: {differ} elements differ"
    _close(got, numpy32, 1e-6, f"np.power(x32, {a!r})")


@pytest.mark.parametrize("a", POW_A, ids=lambda a: f"{a:.4g}")
def test_pow_f64_wide_range(a):
    """np.power(x64, a), 500 000 x log-uniform over [1e-300, 1e300], at the project's 1e-15 relative
    (numpy's float64 power is its host library's). Measured on an MI355X against numpy 2.2.6 on an
    x86-64 host: the largest distance is 1 float64 ulp for every exponent here, on 9 % (a = 3) to 26 %
    (a = 0.7, 1/3, 0.5) of the elements; the distance is printed."""
    x = _loguniform(F64)
    got = _ew("pow", F64, x.size, x, a=a)
    with np.errstate(all="ignore"):
        want = np.power(x, a)
    worst, differ = _ulps(got, want)
    print(f"pow f64 a={a!r}: max {worst} ulp, {differ} of {x.size} differ from np.power")
    _close(got, want, 1e-15, f"np.power(x64, {a!r})")


@pytest.mark.parametrize("dt", [F32, F64], ids=_pid)
def test_pow_special_cases(dt):
    """C99 Annex F on the edge column, bit for bit against np.power: pow(±0, -1) = ±inf, pow(-8, 0.5) =
    NaN, pow(NaN, 0) = 1, pow(-inf, 3) = -inf, pow(-1, inf) = 1, pow(-0, 0.5) = +0, ...

    Bit for bit wherever the standard fixes the result: x one of ±0, ±inf, NaN, ±1, or a one of ±0,
    ±inf, or a negative x with a non-integer a. The other elements (3 ** 0.5, (1 + ulp) ** -1.5, and
    x ** 1.0 too, which Annex F leaves to the library) are each library's to round: on the host this
    was written on np.power(float32(1 + 2^-23), 0.5) is 1.0000001 where the correctly rounded value is
    1.0, and on an MI355X the float64 pow(3.0, 1.0) is 2.9999999999999996. They are held to the
    project's parity bound against numpy, and for float32 to 1 ulp of the contract's reference."""
    x = np.concatenate([_edge(dt), np.array([-8.0, 8.0, 0.5, -0.5, 2.0, -2.0], dtype=dt)])
    rtol = 1e-6 if dt == F32 else 1e-15
    with np.errstate(all="ignore"):
        for a in (0.5, -1.5, 3.0, 0.0, 1.0, -1.0, math.inf):
            got, want = _ew("pow", dt, x.size, x, a=a), np.power(x, a)
            assert got.dtype == want.dtype
            fixed = (np.isnan(x) | np.isinf(x) | (x == 0) | (np.abs(x) == 1) | (a in (0.0, math.inf))
                     | ((x < 0) & (not float(a).is_integer())))
            assert fixed.sum() >= 7
            _same(got[fixed], want[fixed], f"{_pid(dt)} pow {a!r}, Annex F")
            _close(got[~fixed], want[~fixed], rtol, f"{_pid(dt)} pow {a!r}")
            if dt == F32:
                worst, _ = _ulps(got, np.power(x.astype(F64), float(F32(a))).astype(F32))
                assert worst <= 1, f"float32 pow {a!r}: {worst} ulps from RN_f32(pow64)"


def test_ipow_full_range():
    """k_ipow on full-range values: all 256 int8 values, int64 / uint64 at their extremes and random,
    exponents up to 2^53 (wrapping products; numpy's exponentiation by squaring)."""
    x8 = np.arange(-128, 128, dtype=np.int8)
    rng = np.random.default_rng(41)
    with np.errstate(all="ignore"):
        for e in (0, 1, 2, 3, 7, 63, 64):
            _same(_ew("ipow", np.int8, x8.size, x8, a=float(e)), np.power(x8, e), f"int8 ** {e}")
        for dt in (np.int64, np.uint64):
            info = np.iinfo(dt)
            x = rng.integers(info.min, info.max, 4099, dtype=dt, endpoint=True)
            x[:8] = [info.min, info.max, 0, 1, 2, 3, info.max - 1, info.min + 1]
            if dt == np.int64:
                x[8:11] = [-1, -2, -3]
            for e in (0, 1, 63, 64, 2 ** 53):
                _same(_ew("ipow", dt, x.size, x, a=float(e)), np.power(x, e), f"{np.dtype(dt)} ** {e}")


# ---- D. fa_norm1 --------------------------------------------------------------------------------------

def _norm(x, matrix):
    return float(ops.norm1(_dev(x), matrix).item())


@functools.lru_cache(maxsize=None)
def _norm_data(dt):
    rng = np.random.default_rng(51)
    n = 2 * (COL_PASS + 3)               # the widest matrix below; the vectors are its leading elements
    x = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)).astype(dt)
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("P", [1, 255, 256, 257, NORM_PASS - 1, NORM_PASS, NORM_PASS + 1, 2 * NORM_PASS + 5])
@pytest.mark.parametrize("dt", [F32, F64], ids=_pid)
def test_norm1_vector(dt, P):
    """sum |x| against math.fsum of the float64 values. Every term is non-negative, so the relative
    error is bounded by the adds on the longest path times 2^-53: ceil(P / 262144) in a lane's chain,
    8 tree levels, 4 + 8 in the final reduce (bound: ceil(P / 262144) + 24). Also np.linalg.norm(x, 1)
    (numpy sums float32 pairwise in float32) at the project's 1e-6."""
    x = _norm_data(dt)[:P]
    got = _norm(x, False)
    exact = math.fsum(np.abs(x.astype(F64)).tolist())
    bound = (-(-P // NORM_PASS) + 24) * 2.0 ** -53
    print(f"norm1 {_pid(dt)} P={P}: relative error {abs(got - exact) / exact:.3e}, bound {bound:.3e}")
    assert abs(got - exact) <= bound * exact
    assert abs(got - float(np.linalg.norm(x, 1))) <= 1e-6 * exact


@pytest.mark.parametrize("dt", [np.int8, np.int16, np.int32, np.uint8, np.uint16, np.uint32, np.int64, np.uint64],
                         ids=_pid)
def test_norm1_vector_integers(dt):
    """Integer tensors (numpy: astype(float) first): a total below 2^53 is exact. int64 / uint64 at
    their extremes: the int64 minimum and 2^64 - 1 are each converted with one rounding."""
    info = np.iinfo(dt)
    rng = np.random.default_rng(52)
    lo, hi = max(info.min, -(1 << 31)), min(info.max, (1 << 31) - 1)
    x = rng.integers(lo, hi, NORM_PASS + 1, endpoint=True).astype(dt)
    x[:2] = [lo, hi]
    total = sum(abs(int(v)) for v in x.tolist())
    assert total < 2 ** 53
    got = _norm(x, False)
    assert got == float(total) == float(np.linalg.norm(x, 1))
    if np.dtype(dt).itemsize == 8:
        for ext in ([info.min], [info.max], [info.min, info.max, 0, 1], [info.max] * 3 + [info.min + 1]):
            e = np.array(ext, dtype=dt)
            assert _norm(e, False) == float(np.linalg.norm(e, 1)), ext
        assert _norm(np.array([info.max], dtype=dt), False) == float(info.max)     # 2^63 / 2^64: one rounding


def _colsums_exact(x):
    a = np.abs(x.astype(F64))
    if a.shape[0] <= 2:                   # a sum of two doubles is correctly rounded: fsum's value
        return a.sum(axis=0)
    return np.array([math.fsum(a[:, c].tolist()) for c in range(a.shape[1])])


@pytest.mark.parametrize("shape", [(1, 1), (0, 5), (3, 1), (1, 257), (7, 256), (300, 5), (2, COL_PASS + 3)], ids=str)
@pytest.mark.parametrize("dt", [F32, F64], ids=_pid)
def test_norm1_matrix(dt, shape):
    """max over columns of sum |x| (rows in order, one lane per column): each column sum is within
    (rows + 1) * 2^-53 of its fsum, the max itself is exact. (0, 5) gives 0.0, as numpy."""
    rows, cols = shape
    x = _norm_data(dt)[:rows * cols].reshape(shape)
    got = _norm(x, True)
    want = float(np.linalg.norm(x, 1))
    if rows == 0:
        assert got == want == 0.0 and not math.copysign(1.0, got) < 0
        return
    exact = float(_colsums_exact(x).max())
    assert abs(got - exact) <= (rows + 1) * 2.0 ** -53 * exact
    assert abs(got - want) <= 1e-6 * exact
    # the same with the largest column last (the tail of the last pass over the columns)
    x = x.copy()
    x[0, -1] = -1e7
    got, exact = _norm(x, True), float(_colsums_exact(x[:, -1:]).max())
    assert exact > 9e6 and abs(got - exact) <= (rows + 1) * 2.0 ** -53 * exact
    assert abs(got - float(np.linalg.norm(x, 1))) <= 1e-6 * exact


@pytest.mark.parametrize("dt", [F32, F64], ids=_pid)
def test_norm1_specials(dt):
    """A NaN anywhere gives NaN — in a matrix it wins over a +inf column wherever either lies, the last
    column included; an inf without a NaN gives inf; all -0.0 gives +0."""
    n = NORM_PASS + 7
    v = np.ones(n, dtype=dt)
    for pos in (0, 255, 256, n - 1):
        w = v.copy()
        w[pos] = np.nan
        w[(pos + 300) % n] = np.inf
        assert math.isnan(_norm(w, False)), f"vector NaN at {pos}"
        w[pos] = -np.inf
        assert _norm(w, False) == math.inf, f"vector inf at {pos}"
    z = _norm(np.full(n, -0.0, dtype=dt), False)
    assert z == 0.0 and math.copysign(1.0, z) > 0
    rows, cols = 3, 601
    m = np.ones((rows, cols), dtype=dt)
    for nan_c, inf_c in ((0, 600), (600, 0), (5, 300), (300, 5), (599, 600), (256, 255), (600, 599)):
        w = m.copy()
        w[1, inf_c] = -np.inf
        assert _norm(w, True) == math.inf, f"matrix inf in column {inf_c}"
        w[2, nan_c] = np.nan
        assert math.isnan(_norm(w, True)), f"matrix NaN in column {nan_c}, inf in {inf_c}"
        assert math.isnan(float(np.linalg.norm(w, 1)))
    z = _norm(np.full((rows, cols), -0.0, dtype=dt), True)
    assert z == 0.0 and math.copysign(1.0, z) > 0


# ---- E. fa_cast ---------------------------------------------------------------------------------------

def _cast(x, odt, shape=None):
    """ops.cast of host array / tensor ``x`` into a fresh tensor of torch or numpy dtype ``odt``."""
    xt = x if isinstance(x, torch.Tensor) else _dev(x)
    tdt = odt if isinstance(odt, torch.dtype) else ops.torch_dtype(odt)
    out = torch.empty(tuple(xt.shape) if shape is None else shape, dtype=tdt, device=DEV)
    return ops.cast(out, xt.to(DEV)).cpu()


def test_cast_every_half_and_bfloat16():
    """All 65 536 bit patterns of float16 (against numpy) and of bfloat16 (against torch on the CPU), to
    float32 and to float64: the upcasts every f16 / bf16 kernel of the library is defined on."""
    pat = np.arange(1 << 16, dtype=np.uint16)
    h = pat.view(F16)
    for dst in (F32, F64):
        _same(_cast(h, dst).numpy(), h.astype(dst), f"float16 -> {_pid(dst)}")
    b = torch.from_numpy(pat.view(np.int16).copy()).view(torch.bfloat16)
    for dst in (torch.float32, torch.float64):
        _same(_cast(b, dst).numpy(), b.to(dst).numpy(), f"bfloat16 -> {dst}")


def test_cast_f32_to_f16_every_rounding_boundary():
    """For every finite half h: h, the midpoint to its successor (exact in float32) and one float32 ulp
    either side of each, both signs — every tie and both neighbours of every tie, the subnormal halves
    and the overflow threshold 65520 ± 1 ulp included — against astype(float16)."""
    pat = np.arange(0x7C00, dtype=np.uint16)                      # every non-negative finite half
    h = pat.view(F16).astype(F32)
    succ = np.append(h[1:], F32(65536.0))                         # past 65504 the next step would be 2^16
    mid = (h + succ) / F32(2)
    assert np.array_equal(mid.astype(F64), (h.astype(F64) + succ.astype(F64)) / 2) and mid[-1] == 65520.0
    up, down = F32(np.inf), F32(-np.inf)
    v = np.concatenate([h, np.nextafter(h, up), np.nextafter(h, down), mid, np.nextafter(mid, up), np.nextafter(mid, down)])
    fi = np.finfo(F32)
    spec = np.array([np.inf, np.nan, fi.max, fi.tiny, fi.smallest_subnormal, 2.0 ** -25, 2.0 ** -26, 65536.0, 1e38], dtype=F32)
    v = np.concatenate([v, -v, spec, -spec])
    with np.errstate(all="ignore"):
        want = v.astype(F16)
    _same(_cast(v, F16).numpy(), want, "float32 -> float16")


def test_cast_f64_to_f32_rounding_boundaries():
    """100 000 random float32 bit patterns v (and the subnormal / overflow edges): v, the midpoint to
    its successor (exact in float64) and the midpoint's two float64 neighbours, against astype."""
    rng = np.random.default_rng(61)
    pat = rng.integers(0, 0x7F800000, 100_000, dtype=np.uint32)            # finite, non-negative
    pat = np.concatenate([pat, np.array([0, 1, 2, 0x007FFFFE, 0x007FFFFF, 0x00800000, 0x7F7FFFFE, 0x7F7FFFFF], np.uint32)])
    v = pat.view(F32).astype(F64)
    nxt = (pat + np.uint32(1)).view(F32).astype(F64)
    nxt[np.isinf(nxt)] = 2.0 ** 128                                        # the step past the largest float32
    mid = (v + nxt) / 2
    x = np.concatenate([v, mid, np.nextafter(mid, np.inf), np.nextafter(mid, -np.inf)])
    x = np.concatenate([x, -x, np.array([np.inf, -np.inf, np.nan, 1e300, -1e300, 1e-300, 5e-324])])
    with np.errstate(all="ignore"):
        want = x.astype(F32)
    assert np.isinf(want).sum() > 4 and (np.abs(want[np.isfinite(want)]) < np.finfo(F32).tiny).sum() > 100
    _same(_cast(x, F32).numpy(), want, "float64 -> float32")


def test_cast_int64_uint64_to_f64_rounding():
    """2^k + {-1, 0, 1, 2, 3} for k = 53..63 and the extremes: one round to nearest even."""
    i64 = [s * ((1 << k) + d) for k in range(53, 63) for d in (-1, 0, 1, 2, 3) for s in (1, -1)]
    i64 += [(1 << 63) - 1, (1 << 63) - 2, -(1 << 63), -(1 << 63) + 1, (1 << 63) - 513, (1 << 63) - 512, 0, -1]
    u64 = [(1 << k) + d for k in range(53, 64) for d in (-1, 0, 1, 2, 3)]
    u64 += [(1 << 64) - 1, (1 << 64) - 2, (1 << 64) - 1025, (1 << 64) - 1024, (1 << 64) - 1023, 0]
    for vals, dt in ((i64, np.int64), (u64, np.uint64)):
        x = np.array(vals, dtype=dt)
        _same(_cast(x, F64).numpy(), x.astype(F64), f"{np.dtype(dt)} -> float64")


def test_cast_eight_dimensions():
    """Eight dimensions none of which merge — x of shape (2,1,2,1,2,1,2,1) into (2,3,2,3,2,3,2,3) — is
    the kernel's limit; a ninth raises ValueError."""
    rng = np.random.default_rng(62)
    x = rng.standard_normal((2, 1, 2, 1, 2, 1, 2, 1)).astype(F32)
    shape = (2, 3, 2, 3, 2, 3, 2, 3)
    _same(_cast(x, F64, shape).numpy(), np.broadcast_to(x, shape).astype(F64), "8-d broadcast")
    x9 = rng.standard_normal((2, 1, 2, 1, 2, 1, 2, 1, 2)).astype(F32)
    with pytest.raises(ValueError):
        _cast(x9, F64, shape + (2,))


def test_cast_past_the_grid_cap():
    """P = 4 194 304 + 259 = 17 * 246 739, past the 16384-block grid: contiguous uint8 -> float32 and a
    row broadcast (1, c) -> (r, c) float32 -> float64, every element."""
    P = CAST_PASS + 259
    rng = np.random.default_rng(63)
    u = rng.integers(0, 256, P, dtype=np.uint8)
    _same(_cast(u, F32).numpy(), u.astype(F32), "uint8 -> float32")
    r, c = 17, 246_739
    assert r * c == P
    row = rng.standard_normal((1, c)).astype(F32)
    _same(_cast(row, F64, (r, c)).numpy(), np.broadcast_to(row, (r, c)).astype(F64), "row broadcast")


# ---- F. past the grid cap, in place, refusals ---------------------------------------------------------

PMAX = 2 * EW_PASS + 257


@functools.lru_cache(maxsize=None)
def _big(dt):
    """Two rows of PMAX values of ``dt`` (ordinary floats; integers over their whole range)."""
    rng = np.random.default_rng(71)
    if np.dtype(dt).kind == "f":
        a = rng.standard_normal((2, PMAX), dtype=F64 if dt == F64 else F32).astype(dt)
    else:
        info = np.iinfo(dt)
        a = rng.integers(info.min, info.max, (2, PMAX), dtype=dt, endpoint=True)
    a.setflags(write=False)
    return a


def _int_fold(x, y, n, N):
    with np.errstate(all="ignore"):
        return np.add(x, np.true_divide(np.multiply(n, np.subtract(y, x)), N))


@pytest.mark.parametrize("P", [EW_PASS - 1, EW_PASS, EW_PASS + 1, PMAX])
def test_second_pass_of_every_grid_stride_loop(P):
    """One launch of every fa_elementwise kernel on each side of the 8192-block grid cap — exactly one
    pass less one, one pass, one pass plus one, two passes and a tail — every element against numpy:
    a wrong stride, a dropped tail or a 32-bit index shows here. (k_elementwise<f32,f32,f64> is not
    reachable: float32 operands give a float32 result, see test_refusals.)"""
    with np.errstate(all="ignore"):
        for xdt, ydt in PAIRS:
            x, y = _big(xdt)[0, :P], _big(ydt)[1, :P]
            want = x * 0.9 + y * 0.1
            _same(_ew("axpby", want.dtype, P, x, y, 0.9, 0.1), want, f"axpby {_pid((xdt, ydt))} P={P}")
        x, y = _big(F16)[0, :P], _big(F16)[1, :P]
        _same(_ew("axpby", F16, P, x, y, 0.9, 0.1), x * 0.9 + y * 0.1, f"half axpby P={P}")
        for dt in (np.int8, np.int64):
            x = _big(dt)[0, :P]
            _same(_ew("ipow", dt, P, x, a=3.0), np.power(x, 3), f"{np.dtype(dt)} ** 3 P={P}")
    x, y = _big(np.int16)[0, :P], _big(np.int16)[1, :P]
    _same(_ew("ifold", F64, P, x, y, 2.5, 7.25), _int_fold(x, y, 2.5, 7.25), f"ifold int16 P={P}")
    x, y = _big(np.uint32)[0, :P], _big(np.uint32)[1, :P]
    _same(_ew("nfold", F64, P, x, y, 3.0, 7.0), _int_fold(x, y, 3, 7), f"nfold uint32 P={P}")


@pytest.mark.parametrize("dt", [F32, F64], ids=_pid)
def test_in_place(dt):
    """out may be exactly x or exactly y (serverfunctions' `acc /= total_weight` passes out = x): at
    one pass plus one element each in-place result equals the out-of-place one and numpy's."""
    P = EW_PASS + 1
    x, y = _big(dt)[0, :P], _big(dt)[1, :P]
    tdt = ops.torch_dtype(dt)
    with np.errstate(all="ignore"):
        want_div, want_ax = np.divide(x, 3.1), x * 0.9 + y * 0.1
    xd = _dev(x)
    assert ops.elementwise("div", xd, x=xd, a=3.1) is xd
    _same(xd.cpu().numpy(), want_div, "div in place")
    _same(_ew("div", dt, P, x, a=3.1), want_div, "div out of place")
    out = torch.empty(P, dtype=tdt, device=DEV)
    ops.elementwise("axpby", out, _dev(x), _dev(y), 0.9, 0.1)
    _same(out.cpu().numpy(), want_ax, "axpby out of place")
    xd, yd = _dev(x), _dev(y)
    ops.elementwise("axpby", xd, xd, yd, 0.9, 0.1)
    assert torch.equal(xd.view(torch.uint8), out.view(torch.uint8)), "axpby with out is x"
    _same(yd.cpu().numpy(), y, "y untouched")
    xd = _dev(x)
    ops.elementwise("axpby", yd, xd, yd, 0.9, 0.1)
    assert torch.equal(yd.view(torch.uint8), out.view(torch.uint8)), "axpby with out is y"
    _same(xd.cpu().numpy(), x, "x untouched")


def test_refusals(monkeypatch):
    """Calls fa_elementwise refuses before it launches anything (valid buffers throughout): the status
    is the documented one and `out` keeps its sentinel."""
    n = 1000
    x32, y32 = _dev(_wide(F32)[:n]), _dev(_wide(F32, seed=12)[:n])
    i32 = _dev(np.arange(n, dtype=np.int32))
    monkeypatch.setitem(ops._EW, "no-such-op", 99)
    cases = [("no-such-op", torch.float32, x32, y32, 0.0, _abi.FA_EINVAL),
             ("axpby", torch.float32, x32, None, 1.0, _abi.FA_EINVAL),
             ("axpby", torch.float64, x32, y32, 1.0, _abi.FA_EDTYPE),      # float32 + float32 is float32 in numpy
             ("mul", torch.float64, x32, None, 0.5, _abi.FA_EDTYPE),
             ("sqrt", torch.float32, x32.double(), None, 0.0, _abi.FA_EDTYPE),
             ("ipow", torch.int32, i32, None, -1.0, _abi.FA_EINVAL),
             ("ipow", torch.int32, i32, None, 1.5, _abi.FA_EINVAL),
             ("ipow", torch.int64, i32, None, 2.0, _abi.FA_EDTYPE)]
    for op, odt, x, y, a, status in cases:
        out = torch.full((n,), 7, dtype=odt, device=DEV)
        with pytest.raises(FedAggError) as e:
            ops.elementwise(op, out, x, y, a, 1.0)
        assert e.value.status == status, (op, odt, str(e.value))
        assert bool((out == 7).all()), f"{op}: out written by a refused call"


# ---- the helper's routing onto these kernels ----------------------------------------------------------

def test_helper_routes_to_the_same_kernels():
    """fednamdhelper reaches the kernels above with numpy's operands: power on float32 rounds the
    exponent (in fa_elementwise, so the helper gets it too), add on float32 + float64 runs the mixed
    instantiation, divide by a python scalar the weak-scalar one, norm picks vector or matrix."""
    h = Helper()
    x = _loguniform(F32)[:4099]
    got = h.power([x], 0.7)[0]
    assert np.array_equal(_bits(got), _bits(_ew("pow", F32, x.size, x, a=0.7)))
    with np.errstate(all="ignore"):
        worst, _ = _ulps(got, np.power(x.astype(F64), float(F32(0.7))).astype(F32))
        assert worst <= 1
        ex, ey = _pairs(F32, F64)
        _same(h.add([ex], [ey], 1e30, 1e30)[0], ex * 1e30 + ey * 1e30, "Helper.add float32 + float64")
        _same(h.subtract([ex], [ey], 0.9, 0.1)[0], ex * 0.9 + ey * -0.1, "Helper.subtract")
        e = _edge(F32)
        _same(h.divide([e], [1e-40])[0], np.divide(e, 1e-40), "Helper.divide by a python scalar")
        _same(h.sign([e])[0], np.sign(e), "Helper.sign")
    m = _norm_data(F32)[:300 * 5].reshape(300, 5)
    v = _norm_data(F64)[:257]
    want = 0.0
    for t in (m, v):
        want += np.linalg.norm(t, 1)
    got = h.norm([m, v])
    assert type(got) is type(want) and abs(float(got) - float(want)) <= 1e-6 * float(want)
