"""Shared builders for the per-tensor path's tests (tests/test_mixed_cases_host.py on numpy alone,
tests/test_gpu_mixed_tensor.py on the device): the 12 tensor dtypes, the kinds of num_examples, the edge
columns per dtype, the tensor shapes of one state, the broadcast pairs, the numpy reference of a fold and the
rule that says which folds this build refuses although numpy performs them. Plain numpy and
oracle/numpy_ref.py; nothing here touches a GPU or imports fedn_amd.
"""
import contextlib
import math
import warnings

import numpy as np

from oracle import numpy_ref as ref

NP_DT = {"f16": np.dtype(np.float16), "f32": np.dtype(np.float32), "f64": np.dtype(np.float64),
         "i8": np.dtype(np.int8), "i16": np.dtype(np.int16), "i32": np.dtype(np.int32), "i64": np.dtype(np.int64),
         "u8": np.dtype(np.uint8), "u16": np.dtype(np.uint16), "u32": np.dtype(np.uint32), "u64": np.dtype(np.uint64),
         "bool": np.dtype(np.bool_)}
DTYPES = list(NP_DT)
FOLDED = [d for d in DTYPES if d != "bool"]                     # the 11 dtypes of the 121 accepted pairs
PAIRS = [(x, y) for x in DTYPES for y in DTYPES]                # (model, update): 144

# (n, N) by name. "int", "float", "one", "npf32": the four kinds no pair without bool is refused for unless
# numpy itself widens the fold (refusal(): class (d), np.float32 only).
N_KINDS = {
    "int": (37, 1234),
    "float": (2.5, 9.0),
    "one": (1.0, 4.0),
    "npf32": (np.float32(2.5), np.float32(9.0)),
    "npi64": (np.int64(3), np.int64(11)),
    "npi32": (np.int32(3), 11),
    "npi8": (np.int8(3), 11),
    "300": (300, 1234),                      # numpy's OverflowError for 8-bit differences
    "-5": (-5, 11),                          # numpy's OverflowError for unsigned differences
    "2^53": (1 << 53, 1 << 54),
}
PLAIN_KINDS = ["int", "float", "one", "npf32"]

# one state: a lone 0-d element, a lone element, a ragged strip, an empty tensor, more than one workgroup of the
# grid-stride kernels, a whole-plus-ragged tile of the fold; test_gpu_mixed_tensor.py adds the (4099,) tensor
# once more as a view one element past a 16-byte boundary
SHAPES = [(), (1,), (5,), (3, 0), (257,), (4099,)]

# (model shape, update shape)
BCAST = [((1,), (4099,)), ((4099,), (1,)), ((), (257,)), ((3, 1), (1, 4)), ((2, 1, 5), (3, 1)), ((0,), (1,)),
         ((3, 0), (1,)), ((2, 1, 2, 1, 2, 1, 2, 1), (1, 3, 1, 2, 1, 2, 1, 2))]       # the last: rank 8, kCastMaxDim
BCAST_REFUSED = ((5,), (4,))                                     # numpy's ValueError
RANK9 = ((2, 1, 2, 1, 2, 1, 2, 1, 2), (1, 2, 1, 2, 1, 2, 1, 2, 1))    # 9 non-mergeable dimensions: ops.cast's ValueError
BCAST_DTYPES = [("f32", "f32"), ("f32", "f64"), ("i8", "i16"), ("i64", "f32"), ("u8", "f16")]


@contextlib.contextmanager
def quiet():
    """numpy's overflow / invalid warnings off: the edge columns overflow on purpose."""
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        yield


def edge_columns(dt):
    """[(name, model value, update value)] for dtype ``dt``: the first elements of every tensor. The pairs
    are written for a model and an update of this one dtype (a wrap column wraps there); under another pair
    of dtypes they are extreme values all the same."""
    d = NP_DT[dt]
    if d.kind == "b":
        return [("bool", False, True), ("bool", True, True), ("bool", True, False), ("bool", False, False)]
    if d.kind == "f":
        fi = np.finfo(d)
        mx, sub = float(fi.max), float(fi.smallest_subnormal)
        inf, nan, nnan = math.inf, math.nan, math.copysign(math.nan, -1.0)
        return [("zero", 0.0, 0.0), ("zero", 0.0, -0.0), ("zero", -0.0, 0.0), ("zero", -0.0, -0.0),
                ("subnormal", 0.0, sub), ("subnormal", sub, -sub), ("subnormal", -sub, -sub),
                ("max", mx, mx), ("max", -mx, 1.0), ("overflow-sub", mx, -mx), ("overflow-sub", -mx, mx),
                ("overflow-mul", mx / 4, -mx / 4),
                ("inf", inf, 1.0), ("inf", 1.0, -inf), ("inf-inf", inf, inf), ("inf-inf", -inf, -inf), ("inf", inf, -inf),
                ("nan", nan, 1.0), ("nan", 1.0, nnan), ("nan", nnan, nan), ("nan", inf, nan),
                ("ordinary", 1.5, -3.0)]
    ii = np.iinfo(d)
    mn, mx, signed = int(ii.min), int(ii.max), d.kind == "i"
    cols = [("extreme", mn, mn), ("extreme", mx, mx), ("extreme", 0, 0), ("extreme", -1 if signed else mx - 1, 0),
            ("extreme", 0, -1 if signed else mx - 1),
            ("wrap-sub", mx, mn)]
    cols += [("wrap-sub", mn, mx), ("wrap-sub", -2, mx)] if signed else [("wrap-sub", 1, 0), ("wrap-sub", mx, mx - 1)]
    q = mx // 37 + 1                                             # |d| fits, 37 * d does not
    cols += [("wrap-mul", 0, q), ("wrap-mul", 5, q + 8)]
    if signed:
        cols += [("wrap-mul", 3, -q - 2)]
    if dt == "i32":                                              # 3 * d wraps int32, not int64
        cols += [("i32-2^30", 0, 1 << 30), ("i32-2^30", 5, -(1 << 30) - 7), ("i32-2^30", -(1 << 29), (1 << 29) + 1)]
    if dt in ("i64", "u64"):                                     # the one rounding to float64: ties both ways
        b = 1 << 53
        cols += [("2^53", b + 1, b + 1), ("2^53", b + 3, b + 3), ("2^53", b + 2, b + 3), ("2^53", b + 1, 7), ("2^53", 7, b + 1)]
        if signed:
            cols += [("2^53", -(b + 1), -(b + 1)), ("2^53", -(b + 3), b + 1), ("2^53", 9, -(b + 3))]
    if dt == "u64":
        h = 1 << 63
        cols += [("u64-high", h, h + 1), ("u64-high", mx, h), ("u64-high", h + 1025, 3), ("u64-high", 3, h + 1025)]
    return cols


def _random(rng, d, size):
    if d.kind == "b":
        return rng.integers(0, 2, size).astype(d)
    if d.kind == "f":
        return (rng.standard_normal(size) * 3.0).astype(d)
    ii = np.iinfo(d)
    wide = rng.integers(ii.min, ii.max, size, dtype=d, endpoint=True)
    small = rng.integers(max(ii.min, -100), min(ii.max, 100), size, dtype=d, endpoint=True)
    return np.where(rng.integers(0, 2, size).astype(bool), wide, small)


def tensor(dt, shape, side, seed=0, roll=0):
    """One tensor of dtype ``dt``: its first elements are the edge columns' ``side`` ("model" or "update")
    values, starting at column ``roll`` (so that the one-element tensors of a state meet different columns),
    the rest seeded random data."""
    d = NP_DT[dt]
    size = int(np.prod(shape, dtype=np.int64))
    rng = np.random.default_rng([seed, DTYPES.index(dt), side == "model", size])
    flat = _random(rng, d, size)
    cols = edge_columns(dt)
    vals = [c[1 if side == "model" else 2] for c in cols]
    vals = vals[roll % len(vals):] + vals[:roll % len(vals)]
    k = min(size, len(vals))
    with quiet():
        flat[:k] = np.array(vals[:k], dtype=object).astype(d) if d.kind in "iu" else np.array(vals[:k], dtype=d)
    return flat.reshape(shape)


def state(dt, side, seed=0, shapes=SHAPES):
    """The tensors of one state (``shapes``) in dtype ``dt``."""
    return [tensor(dt, s, side, seed, roll=3 * i) for i, s in enumerate(shapes)]


def fold(xs, ys, n, N):
    """The oracle's increment_average with numpy's warnings off; what numpy raises propagates."""
    with quiet():
        return ref.increment_average(xs, ys, n, N)


def subtract(ys, olds):
    with quiet():
        return ref.subtract(ys, olds)


def numpy_raises(xdt, ydt, n, N):
    """The exception class numpy's fold of a ``ydt`` update into an ``xdt`` model raises, or None."""
    try:
        fold([np.empty(0, NP_DT[xdt])], [np.empty(0, NP_DT[ydt])], n, N)
    except Exception as e:  # noqa: BLE001
        return type(e)
    return None


def refusal(xdt, ydt, n, N):
    """What folding a ``ydt`` update with (n, N) into an ``xdt`` model must do in this build, from numpy alone:
    None (numpy's bits), or (exception class, reason). numpy's own refusals keep numpy's class; on top of them
    this build refuses, with TypeError and before any launch,

    (a) bool on exactly one side (numpy folds it; no kernel takes bool);
    (b) a numpy-integer n whose product dtype with the difference is neither the difference dtype nor float64
        — except np.int64-like n on an int32 difference with |n| < 2^31, folded in float64 (exact: |n*d| < 2^62
        fits int64, and float64's one rounding of the exact product is the int64 -> float64 conversion's);
    (c) |n| >= 2^53 where the product wraps in a narrow / unsigned dtype (NFOLD takes n as a double);
    (d) a numpy-scalar n or N that widens numpy's product or quotient beyond the dtype the fold runs in (the
        difference's float dtype, float64 for an integer difference): np.float32(2.5) times a float16, int8,
        int16, uint8 or uint16 difference is float32; np.int64(3) times a float32 difference is float64."""
    e = numpy_raises(xdt, ydt, n, N)
    if e is not None:
        return e, "numpy"
    x, y = NP_DT[xdt], NP_DT[ydt]
    if (x.kind == "b") != (y.kind == "b"):
        return TypeError, "a"
    with quiet():
        d = np.subtract(np.empty(0, y), np.empty(0, x))
        p = np.multiply(n, d)
        t = np.true_divide(p, N)
    if d.dtype.kind in "iu":
        if p.dtype.kind == "f" and p.dtype != np.float64:
            return TypeError, "d"
        if isinstance(n, np.integer) and p.dtype not in (d.dtype, np.float64) and not (
                d.dtype == np.int32 and p.dtype == np.int64 and abs(int(n)) < 1 << 31):
            return TypeError, "b"
        if isinstance(n, (int, np.integer)) and p.dtype == d.dtype and d.dtype not in (np.int32, np.int64) \
                and abs(int(n)) >= 1 << 53:
            return TypeError, "c"
    arm = d.dtype if d.dtype.kind == "f" else np.dtype(np.float64)
    if t.dtype != arm:
        return TypeError, "d"
    return None


def inplace_pair(xdt, ydt, n, N):
    """Whether a fold of this pair may write the model's own storage: the difference is a float of the
    model's dtype (the continuation fold runs in place on an owned, contiguous model of the result shape)."""
    x, y = NP_DT[xdt], NP_DT[ydt]
    if x.kind != "f" or y.kind == "b":
        return False
    return np.subtract(np.empty(0, y), np.empty(0, x)).dtype == x and refusal(xdt, ydt, n, N) is None
