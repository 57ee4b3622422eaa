"""The per-tensor path's plans (fedn_amd/mixed.py fold_plan / sub_plan) against numpy alone, and the case
builder of tests/mixed_cases.py against what its columns are for. No GPU.

The plans must refuse what numpy refuses, with numpy's exception class, and beyond that only the folds
``mixed_cases.refusal`` names — classes (a) to (d), each a TypeError raised before any launch. A fold outside
those classes that the plan refuses, or a class that grows, fails here.
"""
import numpy as np
import pytest

import mixed_cases as mc
from mixed_cases import NP_DT


def _plan_raises(xdt, ydt, n, N):
    from fedn_amd import mixed
    try:
        with mc.quiet():
            plan = mixed.fold_plan([((0,), NP_DT[xdt])], [((0,), NP_DT[ydt])], n, N)
    except Exception as e:  # noqa: BLE001
        return type(e), None
    return None, plan


def _counts(kind):
    n, N = mc.N_KINDS[kind]
    out = {"accepted": [], "numpy": [], "a": [], "b": [], "c": [], "d": []}
    for x, y in mc.PAIRS:
        want = mc.refusal(x, y, n, N)
        out["accepted" if want is None else want[1]].append((x, y))
    return out


@pytest.mark.parametrize("kind", list(mc.N_KINDS))
def test_fold_plan_refuses_what_the_rule_says(kind):
    """Over the 144 pairs: the plan raises exactly where numpy raises (numpy's class) or the rule's classes
    (a)-(d) say so (TypeError), and an accepted plan carries numpy's difference dtype, result dtype and shape."""
    n, N = mc.N_KINDS[kind]
    for x, y in mc.PAIRS:
        want = mc.refusal(x, y, n, N)
        got, plan = _plan_raises(x, y, n, N)
        assert got is (want[0] if want else None), f"{kind} ({x}, {y}): the plan gives {got}, the rule {want}"
        if want is not None and want[1] == "numpy":
            assert got is mc.numpy_raises(x, y, n, N)
        if plan is not None:
            with mc.quiet():
                d = np.subtract(np.empty(0, NP_DT[y]), np.empty(0, NP_DT[x]))
                r = mc.fold([np.empty(0, NP_DT[x])], [np.empty(0, NP_DT[y])], n, N)[0]
            assert plan == [(d.dtype, r.dtype, (0,))]


@pytest.mark.parametrize("kind", ["int", "float", "one"])
def test_counts_python_scalars(kind):
    """121 pairs accepted by numpy and the plan (every pair without bool), (bool, bool) refused by both with
    TypeError, bool on exactly one side refused by the plan alone: 22."""
    c = _counts(kind)
    assert sorted(c["accepted"]) == sorted((x, y) for x in mc.FOLDED for y in mc.FOLDED) and len(c["accepted"]) == 121
    assert c["numpy"] == [("bool", "bool")] and mc.numpy_raises("bool", "bool", *mc.N_KINDS[kind]) is TypeError
    assert len(c["a"]) == 22 and all((x == "bool") != (y == "bool") for x, y in c["a"])
    assert not c["b"] and not c["c"] and not c["d"]


def test_counts_numpy_float32():
    """np.float32(2.5) over np.float32(9.0): numpy accepts the same 121 pairs, but it is no weak scalar —
    times a float16, int8, int16, uint8 or uint16 difference the product is float32, which no arm computes
    (the half fold runs in half, the integer folds in float64). Those 17 pairs are class (d), refused before
    any launch and never folded in another dtype; the other 104 are numpy's bits."""
    n, N = mc.N_KINDS["npf32"]
    c = _counts("npf32")
    narrow = {"f16", "i8", "i16", "u8", "u16"}
    want_d = [(x, y) for x in mc.FOLDED for y in mc.FOLDED
              if np.subtract(np.empty(0, NP_DT[y]), np.empty(0, NP_DT[x])).dtype in [NP_DT[t] for t in narrow]]
    assert sorted(c["d"]) == sorted(want_d) and len(c["d"]) == 17
    assert len(c["accepted"]) == 104 and len(c["a"]) == 22 and c["numpy"] == [("bool", "bool")]
    assert not c["b"] and not c["c"]
    for x, y in c["d"]:                                  # numpy folds them, in float32
        assert mc.fold([np.ones(3, NP_DT[x])], [np.ones(3, NP_DT[y])], n, N)[0].dtype == np.float32


def test_counts_other_kinds():
    """The product-only set per remaining n kind, by class; it may shrink, never grow."""
    want = {"npi64": dict(accepted=84, numpy=1, a=22, b=17, c=0, d=20),
            "npi32": dict(accepted=84, numpy=1, a=22, b=17, c=0, d=20),
            "npi8": dict(accepted=112, numpy=1, a=22, b=9, c=0, d=0),
            "300": dict(accepted=119, numpy=7, a=18, b=0, c=0, d=0),
            "-5": dict(accepted=105, numpy=25, a=14, b=0, c=0, d=0),
            "2^53": dict(accepted=84, numpy=43, a=10, b=0, c=7, d=0)}
    for kind, w in want.items():
        c = _counts(kind)
        assert {k: len(v) for k, v in c.items()} == w, kind
    # class (b) is a numpy-integer n over a narrow difference; the int32 difference is folded (item 4)
    assert ("i32", "i32") in _counts("npi64")["accepted"] and ("i32", "i64") in _counts("npi64")["accepted"]
    assert all(NP_DT[x].itemsize < 4 or NP_DT[x].kind == "u" for x, y in _counts("npi64")["b"])
    assert mc.numpy_raises("i8", "i8", 300, 1234) is OverflowError and mc.numpy_raises("u8", "u16", -5, 11) is OverflowError
    assert mc.numpy_raises("i32", "i32", 1 << 53, 1 << 54) is OverflowError
    assert _counts("2^53")["c"] == [(x, y) for x, y in mc.PAIRS if "u64" in (x, y) and x[0] == "u" and y[0] == "u"]


def test_int_fold_kind_rule():
    """Which arm an integer difference takes, per n kind (mixed._int_fold_kind), against numpy's product dtype."""
    from fedn_amd import mixed
    for dt in ("i8", "i16", "i32", "i64", "u8", "u16", "u32", "u64"):
        d = NP_DT[dt]
        for kind, (n, N) in mc.N_KINDS.items():
            try:
                with mc.quiet():
                    p = np.multiply(n, np.empty(0, d)).dtype
            except OverflowError:
                with pytest.raises(OverflowError):
                    mixed._int_fold_kind(d, n)
                continue
            want = mc.refusal(dt, dt, n, N)
            if want is not None and want[1] in "bcd" and not (want[1] == "d" and p in (d, np.float64)):
                with pytest.raises(TypeError):
                    mixed._int_fold_kind(d, n)
                continue
            got = mixed._int_fold_kind(d, n)
            if p == np.float64 or (dt == "i32" and p == np.int64):
                assert got == "ifold", (dt, kind)
            else:
                assert p == d and got == ("int" if dt in ("i32", "i64") else "nfold"), (dt, kind)
    assert mixed._int_fold_kind(NP_DT["i32"], np.int64(3)) == "ifold"          # int64 product: exact in float64
    assert mixed._int_fold_kind(NP_DT["i32"], np.int32(3)) == "int" == mixed._int_fold_kind(NP_DT["i64"], np.int64(3))
    assert mixed._int_fold_kind(NP_DT["i64"], np.uint64(3)) == "ifold"         # numpy: float64
    with pytest.raises(TypeError):
        mixed._int_fold_kind(NP_DT["i32"], np.int64(1 << 31))                  # |n * d| could pass 2^62
    # the uniform pipelines hand such a first fold to the per-tensor path
    assert mixed.int_float_n([np.float32, np.int32], 0, np.int64(3)) and mixed.int_float_n([np.int64], 0, np.uint64(3))
    assert not mixed.int_float_n([np.int32, np.int64], 0, np.int32(3)) and not mixed.int_float_n([np.int64], 0, np.int64(3))
    assert not mixed.int_float_n([np.int32], 1, np.int64(3)) and not mixed.int_float_n([np.float32], 0, np.int64(3))


def test_sub_plan_counts():
    """subtract(next, old) = next*1.0 + old*(-1.0): 121 pairs accepted with numpy's dtype, every pair with a
    bool refused (23) although numpy computes it (bool * 1.0 is float64): no kernel takes bool."""
    from fedn_amd import mixed
    ok = bad = 0
    for y, o in mc.PAIRS:
        want = mc.subtract([np.empty(3, NP_DT[y])], [np.empty(1, NP_DT[o])])[0]
        try:
            plan = mixed.sub_plan([((3,), NP_DT[y])], [((1,), NP_DT[o])])
        except TypeError:
            assert "bool" in (y, o)
            bad += 1
            continue
        assert "bool" not in (y, o) and plan == [(want.dtype, (3,))]
        ok += 1
    assert (ok, bad) == (121, 23)
    assert len(mixed.sub_plan([((1,), NP_DT["f32"])] * 3, [((1,), NP_DT["f32"])] * 2)) == 2   # zip truncates
    with pytest.raises(ValueError):
        mixed.sub_plan([((5,), NP_DT["f32"])], [((4,), NP_DT["f32"])])


def test_broadcast_pairs_are_numpys():
    from fedn_amd import mixed
    f4 = NP_DT["f32"]
    for xs, ys in mc.BCAST + [mc.RANK9]:
        want = np.broadcast_shapes(xs, ys)
        assert mixed.fold_plan([(xs, f4)], [(ys, f4)], 37, 1234)[0][2] == tuple(want)
    assert max(len(s) for pair in mc.BCAST for s in pair) == 8 and len(mc.RANK9[0]) == 9
    with pytest.raises(ValueError):
        np.broadcast_shapes(*mc.BCAST_REFUSED)
    with pytest.raises(ValueError):
        mixed.fold_plan([(mc.BCAST_REFUSED[0], f4)], [(mc.BCAST_REFUSED[1], f4)], 37, 1234)


def _col(dt, name):
    cols = [(x, y) for nm, x, y in mc.edge_columns(dt) if nm == name]
    assert cols, (dt, name)
    d = NP_DT[dt]
    mk = lambda v: np.array(v, dtype=object).astype(d) if d.kind in "iu" else np.array(v, dtype=d)  # noqa: E731
    return cols, mk([c[0] for c in cols]), mk([c[1] for c in cols])


@pytest.mark.parametrize("dt", [d for d in mc.DTYPES if NP_DT[d].kind in "iu"])
def test_integer_columns_reach_their_lanes(dt):
    d = NP_DT[dt]
    ii = np.iinfo(d)
    vals = {v for _, x, y in mc.edge_columns(dt) for v in (x, y)}
    assert {int(ii.min), int(ii.max), 0, -1 if d.kind == "i" else int(ii.max) - 1} <= vals
    cols, x, y = _col(dt, "wrap-sub")
    with mc.quiet():
        assert all(int(b) - int(a) != int(v) for (a, b), v in zip(cols, np.subtract(y, x)))      # the difference wraps
    cols, x, y = _col(dt, "wrap-mul")
    with mc.quiet():
        dd = np.subtract(y, x)
        assert all(int(b) - int(a) == int(v) for (a, b), v in zip(cols, dd))                    # it does not wrap ...
        assert all(37 * int(v) != int(w) for v, w in zip(dd, np.multiply(37, dd)))               # ... its product does
    if dt == "i32":
        cols, x, y = _col(dt, "i32-2^30")
        with mc.quiet():
            dd = np.subtract(y, x)
            assert (np.abs(dd.astype(np.int64)) >= 1 << 30).all()
            p32, p64 = np.multiply(np.int32(3), dd), np.multiply(np.int64(3), dd)
        assert p32.dtype == np.int32 and p64.dtype == np.int64 and (p32.astype(np.int64) != p64).all()
        # the two products give different folds: the column separates them
        a = mc.fold([x], [y], np.int32(3), 11)[0]
        b = mc.fold([x], [y], np.int64(3), np.int64(11))[0]
        assert (a != b).all()
    if dt in ("i64", "u64"):
        cols, x, y = _col(dt, "2^53")
        for a, b in cols:                                   # one side at least is no double
            assert any(int(float(v)) != v for v in (a, b))
        assert any(abs(a) % 4 == 1 for a, _ in cols) and any(abs(a) % 4 == 3 for a, _ in cols)   # ties down and up
        assert any(x.astype(np.float64).astype(object) != x.astype(object))
    if dt == "u64":
        cols, x, y = _col(dt, "u64-high")
        assert all(max(a, b) >= 1 << 63 for a, b in cols)


@pytest.mark.parametrize("dt", ["f16", "f32", "f64"])
def test_float_columns_reach_their_lanes(dt):
    d = NP_DT[dt]
    fi = np.finfo(d)
    arr = np.array([v for _, x, y in mc.edge_columns(dt) for v in (x, y)], dtype=d)
    assert (arr == fi.max).any() and (arr == -fi.max).any() and (arr == fi.smallest_subnormal).any()
    assert np.isposinf(arr).any() and np.isneginf(arr).any()
    nan = arr[np.isnan(arr)]
    assert np.signbit(nan).any() and not np.signbit(nan).all()
    zero = arr[arr == 0]
    assert np.signbit(zero).any() and not np.signbit(zero).all()
    cols, x, y = _col(dt, "overflow-sub")
    with mc.quiet():
        assert np.isinf(np.subtract(y, x)).all()            # f16: 65504 against -65504
        cols, x, y = _col(dt, "overflow-mul")
        dd = np.subtract(y, x)
        assert np.isfinite(dd).all() and np.isinf(np.multiply(37, dd)).all()
        cols, x, y = _col(dt, "inf-inf")
        assert np.isnan(np.subtract(y, x)).all()
    if dt == "f16":
        assert (65504.0, -65504.0) in [(a, b) for _, a, b in mc.edge_columns(dt)]


def test_state_tensors_carry_the_columns():
    """Every tensor of a state starts with edge columns, the long ones with all of them; the same arguments
    give the same bytes (a reference computed once can be shared)."""
    for dt in mc.DTYPES:
        xs, ys = mc.state(dt, "model"), mc.state(dt, "update")
        assert [a.shape for a in xs] == mc.SHAPES == [a.shape for a in ys]
        assert all(a.dtype == NP_DT[dt] for a in xs + ys)
        ncol = len(mc.edge_columns(dt))
        for side, st in ((1, xs), (2, ys)):
            want = np.array([c[side] for c in mc.edge_columns(dt)], dtype=object if NP_DT[dt].kind in "iu" else NP_DT[dt])
            want = want.astype(NP_DT[dt])
            for a in st[4:]:
                flat = a.reshape(-1)[:ncol]
                assert sorted(flat.tobytes()) == sorted(want.tobytes())
        again = mc.state(dt, "model")
        assert all(a.tobytes() == b.tobytes() for a, b in zip(xs, again))
