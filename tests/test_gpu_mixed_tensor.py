"""The per-tensor path (fedn_amd/mixed.py: TensorFedAvg, TensorFedOpt) against numpy, bit for bit: values,
dtype, shape, NaN by position. numpy's result is the definition, so no comparison here has a tolerance.

A: one fold at every dtype pair, n kind and ownership; B: folds whose dtypes escalate; C: broadcasting and zip
truncation; D: refusals; E: TensorFedOpt's pseudo-gradient and server step; F: rounds that enter the path
through the plug-ins and the pipelines. Cases, edge columns and the refusal rule: tests/mixed_cases.py. After
every call each input tensor is bitwise what was uploaded, and a refused call has launched nothing.
"""
import numpy as np
import pytest
import torch

import mixed_cases as mc
from golden_io import assert_lists_identical
from mixed_cases import NP_DT
from oracle import numpy_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OFFSET = 5                                    # SHAPES' (4099,) tensor, once more one element past a 16-byte boundary
PARAMS = {"learning_rate": 0.01, "beta1": 0.9, "beta2": 0.99, "tau": 1e-3}


def _stream():
    return torch.cuda.current_stream(DEV)


def _up(arrays, offset=False):
    """Host arrays -> device tensors: mixed.upload, or plain tensors where a bool tensor is among them (upload
    refuses bool). ``offset``: the last tensor becomes a view one element into a longer allocation."""
    from fedn_amd import mixed
    if any(a.dtype == np.bool_ or not a.flags.c_contiguous for a in arrays):
        out = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]
    else:
        out = mixed.upload(arrays, DEV, _stream())
    if offset:
        t = out[-1]
        big = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
        big[1:].copy_(t)
        out[-1] = big[1:]
        assert out[-1].data_ptr() % 16 == t.element_size() % 16 and out[-1].is_contiguous()
    return out


def _host(tensors):
    torch.cuda.synchronize(DEV)
    return [t.cpu().numpy() for t in tensors]


def _bits(tensors):
    return [a.tobytes() for a in _host(tensors)]


def _state(dt, side, seed=0):
    """Host arrays of the seven-tensor state: mixed_cases.SHAPES and the (4099,) tensor again (the offset view)."""
    return mc.state(dt, side, seed) + [mc.tensor(dt, mc.SHAPES[OFFSET], side, seed + 1, roll=7)]


@pytest.fixture
def launches(monkeypatch):
    """Counts every launching entry point the per-tensor path uses."""
    from fedn_amd import ops
    count = {"n": 0}

    def wrap(name):
        fn = getattr(ops, name)

        def inner(*a, **k):
            count["n"] += 1
            return fn(*a, **k)
        monkeypatch.setattr(ops, name, inner)
    for name in ("cast", "elementwise", "fedavg_fold", "fedopt_step"):
        wrap(name)
    return count


def _refused(fa, call, exc, launches, what):
    """``call`` raises ``exc`` before any launch and leaves the TensorFedAvg ``fa`` untouched."""
    from fedn_amd import ops
    before, objs, hold, ran, last = _bits(fa.x), list(fa.x), len(fa.hold), launches["n"], ops.last_kernel()
    with pytest.raises(exc):
        with mc.quiet():
            call()
    assert launches["n"] == ran and ops.last_kernel() == last, f"{what}: launched before refusing"
    assert len(fa.x) == len(objs) and all(a is b for a, b in zip(fa.x, objs)), f"{what}: state replaced"
    assert _bits(fa.x) == before, f"{what}: state written"
    assert len(fa.hold) == hold, f"{what}: a refused update is kept alive"


# ---- A. TensorFedAvg.fold over the dtype grid ----------------------------------------------------------------

@pytest.mark.parametrize("owned", [True, False], ids=["owned", "views"])
@pytest.mark.parametrize("xdt", mc.FOLDED)
def test_fold_dtype_grid(xdt, owned, launches):
    """One fold of the seven-tensor state per (update dtype, n kind): numpy's bits or the rule's refusal. With
    views (owned=False: a staged update) the starting tensors stay bitwise intact; an owned model of an
    in-place pair is folded in its own storage."""
    from fedn_amd import mixed
    xs = _state(xdt, "model")
    for ydt in mc.FOLDED:
        ys = _state(ydt, "update")
        dy = _up(ys, offset=True)
        ybits = [a.tobytes() for a in ys]
        for kind, (n, N) in mc.N_KINDS.items():
            what = f"model {xdt} update {ydt} n {kind} owned {owned}"
            dx = _up(xs, offset=True)
            fa = mixed.TensorFedAvg(DEV, _stream(), dx, owned=owned)
            want = mc.refusal(xdt, ydt, n, N)
            if want is not None:
                _refused(fa, lambda: fa.fold(dy, n, N), want[0], launches, what)
                continue
            with mc.quiet():
                fa.fold(dy, n, N)
            assert_lists_identical(fa.result(), mc.fold(xs, ys, n, N), what)
            assert _bits(dy) == ybits, f"{what}: the update was written"
            inplace = owned and mc.inplace_pair(xdt, ydt, n, N)
            for i, (t, x0) in enumerate(zip(fa.x, dx)):
                if x0.numel() == 0:
                    continue
                if inplace:
                    assert t.data_ptr() == x0.data_ptr(), f"{what}[{i}]: the in-place arm did not run"
                else:
                    assert t.data_ptr() != x0.data_ptr(), f"{what}[{i}]"
            if not inplace:
                assert _bits(dx) == [a.tobytes() for a in xs], f"{what}: the starting tensors were written"


# ---- B. sequences -------------------------------------------------------------------------------------------

CHAINS = {
    "f16-float-first": ("f16", ["u8", "i16", "i32", "f16"], [2.5, 3, 40, 7], [10, 13, 53, 60]),
    "i8-ints": ("i8", ["i8", "u16", "f32", "i64"], [37, 5, 12, 1], [100, 105, 117, 118]),
    "u64-npint": ("u64", ["i64", "u64", "f64"], [np.int64(3), np.int64(8), np.int64(2)], [11, 19, 21]),
    "i32-npint": ("i32", ["i32", "i64", "f32"], [np.int64(3), np.int64(8), np.int64(2)], [11, 19, 21]),
}


@pytest.mark.parametrize("owned", [True, False], ids=["owned", "views"])
@pytest.mark.parametrize("chain", list(CHAINS))
def test_fold_sequences(chain, owned):
    """Folds whose dtypes escalate, checked after every fold against increment_average in the same order."""
    from fedn_amd import mixed
    xdt, ydts, ns, Ns = CHAINS[chain]
    xs = _state(xdt, "model")
    dx = _up(xs, offset=True)
    fa = mixed.TensorFedAvg(DEV, _stream(), dx, owned=owned)
    model = xs
    ups = []
    for k, (ydt, n, N) in enumerate(zip(ydts, ns, Ns)):
        ys = _state(ydt, "update", seed=10 + k)
        dy = _up(ys, offset=k % 2 == 0)
        ups.append((dy, ys))
        with mc.quiet():
            fa.fold(dy, n, N)
        model = mc.fold(model, ys, n, N)
        assert_lists_identical(fa.result(), model, f"{chain} after fold {k} ({ydt}, n {n!r})")
    for dy, ys in ups:
        assert _bits(dy) == [a.tobytes() for a in ys]
    if not owned:
        assert _bits(dx) == [a.tobytes() for a in xs]
    got = fa.result()                        # caller-owned: writing into it changes no later result
    for a in got:
        if a.size:
            a.reshape(-1)[0] = 7
    assert_lists_identical(fa.result(), model, f"{chain}: result() after its arrays were written")


# ---- C. broadcasting and truncation --------------------------------------------------------------------------

@pytest.mark.parametrize("owned", [True, False], ids=["owned", "views"])
@pytest.mark.parametrize("xdt,ydt", mc.BCAST_DTYPES)
def test_fold_broadcast(xdt, ydt, owned):
    """Every broadcast pair in one state, then a second fold of the original model shapes into the
    now-broadcast state (the state keeps the broadcast shape)."""
    from fedn_amd import mixed
    xs = [mc.tensor(xdt, s, "model", roll=i) for i, (s, _) in enumerate(mc.BCAST)]
    ys = [mc.tensor(ydt, s, "update", roll=i) for i, (_, s) in enumerate(mc.BCAST)]
    zs = [mc.tensor(xdt, s, "update", seed=3, roll=i + 2) for i, (s, _) in enumerate(mc.BCAST)]
    # a transposed, non-contiguous (5, 7) model view against (5, 7)
    base = mc.tensor(xdt, (7, 5), "model", seed=4)
    xs.append(base.T)
    ys.append(mc.tensor(ydt, (5, 7), "update", seed=4))
    zs.append(mc.tensor(xdt, (5, 7), "update", seed=5))
    dx = _up(xs[:-1]) + [_up([base])[0].T]
    assert not dx[-1].is_contiguous() and tuple(dx[-1].shape) == (5, 7)
    dy, dz = _up(ys), _up(zs)
    fa = mixed.TensorFedAvg(DEV, _stream(), dx, owned=owned)
    with mc.quiet():
        fa.fold(dy, 37, 1234)
    want = mc.fold(xs, ys, 37, 1234)
    assert [tuple(t.shape) for t in fa.x] == [w.shape for w in want]
    assert_lists_identical(fa.result(), want, f"{xdt}/{ydt} broadcast")
    with mc.quiet():
        fa.fold(dz, 5, 1239)
    want2 = mc.fold(want, zs, 5, 1239)
    assert [tuple(t.shape) for t in fa.x] == [w.shape for w in want]
    assert_lists_identical(fa.result(), want2, f"{xdt}/{ydt} second fold into the broadcast state")
    assert _bits(dy) == [a.tobytes() for a in ys] and _bits(dz) == [a.tobytes() for a in zs]
    # only an owned, contiguous model that already has the difference's dtype and the result's shape is written
    d = np.subtract(np.empty(0, NP_DT[ydt]), np.empty(0, NP_DT[xdt])).dtype
    for i, (got, x, w, t) in enumerate(zip(_bits(dx), xs, want, dx)):
        if not (owned and d == NP_DT[xdt] and d.kind == "f" and x.shape == w.shape and t.is_contiguous()):
            assert got == np.ascontiguousarray(x).tobytes(), f"{xdt}/{ydt}[{i}]: the starting tensor was written"


@pytest.mark.parametrize("nx,ny", [(3, 2), (2, 3)])
def test_fold_zip_truncation(nx, ny):
    from fedn_amd import mixed
    xs = [mc.tensor("f32", (257,), "model", seed=i) for i in range(nx)]
    ys = [mc.tensor("f64", (257,), "update", seed=i) for i in range(ny)]
    dx, dy = _up(xs), _up(ys)
    fa = mixed.TensorFedAvg(DEV, _stream(), dx, owned=True)
    with mc.quiet():
        fa.fold(dy, 37, 1234)
    got = fa.result()
    assert len(got) == 2
    assert_lists_identical(got, mc.fold(xs, ys, 37, 1234), "zip truncation")
    assert _bits(dx) == [a.tobytes() for a in xs] and _bits(dy) == [a.tobytes() for a in ys]


@pytest.mark.parametrize("pair", [mc.BCAST_REFUSED, mc.RANK9], ids=["5-vs-4", "rank9"])
def test_fold_refused_shapes(pair, launches):
    """Shapes numpy cannot broadcast (numpy's ValueError) and nine non-mergeable dimensions (ops.cast's
    ValueError: the kernel walks 8) are refused before any launch — the in-place tensor ahead of them in the
    state included — and a valid fold follows with numpy's bits."""
    from fedn_amd import mixed, ops
    xs = [mc.tensor("f32", (257,), "model"), mc.tensor("f32", pair[0], "model")]
    ys = [mc.tensor("f32", (257,), "update"), mc.tensor("f32", pair[1], "update")]
    dx, dy = _up(xs), _up(ys)
    if pair is mc.RANK9:
        with pytest.raises(ValueError):
            ops.cast(torch.empty(np.broadcast_shapes(*pair), dtype=torch.float32, device=DEV), dx[1])
    else:
        with pytest.raises(ValueError):
            np.broadcast_shapes(*pair)
    fa = mixed.TensorFedAvg(DEV, _stream(), dx, owned=True)
    _refused(fa, lambda: fa.fold(dy, 37, 1234), ValueError, launches, str(pair))
    ok = [ys[0], mc.tensor("f32", pair[0], "update")]
    fa.fold(_up(ok), 37, 1234)
    assert_lists_identical(fa.result(), mc.fold(xs, ok, 37, 1234), "after the refusal")


# ---- D. refusals --------------------------------------------------------------------------------------------

REFUSALS = [("bool", "bool", "int"), ("i8", "i8", "300"), ("u8", "u8", "300"), ("u8", "u16", "-5"), ("u64", "u32", "-5"),
            ("i16", "i16", "2^53"), ("i32", "i32", "2^53"),                               # numpy's own
            ("bool", "f32", "int"), ("i8", "bool", "float"),                              # (a)
            ("i8", "i8", "npi64"), ("u16", "u8", "npi32"), ("u32", "u32", "npi8"),        # (b)
            ("u64", "u64", "2^53"), ("u8", "u64", "2^53"),                                # (c)
            ("f16", "f16", "npf32"), ("i8", "i16", "npf32"), ("f32", "f32", "npi64"), ("f16", "u8", "npi32")]   # (d)


@pytest.mark.parametrize("xdt,ydt,kind", REFUSALS)
def test_fold_refusals(xdt, ydt, kind, launches):
    from fedn_amd import mixed
    n, N = mc.N_KINDS[kind]
    want = mc.refusal(xdt, ydt, n, N)
    assert want is not None
    xs, ys = _state(xdt, "model"), _state(ydt, "update")
    dx, dy = _up(xs, offset=True), _up(ys, offset=True)
    fa = mixed.TensorFedAvg(DEV, _stream(), dx, owned=True)
    _refused(fa, lambda: fa.fold(dy, n, N), want[0], launches, f"{xdt} {ydt} {kind}")
    assert _bits(dy) == [a.tobytes() for a in ys]
    if xdt != "bool":                        # a following valid fold gives numpy's bits
        zs = _state(xdt, "update", seed=9)
        with mc.quiet():
            fa.fold(_up(zs), 1.0, 4.0)
        assert_lists_identical(fa.result(), mc.fold(xs, zs, 1.0, 4.0), f"{xdt} after the refusal")


@pytest.mark.parametrize("bdt", ["bool"])
def test_fold_bool_pairs(bdt, launches):
    """Every pair with a bool side: (bool, bool) is numpy's boolean-subtract TypeError, the other 22 are class
    (a) — numpy folds them, no kernel takes bool, so this build refuses them before any launch."""
    from fedn_amd import mixed
    for xdt, ydt in mc.PAIRS:
        if bdt not in (xdt, ydt):
            continue
        xs, ys = [mc.tensor(xdt, (257,), "model")], [mc.tensor(ydt, (257,), "update")]
        if (xdt, ydt) != ("bool", "bool"):
            mc.fold(xs, ys, 37, 1234)        # numpy folds it
        fa = mixed.TensorFedAvg(DEV, _stream(), _up(xs), owned=True)
        dy = _up(ys)
        _refused(fa, lambda: fa.fold(dy, 37, 1234), TypeError, launches, f"{xdt} {ydt}")


# ---- E. TensorFedOpt ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("odt", mc.FOLDED)
def test_fedopt_add_dtype_grid(odt):
    """The first add (pg = subtract(update, old)) at every (update, old) pair, then an update of another
    dtype folded into the pseudo-gradient."""
    from fedn_amd import mixed
    olds = _state(odt, "model")
    do = _up(olds, offset=True)
    for j, ydt in enumerate(mc.FOLDED):
        zdt = mc.FOLDED[(j + 3) % len(mc.FOLDED)]
        ys, zs = _state(ydt, "update"), _state(zdt, "update", seed=6)
        dy, dz = _up(ys, offset=True), _up(zs)
        fo = mixed.TensorFedOpt(DEV, _stream(), do)
        fo.add(dy, 37, 37)
        pg = mc.subtract(ys, olds)
        assert_lists_identical(_host(fo.acc.x), pg, f"pg of {ydt} over {odt}")
        with mc.quiet():
            fo.add(dz, 5, 42)
        want = mc.fold(pg, mc.subtract(zs, olds), 5, 42)
        assert_lists_identical(_host(fo.acc.x), want, f"pg of {ydt} then {zdt} over {odt}")
        assert _bits(dy) == [a.tobytes() for a in ys] and _bits(dz) == [a.tobytes() for a in zs]
    assert _bits(do) == [a.tobytes() for a in olds]


@pytest.mark.parametrize("nold,ny,nz", [(3, 2, 3), (2, 3, 3), (3, 3, 1)])
def test_fedopt_add_zip_truncation(nold, ny, nz):
    """Fewer tensors in the global model or in an update: subtract and the fold of the pseudo-gradient both
    truncate, as numpy's zip does."""
    from fedn_amd import mixed
    olds = [mc.tensor("f32", (257,), "model", seed=i) for i in range(nold)]
    ys = [mc.tensor("f64", (257,), "update", seed=i) for i in range(ny)]
    zs = [mc.tensor("f16", (257,), "update", seed=5 + i) for i in range(nz)]
    fo = mixed.TensorFedOpt(DEV, _stream(), _up(olds))
    fo.add(_up(ys), 37, 37)
    pg = mc.subtract(ys, olds)
    assert len(fo.acc.x) == len(pg) == min(nold, ny)
    with mc.quiet():
        fo.add(_up(zs), 5, 42)
    want = mc.fold(pg, mc.subtract(zs, olds), 5, 42)
    assert len(want) == min(nold, ny, nz)
    assert_lists_identical(_host(fo.acc.x), want, "pseudo-gradient under zip truncation")


def _fedopt_round(fo_old, updates, m, v, params, fp32=False):
    """One round on TensorFedOpt: (model, m, v) with the updates folded in order."""
    from fedn_amd import mixed
    fo = mixed.TensorFedOpt(DEV, _stream(), fo_old)
    total = 0
    for dy, n in updates:
        total += n
        with mc.quiet():
            fo.add(dy, n, total)
    with mc.quiet():
        return fo.server_step(m, v, params, fp32=fp32)


FAMILIES = [("f16", ["f16", "f16"]), ("f32", ["f16", "f16"]), ("f16", ["f32", "f32"]), ("f64", ["f32", "f32"]),
            ("f32", ["f64", "f32"]), ("f16", ["f64", "f32"]), ("f16", ["i32", "f16"]), ("i8", ["i8", "f32"]), ("u8", ["u8", "f16"]), ("i16", ["i16", "f64"]),
            ("i32", ["i32", "f32"]), ("i64", ["i64", "f32"]), ("i64", ["i32", "i64"])]


@pytest.mark.parametrize("opt", ["adam", "yogi", "adagrad"])
@pytest.mark.parametrize("odt,ydts", FAMILIES, ids=[f"{o}-{'-'.join(y)}" for o, y in FAMILIES])
def test_fedopt_server_step(odt, ydts, opt):
    """Two rounds with m / v carried as device tensors, against fedopt_combine on a FedOptState."""
    params = dict(PARAMS, serveropt=opt)
    state = ref.FedOptState()
    old = _state(odt, "model")
    m = v = None
    for r in range(2):
        ups = [(_state(ydt, "update", seed=20 + 2 * r + k), n) for k, (ydt, n) in enumerate(zip(ydts, (37, 5)))]
        dev = [(_up(a, offset=True), n) for a, n in ups]
        do = _up(old, offset=True)
        with mc.quiet():
            want, nr = ref.fedopt_combine(state, ups, old, params)
        assert nr == 2 and want is not None
        model, m, v = _fedopt_round(do, dev, m, v, params)
        what = f"{opt} {odt} <- {ydts} round {r}"
        assert_lists_identical(model, want, what)
        assert_lists_identical(_host(m), state.m, what + " m")
        assert_lists_identical(_host(v), state.v, what + " v")
        assert _bits(do) == [a.tobytes() for a in old]
        for (dy, _), (a, _) in zip(dev, ups):
            assert _bits(dy) == [x.tobytes() for x in a]
        old = want


@pytest.mark.parametrize("odt", ["f32", "f64"])
def test_fedopt_server_step_fp32_state(odt):
    params = dict(PARAMS, serveropt="adam")
    state = ref.FedOptState()
    old = _state(odt, "model")
    m = v = None
    for r in range(2):
        ups = [(_state("f32", "update", seed=30 + r), 37), (_state("f64", "update", seed=40 + r), 5)]
        dev = [(_up(a), n) for a, n in ups]
        with mc.quiet():
            want, nr = ref.fedopt_combine_f32state(state, ups, old, params)
        model, m, v = _fedopt_round(_up(old), dev, m, v, params, fp32=True)
        what = f"fp32 state over {odt} round {r}"
        assert_lists_identical(model, want, what)
        assert_lists_identical(_host(m), state.m, what + " m")
        assert_lists_identical(_host(v), state.v, what + " v")
        old = want


@pytest.mark.parametrize("oshape,yshape", [((1,), (257,)), ((257,), (1,))])
def test_fedopt_broadcast_rounds(oshape, yshape):
    """A (1,) global model under (257,) updates and the reverse: round 1's state has the broadcast shape and
    feeds round 2."""
    params = dict(PARAMS, serveropt="yogi")
    state = ref.FedOptState()
    old = [mc.tensor("f32", oshape, "model", roll=12)]
    m = v = None
    for r in range(2):
        ups = [([mc.tensor("f32", yshape, "update", seed=r, roll=12)], 37), ([mc.tensor("f64", yshape, "update", seed=5 + r)], 5)]
        with mc.quiet():
            want, _ = ref.fedopt_combine(state, ups, old, params)
        model, m, v = _fedopt_round(_up(old), [(_up(a), n) for a, n in ups], m, v, params)
        assert want[0].shape == (257,) == tuple(m[0].shape) == tuple(v[0].shape)
        assert_lists_identical(model, want, f"round {r}")
        assert_lists_identical(_host(m), state.m, f"round {r} m")
        assert_lists_identical(_host(v), state.v, f"round {r} v")
        old = want


def test_fedopt_truncation_tau0_and_bad_optimizer(launches):
    """m with fewer tensors truncates the step (L = min(...)); tau = 0; an unsupported serveropt raises
    ValueError with nothing launched. Under a shorter m numpy's own v keeps every tensor of the pseudo-gradient
    (add(v, pg^2) truncates to v and pg alone) while the model and m have L; server_step returns L tensors of
    each, so v is compared over those L."""
    from fedn_amd import mixed
    params = dict(PARAMS, serveropt="adam", tau=0.0)
    state = ref.FedOptState()
    old = [mc.tensor("f32", (257,), "model", seed=i) for i in range(3)]
    ups = [([mc.tensor("f32", (257,), "update", seed=i) for i in range(3)], 37),
           ([mc.tensor("f64", (257,), "update", seed=7 + i) for i in range(3)], 5)]
    with mc.quiet():
        want, _ = ref.fedopt_combine(state, ups, old, params)
    model, m, v = _fedopt_round(_up(old), [(_up(a), n) for a, n in ups], None, None, params)
    assert_lists_identical(model, want, "tau = 0")
    assert_lists_identical(_host(v), state.v, "tau = 0 v")
    state.m, m = state.m[:2], m[:2]
    with mc.quiet():
        want2, _ = ref.fedopt_combine(state, ups, want, params)
    model2, m2, v2 = _fedopt_round(_up(want), [(_up(a), n) for a, n in ups], m, v, params)
    assert len(want2) == 2 == len(model2) == len(m2) == len(v2)
    assert_lists_identical(model2, want2, "m with fewer tensors")
    assert_lists_identical(_host(m2), state.m, "m with fewer tensors: m")
    assert len(state.v) == 3
    assert_lists_identical(_host(v2), state.v[:2], "m with fewer tensors: v")
    fo = mixed.TensorFedOpt(DEV, _stream(), _up(old))
    fo.add(_up(ups[0][0]), 37, 37)
    ran = launches["n"]
    with pytest.raises(ValueError):
        fo.server_step(None, None, dict(PARAMS, serveropt="sgd"))
    assert launches["n"] == ran


# ---- F. through the plug-ins and the pipelines --------------------------------------------------------------

F_SHAPES = [(5,), (257,), (3,), (4099,)]
F_DTYPES = ["f32", "i32", "i64", "f32"]


def _f_clients(change):
    """K = 4 updates of an (f32, int32, int64, f32) layout: the second one changes tensor 0 (its dtype to f64, or its
    shape to (1,)), so the uniform pipeline hands over with the first update still a staged view; the third has a
    (4,) tensor against (5,): numpy's ValueError, skipped with its examples counted."""
    ups = [[mc.tensor(d, s, "model" if k == 0 else "update", seed=50 + k, roll=k) for s, d in zip(F_SHAPES, F_DTYPES)]
           for k in range(4)]
    ups[1][0] = mc.tensor("f64", (5,), "update", seed=60) if change == "dtype" else mc.tensor("f32", (1,), "update", seed=60)
    ups[2][0] = mc.tensor("f32", (4,), "update", seed=61)
    return ups


F_NS = {"int": [37, 3, 11, 5], "float": [37.0, 2.5, 11.0, 5.5]}


def _handlers(route):
    from fedn_amd.ingest import StagingUpdateHandler
    from fedn_amd.updatehandler import MemoryUpdateHandler
    uh = MemoryUpdateHandler()
    st = None
    if route == "staged":
        st = StagingUpdateHandler(uh, helper=None, device=DEV, workers=2)
    elif route == "staged_sliced":
        st = StagingUpdateHandler(uh, helper=None, devices=[DEV, DEV], workers=2)
    return uh, st


def _aggregator(mod, route, uh, st, monkeypatch):
    if route == "staged_sliced":
        from fedn_amd import layout
        monkeypatch.setattr(layout, "MULTIDEV_MIN_BYTES", 0)
        return mod.Aggregator(st or uh, devices=[DEV, DEV])
    return mod.Aggregator(st or uh)


@pytest.mark.parametrize("change", ["dtype", "shape"])
@pytest.mark.parametrize("nkind", list(F_NS))
@pytest.mark.parametrize("route", ["host", "staged", "staged_sliced"])
def test_plugin_fedavg_hands_over(route, nkind, change, monkeypatch):
    from fedn_amd.aggregators import fedavg
    ups, ns = _f_clients(change), F_NS[nkind]
    with mc.quiet():
        want, nr = ref.fedavg_combine(list(zip(ups, ns)))
    assert nr == 3
    uh, st = _handlers(route)
    try:
        agg = _aggregator(fedavg, route, uh, st, monkeypatch)
        for a, n in zip(ups, ns):
            uh.submit(a, n, model_id="global", via=st)
        with mc.quiet():
            model, data = agg.combine_models(helper=None, delete_models=True)
    finally:
        if st is not None:
            st.close()
    assert data["nr_aggregated_models"] == nr
    assert_lists_identical(model, want, f"{route} n {nkind} {change}")


@pytest.mark.parametrize("change", ["dtype", "shape"])
def test_pipeline_handover_keeps_the_staged_first_update(change):
    """The uniform pipeline hands over while the running model is still the staged first update (views,
    owned=False): the unchanged f32 tensors are an in-place pair, and the staged bytes must stay intact."""
    from fedn_amd import mixed, staging
    ups, ns = _f_clients(change), F_NS["int"]
    pipe = staging.FedAvgPipeline(DEV, ups[0])
    with mc.quiet():
        pipe.add(ups[1], ns[1], ns[0] + ns[1])
    assert pipe.general is not None
    staged = mixed.tensor_views(pipe.layout, mixed.u8_flats(pipe.layout, pipe.first.dev))
    assert _bits(staged) == [a.tobytes() for a in ups[0]]
    with mc.quiet():
        want, _ = ref.fedavg_combine(list(zip(ups[:2], ns[:2])))
        assert_lists_identical(pipe.result(), want, change)


@pytest.mark.parametrize("change", ["dtype", "shape"])
@pytest.mark.parametrize("route", ["host", "staged", "staged_sliced"])
def test_plugin_fedopt_hands_over(route, change, monkeypatch):
    from fedn_amd.aggregators import fedopt
    params = dict(PARAMS, serveropt="adam")
    ups, ns = _f_clients(change), F_NS["int"]
    old = [mc.tensor("f32" if d == "f32" else d, s, "model", seed=70) for s, d in zip(F_SHAPES, F_DTYPES)]
    state = ref.FedOptState()
    with mc.quiet():
        want, nr = ref.fedopt_combine(state, list(zip(ups, ns)), old, params)
    assert nr == 3 and want is not None
    uh, st = _handlers(route)
    try:
        agg = _aggregator(fedopt, route, uh, st, monkeypatch)
        gid = uh.put_global_model(old, "g0")
        for a, n in zip(ups, ns):
            uh.submit(a, n, model_id=gid, via=st)
        with mc.quiet():
            model, data = agg.combine_models(helper=None, delete_models=True, parameters=params)
    finally:
        if st is not None:
            st.close()
    assert data["nr_aggregated_models"] == nr
    assert_lists_identical(model, want, f"{route} {change}")
    assert_lists_identical(agg.m, state.m, f"{route} {change} m")
    assert_lists_identical(agg.v, state.v, f"{route} {change} v")


@pytest.mark.parametrize("same_layout", [True, False], ids=["uniform", "mixed"])
@pytest.mark.parametrize("sliced", [False, True], ids=["one-device", "sliced"])
def test_pipeline_numpy_int_num_examples(sliced, same_layout, monkeypatch):
    """np.int64 num_examples on a layout of int32 and int64 tensors (the update handlers carry num_examples as
    JSON, so this kind reaches the pipelines only from a caller's own loop). np.int64(3) times an int32
    difference is int64 in numpy — it does not wrap at 32 bits — so the first fold leaves the fused integer
    fold, uniform layout or not; the loop below is fedavg.py's, a refused update skipped and counted."""
    from fedn_amd import layout, multidev, staging
    shapes, dtypes = [(257,), (5,), (4099,)], ["i32", "i64", "i32"]
    ups = [[mc.tensor(d, s, "model" if k == 0 else "update", seed=80 + k, roll=k) for s, d in zip(shapes, dtypes)]
           for k in range(4)]
    if not same_layout:
        ups[1][2] = mc.tensor("i64", (4099,), "update", seed=90)
    ups[2][1] = mc.tensor("i64", (4,), "update", seed=91)          # (4,) against (5,): numpy's ValueError
    ns = [np.int64(37), np.int64(3), np.int64(11), np.int64(5)]
    with mc.quiet():
        want, nr = ref.fedavg_combine(list(zip(ups, ns)))
        # the column that separates an int32 product from an int64 one is in play
        a32 = ref.fedavg_combine([(ups[0], 37), (ups[1], 3)])[0][0]
        a64 = ref.fedavg_combine([(ups[0], ns[0]), (ups[1], ns[1])])[0][0]
    assert nr == 3 and (a32 != a64).any()
    if sliced:
        monkeypatch.setattr(layout, "MULTIDEV_MIN_BYTES", 0)
        pipe = multidev.ShardedFedAvgPipeline([DEV, DEV], ups[0])
    else:
        pipe = staging.FedAvgPipeline(DEV, ups[0])
    total, got_nr, errors = ns[0], 1, []
    for a, n in zip(ups[1:], ns[1:]):
        total += n
        try:
            with mc.quiet():
                pipe.add(a, n, total)
        except Exception as e:  # noqa: BLE001  (fedavg.py:75-78 logs and continues)
            errors.append(e)
            continue
        got_nr += 1
    assert got_nr == nr and [type(e) for e in errors] == [ValueError], errors
    with mc.quiet():
        assert_lists_identical(pipe.result(), want, f"sliced {sliced} same layout {same_layout}")
