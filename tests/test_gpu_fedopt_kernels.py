"""The FedOpt step kernels (``fa_fedopt_step_ex``: ``k_fedopt`` and ``k_fedopt_c``) bit for bit (values
and dtype, NaN by position) against the oracle's ``fedopt_combine`` / ``fedopt_combine_f32state`` with the
server state set directly (tests/fedopt_cases.py; tests/test_fedopt_cases_host.py shows on the oracle
alone that the special columns reach their lanes). Every launch is followed by a check of
``ops.last_kernel()``: ``k_fedopt_c`` while every pointer of the launch is 16-B aligned (all sizes here
are far below the store window's 2^24), ``k_fedopt`` as soon as one is not. Every device buffer has 64
guard elements on each side, filled with a NaN-patterned sentinel: the guards must be unchanged, and
every one of the P elements of ``out`` / ``m_out`` / ``v_out`` must have been written. After a
non-final launch the ``pg`` workspace is compared with numpy's running pseudo-gradient.

Sections and the code they reach (fedn_amd/csrc):

A. ``test_dispatch_grid`` — the 17 dtype pairs of the dispatch in fedagg.hip, each x {adam, yogi, adagrad} x
   m_in in {None, f16, f32, f64} x v_in in {None, f64, f32}, on both kernels (aligned; every buffer
   shifted by one element): every (PG arithmetic x m dtype) branch of ``opt_apply`` and
   ``opt_load_state``, ``mul_pg`` / ``pg_sq`` / ``pg_sub`` of CF16, CF32 and CF64, the weak-scalar
   casts b1f / c1f / c2f and b1h / c1h / c2h. Nothing is paired: the full product runs (36 launches per
   test, twice where aliasing is allowed). The parameter set alternates with (m_in, v_in) so each
   optimizer sees both. A second launch with ``m_out is m_in`` and / or ``v_out is v_in`` runs wherever
   the dtypes allow it. ``test_dispatch_grid_f32state``: the f32 stores of out / v / m and the f32 v load,
   for the six pairs whose old is f32.
B. ``test_element_map`` — P = 1, 3 (one ragged strip), 4 (one whole strip in a ragged tile), 255, 257 (the
   ``j`` loop of ``fedopt_c_body``'s ragged tile), 512 (one wave tile, three idle waves), 515, 2048 (one
   workgroup), 2819 (a whole tile, then a ragged tile with j = 0 full and 3 elements in j = 1), 6151;
   the scalar kernel's ``rem < E`` never occurs (E = 1), its grid does: P = 1, 255, 257, 2819.
C. ``test_client_loop_and_launch_split`` — K = 1, 2, 4, 5, 6, 9 (the batches of kUnroll/2 = 4 after the
   first client and the tail loop of ``fedopt_strip_split`` / ``fedopt_strip``), 64, 65, 129 (the client
   table's boundary: ``launch_fedopt``'s second and third launch are ``!first``), in one call and as
   waves: ``first && !final``, ``!first && !final`` waves of 1, 4, 5 and 8, then ``!first && final`` with
   the last clients, or the K = 0 server-only step. For (f16, f16) the workspace is half
   (``narrow`` / ``widen``).
D. ``test_single_buffer_misalignment`` — ``launch_fedopt``'s ``vec`` test: exactly one of old, pg, m_in,
   m_out, v_in, v_out, out, updates[3], updates[66] off 16 bytes.
E. ``test_special_columns`` — CF32::fold_strip's redo for 0 < |t| < 2^-98 and its zero lanes, CF64::div
   outside [2^-600, 2^600] and for signed zero, r == 0 for |N| >= 2^28 (``fill_table``), ``np_sign``'s
   0 and NaN arms, the half rule's overflow / underflow and its inf n and N, int64 beyond 2^53,
   tau = 0; both kernels, one call and waves with the K = 0 server step (the first wave is clients 0 and 1,
   the fold step the ``fixed:*`` columns are written for), K = 2, 5 and 65.
"""
import numpy as np
import pytest
import torch

import fedopt_cases as fc
from golden_io import assert_lists_identical
from guarded_buf import TORCH_DT, Buf

pytestmark = pytest.mark.gpu

P0, K0 = 2819, 6
_REF = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from fedn_amd import _abi
    _abi.load()
    yield
    _REF.clear()
    torch.cuda.empty_cache()


def _cached(key, make):
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def _shift(shifts, name):
    return 1 if ("all" in shifts or name in shifts) else 0


class Inputs:
    """old and the updates of one case on the device; reused by the launch forms of that case."""

    def __init__(self, pair, old, ups, shifts=()):
        self.pair, self.P, self.shifts = pair, len(old), frozenset(shifts)
        self.old = Buf(self.P, pair[1], _shift(shifts, "old"), old)
        self.ups = [Buf(self.P, pair[0], _shift(shifts, f"u{k}"), u) for k, u in enumerate(ups)]


def _plan(K, form, first=3):
    """The launches of one round as (k0, k1, first, final).
    "call": one call. "waves-final": first && !final, !first && !final waves, the last wave final.
    "waves-k0": every wave non-final, then the K = 0 server-only step. ``first``: the clients of the
    first wave (fewer when K is small)."""
    if form == "call":
        return [(0, K, True, True)]
    sizes, k = [], 0
    seq = [min(first, max(1, K - 1 if form == "waves-final" else K))] + [1, 4, 5, 8] * 40
    for s in seq:
        if k >= K:
            break
        sizes.append(min(s, K - k))
        k += sizes[-1]
    plan, k = [], 0
    for i, s in enumerate(sizes):
        plan.append((k, k + s, i == 0, form == "waves-final" and i == len(sizes) - 1 and i > 0))
        k += s
    if not plan[-1][3]:
        plan.append((K, K, False, True))
    return plan


def _run(inp, ns, m, v, params, *, form="call", plan=None, first_wave=3, f32state=False, alias=(), want_pg=None, what=""):
    """One round on the device. ``m`` / ``v``: (dtype name, array) or None. Returns (out, m_out, v_out) as
    numpy arrays after the kernel-name, guard and coverage checks."""
    from fedn_amd import ops
    pair, P, sh = inp.pair, inp.P, inp.shifts
    K = len(inp.ups)
    Ns = fc.totals(ns)
    pg_dt = fc.pg_dtype(pair)
    m_dt = None if m is None else m[0]
    mo_dt = "f32" if f32state else fc.m_out_dtype(pair, m_dt)
    st_dt = "f32" if f32state else "f64"
    pg = Buf(P, pg_dt, _shift(sh, "pg"))
    m_in = None if m is None else Buf(P, m[0], _shift(sh, "m_in"), m[1])
    v_in = None if v is None else Buf(P, v[0], _shift(sh, "v_in"), v[1])
    if "m" in alias:
        assert m_in is not None and m[0] == mo_dt and _shift(sh, "m_in") == _shift(sh, "m_out")
        m_out = m_in
    else:
        m_out = Buf(P, mo_dt, _shift(sh, "m_out"))
    if "v" in alias:
        assert v_in is not None and v[0] == st_dt and _shift(sh, "v_in") == _shift(sh, "v_out")
        v_out = v_in
    else:
        v_out = Buf(P, st_dt, _shift(sh, "v_out"))
    out = Buf(P, st_dt, _shift(sh, "out"))
    kw = dict(pg=pg.t, m_in=None if m_in is None else m_in.t, m_out=m_out.t, v_in=None if v_in is None else v_in.t,
              v_out=v_out.t, out=out.t, **params)
    passed = {"old", "pg", "m_out", "v_out", "out"} | ({"m_in"} if m_in else set()) | ({"v_in"} if v_in else set())
    for k0, k1, first, final in (plan or _plan(K, form, first_wave)):
        ops.fedopt_step(inp.old.t, [u.t for u in inp.ups[k0:k1]], ns[k0:k1], Ns[k0:k1], first=first, final=final,
                        upd_dtype=TORCH_DT[pair[0]], **kw)
        off = "all" in sh or bool(sh & (passed | {f"u{k}" for k in range(k0, k1)}))
        assert ops.last_kernel() == ("k_fedopt" if off else "k_fedopt_c"), f"{what} launch {k0}:{k1}: {ops.last_kernel()}"
        if not final and want_pg is not None:
            assert_lists_identical([pg.numpy()], [want_pg[k1 - 1]], f"{what} pg after client {k1 - 1}")
    torch.cuda.synchronize()
    res = out.numpy(), m_out.numpy(), v_out.numpy()
    out.check(f"{what} out", True)
    m_out.check(f"{what} m_out", "m" not in alias)
    v_out.check(f"{what} v_out", "v" not in alias)
    pg.check(f"{what} pg", False)
    return res


def _same(got, want, what):
    for g, w, n in zip(got, want, ("out", "m", "v")):
        assert_lists_identical([g], [w], f"{what} {n}")


# ---- ordinary data ---------------------------------------------------------------------------------
def _data(pair, P, K, seed=0):
    """old, updates = old + 0.01 N(0,1) (integers: +-10^6, the first columns the dtype's extremes), ns,
    and m / v of every dtype."""
    def make():
        u, o = pair
        rng = np.random.default_rng(1000 + seed + 17 * fc.PAIRS.index(pair))
        if fc.is_int(u):
            ii = np.iinfo(fc.NP_DT[u])
            ext = [0, -1, int(ii.min), int(ii.max)]
            base = rng.integers(-10 ** 6, 10 ** 6, P)
            ups = [base + rng.integers(-100, 100, P) for _ in range(K)]
            oldv = [int(x) for x in base] if fc.is_int(o) else [float(x) + 0.5 for x in base]
            for c in range(min(P, 16)):
                if fc.is_int(o):
                    oldv[c] = ext[c % 4]
                for k in range(K):
                    ups[k][c] = ext[(c // 4 + k * (c % 2)) % 4]
            old = fc.cast(o, oldv)
            ups = [fc.cast(u, x) for x in ups]
        else:
            base = 1.0 + 0.1 * rng.standard_normal(P)
            old = fc.cast(o, base)
            ups = [fc.cast(u, old.astype(np.float64) + 0.01 * rng.standard_normal(P)) for _ in range(K)]
        ns = fc.client_ns(K, "float" if seed % 2 == 0 else "plain")
        ms = {d: fc.cast(d, 0.01 * rng.standard_normal(P)) for d in ("f16", "f32", "f64")}
        v64 = (0.01 * rng.standard_normal(P)) ** 2 + 1e-6
        vs = {"f64": v64, "f32": fc.as_f32(v64)}
        return old, ups, ns, ms, vs
    return _cached(("data", pair, P, K, seed), make)


def _ref(key, *args, **kw):
    return _cached(("ref",) + key, lambda: fc.reference(*args, **kw))


_ids = "-".join
_KERNEL = {0: "aligned", 1: "shifted"}


# ---- A. dispatch grid ------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 1], ids=_KERNEL.get)
@pytest.mark.parametrize("pair", fc.PAIRS, ids=_ids)
def test_dispatch_grid(pair, shift):
    old, ups, ns, ms, vs = _data(pair, P0, K0)
    inp = Inputs(pair, old, ups, ("all",) if shift else ())
    for opt in fc.OPTS:
        for i, m_dt in enumerate((None, "f16", "f32", "f64")):
            for j, v_dt in enumerate((None, "f64", "f32")):
                pk = "default" if (i + j) % 2 == 0 else "odd"
                p = fc.params(opt, pk)
                m = None if m_dt is None else ms[m_dt]
                v = None if v_dt is None else vs[v_dt]
                what = f"{pair} {opt} m={m_dt} v={v_dt} {pk}"
                want = _ref((pair, opt, m_dt, v_dt, pk), pair, old, ups, ns, m, v, p)
                margs = None if m is None else (m_dt, m)
                vargs = None if v is None else (v_dt, v)
                _same(_run(inp, ns, margs, vargs, p, what=what), want, what)
                alias = (("m",) if m_dt is not None and m_dt == fc.m_out_dtype(pair, m_dt) else ()) + \
                        (("v",) if v_dt == "f64" else ())
                if alias:
                    _same(_run(inp, ns, margs, vargs, p, alias=alias, what=what + " aliased"), want, what + " aliased")


@pytest.mark.parametrize("shift", [0, 1], ids=_KERNEL.get)
@pytest.mark.parametrize("pair", [p for p in fc.PAIRS if p[1] == "f32"], ids=_ids)
def test_dispatch_grid_f32state(pair, shift):
    old, ups, ns, ms, vs = _data(pair, P0, K0)
    inp = Inputs(pair, old, ups, ("all",) if shift else ())
    for opt in fc.OPTS:
        for i, m_dt in enumerate((None, "f16", "f32", "f64")):
            for j, v_dt in enumerate((None, "f32")):
                pk = "default" if (i + j) % 2 == 0 else "odd"
                p = fc.params(opt, pk)
                m = None if m_dt is None else ms[m_dt]
                v = None if v_dt is None else vs[v_dt]
                what = f"{pair} f32state {opt} m={m_dt} v={v_dt} {pk}"
                want = _ref((pair, opt, m_dt, v_dt, pk, "f32state"), pair, old, ups, ns, m, v, p, f32state=True)
                assert want[0].dtype == want[1].dtype == want[2].dtype == np.float32
                margs = None if m is None else (m_dt, m)
                vargs = None if v is None else (v_dt, v)
                _same(_run(inp, ns, margs, vargs, p, f32state=True, what=what), want, what)
                alias = (("m",) if m_dt == "f32" else ()) + (("v",) if v_dt == "f32" else ())
                if alias:
                    _same(_run(inp, ns, margs, vargs, p, f32state=True, alias=alias, what=what + " aliased"), want,
                          what + " aliased")


# ---- B. element map --------------------------------------------------------------------------------
SIZES = [1, 3, 4, 255, 257, 512, 515, 2048, 2819, 6151]
SCALAR_SIZES = [1, 255, 257, 2819]


@pytest.mark.parametrize("pair", [("f32", "f32"), ("bf16", "f32"), ("f16", "f16"), ("f64", "f64"), ("i64", "i64")], ids=_ids)
def test_element_map(pair):
    old, ups, ns, ms, vs = _data(pair, max(SIZES), K0, seed=1)
    m_dt = fc.pg_dtype(pair)
    p = fc.params("adam", "default")
    for shift, sizes in ((0, SIZES), (1, SCALAR_SIZES)):
        for P in sizes:
            o, us, m, v = old[:P], [u[:P] for u in ups], ms[m_dt][:P], vs["f64"][:P]
            want = _ref((pair, "map", P), pair, o, us, ns, m, v, p)
            what = f"{pair} P={P} {_KERNEL[shift]}"
            inp = Inputs(pair, o, us, ("all",) if shift else ())
            _same(_run(inp, ns, (m_dt, m), ("f64", v), p, what=what), want, what)
            wpg = [s.pg for s in _cached(("trace", pair, "map", P), lambda: fc.fold_trace(o, us, ns))]
            _same(_run(inp, ns, (m_dt, m), ("f64", v), p, form="waves-k0", want_pg=wpg, what=what + " waves"), want,
                  what + " waves")


# ---- C. client loop and launch split ---------------------------------------------------------------
KS = [1, 2, 4, 5, 6, 9, 64, 65, 129]


@pytest.mark.parametrize("shift", [0, 1], ids=_KERNEL.get)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("pair", [("f32", "f32"), ("f16", "f16"), ("bf16", "f64")], ids=_ids)
def test_client_loop_and_launch_split(pair, K, shift):
    old, ups, ns, ms, vs = _data(pair, P0, K, seed=2 + K)
    m_dt = fc.pg_dtype(pair)
    p = fc.params("yogi", "default")
    m, v = ms[m_dt], vs["f64"]
    want = _ref((pair, "K", K), pair, old, ups, ns, m, v, p)
    wpg = [s.pg for s in _cached(("trace", pair, "K", K), lambda: fc.fold_trace(old, ups, ns))]
    inp = Inputs(pair, old, ups, ("all",) if shift else ())
    forms = ["call", "waves-k0"] + (["waves-final"] if K >= 2 else [])
    for form in forms:
        plan = _plan(K, form)
        assert sum(k1 - k0 for k0, k1, _, _ in plan) == K and plan[-1][3] and not any(f for *_, f in plan[:-1])
        what = f"{pair} K={K} {form} {_KERNEL[shift]}"
        _same(_run(inp, ns, (m_dt, m), ("f64", v), p, plan=plan, want_pg=wpg, what=what), want, what)


def test_wave_plans_cover_every_launch_form():
    """The plans above contain first && !final, !first && !final waves of 1, 4, 5 and 8, !first && final with
    clients, and the K = 0 server-only step."""
    seen = set()
    for K in KS:
        for form in ("call", "waves-k0", "waves-final"):
            for k0, k1, first, final in _plan(K, form):
                seen.add((first, final, k1 - k0))
    for want in [(True, True, 129), (True, False, 3), (True, False, 1), (False, True, 0)] + \
                [(False, False, s) for s in (1, 4, 5, 8)]:
        assert want in seen, want
    assert any(not first and final and n > 0 for first, final, n in seen)


# ---- D. single-buffer misalignment -----------------------------------------------------------------
@pytest.mark.parametrize("pair", [("f32", "f32"), ("f32", "f64")], ids=_ids)
def test_single_buffer_misalignment(pair):
    K = 70
    old, ups, ns, ms, vs = _data(pair, P0, K, seed=3)
    m_dt = fc.pg_dtype(pair)
    p = fc.params("adam", "odd")
    m, v = ms[m_dt], vs["f64"]
    want = _ref((pair, "mis"), pair, old, ups, ns, m, v, p)
    wpg = [s.pg for s in fc.fold_trace(old, ups, ns)]
    plan = [(0, 40, True, False), (40, K, False, True)]
    base = _run(Inputs(pair, old, ups), ns, (m_dt, m), ("f64", v), p, plan=plan, want_pg=wpg, what=f"{pair} aligned")
    _same(base, want, f"{pair} aligned")
    for name in ("old", "pg", "m_in", "m_out", "v_in", "v_out", "out", "u3", "u66"):
        what = f"{pair} only {name} shifted"
        got = _run(Inputs(pair, old, ups, (name,)), ns, (m_dt, m), ("f64", v), p, plan=plan, want_pg=wpg, what=what)
        _same(got, base, what + " vs aligned")
        _same(got, want, what)


# ---- E. special columns ----------------------------------------------------------------------------
_M_BY_OPT = {"adam": None, "yogi": "f32", "adagrad": "f64"}       # None: the pseudo-gradient's dtype


@pytest.mark.parametrize("kind", ["float", "big"])
@pytest.mark.parametrize("K", [2, 5, 65])
@pytest.mark.parametrize("opt", fc.OPTS)
@pytest.mark.parametrize("pair", fc.PAIRS, ids=_ids)
def test_special_columns(pair, opt, K, kind):
    p = fc.params(opt, "odd" if kind == "float" else "default")
    m_dt = _M_BY_OPT[opt] or fc.pg_dtype(pair)
    c = fc.special_columns(pair, K, opt, p, ns_kind=kind, m_dt=m_dt)
    old, ups, m, v = fc.tile(c.old, P0), [fc.tile(u, P0) for u in c.ups], fc.tile(c.m, P0), fc.tile(c.v, P0)
    assert len(c.old) < 2048                     # the columns repeat into the ragged tile and the ragged strip
    want = fc.reference(pair, old, ups, c.ns, m, v, p)
    wpg = [s.pg for s in fc.fold_trace(old, ups, c.ns)]
    want_none = fc.reference(pair, old, ups, c.ns, None, None, p)      # a first round: m = None, v = tau^2
    for shift in (0, 1):
        inp = Inputs(pair, old, ups, ("all",) if shift else ())
        for form in ("call", "waves-k0"):
            what = f"{pair} {opt} K={K} {kind} {form} {_KERNEL[shift]}"
            # a first wave of clients 0 and 1: pg is compared right after the fold step the fixed:* columns
            # are written for, before later clients (n close to N in the "big" list) wash a wrong ulp out
            _same(_run(inp, c.ns, (m_dt, m), ("f64", v), p, form=form, first_wave=2, want_pg=wpg, what=what), want, what)
        _same(_run(inp, c.ns, None, None, p, what=what + " no state"), want_none, what + " no state")
