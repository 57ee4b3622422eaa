"""The FedAvg fold (``fa_fedavg_fold``: ``k_fedavg`` with its vector and scalar launches, and the other
carriers of the fp32 fold, ``k_fedavg_push`` and the pipelined geometry ``k_fedavg_pipe``) bit for bit
(values and dtype, NaN by position) against the oracle's ``increment_average`` replayed one client at a
time (tests/fedavg_cases.py; tests/test_fedavg_cases_host.py shows on the oracle alone that the special
columns reach their lanes). Every device buffer has 64 guard elements on each side, filled with a
NaN-patterned sentinel. After every call: the aggregate's guards are unchanged and each of its P elements
was written, every update buffer of the call is bitwise what was uploaded, guards included, and
``ops.last_kernel()`` names the expected family (``k_fedavg``: the name covers the 16-byte-strip launch and
the one-element launch alike; ``k_fedavg_pipe`` under the probe library's forced geometry).

Sections and the code they reach (fedn_amd/csrc):

A. ``test_dispatch_grid`` — the seven pairs of fa_fedavg_fold's dispatch x {init, continuation} x {every
   buffer 16-B aligned, every buffer shifted by one element}, K = 6, P = 2819: ``strip_start``'s INIT,
   INT_FIRST and continuation arms, ``widen`` / ``narrow`` of each pair, CF32 / CF64 / CF16.
   ``test_refused_pairs``: the 29 pairs outside the dispatch (FA_EDTYPE, nothing written);
   ``test_single_client``: K = 1 with init is a bitwise copy for equal dtypes and refused otherwise;
   ``test_empty_calls``: K = 0 and P = 0 write nothing.
B. ``test_element_map`` — P = 1, E - 1, E, E + 1, 255 E + 1 (a ragged strip in the block's last lane),
   256 E (one workgroup), 256 E + 3, 3 * 256 E + E + 1 on the vector launch and P = 1, 255, 257, 1027 on
   the scalar one, K = 3 and 10, init and continuation: ``k_fedavg``'s grid and whole-strip test,
   ``k_fedavg_tail`` and ``strip_start``'s ragged arms.
C. ``test_client_loop_and_launch_split`` — K = 2, 3, 8, 9, 10, 11, 17, 64, 65, 66, 129: the ``kUnroll`` = 8
   batch loop and its tail loop after one consumed client (two after INT_FIRST), fp32's 8 -> 4 clients in
   flight at cnt = 9 (``launch_fedavg_small``), the client table's boundary (``launch_fedavg``'s second and
   third launch re-read the stored aggregate: f16 through ``narrow`` / ``widen``); one call and waves.
D. ``test_single_buffer_misalignment`` — ``launch_fedavg``'s ``vec`` test over agg and all K pointers.
E. ``test_special_columns`` — CF32::fold_strip's redo and zero lanes, r == 0 for |N| >= 2^28, CF64::div's
   guard, its zero arm and r == 0 beyond 2^60, CF16's rounding of n, N (``to_half_value``) and of every
   operation, INT_FIRST's wrapping subtract and multiply, ``(double)(Y)t / N``, int64 beyond 2^53 through
   ``widen<int64_t, double>``; ``test_special_columns_in_ragged_strips`` puts every column into
   ``k_fedavg_tail``; ``test_division_by_large_totals`` pins the r == 0 arm where the reciprocal is wrong.
F. ``test_push_*`` (``k_fedavg_push``, peer_push.h) and ``test_pipelined_*`` (``fedavg_pipe_body`` forced
   small, with the client table read from the kernel argument and from lanes: ``LaneTable``).
G. ``test_int32_multiplier`` — n[1] at and beyond int32's ends; ``test_plugin_skips_int32_overflow``.
"""
import numpy as np
import pytest
import torch

import fedavg_cases as fa
from golden_io import assert_lists_identical
from guarded_buf import DEV, SENTINEL, Buf
from oracle import numpy_ref as ref

pytestmark = pytest.mark.gpu

P0, K0 = 2819, 6
P_PIPE = 2 * 8192 + 2819          # two whole tiles of the pipelined geometries (4096 f32, 8192 bf16), a ragged one
_REF = {}
_ids = "-".join
_KERNEL = {0: "aligned", 1: "shifted"}


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


def _same(got, want, what):
    assert_lists_identical([got], [want], what)


# ---- one fold on guarded buffers -------------------------------------------------------------------
def _upload(pair, ups, shifts=()):
    """The updates as guarded buffers; ``shifts``: "all", or names among "u<k>" to move off 16 bytes."""
    return [Buf(len(u), pair[0], 1 if ("all" in shifts or f"u{k}" in shifts) else 0, u) for k, u in enumerate(ups)]


def _agg(pair, P, shifts=(), agg0=None):
    return Buf(P, pair[1], 1 if ("all" in shifts or "agg" in shifts) else 0, agg0)


def _waves(pair, K, form):
    """(k0, k1) per call. "waves": the first wave (one client; two where a first wave of one is the refused
    copy), then continuations of 1, 1, 8 and the rest."""
    if form == "call":
        return [(0, K)]
    out, k = [], 0
    for s in [2 if pair in fa.NO_COPY else 1, 1, 1, 8, K]:
        if k >= K:
            break
        out.append((k, min(K, k + s)))
        k = out[-1][1]
    return out


def _fold(pair, agg, bufs, ns, Ns, init, what, *, plan=None, kernel="k_fedavg", after=None):
    """The calls of ``plan`` on the device with the checks that follow every call; the aggregate as numpy.
    ``after(k1, array)``: called with the aggregate after the call that ended at client k1."""
    from fedn_amd import ops
    K = len(bufs)
    for k0, k1 in plan or [(0, K)]:
        first = init and k0 == 0
        ops.fedavg_fold(agg.t, [b.t for b in bufs[k0:k1]], ns[k0:k1], Ns[k0:k1], init=first)
        if not (first and k1 - k0 == 1):          # (a copy launches no kernel)
            assert ops.last_kernel() == kernel, f"{what} clients {k0}:{k1}: {ops.last_kernel()}"
        torch.cuda.synchronize()
        agg.check(f"{what} agg after {k0}:{k1}", True)
        for k in range(k0, k1):
            bufs[k].check_unchanged(f"{what} updates[{k}]")
        if after is not None:
            after(k1, agg.numpy())
    return agg.numpy()


def _data(pair, P, K, seed=0):
    """Ordinary data: a stored aggregate, updates = base + 0.01 N(0,1) (integers: +-10^6 around a base, the
    first columns the dtype's extremes), and the pair's ns ("float" for float pairs on even seeds)."""
    def make():
        u, a = pair
        rng = np.random.default_rng(2000 + seed + 17 * fa.PAIRS.index(pair))
        if fa.is_int(u):
            ii = np.iinfo(fa.NP_DT[u])
            ext = [0, -1, int(ii.min), int(ii.max)]
            base = rng.integers(-10 ** 6, 10 ** 6, P)
            ups = [base + rng.integers(-100, 100, P) for _ in range(K)]
            for c in range(min(P, 16)):
                for k in range(K):
                    ups[k][c] = ext[(c // 4 + k * (c % 2)) % 4]
            ups = [fa.cast(u, x) for x in ups]
            agg0 = fa.cast(a, base.astype(np.float64) + 0.5)
        else:
            base = 1.0 + 0.1 * rng.standard_normal(P)
            ups = [fa.cast(u, base + 0.01 * rng.standard_normal(P)) for _ in range(K)]
            agg0 = fa.cast(a, base + 0.01 * rng.standard_normal(P))
        kind = "plain" if (fa.is_int(u) or seed % 2) else "float"
        ns = fa.ns_for(pair, K, kind)
        return agg0, ups, ns, fa.totals(ns)
    return _cached(("data", pair, P, K, seed), make)


def _both(pair, agg0, ups, ns, Ns, what, shifts=(), forms=("call",), kernel="k_fedavg", bufs=None):
    """An init fold and a continuation of the same clients onto ``agg0``, each in every form, against
    the reference."""
    P = len(ups[0])
    bufs = bufs or _upload(pair, ups, shifts)
    want_i = fa.reference(pair, None, ups, ns, Ns)
    want_c = fa.reference(pair, agg0, ups, ns, Ns)
    for form in forms:
        if len(ups) >= 2 or pair not in fa.NO_COPY:
            got = _fold(pair, _agg(pair, P, shifts), bufs, ns, Ns, True, f"{what} init {form}",
                        plan=_waves(pair, len(ups), form), kernel=kernel)
            _same(got, want_i, f"{what} init {form}")
        plan = _waves(("f32", "f32"), len(ups), form)          # a continuation's first wave may be one client
        got = _fold(pair, _agg(pair, P, shifts, agg0), bufs, ns, Ns, False, f"{what} continuation {form}", plan=plan,
                    kernel=kernel)
        _same(got, want_c, f"{what} continuation {form}")


def _untouched(buf):
    bits = buf.full.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[buf.size]).cpu().numpy()
    return bool((bits == bits.dtype.type(SENTINEL[buf.size])).all())


# ---- A. dispatch grid ------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 1], ids=_KERNEL.get)
@pytest.mark.parametrize("init", [True, False], ids=["init", "continuation"])
@pytest.mark.parametrize("pair", fa.PAIRS, ids=_ids)
def test_dispatch_grid(pair, init, shift):
    agg0, ups, ns, Ns = _data(pair, P0, K0)
    shifts = ("all",) if shift else ()
    want = fa.reference(pair, None if init else agg0, ups, ns, Ns)
    assert want.dtype == fa.NP_DT[pair[1]]
    what = f"{pair} init={init} {_KERNEL[shift]}"
    got = _fold(pair, _agg(pair, P0, shifts, None if init else agg0), _upload(pair, ups, shifts), ns, Ns, init, what)
    _same(got, want, what)


@pytest.mark.parametrize("pair", fa.REFUSED, ids=_ids)
def test_refused_pairs(pair):
    from fedn_amd import _abi, ops
    P = 40
    ups = [Buf(P, pair[0]) for _ in range(2)]
    for init in (True, False):
        agg = Buf(P, pair[1])
        with pytest.raises(_abi.FedAggError) as e:
            ops.fedavg_fold(agg.t, [u.t for u in ups], [3, 4], [3, 7], init=init)
        assert e.value.status == _abi.FA_EDTYPE
        torch.cuda.synchronize()
        assert _untouched(agg)


@pytest.mark.parametrize("shift", [0, 1], ids=_KERNEL.get)
@pytest.mark.parametrize("pair", fa.PAIRS, ids=_ids)
def test_single_client(pair, shift):
    """K = 1 with init: a bitwise copy (NaN payloads included) where the dtypes are equal, FA_EDTYPE where
    the pair has no such copy; K = 1 as a continuation folds."""
    from fedn_amd import _abi, ops
    c = fa.special_columns(pair, 2)
    y = fa.tile(c.ups[0], 1027)
    shifts = ("all",) if shift else ()
    bufs = _upload(pair, [y], shifts)
    agg = _agg(pair, len(y), shifts)
    if pair in fa.NO_COPY:
        with pytest.raises(_abi.FedAggError) as e:
            ops.fedavg_fold(agg.t, [bufs[0].t], [5], [5], init=True)
        assert e.value.status == _abi.FA_EDTYPE
        torch.cuda.synchronize()
        assert _untouched(agg)
    else:
        ops.fedavg_fold(agg.t, [bufs[0].t], [5], [5], init=True)
        torch.cuda.synchronize()
        agg.check(f"{pair} copy", True)
        bufs[0].check_unchanged(f"{pair} copy source")
        assert np.array_equal(agg.bits(), bufs[0].bits0)
    agg0, ups, ns, Ns = _data(pair, 1027, 1)
    got = _fold(pair, _agg(pair, 1027, shifts, agg0), _upload(pair, ups, shifts), [7], [12], False, f"{pair} K=1 continuation")
    _same(got, fa.reference(pair, agg0, ups, [7], [12]), f"{pair} K=1 continuation")


@pytest.mark.parametrize("pair", fa.PAIRS, ids=_ids)
def test_empty_calls(pair):
    from fedn_amd import ops
    agg = Buf(40, pair[1])
    ops.fedavg_fold(agg.t, [], [], [], init=False)                       # K = 0
    ups = [Buf(0, pair[0]) for _ in range(2)]
    empty = Buf(0, pair[1])
    for init in (True, False):
        ops.fedavg_fold(empty.t, [u.t for u in ups], [3, 4], [3, 7], init=init)      # P = 0
    torch.cuda.synchronize()
    assert _untouched(agg) and _untouched(empty) and all(_untouched(u) for u in ups)


# ---- B. element map --------------------------------------------------------------------------------
def _sizes(E):
    return sorted({1, E - 1, E, E + 1, 255 * E + 1, 256 * E, 256 * E + 3, 3 * 256 * E + E + 1} - {0})


SCALAR_SIZES = [1, 255, 257, 1027]


@pytest.mark.parametrize("K", [3, 10])
@pytest.mark.parametrize("pair", fa.PAIRS, ids=_ids)
def test_element_map(pair, K):
    E = fa.E_OF[pair]
    agg0, ups, ns, Ns = _data(pair, max(_sizes(E)), K, seed=1)
    for shift, sizes in ((0, _sizes(E)), (1, SCALAR_SIZES)):
        for P in sizes:
            _both(pair, agg0[:P], [u[:P] for u in ups], ns, Ns, f"{pair} K={K} P={P} {_KERNEL[shift]}",
                  ("all",) if shift else ())


# ---- C. client loop and launch split ---------------------------------------------------------------
KS = [2, 3, 8, 9, 10, 11, 17, 64, 65, 66, 129]


@pytest.mark.parametrize("shift", [0, 1], ids=_KERNEL.get)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("pair", fa.PAIRS, ids=_ids)
def test_client_loop_and_launch_split(pair, K, shift):
    agg0, ups, ns, Ns = _data(pair, P0, K, seed=2 + K)
    _both(pair, agg0, ups, ns, Ns, f"{pair} K={K} {_KERNEL[shift]}", ("all",) if shift else (), forms=("call", "waves"))


def test_wave_plans():
    """One call and waves cover: a first wave of one client (the copy) and of two, continuations of 1, 1, 8
    and the rest, and in one call a second launch of 1 and of 2 clients behind the 64-entry table."""
    assert _waves(("f32", "f32"), 129, "waves") == [(0, 1), (1, 2), (2, 3), (3, 11), (11, 129)]
    assert _waves(("i32", "f64"), 129, "waves") == [(0, 2), (2, 3), (3, 4), (4, 12), (12, 129)]
    assert _waves(("i64", "f64"), 2, "waves") == [(0, 2)] and _waves(("f16", "f16"), 2, "waves") == [(0, 1), (1, 2)]
    assert {K - 64 for K in KS if 64 < K <= 128} >= {1, 2} and 9 in KS and 10 in KS
    for pair in fa.PAIRS:
        for K in KS:
            plan = _waves(pair, K, "waves")
            assert plan[0][0] == 0 and plan[-1][1] == K and all(a[1] == b[0] for a, b in zip(plan, plan[1:]))


# ---- D. single-buffer misalignment -----------------------------------------------------------------
@pytest.mark.parametrize("pair", fa.PAIRS, ids=_ids)
def test_single_buffer_misalignment(pair):
    K = 70
    agg0, ups, ns, Ns = _data(pair, P0, K, seed=3)
    want_i = fa.reference(pair, None, ups, ns, Ns)
    want_c = fa.reference(pair, agg0, ups, ns, Ns)
    for name in ("agg", "u0", "u1", f"u{K - 1}", "u65"):
        bufs = _upload(pair, ups, (name,))
        assert sum(b.t.data_ptr() % 16 != 0 for b in bufs) == (name != "agg")
        for init, agg0_, want in ((True, None, want_i), (False, agg0, want_c)):
            what = f"{pair} only {name} shifted init={init}"
            agg = _agg(pair, P0, (name,), agg0_)
            assert (agg.t.data_ptr() % 16 != 0) == (name == "agg")
            _same(_fold(pair, agg, bufs, ns, Ns, init, what), want, what)


# ---- E. special columns ----------------------------------------------------------------------------
def _special_cases():
    return [(p, k) for p in fa.PAIRS for k in fa.kinds(p)]


@pytest.mark.parametrize("K", [2, 5, 65])
@pytest.mark.parametrize("pair,kind", _special_cases(), ids=lambda v: v if isinstance(v, str) else _ids(v))
def test_special_columns(pair, kind, K):
    c = fa.special_columns(pair, K, kind)
    assert len(c.names) < P0 // 2                    # every column at least twice, also in the last block
    ups = [fa.tile(u, P0) for u in c.ups]
    want = fa.reference(pair, None, ups, c.ns, c.Ns)
    first = fa.reference(pair, None, ups[:2], c.ns[:2], c.Ns[:2])      # the step the fixed:* columns are written for
    for shift in (0, 1):
        shifts = ("all",) if shift else ()
        bufs = _upload(pair, ups, shifts)
        what = f"{pair} {kind} K={K} {_KERNEL[shift]}"
        _same(_fold(pair, _agg(pair, P0, shifts), bufs, c.ns, c.Ns, True, what), want, what)
        if K > 2:
            # a first wave of clients 0 and 1: compared right after the first step, before later clients
            # (n close to N in the "big" lists) wash a wrong ulp out; then the rest as a continuation
            def after(k1, got):
                if k1 == 2:
                    _same(got, first, what + " first wave")
            _same(_fold(pair, _agg(pair, P0, shifts), bufs, c.ns, c.Ns, True, what + " waves", plan=[(0, 2), (2, K)],
                        after=after), want, what + " waves")
        else:
            _same(want, first, what)


@pytest.mark.parametrize("pair,kind", _special_cases(), ids=lambda v: v if isinstance(v, str) else _ids(v))
def test_special_columns_in_ragged_strips(pair, kind):
    """Every special column through ``k_fedavg_tail`` and ``strip_start``'s ragged arms: E - 1 columns per
    call at a 16-B aligned address (so the call takes the vector launch and its only strip is ragged), the
    element behind them a sentinel that must stay one. Init (INT_FIRST for integers) and continuation."""
    from fedn_amd import ops
    K, E = 5, fa.E_OF[pair]
    c = fa.special_columns(pair, K, kind)
    C = len(c.names)
    n = E - 1
    chunks = (C + n - 1) // n
    pos = np.array([(i // n) * E + i % n for i in range(C)])

    def spread(a):
        out = np.zeros(chunks * E, a.dtype)
        out[pos] = a
        return out
    bufs = _upload(pair, [spread(u) for u in c.ups])
    want = fa.reference(pair, None, c.ups, c.ns, c.Ns)
    agg = _agg(pair, chunks * E)
    for j in range(chunks):
        ops.fedavg_fold(agg.t[j * E:j * E + n], [b.t[j * E:j * E + n] for b in bufs], c.ns, c.Ns, init=True)
        assert ops.last_kernel() == "k_fedavg"
    torch.cuda.synchronize()
    agg.check(f"{pair} {kind} ragged", False)
    got = agg.numpy()
    _same(got[pos], want, f"{pair} {kind} ragged init")
    pad = np.arange(chunks) * E + n                   # the element behind each call's ragged strip
    sent = agg.bits()[pad]
    assert (sent == sent.dtype.type(SENTINEL[agg.size])).all(), f"{pair} {kind}: the element behind a ragged strip was written"
    first = fa.reference(pair, None, c.ups[:2], c.ns[:2], c.Ns[:2])
    cont = _agg(pair, chunks * E, (), spread(first))
    for j in range(chunks):
        ops.fedavg_fold(cont.t[j * E:j * E + n], [b.t[j * E:j * E + n] for b in bufs[2:]], c.ns[2:], c.Ns[2:], init=False)
    torch.cuda.synchronize()
    cont.check(f"{pair} {kind} ragged continuation", False)
    _same(cont.numpy()[pos], want, f"{pair} {kind} ragged continuation")
    assert np.array_equal(cont.bits()[pad], cont.bits0[pad])
    for k, b in enumerate(bufs):
        b.check_unchanged(f"{pair} {kind} ragged updates[{k}]")


@pytest.mark.parametrize("shift", [0, 1], ids=_KERNEL.get)
def test_division_by_large_totals(shift):
    """|N| >= 2^28 must divide (r == 0): ties of t / N between f32 subnormals with |t| >= 2^-98, which no redo
    covers and the reciprocal rounds the other way (fedavg_cases.large_total_ties)."""
    ups, ns = fa.large_total_ties()
    ups = [fa.tile(u, 1027) for u in ups]
    pair = ("f32", "f32")
    shifts = ("all",) if shift else ()
    want = fa.reference(pair, None, ups, ns, fa.totals(ns))
    _same(_fold(pair, _agg(pair, 1027, shifts), _upload(pair, ups, shifts), ns, fa.totals(ns), True, "large totals"), want,
          "large totals")


# ---- F. the other carriers of the fp32 fold --------------------------------------------------------
def _f32_cases(P):
    """(name, agg0, ups, ns, Ns) for the carriers: the f32 special columns at K = 5 (8 clients in flight in the
    small geometries), 12 (4 in flight) and 70 (a second launch), every ns list; ordinary data over section
    C's K list; the large-total ties."""
    def make():
        pair = ("f32", "f32")
        out = []
        for K in (5, 12, 70):
            for kind in fa.kinds(pair):
                c = fa.special_columns(pair, K, kind)
                ups = [fa.tile(u, P) for u in c.ups]
                agg0 = fa.tile(fa.reference(pair, None, c.ups[:2], c.ns[:2], c.Ns[:2]), P)
                out.append((f"special K={K} {kind}", agg0, ups, c.ns, c.Ns))
        for K in KS:
            agg0, ups, ns, Ns = _data(pair, P, K, seed=2 + K)
            out.append((f"ordinary K={K}", agg0, ups, ns, Ns))
        ups, ns = fa.large_total_ties()
        ups = [fa.tile(u, P) for u in ups]
        out.append(("large totals", ups[1], ups, ns, fa.totals(ns)))
        return out
    return _cached(("f32 cases", P), make)


def _case_ids(P):
    pair = ("f32", "f32")
    return [f"special-K{K}-{kind}" for K in (5, 12, 70) for kind in fa.kinds(pair)] + [f"ordinary-K{K}" for K in KS] + ["large-totals"]


@pytest.mark.parametrize("i", range(len(_case_ids(P0))), ids=_case_ids(P0))
def test_push_carries_the_f32_fold(i):
    """``ops.fedavg_fold_push`` with two destinations, init and continuation: agg and both destinations equal
    the reference; their guards, and the updates, are unchanged."""
    from fedn_amd import ops
    pair = ("f32", "f32")
    name, agg0, ups, ns, Ns = _f32_cases(P0)[i]
    bufs = _upload(pair, ups)
    st = torch.cuda.current_stream(DEV)
    for init in (True, False):
        agg = _agg(pair, P0, (), None if init else agg0)
        dsts = [Buf(P0, "f32") for _ in range(2)]
        ran = ops.fedavg_fold_push(agg.t.data_ptr(), [b.t.data_ptr() for b in bufs], ns, Ns, P0, init,
                                   [d.t.data_ptr() for d in dsts], st, torch.device(DEV))
        assert ran
        torch.cuda.synchronize()
        want = fa.reference(pair, None if init else agg0, ups, ns, Ns)
        for t, what in [(agg, "agg")] + [(d, f"destination {j}") for j, d in enumerate(dsts)]:
            t.check(f"push {name} init={init} {what}", True)
            _same(t.numpy(), want, f"push {name} init={init} {what}")
        for k, b in enumerate(bufs):
            b.check_unchanged(f"push {name} updates[{k}]")


@pytest.mark.parametrize("lanetab", [0, 1], ids=["kernarg-table", "lane-table"])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("i", range(len(_case_ids(P_PIPE))), ids=_case_ids(P_PIPE))
def test_pipelined_geometry_carries_the_f32_fold(i, dt, lanetab):
    """The pipelined geometry forced small through the probe library (the product takes it from 160 MiB per
    client): two whole tiles and a ragged one (``k_fedavg_tail`` over a whole tile's width), the client
    table from the kernel argument and from ``LaneTable``'s lanes. The bf16 columns are the f32 ones
    through ``to_bf16`` (test_fedavg_cases_host.py::test_bf16_rounding_of_the_f32_columns)."""
    from fedn_amd import _abi, ops
    name, agg0, ups, ns, Ns = _f32_cases(P_PIPE)[i]
    pair = (dt, "f32")
    if dt == "bf16":
        ups = [fa.to_bf16(u) for u in ups]
    bufs = _upload(pair, ups)
    with _abi.use_probe():
        ops.tune(auto_geom=0, lanetab=lanetab)
        try:
            _both(pair, agg0, ups, ns, Ns, f"pipelined {dt} {name}", kernel="k_fedavg_pipe", bufs=bufs)
        finally:
            ops.tune(auto_geom=1, lanetab=0)
    _both(pair, agg0, ups, ns, Ns, f"product {dt} {name}", bufs=bufs)          # the product's geometry: the same bits


# ---- G. the int32 multiplier -----------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 1], ids=_KERNEL.get)
@pytest.mark.parametrize("n1", [2 ** 31 - 1, 2 ** 31, -2 ** 31, -2 ** 31 - 1])
def test_int32_multiplier(n1, shift):
    """numpy multiplies the first integer difference by n[1] in int32 and raises OverflowError for a python
    int outside it: inside, the fold matches; outside, it is refused (FA_EINVAL) and nothing is written."""
    from fedn_amd import _abi, ops
    pair = ("i32", "f64")
    c = fa.special_columns(pair, 2, "plain")
    ups = [fa.tile(u, 1027) for u in c.ups]
    ns = [5, n1]
    Ns = fa.totals(ns)
    shifts = ("all",) if shift else ()
    bufs = _upload(pair, ups, shifts)
    agg = _agg(pair, 1027, shifts)
    if -2 ** 31 <= n1 < 2 ** 31:
        want = fa.reference(pair, None, ups, ns, Ns)
        _same(_fold(pair, agg, bufs, ns, Ns, True, f"n1={n1}"), want, f"n1={n1}")
    else:
        with pytest.raises(OverflowError):
            fa.reference(pair, None, ups, ns, Ns)
        with pytest.raises(_abi.FedAggError) as e:
            ops.fedavg_fold(agg.t, [b.t for b in bufs], ns, Ns, init=True)
        assert e.value.status == _abi.FA_EINVAL and "int32" in str(e.value)
        torch.cuda.synchronize()
        assert _untouched(agg)
        # a continuation multiplies in float64: no such limit
        agg0 = ups[0].astype(np.float64)
        got = _fold(pair, _agg(pair, 1027, shifts, agg0), bufs[1:], ns[1:], Ns[1:], False, f"n1={n1} continuation")
        _same(got, fa.reference(pair, agg0, ups[1:], ns[1:], Ns[1:]), f"n1={n1} continuation")


def test_plugin_skips_int32_overflow():
    """A round of the plug-in on an int32 model whose second client has n = 2^31: the reference's fold raises
    for that update, skips it and keeps its examples counted (fedavg.py:75-78); the refused launch goes
    through the per-update failure isolation to the same model and count."""
    from fedn_amd.aggregators import get_aggregator
    from fedn_amd.updatehandler import MemoryUpdateHandler
    rng = np.random.default_rng(5)
    shapes = [(37, 5), (11,)]
    updates = [([rng.integers(-10 ** 6, 10 ** 6, s).astype(np.int32) for s in shapes], n) for n in (7, 2 ** 31, 12)]
    want, nr = ref.fedavg_combine(updates)
    assert nr == 2 and want[0].dtype == np.float64
    uh = MemoryUpdateHandler()
    for arrays, n in updates:
        uh.submit(arrays, n)
    model, data = get_aggregator("fedavg", uh).combine_models(helper=None, delete_models=True, parameters=None)
    assert data["nr_aggregated_models"] == nr
    assert_lists_identical(model, want, "int32 model, n = 2^31 in the middle")
