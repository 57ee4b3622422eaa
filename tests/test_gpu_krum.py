"""Krum / Multi-Krum on the GPU: ``fa_pairwise_sqdist`` (kernel ``k_pair_sqdist``) through
``ops.pairwise_sqdist``, ``robust.RobustPipeline.select_mean`` and the ``multikrum`` / ``krum`` plug-ins,
against the oracle tests/krum_ref.py: distances within ``ops.sqdist_rtol`` of the exact sums, the same
bits on every call and at every alignment, selections equal, models bit for bit."""
import numpy as np
import pytest
import torch

import krum_ref as kr
from golden_io import assert_lists_identical
from robust_fuzz_cases import krum_gaps, round_updates, selection_bound

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KS = [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64]        # every KP, K = KP, K = KP + 1, padding at its most
PS = [1, 5, 257, 4099, 65539]
DTYPES = ["f32", "f64", "f16", "bf16", "i32", "i64"]
NP_DT = {"f32": np.float32, "f64": np.float64, "f16": np.float16, "bf16": np.float32, "i32": np.int32, "i64": np.int64}
TORCH_DT = {"f32": torch.float32, "f64": torch.float64, "f16": torch.float16, "bf16": torch.bfloat16,
            "i32": torch.int32, "i64": torch.int64}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from fedn_amd import _abi
    _abi.load()
    yield
    # This module's largest test holds about 1 GB at once. empty_cache() returns every cached block to
    # the driver, those of earlier modules included: the modules after this one start from an empty
    # pool, the state the modules that depend on the pool's contents put themselves in anyway
    # (test_gpu_stream_order before every test, test_gpu_parity and others at their large sizes).
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _bf16_exact(x):
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def _data(rng, name, K, n):
    """K updates that are close to each other, as in federated learning: a base plus small noise."""
    dt = np.dtype(NP_DT[name])
    base = rng.standard_normal(n)
    x = base + 0.05 * rng.standard_normal((K, n))
    if dt.kind == "i":
        scale = 2.0 ** 20 if name == "i32" else 2.0 ** 40
        x = np.round(x * scale).astype(dt)
        if name == "i64":                                     # not exact in float64: converted with one rounding
            q = max(1, n // 8)
            x[:, :q] = (2 ** 53 + rng.integers(1, 1000, (K, q))) * rng.choice([-1, 1], (1, q))
        return np.ascontiguousarray(x)
    x = x.astype(dt)
    return _bf16_exact(x) if name == "bf16" else np.ascontiguousarray(x)


def _upload(S, name):
    t = torch.from_numpy(np.ascontiguousarray(S)).to(DEV)
    return t.to(torch.bfloat16) if name == "bf16" else t       # exact: the values are bf16's


def _row_len(n):
    return -(-n // 64) * 64                                    # rows of a (K, row) matrix stay 16-B aligned


def _check(got, want, rtol, what):
    """Every entry within rtol of the reference, relatively; exactly symmetric; a zero diagonal."""
    assert got.dtype == np.float64 and got.shape == want.shape, (what, got.dtype, got.shape)
    assert np.array_equal(got, got.T), f"{what}: not symmetric"
    assert (np.diag(got) == 0).all() and not np.signbit(np.diag(got)).any(), f"{what}: diagonal"
    assert np.isfinite(got).all(), f"{what}: non-finite entries"
    err = np.abs(got - want)
    rel = np.where(want > 0, err / np.where(want > 0, want, 1.0), err)
    worst = float(rel.max()) if rel.size else 0.0
    print(f"{what}: worst relative error {worst:.3e} (bound {rtol:.3e})")
    assert (err <= rtol * want).all(), f"{what}: relative error {worst:.3e} exceeds {rtol:.3e}"


# ---- ops level: the matrix -----------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", DTYPES)
def test_ops_pairwise_sqdist_matrix(name, K):
    from fedn_amd import ops
    te, R, _, _ = ops.sqdist_geometry(TORCH_DT[name], K)
    assert R <= 1024
    sizes = sorted(set(PS + [te - 1, te, te + 1]))
    rng = np.random.default_rng(1000 * DTYPES.index(name) + K)
    S = _data(rng, name, K, _row_len(sizes[-1]))
    want = kr.sqdist_prefixes(S, sizes)                        # one pass for every P
    dev = _upload(S, name)
    for P in sizes:
        D = ops.pairwise_sqdist([dev[k, :P] for k in range(K)])
        assert ops.last_kernel() == "k_pair_sqdist"
        assert D.shape == (K, K) and D.dtype == torch.float64 and D.device == dev.device
        _check(D.cpu().numpy(), want[P], ops.sqdist_rtol(TORCH_DT[name], P), f"{name} K={K} P={P}")


@pytest.mark.parametrize("name", DTYPES)
def test_ops_every_workgroup_two_tiles_and_a_ragged_one(name):
    """K = 4 at a size where the grid is at its cap, every workgroup walks at least two tiles and the
    last tile is ragged."""
    from fedn_amd import ops
    K = 4
    te, _, grid, _ = ops.sqdist_geometry(TORCH_DT[name], K)
    P = 2 * grid * te + te // 2 + 3
    rng = np.random.default_rng(50 + DTYPES.index(name))
    S = _data(rng, name, K, _row_len(P))
    dev = _upload(S, name)
    D = ops.pairwise_sqdist([dev[k, :P] for k in range(K)])
    _check(D.cpu().numpy(), kr.sqdist(S[:, :P]), ops.sqdist_rtol(TORCH_DT[name], P), f"{name} K={K} P={P}")


@pytest.mark.parametrize("name,K", [("f16", 33), ("f16", 9), ("i32", 33)])
def test_ops_chains_flushed_mid_kernel(name, K):
    """A size at which every workgroup walks more tiles than it may sum in one chain, so the chains are
    flushed to f64 in mid-kernel as well as at the end. The updates are constants (client k holds k / 2
    everywhere): every term and every partial sum is exact in f32 and f64, so D[i][j] is EXACTLY
    P (i - j)^2 / 4 — an element dropped or counted twice shows. Then on random data the one call agrees
    with the sum of pieces too short for a mid-kernel flush (the path the matrix test pins)."""
    from fedn_amd import ops
    te, _, grid, flush_tiles = ops.sqdist_geometry(TORCH_DT[name], K)
    P = grid * te * (flush_tiles + 1) + te // 2 + 3
    scale = 0.5 if name == "f16" else 1
    ups = [torch.full((P,), k * scale, dtype=TORCH_DT[name], device=DEV) for k in range(K)]
    got = ops.pairwise_sqdist(ups).cpu().numpy()
    idx = np.arange(K, dtype=np.float64)
    want = P * ((idx[:, None] - idx[None, :]) * scale) ** 2
    assert np.array_equal(got, want), f"{name} K={K} P={P}: worst {np.abs(got - want).max()}"
    gen = torch.Generator(device=DEV).manual_seed(K)
    base = torch.randn(P, generator=gen, device=DEV)
    for k in range(K):                                           # (reusing the buffers: K x P is large)
        noise = torch.randn(P, generator=gen, device=DEV).mul_(0.05).add_(base)
        ups[k].copy_(noise.mul_(1000) if name == "i32" else noise)
    del base, noise
    one = ops.pairwise_sqdist(ups).cpu().numpy()
    piece = grid * te * flush_tiles // 2 // 64 * 64             # at most half the tiles a flush takes
    acc = torch.zeros((K, K), dtype=torch.float64, device=DEV)
    for lo in range(0, P, piece):
        ops.pairwise_sqdist([u[lo:lo + piece] for u in ups], out=acc, accumulate=True)
    acc = acc.cpu().numpy()
    rtol = ops.sqdist_rtol(TORCH_DT[name], P)
    off = ~np.eye(K, dtype=bool)
    print(f"{name} K={K} P={P}: one call vs pieces, worst relative difference "
          f"{float((np.abs(one - acc)[off] / acc[off]).max()):.3e} (bound {2 * rtol:.3e})")
    assert np.isfinite(one).all() and np.array_equal(one, one.T) and (np.diag(one) == 0).all()
    assert (np.abs(one - acc) <= 2 * rtol * acc).all(), "both are within the bound of the exact sums"


def test_ops_empty_and_single():
    """P = 0 and K = 1 still write their zeros when the matrix is written, and add nothing when it is
    accumulated into."""
    from fedn_amd import ops
    for name in DTYPES:
        for K in (1, 3, 64):
            out = torch.full((K, K), 7.0, dtype=torch.float64, device=DEV)
            ups = [torch.empty(0, dtype=TORCH_DT[name], device=DEV) for _ in range(K)]
            assert ops.pairwise_sqdist(ups, out=out) is out
            assert (out.cpu().numpy() == 0).all(), (name, K)
            out.fill_(7.0)
            ops.pairwise_sqdist(ups, out=out, accumulate=True)
            assert (out.cpu().numpy() == 7).all(), (name, K)
        one = _upload(_data(np.random.default_rng(1), name, 1, 4160), name)
        D = ops.pairwise_sqdist([one[0, :4099]])
        assert D.shape == (1, 1) and D.item() == 0.0


def test_ops_refuses_bad_arguments():
    from fedn_amd import ops
    x = torch.zeros(8, device=DEV)
    with pytest.raises(ValueError):
        ops.pairwise_sqdist([])
    with pytest.raises(ValueError):
        ops.pairwise_sqdist([x] * 65)
    with pytest.raises(ValueError):
        ops.pairwise_sqdist([x, torch.zeros(9, device=DEV)])                          # lengths differ
    with pytest.raises(TypeError):
        ops.pairwise_sqdist([x, torch.zeros(8, dtype=torch.float64, device=DEV)])     # dtypes differ
    with pytest.raises(TypeError):
        ops.pairwise_sqdist([torch.zeros(8, dtype=torch.int8, device=DEV)] * 2)       # not one of the six
    with pytest.raises(ValueError):
        ops.pairwise_sqdist([x, x], out=torch.zeros(5, dtype=torch.float64, device=DEV))
    with pytest.raises(TypeError):
        ops.pairwise_sqdist([x, x], out=torch.zeros(4, dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError):
        ops.pairwise_sqdist([x, x], accumulate=True)                                  # nothing to add to
    with pytest.raises(ValueError):
        ops.pairwise_sqdist([x, x.cpu()])
    with pytest.raises(TypeError):
        ops.sqdist_rtol(torch.int8, 10)
    assert ops.sqdist_rtol(torch.float32, 10) == ops.sqdist_rtol(np.float16, 10 ** 9) <= 6.2e-5
    assert ops.sqdist_rtol(torch.int64, 60) == 64 * 2.0 ** -53


# ---- the same bits ---------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [3, 8, 17, 64])
@pytest.mark.parametrize("name", DTYPES)
def test_same_bits_every_call_and_alignment(name, K):
    from fedn_amd import ops
    te, _, _, _ = ops.sqdist_geometry(TORCH_DT[name], K)
    n = _row_len(2 * te + 70)
    dev = _upload(_data(np.random.default_rng(7 + K), name, K, n), name)
    for P in (5, te - 1, te + 1, 2 * te + 9):
        shifted = [dev[k, 1:1 + P] for k in range(K)]           # one element past a 16-B boundary
        assert all(v.data_ptr() % 16 for v in shifted)
        aligned = [v.clone() for v in shifted]
        assert not any(v.data_ptr() % 16 for v in aligned)
        a = ops.pairwise_sqdist(aligned).cpu().numpy()
        b = ops.pairwise_sqdist(aligned).cpu().numpy()
        c = ops.pairwise_sqdist(shifted).cpu().numpy()
        mixed = [s if k % 2 else v for k, (s, v) in enumerate(zip(shifted, aligned))]
        d = ops.pairwise_sqdist(mixed).cpu().numpy()
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), f"{name} K={K} P={P}: two calls differ"
        assert np.array_equal(a.view(np.uint64), c.view(np.uint64)), f"{name} K={K} P={P}: unaligned views differ"
        assert np.array_equal(a.view(np.uint64), d.view(np.uint64)), f"{name} K={K} P={P}: mixed alignment differs"


@pytest.mark.parametrize("name", DTYPES)
def test_accumulate_over_two_halves(name):
    from fedn_amd import ops
    K, P = 9, 65539
    S = _data(np.random.default_rng(21), name, K, _row_len(P))
    dev = _upload(S, name)
    h = 32768
    first, second = [dev[k, :h] for k in range(K)], [dev[k, h:P] for k in range(K)]
    one = ops.pairwise_sqdist([dev[k, :P] for k in range(K)]).cpu().numpy()
    d1 = ops.pairwise_sqdist(first).cpu().numpy()
    d2 = ops.pairwise_sqdist(second).cpu().numpy()
    acc = torch.full((K, K), 7.0, dtype=torch.float64, device=DEV)
    ops.pairwise_sqdist(first, out=acc)                          # written: the 7s are gone
    ops.pairwise_sqdist(second, out=acc, accumulate=True)
    acc = acc.cpu().numpy()
    assert np.array_equal(acc.view(np.uint64), (d1 + d2).view(np.uint64)), "accumulate is the f64 sum of the two calls"
    rtol = ops.sqdist_rtol(TORCH_DT[name], P)
    # both halves are within their bounds of their exact sums, the one add is rounded once: the total is
    # within the whole model's bound of the exact total, and so within twice the bound of the one call
    _check(acc, kr.sqdist(S[:, :P]), rtol, f"{name} accumulated")
    assert (np.abs(acc - one) <= 2 * rtol * one).all()


# ---- bounds ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [4, 5, 9, 17, 33])
@pytest.mark.parametrize("name", ["f32", "f16", "f64", "i32"])
def test_nothing_outside_the_windows(name, K):
    """Every update sits inside a larger buffer between sentinels that would wreck the distances if read,
    D is a K x K window of a larger sentinel-filled buffer: the result is the K-exact reference's (padded
    clients contribute nothing) and nothing outside the window changes."""
    from fedn_amd import ops
    te, _, _, _ = ops.sqdist_geometry(TORCH_DT[name], K)
    guard = 64
    sentinel = {"f32": 3e30, "f16": 6e4, "f64": 1e300, "i32": 2 ** 31 - 1}[name]
    for P in (257, te + 1):
        for off in (0, 1):
            S = _data(np.random.default_rng(K + P), name, K, P)
            big = np.full((K, guard + off + P + guard), sentinel, dtype=NP_DT[name])
            big[:, guard + off:guard + off + P] = S
            dev = _upload(big, name)
            before = dev.clone()
            out = torch.full((K * K + 2 * guard,), -5.0, dtype=torch.float64, device=DEV)
            win = out[guard:guard + K * K]
            ops.pairwise_sqdist([dev[k, guard + off:guard + off + P] for k in range(K)], out=win)
            o = out.cpu().numpy()
            assert (o[:guard] == -5).all() and (o[guard + K * K:] == -5).all(), (name, K, P, off)
            _check(o[guard:guard + K * K].reshape(K, K), kr.sqdist(S), ops.sqdist_rtol(TORCH_DT[name], P),
                   f"{name} K={K} P={P} off={off}")
            assert torch.equal(dev, before), "the updates are read only"


# ---- specials --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["f32", "bf16", "f16", "f64"])
def test_specials(name):
    """One client with an inf, one with a NaN, one whose squared difference overflows the compute type:
    their rows and columns are non-finite, every other entry is what it is without them, bit for bit."""
    from fedn_amd import ops
    K, P = 7, 4099
    S = _data(np.random.default_rng(31), name, K, _row_len(P))
    bad = {1: np.inf, 3: np.nan}
    if name != "f16":                                            # (f16's range squares into f32 without overflow)
        bad[4] = {"f32": 1e20, "bf16": 1e20, "f64": 1e200}[name]
    T = S.copy()
    for k, v in bad.items():
        T[k, 1000 + k] = v
    if name == "bf16":
        T = _bf16_exact(T)
    Z = S.copy()
    for k in bad:
        Z[k, :] = 0
    got = ops.pairwise_sqdist([r[:P] for r in _upload(T, name)]).cpu().numpy()    # returns: FA_OK
    ref = ops.pairwise_sqdist([r[:P] for r in _upload(Z, name)]).cpu().numpy()
    good = [k for k in range(K) if k not in bad]
    for k in bad:
        others = [j for j in range(K) if j != k]
        assert not np.isfinite(got[k, others]).any() and not np.isfinite(got[others, k]).any(), (name, k, got[k])
        assert got[k, k] == 0
    sub = np.ix_(good, good)
    assert np.array_equal(got[sub].view(np.uint64), ref[sub].view(np.uint64)), "the other entries are unaffected"
    _check(got[sub], kr.sqdist(S[good, :P]), ops.sqdist_rtol(TORCH_DT[name], P), f"{name} specials, good clients")


# ---- plug-in rounds --------------------------------------------------------------------------------
ROUNDS = [(4, 257), (5, 257), (10, 4099), (17, 4099), (64, 4099)]
# seeds for which the score gaps at the selection boundaries are at least 10 x the distance bound (the
# precondition _selection asserts): found on the CPU with the oracle alone
SEEDS = {(4, 257): 0, (5, 257): 0, (10, 4099): 0, (17, 4099): 0, (64, 4099): 0}
FRACTION = 0.2


def _round_updates(seed, K, spec, fraction=FRACTION):
    """K updates of the model ``spec`` with f = byzantine_count(fraction, K) hostile ones: the generator the
    robust rules' tests share (tests/robust_fuzz_cases.round_updates). Returns (updates, hostile indices)."""
    return round_updates(seed, K, kr.byzantine_count(fraction, K), spec)


def _selection(ups, m, what):
    """The oracle's selection, after asserting the precondition in float64 on the CPU: the relative
    score gaps between the best and second-best client and between the m-th and (m+1)-th are at least
    10 x the distance bound, so the kernel's rounding cannot change the selection (the gaps and their one
    structural exception, at K <= 3: tests/robust_fuzz_cases.krum_gaps)."""
    K = len(ups)
    f = kr.byzantine_count(FRACTION, K)
    D = kr.model_distances(ups)
    bound = selection_bound(ups)
    gaps = krum_gaps(D, f, m)
    print(f"{what}: score gaps {gaps}, needed {bound:.2e}")
    assert all(g >= bound for g in gaps), f"{what}: precondition — score gaps {gaps} below {bound:.2e}: pick another seed"
    return f, kr.select(D.tolist(), f, m)


def _run_round(agg_name, ups, staged, parameters=None, budget=None, agg=None, uh=None):
    from fedn_amd.aggregators import get_aggregator
    from fedn_amd.ingest import StagingUpdateHandler
    from fedn_amd.updatehandler import MemoryUpdateHandler
    uh = uh or MemoryUpdateHandler()
    st = StagingUpdateHandler(uh, helper=None, device=DEV, workers=2) if staged else None
    try:
        if agg is None:
            agg = get_aggregator(agg_name, st or uh)
            agg.device, agg.hbm_budget = torch.device(DEV), budget
        mus = [uh.submit(u, 10 + k, via=st) for k, u in enumerate(ups)]
        model, data = agg.combine_models(helper=None, parameters=parameters)
    finally:
        if st is not None:
            st.close()
    return model, data, uh, mus, agg


@pytest.mark.parametrize("staged", [False, True], ids=["host", "staged"])
@pytest.mark.parametrize("K,P", ROUNDS)
@pytest.mark.parametrize("agg_name", ["multikrum", "krum"])
def test_plugin_round(agg_name, K, P, staged):
    spec = [((P,), np.float32), ((P // 4 + 3,), np.int32)]       # two dtype groups: f32 and i32
    ups, hostile = _round_updates(SEEDS[(K, P)], K, spec)
    f = kr.byzantine_count(FRACTION, K)
    assert len(hostile) == f
    m = K - f if agg_name == "multikrum" else 1
    _, want_sel = _selection(ups, m, f"{agg_name} K={K} P={P}")
    model, data, uh, _, agg = _run_round(agg_name, ups, staged, {"byzantine_fraction": FRACTION})
    assert data["nr_aggregated_models"] == K
    for key in ("time_model_load", "time_model_aggregation", "time_h2d", "time_kernel", "time_pack", "time_d2h"):
        assert key in data
    assert agg.selected == want_sel and len(agg.scores) == K
    assert not set(agg.selected) & set(hostile), "no hostile client is selected"
    assert_lists_identical(model, kr.combine(ups, want_sel), f"{agg_name} K={K} P={P}")
    assert [a.dtype for a in model] == [np.dtype(np.float32), np.dtype(np.float64)]
    assert uh.model_updates.qsize() == 0 and not uh.store.models, "every update is deleted once the result exists"


def test_default_fraction_is_a_fifth():
    """No parameters: byzantine_fraction = 0.2."""
    K, P = 10, 4099
    spec = [((P,), np.float32), ((P // 4 + 3,), np.int32)]
    ups, hostile = _round_updates(SEEDS[(K, P)], K, spec)
    _, want_sel = _selection(ups, K - 2, "default fraction")
    model, data, _, _, agg = _run_round("multikrum", ups, False)
    assert data["nr_aggregated_models"] == K and agg.selected == want_sel and len(want_sel) == 8
    assert_lists_identical(model, kr.combine(ups, want_sel), "default fraction")


@pytest.mark.parametrize("agg_name", ["multikrum", "krum"])
def test_budget_keeps_updates_on_the_host(agg_name, monkeypatch):
    """A budget of 3 updates with K = 12: nine stay on the host, and both passes walk them slice by slice
    through the ring — the same selection and the same model as with everything in HBM."""
    from fedn_amd import robust
    from fedn_amd.budget import HbmBudget
    from fedn_amd.layout import Layout
    K = 12
    spec = [((300, 200), np.float32), ((77,), np.int64), ((1001,), np.float32), ((), np.float32)]
    ups, hostile = _round_updates(0, K, spec)
    f = kr.byzantine_count(FRACTION, K)
    m = K - f if agg_name == "multikrum" else 1
    _, want_sel = _selection(ups, m, f"{agg_name} budget")
    free, data0, _, _, agg0 = _run_round(agg_name, ups, False)
    assert agg0.host_side == 0 and data0["nr_aggregated_models"] == K and agg0.selected == want_sel
    monkeypatch.setattr(robust, "SLICE_BYTES", 16384)
    budget = HbmBudget(limit=3 * Layout.of(ups[0]).nbytes)
    model, data, uh, _, agg = _run_round(agg_name, ups, False, budget=budget)
    assert agg.host_side == 9 and data["nr_aggregated_models"] == K, "every update is counted"
    assert agg.selected == want_sel and not set(agg.selected) & set(hostile)
    assert_lists_identical(model, free, "budgeted vs unbudgeted")
    assert_lists_identical(model, kr.combine(ups, want_sel), "budgeted vs oracle")
    assert not uh.store.models
    del agg, agg0
    import gc
    gc.collect()
    assert budget.used(DEV) == 0, "the round's reservations went back to the budget"


# ---- refusals and failures ---------------------------------------------------------------------------
def test_more_than_64_updates_refused():
    ups, _ = _round_updates(12, 65, [((33,), np.float32)])
    model, data, uh, mus, _ = _run_round("multikrum", ups, False)
    assert model is None and data["nr_aggregated_models"] == 0
    assert uh.model_updates.qsize() == 0
    assert set(uh.store.models) == {m.model_update_id for m in mus}, "nothing is deleted"


@pytest.mark.parametrize("staged", [False, True], ids=["host", "staged"])
def test_layout_mismatch_is_skipped_and_kept(staged):
    K, P = 10, 4099
    spec = [((P,), np.float32), ((P // 4 + 3,), np.int32)]
    ups, hostile = _round_updates(SEEDS[(K, P)], K, spec)
    odd = [np.zeros((5, 3), dtype=np.float32), np.zeros(7, dtype=np.int32)]      # not this round's layout
    queue = ups[:3] + [odd] + ups[3:]
    f, want_sel = _selection(ups, K - 2, "layout mismatch")
    model, data, uh, mus, agg = _run_round("multikrum", queue, staged)
    assert data["nr_aggregated_models"] == K
    assert agg.selected == want_sel, "indices count the admitted updates"
    assert_lists_identical(model, kr.combine(ups, want_sel), "multikrum without the mismatching update")
    assert set(uh.store.models) == {mus[3].model_update_id}, "the skipped update stays in storage"


def test_all_scores_non_finite_keeps_every_update():
    """A NaN in every update: no finite score, nothing to select — (None, data), nothing deleted."""
    ups, _ = _round_updates(5, 6, [((257,), np.float32)])
    for u in ups:
        u[0][3] = np.nan
    model, data, uh, mus, agg = _run_round("krum", ups, False)
    assert model is None and data["nr_aggregated_models"] == 0 and agg.selected is None
    assert set(uh.store.models) == {mu.model_update_id for mu in mus}


def test_failed_launch_keeps_every_update(monkeypatch):
    """A launch that fails (injected at the wrapper: no device fault): the round is (None, data), the
    updates stay in storage, and the aggregator's next round is exact."""
    from fedn_amd import _abi, ops
    K, P = 10, 4099
    spec = [((P,), np.float32), ((P // 4 + 3,), np.int32)]
    ups, _ = _round_updates(SEEDS[(K, P)], K, spec)
    calls = []

    def boom(*a, **kw):
        calls.append(1)
        raise _abi.FedAggError(_abi.FA_EHIP, "pairwise_sqdist: injected failure")

    with monkeypatch.context() as mp:
        mp.setattr(ops, "pairwise_sqdist", boom)
        model, data, uh, mus, agg = _run_round("multikrum", ups, False)
    assert calls and model is None and data["nr_aggregated_models"] == 0
    assert uh.model_updates.qsize() == 0
    assert set(uh.store.models) == {mu.model_update_id for mu in mus}, "every update stays in storage"
    _, want_sel = _selection(ups, K - 2, "after a failed launch")
    model, data, uh, mus2, _ = _run_round("multikrum", ups, False, agg=agg, uh=uh)
    assert data["nr_aggregated_models"] == K and agg.selected == want_sel
    assert_lists_identical(model, kr.combine(ups, want_sel), "the round after a failed launch")
    assert set(uh.store.models) == {mu.model_update_id for mu in mus}
