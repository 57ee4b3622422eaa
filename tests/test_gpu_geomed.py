"""The geometric median on the GPU: ``fa_weighted_mean_sqdist`` (kernel ``k_wmean_dist``) through
``ops.weighted_mean_sqdist``, ``robust.RobustPipeline.geometric_median`` and the ``geomedian`` plug-in,
against the oracle tests/geomed_ref.py: the weighted mean bit for bit, the distances within
``ops.sqdist_rtol`` of the exact sums, the same bits on every call and at every alignment, and the
Weiszfeld chain pinned pass by pass with the pipeline's own trace."""
import gc

import numpy as np
import pytest
import torch

import geomed_ref as gr
from golden_io import assert_lists_identical
from robust_checks import check_geomed_chain as _check_chain
from robust_checks import nan_clients as _nan_clients
from robust_checks import same_bits as _same_bits
from robust_fuzz_cases import round_updates

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KS = [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64]
PS = [1, 5, 257, 4099, 65539]
DTYPES = ["f32", "f64", "f16", "bf16", "i32", "i64"]
NP_DT = {"f32": np.float32, "f64": np.float64, "f16": np.float16, "bf16": np.float32, "i32": np.int32, "i64": np.int64}
TORCH_DT = {"f32": torch.float32, "f64": torch.float64, "f16": torch.float16, "bf16": torch.bfloat16,
            "i32": torch.int32, "i64": torch.int64}
OUT_DT = {"f32": torch.float32, "f64": torch.float64, "f16": torch.float16, "bf16": torch.float32,
          "i32": torch.float64, "i64": torch.float64}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from fedn_amd import _abi
    _abi.load()
    yield
    # the flush test holds a quarter of a GB: the modules after this one start from an empty pool
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


def _beta(rng, K):
    """Random weights that do not sum to 1, one of them 0 (K > 1)."""
    beta = rng.uniform(0.05, 1.0, K)
    if K > 1:
        beta[int(rng.integers(0, K))] = 0.0
    return beta.tolist()


def _check_d(got, want, rtol, what):
    """Every distance within rtol of the reference, relatively."""
    assert got.dtype == np.float64 and got.shape == want.shape, (what, got.dtype, got.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite distances {got}"
    err = np.abs(got - want)
    rel = np.where(want > 0, err / np.where(want > 0, want, 1.0), err)
    worst = float(rel.max()) if rel.size else 0.0
    print(f"{what}: worst relative error {worst:.3e} (bound {rtol:.3e})")
    assert (err <= rtol * want).all(), f"{what}: relative error {worst:.3e} exceeds {rtol:.3e}"


def _z(t):
    return t.cpu().numpy()


# ---- ops level: z and d ----------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", DTYPES)
def test_ops_mean_and_distances(name, K):
    from fedn_amd import ops
    te, R, _, _ = ops.wmean_geometry(TORCH_DT[name], K)
    assert R <= 1024
    sizes = sorted(set(PS + [te - 1, te, te + 1]))
    rng = np.random.default_rng(1000 * DTYPES.index(name) + K)
    S = _data(rng, name, K, _row_len(sizes[-1]))
    beta = _beta(rng, K)
    zw = gr.wmean(S, beta)                                     # per element: every prefix is a prefix of it
    dw = gr.dists_prefixes(S, zw, sizes)
    dev = _upload(S, name)
    for P in sizes:
        z, d = ops.weighted_mean_sqdist([dev[k, :P] for k in range(K)], beta)
        assert ops.last_kernel() == "k_wmean_dist"
        assert z.shape == (P,) and z.dtype == OUT_DT[name] and z.device == dev.device
        assert d.shape == (K,) and d.dtype == torch.float64 and d.device == dev.device
        _same_bits(_z(z), zw[:P], f"{name} K={K} P={P}: z")
        _check_d(_z(d), dw[P], ops.sqdist_rtol(TORCH_DT[name], P), f"{name} K={K} P={P}")


@pytest.mark.parametrize("K", [1, 2, 4, 8, 16, 32, 64])
@pytest.mark.parametrize("name", DTYPES)
def test_ops_power_of_two_mean_is_the_trimmed_mean(name, K):
    """beta = 1/K with K a power of two scales exactly, so z is the trimmed mean at trim 0 bit for bit —
    given the same order of the adds: that rule adds in ascending order of the values, this one in client
    order, so the updates are sorted along the client axis."""
    from fedn_amd import ops
    P = 4099
    S = np.sort(_data(np.random.default_rng(K), name, K, _row_len(P)), axis=0)
    dev = _upload(S, name)
    views = [dev[k, :P] for k in range(K)]
    want = torch.empty(P, dtype=OUT_DT[name], device=DEV)
    ops.trimmed_mean(want, views, 0)
    z, _ = ops.weighted_mean_sqdist(views, [1.0 / K] * K)
    _same_bits(_z(z), _z(want), f"{name} K={K}")
    _same_bits(_z(z), gr.wmean(S[:, :P], [1.0 / K] * K), f"{name} K={K} vs oracle")


@pytest.mark.parametrize("name", DTYPES)
def test_ops_every_workgroup_two_tiles_and_a_ragged_one(name):
    """K = 4 at a size where the grid is at its cap, every workgroup walks at least two tiles and the
    last tile is ragged."""
    from fedn_amd import ops
    K = 4
    te, _, grid, _ = ops.wmean_geometry(TORCH_DT[name], K)
    P = 2 * grid * te + te // 2 + 3
    rng = np.random.default_rng(50 + DTYPES.index(name))
    S = _data(rng, name, K, _row_len(P))
    beta = _beta(rng, K)
    dev = _upload(S, name)
    z, d = ops.weighted_mean_sqdist([dev[k, :P] for k in range(K)], beta)
    zw = gr.wmean(S[:, :P], beta)
    _same_bits(_z(z), zw, f"{name} K={K} P={P}: z")
    _check_d(_z(d), gr.dists(S[:, :P], zw), ops.sqdist_rtol(TORCH_DT[name], P), f"{name} K={K} P={P}")


@pytest.mark.parametrize("name,K", [("f16", 33), ("f16", 9), ("i32", 33)])
def test_ops_chains_flushed_mid_kernel(name, K):
    """A size at which every workgroup walks more tiles than one flush period, so the chains are flushed
    to f64 in mid-kernel as well as at the end. The updates are constants (client k holds k / 2; k for
    integers) and beta is one-hot on client j: z is that client's constant and every term and partial sum
    is exact in f32 and f64, so d[k] is EXACTLY P ((k - j) scale)^2 — an element dropped or counted twice
    shows."""
    from fedn_amd import ops
    te, _, grid, flush_tiles = ops.wmean_geometry(TORCH_DT[name], K)
    P = grid * te * (flush_tiles + 1) + te // 2 + 3
    scale = 0.5 if name == "f16" else 1
    ups = [torch.full((P,), k * scale, dtype=TORCH_DT[name], device=DEV) for k in range(K)]
    idx = np.arange(K, dtype=np.float64)
    for j in (0, K // 2):
        beta = [0.0] * K
        beta[j] = 1.0
        z, d = ops.weighted_mean_sqdist(ups, beta)
        assert bool((z == j * scale).all()), f"{name} K={K} P={P}: z is not client {j}'s constant"
        want = P * ((idx - j) * scale) ** 2
        got = _z(d)
        assert np.array_equal(got, want), f"{name} K={K} P={P} j={j}: worst {np.abs(got - want).max()}"


@pytest.mark.parametrize("name,K", [("f32", 5), ("f16", 17), ("bf16", 8), ("f64", 33), ("i32", 3), ("i64", 64)])
def test_store_and_no_store(name, K):
    """``store=False`` forms z for the distances only: the same d bits, and a sentinel-filled out is not
    touched."""
    from fedn_amd import ops
    te, _, _, _ = ops.wmean_geometry(TORCH_DT[name], K)
    rng = np.random.default_rng(K)
    for P in (257, 2 * te + 9):
        dev = _upload(_data(rng, name, K, _row_len(P)), name)
        views = [dev[k, :P] for k in range(K)]
        beta = _beta(rng, K)
        z, d = ops.weighted_mean_sqdist(views, beta)
        out = torch.full((P,), 7.0, dtype=OUT_DT[name], device=DEV)
        none, d2 = ops.weighted_mean_sqdist(views, beta, out=out, store=False)
        assert none is None and bool((out == 7).all()), "out is left alone"
        _same_bits(_z(d2), _z(d), f"{name} K={K} P={P}: d without the store")
        none, d3 = ops.weighted_mean_sqdist(views, beta, store=False)
        assert none is None
        _same_bits(_z(d3), _z(d), f"{name} K={K} P={P}: d without an out")
        got, _ = ops.weighted_mean_sqdist(views, beta, out=out)
        assert got is out
        _same_bits(_z(out), _z(z), f"{name} K={K} P={P}: z into a given out")


# ---- the same bits ---------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [3, 8, 17, 64])
@pytest.mark.parametrize("name", DTYPES)
def test_same_bits_every_call_and_alignment(name, K):
    from fedn_amd import ops
    te, _, _, _ = ops.wmean_geometry(TORCH_DT[name], K)
    n = _row_len(2 * te + 70)
    rng = np.random.default_rng(7 + K)
    dev = _upload(_data(rng, name, K, n), name)
    beta = _beta(rng, K)
    for P in (5, te - 1, te + 1, 2 * te + 9):
        shifted = [dev[k, 1:1 + P] for k in range(K)]           # one element past a 16-B boundary
        assert all(v.data_ptr() % 16 for v in shifted)
        aligned = [v.clone() for v in shifted]
        assert not any(v.data_ptr() % 16 for v in aligned)
        mixed = [s if k % 2 else v for k, (s, v) in enumerate(zip(shifted, aligned))]
        odd_out = torch.empty(P + 1, dtype=OUT_DT[name], device=DEV)[1:]
        runs = [ops.weighted_mean_sqdist(aligned, beta), ops.weighted_mean_sqdist(aligned, beta),
                ops.weighted_mean_sqdist(shifted, beta), ops.weighted_mean_sqdist(mixed, beta),
                ops.weighted_mean_sqdist(shifted, beta, out=odd_out)]
        z0, d0 = _z(runs[0][0]), _z(runs[0][1])
        for what, (z, d) in zip(("second call", "unaligned views", "mixed alignment", "unaligned out"), runs[1:]):
            _same_bits(_z(z), z0, f"{name} K={K} P={P}: z, {what}")
            _same_bits(_z(d), d0, f"{name} K={K} P={P}: d, {what}")


@pytest.mark.parametrize("name", DTYPES)
def test_accumulate_over_two_halves(name):
    from fedn_amd import ops
    K, P = 9, 65539
    rng = np.random.default_rng(21)
    S = _data(rng, name, K, _row_len(P))
    beta = _beta(rng, K)
    dev = _upload(S, name)
    h = 32768
    first, second = [dev[k, :h] for k in range(K)], [dev[k, h:P] for k in range(K)]
    z, one = ops.weighted_mean_sqdist([dev[k, :P] for k in range(K)], beta)
    z1, d1 = ops.weighted_mean_sqdist(first, beta)
    z2, d2 = ops.weighted_mean_sqdist(second, beta)
    acc = torch.full((K,), 7.0, dtype=torch.float64, device=DEV)
    ops.weighted_mean_sqdist(first, beta, dist=acc, store=False)               # written: the 7s are gone
    _, same = ops.weighted_mean_sqdist(second, beta, dist=acc, accumulate=True, store=False)
    assert same is acc
    acc, one = _z(acc), _z(one)
    _same_bits(acc, _z(d1) + _z(d2), "accumulate is the f64 sum of the two calls")
    _same_bits(np.concatenate([_z(z1), _z(z2)]), _z(z), "z of the halves is z of the whole")
    rtol = ops.sqdist_rtol(TORCH_DT[name], P)
    # both halves are within their bounds of their exact sums, the one add is rounded once: the total is
    # within the whole model's bound of the exact total, and so within twice the bound of the one call
    _check_d(acc, gr.dists(S[:, :P], _z(z)), rtol, f"{name} accumulated")
    assert (np.abs(acc - one) <= 2 * rtol * one).all()


# ---- bounds ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [4, 5, 9, 17, 33])
@pytest.mark.parametrize("name", ["f32", "f16", "f64", "i32"])
def test_nothing_outside_the_windows(name, K):
    """Every update sits inside a larger buffer between sentinels that would wreck z and d if read; out and
    dist are windows of larger sentinel-filled buffers: the results are the oracle's and nothing outside
    the windows changes."""
    from fedn_amd import ops
    te, _, _, _ = ops.wmean_geometry(TORCH_DT[name], K)
    guard = 64
    sentinel = {"f32": 3e30, "f16": 6e4, "f64": 1e300, "i32": 2 ** 31 - 1}[name]
    rng = np.random.default_rng(K)
    for P in (257, te + 1):
        for off in (0, 1):
            S = _data(np.random.default_rng(K + P), name, K, P)
            beta = _beta(rng, K)
            big = np.full((K, guard + off + P + guard), sentinel, dtype=NP_DT[name])
            big[:, guard + off:guard + off + P] = S
            dev = _upload(big, name)
            before = dev.clone()
            out = torch.full((P + 2 * guard + off,), -5.0, dtype=OUT_DT[name], device=DEV)
            dist = torch.full((K + 2 * guard,), -5.0, dtype=torch.float64, device=DEV)
            lo = guard + off
            ops.weighted_mean_sqdist([dev[k, lo:lo + P] for k in range(K)], beta, out=out[lo:lo + P],
                                     dist=dist[guard:guard + K])
            o, d = _z(out), _z(dist)
            assert (o[:lo] == -5).all() and (o[lo + P:] == -5).all(), (name, K, P, off)
            assert (d[:guard] == -5).all() and (d[guard + K:] == -5).all(), (name, K, P, off)
            zw = gr.wmean(S, beta)
            _same_bits(o[lo:lo + P], zw, f"{name} K={K} P={P} off={off}: z")
            _check_d(d[guard:guard + K], gr.dists(S, zw), ops.sqdist_rtol(TORCH_DT[name], P),
                     f"{name} K={K} P={P} off={off}")
            assert torch.equal(dev, before), "the updates are read only"


# ---- specials --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["f32", "bf16", "f16", "f64"])
def test_specials(name):
    """One client holds an inf, one a NaN. With their weights 0, z is finite and is the z of the run with
    those clients zeroed, bit for bit; their own d is non-finite and the others' d has that run's bits.
    With nonzero weights z is non-finite at exactly those elements; neither is an error."""
    from fedn_amd import ops
    K, P = 7, 4099
    rng = np.random.default_rng(31)
    S = _data(rng, name, K, _row_len(P))
    bad = {1: np.inf, 3: np.nan}
    T = S.copy()
    for k, v in bad.items():
        T[k, 1000 + k] = v
    Z = S.copy()
    for k in bad:
        Z[k, :] = 0
    beta = rng.uniform(0.05, 1.0, K)
    beta[list(bad)] = 0.0
    beta = beta.tolist()
    z, d = ops.weighted_mean_sqdist([r[:P] for r in _upload(T, name)], beta)      # returns: FA_OK
    zr, dr = ops.weighted_mean_sqdist([r[:P] for r in _upload(Z, name)], beta)
    z, d, zr, dr = _z(z), _z(d), _z(zr), _z(dr)
    assert np.isfinite(z.astype(np.float64)).all()
    _same_bits(z, zr, f"{name}: z with the bad clients at weight 0")
    _same_bits(z, gr.wmean(T[:, :P], beta), f"{name}: z against the oracle")
    good = [k for k in range(K) if k not in bad]
    assert not np.isfinite(d[list(bad)]).any(), d
    _same_bits(d[good], dr[good], f"{name}: the other clients' d")
    _check_d(d[good], gr.dists(S[good, :P], z), ops.sqdist_rtol(TORCH_DT[name], P), f"{name} specials, good clients")
    beta2 = rng.uniform(0.05, 1.0, K).tolist()
    z2, d2 = ops.weighted_mean_sqdist([r[:P] for r in _upload(T, name)], beta2)
    z2 = _z(z2).astype(np.float64)
    assert sorted(np.flatnonzero(~np.isfinite(z2)).tolist()) == sorted(1000 + k for k in bad)
    assert not np.isfinite(_z(d2)).any(), "every client is non-finitely far from a non-finite z"


# ---- edges -----------------------------------------------------------------------------------------
def test_ops_empty_and_single():
    """P = 0 still writes its K zeros when dist is written and adds nothing when it is accumulated into;
    K = 1 with beta = [1] is a converting copy at distance 0 exactly."""
    from fedn_amd import ops
    for name in DTYPES:
        for K in (1, 3, 64):
            dist = torch.full((K,), 7.0, dtype=torch.float64, device=DEV)
            ups = [torch.empty(0, dtype=TORCH_DT[name], device=DEV) for _ in range(K)]
            z, d = ops.weighted_mean_sqdist(ups, [1.0] * K, dist=dist)
            assert d is dist and z.numel() == 0 and z.dtype == OUT_DT[name]
            assert (_z(dist) == 0).all(), (name, K)
            dist.fill_(7.0)
            ops.weighted_mean_sqdist(ups, [1.0] * K, dist=dist, accumulate=True)
            assert (_z(dist) == 7).all(), (name, K)
        S = _data(np.random.default_rng(1), name, 1, 4160)
        one = _upload(S, name)
        z, d = ops.weighted_mean_sqdist([one[0, :4099]], [1.0])
        assert d.shape == (1,) and d.item() == 0.0
        want = S[0, :4099].astype(np.float64) if NP_DT[name] in (np.int32, np.int64) else S[0, :4099]
        _same_bits(_z(z), want, f"{name}: K = 1 is a converting copy")


def test_ops_refuses_bad_arguments():
    from fedn_amd import _abi, ops
    x = torch.zeros(8, device=DEV)
    d2 = torch.zeros(2, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError):
        ops.weighted_mean_sqdist([], [])
    with pytest.raises(ValueError):
        ops.weighted_mean_sqdist([x] * 65, [1.0] * 65)
    with pytest.raises(ValueError):
        ops.weighted_mean_sqdist([x, torch.zeros(9, device=DEV)], [1.0, 1.0])                      # lengths differ
    with pytest.raises(TypeError):
        ops.weighted_mean_sqdist([x, torch.zeros(8, dtype=torch.float64, device=DEV)], [1.0, 1.0])  # dtypes differ
    with pytest.raises(TypeError):
        ops.weighted_mean_sqdist([torch.zeros(8, dtype=torch.int8, device=DEV)] * 2, [1.0, 1.0])   # not one of the six
    with pytest.raises(ValueError):
        ops.weighted_mean_sqdist([x, x], [1.0, 1.0], out=torch.zeros(5, device=DEV))
    with pytest.raises(TypeError):
        ops.weighted_mean_sqdist([x, x], [1.0, 1.0], out=torch.zeros(8, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError):
        ops.weighted_mean_sqdist([x, x], [1.0, 1.0], dist=torch.zeros(3, dtype=torch.float64, device=DEV))
    with pytest.raises(TypeError):
        ops.weighted_mean_sqdist([x, x], [1.0, 1.0], dist=torch.zeros(2, dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError):
        ops.weighted_mean_sqdist([x, x], [1.0, 1.0], accumulate=True)                              # nothing to add to
    with pytest.raises(ValueError):
        ops.weighted_mean_sqdist([x, x.cpu()], [1.0, 1.0])
    with pytest.raises(ValueError):
        ops.weighted_mean_sqdist([x, x], [1.0])                                                    # one weight short
    with pytest.raises(ValueError):
        ops.weighted_mean_sqdist([x, x], [1.0, 1.0, 1.0])
    for beta in ([1.0, -1.0], [1.0, float("nan")], [0.0, 0.0]):                                    # the library's refusals
        with pytest.raises(_abi.FedAggError) as e:
            ops.weighted_mean_sqdist([x, x], beta, dist=d2)
        assert e.value.status == _abi.FA_EINVAL
    with pytest.raises(_abi.FedAggError) as e:
        ops.wmean_geometry(torch.int8, 4)
    assert e.value.status == _abi.FA_EDTYPE


# ---- plug-in rounds --------------------------------------------------------------------------------
ROUNDS = [(4, 257), (5, 257), (10, 4099), (17, 4099), (64, 4099)]
FRACTION = 0.2
NU = 1e-6


def _byzantine_count(fraction, K):
    import math
    if K < 3:
        return 0
    return min(math.floor(fraction * K), (K - 3) // 2)


def _round_updates(seed, K, spec, fraction=FRACTION):
    """K updates of the model ``spec`` with f = byzantine_count(fraction, K) hostile ones: the generator the
    robust rules' tests share (tests/robust_fuzz_cases.round_updates). Returns (updates, hostile indices)."""
    return round_updates(seed, K, _byzantine_count(fraction, K), spec)


def _run_round(ups, staged, parameters=None, budget=None, agg=None, uh=None):
    from fedn_amd.aggregators import get_aggregator
    from fedn_amd.ingest import StagingUpdateHandler
    from fedn_amd.updatehandler import MemoryUpdateHandler
    uh = uh or MemoryUpdateHandler()
    st = StagingUpdateHandler(uh, helper=None, device=DEV, workers=2) if staged else None
    try:
        if agg is None:
            agg = get_aggregator("geomedian", st or uh)
            agg.device, agg.hbm_budget = torch.device(DEV), budget
        mus = [uh.submit(u, 10 + k, via=st) for k, u in enumerate(ups)]
        model, data = agg.combine_models(helper=None, parameters=parameters)
    finally:
        if st is not None:
            st.close()
    return model, data, uh, mus, agg


def _flat64(model):
    return np.concatenate([np.asarray(a, dtype=np.float64).reshape(-1) for a in model])


def _check_robust(ups, hostile, device_trace, model, iterations, nu, what):
    """The precondition in float64 on the CPU, then the same two facts on the device result: from pass 1
    on the largest hostile weight is at most 0.46 x the smallest honest one — orders of magnitude beyond
    what the distance bound could move — and (K >= 5) the result is at least 4 x nearer the honest
    clients' mean than the plain mean of the finite clients is."""
    K = len(ups)
    nan = _nan_clients(ups)
    honest = [k for k in range(K) if k not in hostile]
    trace, z64 = gr.weiszfeld_f64(ups, iterations, nu, excluded=nan)
    for t, (beta, _) in enumerate(trace[1:], 1):
        assert beta[hostile].max() <= 0.46 * beta[honest].min(), f"{what}: precondition, pass {t}: {beta}"
    for t, (beta, _) in enumerate(device_trace[1:], 1):
        assert beta[hostile].max() <= 0.46 * beta[honest].min(), f"{what}: device pass {t}: {beta}"
    if K >= 5:
        X = np.stack([_flat64(u) for u in ups])
        centre = X[honest].mean(axis=0)
        finite = [k for k in range(K) if k not in nan]
        plain = np.linalg.norm(X[finite].mean(axis=0) - centre)
        assert 4 * np.linalg.norm(z64 - centre) <= plain, f"{what}: precondition"
        got = np.linalg.norm(_flat64(model) - centre)
        print(f"{what}: distance to the honest mean {got:.4g}, the plain mean's {plain:.4g}")
        assert 4 * got <= plain, f"{what}: {got} vs {plain}"


@pytest.mark.parametrize("staged", [False, True], ids=["host", "staged"])
@pytest.mark.parametrize("K,P", ROUNDS)
def test_plugin_round(K, P, staged):
    spec = [((P,), np.float32), ((P // 4 + 3,), np.int32)]       # two dtype groups: f32 and i32
    ups, hostile = _round_updates(0, K, spec)
    assert len(hostile) == _byzantine_count(FRACTION, K)
    if K in (17, 64):
        assert _nan_clients(ups), "these rounds exercise the exclusion path"
    T = 3
    model, data, uh, _, agg = _run_round(ups, staged, {"iterations": T, "nu": NU})
    assert data["nr_aggregated_models"] == K, "excluded clients are counted"
    for key in ("time_model_load", "time_model_aggregation", "time_h2d", "time_kernel", "time_pack", "time_d2h"):
        assert key in data
    assert [a.dtype for a in model] == [np.dtype(np.float32), np.dtype(np.float64)]
    assert [a.shape for a in model] == [(P,), (P // 4 + 3,)]
    _check_chain(ups, agg, model, T, NU, f"K={K} P={P}")
    if hostile:
        _check_robust(ups, hostile, agg.trace, model, T, NU, f"K={K} P={P}")
    assert uh.model_updates.qsize() == 0 and not uh.store.models, "every update is deleted once the result exists"


def test_default_parameters():
    """No parameters: 3 iterations at nu = 1e-6."""
    K, P = 10, 4099
    spec = [((P,), np.float32), ((P // 4 + 3,), np.int32)]
    ups, hostile = _round_updates(0, K, spec)
    model, data, _, _, agg = _run_round(ups, False)
    assert data["nr_aggregated_models"] == K
    _check_chain(ups, agg, model, 3, 1e-6, "defaults")
    _check_robust(ups, hostile, agg.trace, model, 3, 1e-6, "defaults")


def test_zero_iterations_is_the_plain_mean():
    K, P = 10, 4099
    spec = [((P,), np.float32), ((P // 4 + 3,), np.int32)]
    ups, _ = _round_updates(0, K, spec)
    model, data, _, _, agg = _run_round(ups, False, {"iterations": 0})
    assert data["nr_aggregated_models"] == K and len(agg.trace) == 1 and agg.excluded == []
    assert_lists_identical(model, gr.model_wmean(ups, [1.0 / K] * K), "iterations = 0")
    _check_chain(ups, agg, model, 0, 1e-6, "iterations = 0")


def test_single_update_is_a_converting_copy():
    spec = [((257,), np.float32), ((67,), np.int32)]
    ups, _ = _round_updates(0, 1, spec)
    model, data, _, _, agg = _run_round(ups, False, {"iterations": 5})
    assert data["nr_aggregated_models"] == 1 and len(agg.trace) == 1
    assert_lists_identical(model, [ups[0][0], ups[0][1].astype(np.float64)], "K = 1")
    assert agg.weights.tolist() == [1.0] and agg.distances.tolist() == [0.0]


def test_budget_keeps_updates_on_the_host(monkeypatch):
    """A budget of 3 updates with K = 12: nine stay on the host and every pass walks them slice by slice
    through the ring. The slices change d's last bits and hence beta, so the model is pinned by the
    round's own chain, not against the unbudgeted round."""
    from fedn_amd import robust
    from fedn_amd.budget import HbmBudget
    from fedn_amd.layout import Layout
    K = 12
    spec = [((300, 200), np.float32), ((77,), np.int64), ((1001,), np.float32), ((), np.float32)]
    ups, hostile = _round_updates(0, K, spec)
    monkeypatch.setattr(robust, "SLICE_BYTES", 16384)
    budget = HbmBudget(limit=3 * Layout.of(ups[0]).nbytes)
    model, data, uh, _, agg = _run_round(ups, False, {"iterations": 2}, budget=budget)
    assert agg.host_side == 9 and data["nr_aggregated_models"] == K, "every update is counted"
    _check_chain(ups, agg, model, 2, 1e-6, "budget")
    _check_robust(ups, hostile, agg.trace, model, 2, 1e-6, "budget")
    assert not uh.store.models
    del agg
    gc.collect()
    assert budget.used(DEV) == 0, "the round's reservations went back to the budget"


# ---- refusals and failures ---------------------------------------------------------------------------
def test_more_than_64_updates_refused():
    ups, _ = _round_updates(12, 65, [((33,), np.float32)])
    model, data, uh, mus, _ = _run_round(ups, False)
    assert model is None and data["nr_aggregated_models"] == 0
    assert uh.model_updates.qsize() == 0
    assert set(uh.store.models) == {m.model_update_id for m in mus}, "nothing is deleted"


@pytest.mark.parametrize("staged", [False, True], ids=["host", "staged"])
def test_layout_mismatch_is_skipped_and_kept(staged):
    K, P = 10, 4099
    spec = [((P,), np.float32), ((P // 4 + 3,), np.int32)]
    ups, _ = _round_updates(0, K, spec)
    odd = [np.zeros((5, 3), dtype=np.float32), np.zeros(7, dtype=np.int32)]      # not this round's layout
    queue = ups[:3] + [odd] + ups[3:]
    model, data, uh, mus, agg = _run_round(queue, staged)
    assert data["nr_aggregated_models"] == K
    _check_chain(ups, agg, model, 3, 1e-6, "layout mismatch")     # indices count the admitted updates
    assert set(uh.store.models) == {mus[3].model_update_id}, "the skipped update stays in storage"


def test_nan_in_every_update_keeps_every_update():
    """A NaN in every update: every distance is non-finite and nobody can be excluded — (None, data),
    nothing deleted."""
    ups, _ = _round_updates(5, 6, [((257,), np.float32)])
    for u in ups:
        u[0][3] = np.nan
    model, data, uh, mus, agg = _run_round(ups, False)
    assert model is None and data["nr_aggregated_models"] == 0 and agg.weights is None
    assert set(uh.store.models) == {mu.model_update_id for mu in mus}


def test_failed_launch_keeps_every_update(monkeypatch):
    """A launch that fails (injected at the wrapper: no device fault): the round is (None, data), the
    updates stay in storage, and the aggregator's next round passes the chain."""
    from fedn_amd import _abi, ops
    K, P = 10, 4099
    spec = [((P,), np.float32), ((P // 4 + 3,), np.int32)]
    ups, _ = _round_updates(0, K, spec)
    calls = []

    def boom(*a, **kw):
        calls.append(1)
        raise _abi.FedAggError(_abi.FA_EHIP, "weighted_mean_sqdist: injected failure")

    with monkeypatch.context() as mp:
        mp.setattr(ops, "weighted_mean_sqdist", boom)
        model, data, uh, mus, agg = _run_round(ups, False)
    assert calls and model is None and data["nr_aggregated_models"] == 0
    assert uh.model_updates.qsize() == 0
    assert set(uh.store.models) == {mu.model_update_id for mu in mus}, "every update stays in storage"
    model, data, uh, mus2, _ = _run_round(ups, False, agg=agg, uh=uh)
    assert data["nr_aggregated_models"] == K
    _check_chain(ups, agg, model, 3, 1e-6, "the round after a failed launch")
    assert set(uh.store.models) == {mu.model_update_id for mu in mus}
