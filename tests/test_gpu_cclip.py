"""Centred clipping on the GPU: ``fa_centered_clip_step`` (kernel ``k_cclip_dist``) through
``ops.centered_clip_step``, ``robust.RobustPipeline.centered_clip`` and the ``centeredclip`` plug-in, against
the oracle tests/cclip_ref.py: the new point bit for bit, the distances within ``ops.sqdist_rtol`` of the
exact sums, in place as out of place, the same bits on every call and at every alignment, and the rule's
chain pinned pass by pass with the pipeline's own trace."""
import gc
import math

import numpy as np
import pytest
import torch

import cclip_ref as cr
from golden_io import assert_lists_identical
from robust_checks import check_cclip_chain as _check_chain
from robust_checks import nan_clients as _nan_clients
from robust_checks import same_bits as _same_bits
from robust_fuzz_cases import center_round_updates

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KS = [1, 2, 3, 5, 8, 9, 16, 17, 32, 33, 63, 64]
PS = [1, 5, 257, 4099, 65539]
DTYPES = ["f32", "f64", "f16", "bf16", "i32", "i64"]
NP_DT = {"f32": np.float32, "f64": np.float64, "f16": np.float16, "bf16": np.float32, "i32": np.int32, "i64": np.int64}
NP_OUT = {"f32": np.float32, "f64": np.float64, "f16": np.float16, "bf16": np.float32, "i32": np.float64, "i64": np.float64}
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
    """K updates that are close to each other, as in federated learning — a base plus small noise — and a
    centre, the base plus other small noise, in the output type."""
    dt = np.dtype(NP_DT[name])
    base = rng.standard_normal(n)
    x = base + 0.05 * rng.standard_normal((K, n))
    v = base + 0.02 * rng.standard_normal(n)
    if dt.kind == "i":
        scale = 2.0 ** 20 if name == "i32" else 2.0 ** 40
        x = np.round(x * scale).astype(dt)
        v = np.round(v * scale)                                  # float64: the output type
        if name == "i64":                                     # not exact in float64: converted with one rounding
            q = max(1, n // 8)
            sign = rng.choice([-1, 1], (1, q))
            x[:, :q] = (2 ** 53 + rng.integers(1, 1000, (K, q))) * sign
            v[:q] = (2.0 ** 53 + 2.0 * rng.integers(1, 500, q)) * sign[0]
        return np.ascontiguousarray(x), np.ascontiguousarray(v)
    x = x.astype(dt)
    v = v.astype(NP_OUT[name])
    return (_bf16_exact(x) if name == "bf16" else np.ascontiguousarray(x)), v


def _upload(S, name):
    t = torch.from_numpy(np.ascontiguousarray(S)).to(DEV)
    return t.to(torch.bfloat16) if name == "bf16" else t       # exact: the values are bf16's


def _up_center(v):
    return torch.from_numpy(np.ascontiguousarray(v)).to(DEV)


def _row_len(n):
    return -(-n // 64) * 64                                    # rows of a (K, row) matrix stay 16-B aligned


def _coef(rng, K):
    """Random coefficients in (0, 1], one of them exactly 0 (K > 1)."""
    coef = rng.uniform(0.05, 1.0, K)
    if K > 1:
        coef[int(rng.integers(0, K))] = 0.0
    return coef.tolist()


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


# ---- ops level: v' and d ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", DTYPES)
def test_ops_step_and_distances(name, K):
    from fedn_amd import ops
    te, R, _, _ = ops.cclip_geometry(TORCH_DT[name], K)
    assert R <= 1024
    sizes = sorted(set(PS + [te - 1, te, te + 1]))
    rng = np.random.default_rng(1000 * DTYPES.index(name) + K)
    S, v = _data(rng, name, K, _row_len(sizes[-1]))
    coef = _coef(rng, K)
    zw = cr.step(S, v, coef)                                   # per element: every prefix is a prefix of it
    dw = cr.dists_prefixes(S, zw, sizes)
    dev, cen = _upload(S, name), _up_center(v)
    for P in sizes:
        z, d = ops.centered_clip_step([dev[k, :P] for k in range(K)], cen[:P], coef)
        assert ops.last_kernel() == "k_cclip_dist"
        assert z.shape == (P,) and z.dtype == OUT_DT[name] and z.device == dev.device
        assert d.shape == (K,) and d.dtype == torch.float64 and d.device == dev.device
        _same_bits(_z(z), zw[:P], f"{name} K={K} P={P}: v'")
        _check_d(_z(d), dw[P], ops.sqdist_rtol(TORCH_DT[name], P), f"{name} K={K} P={P}")
    _same_bits(_z(cen), v, f"{name} K={K}: an out-of-place centre is read only")


@pytest.mark.parametrize("name,K", [("f32", 5), ("f16", 17), ("bf16", 8), ("f64", 33), ("i32", 3), ("i64", 64)])
def test_all_zero_coefficients(name, K):
    """Every coefficient 0 — the pass that starts the rule: v' is the centre bit for bit, d the distances to
    the centre; with ``store=False`` a sentinel-filled out is not touched and d has the same bits."""
    from fedn_amd import ops
    te, _, _, _ = ops.cclip_geometry(TORCH_DT[name], K)
    rng = np.random.default_rng(K)
    for P in (257, 2 * te + 9):
        S, v = _data(rng, name, K, _row_len(P))
        v[:4] = [-0.0, 0.0, -1.0, 1.0]
        dev, cen = _upload(S, name), _up_center(v)
        views = [dev[k, :P] for k in range(K)]
        zero = [0.0] * K
        z, d = ops.centered_clip_step(views, cen[:P], zero)
        _same_bits(_z(z), v[:P], f"{name} K={K} P={P}: v' at coef 0 is the centre")
        _check_d(_z(d), cr.dists(S[:, :P], v[:P]), ops.sqdist_rtol(TORCH_DT[name], P), f"{name} K={K} P={P}")
        out = torch.full((P,), 7.0, dtype=OUT_DT[name], device=DEV)
        none, d2 = ops.centered_clip_step(views, cen[:P], zero, out=out, store=False)
        assert none is None and bool((out == 7).all()), "out is left alone"
        _same_bits(_z(d2), _z(d), f"{name} K={K} P={P}: d without the store")
        none, d3 = ops.centered_clip_step(views, cen[:P], zero, store=False)
        assert none is None
        _same_bits(_z(d3), _z(d), f"{name} K={K} P={P}: d without an out")
        coef = _coef(rng, K)                                   # and no store at nonzero coefficients
        z4, d4 = ops.centered_clip_step(views, cen[:P], coef)
        none, d5 = ops.centered_clip_step(views, cen[:P], coef, out=out, store=False)
        assert none is None and bool((out == 7).all())
        _same_bits(_z(d5), _z(d4), f"{name} K={K} P={P}: d of a step that is not stored")
        got, _ = ops.centered_clip_step(views, cen[:P], coef, out=out)
        assert got is out
        _same_bits(_z(out), _z(z4), f"{name} K={K} P={P}: v' into a given out")


@pytest.mark.parametrize("K", [1, 4, 9, 33, 64])
@pytest.mark.parametrize("name", DTYPES)
def test_in_place_is_out_of_place(name, K):
    """``out is center``: the same v' and d bits as into a separate buffer — below a tile, across a tile
    edge, and with the grid at its cap so that every workgroup walks several tiles of the buffer it
    overwrites."""
    from fedn_amd import ops
    te, _, grid, _ = ops.cclip_geometry(TORCH_DT[name], K)
    big = 2 * grid * te + te // 2 + 3 if K == 4 else 3 * te + 5
    rng = np.random.default_rng(300 + K)
    S, v = _data(rng, name, K, _row_len(big))
    coef = _coef(rng, K)
    dev = _upload(S, name)
    for P in (te - 1, te + 1, big):
        views = [dev[k, :P] for k in range(K)]
        cen = _up_center(v)
        z, d = ops.centered_clip_step(views, cen[:P], coef)
        got, d2 = ops.centered_clip_step(views, cen[:P], coef, out=cen[:P])
        assert got.data_ptr() == cen.data_ptr()
        _same_bits(_z(cen[:P]), _z(z), f"{name} K={K} P={P}: v' in place")
        _same_bits(_z(d2), _z(d), f"{name} K={K} P={P}: d in place")
        _same_bits(_z(cen[P:]), v[P:], f"{name} K={K} P={P}: the centre past P")
        _same_bits(_z(z), cr.step(S[:, :P], v[:P], coef), f"{name} K={K} P={P}: v' against the oracle")
        # shifted one element: in place through the element loads
        cen1 = torch.empty(P + 1, dtype=OUT_DT[name], device=DEV)[1:]
        cen1.copy_(_up_center(v[:P]))
        assert cen1.data_ptr() % 16
        _, d3 = ops.centered_clip_step(views, cen1, coef, out=cen1)
        _same_bits(_z(cen1), _z(z), f"{name} K={K} P={P}: v' in place, unaligned")
        _same_bits(_z(d3), _z(d), f"{name} K={K} P={P}: d in place, unaligned")


@pytest.mark.parametrize("name", DTYPES)
def test_ops_every_workgroup_two_tiles_and_a_ragged_one(name):
    """K = 4 at a size where the grid is at its cap, every workgroup walks at least two tiles and the
    last tile is ragged."""
    from fedn_amd import ops
    K = 4
    te, _, grid, _ = ops.cclip_geometry(TORCH_DT[name], K)
    P = 2 * grid * te + te // 2 + 3
    rng = np.random.default_rng(50 + DTYPES.index(name))
    S, v = _data(rng, name, K, _row_len(P))
    coef = _coef(rng, K)
    dev, cen = _upload(S, name), _up_center(v)
    z, d = ops.centered_clip_step([dev[k, :P] for k in range(K)], cen[:P], coef)
    zw = cr.step(S[:, :P], v[:P], coef)
    _same_bits(_z(z), zw, f"{name} K={K} P={P}: v'")
    _check_d(_z(d), cr.dists(S[:, :P], zw), ops.sqdist_rtol(TORCH_DT[name], P), f"{name} K={K} P={P}")


@pytest.mark.parametrize("name,K", [("f16", 33), ("bf16", 33), ("i32", 33)])
def test_ops_chains_flushed_mid_kernel(name, K):
    """A size at which every workgroup walks more tiles than one flush period, so the chains are flushed
    to f64 in mid-kernel as well as at the end. The updates are constants (client k holds k / 2; k for
    integers), the centre is client 1's constant and coef is one-hot with value 1 on client j: v' is that
    client's constant and every term and partial sum is exact in f32 and f64, so d[k] is EXACTLY
    P ((k - j) scale)^2 — an element dropped or counted twice shows."""
    from fedn_amd import ops
    te, _, grid, flush_tiles = ops.cclip_geometry(TORCH_DT[name], K)
    P = grid * te * (flush_tiles + 1) + te // 2 + 3
    scale = 0.5 if name == "f16" else 1
    idx = np.arange(K, dtype=np.float64)
    small = np.repeat((idx * scale).astype(NP_DT[name])[:, None], 3, axis=1)
    centre = np.full(3, scale, dtype=NP_OUT[name])
    ups = [torch.full((P,), k * scale, dtype=TORCH_DT[name], device=DEV) for k in range(K)]
    for j in (0, K // 2):
        coef = [0.0] * K
        coef[j] = 1.0
        assert (cr.step(small, centre, coef) == j * scale).all(), "v + 1 (u_j - v) is exact for these constants"
        cen = torch.full((P,), scale, dtype=OUT_DT[name], device=DEV)
        z, d = ops.centered_clip_step(ups, cen, coef, out=cen)
        assert bool((cen == j * scale).all()), f"{name} K={K} P={P}: v' is not client {j}'s constant"
        want = P * ((idx - j) * scale) ** 2
        got = _z(d)
        assert np.array_equal(got, want), f"{name} K={K} P={P} j={j}: worst {np.abs(got - want).max()}"


# ---- the same bits ---------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [3, 8, 17, 64])
@pytest.mark.parametrize("name", DTYPES)
def test_same_bits_every_call_and_alignment(name, K):
    from fedn_amd import ops
    te, _, _, _ = ops.cclip_geometry(TORCH_DT[name], K)
    n = _row_len(2 * te + 70)
    rng = np.random.default_rng(7 + K)
    S, v = _data(rng, name, K, n)
    dev, cen = _upload(S, name), _up_center(v)
    coef = _coef(rng, K)
    for P in (5, te - 1, te + 1, 2 * te + 9):
        shifted = [dev[k, 1:1 + P] for k in range(K)]           # one element past a 16-B boundary
        cshift = cen[1:1 + P]
        assert all(t.data_ptr() % 16 for t in shifted + [cshift])
        aligned, calign = [t.clone() for t in shifted], cshift.clone()
        assert not any(t.data_ptr() % 16 for t in aligned + [calign])
        mixed = [s if k % 2 else a for k, (s, a) in enumerate(zip(shifted, aligned))]
        odd_out = torch.empty(P + 1, dtype=OUT_DT[name], device=DEV)[1:]
        runs = [ops.centered_clip_step(aligned, calign, coef), ops.centered_clip_step(aligned, calign, coef),
                ops.centered_clip_step(shifted, calign, coef), ops.centered_clip_step(mixed, calign, coef),
                ops.centered_clip_step(aligned, cshift, coef), ops.centered_clip_step(shifted, cshift, coef),
                ops.centered_clip_step(shifted, calign, coef, out=odd_out)]
        z0, d0 = _z(runs[0][0]), _z(runs[0][1])
        names = ("second call", "unaligned views", "mixed alignment", "unaligned centre", "all unaligned", "unaligned out")
        for what, (z, d) in zip(names, runs[1:]):
            _same_bits(_z(z), z0, f"{name} K={K} P={P}: v', {what}")
            _same_bits(_z(d), d0, f"{name} K={K} P={P}: d, {what}")


@pytest.mark.parametrize("name", DTYPES)
def test_accumulate_over_two_halves(name):
    from fedn_amd import ops
    K, P = 9, 65539
    rng = np.random.default_rng(21)
    S, v = _data(rng, name, K, _row_len(P))
    coef = _coef(rng, K)
    dev, cen = _upload(S, name), _up_center(v)
    h = 32768
    first, second = [dev[k, :h] for k in range(K)], [dev[k, h:P] for k in range(K)]
    z, one = ops.centered_clip_step([dev[k, :P] for k in range(K)], cen[:P], coef)
    z1, d1 = ops.centered_clip_step(first, cen[:h], coef)
    z2, d2 = ops.centered_clip_step(second, cen[h:P], coef)
    acc = torch.full((K,), 7.0, dtype=torch.float64, device=DEV)
    ops.centered_clip_step(first, cen[:h], coef, dist=acc, store=False)               # written: the 7s are gone
    _, same = ops.centered_clip_step(second, cen[h:P], coef, dist=acc, accumulate=True, store=False)
    assert same is acc
    acc, one = _z(acc), _z(one)
    _same_bits(acc, _z(d1) + _z(d2), "accumulate is the f64 sum of the two calls")
    _same_bits(np.concatenate([_z(z1), _z(z2)]), _z(z), "v' of the halves is v' of the whole")
    rtol = ops.sqdist_rtol(TORCH_DT[name], P)
    # both halves are within their bounds of their exact sums, the one add is rounded once: the total is
    # within the whole model's bound of the exact total, and so within twice the bound of the one call
    _check_d(acc, cr.dists(S[:, :P], _z(z)), rtol, f"{name} accumulated")
    assert (np.abs(acc - one) <= 2 * rtol * one).all()


# ---- bounds ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [4, 5, 9, 17, 33])
@pytest.mark.parametrize("name", ["f32", "f16", "bf16", "f64", "i32"])
def test_nothing_outside_the_windows(name, K):
    """Every update and the centre sit inside larger buffers between sentinels that would wreck v' and d if
    read; out and dist are windows of larger sentinel-filled buffers: the results are the oracle's, nothing
    outside the windows changes, and the updates and the out-of-place centre are unchanged."""
    from fedn_amd import ops
    te, _, _, _ = ops.cclip_geometry(TORCH_DT[name], K)
    guard = 64
    sentinel = {"f32": 3e30, "f16": 6e4, "bf16": 3e30, "f64": 1e300, "i32": 2 ** 31 - 1}[name]
    csentinel = {"f32": 3e30, "f16": 6e4, "bf16": 3e30, "f64": 1e300, "i32": 1e300}[name]
    rng = np.random.default_rng(K)
    for P in (257, te + 1):
        for off in (0, 1):
            S, v = _data(np.random.default_rng(K + P), name, K, P)
            coef = _coef(rng, K)
            big = np.full((K, guard + off + P + guard), sentinel, dtype=NP_DT[name])
            lo = guard + off
            big[:, lo:lo + P] = S
            cbig = np.full(guard + off + P + guard, csentinel, dtype=NP_OUT[name])
            cbig[lo:lo + P] = v
            dev, cen = _upload(_bf16_exact(big) if name == "bf16" else big, name), _up_center(cbig)
            before, cbefore = dev.clone(), cen.clone()
            out = torch.full((P + 2 * guard + off,), -5.0, dtype=OUT_DT[name], device=DEV)
            dist = torch.full((K + 2 * guard,), -5.0, dtype=torch.float64, device=DEV)
            views = [dev[k, lo:lo + P] for k in range(K)]
            ops.centered_clip_step(views, cen[lo:lo + P], coef, out=out[lo:lo + P], dist=dist[guard:guard + K])
            o, d = _z(out), _z(dist)
            assert (o[:lo] == -5).all() and (o[lo + P:] == -5).all(), (name, K, P, off)
            assert (d[:guard] == -5).all() and (d[guard + K:] == -5).all(), (name, K, P, off)
            zw = cr.step(S, v, coef)
            _same_bits(o[lo:lo + P], zw, f"{name} K={K} P={P} off={off}: v'")
            _check_d(d[guard:guard + K], cr.dists(S, zw), ops.sqdist_rtol(TORCH_DT[name], P),
                     f"{name} K={K} P={P} off={off}")
            assert torch.equal(dev, before), "the updates are read only"
            assert torch.equal(cen, cbefore), "an out-of-place centre is read only"
            # in place: the window of the centre is v', its guards stay
            ops.centered_clip_step(views, cen[lo:lo + P], coef, out=cen[lo:lo + P], dist=dist[guard:guard + K])
            c = _z(cen)
            _same_bits(c[lo:lo + P], zw, f"{name} K={K} P={P} off={off}: v' in place")
            assert (c[:lo] == NP_OUT[name](csentinel)).all() and (c[lo + P:] == NP_OUT[name](csentinel)).all()
            assert torch.equal(dev, before)


# ---- specials --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["f32", "bf16", "f16", "f64"])
def test_specials(name):
    """One client holds an inf, one a NaN. With their coefficients 0, v' is finite and is the v' of the run
    with those clients zeroed, bit for bit; their own d is non-finite and the others' d has that run's
    bits. With nonzero coefficients v' is non-finite at exactly those elements; neither is an error."""
    from fedn_amd import ops
    K, P = 7, 4099
    rng = np.random.default_rng(31)
    S, v = _data(rng, name, K, _row_len(P))
    bad = {1: np.inf, 3: np.nan}
    T = S.copy()
    for k, val in bad.items():
        T[k, 1000 + k] = val
    Z = S.copy()
    for k in bad:
        Z[k, :] = 0
    coef = rng.uniform(0.05, 1.0, K)
    coef[list(bad)] = 0.0
    coef = coef.tolist()
    cen = _up_center(v)
    z, d = ops.centered_clip_step([r[:P] for r in _upload(T, name)], cen[:P], coef)      # returns: FA_OK
    zr, dr = ops.centered_clip_step([r[:P] for r in _upload(Z, name)], cen[:P], coef)
    z, d, zr, dr = _z(z), _z(d), _z(zr), _z(dr)
    assert np.isfinite(z.astype(np.float64)).all()
    _same_bits(z, zr, f"{name}: v' with the bad clients at coefficient 0")
    _same_bits(z, cr.step(T[:, :P], v[:P], coef), f"{name}: v' against the oracle")
    good = [k for k in range(K) if k not in bad]
    assert not np.isfinite(d[list(bad)]).any(), d
    _same_bits(d[good], dr[good], f"{name}: the other clients' d")
    _check_d(d[good], cr.dists(S[good, :P], z), ops.sqdist_rtol(TORCH_DT[name], P), f"{name} specials, good clients")
    coef2 = rng.uniform(0.05, 1.0, K).tolist()
    z2, d2 = ops.centered_clip_step([r[:P] for r in _upload(T, name)], cen[:P], coef2)
    z2 = _z(z2).astype(np.float64)
    assert sorted(np.flatnonzero(~np.isfinite(z2)).tolist()) == sorted(1000 + k for k in bad)
    assert not np.isfinite(_z(d2)).any(), "every client is non-finitely far from a non-finite v'"


# ---- edges -----------------------------------------------------------------------------------------
def test_ops_empty_and_single():
    """P = 0 still writes its K zeros when dist is written and adds nothing when it is accumulated into;
    K = 1 with coef = [1] from a centre of zeros is a converting copy at distance 0 exactly."""
    from fedn_amd import ops
    for name in DTYPES:
        for K in (1, 3, 64):
            dist = torch.full((K,), 7.0, dtype=torch.float64, device=DEV)
            ups = [torch.empty(0, dtype=TORCH_DT[name], device=DEV) for _ in range(K)]
            cen = torch.empty(0, dtype=OUT_DT[name], device=DEV)
            z, d = ops.centered_clip_step(ups, cen, [1.0] * K, dist=dist)
            assert d is dist and z.numel() == 0 and z.dtype == OUT_DT[name]
            assert (_z(dist) == 0).all(), (name, K)
            dist.fill_(7.0)
            ops.centered_clip_step(ups, cen, [0.0] * K, dist=dist, accumulate=True)
            assert (_z(dist) == 7).all(), (name, K)
        S, _ = _data(np.random.default_rng(1), name, 1, 4160)
        one = _upload(S, name)
        cen = torch.zeros(4099, dtype=OUT_DT[name], device=DEV)
        z, d = ops.centered_clip_step([one[0, :4099]], cen, [1.0])
        assert d.shape == (1,) and d.item() == 0.0
        want = S[0, :4099].astype(np.float64) if NP_DT[name] in (np.int32, np.int64) else S[0, :4099]
        _same_bits(_z(z), want, f"{name}: K = 1 at coef 1 from zeros is a converting copy")


def test_ops_refuses_bad_arguments():
    from fedn_amd import _abi, ops
    x = torch.zeros(8, device=DEV)
    c = torch.zeros(8, device=DEV)
    d2 = torch.zeros(2, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError):
        ops.centered_clip_step([], c, [])
    with pytest.raises(ValueError):
        ops.centered_clip_step([x] * 65, c, [1.0] * 65)
    with pytest.raises(ValueError):
        ops.centered_clip_step([x, torch.zeros(9, device=DEV)], c, [1.0, 1.0])                      # lengths differ
    with pytest.raises(TypeError):
        ops.centered_clip_step([x, torch.zeros(8, dtype=torch.float64, device=DEV)], c, [1.0, 1.0])  # dtypes differ
    with pytest.raises(TypeError):
        ops.centered_clip_step([torch.zeros(8, dtype=torch.int8, device=DEV)] * 2, c, [1.0, 1.0])   # not one of the six
    with pytest.raises(ValueError):
        ops.centered_clip_step([x, x], torch.zeros(5, device=DEV), [1.0, 1.0])                      # a short centre
    with pytest.raises(TypeError):
        ops.centered_clip_step([x, x], torch.zeros(8, dtype=torch.float64, device=DEV), [1.0, 1.0])  # centre not in O
    with pytest.raises(TypeError):
        ops.centered_clip_step([torch.zeros(8, dtype=torch.int32, device=DEV)] * 2,
                               torch.zeros(8, dtype=torch.int32, device=DEV), [1.0, 1.0])           # ... for integers: float64
    with pytest.raises(ValueError):
        ops.centered_clip_step([x, x], c.cpu(), [1.0, 1.0])
    with pytest.raises(TypeError):
        ops.centered_clip_step([x, x], c.cpu().numpy(), [1.0, 1.0])
    with pytest.raises(ValueError):
        ops.centered_clip_step([x, x], c, [1.0, 1.0], out=torch.zeros(5, device=DEV))
    with pytest.raises(TypeError):
        ops.centered_clip_step([x, x], c, [1.0, 1.0], out=torch.zeros(8, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError):
        ops.centered_clip_step([x, x], c, [1.0, 1.0], dist=torch.zeros(3, dtype=torch.float64, device=DEV))
    with pytest.raises(TypeError):
        ops.centered_clip_step([x, x], c, [1.0, 1.0], dist=torch.zeros(2, dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError):
        ops.centered_clip_step([x, x], c, [1.0, 1.0], accumulate=True)                              # nothing to add to
    with pytest.raises(ValueError):
        ops.centered_clip_step([x, x.cpu()], c, [1.0, 1.0])
    with pytest.raises(ValueError):
        ops.centered_clip_step([x, x], c, [1.0])                                                    # one coefficient short
    with pytest.raises(ValueError):
        ops.centered_clip_step([x, x], c, [1.0, 1.0, 1.0])
    for coef in ([1.0, -1.0], [1.0, float("nan")], [float("inf"), 0.0], [1e39, 0.0]):              # the library's refusals
        with pytest.raises(_abi.FedAggError) as e:
            ops.centered_clip_step([x, x], c, coef, dist=d2)
        assert e.value.status == _abi.FA_EINVAL
    buf = torch.zeros(12, device=DEV)
    with pytest.raises(_abi.FedAggError) as e:                                                     # a partial overlap
        ops.centered_clip_step([x, x], buf[:8], [1.0, 1.0], out=buf[4:], dist=d2)
    assert e.value.status == _abi.FA_EINVAL
    assert bool((buf == 0).all()) and bool((d2 == 0).all())
    with pytest.raises(_abi.FedAggError) as e:
        ops.cclip_geometry(torch.int8, 4)
    assert e.value.status == _abi.FA_EDTYPE


# ---- plug-in rounds --------------------------------------------------------------------------------
ROUNDS = [(4, 257), (5, 257), (10, 4099), (17, 4099), (64, 4099)]
FRACTION = 0.2
L = 3


def _byzantine_count(fraction, K):
    if K < 3:
        return 0
    return min(math.floor(fraction * K), (K - 3) // 2)


def _round_updates(seed, K, spec, fraction=FRACTION):
    """K updates of the model ``spec`` around the global model they started from, f = byzantine_count(fraction,
    K) of them hostile: the generator the robust rules' tests share
    (tests/robust_fuzz_cases.center_round_updates). Returns (updates, hostile indices, global model)."""
    return center_round_updates(seed, K, _byzantine_count(fraction, K), spec)


def _spec(P):
    return [((P,), np.float32), ((P // 4 + 3,), np.int32)]       # two dtype groups: f32 and i32


def _tau(spec):
    return 0.3 * math.sqrt(sum(int(np.prod(s)) for s, _ in spec))


def _run_round(ups, center, staged, parameters, budget=None, agg=None, uh=None):
    from fedn_amd.aggregators import get_aggregator
    from fedn_amd.ingest import StagingUpdateHandler
    from fedn_amd.updatehandler import MemoryUpdateHandler
    uh = uh or MemoryUpdateHandler()
    gid = uh.put_global_model(center) if center is not None else "no-such-model"
    st = StagingUpdateHandler(uh, helper=None, device=DEV, workers=2) if staged else None
    try:
        if agg is None:
            agg = get_aggregator("centeredclip", st or uh)
            agg.device, agg.hbm_budget = torch.device(DEV), budget
        mus = [uh.submit(u, 10 + k, model_id=gid, via=st) for k, u in enumerate(ups)]
        model, data = agg.combine_models(helper=None, parameters=parameters)
    finally:
        if st is not None:
            st.close()
    return model, data, uh, mus, agg, gid


def _flat64(model):
    return np.concatenate([np.asarray(a, dtype=np.float64).reshape(-1) for a in model])


def _check_robust(ups, hostile, center, model, iterations, tau, what):
    """The precondition in float64 on the CPU — the rule's result is at least 3 x nearer the honest
    clients' mean than the plain mean of the finite clients is, and nearer than the global model — then
    on the device result: at least 2 x nearer, and nearer than the global model."""
    K = len(ups)
    nan = _nan_clients(ups)
    honest = [k for k in range(K) if k not in hostile]
    _, v64 = cr.cclip_f64(ups, center, iterations, tau)
    X = np.stack([_flat64(u) for u in ups])
    target = X[honest].mean(axis=0)
    finite = [k for k in range(K) if k not in nan]
    plain = np.linalg.norm(X[finite].mean(axis=0) - target)
    start = np.linalg.norm(_flat64(center) - target)
    pre = np.linalg.norm(v64 - target)
    assert 3 * pre <= plain and pre < start, f"{what}: precondition: {pre} vs plain {plain}, global {start}"
    got = np.linalg.norm(_flat64(model) - target)
    print(f"{what}: distance to the honest mean {got:.4g} (float64 {pre:.4g}), the plain mean's {plain:.4g}, "
          f"the global model's {start:.4g}")
    assert 2 * got <= plain and got < start, f"{what}: {got} vs plain {plain}, global {start}"


@pytest.mark.parametrize("staged", [False, True], ids=["host", "staged"])
@pytest.mark.parametrize("K,P", ROUNDS)
def test_plugin_round(K, P, staged):
    spec = _spec(P)
    ups, hostile, center = _round_updates(0, K, spec)
    assert len(hostile) == _byzantine_count(FRACTION, K)
    if K in (17, 64):
        assert _nan_clients(ups), "these rounds exercise the exclusion path"
    tau = _tau(spec)
    model, data, uh, _, agg, gid = _run_round(ups, center, staged, {"tau": tau, "iterations": L})
    assert data["nr_aggregated_models"] == K, "excluded clients are counted"
    for key in ("time_model_load", "time_model_aggregation", "time_h2d", "time_kernel", "time_pack", "time_d2h"):
        assert key in data
    assert [a.dtype for a in model] == [np.dtype(np.float32), np.dtype(np.float64)]
    assert [a.shape for a in model] == [(P,), (P // 4 + 3,)]
    _check_chain(ups, center, agg, model, L, tau, f"K={K} P={P}")
    if K >= 5:
        _check_robust(ups, hostile, center, model, L, tau, f"K={K} P={P}")
    assert uh.model_updates.qsize() == 0, "the queue is drained"
    assert set(uh.store.models) == {gid}, "every update is deleted once the result exists; the global model stays"


def test_zero_iterations_returns_the_global_model():
    K, P = 10, 4099
    ups, _, center = _round_updates(0, K, _spec(P))
    model, data, _, _, agg, _ = _run_round(ups, center, False, {"tau": 1.0, "iterations": 0})
    assert data["nr_aggregated_models"] == K and len(agg.trace) == 1 and agg.excluded == _nan_clients(ups)
    assert_lists_identical(model, [center[0], center[1].astype(np.float64)], "iterations = 0")
    _check_chain(ups, center, agg, model, 0, 1.0, "iterations = 0")


def test_default_iterations():
    K, P = 10, 4099
    spec = _spec(P)
    ups, hostile, center = _round_updates(0, K, spec)
    model, data, _, _, agg, _ = _run_round(ups, center, False, {"tau": _tau(spec)})
    assert data["nr_aggregated_models"] == K
    _check_chain(ups, center, agg, model, 3, _tau(spec), "defaults")


def test_budget_keeps_updates_on_the_host(monkeypatch):
    """A budget of 3 updates with K = 12: nine stay on the host and every pass walks them slice by slice
    through the ring, the centre moved in place slice by slice. The slices change d's last bits and hence
    the coefficients, so the model is pinned by the round's own chain."""
    from fedn_amd import robust
    from fedn_amd.budget import HbmBudget
    from fedn_amd.layout import Layout
    K = 12
    spec = [((300, 200), np.float32), ((77,), np.int64), ((1001,), np.float32), ((), np.float32)]
    ups, hostile, center = _round_updates(0, K, spec)
    monkeypatch.setattr(robust, "SLICE_BYTES", 16384)
    budget = HbmBudget(limit=3 * Layout.of(ups[0]).nbytes)
    tau = _tau(spec)
    model, data, uh, _, agg, gid = _run_round(ups, center, False, {"tau": tau, "iterations": 2}, budget=budget)
    assert agg.host_side == 9 and data["nr_aggregated_models"] == K, "every update is counted"
    _check_chain(ups, center, agg, model, 2, tau, "budget")
    _check_robust(ups, hostile, center, model, 2, tau, "budget")
    assert set(uh.store.models) == {gid}
    del agg
    gc.collect()
    assert budget.used(DEV) == 0, "the round's reservations went back to the budget"


# ---- refusals and failures ---------------------------------------------------------------------------
def _kept(uh, mus, gid):
    return set(uh.store.models) == {m.model_update_id for m in mus} | ({gid} if gid in uh.store.models else set())


def test_more_than_64_updates_refused():
    ups, _, center = _round_updates(12, 65, [((33,), np.float32)])
    model, data, uh, mus, _, gid = _run_round(ups, center, False, {"tau": 1.0})
    assert model is None and data["nr_aggregated_models"] == 0
    assert uh.model_updates.qsize() == 0
    assert _kept(uh, mus, gid), "nothing is deleted"


@pytest.mark.parametrize("staged", [False, True], ids=["host", "staged"])
def test_layout_mismatch_is_skipped_and_kept(staged):
    K, P = 10, 4099
    spec = _spec(P)
    ups, _, center = _round_updates(0, K, spec)
    odd = [np.zeros((5, 3), dtype=np.float32), np.zeros(7, dtype=np.int32)]      # not this round's layout
    queue = ups[:3] + [odd] + ups[3:]
    model, data, uh, mus, agg, gid = _run_round(queue, center, staged, {"tau": _tau(spec)})
    assert data["nr_aggregated_models"] == K
    _check_chain(ups, center, agg, model, 3, _tau(spec), "layout mismatch")     # indices count the admitted updates
    assert set(uh.store.models) == {mus[3].model_update_id, gid}, "the skipped update stays in storage"


@pytest.mark.parametrize("case", ["missing", "shape", "count", "dtype"])
def test_global_model_missing_or_of_another_layout(case):
    K, P = 5, 257
    ups, _, center = _round_updates(0, K, _spec(P))
    bad = {"missing": None,
           "shape": [center[0][:-1], center[1]],
           "count": center[:1],
           "dtype": [center[0].astype(np.float64), center[1]]}[case]       # float64 is not float32's output type
    model, data, uh, mus, agg, gid = _run_round(ups, bad, False, {"tau": 1.0})
    assert model is None and data["nr_aggregated_models"] == 0 and agg.trace is None
    assert uh.model_updates.qsize() == 0
    assert _kept(uh, mus, gid), "nothing is deleted"


def test_float64_global_model_over_int32_updates():
    """After a round of this rule an int32 tensor of the model is float64: the next round takes it."""
    K, P = 5, 257
    spec = _spec(P)
    ups, _, center = _round_updates(0, K, spec)
    tau = _tau(spec)
    first, _, _, _, agg, _ = _run_round(ups, center, False, {"tau": tau, "iterations": 1})
    assert first[1].dtype == np.float64
    model, data, _, _, agg2, _ = _run_round(ups, first, False, {"tau": tau, "iterations": 1})
    assert data["nr_aggregated_models"] == K
    _check_chain(ups, first, agg2, model, 1, tau, "a float64 global model over int32 updates")
    as_f64 = [center[0], center[1].astype(np.float64)]
    again, _, _, _, agg3, _ = _run_round(ups, as_f64, False, {"tau": tau, "iterations": 1})
    assert_lists_identical(again, first, "the converted global model gives the int32 one's round")


def test_nan_in_the_global_model():
    """A NaN in the global model: every distance to it is non-finite — (None, data), nothing deleted."""
    K, P = 6, 257
    ups, _, center = _round_updates(5, K, [((P,), np.float32)])
    center[0][3] = np.nan
    model, data, uh, mus, agg, gid = _run_round(ups, center, False, {"tau": 1.0})
    assert model is None and data["nr_aggregated_models"] == 0 and agg.coefficients is None
    assert _kept(uh, mus, gid)


def test_failed_launch_keeps_every_update(monkeypatch):
    """A launch that fails (injected at the wrapper: no device fault): the round is (None, data), the
    updates stay in storage, and the aggregator's next round passes the chain."""
    from fedn_amd import _abi, ops
    K, P = 10, 4099
    spec = _spec(P)
    ups, _, center = _round_updates(0, K, spec)
    tau = _tau(spec)
    calls = []

    def boom(*a, **kw):
        calls.append(1)
        raise _abi.FedAggError(_abi.FA_EHIP, "centered_clip_step: injected failure")

    with monkeypatch.context() as mp:
        mp.setattr(ops, "centered_clip_step", boom)
        model, data, uh, mus, agg, gid = _run_round(ups, center, False, {"tau": tau})
    assert calls and model is None and data["nr_aggregated_models"] == 0
    assert uh.model_updates.qsize() == 0
    assert _kept(uh, mus, gid), "every update stays in storage"
    model, data, uh, mus2, _, gid2 = _run_round(ups, center, False, {"tau": tau}, agg=agg, uh=uh)
    assert data["nr_aggregated_models"] == K
    _check_chain(ups, center, agg, model, 3, tau, "the round after a failed launch")
    assert set(uh.store.models) == {mu.model_update_id for mu in mus} | {gid, gid2}
