"""Seeded fuzz of the five robust entry points at ops level — ``ops.trimmed_mean``,
``ops.median_window_mean``, ``ops.pairwise_sqdist``, ``ops.weighted_mean_sqdist``,
``ops.centered_clip_step`` — with every client in an allocation of its own.

The entry points decide "16-byte path or scalar path" as an AND over every client pointer, and the matrix
tests pass the clients as rows of one matrix: all aligned or all shifted by one. Here every client lives
in its own ``guarded_buf.Buf`` with its own shift of 0-3 elements past a 16-byte boundary — all aligned,
exactly one unaligned, all unaligned and random mixes over the seed range — and so do the output, the
centre and the distances. The guards are NaNs no computation produces (large integers for the integer
dtypes): a READ past either end of an input that reaches the arithmetic poisons the result and fails the
value check, which separate allocations alone make visible; a write past an output's end, an element never
written and a changed input show in the buffers' own checks.

Each seed draws the entry point, one of the six dtypes (bf16 as exact upcasts), K in 1..64 biased to the
sorting networks' widths and their neighbours, and P among 1..9, 1024 m + (-3..3) and the kernel's own tile
length TE - 1, TE, TE + 1, 2 TE + 3 (P <= 70 000). The oracle call and the bar are the op's matrix test's:
values bit for bit (NaN by position), distances within ``ops.sqdist_rtol``, D symmetric with a zero
diagonal. Extended runs: FEDN_AMD_FUZZ_BASE / FEDN_AMD_FUZZ_SCALE as in tests/test_gpu_fuzz.py."""
import numpy as np
import pytest
import torch

import bulyan_ref as br
import cclip_ref as cr
import geomed_ref as gr
import krum_ref as kr
import robust_ref as rr
from guarded_buf import SENTINEL, TORCH_DT, Buf
from robust_checks import same_bits
from test_gpu_cclip import _coef
from test_gpu_cclip import _data as _center_data
from test_gpu_fuzz import _seeds
from test_gpu_geomed import _beta
from test_gpu_krum import _data as _near_data
from test_gpu_robust import _random, _same

pytestmark = pytest.mark.gpu

OPS = ["trimmed_mean", "median_window_mean", "pairwise_sqdist", "weighted_mean_sqdist", "centered_clip_step"]
DTYPES = ["f32", "f64", "f16", "bf16", "i32", "i64"]
OUT_NAME = {"f32": "f32", "f64": "f64", "f16": "f16", "bf16": "f32", "i32": "f64", "i64": "f64"}
ITEM = {"f32": 4, "f64": 8, "f16": 2, "bf16": 2, "i32": 4, "i64": 8}
KPS = [1, 2, 4, 8, 16, 32, 64]
P_MAX = 70_000
ALIGNMENTS = ["all aligned", "one unaligned", "all unaligned", "random"]
SEEDS = _seeds(40)
_WORST = {}                        # dtype -> (worst relative distance error, its bound)
_SEEN = set()


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from fedn_amd import _abi
    _abi.load()
    yield
    torch.cuda.synchronize()
    print("\nrobust ops fuzz: worst relative distance error per dtype (its bound): " +
          ", ".join(f"{n} {w:.3e} ({b:.3e})" for n, (w, b) in sorted(_WORST.items())))
    print(f"robust ops fuzz: alignments seen {sorted(_SEEN)}")


def _draw(seed):
    """(rng, op, dtype name, K, P, alignment kind) of a seed: the op and the alignment kind rotate so that
    every pair occurs within 20 consecutive seeds, the rest is random."""
    from fedn_amd import ops
    rng = np.random.default_rng([31_000, seed])
    op = OPS[seed % 5]
    kind = ALIGNMENTS[(seed // 5) % 4]
    name = DTYPES[int(rng.integers(0, 6))]
    if rng.random() < 0.6:
        K = int(np.clip(KPS[int(rng.integers(0, 7))] + int(rng.integers(-1, 2)), 1, 64))
    else:
        K = int(rng.integers(1, 65))
    geometry = {"pairwise_sqdist": ops.sqdist_geometry, "weighted_mean_sqdist": ops.wmean_geometry,
                "centered_clip_step": ops.cclip_geometry}.get(op)
    sizes = [1024 * int(rng.integers(1, 69)) + int(rng.integers(-3, 4))]
    r = rng.random()
    if r < 0.3:
        sizes = [int(rng.integers(1, 10))]
    elif r < 0.6 and geometry is not None:
        te = geometry(TORCH_DT[name], K)[0]
        sizes = [p for p in (te - 1, te, te + 1, 2 * te + 3) if 1 <= p <= P_MAX] or sizes
    P = sizes[int(rng.integers(0, len(sizes)))]
    assert 1 <= P <= P_MAX
    return rng, op, name, K, P, kind


def _shifts(rng, kind, K, name):
    """Each client's shift in elements; ``unaligned`` shifts are those that leave the 16-byte grid."""
    off = [s for s in (1, 2, 3) if s * ITEM[name] % 16]

    def pick():
        return off[int(rng.integers(0, len(off)))]

    if kind == "all aligned":
        return [0] * K
    if kind == "all unaligned":
        return [pick() for _ in range(K)]
    if kind == "one unaligned":
        shifts = [0] * K
        shifts[int(rng.integers(0, K))] = pick()
        return shifts
    return [int(rng.integers(0, 4)) for _ in range(K)]


def _untouched(buf, what):
    """An output the call was told to leave alone: every element and both guards still the sentinel."""
    buf.check(what, False)
    assert (buf.bits() == SENTINEL[buf.size]).all(), f"{what}: an output that was to be left alone was written"


def _check_sums(got, want, rtol, name, what):
    """Every distance within rtol of the reference, relatively, and finite (a guard that was read is not)."""
    assert got.dtype == np.float64 and got.shape == want.shape, (what, got.dtype, got.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite distances"
    err = np.abs(got - want)
    worst = float((err / np.where(want > 0, want, 1.0)).max()) if err.size else 0.0
    print(f"{what}: worst relative error {worst:.3e} (bound {rtol:.3e})")
    if worst >= _WORST.get(name, (-1.0, 0.0))[0]:
        _WORST[name] = (worst, rtol)
    assert (err <= rtol * want).all(), f"{what}: relative error {worst:.3e} exceeds {rtol:.3e}"


@pytest.mark.parametrize("seed", SEEDS)
def test_fuzz_ops(seed):
    from fedn_amd import ops
    rng, op, name, K, P, kind = _draw(seed)
    shifts = _shifts(rng, kind, K, name)
    oshift = int(rng.integers(0, 4))
    what = f"seed {seed} {op} {name} K={K} P={P} {kind} shifts {shifts} out shift {oshift}"
    print(what)
    unaligned = sum(1 for s in shifts if s * ITEM[name] % 16)
    _SEEN.add("all aligned" if not unaligned else "all unaligned" if unaligned == K else
              "one unaligned" if unaligned == 1 else "some unaligned")
    tdt, oname = TORCH_DT[name], OUT_NAME[name]
    rtol = ops.sqdist_rtol(tdt, P)
    center = None
    if op in ("trimmed_mean", "median_window_mean"):
        S = _random(rng, name, K, P)                            # ties, +-0, +-inf, NaNs in the first quarter
    elif op == "centered_clip_step":
        S, center = _center_data(rng, name, K, P)
    else:
        S = _near_data(rng, name, K, P)
    bufs = [Buf(P, name, shift=shifts[k], data=S[k]) for k in range(K)]
    views = [b.t for b in bufs]
    assert [bool(v.data_ptr() % 16) for v in views] == [bool(s * ITEM[name] % 16) for s in shifts]
    out = Buf(P, oname, shift=oshift)

    if op == "trimmed_mean":
        t = int(rng.integers(0, (K - 1) // 2 + 1))
        ops.trimmed_mean(out.t, views, t)
        assert ops.last_kernel() == "k_order_mean"
        _same(out.numpy(), rr.mean_of_sorted(rr.sorted_values(S), t), f"{what} trim={t}")
        out.check(what, written=True)
    elif op == "median_window_mean":
        keep = int(rng.integers(1, K + 1))
        ops.median_window_mean(out.t, views, keep)
        assert ops.last_kernel() == "k_median_window"
        _same(out.numpy(), br.window_mean(S, keep), f"{what} keep={keep}")
        out.check(what, written=True)
    elif op == "pairwise_sqdist":
        accumulate = bool(rng.integers(0, 2))
        D = Buf(K * K, "f64", shift=int(rng.integers(0, 2)))
        ops.pairwise_sqdist(views, out=D.t)
        assert ops.last_kernel() == "k_pair_sqdist"
        got = D.numpy().reshape(K, K)
        assert np.array_equal(got, got.T), f"{what}: not symmetric"
        assert (np.diag(got) == 0).all() and not np.signbit(np.diag(got)).any(), f"{what}: diagonal"
        _check_sums(got, kr.sqdist(S), rtol, name, what)
        D.check(what, written=True)
        if accumulate:                                          # added to what the matrix holds: the f64 sum
            before = rng.uniform(0.0, 10.0, K * K)
            A = Buf(K * K, "f64", shift=int(rng.integers(0, 2)), data=before)
            ops.pairwise_sqdist(views, out=A.t, accumulate=True)
            same_bits(A.numpy(), before + got.reshape(-1), f"{what}: accumulate")
            A.check(what, written=True)
    else:
        accumulate, store = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
        before = rng.uniform(0.0, 10.0, K) if accumulate else None
        dist = Buf(K, "f64", shift=int(rng.integers(0, 2)), data=before)
        if op == "weighted_mean_sqdist":
            w = _beta(rng, K)
            z = gr.wmean(S, w)
            ops.weighted_mean_sqdist(views, w, out=out.t, dist=dist.t, accumulate=accumulate, store=store)
            assert ops.last_kernel() == "k_wmean_dist"
            want_d = gr.dists(S, z)
            target = out
        else:
            w = _coef(rng, K)
            z = cr.step(S, center, w)
            in_place = store and bool(rng.integers(0, 2))
            cen = Buf(P, oname, shift=int(rng.integers(0, 4)), data=center)
            target = cen if in_place else out
            ops.centered_clip_step(views, cen.t, w, out=target.t, dist=dist.t, accumulate=accumulate, store=store)
            assert ops.last_kernel() == "k_cclip_dist"
            want_d = cr.dists(S, z)
            what += f" in_place={in_place}"
            if in_place:
                _untouched(out, what)
            else:
                cen.check_unchanged(f"{what}: the out-of-place centre")
        what += f" accumulate={accumulate} store={store}"
        if store:
            same_bits(target.numpy(), z, f"{what}: the point")
            target.check(what, written=True)                    # (in place: the centre's guards)
        else:
            _untouched(out, what)
        got = dist.numpy()
        if accumulate:                                          # the call's own sums: what it added
            fresh = Buf(K, "f64")
            (ops.weighted_mean_sqdist if op == "weighted_mean_sqdist" else ops.centered_clip_step)(
                *((views, w) if op == "weighted_mean_sqdist" else (views, Buf(P, oname, data=center).t, w)),
                dist=fresh.t, store=False)
            same_bits(got, before + fresh.numpy(), f"{what}: accumulate is the f64 sum")
            got = fresh.numpy()
            fresh.check(what, written=True)
        _check_sums(got, want_d, rtol, name, what)
        dist.check(what, written=True)
    for k, b in enumerate(bufs):
        b.check_unchanged(f"{what}: update {k}")


def test_the_seed_range_covers_every_alignment():
    """All-aligned, exactly-one-unaligned and all-unaligned calls occur for every entry point within the
    default seeds (the draw alone: no launch)."""
    seen = set()
    for seed in range(40):
        rng, op, name, K, P, kind = _draw(seed)
        shifts = _shifts(rng, kind, K, name)
        n = sum(1 for s in shifts if s * ITEM[name] % 16)
        seen.add((op, "aligned" if n == 0 else "all" if n == K else "one" if n == 1 else "some"))
    for op in OPS:
        for kind in ("aligned", "one", "all"):
            assert (op, kind) in seen, (op, kind)
