"""DP-FedAvg and centred clipping on rounds of MORE than 64 updates:
``RobustPipeline.dp_clipped_mean`` / ``centered_clip`` by chunks of 64 clients (``fa_clip_fold`` for the step,
``fa_centered_clip_step`` at zero coefficients for the distances) against the one-shot oracle
tests/cclip_ref.py, the noise against tests/dpnoise_ref.py on the device's deviates, with updates on the host
under a budget, and the ``dpfedavg`` plug-in end to end.

The rounds are ``center_round_updates(K, K, f, SPEC)`` at ``clip = 18``: each has clipped and unclipped
clients (asserted from the oracle's distances first, so a changed generator cannot empty a branch)."""
import functools
import gc

import numpy as np
import pytest
import torch

import cclip_ref as cr
import dpnoise_ref as dr
from golden_io import assert_lists_identical
from robust_checks import check_cclip_chain, nan_clients, rtol_of, same_bits
from robust_fuzz_cases import center_round_updates

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SPEC = [((37, 11), np.float32), ((129,), np.float16), ((5, 7), np.int32), ((1001,), np.float32), ((), np.float16)]
CLIP, NOISE, SEED, ROUND = 18.0, 1.3, 0x0123456789ABCDEF, 5
# K: (hostile clients, clipped, unclipped, excluded)
ROUNDS = {65: (0, 33, 32, []), 129: (3, 97, 31, [125]), 200: (0, 169, 31, [])}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from fedn_amd import _abi
    _abi.load()
    yield
    torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def _round(K):
    """The round of K updates, its global model and the oracle's distances to it (read only); the split into
    clipped, unclipped and excluded clients is asserted here."""
    f, clipped, unclipped, excluded = ROUNDS[K]
    ups, _, center = center_round_updates(K, K, f, SPEC)
    d0 = cr.model_dists(ups, cr.model_center(ups, center))
    fin = np.isfinite(d0)
    assert nan_clients(ups) == excluded == np.flatnonzero(~fin).tolist()
    with np.errstate(invalid="ignore"):
        r = np.sqrt(d0)
    assert (int((r[fin] > CLIP).sum()), int((r[fin] <= CLIP).sum())) == (clipped, unclipped), "the round's split"
    return ups, center, d0


def _pipe(ups, budget=None, cls=None):
    from fedn_amd import robust
    pipe = (cls or robust.RobustPipeline)(DEV, ups[0], tag=0, budget=budget)
    for k, u in enumerate(ups[1:], 1):
        pipe.add(u, tag=k)
    return pipe


@functools.lru_cache(maxsize=None)
def _z_gpu(seed, stream_id, round_id, P):
    """The device's deviates of ``[0, P)`` (float64 out, no x, sigma 1): once per range, read only."""
    from fedn_amd import ops
    z = torch.empty(P, dtype=torch.float64, device=DEV)
    ops.gaussian_noise(z, None, sigma=1.0, seed=seed, stream_id=stream_id, round_id=round_id)
    z = z.cpu().numpy()
    z.setflags(write=False)
    return z


def _noised(pipe, clipped, sigma, seed, round_id):
    """The applied rule on the clipped model: dtype group g takes stream g of the device's deviates."""
    want = [None] * len(clipped)
    lay = pipe.layout
    for g, dt in enumerate(lay.groups):
        flat = np.concatenate([np.asarray(clipped[i]).reshape(-1) for i, _ in sorted(lay.members[dt], key=lambda m: m[1])])
        full = dr.apply(flat, sigma, _z_gpu(seed, g, round_id, flat.size), flat.dtype)
        for i, off in lay.members[dt]:
            want[i] = full[off:off + lay.sizes[i]].reshape(lay.shapes[i])
    return want


def _check_pass0(ups, d, d0, what):
    fin = np.isfinite(d0)
    assert np.array_equal(np.isfinite(d), fin), f"{what}: non-finite distances {d} vs {d0}"
    err = np.abs(d[fin] - d0[fin])
    rtol = rtol_of(ups)
    print(f"{what}: pass 0: worst relative error {float((err / d0[fin]).max()):.3e} (bound {rtol:.3e})")
    assert (err <= rtol * d0[fin]).all(), f"{what}: pass 0 distances"


# ---- pipeline --------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", sorted(ROUNDS))
def test_pipeline_is_the_one_shot_rule(K):
    from fedn_amd import robust
    ups, center, d0 = _round(K)
    _, clipped, _, excluded = ROUNDS[K]
    what = f"K={K}"
    pipe = _pipe(ups)
    assert pipe.host_side == 0
    quiet = pipe.dp_clipped_mean(center, CLIP, 0.0, SEED, ROUND)
    assert len(pipe.trace) == 2 and not pipe.trace[0][0].any()
    d = pipe.trace[0][1]
    _check_pass0(ups, d, d0, what)
    coef = robust.clip_coefficients(d, CLIP)
    same_bits(pipe.coefficients, coef, f"{what}: the coefficients are the host rule of pass 0")
    same_bits(pipe.trace[1][0], coef, f"{what}: trace[1]")
    assert pipe.excluded == excluded and pipe.clipped == clipped and pipe.sigma == 0.0
    assert all(coef[k] == 0.0 for k in excluded)
    want = cr.model_step(ups, cr.model_center(ups, center), coef)
    assert_lists_identical(quiet, want, f"{what}: noise_multiplier = 0 is the one-shot step over all K")
    with np.errstate(invalid="ignore"):
        same_bits(pipe.distances, np.sqrt(pipe.trace[1][1]), f"{what}: distances")
    d1 = cr.model_dists(ups, want)
    fin = np.isfinite(d1)
    assert (np.abs(pipe.trace[1][1][fin] - d1[fin]) <= rtol_of(ups) * d1[fin]).all(), f"{what}: distances to v'"
    trace1 = pipe.trace[1][1].copy()

    noisy = pipe.dp_clipped_mean(center, CLIP, NOISE, SEED, ROUND)
    sigma = (np.float64(NOISE) * np.float64(CLIP)) / np.float64(K - len(excluded))
    assert pipe.sigma == sigma and pipe.excluded == excluded and pipe.clipped == clipped
    same_bits(pipe.coefficients, coef, f"{what}: the clipping pass does not depend on the noise")
    same_bits(pipe.trace[1][1], trace1, f"{what}: nor do its distances")
    assert_lists_identical(noisy, _noised(pipe, want, sigma, SEED, ROUND), f"{what}: clipped + sigma * z_gpu")
    assert not np.array_equal(noisy[0], quiet[0]), "the noise shows"
    again = pipe.dp_clipped_mean(center, CLIP, NOISE, SEED, ROUND)
    assert_lists_identical(again, noisy, f"{what}: two calls, the same bits")
    same_bits(pipe.trace[0][1], d, f"{what}: pass 0 again")
    pipe.release()


def test_centered_clip_chain_at_129():
    """Two iterations at K = 129: the rule's chain, pass by pass, from the pipeline's own trace."""
    ups, center, _ = _round(129)
    pipe = _pipe(ups)
    model = pipe.centered_clip(center, 2, CLIP)
    check_cclip_chain(ups, center, pipe, model, 2, CLIP, "centered_clip K=129")
    pipe.release()


def test_other_rules_keep_64():
    ups, center, _ = _round(65)
    pipe = _pipe(ups)
    for run in (lambda: pipe.result(0), lambda: pipe.select_mean(0, 1), lambda: pipe.bulyan(0),
                lambda: pipe.geometric_median(1, 1e-6)):
        with pytest.raises(ValueError, match="1..64 updates, got 65"):
            run()
    pipe.release()


def test_same_bits_with_updates_on_the_host(monkeypatch):
    """K = 129 under a budget of two updates, slices of 1 KiB: 127 updates go through the ring chunk by chunk
    and slice by slice; the model, every d and the coefficients are the in-HBM run's, and the budget is
    returned."""
    from fedn_amd import robust
    from fedn_amd.budget import HbmBudget
    from fedn_amd.layout import Layout
    K = 129
    ups, center, _ = _round(K)
    monkeypatch.setattr(robust, "SLICE_BYTES", 1024)         # (the in-HBM run walks these bounds too)
    in_hbm = _pipe(ups)
    want = in_hbm.dp_clipped_mean(center, CLIP, NOISE, SEED, 2)
    assert in_hbm.host_side == 0
    trace = [(c.copy(), d.copy()) for c, d in in_hbm.trace]
    in_hbm.release()
    budget = HbmBudget(limit=2 * Layout.of(ups[0]).nbytes)
    pipe = _pipe(ups, budget)
    assert pipe.host_side == K - 2
    got = pipe.dp_clipped_mean(center, CLIP, NOISE, SEED, 2)
    assert_lists_identical(got, want, "updates on the host")
    assert len(pipe.trace) == len(trace) == 2
    for t, ((c, d), (cw, dw)) in enumerate(zip(pipe.trace, trace)):
        same_bits(c, cw, f"pass {t}: coefficients")
        same_bits(d, dw, f"pass {t}: d")
    assert pipe.excluded == [125]
    pipe.release()
    del pipe
    gc.collect()
    assert budget.used(DEV) == 0


# ---- plug-in end to end ----------------------------------------------------------------------------
def _submit(uh, K):
    ups, center, _ = _round(K)
    gid = uh.put_global_model(center)
    return [uh.submit(u, 10 + k, model_id=gid) for k, u in enumerate(ups)], gid


def _aggregator(uh):
    from fedn_amd.aggregators import get_aggregator
    agg = get_aggregator("dpfedavg", uh)
    agg.device = torch.device(DEV)
    return agg


@pytest.mark.parametrize("K", [65, 129])
def test_plugin_aggregates_more_than_64(K):
    from fedn_amd.updatehandler import MemoryUpdateHandler
    ups, center, _ = _round(K)
    ref = _pipe(ups)
    want = ref.dp_clipped_mean(center, CLIP, NOISE, 77, 0)
    sigma, clipped, distances, excluded = ref.sigma, ref.clipped, ref.distances.copy(), list(ref.excluded)
    ref.release()
    uh = MemoryUpdateHandler()
    agg = _aggregator(uh)
    assert agg.max_updates == 1024
    _, gid = _submit(uh, K)
    model, data = agg.combine_models(helper=None, parameters={"clip": CLIP, "noise_multiplier": NOISE, "seed": 77})
    assert model is not None and data["nr_aggregated_models"] == K
    assert uh.model_updates.qsize() == 0 and set(uh.store.models) == {gid}, "the updates are deleted, the global model stays"
    assert agg.sigma == sigma and agg.clipped == clipped and agg.excluded == excluded
    same_bits(np.asarray(agg.distances), distances, f"K={K}: distances")
    assert_lists_identical(model, want, f"K={K}: the plug-in's model is the pipeline's")


def test_plugin_refuses_past_max_updates(monkeypatch):
    from fedn_amd.aggregators import dpfedavg
    from fedn_amd.updatehandler import MemoryUpdateHandler
    monkeypatch.setattr(dpfedavg.Aggregator, "max_updates", 70)
    ups, center, _ = _round(129)
    uh = MemoryUpdateHandler()
    gid = uh.put_global_model(center)
    mus = [uh.submit(u, 10 + k, model_id=gid) for k, u in enumerate(ups[:71])]
    agg = _aggregator(uh)
    model, data = agg.combine_models(helper=None, parameters={"clip": CLIP, "noise_multiplier": NOISE, "seed": 77})
    assert model is None and data["nr_aggregated_models"] == 0 and agg.sigma is None
    assert uh.model_updates.qsize() == 0, "the queue is drained"
    assert set(uh.store.models) == {m.model_update_id for m in mus} | {gid}, "nothing is deleted"
