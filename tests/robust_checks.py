"""Checks the robust GPU tests share: bitwise comparison, and the pass-by-pass chain checks of the
geometric median (tests/geomed_ref.py) and of centred clipping (tests/cclip_ref.py) against the trace a
``robust.RobustPipeline`` — or the plug-in that copies it — keeps of its own passes."""
import numpy as np

import cclip_ref as cr
import geomed_ref as gr
from golden_io import assert_lists_identical


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(f"u{a.dtype.itemsize}")


def same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    diff = bits(got) != bits(want)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} values differ, first at {int(np.argmax(diff))}"


def nan_clients(ups):
    return [k for k, u in enumerate(ups) if any(np.dtype(a.dtype).kind == "f" and not np.isfinite(a).all() for a in u)]


def rtol_of(ups):
    from fedn_amd import ops
    return max(ops.sqdist_rtol(np.asarray(a).dtype, np.asarray(a).size) for a in ups[0])


def check_geomed_chain(ups, agg, model, iterations, nu, what):
    """The Weiszfeld chain, pass by pass, from the pipeline's own trace: (a) beta_0 is 1/K_good with zeros
    on the excluded clients; (b) every d_t is within the bound of the oracle's distances to the oracle's
    mean at beta_t, non-finite where the oracle's are; (c) beta_t+1 is the host rule of d_t, bit for bit;
    (d) the model is the oracle's mean at the last beta, bit for bit."""
    K = len(ups)
    T = 0 if K == 1 else iterations
    trace = agg.trace
    assert len(trace) == T + 1, f"{what}: {len(trace)} passes for {iterations} iterations"
    want_excluded = nan_clients(ups)
    assert agg.excluded == want_excluded, f"{what}: excluded {agg.excluded}, the NaN clients are {want_excluded}"
    beta0 = np.full(K, 1.0 / (K - len(want_excluded)))
    beta0[want_excluded] = 0.0
    same_bits(np.asarray(trace[0][0]), beta0, f"{what}: (a) beta_0")
    rtol = rtol_of(ups)
    for t, (beta, d) in enumerate(trace):
        assert beta.dtype == np.float64 and d.dtype == np.float64 and beta.shape == d.shape == (K,)
        want = gr.model_dists(ups, beta)
        fin = np.isfinite(want)
        assert np.array_equal(np.isfinite(d), fin), f"{what}: (b) pass {t}: non-finite entries {d} vs {want}"
        assert sorted(np.flatnonzero(~fin).tolist()) == want_excluded
        err = np.abs(d[fin] - want[fin])
        worst = float((err / np.where(want[fin] > 0, want[fin], 1.0)).max())
        print(f"{what}: pass {t}: worst relative error {worst:.3e} (bound {rtol:.3e})")
        assert (err <= rtol * want[fin]).all(), f"{what}: (b) pass {t}"
        if t + 1 < len(trace):
            same_bits(np.asarray(trace[t + 1][0]), np.array(gr.weights(d, nu)), f"{what}: (c) beta_{t + 1}")
    same_bits(np.asarray(agg.weights), np.asarray(trace[-1][0]), f"{what}: weights")
    with np.errstate(invalid="ignore"):
        same_bits(np.asarray(agg.distances), np.sqrt(trace[-1][1]), f"{what}: distances")
    assert all(agg.weights[k] == 0 for k in want_excluded)
    assert_lists_identical(model, gr.model_wmean(ups, trace[-1][0]), f"{what}: (d) model")


def check_cclip_chain(ups, center, agg, model, iterations, tau, what):
    """The rule's chain, pass by pass, from the pipeline's own trace: (a) coef_0 is all zeros; (b) every
    d_t is within the bound of the oracle's distances to the replayed v_t, non-finite exactly for the NaN
    clients; (c) coef_t+1 is the host rule of d_t, bit for bit; (d) the model is the oracle's chain
    v_0 -> ... -> v_L replayed with the device's coefficients, bit for bit."""
    K = len(ups)
    trace = agg.trace
    assert len(trace) == iterations + 1, f"{what}: {len(trace)} passes for {iterations} iterations"
    want_excluded = nan_clients(ups)
    assert agg.excluded == want_excluded, f"{what}: excluded {agg.excluded}, the NaN clients are {want_excluded}"
    same_bits(np.asarray(trace[0][0]), np.zeros(K), f"{what}: (a) coef_0")
    rtol = rtol_of(ups)
    v = cr.model_center(ups, center)
    for t, (coef, d) in enumerate(trace):
        assert coef.dtype == np.float64 and d.dtype == np.float64 and coef.shape == d.shape == (K,)
        if t:
            v = cr.model_step(ups, v, coef)
        want = cr.model_dists(ups, v)
        fin = np.isfinite(want)
        assert np.array_equal(np.isfinite(d), fin), f"{what}: (b) pass {t}: non-finite entries {d} vs {want}"
        assert sorted(np.flatnonzero(~fin).tolist()) == want_excluded
        err = np.abs(d[fin] - want[fin])
        worst = float((err / np.where(want[fin] > 0, want[fin], 1.0)).max())
        print(f"{what}: pass {t}: worst relative error {worst:.3e} (bound {rtol:.3e})")
        assert (err <= rtol * want[fin]).all(), f"{what}: (b) pass {t}"
        if t + 1 < len(trace):
            same_bits(np.asarray(trace[t + 1][0]), np.array(cr.coefficients(d, tau)), f"{what}: (c) coef_{t + 1}")
    same_bits(np.asarray(agg.coefficients), np.asarray(trace[-1][0]), f"{what}: coefficients")
    with np.errstate(invalid="ignore"):
        same_bits(np.asarray(agg.distances), np.sqrt(trace[-1][1]), f"{what}: distances")
    assert all(c[k] == 0 for c, _ in trace for k in want_excluded)
    assert_lists_identical(model, v, f"{what}: (d) model")
