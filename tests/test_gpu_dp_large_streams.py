"""The stream order of ``RobustPipeline.dp_clipped_mean`` on a round of more than 64 updates (the chunked
passes of fedn_amd/robust.py) under LATE LAUNCHES.

Every launch — the ``clip_fold`` launches of a slice, the ``centered_clip_step`` launches that take the
distances behind them and the ``gaussian_noise`` launches — is delayed by a device spin on the compute stream
(tests/late_streams.py; its wrapper list predates the fold and the noise op, so the subclass below adds them),
with the copy stream one that really runs beside it and a budget that sends four of seventy updates through
the ring. This pins the carry's reuse by the next slice behind the launch that last read it, the in-place
store of the centre's slice behind the last launch that takes differences to it, the distance launches
behind the fold that moves the slice, and the ring buffers' reuse. The expected bits are those of an
undelayed round, which tests/test_gpu_dp_large.py pins to the definition."""
import contextlib

import numpy as np
import pytest
import torch

from golden_io import assert_lists_identical
from late_streams import (DEV, LATE_OPS, LateLaunches, late_pipeline, poison_knob, require_side_by_side,
                          side_by_side_streams)
from robust_fuzz_cases import center_round_updates

pytestmark = pytest.mark.gpu

K = 70
SPEC = [((300, 200), np.float32), ((77,), np.int64), ((1001,), np.float32), ((), np.float32), ((513,), np.float16)]
SLICE = 65536            # robust.SLICE_BYTES here: the f32 group (61002 elements) takes 4 slices of 16384
HOST_SIDE = 4
CLIP, NOISE, SEED, ROUND = 40.0, 1.1, 0xC0FFEE, 3
FOLD_OP, NOISE_OP = "clip_fold", "gaussian_noise"


class LateWithFoldAndNoise(LateLaunches):
    """LateLaunches with the fold and the noise op among the delayed ones. A noise launch follows a pass whose
    distances the host has read (a synchronise), so it starts a walk of its own."""

    @contextlib.contextmanager
    def patched(self, monkeypatch):
        from fedn_amd import ops
        with super().patched(monkeypatch), monkeypatch.context() as mp:
            late = self._late(NOISE_OP, ops.gaussian_noise)

            def noise(*a, **kw):
                self.begin_walk()
                return late(*a, **kw)

            mp.setattr(ops, NOISE_OP, noise)
            mp.setattr(ops, FOLD_OP, self._late(FOLD_OP, ops.clip_fold))
            yield self


def _pipeline(ups, copy, late, budgeted):
    from fedn_amd.budget import HbmBudget
    from fedn_amd.layout import Layout

    class Chunked(late_pipeline(copy, late)):
        def _clip_pass_chunked(self, *a, **kw):          # a pass is one walk: the host reads d behind it
            if late is not None:
                late.begin_walk()
            return super()._clip_pass_chunked(*a, **kw)

    budget = HbmBudget(limit=(K - HOST_SIDE if budgeted else K) * Layout.of(ups[0]).nbytes)
    pipe = Chunked(DEV, ups[0], tag=0, budget=budget)
    for k, u in enumerate(ups[1:], 1):
        pipe.add(u, tag=k)
    assert pipe.host_side == (HOST_SIDE if budgeted else 0)
    return pipe


def test_late_chunked_round_has_the_undelayed_bits(monkeypatch):
    from fedn_amd import robust
    what = "dp_clipped_mean K=70, late"
    assert NOISE_OP not in LATE_OPS and FOLD_OP not in LATE_OPS
    monkeypatch.setattr(robust, "SLICE_BYTES", SLICE)
    ups, _, center = center_round_updates(0, K, 1, SPEC)
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")

    # undelayed rounds first: the expected bits, and warm code objects and pools
    plain = _pipeline(ups, None, None, True)
    want = plain.dp_clipped_mean(center, CLIP, NOISE, SEED, ROUND)
    coef = plain.coefficients.copy()
    assert 0 < plain.clipped < K, "precondition: clipped and unclipped clients"
    plain.release()
    in_hbm = _pipeline(ups, None, None, False)
    assert_lists_identical(in_hbm.dp_clipped_mean(center, CLIP, NOISE, SEED, ROUND), want, "in HBM vs through the ring")
    in_hbm.release()

    copy, compute = side_by_side_streams()
    with torch.cuda.stream(compute), poison_knob():
        spin_ms = require_side_by_side(copy, compute)
        for budgeted in (True, False):
            late = LateWithFoldAndNoise()
            with late.patched(monkeypatch):
                pipe = _pipeline(ups, copy, late, budgeted)
                got = pipe.dp_clipped_mean(center, CLIP, NOISE, SEED, ROUND)
            late.require_late(spin_ms, f"{what}, budgeted={budgeted}")
            names = [c["name"] for c in late.calls]
            groups = sum(1 for dt in pipe.layout.groups if pipe.layout.group_elems[dt])
            slices = 4 + 1 + 1                               # the f32 group's four, one each of i64 and f16
            assert names[-groups:] == [NOISE_OP] * groups, "one noise launch per dtype group, behind every other launch"
            assert names[:2 * slices] == ["centered_clip_step"] * (2 * slices), "pass 0: two chunks' distances per slice"
            assert names[2 * slices:-groups] == [FOLD_OP, FOLD_OP, "centered_clip_step", "centered_clip_step"] * slices, \
                "the moving pass: per slice both chunks' folds, then both chunks' distances"
            assert np.array_equal(pipe.coefficients, coef)
            for i, a in enumerate(got):
                assert not np.isnan(a).any(), f"{what}: NaN in tensor {i}: read before the copy landed"
            assert_lists_identical(got, want, f"{what}, budgeted={budgeted}: late vs undelayed")
            pipe.release()
