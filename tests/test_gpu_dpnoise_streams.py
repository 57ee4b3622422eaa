"""The stream order of ``RobustPipeline.dp_clipped_mean`` (fedn_amd/robust.py) under LATE LAUNCHES: the noise
launch of each dtype group must sit behind the clipping pass that moves the centre and ahead of the centre's
copy to the host.

Every launch — the two passes of ``centered_clip_step`` and the ``gaussian_noise`` launches — is delayed by a
device spin on the compute stream (tests/late_streams.py; its wrapper list predates the noise op, so the
subclass below adds it), with the copy stream one that really runs beside it and a budget that sends four
of six updates through the ring. A noise launch that ran ahead of the clipping pass would be overwritten by
it; a copy to the host that did not wait for the noise would carry the clipped model without it. The
expected bits are those of an undelayed round, which tests/test_gpu_dpnoise.py pins to the definition."""
import contextlib

import numpy as np
import pytest
import torch

from golden_io import assert_lists_identical
from late_streams import (DEV, LATE_OPS, LateLaunches, late_pipeline, poison_knob, require_side_by_side,
                          side_by_side_streams)
from robust_fuzz_cases import center_round_updates

pytestmark = pytest.mark.gpu

K = 6
SPEC = [((300, 200), np.float32), ((77,), np.int64), ((1001,), np.float32), ((), np.float32), ((513,), np.float16)]
SLICE = 16384            # robust.SLICE_BYTES here: the f32 group (61002 elements) takes 15 slices of 4096
HOST_SIDE = 4
CLIP, NOISE, SEED, ROUND = 40.0, 1.1, 0xC0FFEE, 3
NOISE_OP = "gaussian_noise"


class LateWithNoise(LateLaunches):
    """LateLaunches with the noise op among the delayed ones. A noise launch follows a pass whose distances
    the host has read (a synchronise), so it starts a walk of its own: precondition (b) speaks of the
    launches inside a sliced walk."""

    @contextlib.contextmanager
    def patched(self, monkeypatch):
        from fedn_amd import ops
        with super().patched(monkeypatch), monkeypatch.context() as mp:
            late = self._late(NOISE_OP, ops.gaussian_noise)

            def noise(*a, **kw):
                self.begin_walk()
                return late(*a, **kw)

            mp.setattr(ops, NOISE_OP, noise)
            yield self


def _pipeline(ups, copy, late, budgeted):
    from fedn_amd.budget import HbmBudget
    from fedn_amd.layout import Layout
    budget = HbmBudget(limit=(K - HOST_SIDE if budgeted else K) * Layout.of(ups[0]).nbytes)
    pipe = late_pipeline(copy, late)(DEV, ups[0], tag=0, budget=budget)
    for k, u in enumerate(ups[1:], 1):
        pipe.add(u, tag=k)
    assert pipe.host_side == (HOST_SIDE if budgeted else 0)
    return pipe


def _scrub_pinned(pipe):
    """Pinned blocks of the sizes the centre's groups take, filled with 0xFF and returned to torch's host
    pool: a result read before its D2H landed shows as NaN / -1."""
    sizes = {pipe.layout.group_elems[dt] * pipe._out_dt[dt].itemsize for dt in pipe.layout.groups}
    blocks = [torch.empty(n, dtype=torch.uint8, pin_memory=True) for n in sizes for _ in range(4)]
    for b in blocks:
        b.fill_(0xFF)
    del blocks


def test_late_noise_sits_between_the_clip_pass_and_the_copy_out(monkeypatch):
    from fedn_amd import robust
    what = "dp_clipped_mean, late"
    assert NOISE_OP not in LATE_OPS
    monkeypatch.setattr(robust, "SLICE_BYTES", SLICE)
    ups, _, center = center_round_updates(0, K, 1, SPEC)
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")

    # undelayed rounds first: the expected bits, and warm code objects and pools (precondition (b) compares
    # the spin with the host's steady work per slice)
    plain = _pipeline(ups, None, None, True)
    clipped = plain.centered_clip(center, 1, CLIP)
    want = plain.dp_clipped_mean(center, CLIP, NOISE, SEED, ROUND)
    assert not np.array_equal(want[0], clipped[0]), "precondition: the noise shows"
    plain.release()
    in_hbm = _pipeline(ups, None, None, False)
    assert_lists_identical(in_hbm.dp_clipped_mean(center, CLIP, NOISE, SEED, ROUND), want, "in HBM vs through the ring")
    in_hbm.release()

    copy, compute = side_by_side_streams()
    with torch.cuda.stream(compute), poison_knob():
        spin_ms = require_side_by_side(copy, compute)
        for budgeted in (True, False):
            late = LateWithNoise()
            with late.patched(monkeypatch):
                pipe = _pipeline(ups, copy, late, budgeted)
                _scrub_pinned(pipe)
                got = pipe.dp_clipped_mean(center, CLIP, NOISE, SEED, ROUND)
            late.require_late(spin_ms, f"{what}, budgeted={budgeted}")
            names = [c["name"] for c in late.calls]
            groups = sum(1 for dt in pipe.layout.groups if pipe.layout.group_elems[dt])
            assert names[-groups:] == [NOISE_OP] * groups and set(names[:-groups]) == {"centered_clip_step"}, \
                "one noise launch per dtype group, behind every clipping launch"
            for i, a in enumerate(got):
                assert not np.isnan(a).any(), f"{what}: NaN in tensor {i}: read before the copy landed"
            assert_lists_identical(got, want, f"{what}, budgeted={budgeted}: late vs undelayed")
            pipe.release()
