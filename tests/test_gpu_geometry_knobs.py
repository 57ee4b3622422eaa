"""The FedAvg geometry sweep of the probe library (fa_tune STRIPS / UNROLL / NT / LANETAB / BLOCK /
NT_STORE / NARROW / GRID; probe_fedavg_geometry in probes.h) against the oracle, in full, bit for bit.

Every geometry the sweep table instantiates folds fp32 and bf16 updates into an fp32 aggregate at
the smallest shapes at which these kernels can still go wrong, with AUTO_GEOM 0 so that the knobs
hold at every size. After each launch ops.last_kernel() must name the kernel family the setting
selects (k_fedavg_pipe for UNROLL 0, k_fedavg otherwise), so no case passes on the bits of the
1 x 8 fallback that a combination missing from the table would run.
"""
import functools

import numpy as np
import pytest
import torch

from golden_io import assert_lists_identical
from oracle import numpy_ref as ref

from fedn_amd import _abi, ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_DEFAULTS = dict(strips=4, unroll=0, nt=0, lanetab=0, grid=0, block=256, nt_store=1, narrow=1, auto_geom=1)

# The largest instantiated tile is 32 768 elements (512 lanes x 8 strips x 8 bf16). 65 579: two such
# tiles, then ragged strips and a 3-element strip end; 1 000: a tail only. K even and odd through the
# pipelined kernel's ping-pong.
SHAPES = [(K, P) for P in (65_579, 1_000) for K in (2, 5)]

# (strips, unroll, nt) of k_fedavg, then of k_fedavg_pipe (unroll 0): the sweep table, whole
TRIPLES = [(1, 4, 0), (1, 8, 0), (1, 16, 0), (2, 4, 0), (2, 8, 0), (2, 16, 0), (4, 1, 0), (4, 2, 0), (4, 4, 0),
           (8, 1, 0), (8, 2, 0), (16, 1, 0), (1, 8, 1), (4, 2, 1), (8, 1, 1),
           (2, 0, 0), (4, 0, 0), (8, 0, 0), (4, 0, 1)]
SETTINGS = ([dict(strips=s, unroll=u, nt=nt) for s, u, nt in TRIPLES] +
            [dict(strips=s, lanetab=1) for s in (2, 4, 8)] +
            [dict(strips=s, block=512) for s in (4, 8)] +
            [dict(strips=s, block=1024) for s in (2, 4)] +
            [dict(nt_store=v) for v in (0, 1, 2)] +
            [dict(narrow=v) for v in (0, 1)])


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _abi.load()


@functools.lru_cache(maxsize=None)
def _case(dt, K, P):
    """K clients of P elements on the device in ``dt``, their example counts, and the oracle's fold
    of what the device holds (bf16 is defined by its exact upcast). Made once, never written."""
    rng = np.random.default_rng(K * 1_000_003 + P)
    base = rng.standard_normal(P)
    ups = [(base + 0.01 * rng.standard_normal(P)).astype(np.float32) for _ in range(K)]
    ns = [int(v) for v in rng.integers(1, 5001, K)]
    if dt == "bf16":
        dev = [torch.from_numpy(u).to(torch.bfloat16).to(DEV) for u in ups]
        ups = [d.float().cpu().numpy() for d in dev]
    else:
        dev = [torch.from_numpy(u).to(DEV) for u in ups]
    with np.errstate(all="ignore"):
        want = ref.fedavg_flat(ups, ns)
    return dev, ns, [int(v) for v in np.cumsum(ns)], want


def _check(knobs, shapes, dts=("f32", "bf16")):
    kernel = "k_fedavg_pipe" if knobs.get("unroll", 0) == 0 else "k_fedavg"
    with _abi.use_probe():
        try:
            ops.tune(**{**_DEFAULTS, **knobs, "auto_geom": 0})
            for dt in dts:
                for K, P in shapes:
                    dev, ns, Ns, want = _case(dt, K, P)
                    agg = torch.full((P,), float("nan"), dtype=torch.float32, device=DEV)
                    ops.fedavg_fold(agg, dev, ns, Ns, init=True)
                    assert ops.last_kernel() == kernel, f"{knobs} {dt} K={K} P={P}"
                    torch.cuda.synchronize()
                    assert_lists_identical([agg.cpu().numpy()], [want], f"{knobs} {dt} K={K} P={P}")
        finally:
            ops.tune(**_DEFAULTS)


@pytest.mark.parametrize("knobs", SETTINGS, ids=lambda k: "-".join(f"{n}{v}" for n, v in k.items()))
def test_geometry_matches_oracle(knobs):
    _check(knobs, SHAPES)


def test_default_geometry_continuation_launch():
    """66 clients: a second launch continues from the stored aggregate (INIT = false)."""
    _check({}, [(66, 65_579), (66, 1_000)])


def test_persistent_grid_takes_several_tiles_per_workgroup():
    """GRID 1: at most one workgroup per CU sweeps 601 tiles of 4 096 elements, the last one ragged."""
    _check(dict(grid=1), [(3, 4096 * 600 + 5)], dts=("f32",))
