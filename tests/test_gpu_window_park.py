"""Store-window mode 3, "parked" (fedavg_park_body in fedavg_kernels.h): a persistent grid whose
workgroups park a finished tile in LDS, go on to their next tile and store the parked one when the
window opens.

Every case runs the probe library (fa_tune AUTO_GEOM 0, AVG_WIN_MODE 3, an explicit period and
window), checks the kernel family of the launch, and compares the whole result bit for bit with
oracle/numpy_ref.py and with the mode-0 launch of the same inputs. fp32 throughout; a tile is 4096
elements. GRID 1 gives one workgroup per CU, so a few hundred tiles already give every workgroup
several.

One case cannot name its kernel: fa_fedavg_fold copies a lone first client without a launch, so
K = 1 reaches no fold kernel in either mode; its bits are still compared.
"""
import contextlib

import numpy as np
import pytest
import torch

from golden_io import assert_lists_identical
from oracle import numpy_ref as ref

from fedn_amd import _abi, ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TILE = 4096
WIN = "k_fedavg_pipe_win"
_RESET = dict(auto_geom=1, grid=0, avg_win_period=0, avg_win_w=0, avg_win_mode=0)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _abi.load()


@contextlib.contextmanager
def _probe(**knobs):
    with _abi.use_probe():
        try:
            ops.tune(**knobs)
            yield
        finally:
            ops.tune(**_RESET)


def _inputs(K, P):
    rng = np.random.default_rng(K * 1_000_003 + P)
    base = rng.standard_normal(P)
    ups = [(base + 0.01 * rng.standard_normal(P)).astype(np.float32) for _ in range(K)]
    ns = [int(v) for v in rng.integers(1, 5001, K)]
    return ups, ns


def _fold(dev, ns, mode, period, w, grid, kernel=WIN):
    """One first launch under ``mode``; the family it ran is checked unless ``kernel`` is None."""
    agg = torch.full((dev[0].numel(),), float("nan"), dtype=torch.float32, device=DEV)
    with _probe(auto_geom=0, grid=grid if mode == 3 else 0, avg_win_period=period, avg_win_w=w, avg_win_mode=mode):
        ops.fedavg_fold(agg, dev, ns, [int(v) for v in np.cumsum(ns)], init=True)
        if kernel is not None:
            assert ops.last_kernel() == kernel, f"mode {mode}"
    torch.cuda.synchronize()
    return agg.cpu().numpy()


def _case(K, P, period, w, grid=1, kernel=WIN):
    ups, ns = _inputs(K, P)
    with np.errstate(all="ignore"):
        want = ref.fedavg_flat(ups, ns)
    dev = [torch.from_numpy(u).to(DEV) for u in ups]
    parked = _fold(dev, ns, 3, period, w, grid, kernel)
    plain = _fold(dev, ns, 0, period, w, grid, kernel)
    what = f"K={K} P={P} period={period} w={w} grid={grid}"
    assert_lists_identical([parked], [want], what + " parked vs oracle")
    assert_lists_identical([parked], [plain], what + " parked vs mode 0")


@pytest.mark.parametrize("K", [3, 64])
def test_park_several_tiles_and_ragged_tail(K):
    """600 tiles and 5 elements over one workgroup per CU: two to three tiles each, and the ragged
    tile handed to a workgroup that holds a parked one."""
    _case(K, TILE * 600 + 5, 600, 150)


@pytest.mark.parametrize("P", [TILE * 255, TILE * 3])
def test_park_one_tile_per_workgroup(P):
    """Parked once, stored by the end of the sweep alone; and fewer tiles than the grid."""
    _case(2, P, 600, 150)


@pytest.mark.parametrize("period,w", [(512, 512), (4096, 1)])
def test_park_window_always_open_and_nearly_never(period, w):
    """Always open: stored at the first poll. One tick in 4096: mostly by the bounded wait before
    the next tile is parked."""
    _case(5, TILE * 700, period, w)


def test_park_two_clients():
    _case(2, TILE * 520 + 1, 600, 150)


def test_park_one_client():
    """No client loop, so no poll; fa_fedavg_fold makes a lone first client a copy (no kernel to name)."""
    _case(1, TILE * 520 + 1, 600, 150, kernel=None)


def test_park_k70_continuation_unparked():
    """70 clients: the first 64 in the parked launch, the other 6 continue from the stored aggregate
    in k_fedavg_pipe."""
    P, K = TILE * 300 + 77, 70
    ups, ns = _inputs(K, P)
    Ns = [int(v) for v in np.cumsum(ns)]
    with np.errstate(all="ignore"):
        want = ref.fedavg_flat(ups, ns)
    dev = [torch.from_numpy(u).to(DEV) for u in ups]
    got = {}
    for mode in (3, 0):
        agg = torch.full((P,), float("nan"), dtype=torch.float32, device=DEV)
        with _probe(auto_geom=0, grid=1 if mode == 3 else 0, avg_win_period=600, avg_win_w=150, avg_win_mode=mode):
            ops.fedavg_fold(agg, dev[:64], ns[:64], Ns[:64], init=True)
            assert ops.last_kernel() == WIN
            ops.fedavg_fold(agg, dev[64:], ns[64:], Ns[64:], init=False)
            # (mode 0's forced window covers continuation launches too; mode 3 is for first launches)
            assert ops.last_kernel() == ("k_fedavg_pipe" if mode == 3 else WIN)
        torch.cuda.synchronize()
        got[mode] = agg.cpu().numpy()
    assert_lists_identical([got[3]], [want], "K=70 parked vs oracle")
    assert_lists_identical([got[3]], [got[0]], "K=70 parked vs mode 0")


@pytest.mark.parametrize("which", ["aggregate", "update"])
def test_park_misaligned_takes_todays_kernel(which):
    """A buffer off 16-B alignment takes the scalar (E = 1) route, whatever the window mode."""
    P, K = TILE * 40 + 3, 3
    ups, ns = _inputs(K, P)
    Ns = [int(v) for v in np.cumsum(ns)]
    with np.errstate(all="ignore"):
        want = ref.fedavg_flat(ups, ns)
    dev = [torch.from_numpy(u).to(DEV) for u in ups]
    if which == "update":
        pad = torch.empty(P + 1, dtype=torch.float32, device=DEV)
        pad[1:].copy_(dev[1])
        dev[1] = pad[1:]
    got, kern = {}, {}
    for mode in (3, 0):
        buf = torch.full((P + 1,), float("nan"), dtype=torch.float32, device=DEV)
        agg = buf[1:] if which == "aggregate" else buf[:P]
        with _probe(auto_geom=0, grid=1 if mode == 3 else 0, avg_win_period=600, avg_win_w=150, avg_win_mode=mode):
            ops.fedavg_fold(agg, dev, ns, Ns, init=True)
            kern[mode] = ops.last_kernel()
        torch.cuda.synchronize()
        got[mode] = agg.cpu().numpy()
    assert kern[3] == kern[0] and kern[3] != WIN, kern
    assert_lists_identical([got[3]], [want], f"misaligned {which} vs oracle")
    assert_lists_identical([got[3]], [got[0]], f"misaligned {which} vs mode 0")
