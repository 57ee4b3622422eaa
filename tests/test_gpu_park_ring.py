"""The generalised parked fold's client ring and parked-tile FIFO (fedavg_park_body<DEPTH, SLOTS> in
fedavg_kernels.h, k_fedavg_park): DEPTH client buffers in the load ring (the load cursor runs
DEPTH - 1 stream positions ahead of the consume cursor, across tile boundaries), SLOTS parked tiles
per workgroup in LDS.

Every case runs the probe library (fa_tune AUTO_GEOM 0, AVG_WIN_MODE 3, AVG_PARK_DEPTH / _SLOTS, an
explicit period and window), checks the kernel family of the launch, and compares the whole result
bit for bit with oracle/numpy_ref.py and with the mode-0 launch of the same inputs. fp32 throughout;
a tile is 4096 elements; C is the device's CU count, so GRID 1 runs C workgroups.

The shapes are the smallest at which the ring can go wrong: more tiles per workgroup than slots
under a window that is nearly never open (every slot fills, the bounded wait runs with a full FIFO,
slot indices wrap); a window that is always open (every poll flushes); fewer clients than ring
buffers (loads of two or three tiles in flight at once); streams shorter than the prologue; tile
counts around the grid size; the workload's 64 clients; a continuation launch behind the parked one.
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
_RESET = dict(auto_geom=1, grid=0, avg_win_period=0, avg_win_w=0, avg_win_mode=0, avg_park_depth=0, avg_park_slots=0)
COMBOS = [(d, s) for d in (2, 3, 4) for s in (1, 2, 4)]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _abi.load()


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@contextlib.contextmanager
def _probe(**knobs):
    with _abi.use_probe():
        try:
            ops.tune(**knobs)
            yield
        finally:
            ops.tune(**_RESET)


_cache = {}


def _inputs(K, P):
    """Inputs, oracle result and mode-0 result of (K, P): computed once, shared, never written."""
    if (K, P) not in _cache:
        _cache.clear()                                      # one shape's tensors on the device at a time
        rng = np.random.default_rng(K * 1_000_003 + P)
        base = rng.standard_normal(P)
        ups = [(base + 0.01 * rng.standard_normal(P)).astype(np.float32) for _ in range(K)]
        ns = [int(v) for v in rng.integers(1, 5001, K)]
        with np.errstate(all="ignore"):
            want = ref.fedavg_flat(ups, ns)
        dev = [torch.from_numpy(u).to(DEV) for u in ups]
        plain = _fold(dev, ns, 0, 600, 150, 0, 0, 0)
        for a in (want, plain):
            a.setflags(write=False)
        _cache[(K, P)] = (dev, ns, want, plain)
    return _cache[(K, P)]


def _fold(dev, ns, mode, period, w, grid, depth, slots):
    agg = torch.full((dev[0].numel(),), float("nan"), dtype=torch.float32, device=DEV)
    with _probe(auto_geom=0, grid=grid if mode == 3 else 0, avg_win_period=period, avg_win_w=w, avg_win_mode=mode,
                avg_park_depth=depth, avg_park_slots=slots):
        ops.fedavg_fold(agg, dev, ns, [int(v) for v in np.cumsum(ns)], init=True)
        assert ops.last_kernel() == WIN, f"mode {mode}"
    torch.cuda.synchronize()
    return agg.cpu().numpy()


def _case(K, P, depth, slots, period=600, w=150, grid=1):
    dev, ns, want, plain = _inputs(K, P)
    parked = _fold(dev, ns, 3, period, w, grid, depth, slots)
    what = f"K={K} P={P} depth={depth} slots={slots} period={period} w={w} grid={grid}"
    assert_lists_identical([parked], [want], what + " parked vs oracle")
    assert_lists_identical([parked], [plain], what + " parked vs mode 0")


@pytest.mark.parametrize("period,w", [(4096, 1), (512, 512), (600, 150)])
@pytest.mark.parametrize("depth,slots", COMBOS)
def test_ring_every_depth_and_slots(cus, depth, slots, period, w):
    """6 to 7 tiles per workgroup and a ragged tail. (4096, 1): every slot fills, the fallback wait
    runs with a full FIFO and the slot index wraps; (512, 512): every poll flushes."""
    _case(5, TILE * (6 * cus + 37) + 5, depth, slots, period, w)


@pytest.mark.parametrize("slots", [1, 4])
@pytest.mark.parametrize("K", [2, 3])
def test_ring_fewer_clients_than_buffers(cus, K, slots):
    """Depth 4 over K = 2 and 3: the ring holds clients of two or three tiles at once, and a tile is
    finished while the next one's first client is already in the ring."""
    _case(K, TILE * (3 * cus + 1) + 1, 4, slots)


@pytest.mark.parametrize("P", [TILE * 3, TILE])
def test_ring_stream_shorter_than_prologue(P):
    """Depth 4, K = 2: workgroups with one tile (a stream of two positions under a prologue that
    wants three) or none."""
    _case(2, P, 4, 1)
    _case(2, P, 4, 4)


@pytest.mark.parametrize("dp", [0, TILE, -1])
def test_ring_tile_counts_around_the_grid(cus, dp):
    """Exactly one tile each; one workgroup with two; the ragged tile owned by a workgroup (the last)
    whose own whole tile is gone."""
    _case(4, TILE * cus + dp, 3, 2)


def test_ring_64_clients():
    _case(64, TILE * 600 + 5, 4, 4, grid=2)


def test_ring_k70_continuation():
    """70 clients: the first 64 in the parked launch (depth 4, 4 slots), the other 6 continue from the
    stored aggregate in k_fedavg_pipe."""
    P, K = TILE * 300 + 77, 70
    rng = np.random.default_rng(K * 1_000_003 + P)
    base = rng.standard_normal(P)
    ups = [(base + 0.01 * rng.standard_normal(P)).astype(np.float32) for _ in range(K)]
    ns = [int(v) for v in rng.integers(1, 5001, K)]
    Ns = [int(v) for v in np.cumsum(ns)]
    with np.errstate(all="ignore"):
        want = ref.fedavg_flat(ups, ns)
    dev = [torch.from_numpy(u).to(DEV) for u in ups]
    got = {}
    for mode in (3, 0):
        agg = torch.full((P,), float("nan"), dtype=torch.float32, device=DEV)
        with _probe(auto_geom=0, grid=1 if mode == 3 else 0, avg_win_period=600, avg_win_w=150, avg_win_mode=mode,
                    avg_park_depth=4, avg_park_slots=4):
            ops.fedavg_fold(agg, dev[:64], ns[:64], Ns[:64], init=True)
            assert ops.last_kernel() == WIN
            ops.fedavg_fold(agg, dev[64:], ns[64:], Ns[64:], init=False)
            assert ops.last_kernel() == ("k_fedavg_pipe" if mode == 3 else WIN)
        torch.cuda.synchronize()
        got[mode] = agg.cpu().numpy()
    assert_lists_identical([got[3]], [want], "K=70 depth 4 slots 4 vs oracle")
    assert_lists_identical([got[3]], [got[0]], "K=70 depth 4 slots 4 vs mode 0")
