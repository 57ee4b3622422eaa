"""The parked fold's tall tiles and the ring's load policy (fedavg_park_body<DEPTH, SLOTS, HEIGHT, POL>
in fedavg_kernels.h, k_fedavg_park): a workgroup visits each client for HEIGHT
consecutive 16 KiB pieces, so the stream of positions is (tall tile, client, piece), the loop is
unrolled lcm(DEPTH, HEIGHT) times, a parked tile is HEIGHT pieces of LDS, and what is no whole tall
tile (up to HEIGHT - 1 whole tiles and the ragged one) goes through the tail path in workgroups of
its own (park_partition.h).

Every case runs the probe library (fa_tune AUTO_GEOM 0, AVG_WIN_MODE 3, AVG_PARK_DEPTH / _SLOTS /
_HEIGHT / _LOADPOL, an explicit period and window), checks the kernel family of the launch, and
compares the whole result bit for bit with oracle/numpy_ref.py and with the mode-0 launch of the
same inputs. fp32 throughout; T is a tile of 4096 elements, H the height; C is the device's CU count,
so GRID 1 runs C workgroups.

The shapes are the smallest at which the new code can go wrong: an odd K, so that a tall tile's
K * H positions are no multiple of the unroll, with 6 to 7 tall tiles per workgroup, H - 1 leftover
whole tiles and a ragged one, under a window that is nearly never open, one that is always open and
an ordinary one; no tall tile at all; one; tall-tile counts around the grid size; fewer clients than
the ring has buffers at DEPTH 3 (the ring spans a client and a tile boundary at once); the
workload's 64 clients on a grid of two per CU; a continuation launch behind the parked one; every
load policy.
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
T = 4096
WIN = "k_fedavg_pipe_win"
_RESET = dict(auto_geom=1, grid=0, avg_win_period=0, avg_win_w=0, avg_win_mode=0, avg_park_depth=0, avg_park_slots=0,
              avg_park_height=0, avg_park_loadpol=0)
# every instantiated (DEPTH, HEIGHT, SLOTS): the nine of height 1, ring 2 at the three tall shapes 64 KiB
# of static LDS allow, ring 3 at height 2
COMBOS = ([(d, 1, s) for d in (2, 3, 4) for s in (1, 2, 4)] + [(2, 2, 1), (2, 2, 2), (2, 4, 1), (3, 2, 1), (3, 2, 2)])
TALL = [c for c in COMBOS if c[1] > 1]


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
        if len(_cache) >= 3:                                # the three heights' shapes of one test at a time
            _cache.clear()
        rng = np.random.default_rng(K * 1_000_003 + P)
        base = rng.standard_normal(P)
        ups = [(base + 0.01 * rng.standard_normal(P)).astype(np.float32) for _ in range(K)]
        ns = [int(v) for v in rng.integers(1, 5001, K)]
        with np.errstate(all="ignore"):
            want = ref.fedavg_flat(ups, ns)
        dev = [torch.from_numpy(u).to(DEV) for u in ups]
        plain = _fold(dev, ns, 0, 600, 150, 0, 0, 0, 0, 0)
        for a in (want, plain):
            a.setflags(write=False)
        _cache[(K, P)] = (dev, ns, want, plain)
    return _cache[(K, P)]


def _fold(dev, ns, mode, period, w, grid, depth, height, slots, pol):
    agg = torch.full((dev[0].numel(),), float("nan"), dtype=torch.float32, device=DEV)
    with _probe(auto_geom=0, grid=grid if mode == 3 else 0, avg_win_period=period, avg_win_w=w, avg_win_mode=mode,
                avg_park_depth=depth, avg_park_slots=slots, avg_park_height=height, avg_park_loadpol=pol):
        ops.fedavg_fold(agg, dev, ns, [int(v) for v in np.cumsum(ns)], init=True)
        assert ops.last_kernel() == WIN, f"mode {mode}"
    torch.cuda.synchronize()
    return agg.cpu().numpy()


def _case(K, P, depth, height, slots, period=600, w=150, grid=1, pol=0):
    dev, ns, want, plain = _inputs(K, P)
    parked = _fold(dev, ns, 3, period, w, grid, depth, height, slots, pol)
    what = f"K={K} P={P} depth={depth} height={height} slots={slots} pol={pol} period={period} w={w} grid={grid}"
    assert_lists_identical([parked], [want], what + " parked vs oracle")
    assert_lists_identical([parked], [plain], what + " parked vs mode 0")


def _first_shape(cus, H):
    """6 to 7 tall tiles per workgroup, H - 1 leftover whole tiles, a ragged tile of 5."""
    return T * H * (6 * cus + 37) + T * (H - 1) + 5


@pytest.mark.parametrize("period,w", [(4096, 1), (512, 512), (600, 150)])
@pytest.mark.parametrize("depth,height,slots", COMBOS)
def test_height_every_instantiation(cus, depth, height, slots, period, w):
    """K = 5: a tall tile's 5 H positions are no multiple of the unroll, so tile boundaries fall on
    every step of the unrolled loop. (4096, 1): every slot fills, the fallback wait runs with a full
    FIFO and the slot index wraps; (512, 512): every poll flushes."""
    _case(5, _first_shape(cus, height), depth, height, slots, period, w)


@pytest.mark.parametrize("depth,height,slots", TALL)
def test_height_no_tall_tile(depth, height, slots):
    """P = T (H - 1) + 1: nothing for the ring, H - 1 whole tiles and one element through the tail path."""
    _case(5, T * (height - 1) + 1, depth, height, slots)


@pytest.mark.parametrize("depth,height,slots", TALL)
def test_height_one_tall_tile(depth, height, slots):
    """P = T H: one workgroup with one tall tile, no tail."""
    _case(5, T * height, depth, height, slots)


@pytest.mark.parametrize("d", ["0", "TH", "T", "-1"])
@pytest.mark.parametrize("depth,height,slots", [(2, 2, 2), (2, 4, 1), (3, 2, 1)])
def test_height_tile_counts_around_the_grid(cus, depth, height, slots, d):
    """P = T H C + d: exactly one tall tile each; one workgroup with two; a leftover whole tile; the
    last workgroup's tall tile gone, H - 1 whole tiles and a ragged one of T - 1 in its place."""
    dp = {"0": 0, "TH": T * height, "T": T, "-1": -1}[d]
    _case(4, T * height * cus + dp, depth, height, slots)


@pytest.mark.parametrize("slots", [1, 2])
@pytest.mark.parametrize("K", [2, 3])
def test_height_ring_spans_client_and_tile_boundary(cus, K, slots):
    """DEPTH 3, HEIGHT 2 (unrolled 6 times) over K = 2 and 3: the two positions in flight behind a
    consume lie across a client boundary, and at a tall tile's end across a tile boundary too."""
    _case(K, T * 2 * (3 * cus + 1) + T + 1, 3, 2, slots)


@pytest.mark.parametrize("depth,height,slots", [(2, 2, 2), (2, 4, 1)])
def test_height_64_clients(depth, height, slots):
    _case(64, T * height * 300 + 5, depth, height, slots, grid=2)


@pytest.mark.parametrize("pol", [0, 1, 2, 3])
def test_height_every_load_policy(cus, pol):
    """The default policy, nt, sc1 and sc1 nt on the ring's loads: the same bits."""
    _case(5, _first_shape(cus, 2), 2, 2, 2, pol=pol)


def test_height_k70_continuation():
    """70 clients: the first 64 in the parked launch (ring 2, height 4), the other 6 continue from the
    stored aggregate in k_fedavg_pipe."""
    P, K = T * 4 * 75 + T * 3 + 77, 70
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
                    avg_park_depth=2, avg_park_slots=1, avg_park_height=4):
            ops.fedavg_fold(agg, dev[:64], ns[:64], Ns[:64], init=True)
            assert ops.last_kernel() == WIN
            ops.fedavg_fold(agg, dev[64:], ns[64:], Ns[64:], init=False)
            assert ops.last_kernel() == ("k_fedavg_pipe" if mode == 3 else WIN)
        torch.cuda.synchronize()
        got[mode] = agg.cpu().numpy()
    assert_lists_identical([got[3]], [want], "K=70 height 4 vs oracle")
    assert_lists_identical([got[3]], [got[0]], "K=70 height 4 vs mode 0")
