"""The store-window kernels (k_fedavg_pipe_win, k_fedopt_cw; fedavg_kernels.h, fedopt_kernels.h) against the
oracle, in full, bit for bit.

The product launches them for large models only (avg_store_window / opt_store_window), where the
oracle can check samples at best. Parts A and B force them through the probe library at a few
thousand elements (fa_tune AUTO_GEOM 0 + AVG_WIN_*; OPT_WIN_* with OPT_WIN_PROD 1), so whole tiles,
the ragged tile, a one-client launch, K > 64, both remainder paths of in_write_window (a power-of-two
period: a mask; any other: a multiply-high) and every update dtype are compared element by element
with oracle/numpy_ref.py. Part C runs the product library at the smallest shapes at which it picks
a window by itself. Every launch is followed by a check of ops.last_kernel(), so no case can pass
on another kernel's bits.
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
MAXK = 64                                   # clients per launch (fedagg.hip kMaxK)
PERIODS = [(512, 128), (600, 150)]          # (period, window) in 10-ns ticks: mask path, multiply-high path
_RESET = dict(auto_geom=1, avg_win_period=0, avg_win_w=0, avg_win_mode=0, opt_win_period=0, opt_win_w=0,
              opt_win_prod=0)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _abi.load()


@contextlib.contextmanager
def _probe(**knobs):
    """The probe library with ``knobs`` set; every window / geometry knob back at its default after."""
    with _abi.use_probe():
        try:
            ops.tune(**knobs)
            yield
        finally:
            ops.tune(**_RESET)


def _same(a, b):
    return torch.equal(a.view(torch.uint8), b.view(torch.uint8))


# ===================================================================== A. FedAvg window, forced small
def _avg_inputs(rng, K, P, dt):
    """K clients of P elements: device tensors in ``dt`` and the float32 arrays the oracle folds
    (bf16 is defined by its exact upcast)."""
    base = rng.standard_normal(P)
    ups = [(base + 0.01 * rng.standard_normal(P)).astype(np.float32) for _ in range(K)]
    ns = [int(v) for v in rng.integers(1, 5001, K)]
    return _avg_to_dev(ups, dt) + (ns,)


def _avg_to_dev(ups, dt):
    if dt == "bf16":
        dev = [torch.from_numpy(u).to(torch.bfloat16).to(DEV) for u in ups]
        return dev, [d.float().cpu().numpy() for d in dev]
    return [torch.from_numpy(u).to(DEV) for u in ups], ups


def _fold_windowed(dev, ns, agg=None, n0=0):
    """Fold ``dev`` in launches of at most 64 clients, as fa_fedavg_fold does, each one checked to
    have run the windowed kernel. ``agg`` given: a stored aggregate of ``n0`` examples to continue
    (no first launch)."""
    Ns = [int(v) + n0 for v in np.cumsum(ns)]
    first = agg is None
    if first:
        agg = torch.empty(dev[0].numel(), dtype=torch.float32, device=DEV)
    for k0 in range(0, len(dev), MAXK):
        sl = slice(k0, k0 + MAXK)
        ops.fedavg_fold(agg, dev[sl], ns[sl], Ns[sl], init=first)
        assert ops.last_kernel() == "k_fedavg_pipe_win", f"launch at client {k0}"
        first = False
    torch.cuda.synchronize()
    return agg.cpu().numpy()


def _avg_case(K, P, dt, period, w, mode=0):
    rng = np.random.default_rng(K * 1_000_003 + P)
    with np.errstate(all="ignore"):
        if K == 1:
            # fa_fedavg_fold copies a lone first client without a kernel, so a one-client launch of
            # the fold kernel is a continuation: the aggregate holds an earlier client already
            dev, ups, ns = _avg_inputs(rng, 2, P, dt)
            want = ref.fedavg_flat(ups, ns)
            with _probe(auto_geom=0, avg_win_period=period, avg_win_w=w, avg_win_mode=mode):
                got = _fold_windowed(dev[1:], ns[1:], agg=dev[0].float(), n0=ns[0])
        else:
            dev, ups, ns = _avg_inputs(rng, K, P, dt)
            want = ref.fedavg_flat(ups, ns)
            with _probe(auto_geom=0, avg_win_period=period, avg_win_w=w, avg_win_mode=mode):
                got = _fold_windowed(dev, ns)
    assert_lists_identical([got], [want], f"{dt} K={K} P={P} period={period} mode={mode}")


# a tile is 4096 elements (bf16 updates: 8192). One-client launch; whole tiles only; a one-element
# ragged tail; three tiles and a tail; odd and even K through the ping-pong; K > 64 (the continuation
# launch reads the stored aggregate, INIT = false: windowed too in forced mode); a tail-only model
AVG_SHAPES = [(1, 4096), (2, 8192), (2, 4097), (3, 8192 * 3 + 7), (64, 4099), (65, 8192 * 2 + 5), (130, 100_003),
              (5, 1)]


@pytest.mark.parametrize("period,w", PERIODS)
@pytest.mark.parametrize("K,P", AVG_SHAPES)
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_fedavg_window_forced_small(dt, K, P, period, w):
    _avg_case(K, P, dt, period, w)


@pytest.mark.parametrize("mode", [1, 2])
def test_fedavg_window_forced_small_read_modes(mode):
    """AVG_WIN_MODE 1 / 2 (reads kept out of the window per tile / per client pair): the same bits."""
    _avg_case(65, 8192 * 2 + 5, "f32", 600, 150, mode)


@pytest.mark.parametrize("period,w", PERIODS)
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_fedavg_window_special_values(dt, period, w):
    """zeros, signed zeros, subnormals, huge values, inf and NaN through the windowed fold."""
    vals = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, 3e38, -3e38, np.inf, -np.inf, np.nan, 1.0, -2.5],
                    dtype=np.float32)
    P = 4096 * 2 + 9
    rng = np.random.default_rng(5)
    dev, ups = _avg_to_dev([rng.permutation(np.resize(vals, P)) for _ in range(7)], dt)
    ns = [3, 1, 4000, 1, 5, 9, 2]
    with np.errstate(all="ignore"):
        want = ref.fedavg_flat(ups, ns)
    with _probe(auto_geom=0, avg_win_period=period, avg_win_w=w, avg_win_mode=0):
        got = _fold_windowed(dev, ns)
    assert_lists_identical([got], [want], f"{dt} special")


# ===================================================================== B. FedOpt window, forced small
OPTS = ["adam", "yogi", "adagrad"]
OPT_DTYPES = [("f32", "f32"), ("f64", "f32"), ("f64", "f64"), ("f32", "bf16"), ("f32", "f16")]   # (old, update)
OPT_P = [1, 511, 512, 2048, 2053, 2048 * 3 + 513]     # a wave tile is 512 elements, a workgroup 2048
OPT_K = [1, 5, 64]
OPT_PERIODS = [512, 600]
_NP = {"f32": np.float32, "f64": np.float64, "f16": np.float16}
_PARAMS = {"learning_rate": 1e-2, "beta1": 0.9, "beta2": 0.99, "tau": 1e-3}


def _opt_cases():
    """Every (optimizer, dtype pair, P) with K and the period rotating: every value of every axis
    with every optimizer (and every K and period with every dtype pair and every P)."""
    cases = []
    for io, opt in enumerate(OPTS):
        for idt, (old_dt, upd_dt) in enumerate(OPT_DTYPES):
            for ip, P in enumerate(OPT_P):
                s = idt + ip
                cases.append((opt, old_dt, upd_dt, P, OPT_K[s % 3], OPT_PERIODS[(s + io) % 2]))
    return cases


OPT_CASES = _opt_cases()
for _opt in OPTS:
    for _ax, _vals in ((1, [a for a, _ in OPT_DTYPES]), (2, [b for _, b in OPT_DTYPES]), (3, OPT_P), (4, OPT_K),
                       (5, OPT_PERIODS)):
        assert {c[_ax] for c in OPT_CASES if c[0] == _opt} == set(_vals)


def _opt_updates(rng, old, upd_dt, K):
    """K updates around ``old``: device tensors and the arrays the oracle sees (bf16: the exact upcast)."""
    raw = [old + 0.01 * rng.standard_normal(old.size) for _ in range(K)]
    if upd_dt == "bf16":
        dev = [torch.from_numpy(r.astype(np.float32)).to(torch.bfloat16).to(DEV) for r in raw]
        return dev, [d.float().cpu().numpy() for d in dev]
    arrs = [r.astype(_NP[upd_dt]) for r in raw]
    return [torch.from_numpy(a).to(DEV) for a in arrs], arrs


def _opt_session(opt, old_dt, upd_dt, P, K, period, f32state=False, kernel="k_fedopt_cw"):
    """Three rounds, m / v / the model carried on the device: round 1 reads no state, round 2 the
    first round's m (float32 over a float32 model), round 3 the promoted one. Every round's out, m
    and v against the oracle; every launch checked to be ``kernel`` (None: K > 64, several launches)."""
    rng = np.random.default_rng(P * 131 + K * 7 + len(opt) + period)
    params = {"serveropt": opt, **_PARAMS}
    old = rng.standard_normal(P).astype(_NP[old_dt])
    old_dev = torch.from_numpy(old).to(DEV)
    st = ref.FedOptState()
    combine = ref.fedopt_combine_f32state if f32state else ref.fedopt_combine
    state_dt = torch.float32 if f32state else torch.float64
    m_dev = v_dev = None
    for r in range(3):
        dev, arrs = _opt_updates(rng, old, upd_dt, K)
        ns = [int(v) for v in rng.integers(1, 5001, K)]
        want, _ = combine(st, [([a], n) for a, n in zip(arrs, ns)], [old], params)
        pg_dt, m_dt = ops.fedopt_dtypes(dev[0].dtype, old_dev.dtype, None if m_dev is None else m_dev.dtype)
        m_out = torch.empty(P, dtype=torch.float32 if f32state else m_dt, device=DEV)
        v_out = torch.empty(P, dtype=state_dt, device=DEV)
        out = torch.empty(P, dtype=state_dt, device=DEV)
        pg = torch.empty(P, dtype=pg_dt, device=DEV) if K > MAXK else None
        with _probe(opt_win_period=period, opt_win_w=period // 4, opt_win_prod=1):
            ops.fedopt_step(old_dev, dev, ns, [int(v) for v in np.cumsum(ns)], first=True, final=True, pg=pg,
                            m_in=m_dev, m_out=m_out, v_in=v_dev, v_out=v_out, out=out, **params)
            if kernel is not None:
                assert ops.last_kernel() == kernel, f"round {r + 1}"
        torch.cuda.synchronize()
        what = f"{opt} {old_dt}/{upd_dt} P={P} K={K} period={period} round {r + 1}"
        assert_lists_identical([out.cpu().numpy()], want, what + " out")
        assert_lists_identical([m_out.cpu().numpy()], st.m, what + " m")
        assert_lists_identical([v_out.cpu().numpy()], st.v, what + " v")
        m_dev, v_dev, old_dev, old = m_out, v_out, out, want[0]


@pytest.mark.parametrize("opt,old_dt,upd_dt,P,K,period", OPT_CASES)
def test_fedopt_window_forced_small(opt, old_dt, upd_dt, P, K, period):
    _opt_session(opt, old_dt, upd_dt, P, K, period)


@pytest.mark.parametrize("opt", OPTS)
def test_fedopt_window_forced_small_k70(opt):
    """70 clients: forced mode runs k_fedopt_cwp (pg stores in the window) for the first 64 and
    k_fedopt_c for the rest; the oracle alone decides."""
    _opt_session(opt, "f32", "f32", 2048 * 3 + 513, 70, 600, kernel=None)


@pytest.mark.parametrize("period", OPT_PERIODS)
@pytest.mark.parametrize("P", [2053, 2048 * 3 + 513])
@pytest.mark.parametrize("opt", ["adam", "yogi"])
def test_fedopt_window_forced_small_f32state(opt, P, period):
    """The fp32-state mode (out, v and m stored as float32) through k_fedopt_cw, against its definition."""
    _opt_session(opt, "f32", "f32", P, 5, period, f32state=True)


# ===================================================================== C. the product's own choice
# The smallest shapes at which libfedagg.so picks a window by itself (no probe library, no knob):
# avg_store_window needs a pipelined launch (>= 160 MiB per client), a write share <= 15 % and a
# period >= 500 ticks; opt_store_window needs 2^24 elements, a write share <= 25 % (a first round
# over a float32 model writes 20 bytes per element, so from 14 fp32 clients) and, with optimizer
# state read, 32 clients.
def _device_updates(P, K, seed, dtype=torch.float32):
    g = torch.Generator(device=DEV).manual_seed(seed)
    base = torch.randn(P, generator=g, device=DEV)
    ups = [torch.randn(P, generator=g, device=DEV).mul_(0.01).add_(base).to(dtype) for _ in range(K)]
    ns = [int(v) for v in np.random.default_rng(seed).integers(1, 5001, K)]
    return base, ups, ns, [int(v) for v in np.cumsum(ns)]


def _slices(P, tile):
    """200 000 elements at the start, across a tile boundary in the middle, and at the end (ragged tile)."""
    return [slice(lo, lo + 200_000) for lo in (0, tile * (P // (2 * tile)) - 100_000, P - 200_000)]


def test_fedavg_product_window_f32_whole_output():
    P, K = 41_943_040 + 4096 * 3 + 1000, 8        # just over 160 MiB per client, and a ragged tile
    _, ups, ns, Ns = _device_updates(P, K, 31)
    agg = torch.empty(P, device=DEV)
    ops.fedavg_fold(agg, ups, ns, Ns, init=True)
    assert ops.last_kernel() == "k_fedavg_pipe_win"
    torch.cuda.synchronize()
    host = [u.cpu().numpy() for u in ups]
    del ups
    want = ref.fedavg_flat(host, ns)
    assert_lists_identical([agg.cpu().numpy()], [want], "fedavg f32 product window")
    del agg
    torch.cuda.empty_cache()


def test_fedopt_product_window_round1_whole_output():
    P, K = (1 << 24) + 4096 * 3 + 1000, 14        # 14: the fewest fp32 clients with a write share <= 25 %
    old, ups, ns, Ns = _device_updates(P, K, 32)
    params = dict(ref.DEFAULT_FEDOPT)
    out = torch.empty(P, dtype=torch.float64, device=DEV)
    v = torch.empty(P, dtype=torch.float64, device=DEV)
    m = torch.empty(P, dtype=torch.float32, device=DEV)
    ops.fedopt_step(old, ups, ns, Ns, first=True, final=True, m_out=m, v_out=v, out=out, **params)
    assert ops.last_kernel() == "k_fedopt_cw"
    torch.cuda.synchronize()
    host = [([u.cpu().numpy()], n) for u, n in zip(ups, ns)]
    del ups
    st = ref.FedOptState()
    want, _ = ref.fedopt_combine(st, host, [old.cpu().numpy()], params)
    assert_lists_identical([out.cpu().numpy()], want, "out")
    assert_lists_identical([m.cpu().numpy()], st.m, "m")
    assert_lists_identical([v.cpu().numpy()], st.v, "v")
    del old, out, m, v
    torch.cuda.empty_cache()


def test_fedavg_product_window_bf16():
    """bf16 updates at a 14.3 % write share: the product's windowed launch against the unwindowed
    kernel (whole output, on the device) and against the oracle (three slices)."""
    P, K = 83_886_080 + 8192 * 3 + 1000, 12
    _, ups, ns, Ns = _device_updates(P, K, 33, torch.bfloat16)
    agg = torch.empty(P, device=DEV)
    ops.fedavg_fold(agg, ups, ns, Ns, init=True)
    assert ops.last_kernel() == "k_fedavg_pipe_win"
    plain = torch.empty(P, device=DEV)
    with _probe(avg_win_period=-1):
        ops.fedavg_fold(plain, ups, ns, Ns, init=True)
        assert ops.last_kernel() == "k_fedavg_pipe"
    torch.cuda.synchronize()
    assert _same(agg, plain)
    for sl in _slices(P, 8192):
        want = ref.fedavg_flat([u[sl].float().cpu().numpy() for u in ups], ns)
        assert_lists_identical([agg[sl].cpu().numpy()], [want], f"bf16 slice {sl.start}")
    del ups, agg, plain
    torch.cuda.empty_cache()


@pytest.mark.parametrize("state", ["f64", "f32state"])
def test_fedopt_product_window_steady_state(state):
    """A launch that reads m and v (32 clients), in the reference's fp64 state and in the fp32-state
    mode: the product's windowed launch against the unwindowed kernel (whole out, m and v, on the
    device) and against the oracle (three slices)."""
    P, K = (1 << 24) + 4096 * 3 + 1000, 32
    f32state = state == "f32state"
    sdt = torch.float32 if f32state else torch.float64
    old32, ups, ns, Ns = _device_updates(P, K, 34)
    params = dict(ref.DEFAULT_FEDOPT)
    new = lambda: torch.empty(P, dtype=sdt, device=DEV)  # noqa: E731
    # a first round makes the state the steady-state launch reads (its inputs, as far as this test goes)
    old, v_in, m1 = new(), new(), torch.empty(P, dtype=torch.float32, device=DEV)
    ops.fedopt_step(old32, ups, ns, Ns, first=True, final=True, m_out=m1, v_out=v_in, out=old, **params)
    m_in = m1.to(sdt)
    del old32, m1
    out, m, v = new(), new(), new()
    ops.fedopt_step(old, ups, ns, Ns, first=True, final=True, m_in=m_in, m_out=m, v_in=v_in, v_out=v, out=out, **params)
    assert ops.last_kernel() == "k_fedopt_cw"
    plain = (new(), new(), new())
    with _probe(opt_win_period=-1):
        ops.fedopt_step(old, ups, ns, Ns, first=True, final=True, m_in=m_in, m_out=plain[1], v_in=v_in, v_out=plain[2],
                        out=plain[0], **params)
        assert ops.last_kernel() == "k_fedopt_c"
    torch.cuda.synchronize()
    assert all(_same(a, b) for a, b in zip((out, m, v), plain))
    combine = ref.fedopt_combine_f32state if f32state else ref.fedopt_combine
    for sl in _slices(P, 2048):
        st = ref.FedOptState()
        st.m, st.v = [m_in[sl].cpu().numpy()], [v_in[sl].cpu().numpy()]
        want, _ = combine(st, [([u[sl].cpu().numpy()], n) for u, n in zip(ups, ns)], [old[sl].cpu().numpy()], params)
        what = f"{state} slice {sl.start}"
        assert_lists_identical([out[sl].cpu().numpy()], want, what + " out")
        assert_lists_identical([m[sl].cpu().numpy()], st.m, what + " m")
        assert_lists_identical([v[sl].cpu().numpy()], st.v, what + " v")
    del ups, old, m_in, v_in, out, m, v, plain
    torch.cuda.empty_cache()
