"""The server-function kernels, ``fa_weighted_sum`` (policies ``CWSUM<Y, X>`` for update / accumulator
dtypes (f32, f32), (f32, f64), (f64, f64), (f64, f32)) and ``fa_running_mean`` (``CRUN<T>`` for f32 and
f64), bit for bit (values and dtype, NaN by position) against the reference's own numpy expressions

    weighted sum    acc = start.copy(); for u, w in zip(ups, ws): acc += u * w
    running mean    g = (g * (T - n) + m * n) / T

with python-number scalars, evaluated on what the device holds. Each of the six instantiations can run
three kernels, and every launch here is followed by a check of ``ops.last_kernel()``:

1. the scalar ``k_fedavg`` (one element per lane) when a pointer is not 16-B aligned: every ``off = 1``
   case below, views ``[1 : 1 + P]`` of rows whose length is a multiple of 64 elements;
2. the one-strip ``k_fedavg`` while a client buffer is below ``kPipeMinClientBytes``: the ``off = 0``
   cases, at P = 1 and 5 (less than one strip, only the ragged tail), 4 099 and 65 579 (several
   workgroups, a ragged last strip), K = 1, 2, 64, 65 and 129 (the client table's boundary, the second
   and the third continuation launch);
3. ``k_fedavg_pipe`` (continuation form: the accumulator is read; plain stores; 8-B or 32-B aggregate
   strips under 16-B client strips when the dtypes differ) at and above that size. It is run at the
   smallest P that selects it, plus half a tile, one strip and a ragged strip, so that the last
   workgroup holds whole strips, a ragged one and lanes past the end. Three slices of 70 K elements go
   to numpy; every element is compared with kernel (2) run over the two halves of the same buffers.
   The size is what the threshold asks for (160 MiB per client buffer, under 1.5 GB in all): nothing
   smaller reaches this kernel in the product library.

Special values (+-0, +-inf, NaNs of both signs with payloads, subnormals, the largest finite values,
products that are subnormal or overflow, a sum that overflows before -inf arrives) are columns of
scenarios in the manner of test_gpu_robust._special_columns, run by themselves at K = 5 and 65 and
planted into the sampled slices of (3). All NaNs of one column carry one bit pattern (see
_special_columns): NaN + NaN may keep either operand's payload, the separately compiled kernels choose
differently, and (3)'s every-element comparison is on integers. ``WeightedAverage`` /
``IncrementalAverage`` are run on a model above ``staging.SMALL_UPDATE_BYTES``, where every client is
staged into one of two reused slots.
"""
import numpy as np
import pytest
import torch

from golden_io import assert_lists_identical
from oracle import numpy_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PIPE_MIN_BYTES = 160 << 20       # kPipeMinClientBytes in fedn_amd/csrc/fedavg_launch.h (not exported)
PAIRS = [("f32", "f32"), ("f32", "f64"), ("f64", "f64"), ("f64", "f32")]     # (update, accumulator)
NP_DT = {"f32": np.float32, "f64": np.float64}
TORCH_DT = {"f32": torch.float32, "f64": torch.float64}
INT_DT = {"f32": torch.int32, "f64": torch.int64}
UINT = {4: np.uint32, 8: np.uint64}
NAN_BITS = {"f32": (0x7FC10000, 0xFFC50000), "f64": (0x7FF8200000000000, 0xFFF8A00000000000)}
ROW = 65600                      # a multiple of 64 elements: every row of a matrix is 16-B aligned
PS = [1, 5, 4099, 65579]
KS = [1, 2, 64, 65, 129]
W_SPECIAL = [0, -3, 0.1, 16_777_217, 5000]     # 0 * inf; a sign flip; not an f32 value (twice); plain
# (T, n) of the running-mean steps: plain; T is not an f32 value; neither T nor T - n is one
# (20 000 001 - 5 = 19 999 996 is even and below 2^25, so f32 holds it: the third step is there for
# a scalar `a` that the weak-scalar cast to f32 changes)
STEPS = [(123_457, 4_999), (20_000_001, 5), (20_000_001, 4)]
SENTINEL = 7.0


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from fedn_amd import _abi
    _abi.load()
    yield
    _MATRIX.clear()              # section 2's device matrices: not kept for the files that run next
    torch.cuda.empty_cache()


# ---- the oracle ----------------------------------------------------------------------------------
def _wsum_ref(start, ups, ws):
    acc = start.copy()
    with np.errstate(all="ignore"):
        for u, w in zip(ups, ws):
            acc += u * w
    return acc


def _rmean_ref(g, m, T, n):
    with np.errstate(all="ignore"):
        g = (g * (T - n) + m * n) / T
    return g


def _weights(K):
    """Python ints in 1..5000 with one python float among them."""
    ws = [int(v) for v in np.random.default_rng(1000 + K).integers(1, 5001, K)]
    if K >= 2:
        ws[min(3, K - 1)] = 2.75
    assert all(type(w) in (int, float) for w in ws)
    return ws


def _special_weights(K):
    return [W_SPECIAL[k % len(W_SPECIAL)] for k in range(K)]


def _same(got, want, what):
    assert_lists_identical([got], [want], what)


# ---- special values --------------------------------------------------------------------------------
def _special_columns(name, K, ws, copies=1, seed=5):
    """(K + 1) x C of dtype ``name``: every column a scenario, row 0 the start accumulator (or the
    running model), rows 1..K the updates, their order permuted per column (``copies`` times, each
    with permutations of its own). The structure and the permutations do not depend on the dtype, so
    the matrices of two dtypes line up column by column."""
    rng = np.random.default_rng(seed)
    dt = np.dtype(NP_DT[name])
    fi = np.finfo(dt)
    big, mn, tiny = float(fi.max), float(fi.tiny), float(fi.smallest_subnormal)
    fin = lambda n: [float(v) for v in np.round(rng.standard_normal(n), 1)]      # noqa: E731
    vals = [1.5, 0.0, -0.0, np.inf, -np.inf, np.nan, tiny, -tiny, 3 * tiny, big, -big,
            mn, -2.5 * mn, mn / 4096,           # x 0.1, x 0.1, x 1000: a subnormal product
            big / 2, big / 4000, -big / 1e7]    # x -3, x 5000, x 16 777 217: the product overflows
    cols = []
    for s in vals:                              # every (start, update) pair, all clients alike
        for v in vals:
            cols.append([s] + [v] * K)
    for m in sorted({0, 1, 2, K // 2, K - 1, K} & set(range(K + 1))):
        s = lambda: vals[len(cols) % len(vals)]                                     # noqa: E731
        cols.append([s()] + [np.inf] * m + fin(K - m))
        cols.append([s()] + [-np.inf] * m + fin(K - m))
        cols.append([s()] + [np.nan] * m + fin(K - m))
        cols.append([s()] + [big] * m + [-big] * (K - m))                           # sums that overflow
        cols.append([s()] + [tiny * (k + 1) * (-1) ** k for k in range(m)] + [0.0] * (K - m))
        cols.append([s()] + [-0.0] * m + [0.0] * (K - m))
        if 2 * m <= K:
            cols.append([s()] + [-np.inf] * m + [np.inf] * m + fin(K - 2 * m))
    S0 = np.array(cols, dtype=np.float64).T
    parts = []
    for _ in range(copies):
        S = S0.copy()
        for c in range(S.shape[1]):
            S[1:, c] = S[1 + rng.permutation(K), c]
        parts.append(S)
    # in client order: the sum overflows to inf at the first client with a nonzero weight, then -inf
    # arrives (through the next client's weight) and the result is NaN
    a = next((k for k, w in enumerate(ws[:K]) if w != 0), None)
    if a is not None:
        col = [big] + [0.0] * K
        col[1 + a] = 0.75 * big / ws[a]
        if a + 1 < K:
            col[2 + a] = np.inf if ws[a + 1] < 0 else -np.inf
        parts.append(np.array([col], dtype=np.float64).T)
    with np.errstate(all="ignore"):
        S = np.ascontiguousarray(np.concatenate(parts, axis=1).astype(dt))
    # NaNs with payloads, negative in every other column. Which operand's payload NaN + NaN keeps is
    # fixed neither by IEEE 754 nor by numpy, and the pipelined and the small kernel, compiled apart,
    # choose differently (seen on running_mean: g's in one, m's in the other). So that the two can
    # still be compared as integers, all NaNs of one column carry one pattern, and NAN_BITS' f32 and
    # f64 patterns are each other's image under conversion.
    u = S.view(UINT[dt.itemsize])
    for r, c in np.argwhere(np.isnan(S)):
        u[r, c] = NAN_BITS[name][c % 2]
    return S


def _padded(S):
    """Columns repeated up to a multiple of 64 with at least one spare (for the off = 1 views)."""
    total = -(-(S.shape[1] + 1) // 64) * 64
    return np.ascontiguousarray(S[:, np.arange(total) % S.shape[1]])


# ---- 1. the pipelined kernel at the smallest size that selects it ---------------------------------
def _pipe_P(name):
    isz = np.dtype(NP_DT[name]).itemsize
    E = 16 // isz
    tile = 1024 * E
    P = PIPE_MIN_BYTES // isz + tile // 2 + E + (E - 1)
    assert P * isz >= PIPE_MIN_BYTES and (P - P // 2) * isz < PIPE_MIN_BYTES
    return P


def _slices(P):
    mid = (P // 2) | 1
    return [(0, 70_000), (mid, mid + 70_001), (P - 70_003, P)]     # the last: a full tile and the ragged one


def _plant(bufs, rows, P):
    """Write the special columns into every sampled slice of the device buffers (``rows[i]`` into
    ``bufs[i]``), and once more so that they end at P: the ragged strip holds specials too."""
    C = rows[0].size
    assert 2 * C + 11 <= 70_000
    for t, row in zip(bufs, rows):
        r = torch.from_numpy(np.ascontiguousarray(row)).to(DEV)
        assert r.dtype == t.dtype
        for lo in [lo + 11 for lo, _ in _slices(P)] + [P - C]:
            t[lo:lo + C].copy_(r)


def _bit_equal(a, b, name, what):
    """Every element of two device tensors, compared as integers."""
    ai, bi = a.view(INT_DT[name]), b.view(INT_DT[name])
    if torch.equal(ai, bi):
        return
    idx = torch.nonzero(ai != bi).flatten()
    head = idx[:6]
    mask = (1 << (8 * a.element_size())) - 1
    only_nan = bool((torch.isnan(a[idx]) & torch.isnan(b[idx])).all())
    raise AssertionError(f"{what}: {idx.numel()} of {a.numel()} elements differ bitwise, first at {head.tolist()}: "
                         f"{[hex(v & mask) for v in ai[head].tolist()]} vs {[hex(v & mask) for v in bi[head].tolist()]}; "
                         f"NaN on both sides at every one of them: {only_nan}")


@pytest.mark.parametrize("upd,acc", PAIRS)
def test_pipelined_weighted_sum(upd, acc):
    """k_fedavg_pipe<.., CWSUM<upd, acc>, S=4, INIT=false>: K = 2, 3 (even and odd ping-pong exit) and
    66 (a 64-client launch and a continuation launch), three slices against numpy and every element
    against the small kernel run over the two halves."""
    from fedn_amd import ops
    P = _pipe_P(upd)
    gen = torch.Generator(device=DEV).manual_seed(11 + PAIRS.index((upd, acc)))
    ups = [torch.randn(P, generator=gen, device=DEV, dtype=TORCH_DT[upd]) for _ in range(3)]
    ups[1].mul_(1e-3)
    ups[2].mul_(37.0)
    start = torch.randn(P, generator=gen, device=DEV, dtype=TORCH_DT[acc])
    Su, Sa = _special_columns(upd, 3, _weights(3)), _special_columns(acc, 3, _weights(3))
    _plant([start] + ups, [Sa[0]] + list(Su[1:]), P)
    sl = _slices(P)
    ups_np = [[u[lo:hi].cpu().numpy() for u in ups] for lo, hi in sl]
    start_np = [start[lo:hi].cpu().numpy() for lo, hi in sl]
    piped, halves = torch.empty_like(start), torch.empty_like(start)
    h = (P // 2) // 64 * 64
    for K in (2, 3, 66):
        ws = _weights(K)
        clients = [ups[k % 3] for k in range(K)]
        piped.copy_(start)
        ops.weighted_sum(piped, clients, ws)
        assert ops.last_kernel() == "k_fedavg_pipe", f"K={K}"
        for (lo, hi), un, sn in zip(sl, ups_np, start_np):
            _same(piped[lo:hi].cpu().numpy(), _wsum_ref(sn, [un[k % 3] for k in range(K)], ws),
                  f"{upd}->{acc} K={K} slice {lo}")
        halves.copy_(start)
        for a, b in ((0, h), (h, P)):
            ops.weighted_sum(halves[a:b], [u[a:b] for u in clients], ws)
            assert ops.last_kernel() == "k_fedavg", f"K={K} half {a}"
        _bit_equal(piped, halves, acc, f"{upd}->{acc} K={K}: pipelined vs small")
    del ups, start, piped, halves, clients
    torch.cuda.empty_cache()


@pytest.mark.parametrize("name", ["f32", "f64"])
def test_pipelined_running_mean(name):
    """k_fedavg_pipe<.., CRUN<T>, S=4, INIT=false> with K = 1: the steps of STEPS in place on one g."""
    from fedn_amd import ops
    P = _pipe_P(name)
    gen = torch.Generator(device=DEV).manual_seed(23 + len(name))
    g0 = torch.randn(P, generator=gen, device=DEV, dtype=TORCH_DT[name])
    ms = [torch.randn(P, generator=gen, device=DEV, dtype=TORCH_DT[name]) for _ in STEPS]
    S = _special_columns(name, len(STEPS), [n for _, n in STEPS])
    _plant([g0] + ms, list(S), P)
    sl = _slices(P)
    want = [g0[lo:hi].cpu().numpy() for lo, hi in sl]
    piped, halves = g0.clone(), g0.clone()
    del g0
    h = (P // 2) // 64 * 64
    for i, ((T, n), m) in enumerate(zip(STEPS, ms)):
        ops.running_mean(piped, m, T - n, n, T)
        assert ops.last_kernel() == "k_fedavg_pipe", f"step {i + 1}"
        for j, (lo, hi) in enumerate(sl):
            want[j] = _rmean_ref(want[j], m[lo:hi].cpu().numpy(), T, n)
            _same(piped[lo:hi].cpu().numpy(), want[j], f"{name} step {i + 1} slice {lo}")
        for a, b in ((0, h), (h, P)):
            ops.running_mean(halves[a:b], m[a:b], T - n, n, T)
            assert ops.last_kernel() == "k_fedavg", f"step {i + 1} half {a}"
        _bit_equal(piped, halves, name, f"{name} step {i + 1}: pipelined vs small")
    del ms, piped, halves, m
    torch.cuda.empty_cache()


# ---- 2. small shapes: scalar path, chunk boundaries, tails ------------------------------------------
_MATRIX = {}


def _matrix(name):
    """max(KS) + 1 rows of ROW random values of mixed magnitudes per dtype, on the host and on the
    device (the last row: the random start accumulator / the running model)."""
    if name not in _MATRIX:
        rng = np.random.default_rng({"f32": 61, "f64": 62}[name])
        shape = (max(KS) + 1, ROW)
        x = (rng.standard_normal(shape) * 10.0 ** rng.integers(-12, 12, shape)).astype(NP_DT[name])
        _MATRIX[name] = (x, torch.from_numpy(x).to(DEV))
    return _MATRIX[name]


def _check_outside(out, off, P, what):
    o = out.cpu().numpy()
    assert (o[:off] == SENTINEL).all() and (o[off + P:] == SENTINEL).all(), f"{what}: wrote outside [off, off + P)"


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("upd,acc", PAIRS)
def test_weighted_sum_small_shapes(upd, acc, K):
    from fedn_amd import ops
    U, Ud = _matrix(upd)
    A, Ad = _matrix(acc)
    out = torch.empty(ROW, dtype=TORCH_DT[acc], device=DEV)
    zeros = np.zeros(ROW, NP_DT[acc])
    runs = [(zeros, None, _weights(K)), (A[-1], Ad[-1], _weights(K)), (A[-1], Ad[-1], _special_weights(K))]
    for r, (start, start_dev, ws) in enumerate(runs):
        want = _wsum_ref(start, list(U[:K]), ws)              # elementwise: any view's result is a slice of it
        for off in (0, 1):                                    # 0: 16-B aligned, the vector path; 1: the scalar path
            for P in PS:
                what = f"{upd}->{acc} K={K} run {r} off={off} P={P}"
                out.fill_(SENTINEL)
                o = out[off:off + P]
                if start_dev is None:
                    o.zero_()
                else:
                    o.copy_(start_dev[off:off + P])
                assert (o.data_ptr() % 16 == 0) == (off == 0)
                ops.weighted_sum(o, [Ud[k, off:off + P] for k in range(K)], ws)
                assert ops.last_kernel() == "k_fedavg", what
                _same(o.cpu().numpy(), want[off:off + P], what)
                _check_outside(out, off, P, what)


def test_weighted_sum_mixed_alignment():
    """(f64 update, f32 accumulator): only the accumulator off 16-B alignment, then only the last
    update. Both take the scalar path and give the bits of the all-aligned call."""
    from fedn_amd import ops
    U, Ud = _matrix("f64")
    A, Ad = _matrix("f32")
    K, P = 5, 4099
    ws = _weights(K)
    want = _wsum_ref(A[-1, :P], list(U[:K, :P]), ws)
    out = torch.full((ROW,), SENTINEL, dtype=torch.float32, device=DEV)
    o = out[1:1 + P]
    o.copy_(Ad[-1, :P])
    assert o.data_ptr() % 16 != 0
    ops.weighted_sum(o, [Ud[k, :P] for k in range(K)], ws)
    assert ops.last_kernel() == "k_fedavg"
    _same(o.cpu().numpy(), want, "accumulator offset")
    _check_outside(out, 1, P, "accumulator offset")
    out.fill_(SENTINEL)
    o = out[:P]
    o.copy_(Ad[-1, :P])
    last = torch.zeros(ROW, dtype=torch.float64, device=DEV)[1:1 + P]
    last.copy_(Ud[K - 1, :P])
    assert o.data_ptr() % 16 == 0 and last.data_ptr() % 16 != 0
    ops.weighted_sum(o, [Ud[k, :P] for k in range(K - 1)] + [last], ws)
    assert ops.last_kernel() == "k_fedavg"
    _same(o.cpu().numpy(), want, "last update offset")
    _check_outside(out, 0, P, "last update offset")


@pytest.mark.parametrize("name", ["f32", "f64"])
def test_running_mean_small_shapes(name):
    from fedn_amd import ops
    X, Xd = _matrix(name)
    wants = [X[-1]]
    for i, (T, n) in enumerate(STEPS):
        wants.append(_rmean_ref(wants[-1], X[i], T, n))
    out = torch.empty(ROW, dtype=TORCH_DT[name], device=DEV)
    for off in (0, 1):
        for P in PS:
            out.fill_(SENTINEL)
            o = out[off:off + P]
            o.copy_(Xd[-1, off:off + P])
            for i, (T, n) in enumerate(STEPS):
                what = f"{name} off={off} P={P} step {i + 1}"
                ops.running_mean(o, Xd[i, off:off + P], T - n, n, T)
                assert ops.last_kernel() == "k_fedavg", what
                _same(o.cpu().numpy(), wants[i + 1][off:off + P], what)
            _check_outside(out, off, P, f"{name} off={off} P={P}")


def test_refusals_leave_the_accumulator_alone():
    from fedn_amd import ops
    _, Ud = _matrix("f32")
    P = 4099
    u = [Ud[0, :P], Ud[1, :P]]

    def untouched(t, bits):
        assert torch.equal(t.view(torch.int16 if t.dtype == torch.float16 else torch.int32), bits)

    acc = Ud[-1, :P].clone()
    bits = acc.view(torch.int32).clone()
    acc16 = acc.to(torch.float16)
    bits16 = acc16.view(torch.int16).clone()
    with pytest.raises(ops.FedAggError):
        ops.weighted_sum(acc16, u, [2, 3])                                    # an f16 accumulator
    untouched(acc16, bits16)
    with pytest.raises(ops.FedAggError):
        ops.weighted_sum(acc, [t.to(torch.float16) for t in u], [2, 3])       # f16 updates
    untouched(acc, bits)
    with pytest.raises(ValueError):
        ops.weighted_sum(acc, u, [2, 3, 4])                                   # one weight too many
    with pytest.raises(ValueError):
        ops.weighted_sum(acc, u, [2])
    untouched(acc, bits)
    ops.weighted_sum(acc, [], [])                                             # K = 0: nothing to do
    untouched(acc, bits)
    ops.weighted_sum(acc[7:7], [u[0][7:7], u[1][7:7]], [2, 3])                # P = 0
    untouched(acc, bits)
    with pytest.raises(TypeError):
        ops.running_mean(acc, u[0].double(), 3, 2, 5)                         # dtypes differ
    untouched(acc, bits)
    with pytest.raises(ops.FedAggError):
        ops.running_mean(acc16, u[0].to(torch.float16), 3, 2, 5)              # no f16 rule
    untouched(acc16, bits16)
    ops.running_mean(acc[7:7], u[0][7:7], 3, 2, 5)                            # P = 0
    untouched(acc, bits)


# ---- 3. special values -------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [5, 65])
@pytest.mark.parametrize("upd,acc", PAIRS)
def test_weighted_sum_specials(upd, acc, K):
    from fedn_amd import ops
    for ws in (_special_weights(K), _weights(K)):
        Su = _padded(_special_columns(upd, K, ws, copies=3, seed=77 + K))
        Sa = _padded(_special_columns(acc, K, ws, copies=3, seed=77 + K))
        assert Su.shape == Sa.shape
        n = Su.shape[1] - 1
        want = _wsum_ref(Sa[0], list(Su[1:]), ws)
        assert np.isnan(want).any() and np.isinf(want).any() and np.isfinite(want).any()
        Ud, start = torch.from_numpy(Su).to(DEV), torch.from_numpy(Sa[0]).to(DEV)
        out = torch.empty(n + 1, dtype=TORCH_DT[acc], device=DEV)
        for off in (0, 1):
            what = f"{upd}->{acc} K={K} w0={ws[0]} off={off}"
            out.fill_(SENTINEL)
            o = out[off:off + n]
            o.copy_(start[off:off + n])
            ops.weighted_sum(o, [Ud[1 + k, off:off + n] for k in range(K)], ws)
            assert ops.last_kernel() == "k_fedavg", what
            _same(o.cpu().numpy(), want[off:off + n], what)
            _check_outside(out, off, n, what)


@pytest.mark.parametrize("name", ["f32", "f64"])
def test_running_mean_specials(name):
    """Every (g, m) pair of the special values; T not an f32 value, T - n not one, and a float n."""
    from fedn_amd import ops
    S = _padded(_special_columns(name, 1, [5], copies=2))
    n_el = S.shape[1] - 1
    Sd = torch.from_numpy(S).to(DEV)
    out = torch.empty(n_el + 1, dtype=TORCH_DT[name], device=DEV)
    for T, n in [(20_000_001, 5), (20_000_001, 4), (7.5, 2.5)]:
        want = _rmean_ref(S[0], S[1], T, n)
        assert want.dtype == S.dtype
        for off in (0, 1):
            what = f"{name} T={T} n={n} off={off}"
            out.fill_(SENTINEL)
            o = out[off:off + n_el]
            o.copy_(Sd[0, off:off + n_el])
            ops.running_mean(o, Sd[1, off:off + n_el], T - n, n, T)
            assert ops.last_kernel() == "k_fedavg", what
            _same(o.cpu().numpy(), want[off:off + n_el], what)
            _check_outside(out, off, n_el, what)


# ---- 4. WeightedAverage / IncrementalAverage above the arena size ------------------------------------
BIG_MODEL = [(1100, 1000), (257,), (), (0,)]


def _big_clients(rng, K, hostile):
    base = [rng.standard_normal(s) for s in BIG_MODEL]
    ups = [[np.asarray(b + 0.01 * rng.standard_normal(s), dtype=np.float32).reshape(s) for b, s in zip(base, BIG_MODEL)]
           for _ in range(K)]
    for a in ups[hostile]:                       # a hostile client: huge values, an inf and a NaN
        if a.size:
            a.reshape(-1)[:] = 1e30
            a.reshape(-1)[0] = np.inf
            a.reshape(-1)[-1] = np.nan
    return ups


def _slot_path(model):
    from fedn_amd import staging
    from fedn_amd.layout import Layout
    assert Layout.of(model).nbytes > staging.SMALL_UPDATE_BYTES, "the per-client slot path must be the one that runs"


@pytest.mark.parametrize("prev_dt", [np.float32, np.float64])
def test_weighted_average_large_model(prev_dt):
    """Five clients through two staging slots (each reused, ordered by slot.consumed), one of them
    hostile, one without num_examples; an f64 previous_global makes the accumulator f64."""
    from fedn_amd.serverfunctions import WeightedAverage
    rng = np.random.default_rng(91)
    ups = _big_clients(rng, 5, hostile=2)
    _slot_path(ups[0])
    prev = [rng.standard_normal(s).astype(prev_dt).reshape(s) for s in BIG_MODEL]
    metas = [{"num_examples": int(v)} for v in rng.integers(1, 5001, 5)]
    metas[3] = {}
    updates = {f"client-{k}": [u, md] for k, (u, md) in enumerate(zip(ups, metas))}
    got = WeightedAverage(device=DEV).aggregate(prev, updates)
    with np.errstate(all="ignore"):
        want = ref.sf_weighted_average(prev, {k: (list(u), md) for k, (u, md) in updates.items()})
    assert all(np.asarray(w).dtype == prev_dt for w in want)
    assert_lists_identical(got, want, f"WeightedAverage previous_global {np.dtype(prev_dt)}")


def test_incremental_average_large_model():
    """Two rounds of four clients on one instance (the running total carries over), compared after each."""
    from fedn_amd.serverfunctions import IncrementalAverage
    rng = np.random.default_rng(93)
    sf, oracle = IncrementalAverage(device=DEV), ref.SfIncrementalAverage()
    for r in range(2):
        ups = _big_clients(rng, 4, hostile=1 + r)
        _slot_path(ups[0])
        prev = [rng.standard_normal(s).astype(np.float32).reshape(s) for s in BIG_MODEL]
        for k, u in enumerate(ups):
            md = {"num_examples": 100 + 37 * k + r} if k != 2 else {}
            sf.incremental_aggregate(f"client-{k}", u, md, prev)
            with np.errstate(all="ignore"):
                oracle.incremental_aggregate(f"client-{k}", list(u), md, prev)
        assert_lists_identical(sf.get_incremental_aggregate_model(), oracle.get_incremental_aggregate_model(),
                               f"IncrementalAverage round {r + 1}")
