"""configs[0]'s rounds: a small model's FedAvg round in as few host steps as the GPU allows.

FEDn's own example (examples/mnist-pytorch: 52,650 fp32 parameters, two clients) folds each round
with ``helper.increment_average`` in ~27 µs of numpy inside a ~47 µs loop (fedavg.py:45-83,
numpyhelper.py:32). Through the general pipeline (staging.FedAvgPipeline) the same round built a
pipeline object, packed the updates, mapped a fresh pinned result block, built ctypes argument
arrays and unpacked the result — ~38 µs of Python above the GPU's own floor.

Here an aggregator keeps, per (device, layout), a ``SmallSession``: one pinned arena the updates are
packed into, the native admission plan, the fold plan, a dedicated stream and a pool of pinned
result blocks. A round then costs, per update, one native admission call (exact layout test + the
pack queued to the gather thread: ``_fastpack.admit``) and, at its end, ONE native call
(``_fastpack.fold_host``: wait for the packs, ``fa_fedavg_fold_host`` — the fold reading the arena
and writing the result block in pinned host memory through their device mappings — and the stream
wait) plus one native call building the model's arrays as views of the result block.

The model a round returns is the caller's (FEDn keeps it as the next global model), and its arrays
view a pooled block. ``ResultBlocks`` alone decides when a block may be written again: each round
leases its block as a fresh ndarray that is the base object of the model's arrays, the pool keeps a
weak reference to that lease, and the block is free once the reference is dead — when nothing can
reach the model's bytes any more, through whatever the caller made of them.

Same observable behaviour as the general path (fedavg.py:47-83): FIFO order, ``total_examples``
before the fold, the first update aliased when it is the only one, and the fold is
``fa_fedavg_fold``'s kernel and client table, so the same bits. An update that is not exactly the
first one's layout (dtype, shape, contiguity), one too many for the arena, or a fold that fails
hands the round to the general pipeline, which replays the admitted updates in order and goes on
(``SmallRound.general``): nothing has been launched or deleted before the round's end.

FedOpt's round (fedopt.py:74-121 + 151-258) is the same one on the same core: ``_Session`` (arena,
admission, result blocks), ``_Round`` (the admitted updates, their replay) and ``_Sessions`` (the
sessions an aggregator keeps) carry what the two share.
"""
import collections
import ctypes
import time
import weakref

import numpy as np
import torch

from . import _abi, ops
from .layout import PACK_THREADS, Layout

# a round's updates, packed, at most staging.ZERO_COPY_BYTES (read at each round: one knob for both
# zero-copy forms, FEDN_AMD_ZERO_COPY_BYTES; 0 turns them off) and 64 of them (one launch) go the
# one-call way


def _zero_copy_bytes():
    from . import staging
    return staging.ZERO_COPY_BYTES
_FOLDABLE = {np.dtype(np.float32): _abi.FA_F32, np.dtype(np.float64): _abi.FA_F64,
             np.dtype(np.float16): _abi.FA_F16}   # dtypes whose fold result is their own dtype (numpy)
_POOL = 4                     # pinned result blocks kept per size (a block a caller still holds is skipped)

# the _fastpack module and the addresses of the native functions it calls
_Native = collections.namedtuple("_Native", "fp fold gather_start gather_wait fedopt_step")
_native = None


def _entry_points():
    """The ``_Native`` entry points, or False if an extension is not built (the general path is then
    taken)."""
    global _native
    if _native is None:
        try:
            from . import _fastpack, codec
            lib, npz = _abi.load(), codec.load_lib()
            if not hasattr(_fastpack, "fold_host"):
                raise ImportError("stale _fastpack")
            addr = lambda f: ctypes.cast(f, ctypes.c_void_p).value  # noqa: E731
            _native = _Native(_fastpack, addr(lib.fa_fedavg_fold_host), addr(npz.fnpz_gather_start),
                              addr(npz.fnpz_gather_wait), addr(lib.fa_fedopt_step_host))
        except (ImportError, AttributeError):
            _native = False
    return _native


def _pinned(nbytes):
    return torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)


class ResultBlocks:
    """Pinned blocks for the models small rounds return, and the one rule for writing a block again.

    ``lease(nbytes)`` hands a block out as a fresh uint8 ndarray. The model's arrays are built with
    that lease as their base object (``_fastpack.views``), so it lives exactly as long as anything —
    an array, a slice, a tensor or buffer made from one — can reach the model's bytes. The pool keeps
    only a weak reference to it: a block is free iff that reference is dead. The lease's own base is
    a memoryview, not an ndarray: numpy points a view of a non-owning ndarray at that array's base
    instead, which would let views outlive a lease cut from a kept ndarray."""

    def __init__(self, alloc=_pinned):
        self._alloc = alloc          # nbytes -> uint8 tensor (pinned; pageable in the CPU test)
        self._pools = {}             # nbytes -> [[tensor, memoryview of it, weakref to its last lease]]

    def lease(self, nbytes):
        """A pooled block of ``nbytes`` nothing holds any more, else a new one: pooled while fewer
        than ``_POOL`` of that size are kept, handed out untracked beyond."""
        pool = self._pools.setdefault(nbytes, [])
        for ent in pool:
            if ent[2]() is None:
                break
        else:
            t = self._alloc(nbytes)
            ent = [t, memoryview(t.numpy()), None]       # leased at once, below
            if len(pool) < _POOL:
                pool.append(ent)
        block = np.frombuffer(ent[1], np.uint8)
        ent[2] = weakref.ref(block)
        return block


def eligible(layout, K_hint=2):
    """Whether a round over ``layout`` can take the one-call path: float16/32/64 tensors only (numpy's
    fold keeps their dtype, so the result block has the arena's layout), and at least two updates
    (the first and one more) fit the arena (a layout is never 0 bytes: groups are 256-B aligned)."""
    zc = _zero_copy_bytes()
    return (all(dt in _FOLDABLE for dt in layout.groups) and max(2, K_hint) * layout.nbytes <= zc
            and bool(_entry_points()))


def fedopt_eligible(layout, old_layout):
    """One float16/32/64 group in both the updates and the global model, with the same shapes, a pair the
    fused kernel instantiates, and at least one update fitting the arena."""
    from .staging import fused_fedopt_pair
    if len(layout.groups) != 1 or len(old_layout.groups) != 1 or layout.shapes != old_layout.shapes:
        return False
    dt, odt = layout.groups[0], old_layout.groups[0]
    return (dt in _FOLDABLE and odt in _FOLDABLE and fused_fedopt_pair(ops.torch_dtype(dt), ops.torch_dtype(odt))
            and layout.nbytes <= _zero_copy_bytes() and bool(_entry_points()))


def _layout_of(arrays):
    try:
        return Layout.of(arrays)
    except Exception:  # noqa: BLE001 — not an array list: the general path raises numpy's error
        return None


# ---- sessions: the per-layout resources an aggregator's small rounds reuse -----------------------

class _Session:
    """What every small session keeps: the pinned arena of ``cap`` update slots of ``stride`` bytes,
    the updates' admission plan and the result blocks."""

    def __init__(self, device, layouts, min_cap, tensors):
        self.nat = _entry_points()
        self.device = torch.device(device)
        self.layouts = layouts                 # the session's key: the updates' layout first
        self.layout = layouts[0]
        self.stride = self.layout.nbytes
        self.cap = max(min_cap, min(64, _zero_copy_bytes() // self.stride))
        self.arena = _pinned(self.cap * self.stride)
        self.arena_ptr = self.arena.data_ptr()
        self.window = (self.arena_ptr, self.cap * self.stride)
        self.plan = self.nat.fp.plan(tensors)
        self.blocks = ResultBlocks()

    def admit(self, plan, arrays, dst, window):
        """Queue the pack of ``arrays`` to ``dst`` inside the pinned ``window`` (address, bytes):
        ticket (> 0), 0 (nothing to copy) or -1 (not exactly ``plan``'s layout: nothing done)."""
        t = self.nat.fp.admit(plan, arrays, dst, self.nat.gather_start, PACK_THREADS, window[0], window[1])
        if t == -2:
            from . import codec
            why = codec.load_lib().fnpz_last_error().decode(errors="replace")
            raise codec.CodecError(f"fnpz_gather_start: {why}")
        return t

    def wait(self, ticket):
        if ticket and ticket > 0:
            from . import codec
            codec.gather_wait(ticket)


class SmallSession(_Session):
    """The per-(device, layout) resources a FedAvg session's small rounds reuse (module docstring)."""

    def __init__(self, device, layout):
        offs = {i: off for i, off, _ in layout.pack_plan}
        super().__init__(device, (layout,), 2, [(tuple(sh), np.dtype(dt), offs.get(i, 0))
                                                for i, (sh, dt) in enumerate(zip(layout.shapes, layout.dtypes))])
        self.fold_plan = self.nat.fp.fold_plan([(_FOLDABLE[dt], _FOLDABLE[dt], layout.group_byte_offset[dt],
                                                 layout.group_elems[dt]) for dt in layout.groups])
        with torch.cuda.device(self.device):
            self.stream = torch.cuda.Stream(self.device)   # the fold touches host memory only: no ordering
        self.stream_ptr = self.stream.cuda_stream          # with torch's streams is needed

    def fold(self, block, K, ns, Ns, ticket):
        """Wait for the packs, fold arena slots 0..K-1 into ``block`` (pinned) and wait: one call."""
        nat, plan, arena, stride, stream = self.nat, self.fold_plan, self.arena_ptr, self.stride, self.stream_ptr
        ops.fedavg_fold_host(lambda n, N: nat.fp.fold_host(plan, nat.fold, nat.gather_wait, ticket or 0, arena,
                                                           stride, K, block.ctypes.data, n, N, stream), ns, Ns)

    def views(self, block):
        return self.nat.fp.views(self.plan, block)


class SmallFedOptSession(_Session):
    """The per-(device, update layout, global-model layout) resources of a FedOpt session's small rounds:
    a pinned block for the global model (packed on the round's first update, fedopt.py:89-90), the
    updates' arena, admission plans for both, pinned result blocks, and two pairs of HBM
    buffers per (m, v) dtype the server step writes in turn — the pair the session's state does not
    hold, so a step that fails leaves the state as the last round left it (fedopt.py:36-38).

    Unlike FedAvg's one-call fold (host memory only), the step reads and writes HBM that torch's
    streams also use — m / v from a general round or a regroup copy, and the pair buffers, which the
    caching allocator hands out in the order of the device's current stream (a block freed there may
    still have queued writes from its previous owner) — so it runs on that current stream, ordered
    after them, never on a private one."""

    def __init__(self, device, layout, old_layout):
        (self.dt,) = layout.groups
        (self.odt,) = old_layout.groups
        super().__init__(device, (layout, old_layout), 1, self._tensors(layout, self.dt))
        self.dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.old_layout = old_layout
        self.P = layout.group_elems[self.dt]
        self.old = _pinned(old_layout.nbytes)
        self.old_ptr = self.old.data_ptr()
        self.old_window = (self.old_ptr, old_layout.nbytes)
        self.old_plan = self.nat.fp.plan(self._tensors(old_layout, self.odt))
        self.out_plans = {}                  # state dtype -> views plan of the new model
        self.pairs = {}                      # (m dtype, state dtype) -> [(m, v) HBM buffers]

    @staticmethod
    def _tensors(layout, dt, out_dt=None):
        """An admission / views plan's entries: each tensor at its element offset in the (single) group."""
        out_dt = np.dtype(out_dt if out_dt is not None else dt)
        offs = dict(layout.members[dt])
        return [(tuple(sh), out_dt, offs[i] * out_dt.itemsize) for i, sh in enumerate(layout.shapes)]

    def views(self, block, sdt):
        plan = self.out_plans.get(sdt)
        if plan is None:
            plan = self.out_plans[sdt] = self.nat.fp.plan(self._tensors(self.layout, self.dt, ops.numpy_dtype(sdt)))
        return self.nat.fp.views(plan, block)

    def state_pair(self, m_dt, sdt, m_in, v_in):
        """HBM buffers for the new m / v: a pair whose memory the state does not hold (compared by
        address: the state may hold a view of a pair buffer rather than the buffer object)."""
        pairs = self.pairs.setdefault((m_dt, sdt), [])
        held = {t.data_ptr() for t in (m_in, v_in) if t is not None and t.numel()}
        for m, v in pairs:
            if m.data_ptr() not in held and v.data_ptr() not in held:
                return m, v
        with torch.cuda.device(self.device):
            pair = (torch.empty(self.P, dtype=m_dt, device=self.device), torch.empty(self.P, dtype=sdt, device=self.device))
        pairs.append(pair)
        return pair


# ---- rounds: the pipeline interface the aggregators use, nothing launched before the round's end --

class _Round:
    """The updates a small round admitted (``held``: (arrays, n, N, tag) in FIFO order, packed into the
    arena slot ``len(ns)`` had when each came) and the ticket of the last pack queued. ``fallback`` is
    the general pipeline a round handed its end to (FedOpt's step does): it reports from then on."""

    fallback = None

    def __init__(self, session, ns, Ns):
        self.s = session
        self.held = []
        self.ns, self.Ns = ns, Ns
        self.ticket = None
        self.time_pack = 0.0
        self.time_kernel = 0.0

    def _admit(self, plan, arrays, dst, window):
        """One timed admission; False (nothing done) if ``arrays`` are not exactly ``plan``'s layout."""
        tic = time.perf_counter()
        t = self.s.admit(plan, arrays, dst, window)
        if t < 0:
            return False
        if t:
            self.ticket = t
        self.time_pack += time.perf_counter() - tic
        return True

    def add(self, arrays, n, N, tag=None):
        """Admit one more update; False (nothing done) if it is not exactly the layout or the arena is
        full — the caller then hands the round to the general pipeline (``general``)."""
        s, k = self.s, len(self.ns)
        if k >= s.cap or type(arrays) is not list:
            return False
        if not self._admit(s.plan, arrays, s.arena_ptr + k * s.stride, s.window):
            return False
        self.held.append((arrays, n, N, tag))
        self.ns.append(n)
        self.Ns.append(N)
        return True

    def quiesce(self):
        """The packs still queued to the gather thread have finished (they read the updates and write
        the arena, which the next round reuses)."""
        if self.ticket is not None:
            self.s.wait(self.ticket)
            self.ticket = None
        if self.fallback is not None:
            self.fallback.quiesce()

    def _replay(self, pipe):
        """The admitted updates added to the general pipeline ``pipe`` in order (same n, N and tags), as
        if they had gone that way from the start."""
        try:
            for arrays, n, N, tag in self.held:
                pipe.add(arrays, n, N, tag=tag)
        except BaseException:
            pipe.quiesce()                      # its packs in flight end before the arrays can go
            raise
        return pipe

    def take_skipped(self):
        return self.fallback.take_skipped() if self.fallback is not None else []

    def unsettled(self):
        return self.fallback.unsettled() if self.fallback is not None else 0

    def timings(self):
        """``data`` keys as the general pipeline reports them: no H2D / D2H copies here; the kernel
        time is the one call's wall time (launch, fold over PCIe, wait)."""
        if self.fallback is not None:
            return self.fallback.timings()
        return {"time_h2d": 0.0, "time_kernel": self.time_kernel, "time_pack": self.time_pack, "time_d2h": 0.0}

    def release(self):
        self.quiesce()
        if self.fallback is not None:
            self.fallback.release()


class SmallRound(_Round):
    """One FedAvg round on a SmallSession: the pipeline interface the aggregator uses (add, result,
    timings, quiesce, release), with nothing launched before ``result``."""

    def __init__(self, session, first):
        super().__init__(session, [0.0], [1.0])     # the first update sits in slot 0
        self.first = first

    @classmethod
    def start(cls, s, first):
        """The round if ``first`` is exactly the session's layout (its pack queued), else None."""
        r = cls(s, first)
        return r if r._admit(s.plan, first, s.arena_ptr, s.window) else None

    def general(self, make_pipeline):
        """The round handed to the general pipeline: ``make_pipeline(first)`` and the admitted updates."""
        self.quiesce()
        return self._replay(make_pipeline(self.first))

    def result(self):
        """The model: the first update itself when nothing was folded into it (fedavg.py:65-66), else
        the fold of every admitted update in one native call, as views of a pinned block. Raises
        FedAggError (nothing changed, the arena intact) if the launch fails: the caller goes general."""
        if not self.held:
            self.quiesce()
            return self.first
        block = self.s.blocks.lease(self.s.stride)
        tic = time.perf_counter()
        ticket, self.ticket = self.ticket, None
        try:
            self.s.fold(block, len(self.ns), self.ns, self.Ns, ticket)
        except BaseException:
            self.s.wait(ticket)
            raise
        self.time_kernel = time.perf_counter() - tic
        return self.s.views(block)


class SmallFedOptRound(_Round):
    """One FedOpt round on a SmallFedOptSession: add() admits each update, server_step() is one native
    call (pack wait + fa_fedopt_step_host, FIRST | FINAL: the pseudo-gradient in registers, then Adam /
    Yogi / AdaGrad). Anything else — another layout, a full arena, a failed launch, a state in another
    form — hands the round to the general pipeline (``make_pipeline(old, first)``), replaying the
    admitted updates in FIFO order: nothing was launched or deleted before."""

    def __init__(self, session, old_arrays, first_arrays, make_pipeline):
        super().__init__(session, [], [])
        self.old_arrays, self.first_arrays = old_arrays, first_arrays
        self.make_pipeline = make_pipeline

    @classmethod
    def start(cls, s, old_arrays, first_arrays, make_pipeline):
        """The round if the global model packs into the session's layout (queued), else None."""
        r = cls(s, old_arrays, first_arrays, make_pipeline)
        return r if r._admit(s.old_plan, old_arrays, s.old_ptr, s.old_window) else None

    def general(self):
        """The round handed to the general pipeline, the admitted updates added in order."""
        self.quiesce()
        return self._replay(self.make_pipeline(self.old_arrays, self.first_arrays))

    def server_step(self, state, params):
        """The new model (fedopt.py:108-118): one native call; a state that is not in this layout's
        fused form, or a failed launch (state untouched), goes the general way."""
        opt = params["serveropt"]
        if opt not in ops._OPTS:
            raise ValueError(f"Unsupported server optimizer: {opt}")
        s = self.s
        sig = s.layout.signature()
        if not state.regroup(s.layout, sig, s.device):
            self.fallback = self.general()
            return self.fallback.server_step(state, params)
        dt = s.dt
        old_t = ops.torch_dtype(s.odt)
        m_in = state.m[dt] if state.m is not None else None
        v_in = state.v[dt] if state.v is not None else None
        from .staging import state_dtypes
        m_dt, sdt = state_dtypes(state, dt, old_t, m_in)
        m_out, v_out = s.state_pair(m_dt, sdt, m_in, v_in)
        block = s.blocks.lease(s.P * ops.numpy_dtype(sdt).itemsize)
        ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
        fa = ops.fa_dtype
        st = (ptr(m_in), _abi.FA_NONE if m_in is None else fa(m_in), ptr(m_out), fa(m_out), ptr(v_in),
              _abi.FA_F64 if v_in is None else fa(v_in), ptr(v_out), fa(sdt))
        ticket, self.ticket = self.ticket, None
        nat, old, arena, stride, K, P = s.nat, s.old_ptr, s.arena_ptr, s.stride, len(self.ns), s.P
        stream = torch._C._cuda_getCurrentRawStream(s.dev_index)      # the current stream: see SmallFedOptSession
        upd_fa, old_fa, out = fa(ops.torch_dtype(dt)), fa(old_t), block.ctypes.data
        args = (ops._OPTS[opt], float(params["learning_rate"]), float(params["beta1"]), float(params["beta2"]),
                float(params["tau"]))
        tic = time.perf_counter()
        try:
            ops.fedopt_step_host(lambda n, N: nat.fp.fedopt_host(nat.fedopt_step, nat.gather_wait, ticket or 0, old,
                                                                 arena, stride, K, upd_fa, old_fa, P, out, n, N,
                                                                 stream, st, *args),
                                 self.ns, self.Ns, first=True, final=True)
        except ops.FedAggError:
            s.wait(ticket)                        # nothing of the state was replaced: the general way
            self.fallback = self.general()
            return self.fallback.server_step(state, params)
        except BaseException:
            s.wait(ticket)
            raise
        self.time_kernel = time.perf_counter() - tic
        state.m, state.v, state.signature, state.layout = {dt: m_out}, {dt: v_out}, sig, s.layout
        return s.views(block, sdt)


# ---- the sessions an aggregator keeps -----------------------------------------------------------

class _Sessions:
    """An aggregator's small sessions by (device, layouts): the last one used is tried first, so a
    session's rounds find theirs with one admission call and no layout lookup."""

    def __init__(self, keep=2):
        self.keep = keep
        self._by_key = {}
        self._last = None

    def _recent(self, device, k_hint):
        """The last session used, if it is on ``device``, its arena is still within the zero-copy
        budget and holds ``k_hint`` updates; else None."""
        s = self._last
        if s is not None and s.device == device and s.cap * s.stride <= _zero_copy_bytes() and k_hint <= s.cap:
            return s
        return None

    def _session(self, device, layouts, make):
        """The session kept for ``device`` and ``layouts``; ``make()``'s new one if there is none, its
        key is a recycled id (Layout.of's cache was cleared) or its arena outgrew the budget (the oldest
        session beyond ``keep`` then goes)."""
        key = (str(device), *map(id, layouts))
        s = self._by_key.get(key)
        if s is None or s.layouts != layouts or s.cap * s.stride > _zero_copy_bytes():
            s = self._by_key[key] = make()
            while len(self._by_key) > self.keep:
                self._by_key.pop(next(iter(self._by_key)))
        self._last = s
        return s


class SmallSessions(_Sessions):
    """A FedAvg aggregator's SmallSession per (device, layout)."""

    def round(self, first, device, k_hint=1):
        """A SmallRound for ``first`` on ``device``, or None (not a list of arrays, not eligible, or
        ``k_hint`` — the round's update count as far as the queue shows it — more than the arena holds:
        those rounds go the general way from the start instead of replaying into it part-way)."""
        if type(first) is not list or not first:
            return None
        last = self._recent(device, k_hint)
        if last is not None:
            r = SmallRound.start(last, first)
            if r is not None:
                return r
        layout = _layout_of(first)
        if layout is None or not eligible(layout, k_hint) or k_hint > 64:
            return None
        return SmallRound.start(self._session(device, (layout,), lambda: SmallSession(device, layout)), first)


class SmallFedOptSessions(_Sessions):
    """A FedOpt aggregator's SmallFedOptSession per (device, update layout, global-model layout)."""

    def round(self, old_arrays, first, device, make_pipeline, k_hint=1):
        """A SmallFedOptRound, or None (see SmallSessions.round; ``k_hint``: the round's update count as
        far as the queue shows it)."""
        if type(first) is not list or not first or type(old_arrays) is not list:
            return None
        last = self._recent(device, k_hint)
        if last is not None and last.layout is _layout_of(first):
            r = SmallFedOptRound.start(last, old_arrays, first, make_pipeline)
            if r is not None:
                return r
        layout, old_layout = _layout_of(first), _layout_of(old_arrays)
        if (layout is None or old_layout is None or not fedopt_eligible(layout, old_layout) or k_hint > 64
                or k_hint * layout.nbytes > _zero_copy_bytes()):
            return None
        s = self._session(device, (layout, old_layout), lambda: SmallFedOptSession(device, layout, old_layout))
        return SmallFedOptRound.start(s, old_arrays, first, make_pipeline)
