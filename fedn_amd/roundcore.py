"""The round protocol both pipeline families share: one device (staging.py) or a list of them
(multidev.py).

A round admits updates in FIFO order; one whose layout differs moves the round to the per-tensor
path (mixed.py); device-resident ones queue (``pending``) and fold in batches. A batch's fold is
all-or-nothing: the running state (FedAvg's aggregate, FedOpt's pseudo-gradient) is copied aside
before a fold of several launches continues it and put back when one of them fails, and the
FedAggError propagates. The caller of a failed batch then folds its updates one at a time as FEDn
does (fedavg.py:47-78, fedopt.py:74-106), skipping and reporting the ones whose own fold fails.
Whatever else escapes a flush marks the round lost (``broken``): no model is returned without
the batch.

Nothing here knows where an update's bytes lie. The staging layers (staging._Pipeline,
multidev._ShardedStaging) supply the geometry: ``_parts`` (the running state per device and
stream), ``_nlaunch`` (launches of one fold), ``_sync_all``, ``_before_flush``; the FedAvg and
FedOpt classes on top supply ``_launches`` (a generator that enqueues one launch per step).
"""
import torch

from . import mixed, ops
from .ingest import ShardedStagedModel, StagedModel
from .layout import old_members


NO_SNAPSHOT = object()   # copy_aside could not hold the running state (HBM full)


def copy_aside(parts):
    """Device copies of ``parts`` ([(device, stream, {group: tensor})]), each made on its stream;
    NO_SNAPSHOT when HBM cannot hold them (the fold goes ahead: only a failure part-way is fatal)."""
    out = []
    try:                                        # model-sized clones for the fold's duration (the HBM
        for dv, stream, ts in parts:            # budget's headroom)
            with torch.cuda.device(dv), torch.cuda.stream(stream):
                out.append({dt: t.clone() for dt, t in ts.items()})
    except torch.cuda.OutOfMemoryError:
        return NO_SNAPSHOT
    return out


def put_back(round_, parts, snap, ran=1):
    """Undo a failed fold of which ``ran`` launches had been enqueued: ``snap`` (copy_aside's) back
    into ``parts``. Nothing to do when no launch ran or none was needed (``snap`` None). From
    NO_SNAPSHOT the state cannot be had back: the round ``round_`` is lost."""
    if ran == 0 or snap is None:
        return
    if snap is NO_SNAPSHOT:
        # a launch failed after earlier ones advanced the state, and HBM held no copy of it: the
        # round cannot go on with this update skipped — result() / server_step() raise
        round_.broken = RuntimeError("a multi-launch fold failed part-way and the aggregate could not be "
                                     "copied aside beforehand (HBM full): the round is lost")
        raise round_.broken
    for (dv, stream, ts), saved in zip(parts, snap):
        with torch.cuda.device(dv), torch.cuda.stream(stream):
            for dt, t in saved.items():
                ts[dt].copy_(t)


class Round:
    """Pending batch, failure isolation and the lost-round mark of one aggregation round."""

    def __init__(self):
        self.pending = []                        # device-resident updates not folded yet: (source, n, N, tag)
        # per-update failure isolation (fedavg.py:75-78, fedopt.py:103-106): (tag, exception) of each
        # update whose own fold failed, for the aggregator to log, uncount and keep in storage
        self.skipped = []
        self.broken = None                       # a batch lost beyond recovery: result() raises it
        self.nfolds = 0
        self.general = None                      # mixed.TensorFedAvg / TensorFedOpt once an update differs in layout

    def take_skipped(self):
        """(tag, exception) of the updates skipped since the last call (see ``skipped``)."""
        out, self.skipped = self.skipped, []
        return out

    def unsettled(self):
        """How many of the most recently added updates are admitted but not folded yet (the pending
        batch): their fold may still fail, so the aggregator keeps them in storage until then."""
        return len(self.pending)

    def _check_broken(self):
        if self.broken is not None:
            raise RuntimeError(f"a batched fold failed and could not be recovered: {self.broken}") from self.broken

    def quiesce(self):
        """Nothing of the round still reads the caller's arrays (the staging layers say how)."""

    def release(self):
        """The round's result is on the host (staging._Pipeline gives its resources to the cache)."""

    def _before_flush(self):
        """Bytes admitted on the host reach the device (staging._Pipeline.upload_arena)."""

    # ---- all-or-nothing folds ----------------------------------------------------------------
    def _snapshot(self, launches):
        """The running state copied aside before a continuation fold of ``launches`` launches: one
        that fails part-way leaves it half-advanced, and the recovery needs it back. None when not
        needed: not started (an init fold rewrites it) or one launch (a failed launch ran nothing)."""
        if not self._started() or launches <= 1:
            return None
        return copy_aside(self._state_parts())

    def _restore(self, snap, ran=1):
        put_back(self, self._state_parts(), snap, ran)

    def _all_or_nothing(self, nlaunch, launches):
        """Run ``launches`` (an iterator that enqueues one launch per step, ``nlaunch`` in all). If
        one fails, the state is as before the call and the FedAggError propagates."""
        snap, ran = None, 0
        try:
            snap = self._snapshot(nlaunch)      # inside the try: an update is never skipped for a clone
            for _ in launches:
                ran += 1
        except ops.FedAggError:
            self._restore(snap, ran)
            raise
        self._folded()

    def _fold_batch(self, entries):
        """Fold ``entries`` in one multi-client launch per group (and device), all-or-nothing."""
        self._all_or_nothing(self._nlaunch(), self._launches(entries))

    def _isolate(self, entries):
        """A batched fold over ``entries`` failed: fold them one at a time in FIFO order as FEDn does.
        An update whose own fold fails is skipped and reported with its tag; its examples stay
        counted (its N is already in every later entry's running total), and the state is as the
        previous update left it (each update's launches are all-or-nothing)."""
        for e in entries:
            try:
                self._fold_batch([e])
            except ops.FedAggError as ex:
                self.skipped.append((e[3] if len(e) > 3 else None, ex))

    def _fold_isolated(self, entries):
        try:
            self._fold_batch(entries)
        except ops.FedAggError:
            self._isolate(entries)

    def _recover(self, entries, snap, ran):
        """The round's last launches over ``entries`` failed after ``ran`` of them (and what was
        enqueued has run): the state back first, then the updates one at a time."""
        self._restore(snap, ran)
        self._isolate(entries)

    def _flush(self):
        self._before_flush()
        if self.pending:
            entries, self.pending = self.pending, []
            try:
                self._fold_isolated(entries)
            except BaseException as e:          # the batch is lost: never return a model without it
                self.broken = e
                raise


class FedAvgRound(Round):
    """FedAvg's part of the protocol: the state is the running aggregate ``agg``."""

    def _started(self):
        return self.agg_started

    def _state_parts(self):
        return self._parts(self._agg)

    def _state_meta(self):
        """(shape, dtype) per tensor of the running model: the first update's before any fold,
        numpy's fold result dtype after."""
        lay = self.layout
        if self.nfolds == 0:
            return list(zip(lay.shapes, lay.dtypes))
        return [(s, mixed.np_dtype(ops.fold_result_dtype(ops.torch_dtype(d), ops.torch_dtype(d))))
                for s, d in zip(lay.shapes, lay.dtypes)]

    def _add_general(self, arrays, n, N):
        """The per-tensor path's share of add(): True if the update went that way — the round is on
        it already, or this update differs from the first's layout (numpy promotion / broadcasting,
        mixed.py), checked before any state changes."""
        if self.general is not None:
            self.general.fold(self.tensors_of(arrays), n, N)
        elif (not self.compatible(arrays) or mixed.int_float_n(self.layout.dtypes, self.nfolds, n) or
              mixed.per_tensor_dtypes(self.layout.dtypes)):
            plan = mixed.fold_plan(self._state_meta(), self.meta_of(arrays), n, N)   # raises as numpy
            self._enter_general()
            self.general.fold(self.tensors_of(arrays), n, N, plan=plan)
        else:
            return False
        self.nfolds += 1
        return True

    def _alias(self):
        """The first update itself: the model when nothing was folded into it (fedavg.py:65-66)."""
        first = self.first_arrays
        return first.host if isinstance(first, (StagedModel, ShardedStagedModel)) else first


class FedOptRound(Round):
    """FedOpt's part of the protocol: the state is the pseudo-gradient ``pg``; the round ends in the
    server step."""

    def _init_fedopt(self, old_arrays):
        """The global model against this round's layout (call once the staging layer is set up)."""
        self.old_arrays = old_arrays
        self.pg_started = False                  # pg holds a partial pseudo-gradient
        self.old_ready = set()                   # groups of the global model that are on the device(s)
        # the fused path needs the global model to share the update's shapes with one dtype per
        # update-dtype group, and a (update, old) dtype pair the kernel instantiates; otherwise
        # the round runs on the per-tensor path (numpy promotion / broadcasting, mixed.py)
        self.fused_ok = True
        try:
            self.old_host = old_members(self.layout, old_arrays)
            ops.check_fedopt_dtypes(self.layout)
            for dt, (odt, _) in self.old_host.items():
                if not ops.fused_fedopt_pair(ops.torch_dtype(dt), ops.torch_dtype(odt)):
                    raise TypeError(f"no fused kernel for {dt} updates over a {odt} global model")
        except (ValueError, TypeError):
            self.fused_ok = False
            self.old_host = {}

    def _started(self):
        return self.pg_started

    def _state_parts(self):
        return self._parts(self._pg)

    def _folded(self):
        self.pg_started = True

    def _pg_meta(self):
        """(shape, dtype) per tensor of the pseudo-gradient folded so far (fused layout)."""
        old = {d: ops.torch_dtype(odt) for d, (odt, _) in self.old_host.items()}
        return [(s, mixed.np_dtype(ops.fedopt_dtypes(ops.torch_dtype(d), old[d], None)[0]))
                for s, d in zip(self.layout.shapes, self.layout.dtypes)]

    def _add_general(self, arrays, n, N):
        """The per-tensor path's share of add(): True if the update went that way — the round is on
        it already, or this update differs from the first in dtype or shape, or from the global
        model in shape (checked before any state changes)."""
        if self.general is None and not (self.fused_ok and self.compatible(arrays)):
            splan = mixed.sub_plan(self.meta_of(arrays), mixed.host_meta(self.old_arrays))   # raises as numpy
            if self.nfolds:
                mixed.fold_plan(self._pg_meta(), [(sh, d) for d, sh in splan], n, N)
            self._enter_general()
        if self.general is None:
            return False
        self.general.add(self.tensors_of(arrays), n, N)
        self.nfolds += 1
        return True

    def _zero_copy_step(self, state, params, opt, sig):
        """The whole round in one launch over host memory, where the staging layer has such a form."""
        return None

    def server_step(self, state, params):
        """Apply adam/yogi/adagrad (fedopt.py:139-258); returns the new model (host, f64)."""
        opt = params["serveropt"]
        if opt not in ("adam", "yogi", "adagrad"):
            raise ValueError(f"Unsupported server optimizer: {opt}")
        sig = self._regroup(state) if self.general is None else None
        if sig is None and self.general is None:
            self._enter_general()               # the state's layout differs from this round's
        if self.general is not None:
            m, v = self._state_tensors(state)
            model, m, v = self.general.server_step(m, v, params, fp32=getattr(state, "fp32", False))
            state.set_tensors(m, v)
            return model
        self._check_broken()
        model = self._zero_copy_step(state, params, opt, sig)
        if model is not None:
            return model
        # one fused launch per group (and device): the pending (device-resident) updates, if any,
        # folded into the pseudo-gradient in registers (FIRST when pg holds nothing yet) and the
        # server step; chunked so that each chunk's D2H of the new model overlaps the next chunk
        self._before_flush()
        entries, self.pending = self.pending, []
        if not entries and not self.pg_started:
            # every update's fold was skipped: no pseudo-gradient (fedopt.py:110, 117-118)
            raise ValueError("no update was folded into the pseudo-gradient")
        old_ready = set(self.old_ready)
        try:
            return self._fused_step(state, params, opt, sig, entries)
        except ops.FedAggError:
            if not entries:
                raise                           # the server step itself failed (fedopt.py:111-116)
        # the fused launch failed: the pending updates fold into pg one at a time (a failing one is
        # skipped), then the server step runs alone (K = 0); its failure is the round's (None, data)
        self._sync_all()
        self.old_ready = old_ready              # a global model streamed in part-way is streamed again
        self._fold_isolated(entries)
        return self.server_step(state, params)
