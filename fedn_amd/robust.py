"""Device pipeline of the robust aggregation rules: coordinate-wise trimmed mean and median, the
selection rules Krum / Multi-Krum, the geometric median, and centred clipping.

Unlike the FedAvg fold, which sees one client at a time, an order statistic needs all K updates of a
round at once: per element, the K values are sorted, the ``trim`` smallest and largest dropped and the
rest averaged (``fa_trimmed_mean``, kernel ``k_order_mean``). So the pipeline HOLDS the
round's updates — in HBM while ``budget.HbmBudget`` admits them, on the host otherwise — and
``result(trim)`` reduces them:

  * every update in HBM: ONE launch per dtype group reads each update once and writes the model (the
    two iterated rules below launch once per SLICE_BYTES of a group instead, on the updates in place:
    their distance sums, which steer the next pass, then have the same bits wherever the updates sit);
  * some updates on the host: the groups are reduced slice by slice. A slice of each host-side update
    is copied into a reused device ring (one row per such update, two buffers) on the copy stream
    while the compute stream reduces the previous slice; updates in HBM are addressed in place at
    ``base + lo``; each slice's result is copied out before its buffer is reused. HBM use is bounded
    by the budget plus the ring: never an OOM, never a dropped client.

Krum / Multi-Krum (Blanchard et al., 2017) select WHOLE updates instead of filtering
each coordinate: ``select_mean(f, m)`` makes one pass over the held updates for the K x K matrix of
squared distances (``fa_pairwise_sqdist``, kernel ``k_pair_sqdist``; dtype groups and slices are summed
into one matrix on the device), selects on the host (:func:`krum_select`) and takes the plain mean of
the selected updates with the reduction above at ``trim = 0``.

The geometric median (RFA: Pillutla, Kakade and Harchaoui) is the point with the
smallest sum of distances to the updates: ``geometric_median(iterations, nu)`` runs smoothed Weiszfeld
steps, each ONE pass over the held updates that forms the weighted mean and the K distances to it
(``fa_weighted_mean_sqdist``, kernel ``k_wmean_dist``); the weights of the next step come from the
distances on the host (:func:`weiszfeld_weights`).

Centred clipping (Karimireddy, He and Jaggi) is the one rule anchored at the previous
global model ``v``: ``centered_clip(center_arrays, iterations, tau)`` moves ``v`` by the mean of the
updates' differences to it, each clipped to the norm ``tau``, ``iterations`` times. A step is ONE pass
over the held updates that forms the new point in place and the K distances to it
(``fa_centered_clip_step``, kernel ``k_cclip_dist``); the clipping coefficients of the next step come from
the distances on the host (:func:`clip_coefficients`).

Bulyan (El Mhamdi, Guerraoui and Rouault) joins the two kinds: ``bulyan(f)`` selects
``theta = K - 2f`` updates by Krum iterated on the shrinking set (:func:`bulyan_select`, on the same K x K
matrix) and averages, per coordinate, the ``theta - 2f`` of their values closest to their median
(``fa_median_window_mean``, kernel ``k_median_window``).

Central DP-FedAvg (McMahan, Ramage, Talwar and Zhang) is no robust rule but shares the
frame: ``dp_clipped_mean(center_arrays, clip, noise_multiplier, seed, round_id)`` is one step of centred
clipping around the global model followed by Gaussian noise added to the result on the device
(``fa_gaussian_noise``, kernel ``k_gaussian_noise``), a pure function of ``(seed, round, dtype group,
element)``.

All rules are UNWEIGHTED: ``num_examples`` plays no part. One device only. A round takes at most
``ops.MAX_ORDER_K`` (64) updates — one launch's table, one sorting network, one K x K matrix — except the
two clipping rules, ``centered_clip`` and ``dp_clipped_mean``, which take ``ops.MAX_CLIP_K`` (1024): past 64
their step is a chain of ``fa_clip_fold`` launches over chunks of 64 clients that carries the accumulator in
the compute type (kernel ``k_clip_fold``), the same definition bit for bit.

Stream ordering (the rules DESIGN.md records for fresh HBM, §3.7): a buffer is allocated on the
stream that first writes it (staged updates and the ring on the copy stream, results on the compute
stream); the compute
stream waits for an update's ``ready`` event before the launch that reads it; the copy stream waits
for the launch that last read a ring buffer before it refills it; everything the launches read is
held until the result is on the host.
"""
import math
import time

import numpy as np
import torch

from . import ingest, ops, reuse
from .budget import HbmBudget
from .ingest import ShardedStagedModel, StagedModel
from .layout import Layout

# bytes of one update's slice in the ring (host-side updates only): the ring holds
# 2 x (host-side updates) x SLICE_BYTES
SLICE_BYTES = 32 << 20
SLICE_ALIGN = 64              # slice bounds in elements: every slice base stays 16-B aligned


class UnsupportedRound(TypeError):
    """A round the robust rules do not serve: several devices, parameter-sliced staged updates, an
    androidhelper session, or a dtype ``fa_trimmed_mean`` does not take."""


def trim_count(trim_fraction, K):
    """Values dropped at EACH end of K sorted values: ``floor(trim_fraction * K)``, never more than
    ``(K - 1) // 2`` (at least one value is kept whatever the product's rounding does)."""
    return max(0, min(math.floor(trim_fraction * K), (K - 1) // 2))


def krum_f(byzantine_fraction, K):
    """Byzantine clients Krum assumes among K: ``floor(byzantine_fraction * K)``, never more than the
    paper's condition ``2f + 2 < K`` allows (``(K - 3) // 2``); 0 below K = 3."""
    if K < 3:
        return 0
    return max(0, min(math.floor(byzantine_fraction * K), (K - 3) // 2))


def krum_scores(D, f):
    """Krum's score of each of the K clients of the K x K squared-distance matrix ``D``, in float64:
    the sum of the ``nn = max(K - f - 2, min(1, K - 1))`` smallest ``D[i][j]``, j != i, sorted ascending
    and summed in that order. A non-finite entry counts as +inf."""
    D = np.array(D, dtype=np.float64)
    if D.ndim != 2 or D.shape[0] != D.shape[1] or D.shape[0] < 1:
        raise ValueError(f"a square distance matrix is needed, got shape {D.shape}")
    K = D.shape[0]
    if not 0 <= f < max(K, 1):
        raise ValueError(f"f={f} of K={K} clients")
    D[~np.isfinite(D)] = np.inf
    nn = max(K - f - 2, min(1, K - 1))
    scores = np.zeros(K, dtype=np.float64)
    for i in range(K):
        near = np.sort(np.delete(D[i], i))[:nn]
        acc = np.float64(0.0)
        for v in near:
            acc = acc + v
        scores[i] = acc
    return scores


def krum_select(D, f, m):
    """The FIFO indices (ascending) of the ``m`` clients with the smallest :func:`krum_scores`; ties go
    to the lower index. Krum is ``m = 1``, Multi-Krum ``m = K - f``. Raises ``ValueError`` when fewer
    than ``m`` scores are finite: there is nothing trustworthy to select."""
    scores = krum_scores(D, f)
    K = scores.size
    if not 1 <= m <= K:
        raise ValueError(f"m={m} of K={K} clients")
    finite = int(np.isfinite(scores).sum())
    if finite < m:
        raise ValueError(f"only {finite} of {K} Krum scores are finite, {m} are to be selected")
    order = np.argsort(scores, kind="stable")          # stable: equal scores stay in FIFO order
    return sorted(int(i) for i in order[:m])


def bulyan_f(byzantine_fraction, K):
    """Byzantine clients Bulyan assumes among K: ``floor(byzantine_fraction * K)``, never more than the
    paper's condition ``K >= 4f + 3`` allows (``(K - 3) // 4``); 0 below K = 3."""
    if K < 3:
        return 0
    return max(0, min(math.floor(byzantine_fraction * K), (K - 3) // 4))


def bulyan_select(D, f):
    """Bulyan's selection: Krum iterated ``theta = K - 2f`` times on the shrinking set of clients of the
    K x K squared-distance matrix ``D``. Each iteration takes :func:`krum_scores` of the remaining clients'
    sub-matrix, picks the one with the smallest score (ties to the lower FIFO index) and removes it.
    Returns ``(selected, pick_order, pick_scores)``: the picked FIFO indices ascending, in pick order, and
    each pick's score at its iteration. Raises ``ValueError`` when a pick's score is not finite: nothing
    trustworthy is left."""
    D = np.array(D, dtype=np.float64)
    if D.ndim != 2 or D.shape[0] != D.shape[1] or D.shape[0] < 1:
        raise ValueError(f"a square distance matrix is needed, got shape {D.shape}")
    K = D.shape[0]
    theta = K - 2 * f
    if f < 0 or (f > 0 and K < 4 * f + 3):
        raise ValueError(f"f={f} of K={K} clients: Bulyan needs K >= 4f + 3")
    left = list(range(K))
    order, scores = [], []
    for _ in range(theta):
        sc = krum_scores(D[np.ix_(left, left)], f)
        best = int(np.argmin(sc))                      # the first of equal scores: the lower FIFO index
        if not np.isfinite(sc[best]):
            raise ValueError(f"after {len(order)} of {theta} picks no remaining client has a finite Krum score")
        order.append(left.pop(best))
        scores.append(float(sc[best]))
    return sorted(order), order, scores


def weiszfeld_weights(d, nu):
    """The weights of one smoothed Weiszfeld step from the K squared distances ``d`` to the current
    point, in float64: ``w_k = 1 / max(nu, sqrt(d_k))`` where ``d_k`` is finite, else 0; the sum is taken
    in index order and ``beta = w / sum``. Raises ``ValueError`` when every weight is 0."""
    d = np.asarray(d, dtype=np.float64).reshape(-1)
    nu = np.float64(nu)
    w = np.zeros(d.size, dtype=np.float64)
    total = np.float64(0.0)
    with np.errstate(invalid="ignore"):
        for k in range(d.size):
            if np.isfinite(d[k]):
                r = np.sqrt(d[k])
                w[k] = np.float64(1.0) / (nu if nu > r else r)       # (a NaN r, from d < 0, keeps nu)
            total = total + w[k]
    if not total > 0.0:
        raise ValueError(f"no client has a finite distance: {d}")
    return w / total


def clip_coefficients(d, tau):
    """The coefficients of one centred-clipping step from the K squared distances ``d`` to the current
    point, in float64 and in index order: ``r = sqrt(d_k)``, ``lambda_k = 1`` where ``r <= tau`` else
    ``tau / r``, and 0 where ``r`` is not finite (a non-finite or negative ``d_k``); ``coef_k = lambda_k /
    K_good`` with ``K_good`` the number of clients with a finite ``r``. Raises ``ValueError`` when there is
    none."""
    d = np.asarray(d, dtype=np.float64).reshape(-1)
    tau = np.float64(tau)
    lam = np.zeros(d.size, dtype=np.float64)
    good = 0
    with np.errstate(invalid="ignore"):
        for k in range(d.size):
            r = np.sqrt(d[k])
            if np.isfinite(r):
                lam[k] = np.float64(1.0) if r <= tau else tau / r
                good += 1
    if good == 0:
        raise ValueError(f"no client has a finite distance: {d}")
    return lam / np.float64(good)


def _several_devices():
    from .aggregators.fedavg import env_devices
    devs = env_devices()
    return bool(devs and len(devs) > 1)


class RobustPipeline:
    """Holds one round's updates and reduces them with ``fa_trimmed_mean`` on one device."""

    def __init__(self, device, first, tag=None, budget=None):
        if _several_devices():
            raise UnsupportedRound("the robust rules run on one device: FEDN_AMD_DEVICES names several")
        if isinstance(first, ShardedStagedModel):
            raise UnsupportedRound("the robust rules run on one device: the update is staged as parameter slices")
        self.device = torch.device(device)
        self.layout = first.layout if isinstance(first, StagedModel) else Layout.of([np.asarray(a) for a in first])
        self._out_dt = {}
        for dt in self.layout.groups:
            try:
                self._out_dt[dt] = ops.order_mean_dtype(ops.torch_dtype(dt))
            except TypeError as e:
                raise UnsupportedRound(f"the robust rules take float32 / float64 / float16 / int32 / int64 tensors: {e}") from e
        self.budget = budget if budget is not None else HbmBudget()
        self.compute = torch.cuda.current_stream(self.device)
        self.copy = torch.cuda.Stream(self.device)
        self.updates = []            # StagedModel (in HBM) or list[np.ndarray] (host-side), FIFO
        self.tags = []
        self.host_side = 0           # updates the budget (or a full HBM) left on the host
        self._h2d, self._kern = [], []
        self.selected, self.scores = None, None     # select_mean: FIFO indices, float64 scores
        self.pick_order = None                      # bulyan: the selected FIFO indices in pick order
        self.weights, self.distances = None, None   # geometric_median: the last pass's beta, sqrt(d)
        self.excluded, self.trace = [], []          # ... clients shut out as non-finite; (beta, d) per pass
        self.coefficients = None                    # centered_clip: the last pass's clipping coefficients
        self.sigma, self.clipped = None, None       # dp_clipped_mean: the noise's std, clients scaled down
        self.time_pack = 0.0
        self.time_d2h = 0.0
        self.add(first, tag)

    def __len__(self):
        return len(self.updates)

    # ---- admission -------------------------------------------------------------------
    def add(self, update, tag=None):
        """Admit one update: a StagedModel is used in place; host arrays go to HBM now (copy stream)
        if the budget admits them, else stay on the host. Raises if its layout differs from the
        round's (the first update's), so the aggregator skips it."""
        if isinstance(update, ShardedStagedModel):
            raise UnsupportedRound("the robust rules run on one device: the update is staged as parameter slices")
        if isinstance(update, StagedModel):
            self.layout.check_layout(update.layout)
            if update.dev.device != self.device:
                raise ValueError(f"staged update is on {update.dev.device}, the round runs on {self.device}")
            entry = update
        else:
            arrays = [np.asarray(a) for a in update]
            self.layout.check(arrays)
            entry = self._stage(arrays)
        self.updates.append(entry)
        self.tags.append(tag)

    def _stage(self, arrays):
        parts = [(self.device, self.layout.nbytes)]
        if self.budget.reserve(parts):
            try:
                tic = time.perf_counter()
                with torch.cuda.device(self.device):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(self.copy)
                    staged = ingest.stage_arrays(arrays, self.device, self.copy)
                    b.record(self.copy)
                self._h2d.append((a, b))
                self.time_pack += time.perf_counter() - tic
                return self.budget.hold(staged, parts)
            except torch.cuda.OutOfMemoryError:
                self.budget.release(parts)
        self.host_side += 1
        return arrays

    # ---- reduction -------------------------------------------------------------------
    def _clients(self, cap=ops.MAX_ORDER_K):
        """K, the round's size, within the rule's ``cap`` — what one launch's table holds, or
        ``ops.MAX_CLIP_K`` for the two clipping rules, which fold by chunks: every rule's first check, ahead
        of those of its own arguments."""
        K = len(self.updates)
        if not 1 <= K <= cap:
            raise ValueError(f"a robust round takes 1..{cap} updates, got {K}")
        return K

    def _round(self, body, center=None):
        """The frame of every rule, around its arithmetic ``body``: on the round's device and compute
        stream, wait for every staged update's ``ready`` event, run ``body()`` — it returns the result's
        dtype groups as pinned host tensors, their copies still in flight — synchronise the compute stream
        (timed as D2H) and unpack the groups into host arrays of the layout's shapes.

        ``center`` (centred clipping: the global model's dtype groups as pinned host tensors) is uploaded
        ahead of the waits, allocated on the compute stream that writes and reads it, handed to
        ``body(cen)`` as device tensors by dtype group and copied back into its host tensors ahead of the
        closing synchronise: those are then the result.

        When anything inside fails, what was enqueued drains before the caller may free anything it reads."""
        out = [None] * len(self.layout.shapes)
        try:
            with torch.cuda.device(self.device), torch.cuda.stream(self.compute):
                if center is not None:
                    cen = {}
                    for dt, host in center.items():
                        cen[dt] = torch.empty(host.numel(), dtype=host.dtype, device=self.device)
                        cen[dt].copy_(host, non_blocking=True)
                for u in self.updates:
                    if isinstance(u, StagedModel):
                        self.compute.wait_event(u.ready)
                hosts = body() if center is None else body(cen)
                tic = time.perf_counter()
                if center is not None:
                    hosts = center
                    for dt, host in center.items():
                        host.copy_(cen[dt], non_blocking=True)
                self.compute.synchronize()
                self.time_d2h += time.perf_counter() - tic
        except BaseException:
            torch.cuda.synchronize(self.device)
            raise
        for dt in self.layout.groups:
            self.layout.unpack_group(hosts[dt].numpy(), dt, out, copy=False)
        return out

    def result(self, trim):
        """The round's model as host arrays in the layout's shapes (dtypes: ``ops.order_mean_dtype``):
        per element the mean of the sorted values ``s[trim] .. s[K - trim - 1]``."""
        K = self._clients()
        if trim < 0 or 2 * trim >= K:
            raise ValueError(f"trim={trim} leaves nothing of {K} updates")
        return self._round(lambda: {dt: self._reduce_group(dt, trim) for dt in self.layout.groups})

    def select_mean(self, f, m):
        """Krum (``m = 1``) / Multi-Krum (``m = K - f``): the unweighted mean of the ``m`` updates that
        :func:`krum_select` picks, as host arrays like :meth:`result`'s; ``self.selected`` (FIFO indices)
        and ``self.scores`` stay on the pipeline.

        Pass 1 walks the dtype groups — slice by slice where updates sit on the host, through the same
        ring as :meth:`result` — and sums their squared distances into one K x K matrix on the device
        (``ops.pairwise_sqdist(..., accumulate=...)``); the matrix goes to the host and the selection is
        made there in float64. Pass 2 is the trimmed mean at ``trim = 0`` over the selected updates only
        (``A(y) / 1``, the converting copy, for Krum's single one). A selected update that sits on the
        host is therefore uploaded a second time, slice by slice: HBM stays bounded by the budget plus
        the ring. Raises ``ValueError`` when fewer than ``m`` clients have a finite score."""
        K = self._clients()
        if not (0 <= f < K and 1 <= m <= K):
            raise ValueError(f"f={f}, m={m} of {K} updates")

        def body():
            Dh = self._distance_matrix(K)
            self.scores = krum_scores(Dh, f)
            self.selected = krum_select(Dh, f, m)
            return {dt: self._reduce_group(dt, 0, self.selected) for dt in self.layout.groups}

        return self._round(body)

    def bulyan(self, f):
        """Bulyan (El Mhamdi, Guerraoui and Rouault, 2018) with ``f`` assumed Byzantine
        clients, ``K >= 4f + 3``: :func:`bulyan_select` picks ``theta = K - 2f`` updates by iterated Krum,
        and per coordinate the ``beta = theta - 2f`` of their values closest to their median are averaged
        (``ops.median_window_mean``, kernel ``k_median_window``). Host arrays like :meth:`result`'s;
        ``self.selected`` (FIFO indices, ascending), ``self.pick_order`` and ``self.scores`` (each pick's
        score, in pick order) stay on the pipeline.

        The frame is :meth:`select_mean`'s: one pass for the K x K distance matrix, the selection on the
        host in float64, one reduction over the selected updates — those on the host uploaded a second
        time through the ring. Raises ``ValueError`` when a pick has no finite score."""
        K = self._clients()
        if f < 0 or (f > 0 and K < 4 * f + 3):
            raise ValueError(f"f={f} of {K} updates: Bulyan needs K >= 4f + 3")

        def body():
            Dh = self._distance_matrix(K)
            self.selected, self.pick_order, self.scores = bulyan_select(Dh, f)
            keep = len(self.selected) - 2 * f
            return {dt: self._reduce_group(dt, 0, self.selected, keep) for dt in self.layout.groups}

        return self._round(body)

    def _distance_pass(self, shape, group, coef=None):
        """One pass over the dtype groups that sums squared distances into a zeroed float64 device tensor
        of ``shape``, and that tensor on the host. ``group(dt)`` gives ``(step, after)`` of a dtype group:
        ``step(b, lo, hi, views, stride, acc, accumulate)`` launches one slice's op on the accumulator —
        written by the pass's first launch, added to by the rest — and ``after`` is :meth:`_walk_group`'s.
        With ``coef``, ``(coef, sums)`` is appended to ``trace``. Called inside :meth:`_round`: on the
        compute stream, the staged updates' ``ready`` events already waited for.

        With ``coef`` — a pass of an iterated rule, whose sums become the next pass's weights — the groups
        are walked at the slice bounds WHEREVER the updates sit: the sums are then added in one grouping,
        the same bits whether the budget left updates on the host or not, and so is the model. (The
        selection rules' matrix only has to order the scores: it keeps its one launch per group.)"""
        acc = torch.zeros(shape, dtype=torch.float64, device=self.device)
        written = False
        for dt in self.layout.groups:
            step, after = group(dt)
            if self.layout.group_elems[dt] == 0:     # only empty tensors: no launch
                continue

            def launch(b, lo, hi, views, stride):
                nonlocal written
                step(b, lo, hi, views, stride, acc, written)
                written = True

            self._walk_group(dt, None, launch, after, sliced=coef is not None)
        tic = time.perf_counter()
        sums = acc.cpu().numpy()                     # (synchronises the compute stream)
        self.time_d2h += time.perf_counter() - tic
        if coef is not None:
            self.trace.append((coef, sums))
        return sums

    def _distance_matrix(self, K):
        """The K x K matrix of squared distances between the held updates, on the host."""
        def step(b, lo, hi, views, stride, D, accumulate):
            ops.pairwise_sqdist(views, out=D, accumulate=accumulate, stream=self.compute)

        return self._distance_pass((K, K), lambda dt: (step, None))

    def geometric_median(self, iterations, nu):
        """The smoothed geometric median of the held updates (RFA: Pillutla, Kakade and Harchaoui) by
        ``iterations`` Weiszfeld steps, as host arrays like :meth:`result`'s.

        Pass 0 takes the plain mean (``beta = 1/K``) and the K squared distances to it in ONE fused pass
        (``ops.weighted_mean_sqdist``, kernel ``k_wmean_dist``): the dtype groups are walked — slice by
        slice where updates sit on the host, through the same ring as :meth:`result` — and their
        distances summed into one vector on the device. Passes 1 .. ``iterations`` take
        ``beta = weiszfeld_weights(d, nu)`` of the pass before. Only the last pass stores its mean and
        copies it to the host. Host-side updates are uploaded ONCE PER PASS, slice by slice: HBM stays
        bounded by the budget plus the ring, at ``iterations + 1`` uploads of what the budget refused.

        A non-finite distance after pass 0 means the plain mean was poisoned. Then the K x K distance
        matrix (``fa_pairwise_sqdist``) names the clients whose distance to EVERY other client is
        non-finite; they are excluded (weight 0 in every pass) and pass 0 restarts with ``1/K_good`` on
        the rest. ``ValueError`` when that excludes nobody or everybody, or when a remaining client's
        distance is still non-finite.

        Kept on the pipeline: ``weights`` (the last pass's beta), ``distances`` (sqrt of the last pass's
        d), ``excluded`` (FIFO indices) and ``trace`` (one ``(beta, d)`` pair per pass, float64)."""
        K = self._clients()
        if iterations < 0 or not (nu > 0 and np.isfinite(nu)):
            raise ValueError(f"iterations={iterations}, nu={nu}")
        T = 0 if K == 1 else int(iterations)
        self.weights, self.distances, self.excluded, self.trace = None, None, [], []

        def body():
            beta = np.full(K, 1.0 / K, dtype=np.float64)
            d, hosts = self._weiszfeld_pass(beta, T == 0)
            if not np.isfinite(d).all():
                Dh = self._distance_matrix(K)
                off = ~np.eye(K, dtype=bool)
                bad = [k for k in range(K) if K > 1 and not np.isfinite(Dh[k][off[k]]).any()]
                if not bad or len(bad) == K:
                    raise ValueError(f"non-finite distances to the mean ({d}) and {len(bad)} of {K} clients "
                                     "are non-finite against every other: nothing to exclude")
                self.trace = []
                self.excluded = bad
                beta = np.full(K, 1.0 / (K - len(bad)), dtype=np.float64)
                beta[bad] = 0.0
                d, hosts = self._weiszfeld_pass(beta, T == 0)
                good = np.ones(K, dtype=bool)
                good[bad] = False
                if not np.isfinite(d[good]).all():
                    raise ValueError(f"non-finite distances remain after excluding clients {bad}: {d}")
            for t in range(1, T + 1):
                d, hosts = self._weiszfeld_pass(weiszfeld_weights(d, nu), t == T)
            return hosts

        out = self._round(body)
        self.weights, d = self.trace[-1]             # the last pass's (beta, d)
        with np.errstate(invalid="ignore"):
            self.distances = np.sqrt(d)
        return out

    def _weiszfeld_pass(self, beta, store):
        """One fused pass over every dtype group with the weights ``beta``: ``(d, hosts)`` — the K
        squared distances to the weighted mean as a float64 host array, and (``store``) the mean's
        groups as pinned host tensors, valid once the compute stream is synchronised. Appends
        ``(beta, d)`` to ``trace``."""
        beta = np.array(beta, dtype=np.float64)
        hosts = {}

        def group(dt):
            odt, outs = self._out_dt[dt], {}
            host = hosts[dt] = torch.empty(self.layout.group_elems[dt], dtype=odt, pin_memory=True) if store else None

            def step(b, lo, hi, views, stride, dist, accumulate):
                z = None
                if store:
                    if b not in outs:
                        outs[b] = torch.empty(stride, dtype=odt, device=self.device)
                    z = outs[b][:hi - lo]
                ops.weighted_mean_sqdist(views, beta, out=z, dist=dist, accumulate=accumulate, store=store,
                                         stream=self.compute)

            def after(b, lo, hi):
                host[lo:hi].copy_(outs[b][:hi - lo], non_blocking=True)

            return step, after if store else None

        return self._distance_pass(len(self.updates), group, beta), hosts

    def centered_clip(self, center_arrays, iterations, tau):
        """Centred clipping of the held updates around the previous global model ``center_arrays``
        (Karimireddy, He and Jaggi), ``iterations`` steps with radius ``tau``, as host arrays like
        :meth:`result`'s.

        The centre — arrays of the round's shapes, each tensor of the updates' dtype or of that dtype's
        ``ops.order_mean_dtype`` — is converted to the latter per dtype group on the host and uploaded
        ONCE, allocated on the compute stream; it sits outside the budget like the ring: HBM is bounded
        by the budget plus the ring plus one model. Pass 0 (``coef = 0``, nothing stored) gives the K
        squared distances to the global model; passes 1 .. ``iterations`` take ``coef =
        clip_coefficients(d, tau)`` of the pass before, move the centre IN PLACE — slice by slice where
        updates sit on the host, through the same ring as :meth:`result` — and give the distances to the
        new point (``ops.centered_clip_step``, kernel ``k_cclip_dist``). Only the last pass is followed
        by the centre's copy to the host; ``iterations = 0`` returns the converted centre.

        A client whose distance to the global model is not finite (an ``inf`` or a NaN in its update) is
        excluded: its coefficient is 0 in every pass. ``ValueError`` when that is every client — which a
        non-finite global model also causes — or when a later distance of a remaining client turns
        non-finite.

        A round of more than 64 updates (up to ``ops.MAX_CLIP_K``) takes every pass by chunks of 64 clients
        (:meth:`_clip_pass_chunked`): the same definition and the same kept values.

        Kept on the pipeline: ``coefficients`` (the last pass's), ``distances`` (sqrt of the last pass's
        d), ``excluded`` (FIFO indices) and ``trace`` (one ``(coef, d)`` pair per pass, float64)."""
        K = self._clients(ops.MAX_CLIP_K)
        if iterations < 0 or not (tau > 0 and np.isfinite(tau)):
            raise ValueError(f"iterations={iterations}, tau={tau}")
        L = int(iterations)
        self.coefficients, self.distances, self.excluded, self.trace = None, None, [], []

        def body(cen):
            d = self._clip_pass(np.zeros(K, dtype=np.float64), cen, False)
            good = np.isfinite(d)
            self.excluded = [k for k in range(K) if not good[k]]
            if not good.any():
                raise ValueError(f"no client has a finite distance to the global model: {d}")
            for _ in range(L):
                d = self._clip_pass(clip_coefficients(d, tau), cen, True)
                if not np.isfinite(d[good]).all():
                    raise ValueError(f"a distance turned non-finite after a clipping step: {d}")

        out = self._round(body, self._pack_center(center_arrays))
        self.coefficients, d = self.trace[-1]        # the last pass's (coef, d)
        with np.errstate(invalid="ignore"):
            self.distances = np.sqrt(d)
        return out

    def dp_clipped_mean(self, center_arrays, clip, noise_multiplier, seed, round_id):
        """Central DP-FedAvg with flat clipping (McMahan, Ramage, Talwar and Zhang): the
        global model ``center_arrays`` moved by the mean of the updates' differences to it, each clipped
        to the norm ``clip``, plus Gaussian noise of standard deviation ``sigma = (noise_multiplier * clip)
        / K_good`` on every parameter, as host arrays like :meth:`result`'s.

        The frame and the first two passes are :meth:`centered_clip`'s at one iteration: pass 0 gives the K
        distances to the global model (a client with a non-finite one is excluded), one clipping pass moves
        the centre in place with ``clip_coefficients(d, clip)``. Then ONE launch per dtype group adds the
        noise to the centre in place on the compute stream (``ops.gaussian_noise``, kernel
        ``k_gaussian_noise``) — behind the clipping pass and ahead of the centre's copy to the host — with
        ``stream_id`` the group's index in ``layout.groups`` and ``offset`` 0: the noise is a pure function
        of ``(seed, round_id, group, element)``, the same bits wherever the updates sit. With
        ``noise_multiplier = 0`` nothing is launched and the result is ``centered_clip(center, 1, clip)``
        bit for bit.

        Kept on the pipeline: what :meth:`centered_clip` keeps, ``sigma`` (float64) and ``clipped``, the
        number of clients whose difference was scaled down (``lambda < 1``)."""
        K = self._clients(ops.MAX_CLIP_K)
        if not (clip > 0 and np.isfinite(clip)) or not (noise_multiplier >= 0 and np.isfinite(noise_multiplier)):
            raise ValueError(f"clip={clip}, noise_multiplier={noise_multiplier}")
        for name, v, bits in (("seed", seed, 64), ("round_id", round_id, 32)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) < 1 << bits:
                raise ValueError(f"{name} must be an int in 0 .. 2^{bits} - 1")
        self.coefficients, self.distances, self.excluded, self.trace = None, None, [], []
        self.sigma, self.clipped = None, None

        def body(cen):
            d = self._clip_pass(np.zeros(K, dtype=np.float64), cen, False)
            good = np.isfinite(d)
            self.excluded = [k for k in range(K) if not good[k]]
            if not good.any():
                raise ValueError(f"no client has a finite distance to the global model: {d}")
            with np.errstate(invalid="ignore"):
                self.clipped = int((np.sqrt(d[good]) > np.float64(clip)).sum())
            d = self._clip_pass(clip_coefficients(d, clip), cen, True)
            if not np.isfinite(d[good]).all():
                raise ValueError(f"a distance turned non-finite after the clipping step: {d}")
            self.sigma = (np.float64(noise_multiplier) * np.float64(clip)) / np.float64(int(good.sum()))
            if noise_multiplier > 0:
                for g, dt in enumerate(self.layout.groups):
                    if self.layout.group_elems[dt] == 0:         # only empty tensors: no launch
                        continue
                    k0, k1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    k0.record(self.compute)
                    ops.gaussian_noise(cen[dt], cen[dt], sigma=float(self.sigma), seed=int(seed), stream_id=g,
                                       round_id=int(round_id), offset=0, stream=self.compute)
                    k1.record(self.compute)
                    self._kern.append((k0, k1))

        out = self._round(body, self._pack_center(center_arrays))
        self.coefficients, d = self.trace[-1]        # the clipping pass's (coef, d)
        with np.errstate(invalid="ignore"):
            self.distances = np.sqrt(d)
        return out

    def _pack_center(self, center_arrays):
        """The centre's dtype groups as pinned host tensors of ``ops.order_mean_dtype``, after the layout
        check: the round's shapes, each tensor of the updates' dtype or of that output dtype."""
        arrays = [np.asarray(a) for a in center_arrays]
        if len(arrays) != len(self.layout.shapes):
            raise ValueError(f"the global model has {len(arrays)} tensors, the round's updates {len(self.layout.shapes)}")
        for i, a in enumerate(arrays):
            if tuple(a.shape) != tuple(self.layout.shapes[i]):
                raise ValueError(f"tensor {i} of the global model has shape {a.shape}, the round's {self.layout.shapes[i]}")
        packed = {}
        for dt in self.layout.groups:
            odt = self._out_dt[dt]
            onp = ops.numpy_dtype(odt)
            host = packed[dt] = torch.empty(self.layout.group_elems[dt], dtype=odt, pin_memory=True)
            flat = host.numpy()
            for i, off in self.layout.members[dt]:
                a = arrays[i]
                if a.dtype != dt and a.dtype != onp:
                    raise ValueError(f"tensor {i} of the global model is {a.dtype}, the round's updates are {dt} "
                                     f"(a global model of {onp} is taken too)")
                flat[off:off + a.size] = a.reshape(-1)         # (dt -> its output dtype is exact)
        return packed

    def _clip_pass(self, coef, cen, store):
        """One fused pass over every dtype group with the coefficients ``coef``: the K squared distances to
        the new point as a float64 host array; with ``store`` the centre ``cen`` (device tensors by dtype
        group) is moved in place. Appends ``(coef, d)`` to ``trace``."""
        coef = np.array(coef, dtype=np.float64)
        if len(self.updates) > ops.MAX_ORDER_K:
            return self._clip_pass_chunked(coef, cen, store)

        def group(dt):
            def step(b, lo, hi, views, stride, dist, accumulate):
                v = cen[dt][lo:hi]
                ops.centered_clip_step(views, v, coef, out=v if store else None, dist=dist, accumulate=accumulate,
                                       store=store, stream=self.compute)

            return step, None

        return self._distance_pass(len(self.updates), group, coef)

    def _clip_pass_chunked(self, coef, cen, store):
        """:meth:`_clip_pass` for a round of more than ``ops.MAX_ORDER_K`` updates: the same
        definition, the same ``trace`` entry. Every dtype group is walked at the slice bounds, wherever the
        updates sit, and within a slice the clients in chunks of 64 in FIFO order:

          * ``store``: one ``ops.clip_fold`` per chunk that has a nonzero coefficient, over its clients with a
            nonzero coefficient alone (the others are not read, and not uploaded). The first launch starts
            from the centre's slice, the last writes it in place, the ones between hand the accumulator on
            through a carry of one slice in the compute type — allocated on the compute stream, reused by
            every slice in stream order;
          * then, per chunk, ``ops.centered_clip_step`` with zero coefficients and nothing stored adds the
            chunk's squared distances to the slice of the (moved) centre into its range of ``d``: that range
            is written by the chunk's first launch of the pass and added to by the rest, in this one order —
            the same bits whether the budget left updates on the host or not.

        Host-side updates go through a ring of two buffers of at most 64 rows of one slice, one buffer per
        launch: in a moving pass such an update is uploaded once for the fold and once for the distances,
        the cost of ``v'`` depending on all K clients."""
        K = len(self.updates)
        CH = ops.MAX_ORDER_K
        chunks = [(c0, min(K, c0 + CH)) for c0 in range(0, K, CH)]
        live = [[k for k in range(c0, c1) if coef[k] != 0.0] for c0, c1 in chunks] if store else []
        folds = [ks for ks in live if ks]
        d = torch.zeros(K, dtype=torch.float64, device=self.device)
        written = [False] * len(chunks)
        zeros = [0.0] * CH
        for dt in self.layout.groups:
            n = self.layout.group_elems[dt]
            if n == 0:                               # only empty tensors: no launch
                continue
            tdt = ops.torch_dtype(dt)
            isz, goff = dt.itemsize, self.layout.group_byte_offset[dt]
            step = min(n, max(SLICE_ALIGN, SLICE_BYTES // isz // SLICE_ALIGN * SLICE_ALIGN))
            host = [k for k in range(K) if not isinstance(self.updates[k], StagedModel)]
            flats = {k: self._host_flat(self.updates[k], dt) for k in host}
            rows = max((sum(1 for k in range(c0, c1) if k in flats) for c0, c1 in chunks), default=0)
            ring, consumed, turn = None, [None, None], 0
            if rows:
                with torch.cuda.stream(self.copy):   # allocated on the stream that writes it
                    row = -(-step // SLICE_ALIGN) * SLICE_ALIGN
                    ring = reuse.watch(torch.empty((2, rows, row), dtype=tdt, device=self.device), self.copy)
            carry = None
            if len(folds) > 1:                       # (on the compute stream: the current one inside _round)
                carry = torch.empty(step, dtype=ops.clip_compute_dtype(tdt), device=self.device)

            def launch(ks, lo, hi, op):
                """``op(views)`` on slice [lo, hi) of the clients ``ks`` (one chunk's): the host-side ones
                through the ring's next buffer."""
                nonlocal turn
                up = [k for k in ks if k in flats]
                b = turn % 2
                if up:
                    turn += 1
                    if consumed[b] is not None:
                        self.copy.wait_event(consumed[b])      # the launch that read this buffer ran
                    h0, h1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    with torch.cuda.stream(self.copy):
                        h0.record(self.copy)
                        for r, k in enumerate(up):
                            for flat, off in flats[k]:         # members overlapping [lo, hi)
                                s0, s1 = max(lo, off), min(hi, off + flat.size)
                                if s0 < s1:
                                    ring[b, r, s0 - lo:s1 - lo].copy_(torch.from_numpy(flat[s0 - off:s1 - off]),
                                                                      non_blocking=True)
                        h1.record(self.copy)
                    self._h2d.append((h0, h1))
                    self.compute.wait_event(h1)
                views, r = [], 0
                for k in ks:
                    u = self.updates[k]
                    if isinstance(u, StagedModel):
                        views.append(u.dev[goff + lo * isz:goff + hi * isz].view(tdt))
                    else:
                        views.append(ring[b, r, :hi - lo])
                        r += 1
                k0, k1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                k0.record(self.compute)
                op(views)
                k1.record(self.compute)
                self._kern.append((k0, k1))
                if up:
                    consumed[b] = torch.cuda.Event()
                    consumed[b].record(self.compute)

            for lo in range(0, n, step):
                hi = min(n, lo + step)
                v = cen[dt][lo:hi]
                for i, ks in enumerate(folds):
                    first, last = i == 0, i == len(folds) - 1
                    acc = carry[:hi - lo] if carry is not None else None
                    launch(ks, lo, hi, lambda views, ks=ks, first=first, last=last, acc=acc: ops.clip_fold(
                        views, v, coef[ks], out=v if last else None, carry_in=None if first else acc,
                        carry_out=None if last else acc, stream=self.compute))
                for j, (c0, c1) in enumerate(chunks):
                    launch(list(range(c0, c1)), lo, hi, lambda views, j=j, c0=c0, c1=c1: ops.centered_clip_step(
                        views, v, zeros[:c1 - c0], dist=d[c0:c1], accumulate=written[j], store=False,
                        stream=self.compute))
                    written[j] = True
            if ring is not None:
                ring.record_stream(self.compute)
        tic = time.perf_counter()
        sums = d.cpu().numpy()                       # (synchronises the compute stream)
        self.time_d2h += time.perf_counter() - tic
        self.trace.append((coef, sums))
        return sums

    def _host_flat(self, arrays, dt):
        """(flat array, element offset in the group) of the non-empty members of group ``dt``."""
        return [(np.ascontiguousarray(arrays[i]).reshape(-1), off) for i, off in self.layout.members[dt]
                if self.layout.sizes[i]]

    def _reduce_group(self, dt, trim, subset=None, keep=None):
        """Group ``dt`` of the trimmed mean over the held updates — all of them, or those at the FIFO
        indices ``subset`` — as a pinned host tensor. With ``keep`` the rule is the mean of the ``keep``
        values closest to the median instead (``ops.median_window_mean``; ``trim`` plays no part)."""
        n = self.layout.group_elems[dt]
        odt = self._out_dt[dt]
        host = torch.empty(n, dtype=odt, pin_memory=True)
        if n == 0:                                   # only empty tensors: no launch
            return host
        outs = {}

        def launch(b, lo, hi, views, step):
            if b not in outs:
                outs[b] = torch.empty(step, dtype=odt, device=self.device)
            if keep is None:
                ops.trimmed_mean(outs[b][:hi - lo], views, trim, stream=self.compute)
            else:
                ops.median_window_mean(outs[b][:hi - lo], views, keep, stream=self.compute)

        def after(b, lo, hi):
            # the result leaves on the compute stream: in order behind its launch and ahead of the
            # launch that reuses outs[b]
            host[lo:hi].copy_(outs[b][:hi - lo], non_blocking=True)

        self._walk_group(dt, subset, launch, after)
        return host

    def _walk_group(self, dt, subset, launch, after, sliced=False):
        """Run ``launch(b, lo, hi, views, step)`` over group ``dt`` of the updates at ``subset`` (all when
        None): once when they all sit in HBM, else slice by slice with the host-side ones copied through
        the two-buffer ring; ``after(b, lo, hi)`` follows each launch's timing events. ``sliced`` walks
        the slice bounds even when every update sits in HBM (no ring then: the views are the updates' own).

        Every view handed to ``launch`` starts on a 16-byte boundary, so the kernels take their 16-byte
        load paths: a staged update's group starts at a multiple of ``layout.ALIGN`` bytes, slices
        start at multiples of ``SLICE_ALIGN`` elements, and the ring's rows are padded to one."""
        n = self.layout.group_elems[dt]
        tdt = ops.torch_dtype(dt)
        isz, goff = dt.itemsize, self.layout.group_byte_offset[dt]
        used = list(range(len(self.updates))) if subset is None else list(subset)
        on_host = [k for k in used if not isinstance(self.updates[k], StagedModel)]
        if on_host or sliced:
            step = max(SLICE_ALIGN, SLICE_BYTES // isz // SLICE_ALIGN * SLICE_ALIGN)
        else:
            step = n                                 # every update in HBM: one launch
        step = min(step, n)
        nbuf = 2 if n > step else 1
        flats = {k: self._host_flat(self.updates[k], dt) for k in on_host}
        ring = None
        if on_host:
            with torch.cuda.stream(self.copy):       # allocated on the stream that writes it
                row = -(-step // SLICE_ALIGN) * SLICE_ALIGN        # (a group shorter than a slice: step = n)
                ring = reuse.watch(torch.empty((nbuf, len(on_host), row), dtype=tdt, device=self.device), self.copy)
        consumed = [None] * nbuf
        for s, lo in enumerate(range(0, n, step)):
            hi, b = min(n, lo + step), s % nbuf
            if on_host:
                if consumed[b] is not None:
                    self.copy.wait_event(consumed[b])          # the launch that read this buffer ran
                h0, h1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with torch.cuda.stream(self.copy):
                    h0.record(self.copy)
                    for r, k in enumerate(on_host):
                        for flat, off in flats[k]:             # members overlapping [lo, hi)
                            s0, s1 = max(lo, off), min(hi, off + flat.size)
                            if s0 < s1:
                                ring[b, r, s0 - lo:s1 - lo].copy_(torch.from_numpy(flat[s0 - off:s1 - off]),
                                                                  non_blocking=True)
                    h1.record(self.copy)
                self._h2d.append((h0, h1))
                self.compute.wait_event(h1)
            views, r = [], 0
            for k in used:
                u = self.updates[k]
                if isinstance(u, StagedModel):
                    views.append(u.dev[goff + lo * isz:goff + hi * isz].view(tdt))
                else:
                    views.append(ring[b, r, :hi - lo])
                    r += 1
            k0, k1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            k0.record(self.compute)
            launch(b, lo, hi, views, step)
            k1.record(self.compute)
            self._kern.append((k0, k1))
            if on_host:
                consumed[b] = torch.cuda.Event()
                consumed[b].record(self.compute)
            if after is not None:
                after(b, lo, hi)
        if ring is not None:
            ring.record_stream(self.compute)

    # ---- bookkeeping -----------------------------------------------------------------
    def timings(self):
        """GPU-side H2D and kernel time (s, HIP events) plus host staging and D2H wall time."""
        torch.cuda.synchronize(self.device)
        h2d = sum(a.elapsed_time(b) for a, b in self._h2d) / 1e3
        kern = sum(a.elapsed_time(b) for a, b in self._kern) / 1e3
        return {"time_h2d": h2d, "time_kernel": kern, "time_pack": self.time_pack, "time_d2h": self.time_d2h}

    def release(self):
        """Drop the round's updates once nothing enqueued reads them (their HBM returns to the budget)."""
        torch.cuda.synchronize(self.device)
        self.updates, self.tags = [], []
