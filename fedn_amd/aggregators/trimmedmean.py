"""Coordinate-wise trimmed-mean aggregator plug-in (Yin et al., 2018) — a robust rule FEDn does not
ship; its users write it as a server function in numpy.

Per parameter, the K admitted updates' values are sorted, the ``t = floor(trim_fraction * K)``
smallest and the ``t`` largest are dropped, and the rest averaged:
``np.sort(S, axis=0)[t:K - t].mean(axis=0)`` bit for bit, with ``-0`` before ``+0`` and NaNs last
(``fa_trimmed_mean``). Up to ``t`` faulty or hostile clients — a diverged model, an
``inf``, a NaN — cannot move any parameter past the honest ones' range.

The rule is UNWEIGHTED by definition: ``num_examples`` is validated by the update handler as always,
but it is not a weight here.

Contract (AggregatorBase's and FEDn's, fedavg.py:22-83):
  * drains ``update_handler.model_updates`` in FIFO order; a load failure, and an update whose layout
    differs from the round's first, is logged and skipped (and stays in storage);
  * ``parameters={"trim_fraction": float}`` (default 0.1), validated like FedOpt's (fedopt.py:123-137):
    a value that is not a ``float`` or lies outside [0, 0.5), or an unknown key, returns
    ``(None, data)`` before any device work — the queue is drained, nothing is deleted;
  * returns ``(model, data)`` with ``time_model_load``, ``time_model_aggregation``,
    ``nr_aggregated_models`` and the GPU timing keys (``time_h2d``, ``time_kernel``, ``time_pack``,
    ``time_d2h``); ``(None, data)`` when nothing was admitted. The model is numpy arrays in the
    layout's shapes; float tensors keep their dtype, integer tensors become float64 (numpy's mean);
  * all K updates are needed at once, so updates are deleted only after the result exists; after a
    failed launch the round is ``(None, data)`` and every update stays in storage.

Limits: one device (``FEDN_AMD_DEVICES`` with several entries, parameter-sliced staged updates and
androidhelper sessions are refused: every update is logged and skipped, the round is ``(None, data)``);
at most ``max_updates`` admitted updates per round (64 here) — more are logged, the round is
``(None, data)`` and nothing is deleted.
"""
import contextlib
import logging
import time
import traceback

import torch

from .. import ops
from ..exceptions import InvalidParameterError
from ..parameters import Parameters
from ..robust import RobustPipeline, UnsupportedRound, trim_count
from ..staging import helper_kind
from .aggregatorbase import AggregatorBase, queued_updates
from .fedavg import default_device

logger = logging.getLogger("fedn")

DEFAULT_PARAMETERS = {"trim_fraction": 0.1}
PARAMETER_SCHEMA = {"trim_fraction": float}


class Aggregator(AggregatorBase):
    """Coordinate-wise trimmed mean on MI355X."""

    default_parameters = DEFAULT_PARAMETERS
    parameter_schema = PARAMETER_SCHEMA
    fraction_parameter = "trim_fraction"      # the one parameter, a float in [0, fraction_bound) (subclasses rename it)
    fraction_bound = 0.5                      # ... and its exclusive upper bound (bulyan.py lowers it)
    max_updates = ops.MAX_ORDER_K             # admitted updates a round takes at most (dpfedavg.py raises it)

    def __init__(self, update_handler, device=None, hbm_budget=None):
        super().__init__(update_handler)
        self.name = "trimmedmean"
        self.device = torch.device(device) if device is not None else None
        self.hbm_budget = hbm_budget      # budget.HbmBudget of host updates staged on arrival (default: its own)
        self.host_side = 0                # updates of the last round the budget left on the host

    def trim(self, K, parameters):
        """Values dropped at each end of the K admitted updates' sorted values."""
        return trim_count(parameters["trim_fraction"], K)

    def prepare_round(self, helper, admitted):
        """Called before :meth:`reduce_round` with the session's helper and the admitted ModelUpdates
        (FIFO): a rule that needs more than the updates fetches it here (centeredclip.py: the global
        model). A failure is a failed round: ``(None, data)``, nothing deleted."""

    def reduce_round(self, pipe, K, parameters):
        """The model of the K admitted updates held by ``pipe`` (the rule itself: subclasses override)."""
        return pipe.result(self.trim(K, parameters))

    def combine_models(self, helper=None, delete_models=True, parameters=None):
        self._begin_deletes()
        try:
            return self._combine(helper, delete_models, parameters)
        finally:
            pipe, self._live = getattr(self, "_live", None), None
            try:
                if pipe is not None:
                    pipe.release()
            finally:
                self._end_round(None)

    def _validate_and_merge_parameters(self, parameters):
        if parameters:
            Parameters(parameters).validate(self.parameter_schema)
            parameters = dict(parameters)
        else:
            parameters = {}
        merged = {**self.default_parameters, **parameters}
        f = merged.get(self.fraction_parameter)
        if f is not None and not 0.0 <= f < self.fraction_bound:       # (a NaN fails both comparisons)
            raise InvalidParameterError(f"Parameter {self.fraction_parameter} must lie in [0, {self.fraction_bound}), got {f}")
        return merged

    def _drain(self):
        """Take every queued update off the queue (none is loaded, none deleted)."""
        q = self.update_handler.model_updates
        while not q.empty():
            try:
                self.update_handler.next_model_update()
            except Exception as e:  # noqa: BLE001
                logger.error(f"AGGREGATOR({self.name}): Error encoutered while draining the queue: {e}")

    def _combine(self, helper, delete_models, parameters):
        data = {"time_model_load": 0.0, "time_model_aggregation": 0.0, "nr_aggregated_models": 0}
        try:
            parameters = self._validate_and_merge_parameters(parameters)
        except InvalidParameterError as e:
            logger.error(f"Aggregator {self.name} received invalid parameters: {e}")
            self._drain()
            return None, data

        pipe = None
        admitted = []             # ModelUpdates in the pipeline, FIFO: deleted once the result exists
        over = 0                  # updates past the max_updates a round takes
        logger.info("AGGREGATOR({}): Aggregating model updates... ".format(self.name))
        with contextlib.closing(queued_updates(self.update_handler, helper, size_box=self._ahead_size)) as updates:
            for model_update, load in updates:
                try:
                    tic = time.time()
                    model_next, _metadata = load()
                    data["time_model_load"] += time.time() - tic

                    tic = time.time()
                    if helper_kind(helper) == "androidhelper":
                        raise UnsupportedRound(f"the {self.name} aggregator does not serve androidhelper sessions")
                    if len(admitted) >= self.max_updates:
                        over += 1                 # counted, not staged: the round is refused below
                    elif pipe is None:
                        pipe = self._live = RobustPipeline(self.device or default_device(), model_next, tag=model_update,
                                                           budget=self.hbm_budget)
                        admitted.append(model_update)
                    else:
                        pipe.add(model_next, tag=model_update)
                        admitted.append(model_update)
                    data["time_model_aggregation"] += time.time() - tic
                except Exception as e:  # noqa: BLE001 — fedavg.py:75-78: log and continue
                    logger.error(f"AGGREGATOR({self.name}): Error encoutered while processing model update: {e}")
                    logger.error(traceback.format_exc())

        K = len(admitted)
        self.host_side = pipe.host_side if pipe is not None else 0
        if pipe is None or K == 0:
            return None, data
        if over:
            logger.error(f"AGGREGATOR({self.name}): {K + over} updates admitted, a round takes at most "
                         f"{self.max_updates}; nothing aggregated, nothing deleted")
            return None, data
        try:
            tic = time.time()
            self.prepare_round(helper, admitted)
            model = self.reduce_round(pipe, K, parameters)
            data["time_model_aggregation"] += time.time() - tic
            data.update(pipe.timings())
        except Exception as e:  # noqa: BLE001 — a failed launch: every update stays in storage
            logger.error(f"AGGREGATOR({self.name}): Error during model aggregation: {e}")
            logger.error(traceback.format_exc())
            return None, data
        if delete_models:
            for mu in admitted:
                try:
                    self.update_handler.delete_model(mu)
                except Exception as e:  # noqa: BLE001 — logged, still counted (fedavg.py:73-78)
                    self._log_skip(e, traceback.format_exc())
        data["nr_aggregated_models"] = K
        logger.info("AGGREGATOR({}): Aggregation completed, aggregated {} models.".format(self.name, K))
        return model, data
