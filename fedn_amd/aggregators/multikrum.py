"""Multi-Krum aggregator plug-in (Blanchard et al., NeurIPS 2017) — a robust rule FEDn does not ship;
its users write it as a server function in numpy, where it costs K^2 passes over the model.

Unlike the coordinate-wise rules it selects WHOLE updates. With K admitted updates and
``f = min(floor(byzantine_fraction * K), (K - 3) // 2)`` assumed Byzantine (the paper's condition
``2f + 2 < K``; 0 below K = 3), every client's score is the sum of its ``K - f - 2`` smallest squared
distances to the other clients; the ``m = K - f`` clients with the smallest scores are selected (ties to
the earlier one in the queue) and the model is their plain mean. On the GPU that is ONE pass over the K
updates for the K x K distance matrix (``fa_pairwise_sqdist``, kernel ``k_pair_sqdist``), a few
microseconds of selection on the host in float64 (``robust.krum_select``), and one mean over the
selected updates (``fa_trimmed_mean`` at trim 0): ``robust.RobustPipeline.select_mean``, DESIGN.md §3.8.

UNWEIGHTED like the rest of the robust family, and for the same reason: a hostile client chooses its own
``num_examples``. It is validated by the update handler as always, but it is not a weight.

``parameters={"byzantine_fraction": float}`` (default 0.2, in [0, 0.5)), validated like the trimmed
mean's ``trim_fraction``: a wrong type, a value out of range, a NaN or an unknown key returns
``(None, data)`` with the queue drained, nothing deleted and no device work. Contract, ``data`` keys,
the delete-after-result rule and the refusals (several devices, parameter-sliced staged updates,
androidhelper sessions, more than 64 updates) are the trimmed-mean plug-in's (trimmedmean.py). A round
in which fewer than ``m`` clients have a finite score (NaNs or infs everywhere) is ``(None, data)`` with
nothing deleted.

After a round ``agg.selected`` holds the selected clients' FIFO indices among the admitted updates and
``agg.scores`` every client's score; the selection is logged at info level.

A separate module because FEDn selects aggregators by module name (aggregatorbase.py:44-62). Install
with a shim ``fedn/network/combiner/aggregators/multikrum.py``.
"""
import logging

from ..robust import krum_f
from . import trimmedmean

logger = logging.getLogger("fedn")


class Aggregator(trimmedmean.Aggregator):
    """Multi-Krum on MI355X."""

    default_parameters = {"byzantine_fraction": 0.2}
    parameter_schema = {"byzantine_fraction": float}
    fraction_parameter = "byzantine_fraction"

    def __init__(self, update_handler, device=None, hbm_budget=None):
        super().__init__(update_handler, device=device, hbm_budget=hbm_budget)
        self.name = "multikrum"
        self.selected = None              # FIFO indices of the last round's selected updates
        self.scores = None                # the last round's Krum scores (float64, one per admitted update)

    def selection_size(self, K, f):
        """Updates averaged: all but the f assumed Byzantine."""
        return K - f

    def reduce_round(self, pipe, K, parameters):
        self.selected, self.scores = None, None
        f = krum_f(parameters["byzantine_fraction"], K)
        model = pipe.select_mean(f, self.selection_size(K, f))
        self.selected, self.scores = list(pipe.selected), pipe.scores
        logger.info(f"AGGREGATOR({self.name}): K={K}, f={f}: selected updates {self.selected} "
                    f"(scores {[float(self.scores[i]) for i in self.selected]})")
        return model
