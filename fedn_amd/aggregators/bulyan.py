"""Bulyan aggregator plug-in (El Mhamdi, Guerraoui and Rouault, ICML 2018) — a robust rule FEDn does not
ship. It answers Krum's weakness in high dimension: a selected update is close to the others as a whole and
can still hide one huge coordinate. Bulyan selects whole updates AND filters every coordinate.

With K admitted updates and ``f = min(floor(byzantine_fraction * K), (K - 3) // 4)`` assumed Byzantine (the
paper's condition ``K >= 4f + 3``; 0 below K = 3):

  1. Krum is iterated on the shrinking set: ``theta = K - 2f`` times, the remaining client with the smallest
     Krum score among the remaining ones (ties to the earlier one in the queue) is picked and removed;
  2. per coordinate, the ``beta = theta - 2f`` of the picked updates' values closest to their median are
     averaged.

On the GPU that is ONE pass over the K updates for the K x K distance matrix (``fa_pairwise_sqdist``, kernel
``k_pair_sqdist``), ``theta`` selections on the host in float64 (``robust.bulyan_select``), and one pass
over the selected updates that sorts each coordinate's values in registers, finds the window of ``beta``
values around the median and averages it (``fa_median_window_mean``, kernel ``k_median_window``):
``robust.RobustPipeline.bulyan``, DESIGN.md §3.11.

UNWEIGHTED like the rest of the robust family, and for the same reason: a hostile client chooses its own
``num_examples``. It is validated by the update handler as always, but it is not a weight.

``parameters={"byzantine_fraction": float}`` (default 0.2, in [0, 0.25)), validated like the trimmed
mean's ``trim_fraction``: a wrong type, a value out of range, a NaN or an unknown key returns
``(None, data)`` with the queue drained, nothing deleted and no device work. Contract, ``data`` keys,
the delete-after-result rule and the refusals (several devices, parameter-sliced staged updates,
androidhelper sessions, more than 64 updates) are the trimmed-mean plug-in's (trimmedmean.py). A round
in which a pick has no finite score left (NaNs or infs in too many updates) is ``(None, data)`` with
nothing deleted.

After a round ``agg.selected`` holds the selected clients' FIFO indices among the admitted updates
(ascending), ``agg.pick_order`` the same indices in the order they were picked and ``agg.scores`` each
pick's score at its iteration; the selection is logged at info level.

A separate module because FEDn selects aggregators by module name (aggregatorbase.py:44-62). Install
with a shim ``fedn/network/combiner/aggregators/bulyan.py``.
"""
import logging

from ..robust import bulyan_f
from . import multikrum

logger = logging.getLogger("fedn")


class Aggregator(multikrum.Aggregator):
    """Bulyan on MI355X."""

    fraction_bound = 0.25

    def __init__(self, update_handler, device=None, hbm_budget=None):
        super().__init__(update_handler, device=device, hbm_budget=hbm_budget)
        self.name = "bulyan"
        self.pick_order = None            # the last round's selected FIFO indices, in pick order

    def reduce_round(self, pipe, K, parameters):
        self.selected, self.pick_order, self.scores = None, None, None
        f = bulyan_f(parameters["byzantine_fraction"], K)
        model = pipe.bulyan(f)
        self.selected, self.pick_order, self.scores = list(pipe.selected), list(pipe.pick_order), list(pipe.scores)
        logger.info(f"AGGREGATOR({self.name}): K={K}, f={f}: selected updates {self.selected}, "
                    f"{len(self.selected) - 2 * f} values kept per coordinate (picked in order {self.pick_order}, "
                    f"scores {self.scores})")
        return model
