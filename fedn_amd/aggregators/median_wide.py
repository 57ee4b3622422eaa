"""Coordinate-wise median for cohorts of up to 1024 updates — the ``median`` plug-in with the cap raised
from 64 to ``ops.MAX_WIDE_ORDER_K``: ``np.median(S, axis=0)`` bit for bit, the
``trimmedmean_wide`` plug-in's path (trimmedmean_wide.py; kernel ``k_order_wide`` past 64 updates, DESIGN.md
§3.14) at the trim count ``(K - 1) // 2``.

No parameters; contract, deletes and limits (one device, unweighted, at most 1024 updates a round) are the
``median`` plug-in's. A separate module because FEDn selects aggregators by module name
(aggregatorbase.py:44-62). Install with a shim ``fedn/network/combiner/aggregators/median_wide.py``
(INTEGRATION.md).
"""
from .. import ops
from . import median


class Aggregator(median.Aggregator):
    """Coordinate-wise median of up to 1024 updates on MI355X."""

    max_updates = ops.MAX_WIDE_ORDER_K

    def __init__(self, update_handler, device=None, hbm_budget=None):
        super().__init__(update_handler, device=device, hbm_budget=hbm_budget)
        self.name = "median_wide"

    def reduce_round(self, pipe, K, parameters):
        return pipe.result_wide(self.trim(K, parameters))
