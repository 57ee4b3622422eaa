"""Coordinate-wise trimmed mean for cohorts of up to 1024 updates — the ``trimmedmean`` plug-in with the
cap raised from 64 to ``ops.MAX_WIDE_ORDER_K``. The rule's guarantee improves with the cohort: it tolerates
``t = floor(trim_fraction * K)`` faulty or hostile clients per parameter.

The definition is unchanged, ``np.sort(S, axis=0)[t:K - t].mean(axis=0)`` bit for bit. Up to
64 admitted updates the round runs the ``trimmedmean`` plug-in's kernel; past that one pass of
``fa_order_mean_wide`` reads every update once while a wavefront sorts each parameter's K values (kernel
``k_order_wide``).

Parameters, validation, deletes and limits are the ``trimmedmean`` plug-in's (trimmedmean.py): one device,
unweighted, no androidhelper sessions; past 1024 admitted updates the round is ``(None, data)`` and nothing
is deleted. All K updates are held at once — in HBM while the budget admits them, on the host otherwise, then
reduced slice by slice.

A separate module because FEDn selects aggregators by module name (aggregatorbase.py:44-62). Install with a
shim ``fedn/network/combiner/aggregators/trimmedmean_wide.py``.
"""
from .. import ops
from . import trimmedmean


class Aggregator(trimmedmean.Aggregator):
    """Coordinate-wise trimmed mean of up to 1024 updates on MI355X."""

    max_updates = ops.MAX_WIDE_ORDER_K

    def __init__(self, update_handler, device=None, hbm_budget=None):
        super().__init__(update_handler, device=device, hbm_budget=hbm_budget)
        self.name = "trimmedmean_wide"

    def reduce_round(self, pipe, K, parameters):
        return pipe.result_wide(self.trim(K, parameters))
