"""Mean-around-median aggregator plug-in ("MeaMed": Xie, Koyejo and Gupta, *Generalized Byzantine-tolerant
SGD*, 2018) — a robust rule FEDn does not ship. It has the coordinate-wise median's breakdown point and
averages most of the cohort instead of one or two values: with K admitted updates and
``b = min(floor(byzantine_fraction * K), (K - 1) // 2)`` assumed Byzantine, every parameter is the mean of the
``keep = K - b`` values closest to that parameter's median.

Per parameter the K values are sorted (``-0`` before ``+0``, NaNs last), the median is taken in the
accumulator type, the window of ``keep`` consecutive sorted values closest to it is found (a tie keeps the
lower window) and summed in ascending order: Bulyan's second stage over the whole cohort, DESIGN.md §3.11 bit
for bit. Up to 64 updates that is ``fa_median_window_mean`` (kernel ``k_median_window``); from 65 to 1024 one
pass of ``fa_median_window_mean_wide`` reads every update once while a wavefront sorts each parameter's values
and counts its window start (kernel ``k_window_wide``):
``robust.RobustPipeline.mean_around_median``.

UNWEIGHTED like the rest of the robust family: ``num_examples`` is validated by the update handler as always,
but it is not a weight.

``parameters={"byzantine_fraction": float}`` (default 0.2, in [0, 0.5)), validated like the trimmed mean's
``trim_fraction``. Contract, ``data`` keys, the delete-after-result rule and the refusals (several devices,
parameter-sliced staged updates, androidhelper sessions) are the trimmed-mean plug-in's (trimmedmean.py);
past 1024 admitted updates the round is ``(None, data)`` and nothing is deleted. All K updates are held at
once — in HBM while the budget admits them, on the host otherwise, then reduced slice by slice.

A separate module because FEDn selects aggregators by module name (aggregatorbase.py:44-62). Install with a
shim ``fedn/network/combiner/aggregators/meamed.py``.
"""
from .. import ops
from ..robust import meamed_keep
from . import trimmedmean


class Aggregator(trimmedmean.Aggregator):
    """Mean around median of up to 1024 updates on MI355X."""

    default_parameters = {"byzantine_fraction": 0.2}
    parameter_schema = {"byzantine_fraction": float}
    fraction_parameter = "byzantine_fraction"
    max_updates = ops.MAX_WIDE_ORDER_K

    def __init__(self, update_handler, device=None, hbm_budget=None):
        super().__init__(update_handler, device=device, hbm_budget=hbm_budget)
        self.name = "meamed"

    def keep(self, K, parameters):
        """Values averaged per parameter of the K admitted updates."""
        return meamed_keep(parameters["byzantine_fraction"], K)

    def reduce_round(self, pipe, K, parameters):
        return pipe.mean_around_median(self.keep(K, parameters))
