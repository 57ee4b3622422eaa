"""Coordinate-wise median aggregator plug-in (Yin et al., 2018): the trimmed-mean plug-in with the
trim count ``t = (K - 1) // 2`` for K admitted updates — per parameter the middle value of an odd K,
the mean ``(a + b) / 2`` of the two middle values of an even one; ``np.median(S, axis=0)`` bit for
bit (``-0`` before ``+0``, NaNs last; ``fa_trimmed_mean``).

UNWEIGHTED by definition: ``num_examples`` is validated by the update handler as always, but it is
not a weight. No parameters: any key returns ``(None, data)``, as FEDn's ``Parameters.validate``
refuses unknown keys (fedopt.py:123-137). Contract, return value, deletes and limits (one device, at
most 64 updates per round) are the trimmed-mean plug-in's (trimmedmean.py).

A separate module because FEDn selects aggregators by module name (aggregatorbase.py:44-62). Install
with a shim ``fedn/network/combiner/aggregators/median.py``.
"""
from .. import ops
from . import trimmedmean


class Aggregator(trimmedmean.Aggregator):
    """Coordinate-wise median on MI355X."""

    default_parameters = {}
    parameter_schema = {}

    def __init__(self, update_handler, device=None, hbm_budget=None):
        super().__init__(update_handler, device=device, hbm_budget=hbm_budget)
        self.name = "median"

    def trim(self, K, parameters):
        return ops.median_trim(K)
