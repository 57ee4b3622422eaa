"""Krum aggregator plug-in (Blanchard et al., NeurIPS 2017): the Multi-Krum plug-in with ``m = 1`` —
the model is the ONE update whose ``K - f - 2`` nearest other updates are closest (the smallest score;
ties to the earlier one in the queue), passed through ``fa_trimmed_mean`` at trim 0, the converting copy
``A(y) / 1`` of DESIGN.md §3.7: float tensors keep their dtype, integer tensors become float64.

``parameters={"byzantine_fraction": float}`` (default 0.2, in [0, 0.5)) as for ``multikrum``; contract,
return value, deletes, limits, ``agg.selected`` and ``agg.scores`` are that plug-in's (multikrum.py,
DESIGN.md §3.8).

A separate module because FEDn selects aggregators by module name (aggregatorbase.py:44-62). Install
with a shim ``fedn/network/combiner/aggregators/krum.py``.
"""
from . import multikrum


class Aggregator(multikrum.Aggregator):
    """Krum on MI355X."""

    def __init__(self, update_handler, device=None, hbm_budget=None):
        super().__init__(update_handler, device=device, hbm_budget=hbm_budget)
        self.name = "krum"

    def selection_size(self, K, f):
        return 1
