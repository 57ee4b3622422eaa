"""Centred-clipping aggregator plug-in (Karimireddy, He and Jaggi, "Learning from History for Byzantine
Robust Optimization", ICML 2021) — a robust rule FEDn does not ship.

The one rule of the robust family anchored at the PREVIOUS GLOBAL MODEL: starting from it, ``iterations``
times

    v <- v + (1 / K_good) * sum_k  min(1, tau / ||u_k - v||) * (u_k - v)

so every update is clipped to a ball of radius ``tau`` around the current point before it is averaged,
and a hostile client moves the model by at most ``tau / K`` per step, however it chooses its update. With
one step it is the plain norm-bounding defence. On the GPU a step is ONE pass over the K updates that
moves the point in place and forms the K distances to the new one (``fa_centered_clip_step``, kernel
``k_cclip_dist``), at the bytes of one FedAvg fold plus one model; the clipping coefficients are a few
microseconds on the host in float64 (``robust.clip_coefficients``):
``robust.RobustPipeline.centered_clip``, DESIGN.md §3.10.

The global model is ``update_handler.load_model(helper, model_id)`` of the first admitted update, as
FedOpt obtains ``model_old``. Its shapes must be the round's; per tensor its dtype must be the updates'
or that dtype's output dtype (after a round of this rule an int32 model is float64). A global model that
is missing, of another layout or non-finite makes the round ``(None, data)`` with nothing deleted.

A client whose distance to the global model is not finite (an ``inf`` or a NaN in its update) has
coefficient 0 in every step and is listed in ``agg.excluded``. It still counts in
``nr_aggregated_models`` and is deleted with the rest, as Krum counts the updates it does not select.

UNWEIGHTED like the rest of the robust family, and for the same reason: a hostile client chooses its own
``num_examples``.

``parameters={"tau": float, "iterations": int}``: ``tau`` is finite and > 0 and has NO default (its scale
is the model's: a missing ``tau`` is an invalid parameter); ``iterations`` lies in 0..100, default 3
(``iterations = 0`` returns the global model). A wrong type, a value out of range, a NaN or an unknown key
returns ``(None, data)`` with the queue drained, nothing deleted and no device work. Contract, ``data``
keys, the delete-after-result rule and the refusals (several devices, parameter-sliced staged updates,
androidhelper sessions, more than 64 updates) are the trimmed-mean plug-in's (trimmedmean.py). Updates
the HBM budget leaves on the host are uploaded once per pass.

After a round ``agg.coefficients`` holds the last step's coefficients, ``agg.distances`` every client's
distance to the model, ``agg.excluded`` the excluded clients' FIFO indices among the admitted updates and
``agg.trace`` the ``(coef, d)`` pair of every pass; all are logged at info level.

A separate module because FEDn selects aggregators by module name (aggregatorbase.py:44-62). Install
with a shim ``fedn/network/combiner/aggregators/centeredclip.py``.
"""
import logging
import math

from .. import ops
from ..exceptions import InvalidParameterError
from ..parameters import Parameters
from . import trimmedmean

logger = logging.getLogger("fedn")

MAX_ITERATIONS = 100


class Aggregator(trimmedmean.Aggregator):
    """Centred clipping on MI355X."""

    default_parameters = {"iterations": 3}
    parameter_schema = {"tau": float, "iterations": int}
    fraction_parameter = None
    # The pipeline's rule takes ops.MAX_CLIP_K updates (the chunked fold); this plug-in's
    # refusal past 64 is its documented behaviour and stays until it is lifted here, in this one line.
    max_updates = ops.MAX_ORDER_K

    def __init__(self, update_handler, device=None, hbm_budget=None):
        super().__init__(update_handler, device=device, hbm_budget=hbm_budget)
        self.name = "centeredclip"
        self.coefficients = None          # the last round's final clipping coefficients (float64, one per admitted update)
        self.distances = None             # every admitted update's distance to the model
        self.excluded = None              # FIFO indices of the updates shut out as non-finite
        self.trace = None                 # one (coef, d) pair per pass of the last round (RobustPipeline.trace)
        self._center = None               # the round's global model, between prepare_round and reduce_round

    def _validate_and_merge_parameters(self, parameters):
        if parameters:
            Parameters(parameters).validate(self.parameter_schema)
            parameters = dict(parameters)
        else:
            parameters = {}
        merged = {**self.default_parameters, **parameters}
        if "tau" not in merged:
            raise InvalidParameterError("Parameter tau is required: the clipping radius has the model's scale")
        it, tau = merged["iterations"], merged["tau"]
        if isinstance(it, bool) or not 0 <= it <= MAX_ITERATIONS:
            raise InvalidParameterError(f"Parameter iterations must lie in 0..{MAX_ITERATIONS}, got {it}")
        if not (math.isfinite(tau) and tau > 0.0):
            raise InvalidParameterError(f"Parameter tau must be finite and > 0, got {tau}")
        return merged

    def prepare_round(self, helper, admitted):
        self._center = None
        model_id = admitted[0].model_id
        center = self.update_handler.load_model(helper, model_id)
        if center is None:
            raise ValueError(f"the global model {model_id} of the round's first update is missing")
        self._center = center

    def reduce_round(self, pipe, K, parameters):
        self.coefficients, self.distances, self.excluded, self.trace = None, None, None, None
        center, self._center = self._center, None
        model = pipe.centered_clip(center, parameters["iterations"], parameters["tau"])
        self.coefficients, self.distances, self.excluded = pipe.coefficients, pipe.distances, list(pipe.excluded)
        self.trace = list(pipe.trace)
        logger.info(f"AGGREGATOR({self.name}): K={K}, {len(pipe.trace)} passes: coefficients "
                    f"{[float(c) for c in self.coefficients]}, distances {[float(r) for r in self.distances]}, "
                    f"excluded {self.excluded}")
        return model
