"""Geometric-median aggregator plug-in (RFA, "Robust Aggregation for Federated Learning": Pillutla,
Kakade and Harchaoui) — a robust rule FEDn does not ship; as a numpy server function one Weiszfeld
step costs about 3K passes over the model.

The model is the smoothed geometric median of the K admitted updates: the point with the smallest sum
of Euclidean distances to them, found by ``iterations`` Weiszfeld steps from the plain mean. A step
takes the weights ``beta_k = w_k / sum(w)``, ``w_k = 1 / max(nu, ||u_k - z||)``, from the distances to
the current point ``z`` and moves to ``z = sum_k beta_k u_k``. Its breakdown point is 1/2, the best of
the family, and nothing combinatorial is selected. On the GPU a step is ONE pass over the K updates that
forms the new point and the K distances to it (``fa_weighted_mean_sqdist``, kernel ``k_wmean_dist``),
at the bytes of one FedAvg fold; the weights are a few microseconds on the host in float64
(``robust.weiszfeld_weights``): ``robust.RobustPipeline.geometric_median``, DESIGN.md §3.9.

A client whose update holds an ``inf`` or a NaN poisons the plain mean the iteration starts from. Such
clients — those whose distance to every other client is non-finite — are excluded: their weight is 0 in
every pass, and they are listed in ``agg.excluded``. They still count in ``nr_aggregated_models`` and
are deleted with the rest, as Krum counts the updates it does not select. A round in which that
excludes nobody or everybody (a NaN in every update) is ``(None, data)`` with nothing deleted.

UNWEIGHTED like the rest of the robust family, and for the same reason: a hostile client chooses its own
``num_examples``. It is validated by the update handler as always, but it is not a weight.

``parameters={"iterations": int, "nu": float}`` (defaults 3 and 1e-6; ``iterations`` in 0..100, ``nu``
finite and > 0; ``iterations = 0`` is the plain mean): a wrong type, a value out of range, a NaN or an
unknown key returns ``(None, data)`` with the queue drained, nothing deleted and no device work.
Contract, ``data`` keys, the delete-after-result rule and the refusals (several devices,
parameter-sliced staged updates, androidhelper sessions, more than 64 updates) are the trimmed-mean
plug-in's (trimmedmean.py). Updates the HBM budget leaves on the host are uploaded once per pass.

After a round ``agg.weights`` holds the last step's weights, ``agg.distances`` every client's distance
to the model, ``agg.excluded`` the excluded clients' FIFO indices among the admitted updates and
``agg.trace`` the ``(beta, d)`` pair of every pass; weights, distances and exclusions are logged at info
level.

A separate module because FEDn selects aggregators by module name (aggregatorbase.py:44-62). Install
with a shim ``fedn/network/combiner/aggregators/geomedian.py``.
"""
import logging
import math

from ..exceptions import InvalidParameterError
from ..parameters import Parameters
from . import trimmedmean

logger = logging.getLogger("fedn")

MAX_ITERATIONS = 100


class Aggregator(trimmedmean.Aggregator):
    """Geometric median (RFA) on MI355X."""

    default_parameters = {"iterations": 3, "nu": 1e-6}
    parameter_schema = {"iterations": int, "nu": float}
    fraction_parameter = None

    def __init__(self, update_handler, device=None, hbm_budget=None):
        super().__init__(update_handler, device=device, hbm_budget=hbm_budget)
        self.name = "geomedian"
        self.weights = None               # the last round's final Weiszfeld weights (float64, one per admitted update)
        self.distances = None             # every admitted update's distance to the model
        self.excluded = None              # FIFO indices of the updates shut out as non-finite
        self.trace = None                 # one (beta, d) pair per pass of the last round (RobustPipeline.trace)

    def _validate_and_merge_parameters(self, parameters):
        if parameters:
            Parameters(parameters).validate(self.parameter_schema)
            parameters = dict(parameters)
        else:
            parameters = {}
        merged = {**self.default_parameters, **parameters}
        it, nu = merged["iterations"], merged["nu"]
        if isinstance(it, bool) or not 0 <= it <= MAX_ITERATIONS:
            raise InvalidParameterError(f"Parameter iterations must lie in 0..{MAX_ITERATIONS}, got {it}")
        if not (math.isfinite(nu) and nu > 0.0):
            raise InvalidParameterError(f"Parameter nu must be finite and > 0, got {nu}")
        return merged

    def reduce_round(self, pipe, K, parameters):
        self.weights, self.distances, self.excluded, self.trace = None, None, None, None
        model = pipe.geometric_median(parameters["iterations"], parameters["nu"])
        self.weights, self.distances, self.excluded = pipe.weights, pipe.distances, list(pipe.excluded)
        self.trace = list(pipe.trace)
        logger.info(f"AGGREGATOR({self.name}): K={K}, {len(pipe.trace)} passes: weights "
                    f"{[float(w) for w in self.weights]}, distances {[float(r) for r in self.distances]}, "
                    f"excluded {self.excluded}")
        return model
