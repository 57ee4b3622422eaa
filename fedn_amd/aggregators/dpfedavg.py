"""Central DP-FedAvg aggregator plug-in (McMahan, Ramage, Talwar and Zhang, "Learning Differentially
Private Recurrent Language Models", ICLR 2018, flat clipping) — server-side differential privacy, which
FEDn does not ship.

Starting from the previous global model ``g``,

    model = g + (1 / K_good) * sum_k  min(1, clip / ||u_k - g||) * (u_k - g)  +  N(0, sigma^2 I),
    sigma = noise_multiplier * clip / K_good

so no client moves the mean by more than ``clip / K_good`` and the Gaussian noise is calibrated to that
sensitivity. The clipped mean is one step of centred clipping (``fa_centered_clip_step``, centeredclip.py);
the noise is one deviate per parameter, generated and added ON THE GPU by a counter-based generator
(``fa_gaussian_noise``, kernel ``k_gaussian_noise``: Philox4x32-10 and Box-Muller in float64), a pure
function of ``(seed, round, dtype group, element index)``: ``robust.RobustPipeline.dp_clipped_mean``,
DESIGN.md §3.12.

This is CENTRAL differential privacy under a trusted combiner. No privacy accountant is included: epsilon
follows from ``noise_multiplier``, the clients' sampling rate and the number of rounds, and is the user's
to account. Floating-point Gaussian noise is open to the precision attacks Mironov described (2012); a
discrete mechanism and adaptive clipping are out of scope.

UNWEIGHTED: uniform weights over the admitted updates, the paper's flat-clipping estimator with a fixed
denominator — and, as in the rest of the family, a client chooses its own ``num_examples``.

``parameters={"clip": float, "noise_multiplier": float, "seed": int}``:
  * ``clip`` is finite and > 0, ``noise_multiplier`` finite and >= 0; BOTH are required (a DP aggregator
    that silently adds no noise is a trap; ``noise_multiplier = 0.0`` says so in words);
  * ``seed`` is optional, 0 .. 2^64 - 1. Without it the instance draws ``secrets.randbits(64)`` once and
    never logs it nor puts it in ``data``. With it the session is reproducible, and one warning says that
    a known seed voids the guarantee;
  * a wrong type, a value out of range, a NaN or an unknown key returns ``(None, data)`` with the queue
    drained, nothing deleted and no device work.

The round's noise stream is ``round_id``, a per-instance counter incremented on EVERY ``combine_models``
call (a refused or failed one too), so no two rounds of a session share one.

A round takes up to ``ops.MAX_CLIP_K`` = 1024 admitted updates, not the family's 64: ``sigma`` falls as
``1 / K_good``, so the same privacy costs the model less the larger the cohort is. Past 64 updates the
clipped mean is a chain of ``fa_clip_fold`` launches over chunks of 64 clients that carries the accumulator
in the compute type (kernel ``k_clip_fold``): the same definition bit for bit. More than
1024 are logged, the round is ``(None, data)`` and nothing is deleted.

The global model, the contract, the ``data`` keys, the delete-after-result rule, the excluded non-finite
clients and the other refusals are the centred-clipping plug-in's (centeredclip.py, trimmedmean.py). After a
round ``agg.sigma`` holds the noise's standard deviation, ``agg.clipped`` the number of clients whose
update was scaled down, ``agg.distances`` every client's distance to the clipped mean and
``agg.excluded`` the excluded clients' FIFO indices; all are logged at info level. The seed never is.

A separate module because FEDn selects aggregators by module name (aggregatorbase.py:44-62). Install
with a shim ``fedn/network/combiner/aggregators/dpfedavg.py``.
"""
import logging
import math
import secrets

from .. import ops
from ..exceptions import InvalidParameterError
from ..parameters import Parameters
from . import centeredclip

logger = logging.getLogger("fedn")


class Aggregator(centeredclip.Aggregator):
    """Central DP-FedAvg on MI355X."""

    default_parameters = {}
    parameter_schema = {"clip": float, "noise_multiplier": float, "seed": int}
    max_updates = ops.MAX_CLIP_K          # the noise shrinks with the cohort: rounds past 64 fold by chunks

    def __init__(self, update_handler, device=None, hbm_budget=None):
        super().__init__(update_handler, device=device, hbm_budget=hbm_budget)
        self.name = "dpfedavg"
        self.sigma = None                 # the last round's noise standard deviation (float64)
        self.clipped = None               # ... and the number of its clients whose update was scaled down
        self.round_id = 0                 # the next round's noise stream: one per combine_models call
        self._seed = None                 # drawn or given at the first round; never logged
        self._seed_given = False
        self._round = None                # the running call's round_id

    def _validate_and_merge_parameters(self, parameters):
        if parameters:
            Parameters(parameters).validate(self.parameter_schema)
            parameters = dict(parameters)
        else:
            parameters = {}
        for name in ("clip", "noise_multiplier"):
            if name not in parameters:
                raise InvalidParameterError(f"Parameter {name} is required: a DP aggregator has no default for it")
        clip, nm = parameters["clip"], parameters["noise_multiplier"]
        if not (math.isfinite(clip) and clip > 0.0):
            raise InvalidParameterError(f"Parameter clip must be finite and > 0, got {clip}")
        if not (math.isfinite(nm) and nm >= 0.0):
            raise InvalidParameterError(f"Parameter noise_multiplier must be finite and >= 0, got {nm}")
        seed = parameters.get("seed")
        if seed is not None and (isinstance(seed, bool) or not 0 <= seed < 1 << 64):
            raise InvalidParameterError("Parameter seed must lie in 0 .. 2^64 - 1")
        return parameters

    def _session_seed(self, given):
        """The session's seed: the given one (it may change between rounds; each change is the user's),
        else one drawn once per instance."""
        if given is not None:
            if not self._seed_given:
                logger.warning(f"AGGREGATOR({self.name}): a seed was given: the noise is reproducible, and whoever "
                               "knows the seed can subtract it — the privacy guarantee is void")
            self._seed_given = True
            return int(given)
        if self._seed is None:
            self._seed = secrets.randbits(64)
        return self._seed

    def combine_models(self, helper=None, delete_models=True, parameters=None):
        self._round = self.round_id
        self.round_id += 1
        try:
            return super().combine_models(helper=helper, delete_models=delete_models, parameters=parameters)
        finally:
            self._round = None

    def reduce_round(self, pipe, K, parameters):
        self.coefficients, self.distances, self.excluded, self.trace = None, None, None, None
        self.sigma, self.clipped = None, None
        center, self._center = self._center, None
        model = pipe.dp_clipped_mean(center, parameters["clip"], parameters["noise_multiplier"],
                                     self._session_seed(parameters.get("seed")), self._round)
        self.coefficients, self.distances, self.excluded = pipe.coefficients, pipe.distances, list(pipe.excluded)
        self.trace = list(pipe.trace)
        self.sigma, self.clipped = float(pipe.sigma), pipe.clipped
        logger.info(f"AGGREGATOR({self.name}): K={K}, round {self._round}: sigma {self.sigma}, clipped {self.clipped}, "
                    f"distances {[float(r) for r in self.distances]}, excluded {self.excluded}")
        return model
