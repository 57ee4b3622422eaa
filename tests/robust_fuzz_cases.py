"""The seeded cases of the robust rules' fuzz (tests/test_gpu_robust_fuzz.py, pinned on the CPU by
tests/test_robust_fuzz_cases_host.py): numpy and the ``*_ref.py`` oracles only — nothing here touches a
device or launches a kernel.

``case(rule, seed)`` draws, deterministically, everything a round of one of the seven robust plug-ins
needs: a random layout (1-7 tensors of rank 0-3, empty tensors, now and then one of 20 000-90 000
elements, in float32 / float64 / float16 / int32 / int64 with one dominant dtype), K, the updates (the
graded-sigma generator the rule tests share, :func:`round_updates` / :func:`center_round_updates`), the
rule's parameters, ``robust.SLICE_BYTES`` (derived from a target slice count of the largest dtype group),
the HBM budget in updates and the bit vector of the mixed route. What ``RobustPipeline._walk_group``'s
index arithmetic depends on is forced on fixed shares of the seeds, not left to chance: K in
{1, 2, 3, 4, 33, 64}, three or more dtype groups, an empty dtype group beside a non-empty one, a scalar,
a full last slice with a member that ends exactly on a slice bound, budgets 0 and K.

The selection rules (krum, multikrum, bulyan) are bit-exact only if the device picks the oracle's
clients, so their cases carry the precondition the rule tests assert (:func:`krum_gaps`,
:func:`bulyan_gap`): in float64, from the oracle's distances alone, every decisive relative score gap is
at least 10 x the largest ``ops.sqdist_rtol`` over the model's tensors. A draw that misses it has its
VALUES redrawn with sub-seed ``attempt`` = 1, 2, 3 — the layout, K, the parameters, the slices and the
budget stay."""
import math
from types import SimpleNamespace

import numpy as np

import bulyan_ref as br
import krum_ref as kr

RULES = ["trimmedmean", "median", "krum", "multikrum", "geomedian", "centeredclip", "bulyan"]
SELECTION_RULES = ("krum", "multikrum", "bulyan")
DTYPES = [np.float32, np.float64, np.float16, np.int32, np.int64]
FORCED_K = [1, 2, 3, 4, 33, 64]
SLICE_TARGETS = [1, 2, 3, 5, 8, 16]
MAX_SLICES = 16                # per dtype group and pass: keeps a round under a second
SLICE_ALIGN = 64               # robust.SLICE_ALIGN (asserted equal by the host test)
K64_ELEMENTS = 20_000          # the model's cap at K = 64
ATTEMPTS = 4
DEFAULT_SEEDS = 24


# ---- values: the generators the rule tests share ---------------------------------------------------
def round_updates(seed, K, f, spec):
    """K updates of the model ``spec`` ([(shape, dtype)]): honest ones are base + sigma_k * noise with
    graded sigma_k = 0.05 * (1 + 0.25 * rank) in shuffled order (so the scores are separated at every
    iteration of a selection); the f hostile ones take honest clients' places as a sign flip, large noise
    and one NaN. Integer tensors hold round(1000 * value). Returns (updates, hostile indices)."""
    rng = np.random.default_rng(seed)
    sigma = 0.05 * (1 + 0.25 * rng.permutation(K))
    hostile = sorted(int(i) for i in rng.choice(K, size=f, replace=False))
    base = [rng.standard_normal(s) for s, _ in spec]
    ups = []
    for k in range(K):
        kind = hostile.index(k) % 3 if k in hostile else None
        u = []
        for b, (s, dt) in zip(base, spec):
            v = b + sigma[k] * rng.standard_normal(s)
            if kind == 0:
                v = -v                                           # sign flip
            elif kind == 1:
                v = b + 5.0 * rng.standard_normal(s)             # large noise
            if np.dtype(dt).kind == "i":
                v = np.round(1000.0 * v)
            v = np.asarray(v, dtype=dt).reshape(s)
            if kind == 2 and np.dtype(dt).kind == "f" and v.size:
                v.reshape(-1)[v.size // 2] = np.nan              # one NaN
            u.append(v)
        ups.append(u)
    return ups, hostile


def center_round_updates(seed, K, f, spec):
    """K updates of the model ``spec`` and the global model they started from: the global model is
    ``base``; honest updates are base + shift + sigma_k * noise with a common shift of scale 0.1 and graded
    sigma_k = 0.05 * (1 + 0.25 * rank) in shuffled order; the f hostile ones take honest clients' places as
    a x10 sign flip of the step, noise of scale 5 and one NaN. Integer tensors hold round(value). Returns
    (updates, hostile indices, global model)."""
    rng = np.random.default_rng(seed)
    sigma = 0.05 * (1 + 0.25 * rng.permutation(K))
    hostile = sorted(int(i) for i in rng.choice(K, size=f, replace=False))
    base = [rng.standard_normal(s) for s, _ in spec]
    shift = [0.1 * rng.standard_normal(s) for s, _ in spec]

    def store(v, s, dt):
        if np.dtype(dt).kind == "i":
            v = np.round(v)
        return np.asarray(v, dtype=dt).reshape(s)

    center = [store(b, s, dt) for b, (s, dt) in zip(base, spec)]
    ups = []
    for k in range(K):
        kind = hostile.index(k) % 3 if k in hostile else None
        u = []
        for b, sh, (s, dt) in zip(base, shift, spec):
            step = sh + sigma[k] * rng.standard_normal(s)
            if kind == 0:
                step = -10.0 * step                              # x10 sign flip of the step
            elif kind == 1:
                step = 5.0 * rng.standard_normal(s)              # large noise
            v = store(b + step, s, dt)
            if kind == 2 and np.dtype(dt).kind == "f" and v.size:
                v.reshape(-1)[v.size // 2] = np.nan              # one NaN
            u.append(v)
        ups.append(u)
    return ups, hostile, center


def sprinkle_specials(rng, ups):
    """+-0, +-inf and NaN at random places of the float tensors (test_gpu_robust._random's shares): the
    order statistics' total order is exercised, the distance rules never see these."""
    for u in ups:
        for a in u:
            if a.dtype.kind == "f" and a.size:
                pick = rng.random(a.shape)
                for lo, hi, v in ((0.00, 0.04, 0.0), (0.04, 0.08, -0.0), (0.08, 0.10, np.inf), (0.10, 0.12, -np.inf),
                                  (0.12, 0.14, np.nan)):
                    a[(pick >= lo) & (pick < hi)] = v


# ---- the selection precondition ---------------------------------------------------------------------
def selection_bound(ups):
    """10 x the largest ``ops.sqdist_rtol`` over the model's tensors: what a decisive score gap must reach."""
    from fedn_amd import ops
    return 10 * max(ops.sqdist_rtol(np.asarray(a).dtype, np.asarray(a).size) for a in ups[0])


def _mutual(D, i, j, si, sj):
    """Two clients whose scores are the very same entry of the exactly symmetric D: mutual nearest
    neighbours at nn = 1. Equal on the device whatever its rounding, broken by the FIFO index in both."""
    return si == sj == D[i][j] and math.isfinite(si)


def _gap(lo, hi):
    return (hi - lo) / hi if math.isfinite(hi) else math.inf


def krum_gaps(D, f, m):
    """The decisive relative score gaps of Krum (``m = 1``) / Multi-Krum (``m = K - f``) on the oracle's
    distances ``D``: between the best and the second-best client and between the m-th and the (m+1)-th, in
    float64. An exact structural tie (see :func:`_mutual`: K <= 3, where nn = 1) is no near-tie and is
    stepped over: the gap taken is the one to the client after the tied pair, if there is one."""
    D = np.asarray(D, dtype=np.float64)
    K = D.shape[0]
    sc = kr.scores(D.tolist(), f)
    order = sorted(range(K), key=lambda i: sc[i])              # (stable: equal scores in FIFO order)
    nn = max(K - f - 2, min(1, K - 1))
    gaps = []
    for lo in sorted({0, m - 1}):
        if lo + 1 >= K or not math.isfinite(sc[order[lo]]):
            continue
        nxt = lo + 1
        if nn == 1 and _mutual(D, order[lo], order[nxt], sc[order[lo]], sc[order[nxt]]):
            nxt += 1
        if nxt < K:
            gaps.append(_gap(sc[order[lo]], sc[order[nxt]]))
    return gaps


def bulyan_gap(D, f):
    """The smallest decisive relative score gap of Bulyan's ``K - 2f`` picks on the oracle's distances
    ``D``: at EVERY iteration the gap between the smallest score and the next one, in float64. The exact
    structural tie of two mutual nearest neighbours at nn = 1 (see :func:`_mutual`) is stepped over — with
    two clients left there is nobody after the pair and the pick decides nothing."""
    D = np.asarray(D, dtype=np.float64)
    left = list(range(D.shape[0]))
    worst = math.inf
    for _ in range(D.shape[0] - 2 * f):
        n = len(left)
        sc = kr.scores(D[np.ix_(left, left)].tolist(), f)
        order = sorted(range(n), key=lambda i: sc[i])
        nxt = 1
        if n >= 2 and max(n - f - 2, 1) == 1 and _mutual(D, left[order[0]], left[order[1]], sc[order[0]], sc[order[1]]):
            nxt = 2
        if nxt < n and math.isfinite(sc[order[nxt]]):
            worst = min(worst, _gap(sc[order[0]], sc[order[nxt]]))
        left.pop(order[0])
    return worst


# ---- layout -------------------------------------------------------------------------------------------
def _size(shape):
    return int(np.prod(shape, dtype=np.int64))


def _draw_layout(rng, seed, K):
    """[(shape, dtype)] as test_gpu_fuzz._layout draws it, over the five dtypes, with the forced shares."""
    side = 13 if K == 64 else 41
    big_left = 1 if K == 64 else 7
    shapes = []
    for _ in range(int(rng.integers(1, 8))):
        r = rng.random()
        if r < 0.1:
            shapes.append(())                                   # a scalar tensor
        elif r < 0.2:
            shapes.append((0,) if rng.random() < 0.5 else (3, 0))   # empty
        elif r < 0.3 and big_left:
            big_left -= 1                                       # crosses several tiles
            shapes.append((int(rng.integers(3_000, 8_000) if K == 64 else rng.integers(20_000, 90_000)),))
        else:
            shapes.append(tuple(int(rng.integers(1, side)) for _ in range(int(rng.integers(1, 4)))))
    one = DTYPES[seed % 5]                                      # the dominant dtype: every dtype leads some seeds
    dtypes = [one if rng.random() >= 0.4 else DTYPES[int(rng.integers(0, 5))] for _ in shapes]
    if seed % 8 == 7 and () not in shapes:                      # a scalar
        at = int(rng.integers(0, len(shapes) + 1))
        shapes.insert(at, ())
        dtypes.insert(at, one)
    if not any(_size(s) for s in shapes):                       # at least one tensor is non-empty
        shapes.append((int(rng.integers(1, side)),))
        dtypes.append(one)
    if seed % 6 == 2:                                           # three or more dtype groups
        while len({d for s, d in zip(shapes, dtypes) if _size(s)}) < 3:
            new = [d for d in DTYPES if d not in {d2 for s, d2 in zip(shapes, dtypes) if _size(s)}]
            shapes.append((int(rng.integers(1, side)),))
            dtypes.append(new[int(rng.integers(0, len(new)))])
    if seed % 8 == 3:                                           # a dtype group of empty tensors only
        new = [d for d in DTYPES if d not in dtypes]
        if new:
            at = int(rng.integers(0, len(shapes) + 1))
            shapes.insert(at, (0,) if rng.random() < 0.5 else (3, 0))
            dtypes.insert(at, new[int(rng.integers(0, len(new)))])
    return [(s, d) for s, d in zip(shapes, dtypes)]


def groups_of(spec):
    """The dtype groups of a model in first-appearance order (layout.Layout's rule): ``{dtype: [(tensor
    index, element offset, elements)]}``."""
    groups = {}
    for i, (s, d) in enumerate(spec):
        g = groups.setdefault(np.dtype(d), [])
        g.append((i, sum(n for _, _, n in g), _size(s)))
    return groups


def slice_plan(spec, slice_bytes):
    """``{dtype: (step, slices)}`` of every non-empty dtype group when updates sit on the host:
    ``_walk_group``'s rule, written out again."""
    plan = {}
    for dt, members in groups_of(spec).items():
        n = sum(m[2] for m in members)
        if n:
            step = min(n, max(SLICE_ALIGN, slice_bytes // dt.itemsize // SLICE_ALIGN * SLICE_ALIGN))
            plan[dt] = (step, -(-n // step))
    return plan


def _largest(spec):
    """(dtype, elements) of the dtype group with the most bytes."""
    sizes = {dt: sum(m[2] for m in ms) for dt, ms in groups_of(spec).items()}
    dt = max(sizes, key=lambda d: (sizes[d] * d.itemsize, sizes[d]))
    return dt, sizes[dt]


def _slice_bytes_for(spec, target):
    """SLICE_BYTES at which the largest group takes exactly ``target`` slices of SLICE_ALIGN-multiple
    length and no group more than MAX_SLICES — for the largest target <= ``target`` at which that is
    possible (1 always is)."""
    dt, n = _largest(spec)
    for s in sorted((t for t in SLICE_TARGETS if t <= target), reverse=True):
        step = -(-(-(-n // s)) // SLICE_ALIGN) * SLICE_ALIGN
        sb = step * dt.itemsize
        plan = slice_plan(spec, sb)
        if plan[dt][1] == s and max(c for _, c in plan.values()) <= MAX_SLICES:
            return sb, s
    raise AssertionError("one slice is always possible")


def _full_and_aligned(rng, spec, target):
    """Rebuild ``spec`` so that the largest group's first member ends exactly on the first slice bound and
    its last slice is full: a tensor of one step leads the model, a filler ends it. Returns (spec,
    SLICE_BYTES, slices)."""
    dt, n = _largest(spec)
    s = max(2, min(target, 8))
    step = -(-(-(-n // s)) // SLICE_ALIGN) * SLICE_ALIGN
    fill = s * step - n
    spec = [((step,), dt.type)] + spec + ([((fill,), dt.type)] if fill else [])
    sb = step * dt.itemsize
    plan = slice_plan(spec, sb)
    assert plan[np.dtype(dt)] == (step, s + 1) and max(c for _, c in plan.values()) <= MAX_SLICES, (plan, step, s)
    return spec, sb, s + 1


# ---- the case -----------------------------------------------------------------------------------------
def out_dtype(dt):
    from fedn_amd import ops
    return np.dtype(ops.numpy_dtype(ops.order_mean_dtype(ops.torch_dtype(np.dtype(dt)))))


def trim_count(fraction, K):
    return max(0, min(math.floor(fraction * K), (K - 1) // 2))


def _values(c, attempt):
    """The updates of case ``c`` at sub-seed ``attempt`` (and the global model of centred clipping)."""
    vseed = 7_000_000 + ((RULES.index(c.rule) * 1_000_000 + c.seed) * ATTEMPTS + attempt)
    center = None
    if c.rule == "centeredclip":
        ups, hostile, center = center_round_updates(vseed, c.K, c.f, c.spec)
        rng = np.random.default_rng([vseed, 1])
        center = [a if rng.random() < 0.5 else a.astype(out_dtype(a.dtype)) for a in center]
    else:
        ups, hostile = round_updates(vseed, c.K, c.f, c.spec)
        if c.rule in ("trimmedmean", "median"):
            sprinkle_specials(np.random.default_rng([vseed, 1]), ups)
    return ups, hostile, center


def precondition(rule, ups, f):
    """(holds, decisive gaps, bound, the oracle's D) of a selection rule's round."""
    D = kr.model_distances(ups)
    bound = selection_bound(ups)
    K = len(ups)
    if rule == "bulyan":
        gaps = [bulyan_gap(D, f)]
    else:
        gaps = krum_gaps(D, f, 1 if rule == "krum" else K - f)
    return all(g >= bound for g in gaps), gaps, bound, D


def case(rule, seed):
    """Everything one fuzz round of ``rule`` needs, as a namespace: ``spec`` [(shape, dtype)], ``K``,
    ``ups``, ``hostile``, ``center`` (centred clipping, else None), ``parameters`` (the plug-in's), ``f`` /
    ``trim`` / ``iterations`` / ``nu`` / ``tau`` as they apply, ``slice_bytes`` and ``slices`` (of the largest
    group), ``budget_updates`` (j: the budget is j x ``Layout.of(ups[0]).nbytes``), ``staged_bits`` (the mixed
    route: True = staged on arrival), ``attempt`` (the sub-seed the values resolved at) and, for the
    selection rules, ``D`` (the oracle's distances), ``gaps`` and ``bound``."""
    rng = np.random.default_rng([RULES.index(rule), seed, 20_260])
    c = SimpleNamespace(rule=rule, seed=seed)
    c.K = K = FORCED_K[(seed // 4) % 6] if seed % 4 == 1 else int(rng.integers(1, 25))
    spec = _draw_layout(rng, seed, K)
    target = SLICE_TARGETS[(seed + seed // 6) % 6]
    if seed % 6 == 4:
        spec, c.slice_bytes, c.slices = _full_and_aligned(rng, spec, target)
    else:
        c.slice_bytes, c.slices = _slice_bytes_for(spec, target)
        if rng.random() < 0.5 and max(sum(m[2] for m in ms) for ms in groups_of(spec).values()) <= 1024:
            c.slice_bytes = SLICE_ALIGN                         # the minimum: every step is SLICE_ALIGN
            c.slices = slice_plan(spec, c.slice_bytes)[_largest(spec)[0]][1]
    c.spec = spec
    if K == 64:
        assert sum(_size(s) for s, _ in spec) <= K64_ELEMENTS, spec
    c.budget_updates = 0 if seed % 5 == 0 else K if seed % 5 == 3 else int(rng.integers(0, K + 1))
    bits = rng.random(K) < 0.5
    if K >= 2 and bits.all() == bits.any():                     # both kinds wherever there are two updates
        bits[int(rng.integers(0, K))] ^= True
    c.staged_bits = [bool(b) for b in bits]
    c.f, c.trim, c.iterations, c.nu, c.tau = 0, None, None, None, None
    if rule == "trimmedmean":
        fraction = float(rng.uniform(0.0, 0.5))
        c.parameters, c.trim = {"trim_fraction": fraction}, trim_count(fraction, K)
        c.f = kr.byzantine_count(fraction, K)
    elif rule == "median":
        c.parameters, c.trim = None, (K - 1) // 2
        c.f = kr.byzantine_count(float(rng.uniform(0.0, 0.5)), K)
    elif rule in ("krum", "multikrum"):
        fraction = float(rng.uniform(0.0, 0.5))
        c.parameters, c.f = {"byzantine_fraction": fraction}, kr.byzantine_count(fraction, K)
    elif rule == "bulyan":
        fraction = float(rng.uniform(0.0, 0.25))
        c.parameters, c.f = {"byzantine_fraction": fraction}, br.byzantine_count(fraction, K)
    elif rule == "geomedian":
        c.iterations, c.nu = int(rng.integers(0, 5)), float(10 ** rng.uniform(-8, -2))
        c.parameters = {"iterations": c.iterations, "nu": c.nu}
        c.f = kr.byzantine_count(float(rng.uniform(0.0, 0.5)), K)
    else:
        c.iterations = int(rng.integers(0, 5))
        c.tau = float(rng.uniform(0.05, 1.0) * math.sqrt(sum(_size(s) for s, _ in spec)))
        c.parameters = {"iterations": c.iterations, "tau": c.tau}
        c.f = kr.byzantine_count(float(rng.uniform(0.0, 0.5)), K)
    c.D, c.gaps, c.bound = None, None, None
    for attempt in range(ATTEMPTS):
        c.ups, c.hostile, c.center = _values(c, attempt)
        c.attempt = attempt
        if rule not in SELECTION_RULES:
            return c
        ok, c.gaps, c.bound, c.D = precondition(rule, c.ups, c.f)
        if ok:
            return c
    raise AssertionError(f"{rule} seed {seed}: no values within {ATTEMPTS} attempts meet the selection "
                         f"precondition (gaps {c.gaps}, needed {c.bound:.3e})")


def describe(c):
    return (f"{c.rule} seed {c.seed} (attempt {c.attempt}) K={c.K} f={c.f} spec "
            f"{[(s, np.dtype(d).name) for s, d in c.spec]} SLICE_BYTES={c.slice_bytes} ({c.slices} slices) "
            f"budget {c.budget_updates} updates")
