"""The robust fuzz's case generator (tests/robust_fuzz_cases.py) on the CPU: deterministic, every default
seed resolves its selection precondition within four attempts (three quarters of them at the first), the
default seed range covers what ``RobustPipeline._walk_group``'s index arithmetic depends on, no group takes
more than 16 slices, and the product's host rules give the oracle's selection on the oracle's distances."""
import functools

import numpy as np
import pytest

import bulyan_ref as br
import krum_ref as kr
import robust_fuzz_cases as fc

SEEDS = range(fc.DEFAULT_SEEDS)


@functools.lru_cache(maxsize=None)
def _case(rule, seed):
    return fc.case(rule, seed)


def _blob(c):
    parts = [repr((c.rule, c.seed, c.K, c.f, c.trim, c.iterations, c.nu, c.tau, c.parameters, c.slice_bytes, c.slices,
                   c.budget_updates, c.staged_bits, c.attempt, c.hostile,
                   [(s, np.dtype(d).str) for s, d in c.spec])).encode()]
    for u in c.ups + ([c.center] if c.center is not None else []):
        for a in u:
            parts.append(f"{a.dtype.str}{a.shape}".encode() + np.ascontiguousarray(a).tobytes())
    if c.D is not None:
        parts.append(np.ascontiguousarray(c.D).tobytes())
    return b"".join(parts)


def _oracle_selection(c):
    if c.rule == "bulyan":
        return br.select(c.D.tolist(), c.f)[0]
    return kr.select(c.D.tolist(), c.f, 1 if c.rule == "krum" else c.K - c.f)


def _facts(c):
    """What of the coverage list the case shows."""
    got = set()
    groups = fc.groups_of(c.spec)
    nonempty = [dt for dt, ms in groups.items() if sum(m[2] for m in ms)]
    got |= {("dtype", np.dtype(d).name) for _, d in c.spec}
    if any(s == () for s, _ in c.spec):
        got.add("scalar")
    if any(fc._size(s) == 0 for s, _ in c.spec):
        got.add("empty tensor")
    if len(nonempty) < len(groups):
        got.add("empty group beside a non-empty one")
    if len(nonempty) >= 3:
        got.add("three groups")
    got.add(("K", c.K))
    j, K = c.budget_updates, c.K
    got.add("budget 0" if j == 0 else "budget K" if j == K else "budget between")
    if j < K:                                                   # the host route walks slices
        got.add(("slices", min(c.slices, 5)))
        for dt, (step, count) in fc.slice_plan(c.spec, c.slice_bytes).items():
            n = sum(m[2] for m in groups[dt])
            if count >= 2:
                got.add("full last slice" if n % step == 0 else "ragged last slice")
            for _, off, size in groups[dt]:
                if size and any(off < b < off + size for b in range(step, n, step)):
                    got.add("straddling member")
                if size and (off + size) % step == 0 and off + size < n:
                    got.add("bound-aligned member")
        if c.rule in fc.SELECTION_RULES:
            ring2 = sum(1 for k in _oracle_selection(c) if k >= j)
            if 1 <= ring2 < K - j:
                got.add("smaller second ring")
    return got


WANTED = ([("dtype", np.dtype(d).name) for d in fc.DTYPES] + [("K", k) for k in fc.FORCED_K] +
          [("slices", 1), ("slices", 2), ("slices", 5)] +
          ["scalar", "empty tensor", "empty group beside a non-empty one", "three groups", "budget 0", "budget K",
           "budget between", "full last slice", "ragged last slice", "straddling member", "bound-aligned member"])


def test_the_generator_mirrors_the_product():
    from fedn_amd import robust
    assert fc.SLICE_ALIGN == robust.SLICE_ALIGN
    for K in range(1, 65):
        for frac in (0.0, 0.1, 0.24, 0.26, 0.3333, 0.49):
            assert fc.trim_count(frac, K) == robust.trim_count(frac, K)
            assert kr.byzantine_count(frac, K) == robust.krum_f(frac, K)
            assert br.byzantine_count(frac, K) == robust.bulyan_f(frac, K)


@pytest.mark.parametrize("rule", fc.RULES)
def test_case_is_deterministic(rule):
    for seed in (0, 1, 4, 7, 21):
        assert _blob(fc.case(rule, seed)) == _blob(fc.case(rule, seed)), (rule, seed)


@pytest.mark.parametrize("rule", fc.RULES)
def test_layout_matches_the_products(rule):
    """``groups_of`` / ``slice_plan`` are the product's layout and slicing rules, written out again."""
    from fedn_amd import robust
    from fedn_amd.layout import Layout
    for seed in SEEDS:
        c = _case(rule, seed)
        lay = Layout.of(c.ups[0])
        groups = fc.groups_of(c.spec)
        assert list(groups) == lay.groups
        for dt in lay.groups:
            assert [(i, off) for i, off, _ in groups[dt]] == lay.members[dt]
            n = lay.group_elems[dt]
            assert n == sum(m[2] for m in groups[dt])
            if n:
                step = min(n, max(robust.SLICE_ALIGN, c.slice_bytes // dt.itemsize // robust.SLICE_ALIGN * robust.SLICE_ALIGN))
                assert fc.slice_plan(c.spec, c.slice_bytes)[dt] == (step, len(range(0, n, step)))


@pytest.mark.parametrize("rule", fc.RULES)
def test_every_seed_resolves_and_the_range_covers(rule):
    first, seen = 0, set()
    for seed in SEEDS:
        c = _case(rule, seed)                                   # (raises when four attempts do not resolve)
        assert 0 <= c.attempt < fc.ATTEMPTS
        first += c.attempt == 0
        plan = fc.slice_plan(c.spec, c.slice_bytes)
        assert max(count for _, count in plan.values()) <= fc.MAX_SLICES, fc.describe(c)
        assert plan[fc._largest(c.spec)[0]][1] == c.slices, fc.describe(c)
        assert all(step % fc.SLICE_ALIGN == 0 or count == 1 for step, count in plan.values()), fc.describe(c)
        assert any(fc._size(s) for s, _ in c.spec) and 1 <= len(c.spec)
        assert len(c.ups) == c.K and len(c.hostile) == c.f and 0 <= c.budget_updates <= c.K
        if c.K == 64:
            assert sum(fc._size(s) for s, _ in c.spec) <= fc.K64_ELEMENTS
        if c.K >= 2:
            assert any(c.staged_bits) and not all(c.staged_bits), "the mixed route holds both kinds"
        if rule == "centeredclip":
            for a, g in zip(c.ups[0], c.center):
                assert g.shape == a.shape and g.dtype in (a.dtype, fc.out_dtype(a.dtype))
        seen |= _facts(c)
    share = first / len(SEEDS)
    print(f"{rule}: {first} of {len(SEEDS)} seeds resolve at attempt 0 (share {share:.3f})")
    assert share >= 0.75, f"{rule}: only {first} of {len(SEEDS)} seeds resolve at the first attempt"
    wanted = WANTED + (["smaller second ring"] if rule in fc.SELECTION_RULES else [])
    missing = [w for w in wanted if w not in seen]
    assert not missing, f"{rule}: the default seeds never show {missing}"


@pytest.mark.parametrize("rule", fc.SELECTION_RULES)
def test_host_rules_select_what_the_oracle_selects(rule):
    """``robust.krum_select`` / ``robust.bulyan_select`` on the oracle's D against ``kr.select`` /
    ``br.select``, on every default case; and the precondition holds as the case says."""
    from fedn_amd import robust
    for seed in SEEDS:
        c = _case(rule, seed)
        assert all(g >= c.bound for g in c.gaps), fc.describe(c)
        if rule == "bulyan":
            sel, order, scores = robust.bulyan_select(c.D, c.f)
            wsel, worder, wscores = br.select(c.D.tolist(), c.f)
            assert (sel, order) == (wsel, worder), fc.describe(c)
            assert scores == wscores, fc.describe(c)
        else:
            m = 1 if rule == "krum" else c.K - c.f
            assert robust.krum_select(c.D, c.f, m) == kr.select(c.D.tolist(), c.f, m), fc.describe(c)
            assert robust.krum_scores(c.D, c.f).tolist() == kr.scores(c.D.tolist(), c.f), fc.describe(c)


def test_structural_ties_are_stepped_over():
    """K = 3 (every client's score is its nearest neighbour's distance: the mutual pair ties exactly) and
    Bulyan's last two picks: no gap of 0 is reported for them, a near-tie still is."""
    D = np.array([[0.0, 1.0, 5.0], [1.0, 0.0, 4.0], [5.0, 4.0, 0.0]])
    assert fc.krum_gaps(D, 0, 1) == [(4.0 - 1.0) / 4.0]
    assert fc.krum_gaps(D, 0, 3) == [(4.0 - 1.0) / 4.0]
    assert fc.krum_gaps(np.array([[0.0, 2.0], [2.0, 0.0]]), 0, 1) == []
    assert fc.bulyan_gap(np.array([[0.0, 2.0], [2.0, 0.0]]), 0) == np.inf
    assert fc.bulyan_gap(D, 0) == (4.0 - 1.0) / 4.0
    near = np.array([[0.0, 1.0, 1.0 + 1e-9], [1.0, 0.0, 4.0], [1.0 + 1e-9, 4.0, 0.0]])
    assert fc.krum_gaps(near, 0, 1)[0] < 1e-8                    # 0's and 1's scores are both D[0][1]; 2's is a near-tie
