"""The exact reference of the long-step (bound-flipping) ratio test of the bounded dual loop (tests/test_dual_long_step_host.py,
tests/test_gpu_dual_long_step.py): ``dual_bounded_lps.BoundedDualReference`` with the rule of ``dual_long_step_kernel`` and of
``dual_pivot_kernel<true, true>`` (relp_amd/csrc/dual.hip) over ``Fraction``, and the cases of the pivot-for-pivot comparison.

The rule at one dual pivot, row p leaving on side s with the violation ``delta``: the candidates ``abar_j < 0`` in the order
``(d_j / |abar_j|, j)``; the walk starts with ``slope = delta`` and passes a candidate with an upper bound while
``slope - ub_j |abar_j| > 0``; a candidate without a bound, the last candidate of all, ``max_flips`` passed ones and the first
candidate that would take the slope to 0 or below end it, and that candidate enters.  The passed ones (``F``) go to their other bound
first: complemented, ``rhs -= ub_j sgn_j a_j``, ``x_B -= Binv Delta``; row p is then violated by exactly the remaining slope, on the
same side, which ``step`` asserts.

Three keywords restate limits of the kernels and default to "none", which is the rule above: ``slope_floor`` (a candidate is passed
while ``slope - ub_j |abar_j| > slope_floor`` and a row counts as violated above it: the kernels' ``harris_delta``), ``slots`` (more
boxed candidates than this in one row: F is empty at that pivot and ``skipped`` counts it) and ``max_flips``.  ``walks`` records per
pivot what the walk saw.  ``HarrisLongStepBoundedDualReference`` chooses the entering column outside F by the two-pass rule.  The
planted rows of tests/dual_planted_rows.py use all of these; the random family below uses none.

The family is that of tests/dual_bounded_lps.py with a bound on every structural variable (``every=1``): the more columns are boxed,
the more often a ratio can be passed.
"""
import functools
from fractions import Fraction

import relp_amd
import dual_bounded_lps as lps
from dual_bounded_lps import BoundedDualReference

MARGIN = lps.MARGIN
DUAL_MAX_FLIPS = 32  # relp_amd/csrc/dual.hpp
EVERY = 1
# (seed, n_cuts, n_tight) per m, chosen on the CPU (``search`` below) so that the reference alone meets ``assert_long_step_conditions``.
# m = 5 has two cases: the walks there are short.
LONG_STEP_CASES = {5: [(6, 3, 1), (11, 3, 1)], 64: [(2017, 4, 6)], 65: [(1012, 4, 4)]}
STEEPEST_CASE = {64: (2000, 4, 6)}  # ... for the steepest-edge subclass (``search`` with it)
MIN_FLIPS = {5: 1, 64: 4, 65: 4}
MIN_FLIPS_IN_ONE_PIVOT = {5: 1, 64: 2, 65: 2}


class LongStepBoundedDualReference(BoundedDualReference):
    """... with the long-step ratio test.  ``flips``: per pivot the columns passed, in the order of the walk; ``slope_margins``: per
    pivot the smallest ``|slope'| / delta`` over its slope decisions (1 where there was none); ``margins``: the lead of the leaving row
    as in the base class, and for the column the smaller of the lead of q over the next candidate and of its lead over the last
    passed candidate's ratio."""

    def __init__(self, form, basis, max_flips=DUAL_MAX_FLIPS, slope_floor=0, slots=None):
        super().__init__(form, basis)
        self.max_flips = max_flips
        self.slope_floor = Fraction(slope_floor)  # the walk passes a candidate while ``behind > slope_floor`` (the kernel: harris_delta)
        self.slots = slots  # more boxed candidates than this in one row: no flip at that pivot, ``skipped`` counts it (None: no limit)
        self.skipped = 0
        self.flips, self.slope_margins = [], []
        self.walks = []  # per pivot: what the walk saw (tests/dual_planted_rows.py reads it)

    def entering(self, candidates, k):
        """The index of the entering candidate among ``candidates[k:]``, the sorted ones outside F: the textbook rule takes the first."""
        return k

    def step(self):
        m, form = self.m, self.form
        rows = []
        for i in range(m):
            v, side = self.violation(i)
            if v > self.slope_floor:  # (dual_leave_kernel: a row is violated above harris_delta; the default 0 is the base class's rule)
                rows.append((self.key(i, v), -self.basis[i], -i, v, side))
        if not rows:
            return relp_amd.STOP_NO_ENTERING
        rows.sort(reverse=True)
        worst = min(v for _, _, _, v, _ in rows)
        self.smallest_violation = worst if self.smallest_violation is None else min(worst, self.smallest_violation)
        p, delta, side = -rows[0][2], rows[0][3], rows[0][4]
        lead_row = 1.0 if len(rows) == 1 else float((rows[0][0] - rows[1][0]) / rows[0][0])
        rho = self.inverse[p]
        d = self.signed_costs()
        candidates = []
        for j in range(self.n):
            if d[j] is None:
                continue
            abar = side * self.sgn(j) * sum((v * rho[i] for i, v in form.device_column(j) if rho[i]), Fraction(0))
            if abar < 0:
                assert d[j] >= 0, "the reference lost dual feasibility"
                candidates.append((d[j] / -abar, j, -abar))
        if not candidates:
            return relp_amd.STOP_UNBOUNDED
        candidates.sort()
        # the walk
        boxed = sum(1 for _, j, _ in candidates if self.ub[j] is not None)
        overflow = self.slots is not None and boxed > self.slots
        self.skipped += int(overflow)
        max_flips = 0 if overflow else self.max_flips
        slope, passed, slope_margin, stopped_behind = delta, [], 1.0, None
        while True:
            _, j, magnitude = candidates[len(passed)]
            if self.ub[j] is None or len(passed) == len(candidates) - 1 or len(passed) >= max_flips:
                break
            behind = slope - self.ub[j] * magnitude
            slope_margin = min(slope_margin, float(abs(behind) / delta))
            if behind <= self.slope_floor:
                stopped_behind = behind
                break
            passed.append(j)
            slope = behind
        k = len(passed)
        entered = self.entering(candidates, k)
        self.walks.append({"p": p, "side": side, "delta": delta, "candidates": list(candidates), "boxed": boxed, "overflow": overflow,
                           "passed": list(passed), "forms": [self.flipped[j] for j in passed], "slope": slope, "stopped_behind": stopped_behind,
                           "entered": entered, "costs": d})
        ratio_q, q, _ = candidates[entered]
        leads = []
        if k + 1 < len(candidates):
            following = candidates[k + 1][0]
            leads.append(0.0 if following == 0 else float((following - ratio_q) / following))
        if passed:
            leads.append(0.0 if ratio_q == 0 else float((ratio_q - candidates[k - 1][0]) / ratio_q))
        lead_column = min(leads, default=1.0)
        # the flips: every column of F to its other bound, in the held form
        if passed:
            change = [Fraction(0)] * m
            for j in passed:
                for i, v in form.device_column(j):
                    change[i] += self.ub[j] * self.sgn(j) * v
                self.flipped[j] ^= 1
                self.pos[j] = -2 if self.flipped[j] else -1
            for i in range(m):
                self.rhs[i] -= change[i]
            for r in range(m):
                self.x[r] -= sum((self.inverse[r][i] * change[i] for i in range(m) if change[i] and self.inverse[r][i]), Fraction(0))
            assert self.violation(p) == (slope, side), "row p is not violated by the remaining slope on the same side"
        # the pivot on (p, q), as in the base class
        alpha_q = [self.sgn(q) * sum((self.inverse[r][i] * v for i, v in form.device_column(q) if self.inverse[r][i]), Fraction(0)) for r in range(m)]
        pivot = alpha_q[p]
        assert side * pivot < 0
        theta = (self.x[p] - (self.xub[p] if side < 0 else 0)) / pivot
        assert theta >= 0
        new_row = [v / pivot if v else v for v in rho]
        for r in range(m):
            if r != p and alpha_q[r]:
                factor = alpha_q[r]
                self.inverse[r] = [a - factor * c if c else a for a, c in zip(self.inverse[r], new_row)]
                self.x[r] -= theta * factor
        self.inverse[p] = new_row
        self.x[p] = theta
        leaving = self.basis[p]
        if side < 0:
            for i, v in form.device_column(leaving):
                self.rhs[i] -= self.xub[p] * self.sgn(leaving) * v
            self.flipped[leaving] ^= 1
        self.pos[leaving] = -3 if self.ub[leaving] == 0 else (-2 if self.flipped[leaving] else -1)
        self.xub[p] = self.ub[q]
        self.pos[q] = p
        self.basis[p] = q
        self.pivots.append((q, p, leaving, side))
        self.margins.append((lead_row, lead_column))
        self.flips.append(passed)
        self.slope_margins.append(slope_margin)
        return None

    def total_flips(self):
        return sum(len(passed) for passed in self.flips)


class HarrisLongStepBoundedDualReference(LongStepBoundedDualReference):
    """... with the two-pass rule of ``dual_row_bounded_kernel``, the rewrite of ``dual_long_step_kernel`` and ``dual_choose_kernel`` with
    ``textbook == 0`` for the entering column: the walk is the same (it orders by ``max(d_j, 0) / |abar_j|``); over the candidates
    outside F with ``abar_j < -tol_pivot``, ``theta_max = min (max(d_j, 0) + tol_dual) / |abar_j|``, and q has the largest
    ``|abar_j|`` among those with ``max(d_j, 0) / |abar_j| <= theta_max``, ties to the lowest column.  ``tol_dual`` / ``tol_pivot``: the
    exact values of the handle's doubles.  ``theta_margins``: per pivot the smallest ``|ratio_j - theta_max| / theta_max`` -- the one
    comparison in which the device rounds ``d_j + tol_dual`` and the reference does not."""

    def __init__(self, form, basis, tol_dual, tol_pivot, **options):
        super().__init__(form, basis, **options)
        self.tol_dual, self.tol_pivot = Fraction(tol_dual), Fraction(tol_pivot)
        self.theta_margins = []

    def entering(self, candidates, k):
        rest = [(index, ratio, j, magnitude) for index, (ratio, j, magnitude) in enumerate(candidates) if index >= k and magnitude > self.tol_pivot]
        theta_max = min((ratio * magnitude + self.tol_dual) / magnitude for _, ratio, _, magnitude in rest)
        self.theta_margins.append(min(float(abs(ratio - theta_max) / theta_max) for _, ratio, _, _ in rest))
        within = [(-magnitude, j, index) for index, ratio, j, magnitude in rest if ratio <= theta_max]
        return min(within)[2]


class SteepestLongStepBoundedDualReference(LongStepBoundedDualReference):
    """... with the steepest-edge key of the leaving row, ``v_i^2 / beta_i`` (flips do not touch the row norms of the inverse)."""

    def key(self, i, v):
        return v * v / sum((a * a for a in self.inverse[i] if a), Fraction(0))


def built(m, seed, n_cuts, n_tight, decimal=False):
    return lps.built(m, seed, n_cuts, n_tight, decimal, EVERY)


def long_step_case(m, which=0):
    return built(m, *LONG_STEP_CASES[m][which])


def long_step_walk(reference):
    """``(reason, facts, bases, dual_feasible)``: ``dual_bounded_lps.walk`` plus the flips and the slope margin, and whether the signed
    costs stayed >= 0 after every pivot."""
    bases, dual_feasible = [], True
    while True:
        reason = reference.step()
        if reason is not None:
            break
        bases.append(reference.formulation_basis())
        dual_feasible = dual_feasible and min(c for c in reference.signed_costs() if c is not None) >= 0
    sides = [side for _, _, _, side in reference.pivots]
    facts = {"pivots": len(reference.pivots), "upper": sides.count(-1), "lower": sides.count(1), "flips": reference.total_flips(),
             "most_flips": max((len(passed) for passed in reference.flips), default=0), "margin": reference.smallest_margin(),
             "slope_margin": min(reference.slope_margins, default=1.0), "smallest_violation": reference.smallest_violation,
             "fixed_cost_ties": reference.fixed_cost_ties}
    return reason, facts, bases, dual_feasible


def assert_long_step_conditions(reference, m, reason, facts, dual_feasible):
    """What a walk must be like for the pivot-for-pivot comparison to say something about the long step (conditions on the reference
    alone, met on the CPU): it ends primal feasible and stays dual feasible, flips, leaves on both sides, and f64 cannot have chosen
    another row, column or flip set at any step."""
    assert reason == relp_amd.STOP_NO_ENTERING and reference.feasible(), reason
    assert dual_feasible, "a signed cost went negative"
    assert facts["flips"] >= MIN_FLIPS[m] and facts["most_flips"] >= MIN_FLIPS_IN_ONE_PIVOT[m], facts
    assert facts["upper"] >= 1 and facts["lower"] >= 1, facts
    assert facts["margin"] >= MARGIN and facts["slope_margin"] >= MARGIN and facts["smallest_violation"] >= MARGIN, facts
    assert facts["fixed_cost_ties"] == 0, facts


@functools.lru_cache(maxsize=None)
def walked(m, which=0, steepest=False):
    """The finished walk of a chosen case, made once per process: ``(reference, reason, facts, bases, dual_feasible, start)`` with the
    reference in its final state, ``reference.pivots`` / ``.flips`` per step and ``bases[k]`` the formulation's basis after step k (``start``: before the first).
    Nobody changes what this returns."""
    case = STEEPEST_CASE[m] if steepest else LONG_STEP_CASES[m][which]
    _, _, child, basis, _, _ = built(m, *case)
    reference = (SteepestLongStepBoundedDualReference if steepest else LongStepBoundedDualReference)(child, basis)
    start = reference.formulation_basis()
    return (reference,) + long_step_walk(reference) + (start,)


@functools.lru_cache(maxsize=None)
def plain_walked(m, which=0, steepest=False):
    """The finished walk of the plain rule over the same case: the reference of tests/dual_bounded_lps.py, and its bases per step."""
    case = STEEPEST_CASE[m] if steepest else LONG_STEP_CASES[m][which]
    _, _, child, basis, _, _ = built(m, *case)
    reference = (lps.SteepestBoundedDualReference if steepest else BoundedDualReference)(child, basis)
    reason, _, bases = lps.walk(reference)
    assert reason == relp_amd.STOP_NO_ENTERING
    return reference, bases


def plain_pivots(child, basis, reference_class=BoundedDualReference):
    reference = reference_class(child, basis)
    assert reference.run() == relp_amd.STOP_NO_ENTERING
    return reference


def search(m, seeds, shapes, reference_class=LongStepBoundedDualReference):
    """The first ``(seed, n_cuts, n_tight)`` whose long-step walk meets the conditions, reaches the oracle's objective and differs from
    the plain rule's walk, and its facts (a tool for choosing ``LONG_STEP_CASES``)."""
    for seed in seeds:
        for n_cuts, n_tight in shapes:
            try:
                _, _, child, basis, _, _ = built(m, seed, n_cuts, n_tight)
                reference = reference_class(child, basis)
                if min(c for c in reference.signed_costs() if c is not None) < 0:
                    continue
                reason, facts, _, dual_feasible = long_step_walk(reference)
                assert_long_step_conditions(reference, m, reason, facts, dual_feasible)
                if reference.objective() != child.solve().objective or reference.pivots == plain_pivots(child, basis).pivots:
                    continue
                return (seed, n_cuts, n_tight), facts
            except (AssertionError, StopIteration):
                continue
    return None, None
