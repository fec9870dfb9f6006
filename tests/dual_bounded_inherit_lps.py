"""Inputs of the tests of the inherited start on implicit bounds (tests/test_dual_bounded_inherit_host.py,
tests/test_gpu_dual_bounded_inherit.py), on top of tests/dual_bounded_lps.py: the second generation, and the pure branch.

Two generations.  The first generation is ``dual_bounded_lps.walk_case(FIRST_M)`` walked to its end; the handle that walked it is the
parent of the second.  The grandchild is what ``BoundedCase.child`` makes of the first-generation child, from the basis that handle
reports and the vertex of the walk's exact reference: cuts, tightened bounds, one new bound (``Generation``).  After the walk the
handle holds some basic columns complemented, which ``place_basis`` never does for the grandchild (the sign of the inherited row).
Its positions are another matter: ``Solver.basis()`` lists the basis by position and ``place_basis`` keeps a column on its row, so a
caller that passes the list on as it is never moves a column.  A caller that keeps a basis as a set does: ``by_column`` orders the
constraint rows' entries by column number, which is still a basis of the formulation, and ``place_basis`` then assigns other
positions than the walk left (the map of the inherited rows).  ``GRANDCHILD`` = (seed, cuts, tightened bounds) was chosen on the CPU
with ``search`` so that the exact reference alone meets ``assert_walk_conditions`` on that basis.
"""
import functools
from fractions import Fraction

import dual_bounded_lps as lps

FIRST_M = 64
GRANDCHILD = (3016, 1, 3)


class Generation(lps.BoundedCase):
    """A ``BoundedCase`` whose parent is a formulation that exists already (a first-generation child)."""

    def __init__(self, parent, seed, n_cuts, n_tight):
        self.m, self.seed, self.n_cuts, self.n_tight = parent.m, seed, n_cuts, n_tight
        self.parent = parent


def by_column(form, basis):
    """``basis`` (of the formulation ``form``) with the entries of the constraint rows in ascending column order."""
    basis = [int(c) for c in basis]
    return sorted(basis[:form.m]) + basis[form.m:]


@functools.lru_cache(maxsize=None)
def first_generation(m=FIRST_M):
    """``(child formulation, its start basis, the exact reference walked to its end)``."""
    _, _, child, basis, _, _ = lps.walk_case(m)
    reference = lps.BoundedDualReference(child, basis)
    assert reference.run() == lps.relp_amd.STOP_NO_ENTERING
    return child, basis, reference


def grandchild(child, reported_basis, vertex, shape=GRANDCHILD):
    """``(formulation, basis, cuts, branches)`` of the second generation: ``reported_basis`` is the first generation's final basis of
    its formulation (``Solver.basis()`` or ``reference.formulation_basis()``), ``vertex`` its structural variables' values."""
    seed, n_cuts, n_tight = shape
    return Generation(child, seed, n_cuts, n_tight).child(by_column(child, reported_basis), vertex)


def complemented_basic(reference):
    return sum(1 for j in reference.basis if reference.flipped[j])


def moved_positions(first_reference, second_reference):
    """Positions of the first generation's rows at which ``place_basis`` puts another column than the walk left there."""
    return sum(1 for i in range(first_reference.m) if first_reference.basis[i] != second_reference.basis[i])


def pure_branch(m, n_tight=8, decimal=False, seed=None):
    """``(case, optimum, child, basis, branches)``: k = 0, only bounds tightened (``n_tight`` bounded variables that are positive at the parent's
    vertex; no bound row is added, so the formulation keeps its rows and columns and the basis is the parent's as it is)."""
    seed = lps.WALK_CASES[m][0] if seed is None else seed
    case, optimum, _, _, _, _ = lps.built(m, seed, 0, n_tight, decimal)
    child, basis, branches = tightened_only(case, optimum.basis, {j: v for j, v in optimum.solution if j < case.parent.ns})
    return case, optimum, child, basis, branches


def tightened_only(case, basis, vertex):
    """``(child, basis, branches)`` of ``case`` (``n_cuts == 0``) at ``basis`` / ``vertex`` with the bounds of ``case.branches`` that
    tighten a bound the parent has: no row and no column is added."""
    vertex = {int(j): Fraction(v) for j, v in vertex.items()}
    branches = {j: u for j, u in case.branches(vertex).items() if case.parent.upper[j] is not None}
    child, basis, cuts, branches = case.child(basis, vertex, branches=branches)
    assert child.m == case.parent.m and child.rows == case.parent.rows and not cuts and branches
    return child, basis, branches


def search(seeds, shapes, m=FIRST_M):
    """The first ``(seed, n_cuts, n_tight)`` of a grandchild whose walk meets the conditions (a tool for choosing ``GRANDCHILD``)."""
    child, _, first = first_generation(m)
    for seed in seeds:
        for n_cuts, n_tight in shapes:
            try:
                form, basis, _, _ = grandchild(child, first.formulation_basis(), first.solution(), (seed, n_cuts, n_tight))
                reference = lps.BoundedDualReference(form, basis)
                if min(d for d in reference.signed_costs() if d is not None) < 0 or moved_positions(first, reference) < 1:
                    continue
                reason, facts, _ = lps.walk(reference)
                lps.assert_walk_conditions(reference, m, reason, facts)
                if reference.objective() != form.solve().objective:
                    continue
                return (seed, n_cuts, n_tight), facts
            except (AssertionError, StopIteration):
                continue
    return None, None
