"""Inputs of the objective-cutoff tests of the dual simplex (tests/test_dual_cutoff_host.py, tests/test_gpu_dual_cutoff.py): two LPs
small enough to walk by hand, the walk cases of tests/dual_lps.py and tests/dual_bounded_lps.py with the parent's optimum taken from the
oracle, and the choice of cutoffs along a reference walk.

The hand LP is minimise ``2x + 3y`` with ``x <= 1`` and ``x + y >= 4``; ``x <= 1`` is a row of the plain model and a bound of the
bounded one.  From the slack basis both walks make two dual pivots and the objective goes 0, 8, 11.

A cutoff is placed in the middle of the rise of the objective at one pivot of the reference walk, and only at a pivot where that rise is
at least ``MIN_RISE`` relative to the objectives on either side: the f64 objective of the device is then on the same side of the cutoff
as the exact one after every pivot, so the device stops after exactly that many pivots, on the reference's basis.
"""
import functools
from fractions import Fraction

import relp_amd
from relp_oracle.solve import FiniteOptimum, solve_relaxation_full_basis
import dual_bounded_lps
import dual_lps
import sparse_lps

MIN_RISE = 1e-6
HAND_OBJECTIVES = [0, 8, 11]
HAND_PLAIN_BASES = [[2, 3], [2, 0], [1, 0]]
HAND_BOUNDED_BASES = [[2, 3], [0, 3], [1, 0]]


def hand_plain():
    """``(model, basis)``: 4 provider columns -- x, y, the slack of row 0, the surplus of row 1 --, the slack basis."""
    model = relp_amd.Model.from_general_form([[(0, 1), (1, 1)], [(1, 1)]], ["Less", "Greater"], [1, 4], [(2, 0, None), (3, 0, None)])
    assert model.nr_columns == 4 and model.right_hand_side_exact() == [1, 4]
    return model, [2, 3]


def hand_bounded():
    """``(formulation, basis)``: the constraint row, then the bound row of x; columns x, y, the surplus of row 0, the bound slack."""
    form = dual_bounded_lps.Formulation([[(0, 1)], [(0, 1)]], [4], [2, 3], [1, None], n_greater=1)
    assert form.rows == 2 and form.bound_row == {0: 1} and form.bound_slack == {0: 3}
    return form, [2, 3]


@functools.lru_cache(maxsize=None)
def plain_walk_case(m):
    """``(child model, basis)`` of ``dual_lps.WALK_CASES[m]``, the parent's optimal basis and vertex taken from the oracle as
    tests/test_dual_host.py takes them."""
    seed, n_cuts = dual_lps.WALK_CASES[m]
    case = dual_lps.cut_case(m, dual_lps.MIXED, seed, n_cuts)
    parent = solve_relaxation_full_basis(sparse_lps.Provider(case.parent))
    assert isinstance(parent, FiniteOptimum)
    child, basis, _ = case.child(parent.basis, {j: v for j, v in parent.solution if j < case.n_structural})
    return child, basis


def bounded_walk_case(m):
    """``(child formulation, basis)`` of ``dual_bounded_lps.WALK_CASES[m]``."""
    _, _, child, basis, _, _ = dual_bounded_lps.walk_case(m)
    return child, basis


def plain_pi(reference):
    """``c_B B^-1`` of a ``DualReference``, by row."""
    m = reference.m
    return [sum((reference.cost[reference.basis[k]] * reference.inverse[k][i] for k in range(m) if reference.inverse[k][i]), Fraction(0))
            for i in range(m)]


def state_of(reference):
    """What a test compares the device with at the basis ``reference`` stands on: its objective, its basis as ``Solver.basis()`` reports
    it (a ``BoundedDualReference``: the basis of the formulation) and ``c_B B^-1`` over the rows its basis spans."""
    bounded = isinstance(reference, dual_bounded_lps.BoundedDualReference)
    return {"objective": reference.objective(), "basis": reference.formulation_basis() if bounded else list(reference.basis),
            "pi": reference.pi() if bounded else plain_pi(reference)}


def walk_with_cutoffs(reference):
    """Walks ``reference`` (fresh) to its end.  Returns ``(states, usable)``: ``states[k]`` is ``state_of`` after k pivots, ``usable`` the
    list of ``(k, cutoff)`` over the pivots k >= 1 at which the objective rose by at least ``MIN_RISE`` relative to
    ``max(|before|, |after|, 1)``, ``cutoff`` the midpoint of that rise rounded to a double."""
    states = [state_of(reference)]
    while reference.step() is None:
        states.append(state_of(reference))
    usable = []
    for k in range(1, len(states)):
        before, after = states[k - 1]["objective"], states[k]["objective"]
        assert after >= before, "the dual objective fell"
        if after - before >= Fraction(MIN_RISE) * max(abs(before), abs(after), 1):
            cutoff = float((before + after) / 2)
            assert before < Fraction(cutoff) <= after
            usable.append((k, cutoff))
    return states, usable


def first_middle_last(usable):
    """The three cutoffs a walk is tested at."""
    assert len(usable) >= 3
    return [usable[0], usable[len(usable) // 2], usable[-1]]


def closed_form_value(form, y):
    """``(y over the bound rows, value)`` that ``y`` over the constraint rows of a bounded formulation implies: ``min(0, d_j)`` on the
    bound row of column j, ``d_j >= 0`` asserted for a column without one, ``y_c'b_c + sum_j min(0, d_j) u_j``: recomputed from the
    formulation's own data (zero fixed cost)."""
    y_c = [Fraction(y.get(i, 0)) for i in range(form.m)]
    value = sum((y_c[i] * form.b[i] for i in range(form.m)), Fraction(0))
    bound_rows = {}
    for j in range(form.n_device):
        cost = form.cost[j] if j < form.ns else Fraction(0)
        d = cost - sum((v * y_c[i] for i, v in form.device_column(j)), Fraction(0))
        if j in form.bound_row:
            if d < 0:
                bound_rows[form.bound_row[j]] = d
                value += d * form.upper[j]
        else:
            assert d >= 0, ("a column without a bound prices negative", j, d)
    return bound_rows, value
