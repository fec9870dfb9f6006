"""The dual simplex started from the parent's inverse on the device (``-m gpu``, a real MI355X): ``Solver.begin_dual_from`` /
``solve_dual_from`` against the exact state of the child's basis, the exact walk of tests/dual_lps.py and the cold certified solve.

The parent of every case is solved cold and certified on one handle that stays open; the child is loaded on a second handle and
started from the first.  Helpers and tolerances are those of tests/test_gpu_dual.py and tests/test_gpu_dual_state.py (an un-polished
state: tests/state_checks.py, tests/residual_checks.py); nothing here sets a tolerance of its own.

  border and walk   ``dual_lps.WALK_CASES`` (5 + 3 cuts, 64 + 4, 65 + 3: either side of one wave of rows, child leading dimensions 8, 68
                    and 68): at 0 pivots every row of the inherited inverse -- the k new rows included --, x_B, the objective, every
                    relative cost and a BTRAN against the exact state of the basis; then the walk pivot for pivot; then
                    ``solve_dual_from`` on a fresh handle, certified, with the cold solve's exact objective
  the parent        solves again afterwards to the same exact objective
  two generations   the child solved by ``solve_dual_from`` is the parent of a grandchild: the inherited basis has structural columns on
                    former cut rows
  k = 0             the same rows, right-hand sides tightened
  pivot paths       ``dual_lps.STATE_CASES`` at m = 513 (fused pivot) and 2049 (three-kernel pivot, touched-column tracking):
                    residuals at 0 pivots and after 16 dual pivots, dual feasibility kept; a whole ``solve_dual_from`` on decimal data
                    at m = 513 (the Harris rule)
  refusals          a parent with nothing solved, a parent under the LU carry, a parent that is another LP

Measured on an MI355X, the inherited state at 0 pivots (the guard's first residual; largest device error per part, scales as in
tests/test_gpu_dual.py and tests/test_gpu_dual_state.py); the guard added no GEMM in any case:

  m =    5 + 3 cuts:   residual 5.6e-17  inverse 6.8e-17  x_B 2.4e-17  objective 1.7e-16  costs 1.4e-16  btran 3.8e-17
  m =   64 + 4 cuts:   residual 1.4e-13  inverse 1.1e-14  x_B 4.3e-15  objective 2.0e-15  costs 3.2e-13  btran 5.1e-15
  m =   65 + 3 cuts:   residual 2.6e-13  inverse 1.9e-14  x_B 2.0e-14  objective 1.7e-15  costs 9.4e-13  btran 4.0e-15
  m =  513 + 24 cuts:  residual 3.3e-14  B Binv - I 1.4e-13  B x_B - b 7.4e-13  costs 1.9e-13  btran 7.9e-16   (after 16 pivots: 1.8e-13, 7.2e-13, 6.3e-13, 3.1e-15)
  m = 2049 + 24 cuts:  residual 3.9e-13  B Binv - I 3.7e-12  B x_B - b 1.2e-11  costs 3.7e-12  btran 1.5e-15   (after 16 pivots: 6.7e-13, 1.2e-11, 3.7e-12, 2.3e-15)

Two generations: 2 structural columns on former cut rows, 26 dual pivots in the grandchild; k = 0: 47 right-hand sides lowered, 10
dual pivots; decimal m = 513: 146 dual + 0 primal pivots.  The slowest case, m = 2049, takes 3.4 s.
"""
from fractions import Fraction

import numpy as np
import pytest

import relp_amd
from relp_amd.api import CARRY_LU, ERR_ARGUMENT, ERR_STATE, RelpError
import dual_lps
import sparse_lps
from dual_lps import cold_objective
from residual_checks import assert_residuals
from state_checks import assert_state
from test_gpu_dual_state import OPTIONS, btrans, expected_plan

pytestmark = pytest.mark.gpu


class Family:
    """A parent solved cold and certified on a handle that stays open, and its child: the model, the basis in the order
    ``Solver.basis()`` and ``dual_lps.extended_basis`` produce, and the exact objective of the child's cold certified solve."""

    def __init__(self, case):
        self.case = case
        self.parent = relp_amd.Solver(certify=1).load_model(case.parent)
        result = self.parent.solve_relaxation()
        assert result.kind == relp_amd.FINITE_OPTIMUM and result.certified
        self.parent_objective = self.parent.objective_exact()
        self.child, self.basis, self.cuts = case.child(self.parent.basis(), self.parent.solution_exact())
        self._cold = None

    @property
    def cold(self):
        if self._cold is None:
            self._cold = cold_objective(self.child)[0]
        return self._cold

    def close(self):
        self.parent.close()


@pytest.fixture(scope="module")
def families():
    """The walk cases, each solved once for the tests that share it; the parent handles are closed with the module."""
    made = {}

    def family(m):
        if m not in made:
            seed, n_cuts = dual_lps.WALK_CASES[m]
            made[m] = Family(dual_lps.cut_case(m, dual_lps.MIXED, seed, n_cuts))
        return made[m]
    yield family
    for entry in made.values():
        entry.close()


def solve_from(parent, child, basis, **options):
    """``(result, exact objective, dual pivots, record)`` of ``solve_dual_from`` on a fresh handle."""
    solver = relp_amd.Solver(**(options or dict(certify=1))).load_model(child)
    try:
        result = solver.solve_dual_from(parent, basis)
        assert result.kind == relp_amd.FINITE_OPTIMUM and result.certified == 1
        return result, solver.objective_exact(), solver.dual_pivots(), solver.record()
    finally:
        solver.close()


@pytest.mark.parametrize("m", sorted(dual_lps.WALK_CASES))
def test_the_inherited_inverse_then_the_walk_pivot_for_pivot(families, m):
    family = families(m)
    child, basis = family.child, family.basis
    assert child.dual_refusal() == "" and child.kernel_path()["ratio_textbook"]
    assert child.dual_inherit_refusal(family.case.parent, family.parent.basis(), basis) == ""
    reference = dual_lps.DualReference(child, basis)
    expected_reason = reference.run()
    dual_lps.assert_walk_conditions(reference, m, expected_reason)
    solver = relp_amd.Solver(certify=1).load_model(child)
    try:
        n_art = solver.n_art
        solver.begin_dual_from(family.parent, basis)
        record = solver.record()
        assert record["dual_start"] == "inherited" and record["dual_start_gemms"] <= 2, record
        assert solver.dual_pivots() == 0 and list(solver.basis()) == [int(c) for c in basis]
        # the border itself: every row of the inverse (the k new ones are the last), x_B, the objective, the costs, a BTRAN
        report = {}
        assert_state(solver, sparse_lps.Provider(child).state(basis, 2), parts=("inverse", "vertex", "costs", "btran"), report=report)
        print("m = %d + %d cuts, inherited state (residual %.1e, %d GEMMs, %.2f ms): %s" % (
            m, len(family.cuts), record["dual_start_residual"], record["dual_start_gemms"], 1e3 * record["dual_start_seconds"],
            ", ".join("%s %.1e" % item for item in sorted(report.items()))))
        for step, (q, p, leaving) in enumerate(reference.pivots):
            assert solver.iterate_dual(1) == (1, relp_amd.STOP_BUDGET), step
            assert solver.last_pivot() == (3, n_art + q, p, n_art + leaving), step
        done, reason = solver.iterate_dual(1)
        assert (done, reason) == (0, expected_reason)
        assert solver.dual_pivots() == len(reference.pivots)
        assert list(solver.basis()) == reference.basis
    finally:
        solver.close()
    result, warm, pivots, record = solve_from(family.parent, child, basis)
    assert record["dual_start"] == "inherited" and pivots == len(reference.pivots) == record["dual_pivots"]
    assert warm == family.cold


def test_the_parent_is_only_read(families):
    family = families(64)
    solve_from(family.parent, family.child, family.basis)
    again = family.parent.solve_relaxation()
    assert again.kind == relp_amd.FINITE_OPTIMUM and again.certified
    assert family.parent.objective_exact() == family.parent_objective


# (seed, n_cuts) of the second generation's cuts, chosen on the CPU with the exact reference of tests/dual_lps.py: from the child's
# optimum (structural columns 15 and 100 basic on former cut rows) the three cuts bite, no right-hand side is negative, and the
# grandchild is feasible after 26 dual pivots (seeds 5064 and 6064 do as well: 17 each)
GRANDCHILD = (4064, 3)


def test_two_generations(families):
    family = families(64)
    child = relp_amd.Solver(certify=1).load_model(family.child)
    try:
        result = child.solve_dual_from(family.parent, family.basis)
        assert result.kind == relp_amd.FINITE_OPTIMUM and result.certified == 1 and child.objective_exact() == family.cold
        basis, vertex = child.basis(), child.solution_exact()
        n_structural = family.case.n_structural
        structural_on_cut_rows = [int(c) for c in basis[family.case.m:] if c < n_structural]
        assert structural_on_cut_rows, "no structural column is basic on a former cut row: the case says nothing"
        seed, n_cuts = GRANDCHILD
        model, grandchild_basis, cuts = dual_lps.CutCase(family.child, seed, n_cuts).child(basis, vertex)
        for variables, coefficients, rhs in cuts:  # every cut bites, no right-hand side is negative
            assert rhs >= 0 and sum(a * vertex.get(j, Fraction(0)) for j, a in zip(variables, coefficients)) > rhs
        assert model.right_hand_side_exact() == family.child.right_hand_side_exact() + [rhs for _, _, rhs in cuts]
        result, warm, pivots, record = solve_from(child, model, grandchild_basis)
        assert record["dual_start"] == "inherited" and pivots >= 1
        assert warm == cold_objective(model)[0]
        print("two generations: %d structural columns on former cut rows, %d dual pivots in the grandchild" % (len(structural_on_cut_rows), pivots))
    finally:
        child.close()


def tightened(case, vertex):
    """The parent's rows with the right-hand side of row i lowered to ``max(0, floor(a_i x*) - 1)`` where that is below the activity
    ``a_i x*`` (so the vertex violates the row, and no right-hand side is negative: no row is flipped); the other rows keep theirs."""
    activity = [Fraction(0)] * case.m
    for j, column in enumerate(case.columns):
        for i, v in column:
            activity[i] += v * vertex.get(j, Fraction(0))
    b, lowered = list(case.b), 0
    for i, value in enumerate(activity):
        bound = max(0, value.numerator // value.denominator - 1)
        if bound < value:
            assert bound <= b[i]
            b[i], lowered = bound, lowered + 1
    model = relp_amd.Model.from_general_form(case.columns, ["Less"] * case.m, b, [(c, 0, None) for c in case.cost])
    return model, b, lowered


def test_the_same_rows_with_tightened_right_hand_sides(families):
    family = families(64)
    case = family.case
    model, b, lowered = tightened(case, family.parent.solution_exact())
    assert lowered >= 1 and model.nr_rows == case.m and model.right_hand_side_exact() == b
    basis = family.parent.basis()
    result, warm, pivots, record = solve_from(family.parent, model, basis)
    assert record["dual_start"] == "inherited" and record["dual_start_gemms"] <= 2 and pivots >= 1
    assert warm == cold_objective(model)[0]
    print("k = 0: %d right-hand sides lowered, %d dual pivots" % (lowered, pivots))


def state_family(m, decimal=False):
    """``test_gpu_dual_state.child_of`` with the parent's handle kept open: the plans asserted before the device is touched."""
    seed, n_cuts = dual_lps.STATE_CASES[m]
    case = dual_lps.cut_case(m, dual_lps.MIXED, seed, n_cuts, decimal=decimal)
    plan = case.parent.kernel_path(**OPTIONS)
    assert plan["ratio_textbook"] == (not decimal)
    for field, value in expected_plan(m).items():
        assert plan[field] == value, (field, plan[field], value)
    family = Family(case)
    plan = family.child.kernel_path(**OPTIONS)
    assert family.child.dual_refusal(**OPTIONS) == "" and plan["ratio_textbook"] == (not decimal)
    for field, value in expected_plan(m).items():
        assert plan[field] == value, (field, plan[field], value)
    return family


@pytest.mark.parametrize("m", [513, 2049])
def test_the_other_pivot_paths(m):
    family = state_family(m)
    solver = relp_amd.Solver(**OPTIONS).load_model(family.child)
    try:
        solver.begin_dual_from(family.parent, family.basis)
        record = solver.record()
        assert record["dual_start"] == "inherited" and record["dual_start_gemms"] <= 2, record
        provider, start, after = sparse_lps.Provider(family.child), {}, {}
        assert_residuals(solver, provider, btrans(solver.m), report=start)
        done, reason = solver.iterate_dual(16)
        assert done >= 8 and (reason == relp_amd.STOP_BUDGET) == (done == 16), (done, reason)
        assert_residuals(solver, provider, btrans(solver.m), report=after)
        is_basic = np.zeros(solver.n, dtype=bool)
        is_basic[solver.basis() + solver.n_art] = True
        costs = solver.relative_costs()
        assert costs[~is_basic].min() >= -1e-9, ("dual feasibility", float(costs[~is_basic].min()))
        print("integer m = %4d: inherited (residual %.1e, %d GEMMs, %.2f ms); at 0 pivots %s; after %d dual pivots %s" % (
            m, record["dual_start_residual"], record["dual_start_gemms"], 1e3 * record["dual_start_seconds"],
            "  ".join("%s %.1e" % item for item in sorted(start.items())), done, "  ".join("%s %.1e" % item for item in sorted(after.items()))))
    finally:
        solver.close()
        family.close()


def test_decimal_data_under_the_harris_rule():
    family = state_family(513, decimal=True)
    try:
        result, warm, pivots, record = solve_from(family.parent, family.child, family.basis, polish_period=0, certify=1)
        assert record["dual_start"] == "inherited" and pivots >= 8
        assert warm == family.cold
        print("decimal m =  513: solve_dual_from %d dual + %d primal pivots, start %.2f ms" % (pivots, result.pivots_phase_two, 1e3 * record["dual_start_seconds"]))
    finally:
        family.close()


def test_refusals(families):
    family = families(64)
    child, basis = family.child, family.basis
    solver = relp_amd.Solver(certify=1).load_model(child)
    idle = relp_amd.Solver().load_model(family.case.parent)                 # loaded, nothing solved
    lu = relp_amd.Solver(carry=CARRY_LU).load_model(family.case.parent)     # a plan the dual kernels do not take
    other_case = dual_lps.cut_case(64, dual_lps.MIXED, 3064, 0)             # the LP of another seed, solved
    other = relp_amd.Solver(certify=1).load_model(other_case.parent)
    try:
        with pytest.raises(RelpError) as nothing_solved:
            solver.begin_dual_from(idle, basis)
        assert nothing_solved.value.status == ERR_STATE
        with pytest.raises(RelpError) as itself:
            solver.begin_dual_from(solver, basis)
        assert itself.value.status == ERR_STATE
        assert lu.solve_relaxation().kind == relp_amd.FINITE_OPTIMUM
        before = int(solver.stats().launches), int(lu.stats().launches)
        with pytest.raises(RelpError, match="LU") as plan:
            solver.solve_dual_from(lu, basis)
        assert plan.value.status == ERR_ARGUMENT and (int(solver.stats().launches), int(lu.stats().launches)) == before
        assert other.solve_relaxation().kind == relp_amd.FINITE_OPTIMUM
        before = int(solver.stats().launches), int(other.stats().launches)
        with pytest.raises(RelpError, match="column") as relation:
            solver.begin_dual_from(other, basis)
        assert relation.value.status == ERR_ARGUMENT and (int(solver.stats().launches), int(other.stats().launches)) == before
        with pytest.raises(RelpError, match="begin_dual comes first"):  # nothing was started
            solver.iterate_dual(1)
        result = solver.solve_dual(basis)  # the same handle, from scratch
        assert result.kind == relp_amd.FINITE_OPTIMUM and result.certified == 1 and solver.objective_exact() == family.cold
        assert solver.record()["dual_start"] == "scratch"
    finally:
        for handle in (solver, idle, lu, other):
            handle.close()
