"""The dual simplex on the device (``-m gpu``, a real MI355X): pivot for pivot against the exact reference of tests/dual_lps.py on both
sides of one wave of rows, the infeasible verdict, and the refusals.

The parent of every case is solved cold and certified on the device; the child -- the parent plus cuts its vertex violates
(``dual_lps.CutCase.child``) -- is walked by ``begin_dual`` / ``iterate_dual(1)`` and, on a fresh handle, solved by ``solve_dual``.
The cases are ``dual_lps.WALK_CASES``: small-integer data (the reference's ratio rule runs), ``mixed`` column lengths 1 .. 5, 9, 25, 40.
The conditions under which f64 cannot have chosen otherwise than the exact walk (tests/test_dual_host.py) are asserted again here, on
the basis the device found.  After the walk the f64 state -- every row of the inverse, x_B, the objective, every relative cost, a
BTRAN -- is compared with the exact state of the basis (``SparseBasisState``, ``state_checks.assert_state``).

Largest device error per part after the walk, measured on an MI355X (scales as in tests/test_gpu_sparse_state.py):

  m =  5, 4 dual pivots:   inverse 2.1e-15  x_B 4.5e-17  objective 1.5e-16  costs 7.8e-16  btran 1.9e-15   (cold solve: 5 pivots)
  m = 64, 16 dual pivots:  inverse 3.5e-15  x_B 8.3e-16  objective 4.3e-16  costs 3.7e-14  btran 2.4e-15   (cold solve: 108 pivots)
  m = 65, 12 dual pivots:  inverse 3.8e-15  x_B 1.5e-15  objective 1.9e-16  costs 5.8e-14  btran 1.3e-15   (cold solve: 131 pivots)

``solve_dual`` makes the same dual pivots and no primal one.
"""
import pytest

import relp_amd
from relp_amd.api import ERR_ARGUMENT, ERR_STATE, RelpError
import dual_lps
import sparse_lps
from dual_lps import cold_objective, solved_parent
from state_checks import assert_state

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("m", sorted(dual_lps.WALK_CASES))
def test_pivot_for_pivot_and_the_certified_optimum(m):
    seed, n_cuts = dual_lps.WALK_CASES[m]
    case = dual_lps.cut_case(m, dual_lps.MIXED, seed, n_cuts)
    child, basis, _ = case.child(*solved_parent(case))
    assert child.dual_refusal() == "" and child.kernel_path()["ratio_textbook"]
    reference = dual_lps.DualReference(child, basis)
    expected_reason = reference.run()
    dual_lps.assert_walk_conditions(reference, m, expected_reason)
    solver = relp_amd.Solver(certify=1).load_model(child)
    try:
        n_art = solver.n_art
        solver.begin_dual(basis)
        assert solver.dual_pivots() == 0
        reason = None
        for step, (q, p, leaving) in enumerate(reference.pivots):
            assert solver.iterate_dual(1) == (1, relp_amd.STOP_BUDGET), step
            assert solver.last_pivot() == (3, n_art + q, p, n_art + leaving), step
        done, reason = solver.iterate_dual(1)
        assert (done, reason) == (0, expected_reason)
        assert solver.dual_pivots() == len(reference.pivots)
        assert list(solver.basis()) == reference.basis
        # the f64 state the walk leaves against the exact state of its basis, at the project's tolerances for an un-polished state
        report = {}
        exact = sparse_lps.Provider(child).state(solver.basis(), 2)
        assert_state(solver, exact, parts=("inverse", "vertex", "costs", "btran"), report=report)
        print("m = %d, state after %d dual pivots: %s" % (m, len(reference.pivots), ", ".join("%s %.1e" % item for item in sorted(report.items()))))
    finally:
        solver.close()
    solver = relp_amd.Solver(certify=1).load_model(child)
    try:
        result = solver.solve_dual(basis)
        assert result.kind == relp_amd.FINITE_OPTIMUM and result.certified == 1
        assert solver.dual_pivots() == len(reference.pivots) and solver.record()["dual_pivots"] == len(reference.pivots)
        warm = solver.objective_exact()
        clean_up = result.pivots_phase_two
    finally:
        solver.close()
    cold, cold_result = cold_objective(child)
    assert warm == cold
    print("m = %d: %d dual pivots (+ %d primal) against %d cold pivots, smallest margin %.3g" % (
        m, len(reference.pivots), clean_up, cold_result.pivots_phase_one + cold_result.pivots_phase_two, reference.smallest_margin()))


def test_an_infeasible_child_comes_back_infeasible_and_uncertified():
    m = 64
    seed, _ = dual_lps.WALK_CASES[m]
    case = dual_lps.cut_case(m, dual_lps.MIXED, seed, 0)
    child, basis = dual_lps.infeasible_child(case, *solved_parent(case))
    assert child.right_hand_side_exact() == list(case.b) + [0, 1]  # standardisation kept the rows in order
    solver = relp_amd.Solver(certify=1).load_model(child)
    try:
        result = solver.solve_dual(basis)
        assert result.kind == relp_amd.INFEASIBLE and result.certified == 0
        assert "does not certify infeasibility" in relp_amd.lib().relp_last_error(solver._h).decode()
        cold = solver.solve_relaxation()  # the same handle, cold: phase one proves it
        assert cold.kind == relp_amd.INFEASIBLE
    finally:
        solver.close()


def test_refused_bases_leave_a_handle_that_solves_cold():
    m = 64
    seed, n_cuts = dual_lps.WALK_CASES[m]
    case = dual_lps.cut_case(m, dual_lps.MIXED, seed, n_cuts)
    expected, _ = cold_objective(case.parent)
    solver = relp_amd.Solver(certify=1)
    try:
        slack_basis = [column for _, column in sorted(case.parent.pivot_element_indices())]
        with pytest.raises(RelpError) as unloaded:  # nothing loaded yet: what set_basis answers there
            solver.begin_dual(slack_basis)
        with pytest.raises(RelpError) as set_basis_unloaded:
            solver.set_basis(slack_basis)
        assert unloaded.value.status == set_basis_unloaded.value.status == ERR_STATE
        solver.load_model(case.parent)
        with pytest.raises(RelpError, match="artificial") as artificial:
            solver.begin_dual([-1] + slack_basis[1:])
        assert artificial.value.status == ERR_ARGUMENT
        with pytest.raises(RelpError, match="artificial"):
            solver.solve_dual([-1] + slack_basis[1:])
        with pytest.raises(RelpError, match="not dual feasible") as infeasible:  # the slack basis: a cost is negative there
            solver.begin_dual(slack_basis)
        assert infeasible.value.status == ERR_ARGUMENT
        with pytest.raises(RelpError, match="begin_dual comes first"):
            solver.iterate_dual(1)
        result = solver.solve_relaxation()
        assert result.kind == relp_amd.FINITE_OPTIMUM and result.certified and solver.objective_exact() == expected
    finally:
        solver.close()


def test_a_refused_plan_is_refused_before_anything_is_launched():
    m = 64
    seed, _ = dual_lps.WALK_CASES[m]
    case = dual_lps.cut_case(m, dual_lps.MIXED, seed, 0)
    slack_basis = [column for _, column in sorted(case.parent.pivot_element_indices())]
    solver = relp_amd.Solver(carry=relp_amd.api.CARRY_LU).load_model(case.parent)
    try:
        before = int(solver.stats().launches)
        with pytest.raises(RelpError, match="LU") as refused:
            solver.solve_dual(slack_basis)
        assert refused.value.status == ERR_ARGUMENT and int(solver.stats().launches) == before
    finally:
        solver.close()
