"""The dual simplex on implicit upper bounds on the device (``-m gpu``, a real MI355X): pivot for pivot against the exact reference of
tests/dual_bounded_lps.py on both sides of one wave of rows, the f64 state the walk leaves, the certified optimum, the infeasible
verdict and the refusals.

The parent's optimal basis and vertex are the oracle's (built once per process, ``dual_bounded_lps.built``); the child -- cuts, tightened
bounds, one new bound -- is loaded with ``implicit_bounds=1``, walked by ``begin_dual_bounded`` / ``iterate_dual(1)`` and, on a fresh
handle, solved by ``solve_dual_bounded``.  After every step the formulation's basis (``Solver.basis()``) is the reference's: the side a
column left at shows there, as the variable or its bound slack on the bound row.  After the walk (``polish_period=0``) every row of
the inverse, x_B, every relative cost and the objective are compared with the reference's exact state in the held representation, at
the tolerances of tests/state_checks.py for an un-polished state.

Largest device error per part after the walk, measured on an MI355X (scales as in tests/state_checks.py):

  m =  5, 3 dual pivots (1 at the upper side):   inverse 5.3e-16  x_B 1.9e-16  objective 0        costs 6.0e-35   (cold solve: 4 pivots)
  m = 64, 27 dual pivots (4 at the upper side):  inverse 6.4e-15  x_B 1.1e-14  objective 2.0e-15  costs 8.5e-14   (cold solve: 111 pivots)
  m = 65, 28 dual pivots (3 at the upper side):  inverse 4.7e-15  x_B 1.8e-15  objective 1.9e-16  costs 7.3e-14   (cold solve: 95 pivots)
  m = 64, gather variant of the row kernel:      the figures of m = 64, digit for digit
  m = 64, steepest edge, 14 dual pivots:         inverse 4.7e-14  x_B 1.6e-14  objective 2.0e-15  costs 9.1e-14;
                                                 worst weight error 6.7e-7 of its bound, 5.0e-14 relative

``solve_dual_bounded`` makes the same dual pivots and no primal one.  At m = 513 + 24 cuts and 9 changed bounds, after 16 dual pivots
(78 columns held complemented, one of them basic), the residuals of the held representation (``dual_bounded_lps.HeldState``,
tests/residual_checks.py): B Binv - I 2.2e-13, B x_B - rhs 4.7e-13, objective 1.8e-16, costs 8.4e-13, btran 1.4e-15.  The whole
re-solve makes 1910 dual pivots there where the cold solve makes 1462: without a bound-flipping ratio test a re-solve is not always
the shorter way.  Every figure here is a value one of these tests printed on the device.
"""
from fractions import Fraction

import numpy as np
import pytest

import relp_amd
from relp_amd.api import CARRY_LU, ERR_ARGUMENT, RelpError
import dual_bounded_lps as lps
import dual_lps
from state_checks import TOLERANCE, close, deviation

pytestmark = pytest.mark.gpu


def long_double(values):
    return np.array([np.longdouble(v.numerator) / np.longdouble(v.denominator) for v in map(Fraction, values)], dtype=np.longdouble)


def assert_held_state(solver, reference, label, rows=None):
    """Every row of the inverse (``rows``: those rows only), x_B, the relative costs and the objective against the reference's exact state."""
    m, n = reference.m, reference.n
    report = {"inverse": 0.0}
    for i in (range(m) if rows is None else rows):
        got, want = solver.basis_inverse_row(i)[:m], long_double(reference.inverse[i])
        report["inverse"] = max(report["inverse"], deviation(got, want))
        assert close(got, want), ("row of the inverse", i)
    want = long_double(reference.x)
    report["vertex"] = deviation(solver.b()[:m], want)
    assert close(solver.b()[:m], want), "x_B"
    objective = float(reference.objective())
    report["objective"] = abs(solver.objective_function_value() - objective) / max(1.0, abs(objective))
    assert solver.objective_function_value() == pytest.approx(objective, rel=TOLERANCE["objective"], abs=1e-10)
    want = np.asarray(long_double(reference.relative_costs()), dtype=np.float64)
    got = solver.relative_costs()[solver.n_art:solver.n_art + n]
    report["costs"] = float((np.abs(got - want) / (1 + np.abs(want))).max())
    assert np.allclose(got, want, rtol=TOLERANCE["costs"], atol=TOLERANCE["costs"]), ("relative cost", int(np.argmax(np.abs(got - want))))
    print("%s: %s" % (label, ", ".join("%s %.1e" % item for item in sorted(report.items()))))


def assert_conditions(m, reference_class=lps.BoundedDualReference):
    """The conditions of tests/test_dual_bounded_host.py on the walk of ``reference_class`` over case ``m``, asserted where it is used."""
    _, _, child, basis, _, _ = lps.walk_case(m)
    check = reference_class(child, basis)
    reason, facts, _ = lps.walk(check)
    lps.assert_walk_conditions(check, m, reason, facts)


def walk_on_the_device(m, reference_class=lps.BoundedDualReference, **options):
    """The walk of case ``m`` step by step on a fresh handle; returns ``(solver, reference)`` with the handle still open."""
    _, _, child, basis, _, _ = lps.walk_case(m)
    assert_conditions(m, reference_class)
    reference = reference_class(child, basis)
    solver = relp_amd.Solver(implicit_bounds=1, polish_period=0, **options).load_model(child.model)
    try:
        assert solver.n_art == 0
        before = int(solver.stats().launches)
        solver.begin_dual_bounded(basis)
        assert solver.dual_pivots() == 0 and solver.record()["dual_bounded"] is True
        assert set(solver.basis()) == set(reference.formulation_basis())
        step = 0
        while True:
            expected = reference.step()
            if expected is not None:
                break
            q, p, leaving, _ = reference.pivots[-1]
            assert solver.iterate_dual(1) == (1, relp_amd.STOP_BUDGET), step
            assert solver.last_pivot() == (3, q, p, leaving), (step, reference.pivots[-1])
            assert set(solver.basis()) == set(reference.formulation_basis()), (step, reference.pivots[-1])
            step += 1
        assert solver.iterate_dual(1) == (0, expected) and expected == relp_amd.STOP_NO_ENTERING
        assert solver.dual_pivots() == len(reference.pivots)
        assert int(solver.stats().launches) > before
        return solver, reference
    except BaseException:
        solver.close()
        raise


@pytest.mark.parametrize("m", sorted(lps.WALK_CASES))
def test_pivot_for_pivot_and_the_state_after_the_walk(m):
    _, _, child, basis, _, _ = lps.walk_case(m)
    assert child.model.dual_bounded_refusal(implicit_bounds=1) == "" and child.model.kernel_path(implicit_bounds=1)["ratio_textbook"]
    solver, reference = walk_on_the_device(m)  # (asserts the walk conditions)
    try:
        sides = [side for _, _, _, side in reference.pivots]
        assert_held_state(solver, reference, "m = %d, state after %d dual pivots (%d at the upper side)" % (m, len(sides), sides.count(-1)))
    finally:
        solver.close()


def test_the_gather_variant_of_the_row_kernel_walks_the_same_way():
    solver, reference = walk_on_the_device(64, price_lds_max=64)  # (2 m doubles do not fit: rho and -pi are gathered from memory)
    try:
        assert_held_state(solver, reference, "m = 64, gather variant, %d dual pivots" % len(reference.pivots))
    finally:
        solver.close()


def test_the_steepest_edge_rule_walks_as_its_reference_and_keeps_the_row_norms():
    from test_gpu_dual_se import weight_bounds
    solver, reference = walk_on_the_device(64, reference_class=lps.SteepestBoundedDualReference, dual_pricing=relp_amd.api.DUAL_PRICING_STEEPEST_EDGE)
    try:
        beta, bound = weight_bounds(reference.inverse)
        weights = solver.dual_weights()[:reference.m]
        error = np.abs(weights - beta)
        print("m = 64, steepest edge, weights after %d dual pivots: worst error / bound %.2e, worst relative error %.2e" % (
            len(reference.pivots), float((error / bound).max()), float((error / beta).max())))
        assert (weights > 0).all() and (error <= bound).all(), ("weight of row", int(np.argmax(error / bound)))
        assert_held_state(solver, reference, "m = 64, steepest edge, %d dual pivots" % len(reference.pivots))
    finally:
        solver.close()


def cold_exact(model, **options):
    solver = relp_amd.Solver(certify=1, **options).load_model(model)
    try:
        result = solver.solve_relaxation()
        assert result.kind == relp_amd.FINITE_OPTIMUM and result.certified
        return solver.objective_exact(), result
    finally:
        solver.close()


@pytest.mark.parametrize("m", sorted(lps.WALK_CASES))
def test_solve_dual_bounded_certifies_the_optimum_of_a_cold_solve(m):
    _, _, child, basis, _, _ = lps.walk_case(m)
    assert_conditions(m)
    reference = lps.BoundedDualReference(child, basis)
    assert reference.run() == relp_amd.STOP_NO_ENTERING
    solver = relp_amd.Solver(certify=1, implicit_bounds=1).load_model(child.model)
    try:
        result = solver.solve_dual_bounded(basis)
        assert result.kind == relp_amd.FINITE_OPTIMUM and result.certified == 1
        assert solver.dual_pivots() == len(reference.pivots) == solver.record()["dual_pivots"] and solver.record()["dual_bounded"] is True
        warm = solver.objective_exact()
        x = solver.solution()
        for j in range(child.ns):
            assert -1e-9 <= x[j] and (child.upper[j] is None or x[j] <= child.upper[j] + 1e-9), (j, x[j], child.upper[j])
        clean_up = result.pivots_phase_two
    finally:
        solver.close()
    implicit, implicit_result = cold_exact(child.model, implicit_bounds=1)
    explicit, explicit_result = cold_exact(child.model, implicit_bounds=0)
    assert Fraction(warm) == Fraction(implicit) == Fraction(explicit) == reference.objective()
    print("m = %d: %d dual pivots (+ %d primal) against %d cold pivots on implicit bounds, %d with the bounds as rows" % (
        m, len(reference.pivots), clean_up, implicit_result.pivots_phase_one + implicit_result.pivots_phase_two,
        explicit_result.pivots_phase_one + explicit_result.pivots_phase_two))


def test_a_state_case_of_513_rows():
    """(The parent's optimum is the certified device solve's here: the oracle would take minutes at this size.)"""
    m, seed, n_cuts, n_tight = lps.STATE_CASE
    case = lps.BoundedCase(m, seed, n_cuts, n_tight)
    parent = relp_amd.Solver(certify=1, implicit_bounds=1).load_model(case.parent.model)
    try:
        result = parent.solve_relaxation()
        assert result.kind == relp_amd.FINITE_OPTIMUM and result.certified
        child, basis, cuts, branches = case.child(parent.basis(), parent.solution_exact())
    finally:
        parent.close()
    assert child.m == m + n_cuts and len(branches) == n_tight + 1
    solver = relp_amd.Solver(certify=1, implicit_bounds=1).load_model(child.model)
    try:
        solver.begin_dual_bounded(basis)
        done, _ = solver.iterate_dual(16)
        assert done >= 8 and solver.dual_pivots() == done
        # the f64 state in the middle of the walk against the exact data of its basis in the held representation: every entry of
        # B Binv - I, B x_B - rhs and the objective, every relative cost, three BTRANs, at the bounds of tests/residual_checks.py
        from residual_checks import assert_residuals
        from sparse_lps import btrans
        handle, provider, state = lps.held_pair(solver, child)
        report = {}
        assert_residuals(handle, provider, btrans(child.m), report=report)
        print("m = %d + %d cuts, after %d dual pivots (%d basic columns held complemented, %d columns in all): %s" % (
            m, n_cuts, done, state.complemented_basic, sum(1 for v in state.sgn if v < 0), ", ".join("%s %.1e" % item for item in sorted(report.items()))))
        result = solver.solve_dual_bounded(basis)
        assert result.kind == relp_amd.FINITE_OPTIMUM and result.certified == 1
        warm, pivots = solver.objective_exact(), solver.dual_pivots()
    finally:
        solver.close()
    cold, cold_result = cold_exact(child.model, implicit_bounds=1)
    assert Fraction(warm) == Fraction(cold)
    print("m = %d + %d cuts, %d tightened bounds: %d dual pivots against %d cold pivots" % (
        m, n_cuts, n_tight, pivots, cold_result.pivots_phase_one + cold_result.pivots_phase_two))


def test_an_infeasible_child_comes_back_infeasible_and_uncertified():
    _, _, child, basis = lps.infeasible_child()
    solver = relp_amd.Solver(certify=1, implicit_bounds=1).load_model(child.model)
    try:
        result = solver.solve_dual_bounded(basis)
        assert result.kind == relp_amd.INFEASIBLE and result.certified == 0
        assert "does not certify infeasibility" in relp_amd.lib().relp_last_error(solver._h).decode()
        cold = solver.solve_relaxation()  # the same handle, cold: phase one proves it
        assert cold.kind == relp_amd.INFEASIBLE
    finally:
        solver.close()


def test_refusals_come_before_any_launch_and_leave_a_handle_that_solves_cold():
    case, optimum, child, basis, _, _ = lps.walk_case(64)
    expected, _ = cold_exact(child.model, implicit_bounds=1)
    solver = relp_amd.Solver(certify=1, implicit_bounds=1).load_model(child.model)
    try:
        before = int(solver.stats().launches)
        for row in (0, child.m - 1, child.rows - 1):  # a constraint row, a cut, a bound row of the formulation
            with_artificial = list(basis)
            with_artificial[row] = -1
            with pytest.raises(RelpError, match="artificial") as artificial:
                solver.begin_dual_bounded(with_artificial)
            assert artificial.value.status == ERR_ARGUMENT
        slack_basis = [column for _, column in sorted(child.model.pivot_element_indices())]
        assert len(slack_basis) == child.rows
        with pytest.raises(RelpError, match=r"not dual feasible: column \d+ has the relative cost -") as infeasible:
            solver.begin_dual_bounded(slack_basis)  # the slack basis: a cost is negative there
        assert infeasible.value.status == ERR_ARGUMENT
        with pytest.raises(RelpError, match="begin_dual comes first"):
            solver.iterate_dual(1)
        assert int(solver.stats().launches) == before
        result = solver.solve_relaxation()
        assert result.kind == relp_amd.FINITE_OPTIMUM and result.certified and solver.objective_exact() == expected
    finally:
        solver.close()
    solver = relp_amd.Solver(carry=CARRY_LU, implicit_bounds=1).load_model(child.model)
    try:
        before = int(solver.stats().launches)
        with pytest.raises(RelpError, match="LU") as refused:
            solver.solve_dual_bounded(basis)
        assert refused.value.status == ERR_ARGUMENT and int(solver.stats().launches) == before
    finally:
        solver.close()


def test_an_unbounded_plan_makes_the_pivots_of_solve_dual():
    seed, n_cuts = dual_lps.WALK_CASES[64]
    case = dual_lps.cut_case(64, dual_lps.MIXED, seed, n_cuts)
    child, basis, _ = case.child(*dual_lps.solved_parent(case))
    pivots, objectives = [], []
    for entry in ("solve_dual", "solve_dual_bounded"):
        solver = relp_amd.Solver(certify=1, implicit_bounds=1).load_model(child)  # (no bound: the option does not apply)
        try:
            result = getattr(solver, entry)(basis)
            assert result.kind == relp_amd.FINITE_OPTIMUM and result.certified == 1
            assert solver.record()["dual_bounded"] is False
            pivots.append((solver.dual_pivots(), result.pivots_phase_two, tuple(solver.basis())))
            objectives.append(solver.objective_exact())
        finally:
            solver.close()
    assert pivots[0] == pivots[1] and objectives[0] == objectives[1] and pivots[0][0] >= 8


def test_the_plain_entry_points_still_refuse_a_bounded_plan():
    _, _, child, basis, _, _ = lps.walk_case(5)
    solver = relp_amd.Solver(implicit_bounds=1).load_model(child.model)
    other = relp_amd.Solver(implicit_bounds=1).load_model(child.model)
    try:
        for call in (lambda: solver.solve_dual(basis), lambda: solver.begin_dual(basis), lambda: solver.begin_dual_from(other, basis)):
            with pytest.raises(RelpError, match="implicit upper bounds") as refused:
                call()
            assert refused.value.status == ERR_ARGUMENT
    finally:
        solver.close()
        other.close()
