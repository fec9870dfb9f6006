"""The long-step (bound-flipping) ratio test of the bounded dual loop on the device (``-m gpu``, a real MI355X): pivot for pivot against
the exact reference of tests/dual_long_step_lps.py, the f64 state the walk leaves, the certified optimum, the infeasible verdict, the
switch and the refusals.

The cases are those of tests/test_dual_long_step_host.py (a bound on every structural variable); every walk of a reference is made
once per process (``dual_long_step_lps.walked``) and only read here.  After every ``iterate_dual(1)`` the pivot ``(q, p, leaving)``,
the formulation's basis -- a flipped non-basic column shows there as the variable itself on its bound row -- and the cumulative
``record()["dual_flips"]`` are the reference's.  The state after the walk is held to the checks and bounds of
tests/test_gpu_dual_bounded.py (``assert_held_state``, tests/state_checks.py): no tolerance of this file's own.

Largest device error per part after the walk, measured on an MI355X (scales as in tests/state_checks.py):

  m =  5, case 0, 5 dual pivots, 1 flip:            inverse 1.5e-16  x_B 3.9e-16  objective 0        costs 2.1e-15
  m =  5, case 1, 3 dual pivots, 1 flip:            inverse 2.2e-16  x_B 2.2e-16  objective 3.6e-16  costs 5.1e-16
  m = 64, 32 dual pivots, 8 flips:                  inverse 3.9e-15  x_B 1.3e-15  objective 4.0e-16  costs 3.1e-14
  m = 65, 62 dual pivots, 16 flips:                 inverse 1.3e-14  x_B 5.3e-15  objective 8.0e-16  costs 3.2e-14
  m = 64, gather variant of the row kernel:         the figures of m = 64, digit for digit
  m = 64, steepest edge, 25 dual pivots, 14 flips:  inverse 5.3e-15  x_B 1.6e-15  objective 2.5e-16  costs 2.2e-14

``solve_dual_bounded(long_step=True)`` makes the reference's pivots and flips (32 / 8 and 62 / 16 against 47 and 82 dual pivots of the
plain rule on the same handle options); on the decimal data of the same cases (Harris rule) both rules make 9 and 5 dual pivots, with
1 and 0 flips.  At m = 513 + 24 cuts with a bound on every variable, 16 dual pivots make 8 flips (152 columns held complemented
afterwards), and the residuals of the held representation are B Binv - I 4.4e-14, B x_B - rhs 3.0e-13, objective 0, costs 2.9e-13,
btran 1.9e-15.  Every figure here is a value one of these tests printed on the device.
"""
from fractions import Fraction

import pytest

import relp_amd
from relp_amd.api import DUAL_PRICING_STEEPEST_EDGE, ERR_ARGUMENT, RelpError
import dual_bounded_lps
import dual_lps
import dual_long_step_lps as lps
from test_gpu_dual_bounded import assert_held_state, cold_exact

pytestmark = pytest.mark.gpu

CASES = [(m, which) for m in sorted(lps.LONG_STEP_CASES) for which in range(len(lps.LONG_STEP_CASES[m]))]


def walk_on_the_device(m, which=0, steepest=False, **options):
    """The long-step walk of a chosen case step by step on a fresh handle; returns ``(solver, reference)`` with the handle still open."""
    reference, reason, facts, bases, dual_feasible, start = lps.walked(m, which, steepest)
    lps.assert_long_step_conditions(reference, m, reason, facts, dual_feasible)
    _, _, child, basis, _, _ = lps.built(m, *(lps.STEEPEST_CASE[m] if steepest else lps.LONG_STEP_CASES[m][which]))
    if steepest:
        options["dual_pricing"] = DUAL_PRICING_STEEPEST_EDGE
    solver = relp_amd.Solver(implicit_bounds=1, polish_period=0, **options).load_model(child.model)
    try:
        assert solver.n_art == 0
        solver.set_dual_long_step(True)
        solver.begin_dual_bounded(basis)
        record = solver.record()
        assert record["dual_bounded"] is True and record["dual_long_step"] is True and record["dual_flips"] == 0
        assert set(solver.basis()) == set(start)
        flips = 0
        for step, (q, p, leaving, _) in enumerate(reference.pivots):
            before = int(solver.stats().launches)
            assert solver.iterate_dual(1) == (1, relp_amd.STOP_BUDGET), step
            if not steepest:
                assert int(solver.stats().launches) - before == 1 + 6  # the budget, the five kernels of a pivot and dual_long_step_kernel
            assert solver.last_pivot() == (3, q, p, leaving), (step, reference.pivots[step], reference.flips[step])
            assert set(solver.basis()) == set(bases[step]), (step, reference.pivots[step], reference.flips[step])
            flips += len(reference.flips[step])
            assert solver.record()["dual_flips"] == flips, (step, reference.flips[step])
        assert solver.iterate_dual(1) == (0, relp_amd.STOP_NO_ENTERING)
        assert solver.dual_pivots() == len(reference.pivots) and flips == reference.total_flips() >= lps.MIN_FLIPS[m]
        assert solver.record()["dual_long_step_skipped"] == 0
        return solver, reference
    except BaseException:
        solver.close()
        raise


@pytest.mark.parametrize("m,which", CASES)
def test_pivot_for_pivot_and_the_state_after_the_walk(m, which):
    solver, reference = walk_on_the_device(m, which)
    try:
        assert_held_state(solver, reference, "m = %d, case %d, state after %d dual pivots and %d flips" % (
            m, which, len(reference.pivots), reference.total_flips()))
    finally:
        solver.close()


def test_the_gather_variant_of_the_row_kernel_walks_the_same_way():
    solver, reference = walk_on_the_device(64, price_lds_max=64)  # (2 m doubles do not fit: rho and -pi are gathered from memory)
    try:
        assert_held_state(solver, reference, "m = 64, gather variant, %d dual pivots and %d flips" % (len(reference.pivots), reference.total_flips()))
    finally:
        solver.close()


def test_the_steepest_edge_rule_walks_as_its_reference():
    solver, reference = walk_on_the_device(64, steepest=True)
    try:
        assert_held_state(solver, reference, "m = 64, steepest edge, %d dual pivots and %d flips" % (len(reference.pivots), reference.total_flips()))
    finally:
        solver.close()


def solved(child, basis, long_step):
    """``solve_dual_bounded`` on a fresh handle: ``(exact objective, dual pivots, record)``; certified, within the bounds."""
    solver = relp_amd.Solver(certify=1, implicit_bounds=1).load_model(child.model)
    try:
        result = solver.solve_dual_bounded(basis, long_step=long_step)
        assert result.kind == relp_amd.FINITE_OPTIMUM and result.certified == 1
        record = solver.record()
        assert record["dual_long_step"] is long_step and record["dual_bounded"] is True and record["dual_pivots"] == solver.dual_pivots()
        x = solver.solution()
        for j in range(child.ns):
            assert -1e-9 <= x[j] and (child.upper[j] is None or x[j] <= child.upper[j] + 1e-9), (j, x[j], child.upper[j])
        return solver.objective_exact(), solver.dual_pivots(), record
    finally:
        solver.close()


@pytest.mark.parametrize("m", [64, 65])
def test_solve_dual_bounded_with_the_long_step_certifies_the_optimum_of_a_cold_solve(m):
    reference = lps.walked(m)[0]
    plain_reference, _ = lps.plain_walked(m)
    _, _, child, basis, _, _ = lps.long_step_case(m)
    warm, pivots, record = solved(child, basis, True)
    assert pivots == len(reference.pivots) and record["dual_flips"] == reference.total_flips() and record["dual_long_step_skipped"] == 0
    plain, plain_pivots, plain_record = solved(child, basis, False)
    assert plain_pivots == len(plain_reference.pivots) and plain_record["dual_flips"] == 0
    if len(reference.pivots) <= len(plain_reference.pivots):  # (the reference says so for both chosen cases)
        assert pivots <= plain_pivots
    cold, _ = cold_exact(child.model, implicit_bounds=1)
    assert Fraction(warm) == Fraction(plain) == Fraction(cold) == reference.objective()
    print("m = %d: %d dual pivots and %d flips with the long step, %d dual pivots without" % (m, pivots, record["dual_flips"], plain_pivots))


@pytest.mark.parametrize("m", [64, 65])
def test_the_long_step_under_the_harris_rule_on_decimal_data(m):
    _, _, child, basis, _, _ = lps.built(m, *lps.LONG_STEP_CASES[m][0], decimal=True)
    assert not child.model.kernel_path(implicit_bounds=1)["ratio_textbook"]
    warm, pivots, record = solved(child, basis, True)
    assert record["dual_long_step_skipped"] == 0
    plain, plain_pivots, _ = solved(child, basis, False)
    cold, _ = cold_exact(child.model, implicit_bounds=1)
    assert Fraction(warm) == Fraction(plain) == Fraction(cold)
    print("m = %d, decimal data: %d dual pivots and %d flips with the long step, %d dual pivots without" % (m, pivots, record["dual_flips"], plain_pivots))


def test_a_state_case_of_513_rows():
    """(The parent's optimum is the certified device solve's here, as in tests/test_gpu_dual_bounded.py.)"""
    m, seed, n_cuts, n_tight = dual_bounded_lps.STATE_CASE
    case = dual_bounded_lps.BoundedCase(m, seed, n_cuts, n_tight, every=lps.EVERY)
    parent = relp_amd.Solver(certify=1, implicit_bounds=1).load_model(case.parent.model)
    try:
        result = parent.solve_relaxation()
        assert result.kind == relp_amd.FINITE_OPTIMUM and result.certified
        child, basis, _, _ = case.child(parent.basis(), parent.solution_exact())
    finally:
        parent.close()
    solver = relp_amd.Solver(certify=1, implicit_bounds=1).load_model(child.model)
    try:
        solver.set_dual_long_step(True)
        solver.begin_dual_bounded(basis)
        done, _ = solver.iterate_dual(16)
        record = solver.record()
        assert done >= 8 and solver.dual_pivots() == done
        assert record["dual_flips"] >= 1 and record["dual_long_step_skipped"] == 0, record["dual_flips"]
        from residual_checks import assert_residuals
        from sparse_lps import btrans
        handle, provider, state = dual_bounded_lps.held_pair(solver, child)
        report = {}
        assert_residuals(handle, provider, btrans(child.m), report=report)
        print("m = %d + %d cuts, a bound on every variable, after %d dual pivots and %d flips (%d columns held complemented): %s" % (
            m, n_cuts, done, record["dual_flips"], sum(1 for v in state.sgn if v < 0), ", ".join("%s %.1e" % item for item in sorted(report.items()))))
    finally:
        solver.close()


def test_an_infeasible_child_comes_back_infeasible_and_uncertified():
    _, _, child, basis = dual_bounded_lps.infeasible_child(64)
    solver = relp_amd.Solver(certify=1, implicit_bounds=1).load_model(child.model)
    try:
        result = solver.solve_dual_bounded(basis, long_step=True)
        assert result.kind == relp_amd.INFEASIBLE and result.certified == 0
        assert solver.record()["dual_long_step"] is True
        assert "does not certify infeasibility" in relp_amd.lib().relp_last_error(solver._h).decode()
    finally:
        solver.close()


def test_with_the_switch_off_the_walk_and_the_launches_are_the_plain_rules():
    reference, bases = lps.plain_walked(64)
    assert reference.pivots != lps.walked(64)[0].pivots
    _, _, child, basis, _, _ = lps.long_step_case(64)
    solver = relp_amd.Solver(implicit_bounds=1, polish_period=0).load_model(child.model)
    try:
        solver.set_dual_long_step(True)
        solver.set_dual_long_step(False)  # (it holds until changed: the last call counts)
        solver.begin_dual_bounded(basis)
        assert solver.record()["dual_long_step"] is False
        for step, (q, p, leaving, _) in enumerate(reference.pivots[:8]):
            before = int(solver.stats().launches)
            assert solver.iterate_dual(1) == (1, relp_amd.STOP_BUDGET), step
            assert int(solver.stats().launches) - before == 1 + 5
            assert solver.last_pivot() == (3, q, p, leaving) and set(solver.basis()) == set(bases[step]), step
        before = int(solver.stats().launches)
        count = len(reference.pivots) - 8
        assert solver.iterate_dual(count) == (count, relp_amd.STOP_BUDGET)
        assert int(solver.stats().launches) - before == 1 + 5 * count  # (one batch: pivots_per_launch is larger)
        assert set(solver.basis()) == set(bases[-1])
        assert solver.iterate_dual(1) == (0, relp_amd.STOP_NO_ENTERING)
        record = solver.record()
        assert record["dual_flips"] == 0 and record["dual_long_step_skipped"] == 0 and record["dual_pivots"] == len(reference.pivots)
    finally:
        solver.close()


def test_the_switch_takes_0_and_1_only():
    _, _, child, basis, _, _ = lps.long_step_case(5)
    solver = relp_amd.Solver(implicit_bounds=1).load_model(child.model)
    try:
        solver.set_dual_long_step(1)
        for value in (2, -1):
            with pytest.raises(RelpError, match="0 or 1") as refused:
                solver.set_dual_long_step(value)
            assert refused.value.status == ERR_ARGUMENT
        solver.begin_dual_bounded(basis)
        assert solver.record()["dual_long_step"] is True  # (a refused value changes nothing)
    finally:
        solver.close()


def test_the_plain_entry_points_refuse_while_the_switch_is_on_and_an_unbounded_plan_ignores_it():
    seed, n_cuts = dual_lps.WALK_CASES[64]
    case = dual_lps.cut_case(64, dual_lps.MIXED, seed, n_cuts)
    child, basis, _ = case.child(*dual_lps.solved_parent(case))
    solver = relp_amd.Solver(certify=1).load_model(child)  # (no bound: the plan the plain loop takes)
    other = relp_amd.Solver().load_model(child)
    try:
        solver.set_dual_long_step(True)
        before = int(solver.stats().launches)
        for call in (lambda: solver.begin_dual(basis), lambda: solver.solve_dual(basis), lambda: solver.begin_dual_from(other, basis)):
            with pytest.raises(RelpError, match="long-step ratio test is switched on") as refused:
                call()
            assert refused.value.status == ERR_ARGUMENT
        assert int(solver.stats().launches) == before
        result = solver.solve_dual_bounded(basis)  # the bounded entry on a plan without bounds: the plain kernels, the switch changes nothing
        assert result.kind == relp_amd.FINITE_OPTIMUM and result.certified == 1
        record = solver.record()
        assert record["dual_bounded"] is False and record["dual_long_step"] is False and record["dual_flips"] == 0
        with_switch = (solver.dual_pivots(), tuple(solver.basis()), solver.objective_exact())
        solver.set_dual_long_step(False)
        result = solver.solve_dual(basis)
        assert result.kind == relp_amd.FINITE_OPTIMUM and result.certified == 1
        assert (solver.dual_pivots(), tuple(solver.basis()), solver.objective_exact()) == with_switch and with_switch[0] >= 8
    finally:
        solver.close()
        other.close()
