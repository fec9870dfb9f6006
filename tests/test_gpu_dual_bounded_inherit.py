"""The dual simplex on implicit upper bounds started from the parent's inverse (``-m gpu``, a real MI355X):
``begin_dual_bounded_from`` / ``solve_dual_bounded_from`` against the exact reference of tests/dual_bounded_lps.py.

Border and walk (m = 5, 64, 65): the parent handle gets the oracle's optimal basis through ``set_basis``, the child is
``walk_case(m)`` -- cuts, tightened bounds, one new bound row.  Two generations: the handle that walked the first-generation child
is the parent of a grandchild built from its ``basis()`` (tests/dual_bounded_inherit_lps.py); it holds a basic column complemented and
the grandchild's basis is passed in column order, so the kernel's map and signs are both in force.  A parent solved cold on the
device: its positions are the device's own.  m = 513: residuals of the held representation.  The state is compared at 0 pivots -- what
the kernel and the guard wrote, every row of the inverse, the k rows of the new slacks included -- and after the walk, at the
tolerances of tests/state_checks.py and tests/residual_checks.py.
"""
from fractions import Fraction

import numpy as np
import pytest

import relp_amd
from relp_amd.api import CARRY_LU, ERR_ARGUMENT, ERR_STATE, RelpError
import dual_bounded_inherit_lps as gen
import dual_bounded_lps as lps
from state_checks import TOLERANCE
from test_gpu_dual_bounded import assert_conditions, assert_held_state, cold_exact, walk_on_the_device

pytestmark = pytest.mark.gpu


def parent_with_basis(form, basis, **options):
    """A handle on implicit bounds that holds ``form`` at ``basis`` (of the formulation), inverse and all."""
    solver = relp_amd.Solver(implicit_bounds=1, **options).load_model(form.model)
    try:
        solver.set_basis(basis)
        return solver
    except BaseException:
        solver.close()
        raise


def assert_inherited(solver, label):
    record = solver.record()
    assert record["dual_start"] == "inherited" and record["dual_start_gemms"] <= 2 and record["dual_bounded"] is True, record
    assert solver.dual_pivots() == 0
    print("%s: guard residual %.2e, %d GEMMs, %d complemented, %d moved, %.3f ms" % (
        label, record["dual_start_residual"], record["dual_start_gemms"], record["dual_inherit_complemented"], record["dual_inherit_moved"],
        1e3 * record["dual_start_seconds"]))
    return record


def walk_to_the_end(solver, reference):
    """``iterate_dual(1)`` against ``reference.step()`` until the reference stops, as ``walk_on_the_device`` does."""
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


@pytest.mark.parametrize("m", sorted(lps.WALK_CASES))
def test_the_border_at_zero_pivots_and_the_walk(m):
    case, optimum, child, basis, cuts, _ = lps.walk_case(m)
    assert_conditions(m)
    assert child.m == case.parent.m + len(cuts) and len(cuts) >= 1
    parent = parent_with_basis(case.parent, optimum.basis)
    solver = relp_amd.Solver(implicit_bounds=1, polish_period=0).load_model(child.model)
    try:
        solver.begin_dual_bounded_from(parent, basis)
        record = assert_inherited(solver, "m = %d + %d cuts" % (m, len(cuts)))
        assert record["dual_inherit_complemented"] == 0  # (set_basis holds no basic column complemented)
        reference = lps.BoundedDualReference(child, basis)
        assert set(solver.basis()) == set(reference.formulation_basis())
        assert_held_state(solver, reference, "m = %d, inherited state at 0 pivots" % m)
        walk_to_the_end(solver, reference)
        assert_held_state(solver, reference, "m = %d, state after %d dual pivots" % (m, len(reference.pivots)))
    finally:
        solver.close()
    fresh = relp_amd.Solver(certify=1, implicit_bounds=1).load_model(child.model)
    try:
        result = fresh.solve_dual_bounded_from(parent, basis)
        assert result.kind == relp_amd.FINITE_OPTIMUM and result.certified == 1
        assert fresh.record()["dual_start"] == "inherited" and fresh.dual_pivots() == len(reference.pivots)
        warm = fresh.objective_exact()
    finally:
        fresh.close()
        parent.close()
    cold, _ = cold_exact(child.model, implicit_bounds=1)
    assert Fraction(warm) == Fraction(cold) == reference.objective()


def test_two_generations_the_map_and_the_signs():
    first, first_reference = walk_on_the_device(gen.FIRST_M)  # (the first-generation child, walked: polish_period = 0)
    solver = None
    try:
        child = lps.walk_case(gen.FIRST_M)[2]
        assert gen.complemented_basic(first_reference) >= 1
        form, basis, cuts, branches = gen.grandchild(child, first.basis(), first_reference.solution())
        check = lps.BoundedDualReference(form, basis)
        assert gen.moved_positions(first_reference, check) >= 1
        reason, facts, _ = lps.walk(check)
        lps.assert_walk_conditions(check, gen.FIRST_M, reason, facts)
        reference = lps.BoundedDualReference(form, basis)
        solver = relp_amd.Solver(implicit_bounds=1, polish_period=0).load_model(form.model)
        solver.begin_dual_bounded_from(first, basis)
        record = assert_inherited(solver, "grandchild, m = %d + %d cuts" % (child.m, len(cuts)))
        assert record["dual_inherit_complemented"] >= 1 and record["dual_inherit_moved"] >= 1, record
        assert record["dual_inherit_complemented"] == gen.complemented_basic(first_reference)
        assert record["dual_inherit_moved"] == gen.moved_positions(first_reference, check)
        assert_held_state(solver, reference, "grandchild, inherited state at 0 pivots")
        walk_to_the_end(solver, reference)
        assert_held_state(solver, reference, "grandchild, state after %d dual pivots" % len(reference.pivots))
        # the next start of the same handle from scratch reports neither
        solver.begin_dual_bounded(basis)
        record = solver.record()
        assert (record["dual_start"], record["dual_inherit_complemented"], record["dual_inherit_moved"]) == ("scratch", 0, 0)
    finally:
        first.close()
        if solver is not None:
            solver.close()


def test_a_parent_solved_cold_on_the_device_and_a_pure_branch():
    m = 64
    case = lps.BoundedCase(m, lps.WALK_CASES[m][0], 0, lps.WALK_CASES[m][2])
    parent = relp_amd.Solver(certify=1, implicit_bounds=1).load_model(case.parent.model)
    solver = None
    try:
        result = parent.solve_relaxation()
        assert result.kind == relp_amd.FINITE_OPTIMUM and result.certified
        parent_objective = parent.objective_exact()
        child, basis, branches = gen.tightened_only(case, parent.basis(), parent.solution_exact())
        assert list(basis) == [int(c) for c in parent.basis()] and len(branches) == lps.WALK_CASES[m][2]
        reference = lps.BoundedDualReference(child, basis)
        solver = relp_amd.Solver(certify=1, implicit_bounds=1, polish_period=0).load_model(child.model)
        solver.begin_dual_bounded_from(parent, basis)
        assert_inherited(solver, "m = %d, k = 0, %d tightened bounds, parent solved cold" % (m, len(branches)))
        assert_held_state(solver, reference, "pure branch, inherited state at 0 pivots")
        result = solver.solve_dual_bounded_from(parent, basis)
        assert result.kind == relp_amd.FINITE_OPTIMUM and result.certified == 1 and solver.record()["dual_start"] == "inherited"
        assert solver.dual_pivots() >= 1
        warm = solver.objective_exact()
        cold, _ = cold_exact(child.model, implicit_bounds=1)
        assert Fraction(warm) == Fraction(cold)
        # the parent was only read: it solves again to its exact objective
        again = parent.solve_relaxation()
        assert again.kind == relp_amd.FINITE_OPTIMUM and again.certified and parent.objective_exact() == parent_objective
    finally:
        parent.close()
        if solver is not None:
            solver.close()


def test_a_state_case_of_513_rows():
    """(The parent's optimum is the certified device solve's, as in tests/test_gpu_dual_bounded.py; the parent handle stays open.)"""
    from residual_checks import assert_residuals
    from sparse_lps import btrans
    m, seed, n_cuts, n_tight = lps.STATE_CASE
    case = lps.BoundedCase(m, seed, n_cuts, n_tight)
    parent = relp_amd.Solver(certify=1, implicit_bounds=1).load_model(case.parent.model)
    solver = None
    try:
        result = parent.solve_relaxation()
        assert result.kind == relp_amd.FINITE_OPTIMUM and result.certified
        child, basis, cuts, branches = case.child(parent.basis(), parent.solution_exact())
        assert child.m == m + n_cuts and len(branches) == n_tight + 1
        solver = relp_amd.Solver(implicit_bounds=1).load_model(child.model)
        solver.begin_dual_bounded_from(parent, basis)
        assert_inherited(solver, "m = %d + %d cuts" % (m, n_cuts))
        for pivots in (0, 16):
            if pivots:
                done, _ = solver.iterate_dual(pivots)
                assert done >= 8 and solver.dual_pivots() == done
            handle, provider, state = lps.held_pair(solver, child)
            report = {}
            assert_residuals(handle, provider, btrans(child.m), report=report)
            # dual feasibility is kept: the signed cost of every non-basic column, at the tolerance of a relative cost
            signed = handle.relative_costs()
            free = np.ones(state.n, dtype=bool)
            free[state.held_basis] = False
            assert (signed[free] >= -TOLERANCE["costs"] * (1 + np.abs(signed[free]))).all(), ("signed relative cost", float(signed[free].min()))
            print("m = %d + %d cuts, inherited, after %d dual pivots (%d basic columns held complemented): %s; smallest signed cost %.1e" % (
                m, n_cuts, solver.dual_pivots(), state.complemented_basic, ", ".join("%s %.1e" % item for item in sorted(report.items())), float(signed[free].min())))
    finally:
        parent.close()
        if solver is not None:
            solver.close()


def test_the_long_step_switch_works_through_the_inherited_start():
    case, optimum, child, basis, _, _ = lps.walk_case(64)
    parent = parent_with_basis(case.parent, optimum.basis)
    outcomes = []
    try:
        for inherited in (False, True):
            solver = relp_amd.Solver(certify=1, implicit_bounds=1).load_model(child.model)
            try:
                result = solver.solve_dual_bounded_from(parent, basis, long_step=True) if inherited else solver.solve_dual_bounded(basis, long_step=True)
                assert result.kind == relp_amd.FINITE_OPTIMUM and result.certified == 1
                record = solver.record()
                assert record["dual_long_step"] is True and record["dual_start"] == ("inherited" if inherited else "scratch")
                outcomes.append((solver.objective_exact(), solver.dual_pivots(), record["dual_flips"], tuple(sorted(solver.basis()))))
            finally:
                solver.close()
    finally:
        parent.close()
    assert outcomes[0] == outcomes[1], outcomes


def test_refusals_come_before_any_launch_and_leave_a_handle_that_solves_cold():
    case, optimum, child, basis, _, _ = lps.walk_case(64)
    expected, _ = cold_exact(child.model, implicit_bounds=1)
    parent = parent_with_basis(case.parent, optimum.basis)
    bare = relp_amd.Solver(implicit_bounds=1).load_model(case.parent.model)  # loaded, no basis and inverse yet
    empty = relp_amd.Solver(implicit_bounds=1)  # no LP
    lu_parent = relp_amd.Solver(carry=CARRY_LU, implicit_bounds=1).load_model(case.parent.model)
    rows_parent = relp_amd.Solver(implicit_bounds=0).load_model(case.parent.model)
    solver = relp_amd.Solver(certify=1, implicit_bounds=1).load_model(child.model)
    try:
        before, parent_before = int(solver.stats().launches), int(parent.stats().launches)
        with_artificial = list(basis)
        with_artificial[child.rows - 1] = -1
        changed = list(basis)
        changed[child.m - 1] = next(j for j in range(child.ns) if j not in basis)  # a structural column of the parent's rows on a cut's row
        for call, status, words in (
                (lambda: solver.begin_dual_bounded_from(parent, with_artificial), ERR_ARGUMENT, "artificial"),
                (lambda: solver.begin_dual_bounded_from(parent, changed), ERR_ARGUMENT, "position"),
                (lambda: solver.begin_dual_bounded_from(lu_parent, basis), ERR_ARGUMENT, "the parent's plan"),
                (lambda: solver.begin_dual_bounded_from(rows_parent, basis), ERR_ARGUMENT, "rows of the device LP"),
                (lambda: solver.begin_dual_bounded_from(empty, basis), ERR_STATE, "no LP loaded"),
                (lambda: solver.begin_dual_bounded_from(bare, basis), ERR_STATE, "no basis and inverse yet"),
                (lambda: solver.solve_dual_bounded_from(solver, basis), ERR_STATE, "this handle itself")):
            with pytest.raises(RelpError, match=words) as refused:
                call()
            assert refused.value.status == status, (words, refused.value.status)
        with pytest.raises(RelpError, match="begin_dual comes first"):
            solver.iterate_dual(1)
        assert int(solver.stats().launches) == before and int(parent.stats().launches) == parent_before
        result = solver.solve_relaxation()
        assert result.kind == relp_amd.FINITE_OPTIMUM and result.certified and solver.objective_exact() == expected
    finally:
        for handle in (solver, parent, bare, empty, lu_parent, rows_parent):
            handle.close()
    lu_child = relp_amd.Solver(carry=CARRY_LU, implicit_bounds=1).load_model(child.model)
    parent = parent_with_basis(case.parent, optimum.basis)
    try:
        before = int(lu_child.stats().launches)
        with pytest.raises(RelpError, match="LU") as refused:
            lu_child.solve_dual_bounded_from(parent, basis)
        assert refused.value.status == ERR_ARGUMENT and int(lu_child.stats().launches) == before
    finally:
        lu_child.close()
        parent.close()


def test_the_plain_entry_points_still_refuse_a_bounded_plan():
    case, optimum, child, basis, _, _ = lps.walk_case(5)
    solver = relp_amd.Solver(implicit_bounds=1).load_model(child.model)
    other = parent_with_basis(case.parent, optimum.basis)
    try:
        for call in (lambda: solver.solve_dual(basis), lambda: solver.begin_dual(basis), lambda: solver.begin_dual_from(other, basis),
                     lambda: solver.solve_dual_from(other, basis)):
            with pytest.raises(RelpError, match="implicit upper bounds") as refused:
                call()
            assert refused.value.status == ERR_ARGUMENT
        solver.begin_dual_bounded_from(other, basis)  # ... and the new one takes the pair
        assert solver.record()["dual_start"] == "inherited"
    finally:
        solver.close()
        other.close()
