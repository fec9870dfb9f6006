"""The objective cutoff of the dual simplex and the exact proof of the bound it stops at (``-m gpu``, a real MI355X):
``Solver.set_dual_cutoff`` / ``solve_dual*(..., cutoff=c)`` with ``certify=1``.

Every basis of the dual loop is dual feasible, so its objective is a lower bound of the child.  With a cutoff the leaving-row kernel
stops the loop at the first basis whose objective has reached it, and the dual half of the optimum's certificate proves that bound.
Every check here is an equality or a sign test over ``Fraction``: the number of pivots, the basis, the exact bound and the dual vector
against the reference walks of tests/dual_lps.py and tests/dual_bounded_lps.py at that very basis, the witness against the model
(``relp_amd.witness.check_dual_bound``), and on implicit bounds the entries on the bound rows against the closed form min(0, d_j),
recomputed from the child's own data.  The cutoffs lie in the middle of a rise of the reference's objective that f64 cannot miss
(tests/dual_cutoff_lps.py; tests/test_dual_cutoff_host.py asserts the conditions on the CPU).  Nothing is compared under a tolerance.

Every test needs the setter, so every one fails on a library without it.
"""
import functools
import math
from fractions import Fraction

import pytest

import relp_amd
from relp_amd import WITNESS_DUAL, WITNESS_PRIMAL, WITNESS_RAY
from relp_amd.api import ERR_ARGUMENT, ERR_STATE, RelpError
from relp_amd.witness import check_dual_bound, check_infeasible
import dual_bounded_lps
import dual_cutoff_lps as lps
import dual_lps

pytestmark = pytest.mark.gpu


def last_error(solver):
    return relp_amd.lib().relp_last_error(solver._h).decode()


def proved(solver, result, model, kind=relp_amd.CUTOFF):
    """The assertions every proved bound shares; returns ``(y, value)``."""
    assert result.kind == kind and result.certified == 1, (result.kind, result.certified, last_error(solver))
    assert result.certify_seconds > 0.0 and math.isfinite(result.objective)
    record = solver.record()
    assert record["dual_bound_proved"] is True and record["certified"] is True and record["dual_cutoff"] is not None
    assert record["dual_cutoff_stopped"] is (kind == relp_amd.CUTOFF) and record["result"] == ("cutoff" if kind == relp_amd.CUTOFF else "iteration_limit")
    y, value = solver.witness_exact(WITNESS_DUAL), Fraction(solver.objective_exact())
    check_dual_bound(model, y, value)
    assert solver.witness_exact(WITNESS_DUAL) == y
    for which in (WITNESS_PRIMAL, WITNESS_RAY):  # a bound has no primal point and no ray
        with pytest.raises(RelpError) as refused:
            solver.witness_exact(which)
        assert refused.value.status == ERR_STATE
    return y, value


def plain_solver(model, **options):
    return relp_amd.Solver(certify=1, **options).load_model(model)


def bounded_solver(form, **options):
    return relp_amd.Solver(certify=1, implicit_bounds=1, **options).load_model(form.model)


@pytest.mark.parametrize("cutoff, pivots, y, value", [(5, 1, {1: 2}, 8), (0, 0, {}, 0), (11, 2, {0: -1, 1: 3}, 11)])
def test_the_plain_hand_case(cutoff, pivots, y, value):
    model, basis = lps.hand_plain()
    solver = plain_solver(model)
    try:
        result = solver.solve_dual(basis, cutoff=cutoff)
        assert proved(solver, result, model) == (y, value)
        assert solver.dual_pivots() == pivots and list(solver.basis()) == lps.HAND_PLAIN_BASES[pivots]
        assert solver.objective_exact() == "%d/1" % value and solver.record()["dual_cutoff"] == cutoff
        assert result.pivots_phase_two == 0  # no primal clean-up behind a cutoff
    finally:
        solver.close()


def test_a_cutoff_above_the_optimum_of_the_plain_hand_case_changes_nothing():
    model, basis = lps.hand_plain()
    seen = []
    for cutoff in (None, 12):
        solver = plain_solver(model)
        try:
            result = solver.solve_dual(basis, cutoff=cutoff)
            record = solver.record()
            assert record["dual_cutoff"] == cutoff and record["dual_cutoff_stopped"] is False and record["dual_bound_proved"] is False
            seen.append((result.kind, result.certified, solver.dual_pivots(), solver.objective_exact(), list(solver.basis()),
                         solver.witness_exact(WITNESS_DUAL), solver.witness_exact(WITNESS_PRIMAL)))
        finally:
            solver.close()
    assert seen[0] == seen[1] and seen[0][:5] == (relp_amd.FINITE_OPTIMUM, 1, 2, "11/1", lps.HAND_PLAIN_BASES[2])


@pytest.mark.parametrize("cutoff, pivots, y, value", [(5, 1, {0: 2}, 8), (11, 2, {0: 3, 1: -1}, 11)])
def test_the_bounded_hand_case(cutoff, pivots, y, value):
    form, basis = lps.hand_bounded()
    solver = bounded_solver(form)
    try:
        result = solver.solve_dual_bounded(basis, cutoff=cutoff)
        assert solver.record()["dual_bounded"] is True and solver.record()["device_rows"] == 1
        assert proved(solver, result, form.model) == (y, value)
        assert solver.dual_pivots() == pivots and set(solver.basis()) == set(lps.HAND_BOUNDED_BASES[pivots])
        assert lps.closed_form_value(form, y) == ({i: v for i, v in y.items() if i >= form.m}, value)
    finally:
        solver.close()


@functools.lru_cache(maxsize=None)
def walked(m, bounded, steepest=False):
    """``(model, formulation or None, basis, states, usable)`` of a walk case, the reference walked once per process."""
    if bounded:
        form, basis = lps.bounded_walk_case(m)
        reference = (dual_bounded_lps.SteepestBoundedDualReference if steepest else dual_bounded_lps.BoundedDualReference)(form, basis)
        model = form.model
    else:
        model, basis = lps.plain_walk_case(m)
        form, reference = None, dual_lps.DualReference(model, basis)
    states, usable = lps.walk_with_cutoffs(reference)
    return model, form, basis, states, usable


def assert_stopped_on(solver, result, model, form, state, k, cutoff, kind=relp_amd.CUTOFF):
    """The device stopped after ``k`` pivots on the reference's basis, and proved the reference's objective and dual vector there."""
    y, value = proved(solver, result, model, kind)
    assert solver.dual_pivots() == k, (solver.dual_pivots(), k)
    if form is None:
        assert list(solver.basis()) == state["basis"]
    else:
        assert set(solver.basis()) == set(state["basis"])
    assert value == state["objective"] + model.fixed_cost_exact()
    assert cutoff is None or value >= Fraction(cutoff)
    rows = len(state["pi"])
    assert {i: v for i, v in y.items() if i < rows} == {i: v for i, v in enumerate(state["pi"]) if v}
    if form is not None:
        assert lps.closed_form_value(form, y) == ({i: v for i, v in y.items() if i >= rows}, value)
    else:
        assert all(i < rows for i in y)
    return y, value


@pytest.mark.parametrize("m", sorted(dual_lps.WALK_CASES))
@pytest.mark.parametrize("bounded", [False, True], ids=["plain", "bounded"])
def test_the_walks_stop_at_the_first_a_middle_and_the_last_usable_pivot(m, bounded):
    model, form, basis, states, usable = walked(m, bounded)
    solver = bounded_solver(form) if bounded else plain_solver(model)
    try:
        for k, cutoff in lps.first_middle_last(usable):
            result = solver.solve_dual_bounded(basis, cutoff=cutoff) if bounded else solver.solve_dual(basis, cutoff=cutoff)
            y, value = assert_stopped_on(solver, result, model, form, states[k], k, cutoff)
            print("m = %d %s, cutoff %.17g: %d of %d dual pivots, bound %s (f64 %.17g), %d entries in y, proof %.1f ms" % (
                m, "bounded" if bounded else "plain", cutoff, k, len(states) - 1, value, result.objective, len(y), 1e3 * result.certify_seconds))
    finally:
        solver.close()


def test_64_rows_on_implicit_bounds_under_the_steepest_edge_rule():
    model, form, basis, states, usable = walked(64, True, steepest=True)
    k, cutoff = usable[len(usable) // 2]
    solver = bounded_solver(form, dual_pricing=relp_amd.api.DUAL_PRICING_STEEPEST_EDGE)
    try:
        result = solver.solve_dual_bounded(basis, cutoff=cutoff)
        assert_stopped_on(solver, result, model, form, states[k], k, cutoff)
    finally:
        solver.close()


def test_64_rows_on_implicit_bounds_with_the_long_step_and_from_the_parent():
    model, form, basis, states, usable = walked(64, True)
    k, cutoff = lps.first_middle_last(usable)[1]
    case, optimum, _, _, _, _ = dual_bounded_lps.walk_case(64)
    solver, parent = bounded_solver(form), None
    try:
        # the long step: the reference does not walk that rule; the bound against the closed form over the child's data alone
        result = solver.solve_dual_bounded(basis, long_step=True, cutoff=cutoff)
        assert solver.record()["dual_long_step"] is True
        y, value = proved(solver, result, model)
        assert value >= Fraction(cutoff)
        assert lps.closed_form_value(form, y) == ({i: v for i, v in y.items() if i >= form.m}, value)
        # from scratch, then from the parent's inverse: the same stop, the same proof
        result = solver.solve_dual_bounded(basis, long_step=False, cutoff=cutoff)
        scratch = assert_stopped_on(solver, result, model, form, states[k], k, cutoff)
        assert form.model.dual_bounded_inherit_refusal(case.parent.model, optimum.basis, basis, implicit_bounds=1) == ""
        parent = relp_amd.Solver(implicit_bounds=1).load_model(case.parent.model)
        parent.set_basis(optimum.basis)
        result = solver.solve_dual_bounded_from(parent, basis, cutoff=cutoff)
        assert solver.record()["dual_start"] == "inherited"
        assert assert_stopped_on(solver, result, model, form, states[k], k, cutoff) == scratch
    finally:
        solver.close()
        if parent is not None:
            parent.close()


@pytest.mark.parametrize("bounded", [False, True], ids=["plain", "bounded"])
def test_strong_branching_proves_the_bound_of_the_basis_the_iteration_limit_stopped_on(bounded):
    model, form, basis, states, _ = walked(64, bounded)
    for k in (1, (len(states) - 1) // 2):
        solver = bounded_solver(form, max_pivots=k) if bounded else plain_solver(model, max_pivots=k)
        try:
            solver.set_dual_cutoff(float("inf"))
            result = solver.solve_dual_bounded(basis) if bounded else solver.solve_dual(basis)
            assert solver.record()["dual_cutoff"] == "inf"
            assert_stopped_on(solver, result, model, form, states[k], k, None, kind=relp_amd.ITERATION_LIMIT)
        finally:
            solver.close()


def test_off_on_and_off_again_and_the_refused_arguments():
    model, _, basis, states, usable = walked(64, False)
    k, cutoff = usable[0]
    solver = plain_solver(model)

    def run(**keywords):
        before = int(solver.stats().launches)
        result = solver.solve_dual(basis, **keywords)
        record = solver.record()
        return (result.kind, result.certified, solver.dual_pivots(), result.pivots_phase_two, solver.objective_exact(), list(solver.basis()),
                record["dual_cutoff"], record["dual_cutoff_stopped"], record["dual_bound_proved"], int(solver.stats().launches) - before)
    try:
        run()
        never_set = run()  # (the second solve of the handle, like the last one below: the first also sizes the loop's buffers)
        assert never_set[:2] == (relp_amd.FINITE_OPTIMUM, 1) and never_set[6:9] == (None, False, False)
        stopped = run(cutoff=cutoff)
        assert stopped[:3] == (relp_amd.CUTOFF, 1, k) and stopped[6:9] == (cutoff, True, True)
        assert run()[:3] == stopped[:3]  # None keeps the handle's setting
        solver.set_dual_cutoff(None)
        assert run() == never_set
        # the switch is 0 or 1 and the cutoff a number; a refused call changes nothing
        lib = relp_amd.lib()
        assert lib.relp_set_dual_cutoff(solver._h, 2, 1.0) == ERR_ARGUMENT and "relp_set_dual_cutoff: the switch is 0 or 1" in last_error(solver)
        assert lib.relp_set_dual_cutoff(solver._h, 1, math.nan) == ERR_ARGUMENT and "relp_set_dual_cutoff: the cutoff is NaN" in last_error(solver)
        with pytest.raises(RelpError) as refused:
            solver.set_dual_cutoff(math.nan)
        assert refused.value.status == ERR_ARGUMENT
        assert run() == never_set
    finally:
        solver.close()


def test_without_the_certificate_the_loop_stops_and_nothing_is_certified():
    model, _, basis, states, usable = walked(64, False)
    k, cutoff = usable[len(usable) // 2]
    solver = relp_amd.Solver(certify=0).load_model(model)
    try:
        result = solver.solve_dual(basis, cutoff=cutoff)
        assert result.kind == relp_amd.CUTOFF and result.certified == 0 and solver.dual_pivots() == k and list(solver.basis()) == states[k]["basis"]
        assert result.objective >= cutoff
        record = solver.record()
        assert record["dual_cutoff_stopped"] is True and record["dual_bound_proved"] is False
        with pytest.raises(RelpError) as refused:
            solver.witness_exact(WITNESS_DUAL)
        assert refused.value.status == ERR_STATE
    finally:
        solver.close()


def test_an_infeasible_child_is_still_proved_infeasible_under_a_cutoff():
    seed, _ = dual_lps.WALK_CASES[64]
    case = dual_lps.cut_case(64, dual_lps.MIXED, seed, 0)
    child, basis = dual_lps.infeasible_child(case, *dual_lps.solved_parent(case))
    seen = []
    for cutoff in (None, float("inf")):
        solver = plain_solver(child)
        try:
            result = solver.solve_dual(basis, farkas=True, cutoff=cutoff)
            assert result.kind == relp_amd.INFEASIBLE and result.certified == 1, last_error(solver)
            record = solver.record()
            assert record["dual_farkas_row"] >= 0 and record["dual_cutoff_stopped"] is False and record["dual_bound_proved"] is False
            y, value = solver.witness_exact(WITNESS_DUAL), Fraction(solver.objective_exact())
            check_infeasible(child, y, value)
            seen.append((solver.dual_pivots(), list(solver.basis()), record["dual_farkas_row"], y, value))
        finally:
            solver.close()
    assert seen[0] == seen[1]


def test_the_stepwise_loop_stops_with_the_cutoffs_reason():
    model, _, basis, states, usable = walked(64, False)
    k, cutoff = usable[1]
    solver = relp_amd.Solver().load_model(model)
    try:
        solver.set_dual_cutoff(cutoff)
        solver.begin_dual(basis)
        assert solver.iterate_dual(1000) == (k, relp_amd.STOP_CUTOFF) and relp_amd.STOP_CUTOFF == 6
        assert solver.iterate_dual(1) == (0, relp_amd.STOP_CUTOFF)
        assert list(solver.basis()) == states[k]["basis"] and solver.record()["dual_cutoff_stopped"] is True
        solver.set_dual_cutoff(None)  # read by the next start, which walks to the end
        solver.begin_dual(basis)
        assert solver.iterate_dual(1000) == (len(states) - 1, relp_amd.STOP_NO_ENTERING)
    finally:
        solver.close()
