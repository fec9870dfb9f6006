"""The exact proof of an INFEASIBLE child of the dual simplex (``-m gpu``, a real MI355X): ``Solver.set_dual_farkas`` /
``solve_dual*(..., farkas=True)`` with ``certify=1``.

Where the loop ends dual unbounded at a row p of its basis, row p of the exact inverse is the Farkas vector up to its sign.  Every check
here is an equality or a sign test over ``Fraction``: the witness against the model (``relp_amd.witness.check_infeasible``: y'a_j <= 0
for every column, y'b = the exact objective > 0), against the exact inverse of the basis the reference walk of tests/dual_lps.py ends
on, and -- on implicit bounds, where the basis spans the constraint rows only -- the entries on the bound rows against the closed form
y_br(j) = -max(0, y_c'a_j), recomputed here from the child's own data.  Nothing is compared under a tolerance.

Every test but the last asserts ``certified == 1`` for an INFEASIBLE result of the dual loop, which no handle gave before the switch
existed; the last one needs the keyword.
"""
from fractions import Fraction

import pytest

import relp_amd
from relp_amd import WITNESS_DUAL, WITNESS_PRIMAL, WITNESS_RAY
from relp_amd.api import ERR_ARGUMENT, ERR_STATE, RelpError
from relp_amd.witness import check_infeasible
import dual_bounded_lps
import dual_lps

pytestmark = pytest.mark.gpu

UNPROVED = "does not certify infeasibility"


def last_error(solver):
    return relp_amd.lib().relp_last_error(solver._h).decode()


def proved(solver, result, model):
    """The assertions every proved verdict shares; returns ``(y, value)``."""
    assert result.kind == relp_amd.INFEASIBLE and result.certified == 1, (result.kind, result.certified, last_error(solver))
    assert result.certify_seconds > 0.0
    record = solver.record()
    assert record["dual_farkas"] is True and 0 <= record["dual_farkas_row"] < record["device_rows"] and record["certified"] is True
    y, value = solver.witness_exact(WITNESS_DUAL), Fraction(solver.objective_exact())
    assert record["objective_exact"] == solver.objective_exact()
    check_infeasible(model, y, value)
    assert solver.witness_exact(WITNESS_DUAL) == y  # (a second read scales nothing again)
    for which in (WITNESS_PRIMAL, WITNESS_RAY):  # not defined for this result, as for a cold INFEASIBLE
        with pytest.raises(RelpError) as refused:
            solver.witness_exact(which)
        assert refused.value.status == ERR_STATE
    return y, value


def test_the_hand_case_without_bounds():
    # minimise x with x <= 2 and x >= 3: x + s = 2, x - t = 3
    model = relp_amd.Model.from_general_form([[(0, 1), (1, 1)]], ["Less", "Greater"], [2, 3], [(1, 0, None)])
    assert model.right_hand_side_exact() == [2, 3] and model.nr_columns == 3
    solver = relp_amd.Solver(certify=1).load_model(model)
    try:
        result = solver.solve_dual([1, 2], farkas=True)  # the slack basis: t = -3; x enters on row 1, then row 0 has s = -1 and no candidate
        y, value = proved(solver, result, model)
        assert solver.dual_pivots() == 1 and list(solver.basis()) == [1, 0]
        assert y == {0: Fraction(-1), 1: Fraction(1)} and value == 1 and solver.objective_exact() == "1/1"
        assert solver.record()["dual_farkas_row"] == 0
        check_infeasible(model, y, 1)
    finally:
        solver.close()


def test_the_hand_case_on_implicit_bounds():
    # minimise x with x >= 3 and the bound x <= 2: x - t = 3 on the constraint row, x + s = 2 on the bound row
    model = relp_amd.Model.from_general_form([[(0, 1)]], ["Greater"], [3], [(1, 0, 2)])
    assert model.right_hand_side_exact() == [3, 2] and model.nr_columns == 3  # the constraint row is row 0, the bound row is row 1
    solver = relp_amd.Solver(certify=1, implicit_bounds=1).load_model(model)
    try:
        result = solver.solve_dual_bounded([1, 2], farkas=True)
        y, value = proved(solver, result, model)
        assert solver.record()["dual_bounded"] is True and solver.record()["device_rows"] == 1
        assert y == {0: Fraction(1), 1: Fraction(-1)} and value == 1
        check_infeasible(model, y, 1)
    finally:
        solver.close()


def plain_child(m):
    seed, _ = dual_lps.WALK_CASES[m]
    case = dual_lps.cut_case(m, dual_lps.MIXED, seed, 0)
    parent_basis, vertex = dual_lps.solved_parent(case)
    child, basis = dual_lps.infeasible_child(case, parent_basis, vertex)
    assert child.right_hand_side_exact() == list(case.b) + [0, 1]  # standardisation kept the rows in order
    return case, parent_basis, child, basis


def test_64_rows_against_the_exact_inverse_of_the_reference_walk_and_through_the_parent():
    case, parent_basis, child, basis = plain_child(64)
    reference = dual_lps.DualReference(child, basis)
    assert reference.run() == relp_amd.STOP_UNBOUNDED
    solver = relp_amd.Solver(certify=1).load_model(child)
    try:
        result = solver.solve_dual(basis, farkas=True)
        y, value = proved(solver, result, child)
        assert list(solver.basis()) == reference.basis and solver.dual_pivots() == len(reference.pivots)
        p = solver.record()["dual_farkas_row"]
        rows = [i for i in range(reference.m) if y == {k: -v for k, v in enumerate(reference.inverse[i]) if v} and value == -reference.x[i]]
        assert rows == [p], (rows, p)
        assert reference.x[p] < 0
    finally:
        solver.close()
    assert child.dual_inherit_refusal(case.parent, parent_basis, basis) == ""
    parent = relp_amd.Solver(certify=1).load_model(case.parent)
    inherited = relp_amd.Solver(certify=1).load_model(child)
    try:
        assert parent.solve_relaxation().kind == relp_amd.FINITE_OPTIMUM
        result = inherited.solve_dual_from(parent, basis, farkas=True)
        assert inherited.record()["dual_start"] == "inherited"
        assert proved(inherited, result, child) == (y, value)
    finally:
        inherited.close()
        parent.close()
    print("m = 64 + 2 rows: %d dual pivots, row %d, y with %d entries, y'b = %s" % (len(reference.pivots), p, len(y), value))


def test_65_rows_one_past_a_wave():
    _, _, child, basis = plain_child(65)
    solver = relp_amd.Solver(certify=1).load_model(child)
    try:
        result = solver.solve_dual(basis, farkas=True)
        proved(solver, result, child)
    finally:
        solver.close()


def assert_closed_form(child, y, value):
    """The entries of ``y`` on the bound rows are ``-max(0, r_j)`` with ``r_j = y_c'a_j`` over the constraint rows, a column without a
    bound row has ``r_j <= 0``, and ``value = y_c'b_c - sum_j max(0, r_j) u_j``: recomputed from the child's own data."""
    y_c = [y.get(i, Fraction(0)) for i in range(child.m)]
    expected = sum((y_c[i] * child.b[i] for i in range(child.m)), Fraction(0))
    bound_rows = {}
    for j in range(child.n_device):
        r = sum((v * y_c[i] for i, v in child.device_column(j)), Fraction(0))
        if j in child.bound_row:
            if r > 0:
                bound_rows[child.bound_row[j]] = -r
                expected -= r * child.upper[j]
        else:
            assert r <= 0, ("a column without a bound prices positive", j, r)
    assert {i: v for i, v in y.items() if i >= child.m} == bound_rows
    assert value == expected and value > 0


@pytest.mark.parametrize("variant", ["plain rule", "long step", "steepest edge", "from the parent"])
def test_64_rows_on_implicit_bounds_and_the_closed_form_over_the_bound_rows(variant):
    case, optimum, child, basis = dual_bounded_lps.infeasible_child(64)
    fixed = [j for j in child.bounded if child.upper[j] == 0]
    assert len(fixed) >= 2  # (the fixed-column case: u_j = 0 costs nothing on its bound row)
    options = {"dual_pricing": 1} if variant == "steepest edge" else {}
    solver = relp_amd.Solver(certify=1, implicit_bounds=1, **options).load_model(child.model)
    parent = None
    try:
        if variant == "from the parent":
            assert child.model.dual_bounded_inherit_refusal(case.parent.model, optimum.basis, basis, implicit_bounds=1) == ""
            parent = relp_amd.Solver(implicit_bounds=1).load_model(case.parent.model)
            parent.set_basis(optimum.basis)
            result = solver.solve_dual_bounded_from(parent, basis, farkas=True)
            assert solver.record()["dual_start"] == "inherited"
        else:
            result = solver.solve_dual_bounded(basis, long_step=variant == "long step", farkas=True)
        record = solver.record()
        assert record["dual_bounded"] is True and record["device_rows"] == child.m and record["dual_long_step"] is (variant == "long step")
        y, value = proved(solver, result, child.model)
        assert_closed_form(child, y, value)
        print("m = %d constraint rows, %s: %d dual pivots, row %d, %d bound rows of %d in y, y'b = %s" % (
            child.m, variant, solver.dual_pivots(), record["dual_farkas_row"], sum(i >= child.m for i in y), len(child.bounded), value))
    finally:
        solver.close()
        if parent is not None:
            parent.close()


def test_off_by_default_off_again_and_without_the_certificate():
    _, _, child, basis = plain_child(64)
    solver = relp_amd.Solver(certify=1).load_model(child)
    try:
        result = solver.solve_dual(basis)  # a new handle
        assert result.kind == relp_amd.INFEASIBLE and result.certified == 0 and UNPROVED in last_error(solver)
        assert solver.record()["dual_farkas"] is False and solver.record()["dual_farkas_row"] == -1
        result = solver.solve_dual(basis, farkas=True)
        assert result.certified == 1 and solver.record()["dual_farkas"] is True and solver.record()["dual_farkas_row"] >= 0
        result = solver.solve_dual(basis)  # None keeps the handle's setting
        assert result.certified == 1 and solver.record()["dual_farkas"] is True
        launches = int(solver.stats().launches)
        result = solver.solve_dual(basis, farkas=False)
        assert result.kind == relp_amd.INFEASIBLE and result.certified == 0 and UNPROVED in last_error(solver)
        assert solver.record()["dual_farkas"] is False and solver.record()["dual_farkas_row"] == -1
        off = int(solver.stats().launches) - launches
        with pytest.raises(RelpError) as refused:
            solver.witness_exact(WITNESS_DUAL)
        assert refused.value.status == ERR_STATE
        for on in (2, -1):  # the switch is 0 or 1; a refused value changes nothing
            assert relp_amd.lib().relp_set_dual_farkas(solver._h, on) == ERR_ARGUMENT
            assert "relp_set_dual_farkas: the switch is 0 or 1" in last_error(solver)
        assert solver.solve_dual(basis).certified == 0
        solver.set_dual_farkas(True)
        launches = int(solver.stats().launches)
        assert solver.solve_dual(basis).certified == 1
        assert int(solver.stats().launches) - launches == off + 1  # the pivot loop's launches, and the leaving-row kernel once more
    finally:
        solver.close()
    uncertified = relp_amd.Solver(certify=0).load_model(child)
    try:
        result = uncertified.solve_dual(basis, farkas=True)
        assert result.kind == relp_amd.INFEASIBLE and result.certified == 0 and UNPROVED in last_error(uncertified)
        assert uncertified.record()["dual_farkas"] is True and uncertified.record()["dual_farkas_row"] == -1
        with pytest.raises(RelpError) as refused:
            uncertified.witness_exact(WITNESS_DUAL)
        assert refused.value.status == ERR_STATE
    finally:
        uncertified.close()


def test_a_feasible_child_is_untouched_by_the_switch():
    m = 64
    seed, n_cuts = dual_lps.WALK_CASES[m]
    case = dual_lps.cut_case(m, dual_lps.MIXED, seed, n_cuts)
    child, basis, _ = case.child(*dual_lps.solved_parent(case))
    seen = []
    for farkas in (False, True):
        solver = relp_amd.Solver(certify=1).load_model(child)
        try:
            result = solver.solve_dual(basis, farkas=farkas)
            assert solver.record()["dual_farkas"] is farkas and solver.record()["dual_farkas_row"] == -1
            seen.append((result.kind, result.certified, solver.dual_pivots(), result.pivots_phase_one, result.pivots_phase_two, solver.objective_exact(),
                         int(solver.stats().launches)))
        finally:
            solver.close()
    assert seen[0] == seen[1] and seen[0][:2] == (relp_amd.FINITE_OPTIMUM, 1)
