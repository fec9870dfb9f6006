"""The independent checker of exact witnesses (``relp_amd/witness.py``) and the exact model accessors it reads.  CPU only.

The checker is the judge of tests/test_gpu_witness.py, so it is tried here first on LPs small enough to solve by hand: it accepts
their true witnesses and rejects each of them falsified in one place, with the reason.
"""
import os
from fractions import Fraction as F

import pytest

import relp_amd
from relp_amd.witness import WitnessError, check_infeasible, check_optimum, check_unbounded
from relp_oracle.mps import load_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def slack_of_row(model, row):
    """The slack column of `row`: the one column past the structural ones whose only entry lies there."""
    found = [j for j in range(model.nr_structural, model.nr_columns) if [i for i, _, _ in model.column_exact(j)] == [row]]
    assert len(found) == 1, (row, found)
    return found[0]


def rejected(check, *args):
    with pytest.raises(WitnessError) as info:
        check(*args)
    return info.value


# ---- 1. the checker is not vacuous -----------------------------------------------------------------------------------------------
def optimum_lp():
    """min x + 2y - z + 1/2 with x + z = 3, y + z <= 4, y >= 2.  x = 3 - z turns the cost into 7/2 + 2y - 2z: y = 2 and z = 2 (row 1),
    so x = 1 and the optimum is 7/2.  Duals from the three basic columns: y0 = c_x = 1, y1 = c_z - y0 = -2, y2 = c_y - y1 = 4; the slack
    of row 1 prices at -y1 = 2 and the surplus of row 2 (entry -1) at y2 = 4.  y'b = 3 - 8 + 8 = 3."""
    model = relp_amd.Model.from_general_form([[(0, 1)], [(1, 1), (2, 1)], [(0, 1), (1, 1)]], ["Equal", "Less", "Greater"], [3, 4, 2],
                                             [(1, 0, None), (2, 0, None), (-1, 0, None)], fixed_cost=F(1, 2))
    return model, {0: F(1), 1: F(2), 2: F(2)}, {0: F(1), 1: F(-2), 2: F(4)}, F(7, 2)


def test_checker_accepts_a_hand_computed_optimum_and_rejects_each_falsification():
    model, x, y, objective = optimum_lp()
    assert (model.nr_rows, model.nr_structural, model.nr_columns) == (3, 3, 5)
    check_optimum(model, x, y, objective)
    error = rejected(check_optimum, model, {**x, 0: x[0] + F(1, 7)}, y, objective)  # x off by 1/7: row 0 reads 22/7
    assert (error.condition, error.where) == ("A x = b", ("row", 0))
    surplus = slack_of_row(model, 2)
    assert model.column_exact(surplus) == [(2, -1, 1)]
    error = rejected(check_optimum, model, x, {**y, 2: -y[2]}, objective)  # y2 = -4: column y prices at 8, the surplus of row 2 at -4
    assert (error.condition, error.where) == ("c_j - y'a_j >= 0", ("column", surplus))
    error = rejected(check_optimum, model, x, y, objective + 1)
    assert (error.condition, error.where) == ("c'x + fixed cost = objective", None)
    error = rejected(check_optimum, model, x, {**y, 0: F(0)}, objective)  # dual feasible still (c_x - 0 = 1, c_z - 0 + 2 = 1), but y'b = 0
    assert (error.condition, error.where) == ("y'b + fixed cost = objective", None)
    error = rejected(check_optimum, model, {**x, 0: F(-1), 2: F(4)}, y, objective)  # A x = b along x + z = 3, x negative
    assert (error.condition, error.where) == ("x >= 0", ("column", 0))
    error = rejected(check_optimum, model, {**x, 7: F(1)}, y, objective)
    assert error.where == ("column", 7)


def infeasible_lp():
    """x + y <= 2 and x >= 3.  y = (-1, 1): column x prices at 0, column y at -1, the slack of row 0 at -1, the surplus of row 1 (entry
    -1) at -1, and y'b = -2 + 3 = 1."""
    model = relp_amd.Model.from_general_form([[(0, 1), (1, 1)], [(0, 1)]], ["Less", "Greater"], [2, 3], [(0, 0, None), (0, 0, None)])
    return model, {0: F(-1), 1: F(1)}, F(1)


def test_checker_accepts_a_hand_computed_farkas_vector_and_rejects_each_falsification():
    model, y, value = infeasible_lp()
    check_infeasible(model, y, value)
    error = rejected(check_infeasible, model, {**y, 0: -y[0]}, value)  # y0 = 1: column x prices at 2
    assert (error.condition, error.where) == ("y'a_j <= 0", ("column", 0))
    error = rejected(check_infeasible, model, y, value + 1)
    assert (error.condition, error.where) == ("y'b = value", None)
    error = rejected(check_infeasible, model, {}, F(0))  # y = 0 satisfies every inequality and proves nothing
    assert (error.condition, error.where) == ("y'b > 0", None)
    error = rejected(check_infeasible, model, {**y, 1: y[1] + F(1, 7)}, value)  # y1 = 8/7: column x prices at 1/7
    assert (error.condition, error.where) == ("y'a_j <= 0", ("column", 0))


def unbounded_lp():
    """min -x - y with x - y <= 1, y >= 1.  (x, y) = (0, 1) is feasible with slack 2 on row 0 and surplus 0 on row 1; along d = (1, 1)
    row 0 does not move and the surplus of row 1 grows by 1; c'd = -2."""
    model = relp_amd.Model.from_general_form([[(0, 1)], [(0, -1), (1, 1)]], ["Less", "Greater"], [1, 1], [(-1, 0, None), (-1, 0, None)])
    slack, surplus = slack_of_row(model, 0), slack_of_row(model, 1)
    return model, {1: F(1), slack: F(2)}, {0: F(1), 1: F(1), surplus: F(1)}, surplus


def test_checker_accepts_a_hand_computed_ray_and_rejects_each_falsification():
    model, x, ray, surplus = unbounded_lp()
    check_unbounded(model, x, ray)
    dropped = {j: v for j, v in ray.items() if j != surplus}  # a ray with one entry dropped: row 1 moves
    error = rejected(check_unbounded, model, x, dropped)
    assert (error.condition, error.where) == ("A ray = 0", ("row", 1))
    error = rejected(check_unbounded, model, {**x, 1: x[1] + F(1, 7)}, ray)  # x off by 1/7: row 0 reads 0 - 8/7 + 2
    assert (error.condition, error.where) == ("A x = b", ("row", 0))
    error = rejected(check_unbounded, model, x, {j: -v for j, v in ray.items()})
    assert (error.condition, error.where) == ("ray >= 0", ("column", 0))
    error = rejected(check_unbounded, model, x, {})  # d = 0 keeps x feasible and goes nowhere
    assert (error.condition, error.where) == ("c'ray < 0", None)


# ---- 2. the exact model accessors ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["AFIRO", "SC50A", "ADLITTLE"])
def test_exact_model_accessors_equal_the_oracle_standard_form_and_the_f64_accessors(name):
    path = os.path.join(ROOT, "data", "netlib", name + ".SIF")
    general, data = load_problem(path)
    model = relp_amd.Model(path)
    assert (model.nr_rows, model.nr_columns) == (data.nr_rows(), data.nr_columns())
    costs = [model.cost_exact(j) for j in range(model.nr_columns)]
    assert costs == [F(data.cost_value(j)) for j in range(model.nr_columns)]
    assert [float(c) for c in costs] == [model.cost_value(j) for j in range(model.nr_columns)]
    rhs = model.right_hand_side_exact()
    assert rhs == [F(v) for v in data.right_hand_side()]
    assert [float(v) for v in rhs] == list(model.right_hand_side())
    assert model.fixed_cost_exact() == F(general.fixed_cost) and float(model.fixed_cost_exact()) == model.fixed_cost()
    assert any(c != 0 for c in costs) and any(v != 0 for v in rhs)


def test_exact_accessors_of_a_model_with_fractions_and_a_fixed_cost():
    model, _, _, _ = optimum_lp()
    assert [model.cost_exact(j) for j in range(model.nr_columns)] == [1, 2, -1, 0, 0]
    assert model.right_hand_side_exact() == [3, 4, 2] and model.fixed_cost_exact() == F(1, 2)
    thirds = relp_amd.Model.from_general_form([[(0, (1, 3))]], ["Less"], [(5, 7)], [((-2, 9), 0, None)], fixed_cost=(-4, 11))
    assert thirds.cost_exact(0) == F(-2, 9) and thirds.right_hand_side_exact() == [F(5, 7)] and thirds.fixed_cost_exact() == F(-4, 11)
    with pytest.raises(relp_amd.RelpError) as info:
        model.cost_exact(model.nr_columns)
    assert info.value.status == relp_amd.api.ERR_ARGUMENT


# ---- 3. exports --------------------------------------------------------------------------------------------------------------
def test_the_new_symbols_are_exported():
    assert (relp_amd.WITNESS_PRIMAL, relp_amd.WITNESS_DUAL, relp_amd.WITNESS_RAY) == (0, 1, 2)
    for symbol in ("relp_get_witness_exact", "relp_many_keep_witnesses", "relp_many_get_witness_exact", "relp_many_get_solution_exact",
                   "relp_model_cost_exact", "relp_model_right_hand_side_exact", "relp_model_fixed_cost_exact"):
        assert symbol in relp_amd.SYMBOLS and hasattr(relp_amd.lib(), symbol), symbol
    assert relp_amd.WitnessError is WitnessError and relp_amd.check_optimum is check_optimum
    assert relp_amd.check_infeasible is check_infeasible and relp_amd.check_unbounded is check_unbounded
    for owner, names in ((relp_amd.Solver, ["witness_exact"]), (relp_amd.Many, ["witness_exact", "solution_exact"]),
                         (relp_amd.Model, ["cost_exact", "right_hand_side_exact", "fixed_cost_exact"])):
        for attribute in names:
            assert callable(getattr(owner, attribute)), (owner, attribute)
