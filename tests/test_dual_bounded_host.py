"""The host side of the dual simplex on implicit upper bounds (no GPU): the C ABI's new symbols, ``Model.dual_bounded_refusal``, and the
inputs of the pivot-for-pivot GPU cases -- ``dual_bounded_lps.WALK_CASES`` -- checked with the exact reference alone.

The parent's optimal basis and vertex are the oracle's cold solve; the child's exact optimum is the oracle's cold solve of the child
with its bounds as ``Variable(upper_bound=...)``.
"""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import relp_amd
from relp_amd.api import CARRY_LU, CARRY_LU_INVERSE, CARRY_NETWORK, ERR_ARGUMENT, Result
from relp_oracle.solve import FiniteOptimum
import dual_bounded_lps as lps

NEW_SYMBOLS = ("relp_begin_dual_bounded", "relp_solve_dual_bounded", "relp_debug_dual_bounded_refusal")


def test_the_symbols_exist():
    lib = relp_amd.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in relp_amd.SYMBOLS
    for name in ("begin_dual_bounded", "solve_dual_bounded"):
        assert callable(getattr(relp_amd.Solver, name))
    assert callable(relp_amd.Model.dual_bounded_refusal)


def test_calls_without_a_handle_answer_as_set_basis_does():
    lib = relp_amd.lib()
    basis = np.zeros(4, dtype=np.int32)
    pointer = basis.ctypes.data_as(C.POINTER(C.c_int32))
    expected = lib.relp_set_basis(None, pointer)
    assert expected == ERR_ARGUMENT
    assert lib.relp_solve_dual_bounded(None, pointer, C.byref(Result())) == expected
    assert lib.relp_begin_dual_bounded(None, pointer) == expected
    assert lib.relp_debug_dual_bounded_refusal(None, None, None, 0, None) == ERR_ARGUMENT


@pytest.fixture(scope="module")
def parent():
    return lps.BoundedCase(64, lps.WALK_CASES[64][0], 0, 0).parent


def test_a_bounded_and_an_unbounded_plan_are_taken(parent):
    assert parent.model.kernel_path(implicit_bounds=1)["bounded"] and parent.model.kernel_path(implicit_bounds=1)["m"] == 64
    assert "implicit upper bounds" in parent.model.dual_refusal(implicit_bounds=1)  # (the plain loop still refuses the plan)
    assert parent.model.dual_bounded_refusal(implicit_bounds=1) == ""
    assert parent.model.dual_bounded_refusal() == ""  # the bounds as rows: the plan the plain loop takes
    assert not parent.model.kernel_path()["bounded"]
    without = lps.Formulation(parent.columns, parent.b, parent.cost, [None] * parent.ns)
    assert without.model.dual_bounded_refusal(implicit_bounds=1) == "" and without.model.dual_bounded_refusal() == ""


@pytest.mark.parametrize("carry", [CARRY_LU, CARRY_LU_INVERSE])
def test_the_lu_carries_are_refused(parent, carry):
    assert "LU" in parent.model.dual_bounded_refusal(carry=carry, implicit_bounds=1)
    assert parent.model.dual_bounded_refusal(carry=carry, implicit_bounds=1) == parent.model.dual_refusal(carry=carry)


def test_the_forest_carry_is_refused():
    graph = relp_amd.Model.max_flow(6, [(0, 1, 3), (0, 2, 2), (1, 3, 2), (2, 3, 3), (1, 2, 1), (3, 5, 4), (2, 4, 1), (4, 5, 2)], 0, 5)
    options = dict(carry=CARRY_NETWORK, implicit_bounds=1)
    assert graph.kernel_path(**options)["network"] and graph.kernel_path(**options)["bounded"]
    assert "forest" in graph.dual_bounded_refusal(**options)


def test_the_row_limit_counts_constraint_rows():
    """8192 constraint rows and a bound on every variable: 16 384 rows of the formulation."""
    def model(m):
        columns = [[(i, 1)] if i + 2 >= m else [(i, 1), (i + 1, 2), (i + 2, 1)] for i in range(m)]  # (three entries: no graph layout)
        return relp_amd.Model.from_general_form(columns, ["Less"] * m, [1] * m, [(-1, 0, 2)] * m)
    at_the_limit = model(8192)
    assert at_the_limit.nr_rows == 2 * 8192 and at_the_limit.kernel_path(implicit_bounds=1)["m"] == 8192
    assert at_the_limit.dual_bounded_refusal(implicit_bounds=1) == ""
    assert "8192" in at_the_limit.dual_bounded_refusal()  # the bounds as rows: 16 384 of them
    assert "8192" in at_the_limit.dual_refusal()
    beyond = model(8193)
    assert "8192" in beyond.dual_bounded_refusal(implicit_bounds=1) and "8193" in beyond.dual_bounded_refusal(implicit_bounds=1)


def test_the_three_forms_of_a_formulation_agree(parent):
    model, oracle = parent.model, parent.oracle
    assert (model.nr_rows, model.nr_columns) == (parent.rows, parent.rows + parent.ns) == (oracle.nr_rows(), oracle.nr_columns())
    for j in range(model.nr_columns):
        assert [(i, Fraction(a, b)) for i, a, b in model.column_exact(j)] == oracle.column(j), j
        assert model.cost_exact(j) == oracle.cost_value(j)
    assert model.right_hand_side_exact() == oracle.right_hand_side()
    assert sorted(model.pivot_element_indices()) == sorted(oracle.pivot_element_indices())
    assert sum(1 for u in parent.upper if u is not None) == parent.ns // 2 and 0 in parent.upper


def checked_walk(m, reference_class):
    case, optimum, child, basis, cuts, branches = lps.walk_case(m)
    seed, n_cuts, n_tight = lps.WALK_CASES[m]
    vertex = dict(optimum.solution)
    assert len(cuts) == n_cuts and len(branches) == n_tight + 1 and child.m == m + n_cuts
    gained = [j for j in branches if case.parent.upper[j] is None]
    assert len(gained) == 1 and child.rows == case.parent.rows + n_cuts + 1  # one bound row more than the parent's, beside the cuts
    for variables, coefficients, rhs in cuts:
        assert sum(a * vertex[j] for j, a in zip(variables, coefficients)) > rhs >= 0
    for j, u in branches.items():
        assert vertex[j] > u >= 0 and u == -(-vertex[j].numerator // vertex[j].denominator) - 1
    reference = reference_class(child, basis)
    assert min(d for d in reference.signed_costs() if d is not None) >= 0  # the parent's basis is dual feasible in the child
    assert not reference.feasible()                                         # ... and primal infeasible
    reason, facts, bases = lps.walk(reference)
    return reference, reason, facts, bases, child


@pytest.mark.parametrize("m", sorted(lps.WALK_CASES))
def test_the_walk_cases_meet_their_conditions(m):
    reference, reason, facts, bases, child = checked_walk(m, lps.BoundedDualReference)
    lps.assert_walk_conditions(reference, m, reason, facts)
    cold = child.solve()
    assert isinstance(cold, FiniteOptimum)
    assert reference.objective() == cold.objective
    assert all(len(set(basis)) == child.rows for basis in bases)
    solution = reference.solution()
    assert all(0 <= v and (child.upper[j] is None or v <= child.upper[j]) for j, v in solution.items())
    print("m = %d: %s" % (m, ", ".join("%s %.3g" % (key, float(value)) for key, value in facts.items())))


def test_a_column_of_width_zero_leaves_in_some_case():
    total = 0
    for m in sorted(lps.WALK_CASES):
        _, _, child, basis, _, _ = lps.walk_case(m)
        total += lps.walk(lps.BoundedDualReference(child, basis))[1]["width_zero_leaving"]
    assert total >= 1


@pytest.mark.parametrize("m", sorted(lps.WALK_CASES))
def test_the_steepest_edge_walk_ends_at_the_same_optimum(m):
    reference, reason, facts, _, child = checked_walk(m, lps.SteepestBoundedDualReference)
    lps.assert_walk_conditions(reference, m, reason, facts)
    assert reference.objective() == child.solve().objective
    print("m = %d, steepest edge: %s" % (m, ", ".join("%s %.3g" % (key, float(value)) for key, value in facts.items())))


def test_the_reference_reports_an_infeasible_child():
    from relp_oracle import Infeasible, solve_relaxation
    case, optimum, child, basis = lps.infeasible_child()
    assert child.model.right_hand_side_exact()[:child.m] == list(case.parent.b) + [1]  # the rows kept their order and signs
    reference = lps.BoundedDualReference(child, basis)
    assert reference.run() == relp_amd.STOP_UNBOUNDED and len(reference.pivots) >= 1
    assert solve_relaxation(child.oracle) == Infeasible()


class StateOnTheHost:
    """What ``dual_bounded_lps.HeldState`` reads from a handle, served from an exact ``BoundedDualReference`` rounded to f64."""

    def __init__(self, reference):
        self.reference, self.n_art = reference, 0
        self.inverse = np.array([[float(v) for v in row] for row in reference.inverse])
        self.x = np.array([float(v) for v in reference.x])
        self.costs = np.array([float(v) for v in reference.relative_costs()])
        self.objective = float(reference.objective())

    def basis(self):
        return np.array(self.reference.formulation_basis(), dtype=np.int32)

    def basis_inverse_row(self, k):
        return self.inverse[k].copy()

    def b(self):
        return self.x.copy()

    def objective_function_value(self):
        return self.objective

    def relative_costs(self):
        return self.costs.copy()

    def right_multiply_by_basis_inverse(self, rows, values):
        return np.asarray(values, dtype=np.float64) @ self.inverse[np.asarray(rows)]


def test_the_held_residual_checks_pass_an_exact_state_and_refuse_a_wrong_one():
    """The check of the 513-row GPU case on a state that is right by construction -- in the middle of the walk at m = 64, after a
    column has left at its upper side and a complemented one has entered -- and with one entry of the inverse, of x_B and the objective
    off by 1e-6 and one relative cost off by more than 1."""
    from residual_checks import assert_residuals
    from sparse_lps import btrans
    _, _, child, basis, _, _ = lps.walk_case(64)
    reference = lps.BoundedDualReference(child, basis)
    entered_complemented = False
    while not (entered_complemented and -1 in [side for _, _, _, side in reference.pivots]):
        flipped = list(reference.flipped)
        assert reference.step() is None
        entered_complemented |= bool(flipped[reference.pivots[-1][0]])
    exact = StateOnTheHost(reference)
    handle, provider, state = lps.held_pair(exact, child)
    assert state.sgn == [reference.sgn(j) if reference.pos[j] != -3 else state.sgn[j] for j in range(reference.n)]
    assert state.complemented_basic >= 1 and list(handle.basis()) == reference.basis and provider.b == reference.rhs
    report = {}
    assert_residuals(handle, provider, btrans(child.m), report=report)
    assert set(report) == {"inverse", "vertex", "objective", "costs", "btran"} and max(report.values()) < 1e-12
    k = next(k for k, j in enumerate(reference.basis) if reference.flipped[j])  # a basic column held complemented
    for part, spoil, message in (("inverse", lambda w: w.inverse.__setitem__((k, 0), w.inverse[k, 0] + 1e-6), "B Binv - I"),
                                 ("vertex", lambda w: w.x.__setitem__(k, w.x[k] + 1e-6), "B x_B - b"),
                                 ("vertex", lambda w: setattr(w, "objective", w.objective + 1e-6 * max(1.0, abs(w.objective))), "objective"),
                                 ("costs", lambda w: w.costs.__setitem__(int(np.argmax(np.abs(w.costs))), w.costs.max() + 1), "relative cost")):
        wrong = StateOnTheHost(reference)
        spoil(wrong)
        with pytest.raises(AssertionError, match=message):
            assert_residuals(*lps.held_pair(wrong, child)[:2], btrans(child.m), parts=(part,))
