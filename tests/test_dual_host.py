"""The host side of the dual simplex (no GPU): the C ABI's new symbols, ``Model.dual_refusal`` over the plans the dual kernels do not
take, and the inputs of the pivot-for-pivot GPU cases -- ``dual_lps.WALK_CASES`` -- checked with the exact reference alone.

The parent's optimal basis and vertex come from the oracle's cold solve here (the GPU tests take them from the certified device solve);
the child's exact optimum is the oracle's cold solve of the child.
"""
import ctypes as C

import numpy as np
import pytest

import relp_amd
from relp_amd.api import CARRY_LU, CARRY_LU_INVERSE, CARRY_NETWORK, ERR_ARGUMENT, RelpError, Result
from relp_oracle.solve import FiniteOptimum, solve_relaxation_full_basis
import dual_lps
import sparse_lps

NEW_SYMBOLS = ("relp_solve_dual", "relp_begin_dual", "relp_iterate_dual", "relp_get_dual_pivots", "relp_debug_dual_refusal")


def test_the_symbols_exist():
    lib = relp_amd.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in relp_amd.SYMBOLS
    for name in ("solve_dual", "begin_dual", "iterate_dual", "dual_pivots"):
        assert callable(getattr(relp_amd.Solver, name))
    assert callable(relp_amd.Model.dual_refusal)


def test_calls_without_a_handle_answer_as_set_basis_does():
    lib = relp_amd.lib()
    basis = np.zeros(4, dtype=np.int32)
    pointer = basis.ctypes.data_as(C.POINTER(C.c_int32))
    result, done, reason, pivots = Result(), C.c_int64(), C.c_int32(), C.c_int64()
    expected = lib.relp_set_basis(None, pointer)
    assert expected == ERR_ARGUMENT
    assert lib.relp_solve_dual(None, pointer, C.byref(result)) == expected
    assert lib.relp_begin_dual(None, pointer) == expected
    assert lib.relp_iterate_dual(None, C.c_int64(1), C.byref(done), C.byref(reason)) == expected
    assert lib.relp_get_dual_pivots(None, C.byref(pivots)) == expected
    assert lib.relp_debug_dual_refusal(None, None, None, 0, None) == ERR_ARGUMENT


@pytest.fixture(scope="module")
def less_model():
    return sparse_lps.less_lp(64, 128, dual_lps.MIXED, 2064)


def test_a_less_lp_is_taken_with_the_default_options(less_model):
    assert less_model.dual_refusal() == ""
    assert less_model.dual_refusal(pivot_kernels=1) == ""


@pytest.mark.parametrize("carry", [CARRY_LU, CARRY_LU_INVERSE])
def test_the_lu_carries_are_refused(less_model, carry):
    assert "LU" in less_model.dual_refusal(carry=carry)


def test_the_forest_carry_is_refused(less_model):
    graph = relp_amd.Model.max_flow(6, [(0, 1, 3), (0, 2, 2), (1, 3, 2), (2, 3, 3), (1, 2, 1), (3, 5, 4), (2, 4, 1), (4, 5, 2)], 0, 5)
    options = dict(carry=CARRY_NETWORK, implicit_bounds=1)  # (the capacities as bounds, not rows: the columns are network columns then)
    assert graph.kernel_path(**options)["network"]
    assert "forest" in graph.dual_refusal(**options)
    with pytest.raises(RelpError, match="not a network column"):  # (the load of a general LP under that carry is refused itself)
        less_model.dual_refusal(carry=CARRY_NETWORK)


def test_implicit_bounds_are_refused():
    columns = [[(0, 1), (1, 2)], [(0, 3), (1, 1)]]
    bounded = relp_amd.Model.from_general_form(columns, ["Less", "Less"], [4, 5], [(-1, 0, 3), (-2, 0, None)])
    assert bounded.kernel_path(implicit_bounds=1)["bounded"]
    assert "implicit upper bounds" in bounded.dual_refusal(implicit_bounds=1)
    assert bounded.dual_refusal() == ""  # (the bound as a row of the LP: nothing the dual loop does not know)
    unbounded = relp_amd.Model.from_general_form(columns, ["Less", "Less"], [4, 5], [(-1, 0, None), (-2, 0, None)])
    assert unbounded.dual_refusal(implicit_bounds=1) == ""  # (no bound: the option does not apply)


def test_a_dense_block_is_refused():
    """The plan of ``relp_load_dense_le``: at least 64 columns with more than m / 2 entries in front."""
    m = 64
    rng = np.random.RandomState(7)
    columns = [[(i, int(v)) for i, v in enumerate(rng.randint(1, 4, size=m))] for _ in range(64)]
    dense = relp_amd.Model.from_general_form(columns, ["Less"] * m, [100] * m, [(-1, 0, None)] * 64)
    assert dense.kernel_path()["n_dense"] == 64
    assert dense.dual_refusal() != ""


def test_a_graph_model_in_the_two_entry_layout_is_refused():
    vertices = 7002  # (beyond the row count at which the pricing vectors leave LDS: the plan takes the width-2 layout)
    arcs = [(i, i + 1, 2 + i % 3) for i in range(vertices - 1)] + [(i, i + 2, 1) for i in range(0, vertices - 2, 2)]
    graph = relp_amd.Model.shortest_path(vertices, arcs, 0, vertices - 1)
    plan = graph.kernel_path()
    assert plan["ell_w"] == 2 and plan["generated_columns"]
    assert "generated" in graph.dual_refusal()
    from relp_amd.api import SW_NO_GENERATED_COLUMNS
    assert "two-entry" in graph.dual_refusal(switches=SW_NO_GENERATED_COLUMNS)


def test_more_than_8192_rows_are_refused():
    m = 8193
    columns = [[(i, 1)] if i + 2 >= m else [(i, 1), (i + 1, 2), (i + 2, 1)] for i in range(m)]  # (three entries: no graph layout)
    wide = relp_amd.Model.from_general_form(columns, ["Less"] * m, [1] * m, [(-1, 0, None)] * m)
    assert "8192" in wide.dual_refusal()


@pytest.mark.parametrize("m", sorted(dual_lps.WALK_CASES))
def test_the_walk_cases_meet_their_conditions(m):
    seed, n_cuts = dual_lps.WALK_CASES[m]
    case = dual_lps.cut_case(m, dual_lps.MIXED, seed, n_cuts)
    parent = solve_relaxation_full_basis(sparse_lps.Provider(case.parent))
    assert isinstance(parent, FiniteOptimum)
    vertex = {j: v for j, v in parent.solution if j < case.n_structural}
    child, basis, cuts = case.child(parent.basis, vertex)
    assert len(cuts) == n_cuts and child.nr_rows == m + n_cuts
    for variables, coefficients, rhs in cuts:  # every cut bites, and none was flipped
        assert 1 <= len(variables) <= 3 and rhs >= 0 and set(np.abs(coefficients)) <= {1, 2, 3}
        assert sum(a * vertex[j] for j, a in zip(variables, coefficients)) > rhs
    reference = dual_lps.DualReference(child, basis)
    assert min(reference.reduced_costs()) >= 0  # the parent's basis is dual feasible in the child
    assert min(reference.x) < 0                 # ... and primal infeasible
    reason = reference.run()
    dual_lps.assert_walk_conditions(reference, m, reason)
    cold = solve_relaxation_full_basis(sparse_lps.Provider(child))
    assert isinstance(cold, FiniteOptimum)
    assert reference.objective() == cold.objective
    print("m = %d: %d dual pivots, smallest margin %.3g, smallest infeasibility %.3g" % (
        m, len(reference.pivots), reference.smallest_margin(), float(reference.smallest_infeasibility)))


def test_the_reference_reports_an_infeasible_child():
    seed, _ = dual_lps.WALK_CASES[5]
    case = dual_lps.cut_case(5, dual_lps.MIXED, seed, 0)
    parent = solve_relaxation_full_basis(sparse_lps.Provider(case.parent))
    vertex = {j: v for j, v in parent.solution if j < case.n_structural}
    child, basis = dual_lps.infeasible_child(case, parent.basis, vertex)
    assert child.nr_rows == 7 and child.right_hand_side_exact() == list(case.b) + [0, 1]  # the rows kept their order and signs
    assert len(child.pivot_element_indices()) == 6 and len(set(basis)) == 7              # (the "Greater" row starts from an artificial)
    assert dual_lps.DualReference(child, basis).run() == relp_amd.STOP_UNBOUNDED


class StateOnTheHost:
    """What ``residual_checks.assert_residuals`` reads from a handle, served from an exact ``DualReference`` rounded to f64."""

    def __init__(self, reference):
        self.m, self.n, self.n_art = reference.m, reference.n, 0
        self.reference = reference
        self.inverse = np.array([[float(v) for v in row] for row in reference.inverse])
        self.x = np.array([float(v) for v in reference.x])
        self.costs = np.array([float(v) for v in reference.reduced_costs()])

    def basis(self):
        return np.array(self.reference.basis, dtype=np.int32)

    def basis_inverse_row(self, k):
        return self.inverse[k].copy()

    def b(self):
        return self.x.copy()

    def objective_function_value(self):
        return float(self.reference.objective())

    def relative_costs(self):
        return self.costs.copy()

    def right_multiply_by_basis_inverse(self, rows, values):
        return np.asarray(values, dtype=np.float64) @ self.inverse[np.asarray(rows)]


def test_the_residual_checks_pass_an_exact_state_and_refuse_a_wrong_one():
    """The host-side check of tests/test_gpu_dual_state.py on a state that is right by construction, and with one entry of each part off
    by 1e-6 -- a thousand times the tolerance of an un-polished state."""
    from residual_checks import assert_residuals
    seed, n_cuts = dual_lps.WALK_CASES[5]
    case = dual_lps.cut_case(5, dual_lps.MIXED, seed, n_cuts)
    parent = solve_relaxation_full_basis(sparse_lps.Provider(case.parent))
    child, basis, _ = case.child(parent.basis, {j: v for j, v in parent.solution if j < case.n_structural})
    reference = dual_lps.DualReference(child, basis)
    assert reference.step() is None and reference.step() is None  # two dual pivots in: a basis with structural columns, x_B not yet feasible
    provider = sparse_lps.Provider(child)
    m = reference.m
    btrans = [(np.arange(m, dtype=np.int32), 1.0 + np.arange(m) % 3)]
    state, report = StateOnTheHost(reference), {}
    assert_residuals(state, provider, btrans, report=report)
    assert set(report) == {"inverse", "vertex", "objective", "costs", "btran"} and max(report.values()) < 1e-12
    structural = next(k for k, j in enumerate(reference.basis) if len(provider.columns[j]) > 1)
    wrong = StateOnTheHost(reference)
    wrong.inverse[structural, 0] += 1e-6
    with pytest.raises(AssertionError, match="B Binv - I"):
        assert_residuals(wrong, provider, btrans, parts=("inverse",))
    wrong = StateOnTheHost(reference)
    wrong.x[structural] += 1e-6
    with pytest.raises(AssertionError, match="B x_B - b"):
        assert_residuals(wrong, provider, btrans, parts=("vertex",))
    wrong = StateOnTheHost(reference)
    wrong.costs[int(np.argmax(np.abs(wrong.costs)))] += 1e-6
    with pytest.raises(AssertionError, match="relative cost"):
        assert_residuals(wrong, provider, btrans, parts=("costs",))
    wrong = StateOnTheHost(reference)
    product = wrong.right_multiply_by_basis_inverse
    wrong.right_multiply_by_basis_inverse = lambda rows, values: product(rows, values) + 1e-6
    with pytest.raises(AssertionError, match="btran"):
        assert_residuals(wrong, provider, btrans, parts=("btran",))
