"""The f64 state of a handle against the exact state of its basis, on the dense pipeline (BASELINE config 3) of a real MI355X (``-m gpu``).

Everything a handle holds is a function of its current basis (oracle/basis_state.py), so the state is checked after ANY number of pivots
made by ANY launch shape -- batches, captured graphs, the deferred product form at and around its cap of 32 etas, a polish inside the loop
-- without an oracle that walks the same path.  ``assert_state`` compares every row of the resident inverse, b, the objective, every
relative cost, every steepest-edge weight, four FTRANs through the multi-block pipeline, one BTRAN and the entering-column choice.

Tolerance before a polish: ``close()`` of tests/test_gpu_parity.py (rtol 1e-8, atol 1e-9 x the vector's largest entry; 1e-8 relative for
gamma, 1e-9 for the relative costs).  After a polish: 16 x the error of the numpy f64 restatement of the same Newton-Schulz steps at the
same basis, floor 8 ulps of the largest entry (``basis_state.polished_tolerance``).

The reference can be wrong on purpose: three tests feed the checks a perturbed exact state (or the state before a polish) and expect
them to object.
"""
import numpy as np
import pytest

import relp_amd
from relp_amd.api import SW_NO_DENSE_LANE
from relp_amd.workloads import dense_lp
import state_checks
from basis_state import BasisState, DenseLE
from state_checks import EVERYTHING, assert_state, close, device_inverse

pytestmark = pytest.mark.gpu


def exact_state(solver, lp):
    a, b, c = lp
    return BasisState(DenseLE(a), b, c, solver.basis())


def assert_polished(solver, lp, inverse_before, parts=EVERYTHING):
    """After ``refactor()``: the resident inverse and b within the post-polish tolerance (module docstring) of the exact state."""
    state_checks.assert_polished(solver, exact_state(solver, lp), inverse_before, np.asarray(lp[1], dtype=np.float64), parts=parts)


def pipeline_solver(lp, **options):
    """A handle on the dense pipeline (multi-block FTRAN; deferred product form where m is even), un-polished unless asked."""
    options.setdefault("polish_period", 0)
    solver = relp_amd.Solver(ftran_min_nnz=16, **options).load_dense_le(*lp)
    assert solver.n_art == 0
    solver.begin_phase_one()
    return solver


def pipeline_launches(batches):
    """Launches ``stats()`` counts for un-graphed batches of the pipeline: budget + (price, dense price, partial FTRAN, reduce, ratio, update) per pivot."""
    return sum(1 + 6 * batch for batch in batches)


LP_130 = dense_lp(130, 2000, seed=0x5EED0100 + 130)  # 105 pivots in the numpy restatement; 130 rows are ragged against 64, 16 and 4


# ---- the deferred product form at, below and above its cap of 32 etas ------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [1, 0], ids=["graph", "plain launches"])
def test_state_at_eta_depths_31_32_33(use_graph):
    solver = pipeline_solver(LP_130, use_graph=use_graph)
    for count in (31, 32, 33):  # consolidation at the end of a batch below the cap, at the cap, at the cap and one eta later
        done, reason = solver.iterate(count)
        assert (done, reason) == (count, relp_amd.STOP_BUDGET)
        if count == 31:
            assert solver.stats().launches == pipeline_launches([31])  # (batches shorter than a full one are never replayed from a graph)
        assert_state(solver, exact_state(solver, LP_130))
    done, reason = solver.iterate(10 ** 6)
    assert reason == relp_amd.STOP_NO_ENTERING
    assert_state(solver, exact_state(solver, LP_130))
    solver.close()


@pytest.mark.parametrize("use_graph", [1, 0], ids=["graph", "plain launches"])
def test_state_after_two_consolidations_at_the_cap_and_a_ragged_six(use_graph):
    solver = pipeline_solver(LP_130, use_graph=use_graph)
    before = solver.stats().launches
    assert solver.iterate(70) == (70, relp_amd.STOP_BUDGET)  # one full batch of 64 (etas 32 + 32), then 6
    full_batch = 1 + 3 * 64 if use_graph else pipeline_launches([64])  # (a replayed graph is counted as three launches per pivot)
    assert solver.stats().launches - before == full_batch + pipeline_launches([6])
    assert_state(solver, exact_state(solver, LP_130))
    solver.close()


def test_state_with_a_polish_inside_the_loop():
    solver = pipeline_solver(LP_130, polish_period=16)
    assert solver.iterate(40) == (40, relp_amd.STOP_BUDGET)
    assert_state(solver, exact_state(solver, LP_130))
    _, reason = solver.iterate(10 ** 6)
    assert reason == relp_amd.STOP_NO_ENTERING
    before = device_inverse(solver)
    assert_state(solver, exact_state(solver, LP_130), inverse=before)
    print("residual found by the final polish: %.3e" % solver.refactor())  # the final polish of a solve
    assert_polished(solver, LP_130, before)
    solver.close()
    # the handle above cannot say how often it polished; a whole solve can: with period 16 and the back-off of the period (x2 while the
    # drift stays below 1e-8) the loop polishes after 16 and 48 of its ~100 pivots, and once more at the optimum
    whole = relp_amd.Solver(ftran_min_nnz=16, polish_period=16).load_dense_le(*LP_130)
    result = whole.solve_relaxation()
    print("polishes %d, largest residual found %.3e" % (result.polishes, result.max_residual))
    assert result.kind == relp_amd.FINITE_OPTIMUM and result.polishes >= 3 and result.max_residual > 0.0
    assert_state(whole, exact_state(whole, LP_130))
    whole.close()


# ---- rank-one updates (no deferred product form) ---------------------------------------------------------------------------------
@pytest.mark.parametrize("m, n, options", [(255, 512, {}), (130, 2000, {"product_form": 1})], ids=["odd m", "even m, product_form=1"])
def test_state_without_the_deferred_product_form(m, n, options):
    lp = LP_130 if m == 130 else dense_lp(m, n, seed=0x5EED0100 + m)
    solver = pipeline_solver(lp, **options)
    assert solver.iterate(33) == (33, relp_amd.STOP_BUDGET)
    assert solver.stats().launches == pipeline_launches([33])
    assert_state(solver, exact_state(solver, lp))
    _, reason = solver.iterate(10 ** 6)
    assert reason == relp_amd.STOP_NO_ENTERING
    assert_state(solver, exact_state(solver, lp))
    solver.close()


# ---- the six forms the dense block is priced from --------------------------------------------------------------------------------
STORAGE = {"bytes, column per lane": (0, 0), "bytes, vectors in LDS": (0, SW_NO_DENSE_LANE), "f32, column per lane": (1, 0),
           "f32, vectors in LDS": (1, SW_NO_DENSE_LANE), "f64, column per lane": (2, 0), "f64, vectors in LDS": (2, SW_NO_DENSE_LANE)}


@pytest.mark.parametrize("storage", sorted(STORAGE))
@pytest.mark.parametrize("m, n", [(66, 130), (130, 200)])
def test_costs_weights_and_columns_of_the_storage_forms(m, n, storage):
    lp = dense_lp(m, n, seed=0x5EED0100 + m)
    dense_storage, switches = STORAGE[storage]
    solver = relp_amd.Solver(dense_storage=dense_storage, switches=switches, polish_period=0).load_dense_le(*lp)
    solver.begin_phase_one()
    assert solver.iterate(20) == (20, relp_amd.STOP_BUDGET)
    assert_state(solver, exact_state(solver, lp), parts=("costs", "weights", "alpha", "selection"))
    solver.close()


# ---- the by-rows polish over more than one 64-row tile of touched rows -----------------------------------------------------------
def dominant_diagonal_lp():
    """130 x 200 from the same stream, entries 1 + (a - 1) % 9 and 100 at (j mod m, j): structural j can be brought into row j (the
    generator's own optimal bases hold at most 71 structural columns; cond of the bases on this walk stays below 4e4)."""
    a, b, c = dense_lp(130, 200, seed=0x5EED0100 + 130)
    a = 1 + (a - 1) % 9
    for j in range(a.shape[0]):
        a[j, j % a.shape[1]] = 100
    return a, b, c


@pytest.fixture(scope="module")
def walked():
    """96 forced pivots: structural j into row j.  Returns (handle, LP, whether every leaving variable was non-negative)."""
    lp = dominant_diagonal_lp()
    solver = pipeline_solver(lp)
    feasible = True
    # the exact tableau [A_0..95 | b] D, carried by fraction-free Gauss-Jordan steps on the pivots (j, j) in Python integers
    a, b, _ = lp
    tableau = np.concatenate([a[:96].T, b[:, None]], axis=1).astype(object)
    previous = 1
    for j in range(96):
        column = tableau[:, j].copy()
        assert 10 * abs(column[j]) > max(abs(v) for v in column), j  # |alpha_jj| > 0.1 max|alpha_j|
        feasible = feasible and tableau[j, 96] * previous >= 0
        solver.bring_into_basis(j, j)
        pivot, row = column[j], tableau[j, j:].copy()
        column[j] = 0
        tableau[:, j:] = (tableau[:, j:] * pivot - np.outer(column, row)) // previous
        tableau[j, j:] = row
        previous = pivot
    basis = list(range(96)) + list(range(296, 330))
    assert solver.basis().tolist() == basis
    yield solver, lp, feasible
    solver.close()


def parts_of_a_forced_walk(feasible):
    # A forced pivot on a row whose basic variable is negative moves it to max(x_p, 0) / alpha_pq (pivot_step.hpp: step_decision, as the
    # reference's zero-level pivots do), so past an infeasible vertex b and the objective are not functions of the basis until a
    # polish recomputes them from the inverse.
    return EVERYTHING if feasible else tuple(part for part in EVERYTHING if part != "vertex")


def test_residual_pass_by_rows_after_the_dominant_walk(walked):
    """96 touched rows: gather_basis_kernel and the residual GEMM (gemm_mfma_kernel<1>) over a row list of more than one 64-row tile.
    Measured on an MI355X: this walk leaves the inverse within 6.1e-17 of the exact one, a residual below the 1e-12 under which the
    polish takes no step -- the correction GEMM and copy_rows_kernel do NOT run here (they do in the drifted walk below)."""
    solver, lp, feasible = walked
    before = device_inverse(solver)
    assert_state(solver, exact_state(solver, lp), parts=parts_of_a_forced_walk(feasible), inverse=before)
    assert solver.refactor() < 1e-12
    # Below 1e-12 the restatement returns `before` unchanged, so the bound on the inverse is 16 x the device's own error before the polish:
    # for the inverse this call only says that the polish left it alone.  What it does check is b and the objective, which the polish
    # recomputes from the inverse, and the rest of assert_state.
    assert_polished(solver, lp, before)


def drifting_lp():
    """The same LP without the dominance: 9 at (j mod m, j) among entries 1..9.  The walk of structural j into row j then takes pivots down
    to 1e-4 of their column (numpy f64 restatement: residual 2.8e-10, cond of the last basis 1.5e5), so the polish has something to do."""
    a, b, c = dense_lp(130, 200, seed=0x5EED0100 + 130)
    a = 1 + (a - 1) % 9
    for j in range(a.shape[0]):
        a[j, j % a.shape[1]] = 9
    return a, b, c


# weights carried by the recurrences through pivots of relative size 1e-4 are not refreshed by a polish, and the entering choice reads them
DRIFTED_PARTS = ("inverse", "vertex", "costs", "alpha", "btran")


def drifted_walk():
    lp = drifting_lp()
    solver = pipeline_solver(lp)
    for j in range(96):
        solver.bring_into_basis(j, j)
    assert solver.basis().tolist() == list(range(96)) + list(range(296, 330))
    return solver, lp


def test_by_rows_polish_corrects_a_drifted_inverse_over_two_tiles_of_rows():
    """A Newton step over 96 listed rows: gemm_mfma_kernel<1> and <0> with the row list, copy_rows_kernel."""
    solver, lp = drifted_walk()
    before = device_inverse(solver)
    residual = solver.refactor()
    print("residual found by the polish: %.3e" % residual)
    assert 1e-12 <= residual < 0.5  # the polish took a step (it skips below 1e-12 and starts from scratch at 0.5)
    assert_polished(solver, lp, before, parts=DRIFTED_PARTS)
    solver.close()


# ---- the multi-block FTRAN of select_primal_pivot_row once a batch has used its budget -------------------------------------------
def test_ratio_after_a_spent_budget_computes_the_column_it_is_asked_for(after_31):
    """ftran_partial_kernel leaves at once when the budget of the last batch is used up; ``select_primal_pivot_row`` then returned the alpha
    of an earlier column.  Two different columns, two different alphas, both those of the exact state."""
    exact = exact_state(after_31, LP_130)
    free = np.flatnonzero(~exact.is_basic)
    first, second = int(free[1]), int(free[len(free) // 2])
    alpha_first = after_31.select_primal_pivot_row(first)[1]
    alpha_second = after_31.select_primal_pivot_row(second)[1]
    assert not np.allclose(alpha_first, alpha_second)
    assert close(alpha_first, exact.alpha(first)) and close(alpha_second, exact.alpha(second))


# ---- the checks object to a wrong reference --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def after_31():
    solver = pipeline_solver(LP_130)
    assert solver.iterate(31)[0] == 31
    yield solver
    solver.close()


def test_weights_formed_without_the_one_are_refused(after_31):
    exact = exact_state(after_31, LP_130)
    gammas = exact.gammas
    exact.gammas = lambda columns: gammas(columns) - 1
    with pytest.raises(AssertionError, match="gamma"):
        assert_state(after_31, exact)


def test_the_inverse_of_a_basis_with_two_columns_exchanged_is_refused(after_31):
    basis = after_31.basis()
    basis[[3, 4]] = basis[[4, 3]]
    a, b, c = LP_130
    with pytest.raises(AssertionError, match="row of the inverse"):
        assert_state(after_31, BasisState(DenseLE(a), b, c, basis))


def test_a_drifted_inverse_is_outside_the_tolerance_after_a_polish():
    solver, lp = drifted_walk()
    with pytest.raises(AssertionError, match="polished inverse"):
        assert_polished(solver, lp, device_inverse(solver), parts=DRIFTED_PARTS)  # no refactor() in between
    solver.close()
