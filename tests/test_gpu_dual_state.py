"""The f64 state after dual pivots on the three pivot paths of the explicit carry (``-m gpu``, a real MI355X): m = 513, 1025 and 2049 --
one above 512, 1024 and 2048 rows -- put the parent and its child on the fused pivot with 2 rows per thread, the fused pivot with 4,
and the three-kernel pivot with touched-column tracking (asserted from ``kernel_path()`` before the device is touched).

Every case (``dual_lps.STATE_CASES``, ``mixed`` column lengths, small-integer data, ``polish_period=0``): the parent solved cold and
certified on the device, 24 cuts, ``begin_dual`` and ``iterate_dual(16)``, which must make at least 8 pivots.  Then the state is checked
against the exact data of its basis on the host, independently of every kernel (tests/residual_checks.py, where the bounds are derived
from the project's tolerances for an un-polished state): every entry of ``B Binv - I`` from every row of the device's inverse,
``B x_B - b`` and the objective, every relative cost against ``c_j - y a_j`` with ``y`` formed on the host from those rows, and three
BTRANs with an entry in every row; and every non-basic relative cost is >= -1e-9 (dual feasibility is kept).  Then ``solve_dual`` on a
fresh handle: certified, with the exact objective of the cold certified solve.  One decimal case (every matrix value divided by 10:
the Harris rule runs) at m = 513: ``solve_dual`` certified, the same exact objective; no pivot-for-pivot claim.

The residual form stands where ``state_checks.assert_state`` against ``SparseBasisState`` of ``solver.basis()`` was asked for: about
0.7 m structural columns are basic at the optimum of these LPs (343 of 513 rows), and the exact inverse of that block in Python
integers takes 33 s at m = 513 and grows with its cube -- minutes at 1025, hours at 2049.  That comparison runs at m = 64 and 65
(tests/test_gpu_dual.py); tests/test_dual_host.py shows that the residual checks refuse an entry that is off by 1e-6.

Largest figure per part, measured on an MI355X (inverse: max |B Binv - I|; vertex: max |B x_B - b|; objective: relative; costs: over
1 + |d_j|; btran: over max(1, largest entry)), one line per case:

  integer m =  513: 16 dual pivots of 16, inverse 2.1e-13  vertex 5.8e-13  objective 1.3e-16  costs 6.1e-13  btran 2.6e-15; solve_dual 1097 dual + 0 primal pivots, cold 1310; 0.5 s (0.4 s to the end of the state check)
  integer m = 1025: 16 dual pivots of 16, inverse 3.9e-14  vertex 1.1e-12  objective 0.0e+00  costs 4.0e-13  btran 2.1e-15; solve_dual 1491 dual + 0 primal pivots, cold 3363; 1.0 s (0.8 s to the end of the state check)
  integer m = 2049: 16 dual pivots of 16, inverse 4.7e-13  vertex 1.1e-11  objective 0.0e+00  costs 2.9e-12  btran 2.1e-15; solve_dual 11064 dual + 0 primal pivots, cold 9328; 3.9 s (2.5 s to the end of the state check)
  decimal m =  513: solve_dual 146 dual + 0 primal pivots, cold 1382; 0.3 s

(The small-integer family stalls under the exact-minimum ratio rule with largest-infeasibility pricing -- more dual pivots at m = 2049
than a cold solve makes; DESIGN.md section 10 has the measurements.  The decimal case runs the Harris rule.)
"""
import time

import numpy as np
import pytest

import relp_amd
import dual_lps
import sparse_lps
from dual_lps import cold_objective, solved_parent
from residual_checks import assert_residuals

pytestmark = pytest.mark.gpu
OPTIONS = dict(polish_period=0, certify=0)


def expected_plan(m):
    if m <= 2048:
        return dict(fused=True, fused_rows=2 if m <= 1024 else 4, track_touched=False)
    return dict(fused=False, track_touched=True, update_kernel="PREDICATED_SPLIT_GRID")


def child_of(m, decimal=False):
    seed, n_cuts = dual_lps.STATE_CASES[m]
    case = dual_lps.cut_case(m, dual_lps.MIXED, seed, n_cuts, decimal=decimal)
    plan = case.parent.kernel_path(**OPTIONS)
    assert plan["ratio_textbook"] == (not decimal)
    for field, value in expected_plan(m).items():
        assert plan[field] == value, (field, plan[field], value)
    child, basis, _ = case.child(*solved_parent(case))
    plan = child.kernel_path(**OPTIONS)
    assert child.dual_refusal(**OPTIONS) == "" and plan["ratio_textbook"] == (not decimal)
    for field, value in expected_plan(m).items():  # the cuts do not take the child across the edge its parent sits above
        assert plan[field] == value, (field, plan[field], value)
    return child, basis


def btrans(m):
    """Three vectors with a small non-zero integer in every row (tests/test_gpu_sparse_state.py)."""
    i = np.arange(m)
    rows = i.astype(np.int32)
    return [(rows, (1.0 + i % 7)), (rows, -(1.0 + i % 5)), (rows, (1.0 + (3 * i) % 9) * np.where(i % 2, -1.0, 1.0))]


@pytest.mark.parametrize("m", sorted(dual_lps.STATE_CASES))
def test_state_after_dual_pivots_and_the_certified_optimum(m):
    started = time.perf_counter()
    child, basis = child_of(m)
    solver = relp_amd.Solver(**OPTIONS).load_model(child)
    try:
        solver.begin_dual(basis)
        done, reason = solver.iterate_dual(16)
        assert done >= 8 and (reason == relp_amd.STOP_BUDGET) == (done == 16), (done, reason)
        phase, q, p, leaving = solver.last_pivot()
        assert phase == 3 and solver.basis()[p] == q - solver.n_art
        entered = sum(1 for before, after in zip(basis, solver.basis()) if before != after)
        assert entered >= 8  # (rows of the basis the walk has changed)
        report = {}
        assert_residuals(solver, sparse_lps.Provider(child), btrans(solver.m), report=report)
        is_basic = np.zeros(solver.n, dtype=bool)
        is_basic[solver.basis() + solver.n_art] = True
        costs = solver.relative_costs()
        assert costs[~is_basic].min() >= -1e-9, ("dual feasibility", float(costs[~is_basic].min()))
    finally:
        solver.close()
    checked = time.perf_counter() - started
    solver = relp_amd.Solver(polish_period=0, certify=1).load_model(child)
    try:
        result = solver.solve_dual(basis)
        assert result.kind == relp_amd.FINITE_OPTIMUM and result.certified == 1
        warm, pivots, clean_up = solver.objective_exact(), solver.dual_pivots(), result.pivots_phase_two
    finally:
        solver.close()
    cold, cold_result = cold_objective(child)
    assert warm == cold
    print("integer m = %4d: %2d dual pivots of 16, %s; solve_dual %d dual + %d primal pivots, cold %d; %.1f s (%.1f s to the end of the state check)" % (
        m, done, "  ".join("%s %.1e" % (part, report[part]) for part in ("inverse", "vertex", "objective", "costs", "btran")), pivots, clean_up,
        cold_result.pivots_phase_one + cold_result.pivots_phase_two, time.perf_counter() - started, checked))


def test_decimal_data_under_the_harris_rule():
    started = time.perf_counter()
    child, basis = child_of(513, decimal=True)
    solver = relp_amd.Solver(polish_period=0, certify=1).load_model(child)
    try:
        result = solver.solve_dual(basis)
        assert result.kind == relp_amd.FINITE_OPTIMUM and result.certified == 1
        warm, pivots, clean_up = solver.objective_exact(), solver.dual_pivots(), result.pivots_phase_two
        assert pivots >= 8
    finally:
        solver.close()
    cold, cold_result = cold_objective(child)
    assert warm == cold
    print("decimal m =  513: solve_dual %d dual + %d primal pivots, cold %d; %.1f s" % (
        pivots, clean_up, cold_result.pivots_phase_one + cold_result.pivots_phase_two, time.perf_counter() - started))
