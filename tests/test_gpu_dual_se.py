"""The dual simplex with steepest-edge pricing of the leaving row on the device (``dual_pricing=1``; ``-m gpu``, a real MI355X).

  pivot for pivot   ``dual_se_lps.SE_WALK_CASES`` (the children of ``dual_lps.WALK_CASES``: 8, 68 and 68 rows, one tile of rows and
                    two, one slice of columns) against ``DualSteepestReference``; all three walks leave the walk of largest
                    infeasibility at the first pivot.  After the walk the weights against the exact row norms of the reference's
                    inverse; then ``solve_dual`` on a fresh handle: certified, the cold solve's exact objective, the same pivots
  weights, inverse  ``dual_lps.STATE_CASES`` at m = 513 (fused pivot plan, 8 slices) and 2049 (three-kernel plan, 16 slices),
                    ``polish_period=0``: after 16 dual pivots the weights against the row norms of the device's own inverse, and the
                    residual checks of the state unchanged; ``solve_dual`` certified
  from the parent   ``solve_dual_from`` at m = 64
  rule 0            no weights, the record, and the launches of a batch as they were

Bounds.  The weights are recomputed from the inverse after every pivot, so they differ from the row norms of the device's inverse
only by the order of a sum of m non-negative terms: relative m 2^-52.  Against the exact inverse, an entry of the un-polished device
inverse may be off by ``state_checks``' ``eps = ABSOLUTE max(1, max |row|) + RELATIVE |entry|``, taken at the row's largest entry;
then ``|beta_dev - beta| <= 2 eps sum_j |Binv_ij| + m eps^2 + m 2^-52 beta``.

Measured on an MI355X:

  m =  5 + 3 cuts, 4 dual pivots (rule 0: 4):    worst weight error 2.6e-8 of its bound, 8.3e-16 relative
  m = 64 + 4 cuts, 13 dual pivots (rule 0: 16):  9.0e-8 of its bound, 4.6e-15 relative
  m = 65 + 3 cuts, 9 dual pivots (rule 0: 12):   2.4e-7 of its bound, 1.1e-14 relative
  m =  513 + 24 cuts, 16 pivots: weights against the device's row norms 3.7e-16 relative (bound 1.2e-13); solve_dual 155 dual pivots (rule 0: 1097)
  m = 2049 + 24 cuts, 16 pivots: 4.4e-16 relative (bound 4.6e-13); solve_dual 587 dual pivots (rule 0: 11 064)

The slowest case, m = 2049, takes 3.4 s.
"""
import functools

import numpy as np
import pytest

import relp_amd
from relp_amd.api import DUAL_PRICING_STEEPEST_EDGE, ERR_STATE, RelpError
import dual_lps
import dual_se_lps
import sparse_lps
from dual_lps import cold_objective, solved_parent
from residual_checks import assert_residuals
from state_checks import ABSOLUTE, RELATIVE
from test_gpu_dual_state import OPTIONS, btrans, expected_plan

pytestmark = pytest.mark.gpu
STEEPEST = dict(dual_pricing=DUAL_PRICING_STEEPEST_EDGE)


@functools.lru_cache(maxsize=None)
def walk_child(m):
    """``(case, child, basis)`` of a walk case, the parent solved once for the tests that share it."""
    seed, n_cuts = dual_se_lps.SE_WALK_CASES[m]
    case = dual_lps.cut_case(m, dual_lps.MIXED, seed, n_cuts)
    child, basis, _ = case.child(*solved_parent(case))
    return case, child, tuple(basis)


def weight_bounds(inverse):
    """Per row of an exact inverse (``Fraction``): ``(beta, bound)`` of the docstring, in ``longdouble``."""
    m = len(inverse)
    rows = np.array([[float(v) for v in row] for row in inverse], dtype=np.longdouble)
    beta = np.array([float(b) for b in dual_se_lps.row_norms(inverse)], dtype=np.longdouble)
    largest = np.abs(rows).max(axis=1)
    eps = ABSOLUTE * np.maximum(1.0, largest) + RELATIVE * largest
    return beta, 2 * eps * np.abs(rows).sum(axis=1) + m * eps * eps + m * 2.0 ** -52 * beta


@pytest.mark.parametrize("m", sorted(dual_se_lps.SE_WALK_CASES))
def test_pivot_for_pivot_the_weights_and_the_certified_optimum(m):
    case, child, basis = walk_child(m)
    basis = list(basis)
    assert child.dual_refusal(**STEEPEST) == "" and child.kernel_path(**STEEPEST)["ratio_textbook"]
    reference = dual_se_lps.DualSteepestReference(child, basis)
    expected_reason = reference.run()
    dual_lps.assert_walk_conditions(reference, m, expected_reason)
    plain = dual_lps.DualReference(child, basis)
    plain.run()
    assert plain.pivots[0] != reference.pivots[0]  # (the first pivot already tells the rules apart)
    solver = relp_amd.Solver(certify=1, **STEEPEST).load_model(child)
    try:
        n_art = solver.n_art
        solver.begin_dual(basis)
        assert solver.dual_pivots() == 0 and solver.record()["dual_pricing"] == "steepest_edge"
        start = dual_se_lps.DualSteepestReference(child, basis)
        beta, bound = weight_bounds(start.inverse)
        assert (np.abs(solver.dual_weights() - beta) <= bound).all(), "the weights of the start"
        for step, (q, p, leaving) in enumerate(reference.pivots):
            assert solver.iterate_dual(1) == (1, relp_amd.STOP_BUDGET), step
            assert solver.last_pivot() == (3, n_art + q, p, n_art + leaving), step
        assert solver.iterate_dual(1) == (0, expected_reason)
        assert solver.dual_pivots() == len(reference.pivots) and list(solver.basis()) == reference.basis
        beta, bound = weight_bounds(reference.inverse)
        weights = solver.dual_weights()
        error = np.abs(weights - beta)
        print("m = %d, weights after %d dual pivots: worst error / bound %.2e, worst relative error %.2e" % (
            m, len(reference.pivots), float((error / bound).max()), float((error / beta).max())))
        assert (weights > 0).all()
        assert (error <= bound).all(), ("weight of row", int(np.argmax(error / bound)), float((error / bound).max()))
    finally:
        solver.close()
    solver = relp_amd.Solver(certify=1, **STEEPEST).load_model(child)
    try:
        result = solver.solve_dual(basis)
        assert result.kind == relp_amd.FINITE_OPTIMUM and result.certified == 1
        assert solver.dual_pivots() == len(reference.pivots) == solver.record()["dual_pivots"]
        warm = solver.objective_exact()
    finally:
        solver.close()
    cold, cold_result = cold_objective(child)
    assert warm == cold
    print("m = %d: %d dual pivots (largest infeasibility: %d) against %d cold pivots, smallest margin %.3g" % (
        m, len(reference.pivots), len(plain.pivots), cold_result.pivots_phase_one + cold_result.pivots_phase_two, reference.smallest_margin()))


@pytest.mark.parametrize("m", [513, 2049])
def test_the_weights_track_the_inverse(m):
    seed, n_cuts = dual_lps.STATE_CASES[m]
    case = dual_lps.cut_case(m, dual_lps.MIXED, seed, n_cuts)
    options = dict(OPTIONS, **STEEPEST)
    plan = case.parent.kernel_path(**options)
    for field, value in expected_plan(m).items():  # (before the device is touched)
        assert plan[field] == value, (field, plan[field], value)
    child, basis, _ = case.child(*solved_parent(case))
    plan = child.kernel_path(**options)
    assert child.dual_refusal(**options) == "" and plan["ratio_textbook"]
    for field, value in expected_plan(m).items():
        assert plan[field] == value, (field, plan[field], value)
    solver = relp_amd.Solver(**options).load_model(child)
    try:
        solver.begin_dual(basis)
        done, reason = solver.iterate_dual(16)
        assert done >= 8 and (reason == relp_amd.STOP_BUDGET) == (done == 16), (done, reason)
        weights = solver.dual_weights()
        inverse = np.stack([solver.basis_inverse_row(k) for k in range(solver.m)])
        norms = (inverse * inverse).sum(axis=1)
        relative = np.abs(weights - norms) / norms
        print("m = %d (%d rows), %d dual pivots: weights against the row norms of the device's inverse, worst relative difference %.2e (m 2^-52 = %.2e)" % (
            m, solver.m, done, float(relative.max()), solver.m * 2.0 ** -52))
        assert (weights > 0).all()
        assert (relative <= solver.m * 2.0 ** -52).all(), ("weight of row", int(np.argmax(relative)), float(relative.max()))
        report = {}
        assert_residuals(solver, sparse_lps.Provider(child), btrans(solver.m), report=report)
        print("m = %d: %s" % (m, "  ".join("%s %.1e" % item for item in sorted(report.items()))))
    finally:
        solver.close()
    solver = relp_amd.Solver(polish_period=0, certify=1, **STEEPEST).load_model(child)
    try:
        result = solver.solve_dual(basis)
        assert result.kind == relp_amd.FINITE_OPTIMUM and result.certified == 1
        warm, pivots, clean_up = solver.objective_exact(), solver.dual_pivots(), result.pivots_phase_two
    finally:
        solver.close()
    cold, cold_result = cold_objective(child)
    assert warm == cold
    print("m = %d: solve_dual %d dual + %d primal pivots under the steepest-edge rule, cold %d" % (
        m, pivots, clean_up, cold_result.pivots_phase_one + cold_result.pivots_phase_two))


def test_the_start_from_the_parent():
    m = 64
    seed, n_cuts = dual_se_lps.SE_WALK_CASES[m]
    case = dual_lps.cut_case(m, dual_lps.MIXED, seed, n_cuts)
    parent = relp_amd.Solver(certify=1).load_model(case.parent)
    try:
        result = parent.solve_relaxation()
        assert result.kind == relp_amd.FINITE_OPTIMUM and result.certified
        child, basis, _ = case.child(parent.basis(), parent.solution_exact())
        solver = relp_amd.Solver(certify=1, **STEEPEST).load_model(child)
        try:
            result = solver.solve_dual_from(parent, basis)
            assert result.kind == relp_amd.FINITE_OPTIMUM and result.certified == 1
            record = solver.record()
            assert record["dual_pricing"] == "steepest_edge" and record["dual_start"] == "inherited"
            warm = solver.objective_exact()
        finally:
            solver.close()
    finally:
        parent.close()
    assert warm == cold_objective(child)[0]


def test_the_default_rule_is_untouched():
    _, child, basis = walk_child(64)
    basis = list(basis)
    solver = relp_amd.Solver().load_model(child)
    try:
        with pytest.raises(RelpError) as unstarted:
            solver.dual_weights()
        assert unstarted.value.status == ERR_STATE
        solver.begin_dual(basis)
        with pytest.raises(RelpError, match="dual_pricing") as refused:
            solver.dual_weights()
        assert refused.value.status == ERR_STATE
        assert solver.record()["dual_pricing"] == "infeasibility"
        before = int(solver.stats().launches)
        assert solver.iterate_dual(4) == (4, relp_amd.STOP_BUDGET)
        assert int(solver.stats().launches) - before == 1 + 5 * 4  # the budget, then five launches per pivot: one batch
    finally:
        solver.close()
    solver = relp_amd.Solver(**STEEPEST).load_model(child)
    try:
        with pytest.raises(RelpError, match="begin_dual comes first") as unstarted:
            solver.dual_weights()
        assert unstarted.value.status == ERR_STATE
        solver.begin_dual(basis)
        before = int(solver.stats().launches)
        assert solver.iterate_dual(4) == (4, relp_amd.STOP_BUDGET)
        assert int(solver.stats().launches) - before == 1 + 6 * 4  # ... and the weights behind each pivot (68 rows: one slice)
    finally:
        solver.close()
