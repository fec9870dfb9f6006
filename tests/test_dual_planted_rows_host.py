"""The planted rows of tests/dual_planted_rows.py on the exact reference alone (no GPU): every case hits the branch of the long-step
kernels it is named for, or the device comparison of tests/test_gpu_dual_long_step_edges.py would prove nothing.

Per case (``dual_planted_rows.assert_conditions`` and the case's own ``check``): the start is the identity with basic costs 0; the
numbers of boxed and un-bounded candidates at the planted pivot, the size of F and the place of the entering column in the order;
the column numbers against 8192; the ties, as equal ``Fraction`` ratios; ``behind`` against the floor; the column lengths against
1024; the held forms in F; the side; dual feasibility of every signed cost before and after every pivot; the plan takes the LP and
resolves the ratio rule the case is about.  Up to m = 8 and n = 100 the final objective is the oracle's ``Formulation.solve()``; the
wide and long cases end dual feasible and ``feasible()``.  Two kinds of case cannot end at the oracle's vertex, and say why below.

The sizes the cases are planted around (2048 slots, 32 flips, 8192 columns per trip, 1024 entries per chunk) are compared with the
``constexpr`` lines of relp_amd/csrc/dual.hpp and dual.hip, read as text.
"""
import os
import re
from fractions import Fraction

import pytest

import relp_amd
import dual_long_step_lps as lps
import dual_planted_rows as planted

CSRC = os.path.join(os.path.dirname(os.path.abspath(relp_amd.__file__)), "csrc")


def constant(file_name, name):
    with open(os.path.join(CSRC, file_name)) as source:
        found = re.findall(r"^constexpr int %s = (\d+);" % name, source.read(), flags=re.MULTILINE)
    assert len(found) == 1, (file_name, name, found)
    return int(found[0])


def test_the_planted_sizes_are_the_kernels_constants():
    assert planted.SLOTS == constant("dual.hpp", "DUAL_LONG_STEP_SLOTS") == 2048
    assert planted.MAX_FLIPS == lps.DUAL_MAX_FLIPS == constant("dual.hpp", "DUAL_MAX_FLIPS") == 32
    assert planted.SCAN == constant("dual.hip", "DL_U") * constant("dual.hip", "DL_THREADS") == 8192
    assert planted.CHUNK == constant("dual.hip", "DL_COL_CHUNK") == 1024
    assert planted.LONG_ROWS == planted.CHUNK + 1


@pytest.mark.parametrize("name", sorted(planted.CASES))
def test_a_planted_case_hits_its_branch_on_the_reference_alone(name):
    case, reference = planted.assert_conditions(name)
    form = case.form
    options = dict(implicit_bounds=1, polish_period=0, **case.options)
    assert form.model.dual_bounded_refusal(**options) == ""
    assert form.model.kernel_path(**options)["ratio_textbook"] is (not case.harris)
    if name in planted.TEXTBOOK_BY_DATA:
        assert case.options == {} and form.model.kernel_path(implicit_bounds=1)["ratio_textbook"] is True
    if form.m > planted.ORACLE_MAX_ROWS or form.ns > planted.ORACLE_MAX_COLUMNS:
        return
    optimum = form.solve().objective
    floor, tol_dual, _ = planted.handle_tolerances()
    if case.harris:
        # The Harris rule trades up to tol_dual of dual feasibility for the larger pivot: the final basis is optimal for the costs
        # c + e with e_j = -d_j on the columns whose signed cost ended below 0 (all of them un-complemented at 0 here), so
        # c.x* <= c.x = (c + e).x <= (c + e).x* <= c.x* + tol_dual sum x*_j over the oracle's vertex x*.
        negative = [j for j, c in enumerate(reference.signed_costs()) if c is not None and c < 0]
        assert negative and all(reference.pos[j] == -1 for j in negative)
        total = sum((v for j, v in form.solve().solution if j < form.ns), Fraction(0))
        assert optimum <= reference.objective() <= optimum + tol_dual * total
    elif case.within_floor:
        # The walk stops with one row above its bound by 2^-40 <= harris_delta, which the device calls feasible: a dual feasible basis
        # of an LP that is infeasible by that much bounds the optimum from below; with the floor 0 the same LP walks to the optimum.
        assert reference.objective() < optimum
        exact = lps.LongStepBoundedDualReference(form, case.basis)
        assert exact.run() == relp_amd.STOP_NO_ENTERING and exact.feasible() and exact.objective() == optimum
    else:
        assert reference.feasible() and reference.objective() == optimum


@pytest.mark.parametrize("name", sorted(planted.CASES))
def test_the_kernels_organisation_of_the_walk_passes_what_the_reference_passes(name):
    """``kernel_walk_model`` restates the kernel's walk (one arg-min per round, the un-bounded candidates folded to their minimum);
    the reference sorts.  At every pivot of every case the two pass the same columns and agree on the overflow."""
    _, reference, _, _, _, _ = planted.walked(name)
    for walk in reference.walks:
        assert planted.kernel_walk_model(walk, reference.ub, reference.slope_floor) == (walk["passed"], walk["overflow"])


def test_the_tie_cases_tell_the_column_rule_from_its_absence():
    """Without the clause ``(int)free_rank < j`` the kernel would stop at an un-bounded candidate whenever a boxed one has the same
    ratio: the restated walk without it passes fewer columns on exactly the two rows where the boxed column is the lower one."""
    differs = []
    for name in sorted(planted.CASES):
        _, reference, _, _, _, _ = planted.walked(name)
        walk = reference.walks[0]
        if planted.kernel_walk_model(walk, reference.ub, reference.slope_floor, column_breaks_ties=False)[0] != walk["passed"]:
            differs.append(name)
    assert differs == ["tie_all_zero", "tie_unbounded_higher"]


def test_the_floor_and_the_limits_default_to_the_rule_the_reference_had():
    """``slope_floor = 0`` and ``slots = None``: the walk of a chosen case of tests/dual_long_step_lps.py, pivot for pivot."""
    reference = lps.walked(5)[0]
    _, _, child, basis, _, _ = lps.long_step_case(5)
    again = lps.LongStepBoundedDualReference(child, basis, slope_floor=0, slots=None)
    assert again.run() == relp_amd.STOP_NO_ENTERING
    assert again.pivots == reference.pivots and again.flips == reference.flips and again.skipped == 0
