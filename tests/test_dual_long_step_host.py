"""The host side of the long-step (bound-flipping) ratio test of the bounded dual loop (no GPU): the C ABI's new symbol, and the inputs
of the pivot-for-pivot GPU cases -- ``dual_long_step_lps.LONG_STEP_CASES`` -- checked with the exact reference alone.

``relp_set_dual_long_step`` needs a handle to refuse a value on, and a handle needs a device: without one this file can only see that
2 and -1 are not accepted where the handle is missing either; tests/test_gpu_dual_long_step.py refuses them on a live handle and reads
the message.
"""
import ctypes as C

import numpy as np
import pytest

import relp_amd
from relp_amd import api
from relp_amd.api import ERR_ARGUMENT
import dual_bounded_lps
import dual_long_step_lps as lps

CASES = [(m, which) for m in sorted(lps.LONG_STEP_CASES) for which in range(len(lps.LONG_STEP_CASES[m]))]


def test_the_symbol_exists():
    lib = relp_amd.lib()
    assert hasattr(lib, "relp_set_dual_long_step") and "relp_set_dual_long_step" in relp_amd.SYMBOLS
    assert callable(relp_amd.Solver.set_dual_long_step)
    import inspect
    assert inspect.signature(relp_amd.Solver.solve_dual_bounded).parameters["long_step"].default is None


def test_a_call_without_a_handle_answers_as_its_neighbours_do():
    lib = relp_amd.lib()
    basis = np.zeros(4, dtype=np.int32)
    expected = lib.relp_begin_dual_bounded(None, basis.ctypes.data_as(C.POINTER(C.c_int32)))
    assert expected == ERR_ARGUMENT
    for value in (0, 1, 2, -1):
        assert lib.relp_set_dual_long_step(None, value) == expected


def test_the_options_layout_is_untouched():
    options = api.default_options()
    assert options.dual_pricing == 0 and options.reserved_round7 == 0
    assert C.sizeof(api.Options) == api.Options.reserved_round7.offset + 4
    assert api.Options.dual_pricing.offset == api.Options.carry_weights_min.offset + 8
    assert not any("long_step" in name for name, _ in api.Options._fields_)


@pytest.mark.parametrize("m,which", CASES)
def test_the_chosen_cases_meet_their_conditions(m, which):
    reference, reason, facts, _, dual_feasible, _ = lps.walked(m, which)
    print("m = %d, case %s: %s" % (m, lps.LONG_STEP_CASES[m][which], facts))
    lps.assert_long_step_conditions(reference, m, reason, facts, dual_feasible)
    _, _, child, _, _, _ = lps.long_step_case(m, which)
    assert reference.objective() == child.solve().objective


def test_the_steepest_edge_case_meets_its_conditions():
    reference, reason, facts, _, dual_feasible, _ = lps.walked(64, steepest=True)
    print("m = 64, steepest edge, case %s: %s" % (lps.STEEPEST_CASE[64], facts))
    lps.assert_long_step_conditions(reference, 64, reason, facts, dual_feasible)
    plain, _ = lps.plain_walked(64, steepest=True)
    assert reference.objective() == plain.objective() and reference.pivots != plain.pivots


@pytest.mark.parametrize("m,which", CASES)
def test_the_plain_and_the_long_step_rule_agree_on_the_objective_and_not_on_the_walk(m, which):
    reference = lps.walked(m, which)[0]
    plain, _ = lps.plain_walked(m, which)
    assert reference.objective() == plain.objective()
    assert reference.pivots != plain.pivots  # (otherwise the comparison on the device shows nothing)
    assert len(reference.pivots) <= len(plain.pivots)
    print("m = %d: %d pivots and %d flips against %d pivots of the plain rule" % (m, len(reference.pivots), reference.total_flips(), len(plain.pivots)))


@pytest.mark.parametrize("m", [5, 64])
def test_the_cap_of_one_flip_per_pivot_ends_at_the_same_objective(m):
    _, _, child, basis, _, _ = lps.long_step_case(m)
    capped = lps.LongStepBoundedDualReference(child, basis, max_flips=1)
    assert capped.run() == relp_amd.STOP_NO_ENTERING and capped.feasible()
    assert max(len(passed) for passed in capped.flips) == 1
    assert capped.objective() == lps.walked(m)[0].objective()


def test_no_flip_allowed_is_the_plain_rule():
    _, _, child, basis, _, _ = lps.long_step_case(5)
    capped = lps.LongStepBoundedDualReference(child, basis, max_flips=0)
    assert capped.run() == relp_amd.STOP_NO_ENTERING
    assert capped.pivots == lps.plain_walked(5)[0].pivots and capped.total_flips() == 0


def test_the_search_reproduces_a_chosen_case():
    seed, n_cuts, n_tight = lps.LONG_STEP_CASES[5][0]
    found, facts = lps.search(5, [seed], [(n_cuts, n_tight)])
    assert found == (seed, n_cuts, n_tight) and facts["flips"] >= 1
    assert dual_bounded_lps.MARGIN == lps.MARGIN
