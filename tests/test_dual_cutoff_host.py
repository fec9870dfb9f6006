"""The objective cutoff of the dual simplex on a machine without a GPU: ``relp_set_dual_cutoff`` is declared and exported and refuses a
null handle as its sibling does, the Python entry points take the keyword, ``relp_amd.witness.check_dual_bound`` accepts and refuses what
it should on the two hand LPs, and the references alone meet the conditions tests/test_gpu_dual_cutoff.py rests on: the objective
paths of the hand LPs, and at least three pivots with a usable rise of the objective on each of the six walks."""
import inspect
import math
import os
import re
from fractions import Fraction

import pytest

import relp_amd
from relp_amd.api import ERR_ARGUMENT
from relp_amd.witness import WitnessError, check_dual_bound
import dual_bounded_lps
import dual_cutoff_lps as lps
import dual_lps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_header_declares_the_setter_the_result_kind_and_the_stop_reason():
    text = open(os.path.join(ROOT, "include", "relp_amd.h")).read()
    assert re.search(r"^int32_t relp_set_dual_cutoff\(relp_handle\* handle, int32_t on, double cutoff\);$", text, re.M)
    assert text.index("int32_t relp_set_dual_farkas(") < text.index("int32_t relp_set_dual_cutoff(")
    assert re.search(r"^\s*RELP_RESULT_CUTOFF = 5\b", text, re.M)
    for key in ('"dual_cutoff"', '"dual_cutoff_stopped"', '"dual_bound_proved"', "stop reason 6"):
        assert key in text, key


def test_the_symbol_and_the_constants_are_exported():
    assert "relp_set_dual_cutoff" in relp_amd.SYMBOLS and hasattr(relp_amd.lib(), "relp_set_dual_cutoff")
    assert relp_amd.CUTOFF == 5 and relp_amd.STOP_CUTOFF == 6
    assert relp_amd.check_dual_bound is check_dual_bound


def test_a_null_handle_answers_as_the_sibling_setter_does():
    lib = relp_amd.lib()
    for on in (0, 1, 2):
        for cutoff in (0.0, math.inf, math.nan):
            assert lib.relp_set_dual_cutoff(None, on, cutoff) == lib.relp_set_dual_farkas(None, on) == ERR_ARGUMENT


def test_the_four_solves_take_the_keyword_and_keep_the_order_of_the_ones_they_had():
    for name in ("solve_dual", "solve_dual_from", "solve_dual_bounded", "solve_dual_bounded_from"):
        parameters = inspect.signature(getattr(relp_amd.Solver, name)).parameters
        assert parameters["cutoff"].default is None and parameters["cutoff"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD, name
    for name in ("solve_dual", "solve_dual_from"):  # behind the keyword they had
        assert list(inspect.signature(getattr(relp_amd.Solver, name)).parameters)[-2:] == ["farkas", "cutoff"], name
    for name in ("solve_dual_bounded", "solve_dual_bounded_from"):  # tests/test_dual_farkas_abi.py pins their last two: in front of those
        assert list(inspect.signature(getattr(relp_amd.Solver, name)).parameters)[-3:] == ["cutoff", "long_step", "farkas"], name
    assert "relp_set_dual_cutoff" in inspect.getdoc(relp_amd.Solver.set_dual_cutoff)


def test_check_dual_bound_on_the_plain_hand_lp():
    model, _ = lps.hand_plain()
    check_dual_bound(model, {1: 2}, 8)
    check_dual_bound(model, {}, 0)
    check_dual_bound(model, {0: Fraction(-1), 1: Fraction(3)}, "11/1")
    # y = {1: 4} prices y at d_y = 3 - 4 = -1, but x before it at d_x = 2 - 4 = -2: the first violated column is named.  With
    # y_0 = -2 beside it x prices 0 and column 1 is the only one that fails.
    with pytest.raises(WitnessError) as refused:
        check_dual_bound(model, {1: 4}, 16)
    assert refused.value.condition == "c_j - y'a_j >= 0" and refused.value.where == ("column", 0) and "-2" in str(refused.value)
    with pytest.raises(WitnessError) as refused:
        check_dual_bound(model, {0: -2, 1: 4}, 14)
    assert refused.value.condition == "c_j - y'a_j >= 0" and refused.value.where == ("column", 1) and "-1" in str(refused.value)
    with pytest.raises(WitnessError) as refused:
        check_dual_bound(model, {1: 2}, 9)
    assert refused.value.condition == "y'b + fixed cost = value" and refused.value.where is None


def test_check_dual_bound_on_the_bounded_hand_lp():
    form, _ = lps.hand_bounded()
    assert form.model.nr_rows == 2 and form.model.right_hand_side_exact() == [4, 1]  # the constraint row, then the bound row
    check_dual_bound(form.model, {0: 3, 1: -1}, 11)
    check_dual_bound(form.model, {0: 2}, 8)
    with pytest.raises(WitnessError) as refused:  # without the bound row's multiplier x prices 2 - 3
        check_dual_bound(form.model, {0: 3}, 12)
    assert refused.value.where == ("column", 0)
    assert lps.closed_form_value(form, {0: 3}) == ({1: Fraction(-1)}, 11) and lps.closed_form_value(form, {0: 2}) == ({}, 8)


def test_the_objective_paths_of_the_hand_lps():
    model, basis = lps.hand_plain()
    states, usable = lps.walk_with_cutoffs(dual_lps.DualReference(model, basis))
    assert [s["objective"] for s in states] == lps.HAND_OBJECTIVES and [s["basis"] for s in states] == lps.HAND_PLAIN_BASES
    assert [s["pi"] for s in states] == [[0, 0], [0, 2], [-1, 3]] and usable == [(1, 4.0), (2, 9.5)]
    form, basis = lps.hand_bounded()
    states, usable = lps.walk_with_cutoffs(dual_bounded_lps.BoundedDualReference(form, basis))
    assert [s["objective"] for s in states] == lps.HAND_OBJECTIVES and [s["basis"] for s in states] == lps.HAND_BOUNDED_BASES
    assert [s["pi"] for s in states] == [[0], [2], [3]] and usable == [(1, 4.0), (2, 9.5)]


@pytest.mark.parametrize("m", sorted(dual_lps.WALK_CASES))
@pytest.mark.parametrize("bounded", [False, True], ids=["plain", "bounded"])
def test_every_walk_has_three_usable_pivots(m, bounded):
    if bounded:
        reference = dual_bounded_lps.BoundedDualReference(*lps.bounded_walk_case(m))
    else:
        child, basis = lps.plain_walk_case(m)
        reference = dual_lps.DualReference(child, basis)
    states, usable = lps.walk_with_cutoffs(reference)
    assert len(usable) >= 3, (len(states) - 1, usable)
    rises = [float((states[k]["objective"] - states[k - 1]["objective"]) / max(abs(states[k - 1]["objective"]), abs(states[k]["objective"]), 1))
             for k, _ in usable]
    assert min(rises) >= lps.MIN_RISE
    for k, cutoff in usable:  # the cutoff separates the objectives before and after pivot k, and so every earlier one from every later one
        assert all(s["objective"] < Fraction(cutoff) for s in states[:k]) and all(s["objective"] >= Fraction(cutoff) for s in states[k:])
    print("m = %d %s: %d of %d pivots usable, smallest relative rise %.2g" % (m, "bounded" if bounded else "plain", len(usable), len(states) - 1, min(rises)))
