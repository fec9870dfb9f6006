"""The kernel edges of the long-step ratio test on the device (``-m gpu``, a real MI355X): the planted rows of
tests/dual_planted_rows.py, pivot for pivot against the exact reference of tests/dual_long_step_lps.py with the kernel's slot limit,
flip cap and slope floor (``harris_delta`` of the handle's options), and with the Harris subclass where the case is about that rule.

Every test runs one case on a fresh handle.  Before the planted pivot it asserts the construction on the device -- ``n_art == 0``,
every row of the inverse equal to the unit row ``+-e_i`` and x_B equal to the planted values, entry for entry with no tolerance -- so
a start that loses exactness fails there and not in a tie.  After every ``iterate_dual(1)``: ``last_pivot() == (3, q, p, leaving)``,
the formulation's basis (a flipped column shows there), and the cumulative ``record()["dual_flips"]`` and
``record()["dual_long_step_skipped"]`` are the reference's.  After the walk the state is held to ``assert_held_state`` of
tests/test_gpu_dual_bounded.py with the tolerances of tests/state_checks.py; this file has no tolerance of its own.  What each case
plants, and that it hits its branch on the reference alone, is tests/test_dual_planted_rows_host.py's; the same conditions are
asserted again here before a case is used.

m = 1025 (long columns): the expected state is the reference's (``BoundedDualReference`` machinery, about 1.5 s of CPU for the one
pivot), not a closed form; rows 0, 512 and 1024 of the inverse are compared, and x_B, the objective and the relative costs in full.

Largest device error per part after the walk, measured on an MI355X (scales as in tests/state_checks.py):

  slots, 2048 boxed: 2 dual pivots, 3 flips; 2049 boxed: 3 dual pivots, 2 flips, 1 skipped:   every part 0
  cap, 32 / 33 / 34 / 40 / 40 on the upper side: 1, 1, 2, 2, 2 dual pivots, 31, 32, 32, 38, 38 flips:   every part 0
  wide (8504 device columns), the three rows: 1 dual pivot, 2 flips each:                       every part 0
  tie, two boxed / width zero:                                                                  every part 0
  tie, unbounded lower:   inverse 1.9e-17  x_B 0        objective 0  costs 0
  tie, unbounded higher:  inverse 1.9e-17  x_B 4.9e-17  objective 0  costs 0
  tie, all zero:          inverse 3.7e-17  x_B 4.9e-17  objective 0  costs 0
  floor, the four rows; long columns (m = 1025); harris, both rows:                             every part 0

(0: the device's f64 value is the exact one rounded.  The three tie rows pivot on 3, the only pivot here that is no power of two.)
Every figure is a value one of these tests printed on the device; the slowest case is the one of m = 1025, 1.8 s, most of it the
reference's; the others take 0.4 s at the most.
"""
from fractions import Fraction

import numpy as np
import pytest

import relp_amd
import dual_planted_rows as planted
from test_gpu_dual_bounded import assert_held_state

pytestmark = pytest.mark.gpu


def exactly(values):
    """The planted values as doubles; every one of them is a double."""
    out = [float(v) for v in values]
    assert all(v == w for v, w in zip(values, map(Fraction, out))), "a planted value is no double"
    return np.array(out, dtype=np.float64)


def walk_on_the_device(name, inverse_rows=None):
    """The walk of a planted case step by step on a fresh handle, then the state checks."""
    case, reference = planted.assert_conditions(name)
    _, _, _, bases, start, _ = planted.walked(name)
    form, m = case.form, case.form.m
    options = dict(implicit_bounds=1, polish_period=0, **case.options)
    assert form.model.kernel_path(**options)["ratio_textbook"] is (not case.harris)
    if name in planted.TEXTBOOK_BY_DATA:
        assert form.model.kernel_path(implicit_bounds=1)["ratio_textbook"]
    at_start = case.reference()
    solver = relp_amd.Solver(**options).load_model(form.model)
    try:
        assert solver.n_art == 0
        solver.set_dual_long_step(True)
        solver.begin_dual_bounded(case.basis)
        record = solver.record()
        assert record["dual_bounded"] is True and record["dual_long_step"] is True
        assert record["dual_flips"] == 0 and record["dual_long_step_skipped"] == 0
        assert set(solver.basis()) == set(start)
        for i in range(m):  # the preconditions of the planted pivot: exact, no tolerance
            assert np.array_equal(solver.basis_inverse_row(i)[:m], exactly(at_start.inverse[i])), ("the start inverse is not the unit row", i)
        assert np.array_equal(solver.b()[:m], exactly(at_start.x)), "x_B at the start is not the planted one"
        flips = skipped = 0
        for step, (q, p, leaving, _) in enumerate(reference.pivots):
            assert solver.iterate_dual(1) == (1, relp_amd.STOP_BUDGET), step
            told = (step, reference.pivots[step], reference.flips[step])
            assert solver.last_pivot() == (3, q, p, leaving), told
            assert set(solver.basis()) == set(bases[step]), told
            flips += len(reference.flips[step])
            skipped += int(reference.walks[step]["overflow"])
            record = solver.record()
            assert record["dual_flips"] == flips and record["dual_long_step_skipped"] == skipped, told
        assert solver.iterate_dual(1) == (0, relp_amd.STOP_NO_ENTERING)
        assert solver.dual_pivots() == len(reference.pivots) and skipped == reference.skipped and flips == reference.total_flips()
        assert_held_state(solver, reference, "%s: state after %d dual pivots, %d flips, %d skipped" % (
            case.name, len(reference.pivots), flips, skipped), rows=inverse_rows)
    finally:
        solver.close()


@pytest.mark.parametrize("name", ["slots_2048", "slots_2049"])
def test_a_row_that_fits_the_slots_exactly_flips_and_one_more_candidate_skips_once(name):
    walk_on_the_device(name)


@pytest.mark.parametrize("name", ["cap_32", "cap_33", "cap_34", "cap_40", "cap_40_upper"])
def test_the_cap_of_32_flips_and_both_held_forms_in_one_flip_set(name):
    walk_on_the_device(name)


@pytest.mark.parametrize("name", ["wide_passed", "wide_unbounded", "wide_entering"])
def test_candidates_in_the_second_trip_of_the_column_scans(name):
    walk_on_the_device(name)


@pytest.mark.parametrize("name", ["tie_two_boxed", "tie_unbounded_lower", "tie_unbounded_higher", "tie_all_zero", "tie_width_zero"])
def test_ties_are_broken_by_the_column_under_the_textbook_rule(name):
    walk_on_the_device(name)


@pytest.mark.parametrize("name", ["floor_zero", "floor_zero_passed", "floor_below", "floor_above"])
def test_the_slope_floor_is_harris_delta(name):
    walk_on_the_device(name)


def test_flipped_and_entering_columns_longer_than_one_chunk():
    walk_on_the_device("long_columns", inverse_rows=(0, planted.LONG_P, planted.LONG_ROWS - 1))


@pytest.mark.parametrize("name", ["harris_free", "harris_boxed"])
def test_the_harris_rule_chooses_outside_the_flip_set(name):
    walk_on_the_device(name)
