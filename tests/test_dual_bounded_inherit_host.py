"""The host side of the inherited start on implicit upper bounds (no GPU): the three new symbols of the C ABI, and
``Model.dual_bounded_inherit_refusal`` -- the pure function ``dual_bounded_inherit_refusal`` of relp_amd/csrc/dual_inherit.cpp behind
``relp_debug_dual_bounded_inherit_refusal`` -- over the pairs of tests/dual_bounded_lps.py it takes and every pair it refuses, with
the place named.  The parent's basis is the oracle's optimal one, the child's ``dual_bounded_lps.extended_basis`` of it.

The same function and the reduction it shares with ``Solver::place_basis`` (``reduce_bounded_basis``) are run stand-alone under
``-fsanitize=address,undefined`` (tests/support/dual_bounded_inherit_check.cpp), the way tests/test_dual_inherit_host.py runs its
driver.

The last two tests are the CPU-side conditions of the two-generation case of tests/test_gpu_dual_bounded_inherit.py, asserted with the
exact ``BoundedDualReference`` alone: the finished first-generation walk (m = 64 + 4 cuts, 27 pivots) leaves 1 basic column held
complemented; ``place_basis`` puts the grandchild's columns at other positions than that walk left them (67 of 68, the basis being
passed in column order); the grandchild's walk (34 pivots, 4 at the upper side, 5 complemented columns entering, smallest margin
2.1e-3) meets ``assert_walk_conditions``.
"""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import relp_amd
from relp_amd.api import CARRY_LU, ERR_ARGUMENT, Result
import dual_bounded_inherit_lps as gen
import dual_bounded_lps as lps
import dual_lps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("relp_begin_dual_bounded_from", "relp_solve_dual_bounded_from", "relp_debug_dual_bounded_inherit_refusal")


def test_the_symbols_exist():
    lib = relp_amd.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in relp_amd.SYMBOLS
    for name in ("begin_dual_bounded_from", "solve_dual_bounded_from"):
        assert callable(getattr(relp_amd.Solver, name))
    assert callable(relp_amd.Model.dual_bounded_inherit_refusal)
    header = open(os.path.join(ROOT, "include", "relp_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert "int32_t %s(" % name in header, name


def test_null_arguments_are_refused():
    lib = relp_amd.lib()
    basis = np.zeros(16, dtype=np.int32)
    pointer = basis.ctypes.data_as(C.POINTER(C.c_int32))
    result = Result()
    assert lib.relp_begin_dual_bounded_from(None, None, pointer) == ERR_ARGUMENT
    assert lib.relp_solve_dual_bounded_from(None, None, pointer, C.byref(result)) == ERR_ARGUMENT
    assert lib.relp_debug_dual_bounded_inherit_refusal(None, None, None, None, None, None, 0, None) == ERR_ARGUMENT
    model = lps.walk_case(5)[0].parent.model
    assert lib.relp_debug_dual_bounded_inherit_refusal(model._h, model._h, None, pointer, None, None, 0, None) == ERR_ARGUMENT
    assert lib.relp_debug_dual_bounded_inherit_refusal(model._h, None, pointer, pointer, None, None, 0, None) == ERR_ARGUMENT


class Pair:
    """``walk_case(m)``: the parent with the oracle's optimal basis, the child (cuts, tightened bounds, one new bound row) with its
    extension, and what the variants below are made of."""

    def __init__(self, m):
        self.m = m
        self.case, self.optimum, self.child, self.basis, self.cuts, self.branches = lps.walk_case(m)
        self.parent = self.case.parent
        self.parent_basis = [int(c) for c in self.optimum.basis]
        self.reduced = lps.BoundedDualReference(self.child, self.basis)  # (its constructor is the reduction of place_basis)

    def variant(self, columns=None, b=None, upper=None, n_greater=0):
        child = self.child
        return lps.Formulation(child.columns if columns is None else columns, child.b if b is None else b, child.cost,
                               child.upper if upper is None else upper, n_greater=n_greater)

    def refusal(self, child=None, basis=None, parent_basis=None, **options):
        child = self.child if child is None else child
        options.setdefault("implicit_bounds", 1)
        return child.model.dual_bounded_inherit_refusal(self.parent.model, self.parent_basis if parent_basis is None else parent_basis,
                                                        self.basis if basis is None else basis, **options)

    def basic_structural(self):
        """A structural column of the child's reduced basis that has an entry on the parent's rows: ``(position, column, row, value)``."""
        for position, column in enumerate(self.reduced.basis):
            if column < self.child.ns:
                row, value = next((i, v) for i, v in self.child.columns[column] if i < self.parent.m)
                return position, column, row, value
        raise AssertionError("the optimal basis holds no structural column")


@pytest.fixture(scope="module", params=sorted(lps.WALK_CASES))
def pair(request):
    return Pair(request.param)


def test_the_walk_case_is_taken(pair):
    """Cuts, tightened bounds and one new bound row: the bound slacks' numbers shift between the two models."""
    assert pair.child.m == pair.parent.m + len(pair.cuts) and pair.child.rows > pair.parent.rows + len(pair.cuts)
    assert pair.refusal() == ""
    assert pair.refusal(basis=gen.by_column(pair.child, pair.basis)) == ""  # positions need not agree


def test_a_pure_branch_is_taken(pair):
    _, optimum, child, basis, branches = gen.pure_branch(pair.m, n_tight=min(8, lps.WALK_CASES[pair.m][2]))
    assert child.m == pair.parent.m and child.rows == pair.parent.rows and branches
    assert list(basis) == [int(c) for c in optimum.basis]
    assert child.model.dual_bounded_inherit_refusal(pair.parent.model, pair.parent_basis, basis, implicit_bounds=1) == ""
    # ... and costs and right-hand sides may differ too
    other = lps.Formulation(child.columns, [v + 1 for v in child.b], [c + 1 for c in child.cost], child.upper)
    assert other.model.dual_bounded_inherit_refusal(pair.parent.model, pair.parent_basis, basis, implicit_bounds=1) == ""


def test_a_pair_without_bounds_is_taken_by_the_same_rule():
    seed, n_cuts = dual_lps.WALK_CASES[64]
    case = dual_lps.cut_case(64, dual_lps.MIXED, seed, n_cuts)
    slack_basis = [column for _, column in sorted(case.parent.pivot_element_indices())]
    child, basis, _ = case.child(slack_basis, {j: Fraction(1) for j in range(case.n_structural)})
    for implicit in (0, 1):  # (no bound: the option does not apply)
        assert child.dual_bounded_inherit_refusal(case.parent, slack_basis, basis, implicit_bounds=implicit) == ""
    swapped = list(basis)
    swapped[0], swapped[1] = swapped[1], swapped[0]
    assert child.dual_bounded_inherit_refusal(case.parent, slack_basis, swapped, implicit_bounds=1) == ""
    assert "position 0" in child.dual_inherit_refusal(case.parent, slack_basis, swapped)  # (the plain relation wants the parent's order)


def test_bounds_held_as_rows_are_refused(pair):
    text = pair.refusal(implicit_bounds=0)
    assert "the parent's plan" in text and "rows of the device LP" in text, text


def test_a_changed_coefficient_of_a_basic_column_is_refused_with_its_place(pair):
    position, column, row, value = pair.basic_structural()
    columns = [list(c) for c in pair.child.columns]
    columns[column] = [(i, v + 5 if i == row else v) for i, v in columns[column]]  # (entries are +-1 .. 3: never zero)
    text = pair.refusal(child=pair.variant(columns=columns))
    assert "position %d" % position in text and "structural variable %d" % column in text and "row %d" % row in text, text
    assert "%d/1 in the child, %d/1 in the parent" % (value + 5, value) in text, text
    # the same change in a column that is not basic on the device does not matter
    other = next(j for j in range(pair.child.ns) if j not in pair.reduced.basis)
    columns = [list(c) for c in pair.child.columns]
    columns[other] = [(i, v + 5) for i, v in columns[other]]
    assert pair.refusal(child=pair.variant(columns=columns)) == ""


def test_a_new_row_whose_basic_column_has_two_entries_is_refused(pair):
    """A new structural column over the first two cuts, basic on the first cut's row instead of its slack."""
    child, m = pair.child, pair.parent.m
    columns = [list(c) for c in child.columns] + [[(m, Fraction(1)), (m + 1, Fraction(1))]]
    wide = lps.Formulation(columns, child.b, child.cost + [Fraction(0)], child.upper + [None])
    shifted = [c if c < child.ns else c + 1 for c in pair.basis]  # (every slack moves up by the new column)
    assert wide.model.dual_bounded_inherit_refusal(pair.parent.model, pair.parent_basis, shifted, implicit_bounds=1) == ""
    shifted[m] = child.ns
    text = wide.model.dual_bounded_inherit_refusal(pair.parent.model, pair.parent_basis, shifted, implicit_bounds=1)
    assert "position %d" % m in text and "structural variable %d" % child.ns in text and "2 entries" in text and "rows %d and %d" % (m, m + 1) in text, text


def test_a_basis_with_an_artificial_is_refused_with_its_row(pair):
    text = pair.refusal(parent_basis=[-1] + pair.parent_basis[1:])
    assert "parent's basis holds an artificial" in text and "row 0" in text, text
    text = pair.refusal(basis=pair.basis[:-1] + [-2])  # a bound row of the formulation
    assert "child's basis holds an artificial" in text and "row %d" % (pair.child.rows - 1) in text, text


def test_a_child_with_fewer_rows_is_refused(pair):
    text = pair.parent.model.dual_bounded_inherit_refusal(pair.child.model, pair.basis, pair.parent_basis, implicit_bounds=1)
    assert "%d constraint rows, fewer than its parent's %d" % (pair.parent.m, pair.child.m) in text, text


def test_reordered_rows_are_refused_with_their_place(pair):
    """The parent's rows in reverse order: the first basic column that is not symmetric under that names its position and the row.
    (A row of another kind among the parent's is named by its index: tests/support/dual_bounded_inherit_check.cpp.)"""
    m = pair.parent.m
    columns = [sorted((m - 1 - i if i < m else i, v) for i, v in c) for c in pair.child.columns]
    b = list(reversed(pair.child.b[:m])) + list(pair.child.b[m:])
    text = pair.refusal(child=pair.variant(columns=columns, b=b))
    assert text.startswith("position ") and "of the parent on the parent's rows (row " in text, text


def test_a_plan_the_dual_kernels_do_not_take_is_refused(pair):
    text = pair.refusal(carry=CARRY_LU)
    assert "LU" in text and "the parent's plan" in text, text
    assert pair.child.model.dual_bounded_refusal(carry=CARRY_LU, implicit_bounds=1) in text


def test_a_basis_of_the_wrong_length_is_not_passed_on(pair):
    with pytest.raises(ValueError):
        pair.refusal(basis=pair.basis[:-1])


def test_the_relation_and_the_reduction_stand_alone_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "dual_bounded_inherit_check")
    csrc = os.path.join(ROOT, "relp_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                           os.path.join(ROOT, "tests", "support", "dual_bounded_inherit_check.cpp"), os.path.join(csrc, "dual_inherit.cpp"), "-o", exe])
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0 and done.stdout.strip() == "ok", (done.returncode, done.stdout, done.stderr)


def test_the_first_generation_leaves_a_complemented_basic_column_and_moved_positions():
    child, _, first = gen.first_generation()
    assert first.feasible() and gen.complemented_basic(first) >= 1
    form, basis, cuts, branches = gen.grandchild(child, first.formulation_basis(), first.solution())
    assert form.m == child.m + gen.GRANDCHILD[1] and len(cuts) == gen.GRANDCHILD[1] and len(branches) == gen.GRANDCHILD[2] + 1
    second = lps.BoundedDualReference(form, basis)
    assert gen.moved_positions(first, second) >= 1
    assert all(second.flipped[j] == 0 for j in second.basis)  # place_basis holds no basic column complemented
    assert sorted(second.basis[:child.m] + second.basis[child.m:]) == sorted(first.basis + [form.ns + i for i in range(child.m, form.m)])
    assert form.model.dual_bounded_inherit_refusal(child.model, first.formulation_basis(), basis, implicit_bounds=1) == ""
    print("first generation: %d pivots, %d basic columns held complemented; %d of %d positions moved" % (
        len(first.pivots), gen.complemented_basic(first), gen.moved_positions(first, second), child.m))


def test_the_grandchild_walk_meets_the_walk_conditions():
    child, _, first = gen.first_generation()
    form, basis, _, _ = gen.grandchild(child, first.formulation_basis(), first.solution())
    reference = lps.BoundedDualReference(form, basis)
    assert min(d for d in reference.signed_costs() if d is not None) >= 0
    reason, facts, _ = lps.walk(reference)
    lps.assert_walk_conditions(reference, gen.FIRST_M, reason, facts)
    assert reference.objective() == form.solve().objective
    print("grandchild: %s" % {k: float(v) for k, v in facts.items()})
