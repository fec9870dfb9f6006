"""The host side of the dual simplex's start from a parent's inverse (no GPU): the three new symbols of the C ABI, and
``Model.dual_inherit_refusal`` -- the pure function ``dual_inherit_refusal`` of relp_amd/csrc/dual_inherit.cpp behind
``relp_debug_dual_inherit_refusal`` -- over the pairs it takes and every pair it refuses, with the place named.

The pairs are ``dual_lps.cut_case(5, ...)`` and ``cut_case(64, ...)`` with cuts over a vertex of ones (the relation does not need an
optimal basis, so nothing is solved here) and the parent's slack basis extended by ``dual_lps.extended_basis``; where a case needs a
structural column in the basis, position 0 holds structural column 0 in both.  The same function is run stand-alone under
``-fsanitize=address,undefined`` (tests/support/dual_inherit_check.cpp), the way tests/test_bigint.py runs its driver.
"""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import relp_amd
from relp_amd.api import CARRY_LU, ERR_ARGUMENT, Result
import dual_lps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("relp_begin_dual_from", "relp_solve_dual_from", "relp_debug_dual_inherit_refusal")


def test_the_symbols_exist():
    lib = relp_amd.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in relp_amd.SYMBOLS
    for name in ("begin_dual_from", "solve_dual_from"):
        assert callable(getattr(relp_amd.Solver, name))
    assert callable(relp_amd.Model.dual_inherit_refusal)


def test_null_arguments_are_refused():
    lib = relp_amd.lib()
    basis = np.zeros(4, dtype=np.int32)
    pointer = basis.ctypes.data_as(C.POINTER(C.c_int32))
    result = Result()
    assert lib.relp_begin_dual_from(None, None, pointer) == ERR_ARGUMENT
    assert lib.relp_solve_dual_from(None, None, pointer, C.byref(result)) == ERR_ARGUMENT
    assert lib.relp_debug_dual_inherit_refusal(None, None, None, None, None, None, 0, None) == ERR_ARGUMENT
    model = dual_lps.cut_case(5, dual_lps.MIXED, 2005, 0).parent
    assert lib.relp_debug_dual_inherit_refusal(model._h, model._h, None, pointer, None, None, 0, None) == ERR_ARGUMENT
    assert lib.relp_debug_dual_inherit_refusal(model._h, None, pointer, pointer, None, None, 0, None) == ERR_ARGUMENT


class Pair:
    """A parent, its child with cuts over the vertex of ones, and a basis of each: the slack basis, structural column 0 at position 0."""

    def __init__(self, m):
        seed, n_cuts = dual_lps.WALK_CASES.get(m, (2000 + m, 3))
        self.case = case = dual_lps.cut_case(m, dual_lps.MIXED, seed, n_cuts)
        self.m, self.n_cuts = m, n_cuts
        vertex = {j: Fraction(1) for j in range(case.n_structural)}
        self.parent_basis = [column for _, column in sorted(case.parent.pivot_element_indices())]
        self.parent_basis[0] = 0
        self.child, self.basis, _ = case.child(self.parent_basis, vertex)
        assert self.child.nr_rows == m + n_cuts and len(self.basis) == m + n_cuts and self.basis[0] == 0
        # the child's structural columns (cut rows included), for the variants below
        self.child_columns = [[(i, Fraction(num, den)) for i, num, den in self.child.column_exact(j)] for j in range(case.n_structural)]
        self.child_b = self.child.right_hand_side_exact()

    def variant(self, columns=None, b=None):
        columns = self.child_columns if columns is None else columns
        b = self.child_b if b is None else b
        return relp_amd.Model.from_general_form(columns, ["Less"] * len(b), b, [(c, 0, None) for c in self.case.cost])

    def refusal(self, child=None, basis=None, parent_basis=None, **options):
        child = self.child if child is None else child
        return child.dual_inherit_refusal(self.case.parent, self.parent_basis if parent_basis is None else parent_basis,
                                          self.basis if basis is None else basis, **options)


@pytest.fixture(scope="module", params=[5, 64])
def pair(request):
    return Pair(request.param)


def test_the_cut_child_is_taken(pair):
    assert pair.refusal() == ""
    slack_basis = [column for _, column in sorted(pair.case.parent.pivot_element_indices())]
    assert pair.refusal(basis=dual_lps.extended_basis(pair.case, pair.child, slack_basis), parent_basis=slack_basis) == ""


def test_a_child_that_differs_in_its_right_hand_side_only_is_taken(pair):
    same_rows = relp_amd.Model.from_general_form(pair.case.columns, ["Less"] * pair.m, [v + 1 for v in pair.case.b], [(c, 0, None) for c in pair.case.cost])
    assert same_rows.nr_rows == pair.m
    assert same_rows.dual_inherit_refusal(pair.case.parent, pair.parent_basis, pair.parent_basis) == ""
    # ... and costs may differ too
    other_costs = relp_amd.Model.from_general_form(pair.case.columns, ["Less"] * pair.m, pair.case.b, [(c + 1, 0, None) for c in pair.case.cost])
    assert other_costs.dual_inherit_refusal(pair.case.parent, pair.parent_basis, pair.parent_basis) == ""


def test_a_child_with_fewer_rows_is_refused(pair):
    text = pair.case.parent.dual_inherit_refusal(pair.child, pair.basis, pair.parent_basis)
    assert "fewer than its parent's %d" % (pair.m + pair.n_cuts) in text, text


def test_a_changed_coefficient_of_a_basic_column_is_refused_with_its_place(pair):
    columns = [list(column) for column in pair.child_columns]
    row, value = next((i, v) for i, v in columns[0] if i < pair.m)  # an old row of the column at position 0
    columns[0] = [(i, v + 5 if i == row else v) for i, v in columns[0]]  # (entries are +-1 .. 3: never zero)
    text = pair.refusal(child=pair.variant(columns=columns))
    assert "position 0" in text and "row %d" % row in text and "%d/1 in the child, %d/1 in the parent" % (value + 5, value) in text, text
    # the same change in a column that is not basic does not matter
    other = next(j for j in range(1, pair.case.n_structural) if j not in pair.basis)
    columns = [list(column) for column in pair.child_columns]
    columns[other] = [(i, v + 5) for i, v in columns[other]]
    assert pair.refusal(child=pair.variant(columns=columns)) == ""


def test_swapped_positions_are_refused(pair):
    basis = list(pair.basis)
    basis[0], basis[1] = basis[1], basis[0]
    text = pair.refusal(basis=basis)
    assert "position 0" in text and "column %d of the child" % basis[0] in text, text


def test_a_structural_column_on_a_new_row_is_refused(pair):
    structural = next(j for j in range(1, pair.case.n_structural) if len(pair.child_columns[j]) > 1)
    basis = list(pair.basis)
    basis[pair.m + 1] = structural
    text = pair.refusal(basis=basis)
    assert "row %d" % (pair.m + 1) in text and "column %d" % structural in text and "not the slack" in text, text
    basis = list(pair.basis)
    basis[pair.m], basis[pair.m + 1] = basis[pair.m + 1], basis[pair.m]  # the slack of another new row is no better
    text = pair.refusal(basis=basis)
    assert "row %d" % pair.m in text and "not the slack" in text, text


def test_an_artificial_in_either_basis_is_refused(pair):
    text = pair.refusal(parent_basis=[-1] + pair.parent_basis[1:])
    assert "parent's basis holds an artificial" in text and "row 0" in text, text
    text = pair.refusal(basis=pair.basis[:-1] + [-2])
    assert "child's basis holds an artificial" in text and "row %d" % (pair.m + pair.n_cuts - 1) in text, text


def test_a_plan_the_dual_kernels_do_not_take_is_refused(pair):
    text = pair.refusal(carry=CARRY_LU)
    assert "LU" in text and "plan" in text, text
    assert pair.child.dual_refusal(carry=CARRY_LU) in text


def test_a_basis_of_the_wrong_length_is_not_passed_on(pair):
    with pytest.raises(ValueError):
        pair.refusal(basis=pair.basis[:-1])


def test_the_relation_stand_alone_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "dual_inherit_check")
    csrc = os.path.join(ROOT, "relp_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                           os.path.join(ROOT, "tests", "support", "dual_inherit_check.cpp"), os.path.join(csrc, "dual_inherit.cpp"), "-o", exe])
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0 and done.stdout.strip() == "ok", (done.returncode, done.stdout, done.stderr)
