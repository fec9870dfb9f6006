"""``oracle/basis_state.py`` -- the exact state of a basis, the reference of tests/test_gpu_basis_state.py and tests/test_gpu_polish.py --
pinned against the oracle's own exact objects and against the numpy f64 restatement of the dense loop.  No GPU."""
import json
import os
from fractions import Fraction

import numpy as np
import pytest

from basis_state import (BasisState, DenseLE, fraction_free_inverse, long_double, newton_schulz_inverse, newton_schulz_polish, split)
from f64_dense import DenseModel
from relp_oracle import LUDecomposition, SteepestDescentAlongObjective, Tableau
from relp_oracle.inverse_rows import BasisInverseRows
from relp_oracle.mps import load_problem
from relp_amd.workloads import dense_lp  # (an input generator: it needs neither the library nor a GPU)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def afiro():
    _, data = load_problem(os.path.join(ROOT, "data", "netlib", "AFIRO.SIF"))
    return data, [data.column(j) for j in range(data.nr_columns())]


def test_split_keeps_what_f64_drops():
    for num, den in [(1, 3), (-406659, 875), (10 ** 40 + 1, 7 ** 30), (5, 1), (0, 9)]:
        hi, lo = split(num, den)
        assert hi == num / den
        assert abs(Fraction(num, den) - Fraction(hi) - Fraction(lo)) <= abs(Fraction(num, den)) * Fraction(1, 2 ** 104)


def test_fraction_free_inverse_needs_a_row_exchange():
    matrix = np.array([[0, 2, 1], [3, 0, -1], [1, 1, 0]], dtype=object)
    numerators, det = fraction_free_inverse(matrix)
    assert (matrix.dot(numerators) == det * np.eye(3, dtype=object)).all() and abs(det) == 1
    with pytest.raises(ZeroDivisionError):
        fraction_free_inverse(np.array([[1, 2], [2, 4]], dtype=object))


def test_inverse_equals_basis_inverse_rows_on_afiro(afiro):
    data, columns = afiro
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "AFIRO.json")))
    state = BasisState(columns, data.right_hand_side(), [data.cost_value(j) for j in range(len(columns))], golden["basis"])
    rows = BasisInverseRows.invert(data.column(j) for j in golden["basis"]).rows
    m = state.m
    for k in range(m):
        assert [(i, state.inverse_exact(k, i)) for i in range(m) if state.num[k, i] != 0] == rows[k]
    num, den = golden["objective"].split("/")
    # (the fixture's objective is that of the file: it carries the fixed cost of the shifted variables, AFIRO has none)
    assert state.objective_exact == Fraction(int(num), int(den))
    hi, lo = state.inverse_row(3)
    assert all(Fraction(hi[i]) + Fraction(lo[i]) - state.inverse_exact(3, i) == 0 or
               abs(Fraction(hi[i]) + Fraction(lo[i]) - state.inverse_exact(3, i)) < Fraction(1, 2 ** 100) for i in range(m))


@pytest.mark.parametrize("extended", [None, False], ids=["longdouble", "exact-sample"])
def test_weights_and_vertex_after_the_afiro_steps_of_the_parity_test(afiro, extended):
    """The 19 steps of test_trait_ops_follow_the_oracle on AFIRO, made by the Fraction rule: its gamma, b, relative costs and
    objective are those of the basis it ends on."""
    data, columns = afiro
    tableau = Tableau.new_partially_artificial(data, LUDecomposition)
    rule = SteepestDescentAlongObjective(tableau)
    for _ in range(19):
        selected = rule.select_primal_pivot_column(tableau)
        if selected is None:
            break
        q, cost = selected
        info = tableau.generate_column(q)
        p = tableau.select_primal_pivot_row(info.column)
        rule.after_basis_update(tableau.bring_into_basis(q, p, info, cost), tableau)
    n_art = tableau.nr_artificial_variables()
    carry = tableau.inverse_maintainer
    basis = [c - n_art if c >= n_art else -1 - c for c in carry.basis_indices]
    state = BasisState(columns, data.right_hand_side(), [data.cost_value(j) for j in range(len(columns))], basis,
                       artificial_rows=tableau.kind.column_to_row, phase=1, extended=extended)
    assert state.n == tableau.nr_columns()
    assert state.x_exact == carry.b
    assert state.objective_exact == tableau.objective_function_value()
    free = [j for j in range(n_art, state.n) if not tableau.is_in_basis(j)]
    assert free and all(not state.is_basic[j] for j in free)
    for j in free:
        assert state.gamma_exact(j) == rule.gamma[j], j
        assert state.reduced_cost_exact(j) == tableau.relative_cost(j), j
    # the array forms the GPU tests read: correct to the last bits of f64
    columns_checked = state.columns_to_check(n_grouped=0, minimum=8) if extended is False else np.array(free)
    gammas = state.gammas(columns_checked)
    costs = state.reduced_costs(columns_checked)
    for at, j in enumerate(columns_checked):
        assert float(gammas[at]) == pytest.approx(float(state.gamma_exact(int(j))), rel=4e-16)
        assert float(costs[at]) == pytest.approx(float(state.reduced_cost_exact(int(j))), rel=4e-16, abs=1e-18)
    alpha = state.alpha(free[-1])
    assert np.allclose(np.asarray(alpha, dtype=np.float64), [float(v) for v in state.alpha_exact(free[-1])], rtol=4e-16, atol=1e-18)
    want = carry.basis_inverse.right_multiply_by_basis_inverse([(1, Fraction(2)), (5, Fraction(7))])
    got = state.right_multiply([1, 5], [2, 7])
    assert np.allclose(np.asarray(got, dtype=np.float64), [float(dict(want).get(i, 0)) for i in range(state.m)], rtol=4e-16, atol=0)


@pytest.mark.parametrize("pivots", [20, None], ids=["20 pivots, no polish", "optimum"])
def test_dense_model_state_is_the_state_of_its_basis(pivots):
    """The numpy restatement of the dense loop on the 64 x 128 twin.  Bound: f64 rounding of at most 24 rank-one updates of a
    64-row inverse whose bases have cond < 1e3 -- 2^-53 * 64 * 24 * 1e3 = 1.7e-10 relative to the largest entry (measured: 4e-16
    for the inverse, 1.3e-14 for x_B, 4.9e-14 for gamma)."""
    a, b, c = dense_lp(64, 128)
    model = DenseModel(a, b, c)
    assert model.solve(max_pivots=pivots) == ("limit" if pivots else "optimal")
    model.price()  # applies the weight update of the last pivot
    state = BasisState(DenseLE(a), b, c, model.basis)
    assert np.abs(model.Binv - state.inverse_hi).max() <= 1.7e-10 * np.abs(state.inverse_hi).max()
    assert np.abs(model.xB - state.x_hi).max() <= 1.7e-10 * np.abs(state.x_hi).max()
    assert model.objective() == pytest.approx(float(state.objective_exact), rel=1.7e-10)
    free = np.flatnonzero(~state.is_basic)
    assert np.allclose(model.gamma[free], np.asarray(state.gammas(free), dtype=np.float64), rtol=1.7e-10, atol=0)
    pi = np.asarray(long_double(state.pi_hi, state.pi_lo), dtype=np.float64)
    assert np.abs(model.minus_pi + pi).max() <= 1.7e-10 * np.abs(pi).max()
    # the longdouble products and the exact integer ones are the same numbers
    sample = BasisState(DenseLE(a), b, c, model.basis, extended=False)
    columns = sample.columns_to_check(n_grouped=128, minimum=40)
    assert {0, 15, 16, 111, 112, 127}.issubset(set(columns.tolist())) and len(columns) >= 40
    assert np.allclose(np.asarray(sample.gammas(columns[:24]), dtype=np.float64),
                       np.asarray(state.gammas(columns[:24]), dtype=np.float64), rtol=1e-15, atol=0)
    assert np.allclose(np.asarray(sample.reduced_costs(columns[:24]), dtype=np.float64),
                       np.asarray(state.reduced_costs(columns[:24]), dtype=np.float64), rtol=1e-13, atol=1e-13)


def test_sample_for_the_exact_path_keeps_group_edges_and_the_last_group():
    a, b, c = dense_lp(16, 70)
    state = BasisState(DenseLE(a), b, c, np.arange(70, 86), extended=False)
    columns = set(state.columns_to_check(n_grouped=70, minimum=60).tolist())
    assert {0, 15, 16, 31, 32, 47, 48, 63, 64, 65, 66, 67, 68, 69}.issubset(columns)
    assert set(range(70, 86)).issubset(columns) and len(columns) >= 60
    everything = BasisState(DenseLE(a), b, c, np.arange(70, 86), extended=True)
    assert len(everything.columns_to_check(n_grouped=70)) == 86
    assert np.array_equal(np.asarray(everything.gammas(np.arange(70)), dtype=np.float64), 1.0 + (a.astype(np.float64) ** 2).sum(axis=1))


def test_newton_schulz_restatements_reach_the_exact_inverse():
    a, b, c = dense_lp(64, 128)
    model = DenseModel(a, b, c)
    model.solve(max_pivots=20)
    state = BasisState(DenseLE(a), b, c, model.basis)
    B = state.basis_matrix()
    scale = np.abs(state.inverse_hi).max()
    assert np.abs(newton_schulz_inverse(B) - state.inverse_hi).max() <= 1e-11 * scale
    drifted = state.inverse_hi * (1 + 1e-7 * np.cos(np.arange(64 * 64)).reshape(64, 64))
    assert np.abs(drifted - state.inverse_hi).max() > 1e-9 * scale
    assert np.abs(newton_schulz_polish(B, drifted) - state.inverse_hi).max() <= 1e-11 * scale
