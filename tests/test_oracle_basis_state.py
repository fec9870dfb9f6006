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


# ---- the structured form for sparse LPs of thousands of rows: the same numbers as the dense class ---------------------------------
def assert_same_state(dense, sparse, columns):
    """``SparseBasisState`` against ``BasisState`` of the same basis: exactly equal where both are exact; where both sum ``longdouble`` products of ``hi + lo``
    in their own order, within 2^-56 of the largest entry (up to 40 products of a column entry <= 3 with an entry rounded to a 64-bit
    significand, 40 * 3 * 2^-64 < 2^-57 each way, and the exact value may cancel to zero)."""
    m = dense.m
    assert sparse.den == dense.den
    for k in range(m):
        where, numerators = sparse.row_exact(k)
        filled = np.flatnonzero(dense.num[k] != 0)
        assert where.tolist() == filled.tolist() and [int(v) for v in numerators] == [int(v) for v in dense.num[k, filled]], k
        assert np.array_equal(sparse.inverse_row(k)[0], dense.inverse_row(k)[0]) and np.array_equal(sparse.inverse_row(k)[1], dense.inverse_row(k)[1])
    assert sparse.x_exact == dense.x_exact and sparse.objective_exact == dense.objective_exact
    assert np.array_equal(sparse.x_hi, dense.x_hi) and np.array_equal(sparse.x_lo, dense.x_lo)
    assert np.array_equal(sparse.pi_hi, dense.pi_hi) and np.array_equal(sparse.pi_lo, dense.pi_lo)
    for j in columns:
        assert sparse.reduced_cost_exact(j) == dense.reduced_cost_exact(j), j
        assert sparse.gamma_exact(j) == dense.gamma_exact(j), j
        assert sparse.alpha_nnz(j) == sum(1 for v in dense.alpha_exact(j) if v != 0), j
    if not (sparse.extended and dense.extended):
        return

    def same(got, want):
        return float(np.abs(got - want).max()) <= 2.0 ** -56 * max(1.0, float(np.abs(want).max()))
    columns = np.asarray(columns)
    assert same(sparse.gammas(columns), dense.gammas(columns))
    assert same(sparse.reduced_costs(columns), dense.reduced_costs(columns))
    for j in columns[:12]:
        assert same(sparse.alpha(int(j)), dense.alpha(int(j))), j
    every_row = np.arange(m)
    assert same(sparse.right_multiply(every_row, 1 + every_row % 7), dense.right_multiply(every_row, 1 + every_row % 7))


def test_structured_state_equals_the_dense_one_on_afiro(afiro):
    from basis_state import SparseBasisState
    data, columns = afiro
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "AFIRO.json")))
    arguments = (columns, data.right_hand_side(), [data.cost_value(j) for j in range(len(columns))], golden["basis"])
    assert_same_state(BasisState(*arguments), SparseBasisState(*arguments), range(len(columns)))


@pytest.mark.parametrize("family, mix, m, pivots", [("equality", "mixed", 65, 40), ("equality", "short", 65, 40), ("less", "mixed", 65, 40),
                                                    ("equality", "mixed", 513, 100), ("less", "mixed", 513, 100)])
def test_structured_state_equals_the_dense_one_on_walked_bases(family, mix, m, pivots):
    """Bases reached by the f64 model of the device's loop on the two LP families of tests/sparse_lps.py.  The equality family is still
    in phase one after the walk, so artificials are basic.  Every basis is compared under the phase-one AND the phase-two costs: with
    artificials basic the phase-two cost vector is offset by n_art and c_B mixes zeros with real costs."""
    import sparse_lps
    _, provider, phase = sparse_lps.case(family, mix, m)
    walked = sparse_lps.walk(provider, phase, pivots)
    basis = sparse_lps.basis_of(walked)
    assert (min(basis) < 0) == (family == "equality")  # artificials are present in the equality family's basis
    n = walked.n
    columns = range(n) if m == 65 else sorted(set(range(0, n, 29)) | set(range(n - 8, n)))  # (every length of the mix: 29 is prime to 5 and 8)
    for costs in (1, 2):
        dense = provider.state(basis, costs, cls=BasisState)
        sparse = provider.state(basis, costs)
        assert sparse.k <= pivots and sparse.n_art == walked.n_art
        assert_same_state(dense, sparse, columns)
        if costs == phase:
            assert float(sparse.objective_exact) == pytest.approx(walked.objective(), rel=1e-9)
    # the fallback where longdouble is f64: exact integers on the sample, the same numbers
    dense = provider.state(basis, phase, cls=BasisState)
    sample = provider.state(basis, phase, extended=False)
    checked = sample.columns_to_check(minimum=24)[:40]
    assert np.allclose(np.asarray(sample.gammas(checked), dtype=np.float64), [float(dense.gamma_exact(int(j))) for j in checked], rtol=4e-16, atol=0)
    assert np.allclose(np.asarray(sample.reduced_costs(checked), dtype=np.float64), [float(dense.reduced_cost_exact(int(j))) for j in checked],
                       rtol=4e-16, atol=1e-18)
    assert np.allclose(np.asarray(sample.alpha(int(checked[-1])), dtype=np.float64), [float(v) for v in dense.alpha_exact(int(checked[-1]))],
                       rtol=4e-16, atol=1e-18)


@pytest.mark.slow
def test_structured_state_at_8193_rows_and_the_f64_model():
    """100 pivots of the mixed family at m = 8193, walked by ``f64_model.Model`` without a polish (about half a minute in numpy, most of
    it the model's own dense (m, m) inverse and its first (m, n) product).  The state builds in seconds from k x k integers, and the
    model's inverse and x_B are within ``close()`` of it (measured: 1e-14)."""
    import time
    import tracemalloc
    import sparse_lps
    from state_checks import close
    _, provider, phase = sparse_lps.case("equality", "mixed", 8193)
    walked = sparse_lps.walk(provider, phase, 100)
    basis = sparse_lps.basis_of(walked)

    def build():
        state = provider.state(basis, phase)
        free = np.flatnonzero(~state.is_basic)
        free = free[free >= state.n_art]
        return state, free, state.gammas(free), state.reduced_costs(np.arange(state.n))
    started = time.perf_counter()
    state, free, gammas, costs = build()
    seconds = time.perf_counter() - started
    tracemalloc.start()  # (numpy's buffers are traced too; tracing slows the build, so it is timed above without)
    build()
    grown = tracemalloc.get_traced_memory()[1] / 2.0 ** 20
    tracemalloc.stop()
    print("state, every weight and every relative cost at m = 8193: %.1f s, k = %d, %.0f MB at the peak" % (seconds, state.k, grown))
    # measured 1.3 s and 22 MB; one (m, k) array of Python integers or one (m, m) array of f64 would be 100 MB and more
    assert seconds < 5 and grown < 100 and state.k <= 100
    assert not hasattr(state, "num") and not hasattr(state, "inverse_hi")  # no (m, m) array
    for k in state.rows_that_may_not_be_unit().tolist() + list(range(0, 8193, 64)) + [8192]:
        assert close(walked.Binv[k], long_double(*state.inverse_row(k))), k
    assert close(walked.xB, long_double(*state.x_basic()))
    assert np.abs(walked.gamma[free] / np.asarray(gammas, dtype=np.float64) - 1).max() <= 1e-8
    assert np.allclose(walked.cost + walked.AT @ walked.minus_pi, np.asarray(costs, dtype=np.float64), rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("family, mix, m", [pytest.param(*key, marks=pytest.mark.slow) if key[2] > 2049 else key for key in sorted(__import__("sparse_lps").SEEDS)])
def test_replaced_seeds_meet_the_preconditions_of_the_gpu_cases(family, mix, m):
    """Every LP whose seed is not 1000 + m (``sparse_lps.SEEDS``), walked 100 pivots by the f64 model under the reference's ratio rule --
    the one the device takes on these LPs up to 8192 rows -- meets what tests/test_gpu_sparse_state.py asserts before it compares."""
    import sparse_lps
    _, provider, phase = sparse_lps.case(family, mix, m)
    walked = sparse_lps.walk(provider, phase, sparse_lps.PIVOTS, textbook=True)
    state = provider.state(sparse_lps.basis_of(walked), phase)
    not_unit, columns, nnz, entered = sparse_lps.preconditions(state, provider, mix)
    print("%s %s %d: %d entered columns in the basis, k = %d, nnz(alpha) of the checked columns %r" % (family, mix, m, entered, state.k, nnz))
    assert m - 1 in not_unit and len(columns) >= 3
