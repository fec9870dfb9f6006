"""``oracle/basis_state.py`` -- the exact state of a basis, the reference of tests/test_gpu_basis_state.py and tests/test_gpu_polish.py --
pinned against the oracle's own exact objects and against the numpy f64 restatement of the dense loop.  No GPU.

The last part is about the LPs with a planted basis (tests/lu_lps.py, the inputs of tests/test_gpu_lu_state.py): the state by components
against the dense one, the regions a walk must not join, the preconditions of the GPU cases, the margin of the plain f64 restatement and
the three defects it must refuse.  The reference of the full plant (2049 rows, 1787 non-unit columns in 688 components, the largest 259)
builds in 1.5 s on the machine these tests were written on -- 26 s with one fraction-free elimination per component, 3.1 s with
``Fraction`` rows --; a basis some pivots on re-uses every component no pivot touched (``basis_state._sparse_inverses``)."""
import json
import os
import time
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


# ---- the state by components, on the LPs with a planted basis (tests/lu_lps.py) ----------------------------------------------------------
def test_sparse_inverse_is_the_fraction_free_one():
    from basis_state import sparse_inverse
    import lu_lps
    rng = np.random.RandomState(5)
    blocks = [lu_lps.arrow(9, rng), lu_lps.chain(7, rng), lu_lps.bump(12, rng), lu_lps.wide(8, 3, rng)]
    for n_block, _, columns in blocks:
        matrix = np.zeros((n_block, n_block), dtype=object)
        for a, (_, entries) in enumerate(columns):
            for i, v in entries:
                if i < n_block:  # (the hub row of the chain is no row of the block)
                    matrix[i, a] = v
        numerators, det = sparse_inverse(matrix)
        want, want_det = fraction_free_inverse(matrix)
        assert abs(det) == abs(want_det) and (matrix.dot(numerators) == det * np.eye(n_block, dtype=object)).all()
        assert (numerators * want_det == want * det).all()
    with pytest.raises(ZeroDivisionError):
        sparse_inverse(np.array([[1, 2], [2, 4]], dtype=object))


@pytest.mark.parametrize("pivots", [0, 40])
def test_state_by_components_equals_the_dense_one_on_a_planted_lp(pivots):
    """m = 200, every block kind scaled down (``lu_lps.PLANTS["tiny"]``): ``row_exact``, ``den``, ``x_exact``, ``objective_exact``,
    ``reduced_cost_exact``, ``gamma_exact`` (``assert_same_state``) and ``alpha_exact``, at the planted basis and 40 pivots on."""
    import lu_lps
    import sparse_lps
    lp = lu_lps.case(200)
    basis = lp.basis if pivots == 0 else sparse_lps.basis_of(sparse_lps.walk(lp.provider, 2, pivots, basis=lp.basis))
    dense, sparse = lp.provider.state(basis, 2, cls=BasisState), lp.provider.state(basis, 2)
    assert len(sparse.components) >= 5 and max(len(c.rows) for c in sparse.components) < sparse.k / 2
    assert min(sparse.x_exact) >= 0
    n = sparse.n
    assert_same_state(dense, sparse, range(0, n, 3))
    for j in range(0, n, 41):
        assert sparse.alpha_exact(j) == dense.alpha_exact(j), j


@pytest.mark.parametrize("m, pivots", [(200, 40), (1025, 67)])
def test_a_walk_on_a_planted_lp_joins_no_two_regions(m, pivots):
    """The f64 model from the planted basis: every component of the Schur block lies in ONE region, and is no larger than the largest
    planted block plus the pivots."""
    import lu_lps
    import sparse_lps
    lp = lu_lps.case(m)
    planted = lp.provider.state(lp.basis, 2)
    walked = sparse_lps.walk(lp.provider, 2, pivots, basis=lp.basis)
    basis = sparse_lps.basis_of(walked)
    assert len(set(basis) - set(lp.basis.tolist())) > pivots // 2  # it did walk
    state = lp.provider.state(basis, 2)
    largest = max(len(c.rows) for c in planted.components)
    for c in state.components:
        regions = set(lp.region_of_row[state.rest[c.rows]].tolist()) | {int(lp.region_of_column[basis[k]]) for k in state.other[c.columns]}
        assert len(regions) == 1 and len(c.rows) <= largest + pivots, (regions, len(c.rows))
    assert close_to_model(walked, state)


def close_to_model(walked, state):
    from state_checks import close
    return close(walked.xB, long_double(*state.x_basic())) and all(close(walked.Binv[k], long_double(*state.inverse_row(k))) for k in range(0, state.m, 7))


@pytest.mark.parametrize("m, plant", [(1024, None), (1025, None), (2048, None), (2049, None), (2049, "device"),
                                      pytest.param(4397, None, marks=pytest.mark.slow), pytest.param(4397, "device", marks=pytest.mark.slow),
                                      pytest.param(8712, None, marks=pytest.mark.slow)])
def test_planted_bases_meet_the_preconditions_of_the_gpu_cases(m, plant):
    """``lu_lps.preconditions`` on the planted basis at the sizes of tests/test_gpu_lu_state.py (the plant is the same from 2048 rows on: more
    rows are more slack rows and free columns; "device": the plant of the cases with the refactorisation on the device), and the planted
    basis is primal feasible, exactly."""
    import lu_lps
    lp = lu_lps.case(m, plant=plant)
    summary = lu_lps.preconditions(lu_lps.basis_columns(lp.provider, lp.basis), lp.plant)
    print("m = %d (%s):" % (m, lp.plant), summary)
    started = time.perf_counter()
    state = lp.provider.state(lp.basis, 2)
    print("the reference: %.1f s, k = %d in %d components, the largest %d" % (
        time.perf_counter() - started, state.k, len(state.components), max(len(c.rows) for c in state.components)))
    assert min(state.x_exact) >= 1


def test_the_device_plant_keeps_its_long_inverted_rows_across_a_refactorisation():
    """Moment (d) of the cases with the refactorisation on the device, in the f64 model: 63 + 4 pivots from the planted basis of 2049 rows
    leave no row of the basis longer than the device's elimination takes, and an inverted row beyond 256 entries."""
    import lu_lps
    import sparse_lps
    lp = lu_lps.case(2049, plant="device")
    basis = sparse_lps.basis_of(sparse_lps.walk(lp.provider, 2, 67, basis=lp.basis))
    summary = lu_lps.preconditions(lu_lps.basis_columns(lp.provider, basis), lp.plant, planted=False)
    print(summary)


def test_known_limit_lu_factor_host_grows_l_on_a_cut_chain_of_entries_3_and_1():
    """A KNOWN LIMIT of ``lu_factor_host``, stated so that it stays visible -- not a property to keep.  The plant of 1025 rows with the
    chain ``(j: 3, j + 1: +-1)`` (``lu_lps.steep_chain``) in place of the planted one, 67 pivots of the f64 model on: the walked basis has
    cond_2 = 6.2e3, but the chain, cut by the pivots, is eliminated backwards from the cuts, row singleton after row singleton, each with the
    multiplier 3 -- max |L| = 3^21 = 1.05e10, and plain f64 substitution over these factors is 3e-6 from the inverse.  The row-relative
    threshold bounds a row of U against its pivot, not the multipliers of L.  The planted chain has equal entries for this reason (the
    same walk there: max |L| = 729, 4e-14).  When the factorisation bounds its multipliers the first assertion fails: turn it around."""
    import lu_lps
    import sparse_lps
    from relp_amd.basis_inverse import lu_factor_host
    m = 1025
    lp = lu_lps.case(m, plant="steep")
    basis = sparse_lps.basis_of(sparse_lps.walk(lp.provider, 2, 67, basis=lp.basis))
    columns = lu_lps.basis_columns(lp.provider, basis)
    B = np.zeros((m, m))
    for k, column in enumerate(columns):
        for i, v in column:
            B[i, k] = v
    growth = max(abs(v) for row in lu_factor_host(columns)["lower_rows"] for _, v in row)
    carry = lu_lps.HostCarry(lp.provider, basis)
    error = float(np.abs(np.stack([carry.basis_inverse_row(i) for i in range(m)]) - np.linalg.inv(B)).max())
    print("max |L| %.3g, cond_2 %.3g, substitution against numpy's inverse %.3g" % (growth, np.linalg.cond(B), error))
    assert np.linalg.cond(B) < 1e4
    assert growth > 1e9 and error > 1e-7  # (the limit as measured; a sound factorisation of this basis stays below 1e-11)


def test_kernel_path_takes_the_last_sizes_that_the_restated_lds_bytes_give():
    """``lu_lps.lds_fixed_bytes`` against the load-time plan: the last size each carry takes at its default period, and from it the size at
    which the inverse-factor form goes from four LDS vectors to three (no plan field says so: tests/test_gpu_lu_state.py computes it)."""
    import lu_lps
    import relp_amd
    from relp_amd.api import CARRY_LU, CARRY_LU_INVERSE, RelpError

    def takes(m, carry):
        model = relp_amd.Model.from_general_form([[(i, 1)] for i in range(m)], ["Less"] * m, [1] * m, [(-1, 0, None)] * m)
        try:
            plan = model.kernel_path(carry=carry)
        except RelpError:
            return None
        return plan["refactor_period"]
    assert (lu_lps.last_size(False, 32), lu_lps.last_size(True, 48), lu_lps.last_size(True, 48, vectors=4)) == (8712, 5850, 4396)
    assert takes(8712, CARRY_LU) == 31 and takes(8713, CARRY_LU) is None
    assert takes(5850, CARRY_LU_INVERSE) == 47 and takes(5851, CARRY_LU_INVERSE) is None
    assert (lu_lps.inverse_vectors(4396, 48), lu_lps.inverse_vectors(4397, 48), lu_lps.inverse_vectors(4397, 64)) == (4, 3, 3)


@pytest.fixture(scope="module")
def planted_2049():
    import lu_lps
    lp = lu_lps.case(2049)
    exact = lp.provider.state(lp.basis, 2)
    return lp, exact, lu_lps.checks_of(lp, exact)


def test_the_f64_restatement_stays_a_hundredth_of_the_tolerance_from_the_exact_state(planted_2049):
    """Forward and back substitution in f64 over the rows of ``lu_factor_host`` (``lu_lps.HostCarry``) at the planted basis of 2049 rows,
    through ``assert_state`` itself: per part at most 1 / 100 of the tolerance of an un-polished state -- two decades for the device's other
    order of summation and its up to 63 updates.  The LP's values were chosen for this; the basis has cond_2 = 6.6e3, asserted below 1e4:
    2^-53 times that is a tenth of the margin of 1e-11.
    Measured: inverse 2.8e-15, x_B 2.9e-15, objective 0, costs 2.8e-13, weights 1.8e-14, alpha 5.1e-16, btran 5.6e-16."""
    import lu_lps
    from state_checks import EVERYTHING, TOLERANCE, assert_state
    lp, exact, checks = planted_2049
    report = {}
    assert_state(lu_lps.HostCarry(lp.provider, lp.basis), exact, parts=EVERYTHING, report=report, **checks)
    print(", ".join("%s %.1e" % item for item in sorted(report.items())))
    assert set(report) == set(TOLERANCE)
    for part, error in report.items():
        assert error <= TOLERANCE[part] / 100, (part, error)
    condition = np.linalg.cond(exact.basis_matrix())
    print("cond_2 of the planted basis: %.2e" % condition)
    assert condition < 1e4


def test_the_f64_restatement_stays_within_the_same_margin_on_the_plant_of_the_device_cases():
    """The same at the planted basis of 2049 rows of ``PLANTS["device"]`` (cond_2 = 1.7e4, asserted below 2e4: 2^-53 times that is a fifth of
    the margin of 1e-11).  Measured: inverse 3.5e-15, x_B 2.5e-15, objective 0, costs 3.0e-13, weights 1.2e-14, alpha 9.7e-16, btran 4.3e-16."""
    import lu_lps
    from state_checks import EVERYTHING, TOLERANCE, assert_state
    lp = lu_lps.case(2049, plant="device")
    exact = lp.provider.state(lp.basis, 2)
    report = {}
    assert_state(lu_lps.HostCarry(lp.provider, lp.basis), exact, parts=EVERYTHING, report=report, **lu_lps.checks_of(lp, exact))
    print(", ".join("%s %.1e" % item for item in sorted(report.items())))
    assert set(report) == set(TOLERANCE)
    for part, error in report.items():
        assert error <= TOLERANCE[part] / 100, (part, error)
    assert np.linalg.cond(exact.basis_matrix()) < 2e4


@pytest.mark.parametrize("defect", range(3), ids=["extra entries", "last slot of 64", "second chunk"])
def test_the_planted_lp_refuses_a_defective_task_list(planted_2049, defect):
    """What the plant is there to catch, done to the restatement: each takes at least one checked vector out of the tolerance."""
    import lu_lps
    from state_checks import assert_state
    lp, exact, checks = planted_2049
    carry = lu_lps.HostCarry(lp.provider, lp.basis, defect=lu_lps.DEFECTS[defect])
    with pytest.raises(AssertionError, match="row of the inverse"):
        assert_state(carry, exact, parts=("inverse",), **checks)
    with pytest.raises(AssertionError, match="btran"):
        assert_state(carry, exact, parts=("btran",), **checks)
