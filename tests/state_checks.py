"""The comparison of a handle's f64 state with the exact state of its basis (oracle/basis_state.py), shared by
tests/test_gpu_basis_state.py (dense pipeline, ``BasisState``) and tests/test_gpu_sparse_state.py (sparse pivot paths,
``SparseBasisState``).  Tolerance of an un-polished state: ``close()`` (rtol 1e-8, atol 1e-9 x the vector's largest entry), 1e-8
relative for gamma, 1e-9 for the relative costs."""
import numpy as np
import pytest

from basis_state import long_double, newton_schulz_polish, polished_tolerance

EVERYTHING = ("inverse", "vertex", "costs", "weights", "alpha", "btran", "selection")
# The tolerance of an un-polished state per part of ``assert_state``'s ``report``, on the scale the report is in: the absolute term of
# ``close()`` (inverse, vertex, alpha, btran), relative to max(1, |objective|), to 1 + |cost|, and relative for the weights.
ABSOLUTE, RELATIVE = 1e-9, 1e-8  # close(): |error| <= ABSOLUTE max(1, max |want|) + RELATIVE |want|
TOLERANCE = {"inverse": ABSOLUTE, "vertex": ABSOLUTE, "objective": 1e-9, "costs": 1e-9, "weights": 1e-8, "alpha": ABSOLUTE, "btran": ABSOLUTE}


def close(got, want):
    """``close()`` of tests/test_gpu_parity.py against a ``longdouble`` vector."""
    want = np.asarray(want, dtype=np.longdouble)
    scale = max(1.0, float(np.abs(want).max()))
    error = np.abs(np.asarray(got, dtype=np.longdouble) - want)
    return bool((error <= ABSOLUTE * scale + RELATIVE * np.abs(want)).all())


def deviation(got, want):
    """Largest error of ``got`` over ``max(1, max |want|)``, the scale of ``close()``'s absolute term."""
    want = np.asarray(want, dtype=np.longdouble)
    return float(np.abs(np.asarray(got, dtype=np.longdouble) - want).max()) / max(1.0, float(np.abs(want).max()))


def device_inverse(solver):
    return np.stack([solver.basis_inverse_row(i) for i in range(solver.m)])


def _note(report, part, value):
    if report is not None:
        report[part] = max(report.get(part, 0.0), float(value))


def assert_state(solver, exact, parts=EVERYTHING, inverse=None, inverse_rows=None, alpha_columns=None, btrans=None, report=None):
    """``exact``: the ``BasisState`` of ``solver.basis()``.  ``inverse``: what ``device_inverse`` has just read, if the caller holds it.
    ``inverse_rows``: the rows of the inverse to compare, each read from the device on its own (default: all of them, stacked);
    ``alpha_columns``: the columns whose FTRAN is compared (default: the dense LP's choice); ``btrans``: ``[(rows, values)]`` (default:
    one with three entries).  ``report``: a dict that receives the device's largest error per part."""
    m, n = solver.m, solver.n
    assert (n, solver.n_art) == (exact.n, exact.n_art)
    n_dense = getattr(exact.columns, "n", 0)  # (the columns of the dense block come first; a sparse LP has none)
    free = np.flatnonzero(~exact.is_basic)
    free = free[free >= exact.n_art]
    checked = exact.columns_to_check(n_grouped=n_dense)  # every column, unless longdouble is f64 here: then the sample of the exact path
    checked_free = np.intersect1d(checked, free)
    selected = solver.select_primal_pivot_column()  # (applies the pending weight update, as the next pricing pass would)
    want_cost = exact.reduced_costs(checked)
    if "inverse" in parts:
        if inverse is None and inverse_rows is None:
            inverse = device_inverse(solver)
        for i in (range(m) if inverse_rows is None else inverse_rows):
            got = solver.basis_inverse_row(int(i)) if inverse is None else inverse[i]
            want = long_double(*exact.inverse_row(int(i)))
            _note(report, "inverse", deviation(got, want))
            assert close(got, want), ("row of the inverse", int(i), float(np.abs(got - want).max()))
    if "vertex" in parts:
        _note(report, "vertex", deviation(solver.b(), long_double(*exact.x_basic())))
        assert close(solver.b(), long_double(*exact.x_basic())), "b"
        _note(report, "objective", abs(solver.objective_function_value() - float(exact.objective_exact)) / max(1.0, abs(float(exact.objective_exact))))
        assert solver.objective_function_value() == pytest.approx(float(exact.objective_exact), rel=TOLERANCE["objective"], abs=1e-10)
    if "costs" in parts:
        got = solver.relative_costs()[checked]
        _note(report, "costs", (np.abs(got - np.asarray(want_cost, dtype=np.float64)) / (1 + np.abs(np.asarray(want_cost, dtype=np.float64)))).max())
        assert np.allclose(got, np.asarray(want_cost, dtype=np.float64), rtol=TOLERANCE["costs"], atol=TOLERANCE["costs"]), \
            ("relative cost", int(checked[np.argmax(np.abs(got - np.asarray(want_cost, dtype=np.float64)))]))
    want_gamma = exact.gammas(checked_free)
    if "weights" in parts:
        got = solver.gamma()
        assert np.isnan(got[exact.is_basic]).all()
        relative = np.abs(np.asarray(got[checked_free], dtype=np.longdouble) / want_gamma - 1)
        _note(report, "weights", relative.max())
        assert relative.max() <= TOLERANCE["weights"], ("gamma", int(checked_free[np.argmax(relative)]), float(relative.max()))
    if "alpha" in parts:
        if alpha_columns is None:
            slack = next((int(j) for j in free if j >= n_dense), n_dense)
            dense_free = free[free < n_dense]
            alpha_columns = sorted({int(free[0]), int(dense_free[len(dense_free) // 3]), n_dense - 1, slack})
        for q in alpha_columns:
            _, alpha = solver.select_primal_pivot_row(q)  # the multi-block FTRAN where the pipeline is in force
            want = exact.alpha(q)
            _note(report, "alpha", deviation(alpha, want))
            assert close(alpha, want), ("alpha", q)
    if "btran" in parts:
        if btrans is None:
            btrans = [(np.array([1, m // 2, m - 1], dtype=np.int32), np.array([3.0, 5.0, 7.0]))]
        for rows, values in btrans:
            got, want = solver.right_multiply_by_basis_inverse(rows, values), exact.right_multiply(rows, values)
            _note(report, "btran", deviation(got, want))
            assert close(got, want), "btran"
    if "selection" in parts:
        position = {int(j): at for at, j in enumerate(checked)}
        cost_free = np.array([want_cost[position[int(j)]] for j in checked_free], dtype=np.longdouble)
        key = np.where(cost_free < 0, cost_free * cost_free / want_gamma, 0)
        if selected is None:
            # the device's costs are within 1e-9 of the exact ones (asserted above) and tol_dual is 1e-9: nothing is 3e-9 below zero
            assert float(cost_free.min()) >= -3e-9
        else:
            q, cost_q = selected
            exact_q = exact.reduced_cost_exact(q)
            assert cost_q == pytest.approx(float(exact_q), rel=1e-9, abs=1e-12)
            key_q = float(exact_q * exact_q / exact.gamma_exact(q))
            if len(checked) == n:
                assert key_q == pytest.approx(float(key.max()), rel=1e-9)  # same maximum (ties may pick another column)
            else:
                assert key_q >= float(key.max()) * (1 - 1e-9)  # (a sample: the choice is at least as good as every column in it)


def assert_polished(solver, exact, inverse_before, rhs, parts=EVERYTHING, **state_options):
    """After ``refactor()``: the resident inverse and b within the post-polish tolerance of the exact state -- 16 x the error of the numpy
    f64 restatement of the same Newton-Schulz steps from ``inverse_before``, floor 8 ulps (``basis_state.polished_tolerance``).  ``rhs``:
    the right-hand side in f64.  ``state_options`` go on to ``assert_state``."""
    B = exact.basis_matrix()
    reference = newton_schulz_polish(B, inverse_before)
    got = device_inverse(solver)
    exact_inverse = np.stack([long_double(*exact.inverse_row(i)) for i in range(solver.m)])
    bound, error = polished_tolerance(reference, exact_inverse)
    device_error = float(np.abs(got - exact_inverse).max())
    print("polish: device error %.3e, restatement %.3e, bound %.3e" % (device_error, error, bound))
    assert device_error <= bound, ("polished inverse", device_error, error, bound)
    bound, error = polished_tolerance(reference @ rhs, long_double(*exact.x_basic()))
    device_error = float(np.abs(solver.b() - long_double(*exact.x_basic())).max())
    print("polish: b: device error %.3e, restatement %.3e, bound %.3e" % (device_error, error, bound))
    assert device_error <= bound, ("polished b", device_error, error, bound)
    assert_state(solver, exact, parts=parts, inverse=got, **state_options)  # ... and everything else still at the tolerance of the unpolished state
