"""The f64 state of a handle against the EXACT DATA of its basis, where the exact state itself is out of reach: at the optimum of a sparse LP
of a thousand rows most basic columns are structural, and the exact inverse of that block (``basis_state.SparseBasisState``) costs its
cube in big integers.  The equations the state has to satisfy need the model's exact small-integer columns only, and the host
evaluates them in ``longdouble`` over rows read from the device, in O(nnz(B) m):

  inverse   ``B Binv - I``, every entry, with every row of the device's inverse
  vertex    ``B x_B - b``, and the objective against ``c_B x_B``
  costs     every relative cost against ``c_j - y a_j`` with ``y = c_B' Binv`` formed on the host from the device's rows
  btran     ``v' Binv`` of the device against the same combination of its rows on the host

Bounds.  The project's tolerance for an un-polished state (tests/state_checks.py) allows a row k of the inverse an error of
``e_k[j] = 1e-9 max(1, max |row k|) + 1e-8 |Binv[k, j]|`` and x_B the same with its own scale.  An inverse within it has
``|B Binv - I|[i, j] <= sum_k |B[i, k]| e_k[j]`` and a vertex within it ``|B x_B - b|[i] <= sum_k |B[i, k]| e[k]``: those are the
bounds of the first two parts (the device's values stand in for the exact ones inside ``e``; the difference is of second order).  A
relative cost may differ from the exact one by 1e-9 (1 + |d_j|) (``rtol = atol = 1e-9`` there); the host's own value carries the error of
``y``, ``sum_r |a_rj| sum_k |c_Bk| e_k[r]``, and the bound is the sum of the two.  The objective: ``rel = 1e-9, abs = 1e-10`` as there, plus
``sum_k |c_Bk| e[k]``.  The BTRAN is ``state_checks.close`` unchanged.  A residual is a necessary condition, weaker than the comparison
with the exact state by the condition of B; it is independent of every kernel of the device.
"""
import numpy as np

from state_checks import close

LONG = np.longdouble


def entry_tolerance(values):
    """``e`` of the docstring for one vector (a row of the inverse, x_B)."""
    values = np.abs(np.asarray(values, dtype=LONG))
    return 1e-9 * max(1.0, float(values.max())) + 1e-8 * values


def basis_rows(columns, basis, m):
    """``B`` by rows: ``rows[i] = [(k, value)]`` with k the basis position, from the exact columns (small integers: exact in f64)."""
    rows = [[] for _ in range(m)]
    for k, j in enumerate(basis):
        for i, v in columns[j]:
            rows[i].append((k, float(v)))
    return rows


def assert_residuals(solver, provider, btrans, parts=("inverse", "vertex", "costs", "btran"), report=None):
    """``solver``: a handle in phase two without artificials (``basis()``, ``basis_inverse_row``, ``b``, ``objective_function_value``,
    ``relative_costs``, ``right_multiply_by_basis_inverse``); ``provider``: ``sparse_lps.Provider`` of its model."""
    m = solver.m
    assert solver.n_art == 0 and provider.m == m
    basis = [int(c) for c in solver.basis()]
    assert min(basis) >= 0 and len(set(basis)) == m
    rows_of_b = basis_rows(provider.columns, basis, m)
    inverse = np.stack([solver.basis_inverse_row(k) for k in range(m)]).astype(LONG)
    allowed = np.stack([entry_tolerance(inverse[k]) for k in range(m)])
    cost_basic = np.array([float(provider.cost[j]) for j in basis], dtype=LONG)

    def note(part, value):
        if report is not None:
            report[part] = max(report.get(part, 0.0), float(value))
    if "inverse" in parts:
        for i, entries in enumerate(rows_of_b):
            residual, bound = np.zeros(m, dtype=LONG), np.zeros(m, dtype=LONG)
            for k, v in entries:
                residual += v * inverse[k]
                bound += abs(v) * allowed[k]
            residual[i] -= 1
            note("inverse", np.abs(residual).max())
            assert (np.abs(residual) <= bound).all(), ("row of B Binv - I", i, float(np.abs(residual).max()))
    if "vertex" in parts:
        x = solver.b().astype(LONG)
        allowed_x = entry_tolerance(x)
        for i, entries in enumerate(rows_of_b):
            residual = sum((v * x[k] for k, v in entries), LONG(0)) - LONG(float(provider.b[i]))
            bound = sum((abs(v) * allowed_x[k] for k, v in entries), LONG(0))
            note("vertex", abs(residual))
            assert abs(residual) <= bound, ("B x_B - b", i, float(residual))
        want = float(cost_basic @ x)
        got = solver.objective_function_value()
        note("objective", abs(got - want) / max(1.0, abs(want)))
        assert abs(got - want) <= 1e-10 + 1e-9 * abs(want) + float(np.abs(cost_basic) @ allowed_x), ("objective", got, want)
    if "costs" in parts:
        y = cost_basic @ inverse
        y_error = np.abs(cost_basic) @ allowed
        got = solver.relative_costs()
        is_basic = np.zeros(solver.n, dtype=bool)
        is_basic[basis] = True
        for j in range(solver.n):
            want = LONG(float(provider.cost[j])) - sum((float(v) * y[i] for i, v in provider.columns[j]), LONG(0))
            bound = 1e-9 * (1 + abs(want)) + sum((abs(float(v)) * y_error[i] for i, v in provider.columns[j]), LONG(0))
            note("costs", abs(got[j] - want) / (1 + abs(want)))
            assert abs(got[j] - want) <= bound, ("relative cost", j, float(got[j]), float(want))
    if "btran" in parts:
        for rows, values in btrans:
            want = np.asarray(values, dtype=LONG) @ inverse[np.asarray(rows)]
            got = solver.right_multiply_by_basis_inverse(rows, values)
            note("btran", float(np.abs(got - want).max()) / max(1.0, float(np.abs(want).max())))
            assert close(got, want), "btran"
