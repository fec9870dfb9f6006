"""Newton-Schulz on the device -- ``Solver::invert_from_scratch`` behind ``set_basis`` and ``Solver::polish`` behind ``refactor()`` -- against the
EXACT inverse of the basis (oracle/basis_state.py), on a real MI355X (``-m gpu``).  Covers residual_kernel, scaled_basis_kernel and the
polish GEMM as gemm_mfma_kernel<0> (default) and as the plain-FMA gemm_polish_kernel<0> (``switches=SW_GEMM_VECTOR``), at row counts ragged
against the 64 x 64 tile, the K step of 16 and the 4-wide loads.

Tolerance (``basis_state.polished_tolerance``): the numpy f64 restatement of the same iteration at the same basis is compared with the
same exact inverse; the device gets 16 x that error, floor 8 * 2^-53 * max|B^-1| -- computed here from the reference, never from the
device's own residual.  b() = B^-1 b likewise, against the restatement's X b.

Measured on an MI355X, device error / restatement error (the same figures with the matrix-core and the plain-FMA GEMM):

    LP       from scratch: inverse   b      after refactor(): inverse   b
    AFIRO                  0.36      0.74                     1.00      1.00
    SC50A                  1.27      2.51                     1.00      0.57
    SC105                  0.77      0.80                     1.00      1.00
    SCAGR7                 0.63      0.91                     1.00      1.27
    SC205                  0.80      1.42                     1.00      1.00
    E226                   0.98      0.52                     1.00      1.37
    SC105, LU carry        1.76      0.90                     1.80      1.52
    SC105, LU inverse      1.65      0.97                     1.68      1.24

Nothing is near the factor of 16.  The ratio 1.00 after ``refactor()`` is no accident: about fifteen product-form updates from an
inverse that was exact leave a residual below the 1e-12 under which ``Solver::polish`` -- and its restatement -- take no step.
"""
import json
import os

import numpy as np
import pytest

import relp_amd
from relp_amd.api import CARRY_EXPLICIT, CARRY_LU, CARRY_LU_INVERSE, SW_GEMM_VECTOR
from relp_oracle.mps import load_problem
from basis_state import BasisState, long_double, newton_schulz_inverse, newton_schulz_polish, polished_tolerance

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
#        LP        m    cond of the golden basis
CASES = [("AFIRO", 27, 1.3e1), ("SC50A", 50, 5.1e1), ("SC105", 105, 1.6e2), ("SCAGR7", 129, 4.4e3), ("SC205", 205, 8.0e2), ("E226", 223, 3.0e6)]

_problems = {}


def problem(name):
    """(path, golden basis, provider columns, b, costs), read once per LP."""
    if name not in _problems:
        golden = json.load(open(os.path.join(ROOT, "tests", "golden", name + ".json")))
        path = os.path.join(ROOT, golden["file"])
        _, data = load_problem(path)
        columns = [data.column(j) for j in range(data.nr_columns())]
        _problems[name] = (path, golden["basis"], columns, data.right_hand_side(), [data.cost_value(j) for j in range(len(columns))])
    return _problems[name]


_states = {}


def exact_state(name, solver):
    """The exact state of the handle's basis (cached: both GEMM forms visit the same bases)."""
    basis = solver.basis()
    key = (name, tuple(basis.tolist()))
    if key not in _states:
        _, _, columns, b, cost = problem(name)
        artificial_rows = []  # (artificial k of these LPs never stays basic; a basis that held one would need its row here)
        assert (basis >= 0).all()
        _states[key] = BasisState(columns, b, cost, basis, artificial_rows=artificial_rows)
    return _states[key]


def device_inverse(solver):
    return np.stack([solver.basis_inverse_row(i) for i in range(solver.m)])


def assert_inverse_and_b(solver, exact, reference, what):
    want = exact.inverse_long()
    bound, error = polished_tolerance(reference, want)
    device_error = float(np.abs(device_inverse(solver) - want).max())
    print("%s: inverse: device %.3e restatement %.3e ratio %.2f bound %.3e" % (what, device_error, error, device_error / max(error, 1e-300), bound))
    assert device_error <= bound, (what, "inverse", device_error, error, bound)
    rhs = np.array([float(v) for v in exact.b])
    want = long_double(*exact.x_basic())
    bound, error = polished_tolerance(reference @ rhs, want)
    device_error = float(np.abs(solver.b() - want).max())
    print("%s: b: device %.3e restatement %.3e ratio %.2f bound %.3e" % (what, device_error, error, device_error / max(error, 1e-300), bound))
    assert device_error <= bound, (what, "b", device_error, error, bound)


def walk_to_a_drifted_neighbour(solver):
    """Away from the optimal basis by forced pivots on evenly spaced non-basic columns (each through its ratio-test row), then up to
    ten pivots of the loop: a neighbouring basis whose resident inverse carries the rounding of about fifteen product-form updates."""
    basic = set(solver.basis().tolist())
    free = [j for j in range(solver.n_provider) if j not in basic]
    made = 0
    for j in free[::max(1, len(free) // 8)]:
        q = solver.n_art + j
        row, alpha = solver.select_primal_pivot_row(q)
        if row is None or abs(alpha[row]) < 1e-3 * np.abs(alpha).max():
            continue
        solver.bring_into_basis(q, row)
        made += 1
        if made == 5:
            break
    assert made >= 3
    done, _ = solver.iterate(10)
    return made + done


def check(name, **options):
    path, golden_basis, _, _, _ = problem(name)
    solver = relp_amd.Solver(polish_period=0, **options).load_mps(path)
    solver.set_basis(golden_basis)  # invert_from_scratch
    exact = exact_state(name, solver)
    B = exact.basis_matrix()
    assert_inverse_and_b(solver, exact, newton_schulz_inverse(B), name + " from scratch")
    assert walk_to_a_drifted_neighbour(solver) >= 3
    exact = exact_state(name, solver)
    B = exact.basis_matrix()
    if options.get("carry", CARRY_EXPLICIT) == CARRY_EXPLICIT:
        reference = newton_schulz_polish(B, device_inverse(solver))  # at most two steps from the device's drifted inverse
    else:
        reference = newton_schulz_inverse(B)  # an LU carry refactorises: it is held to the explicit carry's tolerance from scratch
    solver.refactor()
    assert_inverse_and_b(solver, exact, reference, name + " polished")
    solver.close()


@pytest.mark.parametrize("switches", [0, SW_GEMM_VECTOR], ids=["matrix cores", "plain FMA"])
@pytest.mark.parametrize("name, m, cond", CASES, ids=[case[0] for case in CASES])
def test_inversion_and_polish_against_the_exact_inverse(name, m, cond, switches):
    check(name, switches=switches)


@pytest.mark.parametrize("carry", [CARRY_EXPLICIT, CARRY_LU, CARRY_LU_INVERSE], ids=["explicit", "lu", "lu_inverse"])
def test_every_carry_on_sc105(carry):
    check("SC105", carry=carry)


def walk_through_small_pivots(solver, count=12, smallest=1e-3):
    """Forced pivots on evenly spaced non-basic columns, each on the row with the SMALLEST entry of its column that is still ``smallest``
    of the largest: a neighbouring basis of worse condition whose resident inverse has drifted (numpy restatement on E226: residual
    2.9e-8, cond 4e8).  The vertex need not stay feasible: the polish recomputes b from the inverse."""
    basic = set(solver.basis().tolist())
    free = [j for j in range(solver.n_provider) if j not in basic]
    made = 0
    for j in free[::max(1, len(free) // (2 * count))]:
        q = solver.n_art + j
        _, alpha = solver.select_primal_pivot_row(q)
        size = np.abs(alpha)
        if size.max() == 0.0:
            continue
        row = int(np.argmin(np.where(size >= smallest * size.max(), size, np.inf)))
        solver.bring_into_basis(q, row)
        made += 1
        if made == count:
            break
    return made


@pytest.mark.parametrize("switches", [0, SW_GEMM_VECTOR], ids=["matrix cores", "plain FMA"])
def test_polish_step_on_a_drifted_inverse(switches):
    """``Solver::polish`` taking its Newton steps (residual_kernel writing S, the polish GEMM in both forms) on E226, m = 223."""
    path, golden_basis, _, _, _ = problem("E226")
    solver = relp_amd.Solver(polish_period=0, switches=switches).load_mps(path)
    solver.set_basis(golden_basis)
    assert walk_through_small_pivots(solver) == 12
    exact = exact_state("E226", solver)
    reference = newton_schulz_polish(exact.basis_matrix(), device_inverse(solver))
    residual = solver.refactor()
    print("E226 drifted: residual found by the polish %.3e" % residual)
    assert 1e-12 <= residual < 0.5  # a step was taken (none below 1e-12; from scratch at 0.5)
    assert_inverse_and_b(solver, exact, reference, "E226 drifted, polished")
    solver.close()
