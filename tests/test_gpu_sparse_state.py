"""The f64 state of a handle on the SPARSE pivot paths against the exact state of its basis, on each side of every row count at which
``plan_kernel_path`` takes another instantiation (``-m gpu``, a real MI355X).

The kernels are price_kernel<LDS | GATHER>, the k2f_* front half, pivot_fused_kernel<_, 2 | 4>, ftran_ratio_fast_kernel<_, 2 | 4 | 8 | 16>,
the k2l_* chain beyond 8192 rows and update_kernel<EAGER | PREDICATED | PREDICATED_SPLIT_GRID>.  Their row slots are ``i = tid + r * 512``,
so the sizes are 512 | 513, 1024 | 1025, 2048 | 2049, 4096 | 4097 and 8192 | 8193, on LPs (tests/sparse_lps.py) whose alphas reach every
slot, the last ragged one included.  Every case: ``Solver(polish_period=0, certify=0)``, 100 pivots (a batch of 64 -- replayed from a
graph unless ``use_graph=0`` -- and one of 36), ``stats().launches`` as the plan counts them, then ``assert_state`` (tests/state_checks.py)
against ``SparseBasisState`` of ``solver.basis()``: rows of the inverse (all for m <= 4097; at 8192 | 8193 every row that is not a unit
vector, rows 0 and m - 1, both sides of every multiple of 512 and every 16th), x_B, the objective, every relative cost, every
steepest-edge weight, three BTRANs with a small non-zero integer in every row, FTRANs through ``select_primal_pivot_row`` (one free column
of every length of the mix, one with the most and one with the fewest non-zeros in alpha) and the entering choice.

Tolerances are the project's for an un-polished state, unchanged (tests/state_checks.py); ``polished_tolerance`` after ``refactor()``.
Preconditions are asserted from the exact state so that no case goes trivial (``sparse_lps.preconditions``).  Each case asserts the fields of
``kernel_path()`` that name its instantiation before the device is touched.

Largest device error per part, measured on an MI355X (inverse, x_B, BTRAN, alpha: over max(1, largest entry); weights: relative; costs:
over 1 + |cost|, the scale of rtol = atol = 1e-9); one line per case:

  equality mixed  512  default         inverse 9.3e-14  x_B 3.3e-15  objective 3.2e-16  costs 2.7e-11  weights 2.3e-13  alpha 1.8e-14  btran 1.5e-14  (0.5 s)
  equality mixed  513  default         inverse 1.8e-14  x_B 1.3e-15  objective 3.3e-16  costs 1.0e-12  weights 2.1e-13  alpha 5.1e-15  btran 9.3e-15  (0.3 s)
  equality mixed 1024  default         inverse 5.5e-15  x_B 8.9e-16  objective 1.3e-16  costs 2.0e-12  weights 4.6e-13  alpha 1.1e-15  btran 1.7e-15  (0.4 s)
  equality mixed 1025  default         inverse 8.2e-15  x_B 9.4e-16  objective 4.0e-16  costs 2.0e-12  weights 8.5e-13  alpha 3.1e-15  btran 2.7e-15  (0.5 s)
  equality mixed 2048  default         inverse 8.5e-15  x_B 5.2e-16  objective 0.0e+00  costs 2.7e-12  weights 6.0e-13  alpha 1.6e-15  btran 2.1e-15  (0.8 s)
  equality mixed 2049  default         inverse 4.1e-15  x_B 5.0e-16  objective 3.8e-16  costs 1.1e-12  weights 3.3e-13  alpha 7.3e-16  btran 2.1e-15  (0.9 s)
  equality mixed 4096  default         inverse 8.2e-15  x_B 3.1e-16  objective 0.0e+00  costs 1.3e-12  weights 8.1e-14  alpha 7.7e-16  btran 1.0e-15  (2.0 s)
  equality mixed 4097  default         inverse 2.0e-15  x_B 3.8e-16  objective 0.0e+00  costs 1.2e-12  weights 7.5e-13  alpha 8.1e-16  btran 2.1e-15  (2.0 s)
  equality mixed 8192  default         inverse 1.8e-15  x_B 4.6e-16  objective 1.2e-16  costs 1.0e-12  weights 1.8e-13  alpha 4.9e-16  btran 1.3e-15  (3.6 s)
  equality mixed 8193  default         inverse 3.3e-15  x_B 4.5e-16  objective 0.0e+00  costs 1.4e-12  weights 1.1e-13  alpha 5.1e-16  btran 9.0e-16  (3.5 s)
  equality mixed  512  three kernels   inverse 9.3e-14  x_B 3.3e-15  objective 3.2e-16  costs 2.7e-11  weights 2.3e-13  alpha 1.8e-14  btran 1.5e-14  (0.2 s)
  equality mixed  513  three kernels   inverse 1.8e-14  x_B 1.3e-15  objective 3.3e-16  costs 1.0e-12  weights 2.1e-13  alpha 5.1e-15  btran 9.3e-15  (0.2 s)
  equality mixed 1024  three kernels   inverse 5.5e-15  x_B 8.9e-16  objective 1.3e-16  costs 2.0e-12  weights 4.6e-13  alpha 1.1e-15  btran 1.7e-15  (0.3 s)
  equality mixed 1025  three kernels   inverse 8.2e-15  x_B 9.4e-16  objective 4.0e-16  costs 2.0e-12  weights 8.5e-13  alpha 3.1e-15  btran 2.7e-15  (0.3 s)
  equality mixed 2048  three kernels   inverse 8.5e-15  x_B 5.2e-16  objective 0.0e+00  costs 2.7e-12  weights 6.0e-13  alpha 1.6e-15  btran 2.1e-15  (0.6 s)
  equality mixed 8193  one workgroup   inverse 3.3e-15  x_B 4.5e-16  objective 0.0e+00  costs 1.4e-12  weights 2.2e-13  alpha 5.1e-16  btran 9.0e-16  (2.1 s)
  equality mixed 2049  no touched rows inverse 4.1e-15  x_B 5.0e-16  objective 3.8e-16  costs 1.1e-12  weights 3.3e-13  alpha 7.3e-16  btran 2.1e-15  (0.6 s)
  equality short 1025  default         inverse 1.2e-14  x_B 3.8e-15  objective 3.9e-16  costs 1.4e-12  weights 3.5e-14  alpha 2.4e-15  btran 3.5e-15  (0.3 s)
  equality short 2049  default         inverse 2.5e-15  x_B 9.4e-16  objective 5.0e-16  costs 7.5e-14  weights 5.8e-13  alpha 7.0e-16  btran 1.9e-15  (0.6 s)
  less     mixed  513  default         inverse 1.7e-14  x_B 1.1e-15  objective 6.2e-16  costs 6.9e-12  weights 1.2e-12  alpha 2.4e-14  btran 7.2e-15  (0.2 s)
  less     mixed 1025  default         inverse 4.4e-15  x_B 4.2e-16  objective 1.9e-16  costs 1.0e-12  weights 7.8e-13  alpha 1.8e-15  btran 2.4e-15  (0.4 s)
  less     mixed 2049  default         inverse 3.1e-15  x_B 3.7e-16  objective 0.0e+00  costs 1.7e-12  weights 1.4e-12  alpha 3.5e-16  btran 1.6e-15  (1.0 s)
  less     mixed 4097  default         inverse 4.7e-15  x_B 5.6e-17  objective 2.2e-16  costs 2.3e-12  weights 1.1e-11  alpha 1.0e-15  btran 1.4e-15  (1.9 s)
  equality mixed 1025  plain launches  inverse 8.2e-15  x_B 9.4e-16  objective 4.0e-16  costs 2.0e-12  weights 8.5e-13  alpha 3.1e-15  btran 2.7e-15  (0.3 s)
  equality mixed 2049  plain launches  inverse 4.1e-15  x_B 5.0e-16  objective 3.8e-16  costs 1.1e-12  weights 3.3e-13  alpha 7.3e-16  btran 2.1e-15  (0.6 s)

(seconds: the whole case with its reference, the slowest being 8192 | 8193; the 100 pivots themselves take 2 - 13 ms, the rest is the
host's reference and the read-backs.)  The walk at
m = 2049 leaves a residual of 1.2e-14, below the 1e-12 under which the polish takes no step: after ``refactor()`` the inverse is 9.4e-15
from the exact one (bound 1.5e-13) and x_B 3.8e-14 (bound 6.2e-13).

Entered columns still basic after the 100 pivots (``sparse_lps.preconditions`` asks for 90 at the least), on the device, the same under
every option: equality mixed 512: 98, 513: 99, 1024: 100, 1025: 100, 2048: 99, 2049: 100, 4096: 100, 4097: 100, 8192: 99, 8193: 100;
equality short 1025: 100, 2049: 99; less mixed 513: 97, 1025: 99, 2049: 99, 4097: 99.

What the cases found: ``select_primal_pivot_row`` on the register-resident ratio test (``ftran_ratio_fast_kernel``, mode 2) left the
alpha of an EARLIER column in place when no row blocks the step (case equality-mixed-512: column 512, alpha = -3 on one row) -- it
stores the column on that way out now, as ``ftran_ratio_kernel`` always did.
"""
import time

import numpy as np
import pytest

import relp_amd
from relp_amd.api import SW_K2_SINGLE, SW_NO_TOUCHED
from basis_state import long_double
from state_checks import assert_polished, assert_state, device_inverse
import sparse_lps
from sparse_lps import btrans

pytestmark = pytest.mark.gpu
PIVOTS, BATCH = sparse_lps.PIVOTS, sparse_lps.BATCH


def expected_plan(family, m, options):
    """The fields of ``kernel_path()`` that name the instantiations a case is there for."""
    plan = {"n_dense": 0, "dense_blocks": 0, "ftran_slices": 0, "eta_mode": False, "lu_mode": False}  # neither a dense block nor the multi-block FTRAN
    three_kernels = options.get("pivot_kernels") == 1
    if family == "less":
        plan["n_art"] = 0
    if m <= 2048:
        rows = 2 if m <= 1024 else 4
        plan.update(fused=not three_kernels, ratio_kernel="REGISTERS_%d" % rows, ratio_kernel_no_change="REGISTERS_%d" % rows, update_kernel="EAGER")
        if not three_kernels:
            plan["fused_rows"] = rows
    else:
        touched = not options.get("switches", 0) & SW_NO_TOUCHED
        plan.update(fused=False, track_touched=touched, update_kernel="PREDICATED_SPLIT_GRID" if touched else "PREDICATED")
        if m <= 4096:
            plan.update(ratio_kernel="REGISTERS_8", ratio_kernel_no_change="REGISTERS_8", price_kernel="LDS")
        else:
            plan.update(price_kernel="GATHER", ell_w=8, generated_columns=False)
            if m <= 8192:
                plan.update(ratio_kernel="REGISTERS_16", ratio_kernel_no_change="REGISTERS_16")
            else:
                single = bool(options.get("switches", 0) & SW_K2_SINGLE)
                plan.update(ratio_kernel="ONE_WORKGROUP" if single else "MULTI_WORKGROUP", ratio_kernel_no_change="ONE_WORKGROUP")
    return plan


def launches(plan, use_graph):
    """What ``stats()`` counts for a batch of 64 and one of 36 (kernel_path.hpp: a replayed batch is the three-kernel chain, one budget launch)."""
    first = 1 + plan["launches_per_pivot_replayed"] * BATCH if use_graph else plan["launches_per_batch"] + plan["launches_per_pivot"] * BATCH
    return first + plan["launches_per_batch"] + plan["launches_per_pivot"] * (PIVOTS - BATCH)


def inverse_rows(exact, not_unit):
    m = exact.m
    if m <= 4097:
        return range(m)
    rows = set(not_unit) | {0, m - 1} | set(range(0, m, 16))
    for edge in range(512, m, 512):
        rows |= {edge - 1, edge}
    return sorted(rows)


def walked(family, mix, m, options):
    """A handle after 100 pivots, its exact state and what to check: the plan, the walk, the launch count and the preconditions."""
    model, provider, phase = sparse_lps.case(family, mix, m)
    options = dict(polish_period=0, certify=0, **options)
    plan = model.kernel_path(**options)
    for field, value in expected_plan(family, m, options).items():
        assert plan[field] == value, (field, plan[field], value)
    solver = relp_amd.Solver(**options).load_model(model)
    try:
        solver.begin_phase_one()  # (identity inverse, initial basis; with no artificial -- the `less` family -- this starts phase two)
        if phase == 2:
            assert solver.n_art == 0
            solver.begin_phase_two()  # the costs and weights of phase two once more, from the slack basis
        before = int(solver.stats().launches)
        started = time.perf_counter()
        assert solver.iterate(PIVOTS) == (PIVOTS, relp_amd.STOP_BUDGET)
        seconds = time.perf_counter() - started
        assert int(solver.stats().launches) - before == launches(plan, options.get("use_graph", 1))
        exact = provider.state(solver.basis(), phase)
        not_unit, columns, nnz, entered = sparse_lps.preconditions(exact, provider, mix)
    except BaseException:
        solver.close()
        raise
    checks = dict(inverse_rows=inverse_rows(exact, not_unit), alpha_columns=columns, btrans=btrans(m))
    print("%s %s m = %d %r: walk %.3f s, %d entered columns in the basis, k = %d, %d rows of the inverse are no unit vectors, nnz(alpha) of the checked columns %r" % (
        family, mix, m, options, seconds, entered, exact.k, len(not_unit), nnz))
    return solver, exact, provider, checks


OPTIONS = {"default": {}, "three kernels": {"pivot_kernels": 1}, "one workgroup": {"switches": SW_K2_SINGLE},
           "no touched rows": {"switches": SW_NO_TOUCHED}, "plain launches": {"use_graph": 0}}
CASES = [("equality", "mixed", m, "default") for m in (512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193)] + \
        [("equality", "mixed", m, "three kernels") for m in (512, 513, 1024, 1025, 2048)] + \
        [("equality", "mixed", 8193, "one workgroup"), ("equality", "mixed", 2049, "no touched rows")] + \
        [("equality", "short", m, "default") for m in (1025, 2049)] + \
        [("less", "mixed", m, "default") for m in (513, 1025, 2049, 4097)] + \
        [("equality", "mixed", m, "plain launches") for m in (1025, 2049)]


@pytest.mark.parametrize("family, mix, m, options", CASES, ids=["%s-%s-%d-%s" % case for case in CASES])
def test_state_after_100_pivots(family, mix, m, options):
    started = time.perf_counter()
    solver, exact, _, checks = walked(family, mix, m, OPTIONS[options])
    try:
        report = {}
        assert_state(solver, exact, report=report, **checks)
        print("%s %s %d, %s: %s; %.1f s" % (family, mix, m, options, ", ".join("%s %.1e" % item for item in sorted(report.items())),
                                          time.perf_counter() - started))
    finally:
        solver.close()


def test_by_rows_polish_over_the_touched_rows_of_a_sparse_walk():
    """``refactor()`` after the walk at m = 2049: the polish by rows over the rows the sparse path tracked as touched (the dense tests
    reach it only through ``eta_mode``).  Measured: the walk's residual is 1.2e-14, under the 1e-12 below which the polish takes no step,
    so for the inverse this says that the residual pass over the listed rows found nothing and left it alone; x_B and the objective are
    recomputed from it either way, and everything else is checked again."""
    solver, exact, provider, checks = walked("equality", "mixed", 2049, {})
    try:
        before = device_inverse(solver)
        print("residual found by the polish: %.3e" % solver.refactor())
        del checks["inverse_rows"]  # (assert_polished has read every row)
        assert_polished(solver, exact, before, np.array([float(v) for v in provider.b]), **checks)
    finally:
        solver.close()


# ---- the checks object to a wrong reference --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def at_1025():
    solver, exact, provider, checks = walked("equality", "mixed", 1025, {})
    yield solver, exact, provider, checks
    solver.close()


def test_weights_formed_without_the_one_are_refused(at_1025):
    solver, _, provider, checks = at_1025
    exact = provider.state(solver.basis(), 1)
    gammas = exact.gammas
    exact.gammas = lambda columns: gammas(columns) - 1
    with pytest.raises(AssertionError, match="gamma"):
        assert_state(solver, exact, **checks)


def test_the_state_of_a_basis_with_two_rows_exchanged_is_refused(at_1025):
    solver, exact, provider, checks = at_1025
    basis = solver.basis()
    first, second = (int(k) for k in exact.other[:2])  # two rows that hold structural columns: their rows of the inverse differ
    basis[[first, second]] = basis[[second, first]]
    with pytest.raises(AssertionError, match="row of the inverse"):
        assert_state(solver, provider.state(basis, 1), **checks)


def test_a_reference_with_a_wrong_last_stripe_is_refused_by_the_inverse_and_by_the_btran(at_1025):
    """Row m - 1 of the exact inverse replaced by the unit row: the row itself differs, and so does every BTRAN with an entry there."""
    solver, _, provider, checks = at_1025
    exact = provider.state(solver.basis(), 1)
    m = exact.m
    assert len(exact.row_exact(m - 1)[0]) > 1
    inverse_row, right_multiply = exact.inverse_row, exact.right_multiply
    unit = np.zeros(m)
    unit[m - 1] = 1.0

    def wrong_row(k):
        return (unit, np.zeros(m)) if k == m - 1 else inverse_row(k)

    def wrong_product(rows, values):
        weight = sum(float(v) for r, v in zip(rows, values) if r == m - 1)
        return right_multiply(rows, values) + weight * (long_double(unit, 0 * unit) - long_double(*inverse_row(m - 1)))
    exact.inverse_row = wrong_row
    with pytest.raises(AssertionError, match="row of the inverse"):
        assert_state(solver, exact, parts=("inverse",), **checks)
    exact.inverse_row = inverse_row
    exact.right_multiply = wrong_product
    with pytest.raises(AssertionError, match="btran"):
        assert_state(solver, exact, parts=("btran",), **checks)
    exact.right_multiply = right_multiply
    assert_state(solver, exact, parts=("inverse", "btran"), **checks)  # (and the true reference passes both)


def test_begin_phase_two_before_a_basis_is_refused():
    """``begin_phase_two()`` on a freshly loaded handle (the `less` family has no artificial, so phase two looks like the place to start)
    once ran set_phase over a basis, positions and an inverse nobody had written.  It is refused now; ``begin_phase_one()`` starts
    phase two on such an LP."""
    model, _, _ = sparse_lps.case("less", "mixed", 513)
    solver = relp_amd.Solver(polish_period=0, certify=0).load_model(model)
    try:
        with pytest.raises(relp_amd.api.RelpError, match="no basis yet") as refused:
            solver.begin_phase_two()
        assert refused.value.status == 5  # RELP_ERR_STATE: a call out of order
        solver.begin_phase_one()
        solver.begin_phase_two()
        assert solver.iterate(1) == (1, relp_amd.STOP_BUDGET)
    finally:
        solver.close()
