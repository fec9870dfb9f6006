"""The host side of the dual simplex's steepest-edge leaving rule (no GPU): the option in the ABI -- the new symbol, the default, the
values ``relp_create`` refuses, a struct of the previous size -- and the inputs of the pivot-for-pivot GPU cases,
``dual_se_lps.SE_WALK_CASES``, checked with the exact reference alone.

As in tests/test_dual_host.py the parent's optimal basis and vertex come from the oracle's cold solve here (the GPU tests take them
from the certified device solve), and the child's exact optimum is the oracle's cold solve of the child.
"""
import ctypes as C

import pytest

import relp_amd
from relp_amd import api
from relp_oracle.solve import FiniteOptimum, solve_relaxation_full_basis
import dual_lps
import dual_se_lps
import sparse_lps


def test_the_symbols_exist():
    lib = relp_amd.lib()
    assert hasattr(lib, "relp_get_dual_weights") and "relp_get_dual_weights" in relp_amd.SYMBOLS
    assert callable(relp_amd.Solver.dual_weights)
    assert (api.DUAL_PRICING_INFEASIBILITY, api.DUAL_PRICING_STEEPEST_EDGE) == (0, 1)
    assert lib.relp_get_dual_weights(None, None) == api.ERR_ARGUMENT


def test_the_default_is_largest_infeasibility():
    options = api.default_options()
    assert options.dual_pricing == 0 and options.reserved_round7 == 0
    assert api.Options.dual_pricing.offset == api.Options.carry_weights_min.offset + 8
    assert C.sizeof(api.Options) == api.Options.reserved_round7.offset + 4  # eight bytes more, no tail padding


@pytest.mark.parametrize("field,value", [("dual_pricing", 2), ("dual_pricing", -1), ("reserved_round7", 1)])
def test_create_refuses_what_the_option_does_not_name(field, value):
    options = api.default_options(**{field: value})
    handle = C.c_void_p()
    assert relp_amd.lib().relp_create(C.byref(options), C.byref(handle)) == api.ERR_ARGUMENT
    assert not handle.value


def test_a_struct_of_the_previous_size_is_still_accepted():
    """A caller built against the header before this option: ``relp_options_default_sized`` writes its bytes only, and ``relp_create``
    reads that many -- whatever lies behind them in the caller's memory, the handle prices by largest infeasibility."""
    lib = relp_amd.lib()
    previous = api.Options.carry_weights_min.offset + 8
    assert previous == C.sizeof(api.Options) - 8
    buffer = (C.c_ubyte * C.sizeof(api.Options))(*([0xAB] * C.sizeof(api.Options)))
    options = C.cast(buffer, C.POINTER(api.Options))
    assert lib.relp_options_default_sized(options, previous) == api.OK
    assert options.contents.struct_size == previous and all(b == 0xAB for b in bytes(buffer)[previous:])
    handle = C.c_void_p()
    status = lib.relp_create(options, C.byref(handle))
    assert status != api.ERR_ARGUMENT  # (without a device the options are adopted and the handle's stream cannot be made: another status)
    if status == api.OK:
        lib.relp_destroy(handle)
    stale = api.default_options()
    stale.struct_size = previous + 4  # half of the new fields: no header ever had that size
    assert lib.relp_create(C.byref(stale), C.byref(handle)) == api.ERR_ARGUMENT


@pytest.mark.parametrize("m", sorted(dual_se_lps.SE_WALK_CASES))
def test_the_walk_cases_meet_their_conditions(m):
    seed, n_cuts = dual_se_lps.SE_WALK_CASES[m]
    case = dual_lps.cut_case(m, dual_lps.MIXED, seed, n_cuts)
    parent = solve_relaxation_full_basis(sparse_lps.Provider(case.parent))
    assert isinstance(parent, FiniteOptimum)
    vertex = {j: v for j, v in parent.solution if j < case.n_structural}
    child, basis, cuts = case.child(parent.basis, vertex)
    assert len(cuts) == n_cuts and child.nr_rows == m + n_cuts
    reference = dual_se_lps.DualSteepestReference(child, basis)
    assert min(reference.reduced_costs()) >= 0 and min(reference.x) < 0  # dual feasible, primal infeasible
    reason = reference.run()
    dual_lps.assert_walk_conditions(reference, m, reason)
    assert min(reference.x) >= 0 and min(reference.reduced_costs()) >= 0  # the walk's own x: optimal
    cold = solve_relaxation_full_basis(sparse_lps.Provider(child))
    assert isinstance(cold, FiniteOptimum)
    assert reference.objective() == cold.objective
    # x as the subclass keeps it is B^-1 b of the basis it ends at
    assert reference.x == [sum((row[i] * reference.b[i] for i in range(reference.m) if row[i]), 0) for row in reference.inverse]
    plain = dual_lps.DualReference(child, basis)
    plain.run()
    differs = next((k for k, (ours, theirs) in enumerate(zip(reference.pivots, plain.pivots)) if ours != theirs), None)
    print("m = %d: %d dual pivots (largest infeasibility: %d), smallest margin %.3g, smallest infeasibility %.3g, first differing pivot %s" % (
        m, len(reference.pivots), len(plain.pivots), reference.smallest_margin(), float(reference.smallest_infeasibility), differs))


def test_at_least_one_walk_differs_from_largest_infeasibility():
    """Otherwise the pivot-for-pivot comparison on the device could not tell the two rules apart."""
    differing = 0
    for m, (seed, n_cuts) in sorted(dual_se_lps.SE_WALK_CASES.items()):
        if m > 5 and differing:
            break  # (one is enough, and the small case is the cheap one)
        case = dual_lps.cut_case(m, dual_lps.MIXED, seed, n_cuts)
        parent = solve_relaxation_full_basis(sparse_lps.Provider(case.parent))
        child, basis, _ = case.child(parent.basis, {j: v for j, v in parent.solution if j < case.n_structural})
        steepest, plain = dual_se_lps.DualSteepestReference(child, basis), dual_lps.DualReference(child, basis)
        steepest.run()
        plain.run()
        differing += steepest.pivots != plain.pivots
    assert differing >= 1


def test_the_exact_weights_are_the_row_norms():
    from fractions import Fraction
    assert dual_se_lps.row_norms([[Fraction(1, 2), Fraction(0)], [Fraction(-3), Fraction(4)]]) == [Fraction(1, 4), Fraction(25)]
