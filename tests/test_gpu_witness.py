"""The exact witnesses of certified results (``Solver.witness_exact``, ``Many.witness_exact``, ``Many.solution_exact``): x, the dual
solution or Farkas vector y, and the ray ("What the certificate hands out").

The judge is ``relp_amd/witness.py``: rational arithmetic on the model's exact data, no call into the solver or the certificate
(tests/test_witness_host.py tries it on hand-computed LPs).  Every comparison is equality of rationals or an exact inequality."""
import random
from fractions import Fraction

import pytest

import relp_amd
from relp_amd import WITNESS_DUAL, WITNESS_PRIMAL, WITNESS_RAY
from relp_amd.api import ERR_ARGUMENT, ERR_STATE, MANY_CERTIFY_ALL_KINDS, MANY_CERTIFY_OPTIMA, MANY_CERTIFY_SERIAL, MANY_FALLBACK_NAMES
from relp_amd.witness import WitnessError, check_infeasible, check_optimum, check_unbounded
from test_gpu_many_certify import model_of_case, netlib, random_lp

pytestmark = pytest.mark.gpu

DEFINED = {relp_amd.FINITE_OPTIMUM: (WITNESS_PRIMAL, WITNESS_DUAL), relp_amd.INFEASIBLE: (WITNESS_DUAL,),
           relp_amd.UNBOUNDED: (WITNESS_PRIMAL, WITNESS_RAY)}

# (counts of =, <=, >= rows; columns; b; cost; upper): the seven LPs (a)-(g) of tests/test_gpu_many_certify_kinds.py
SMALL = [
    ([0, 0, 1], [[(0, -1)]], [1], [0], [None]),                                        # (a) -x >= 1: infeasible, phase-one optimum 1
    ([0, 0, 1], [[(0, 1)]], [1], [-1], [None]),                                        # (b) min -x, x >= 1: unbounded
    ([0, 1, 0], [[(0, 1)], [(0, -1)]], [0], [-1, 0], [None, None]),                    # (c) min -x, x - y <= 0: unbounded, b = 0
    ([0, 1, 0], [[(0, 1)], []], [3], [0, -1], [None, None]),                           # (d) min -z, z in no row: the ray is e_z
    ([2, 0, 0], [[(0, 1), (1, 1)], [(0, -1), (1, -1)]], [2, 2], [0, -1], [None, None]),  # (e) x - z = 2 twice, min -z: unbounded
    ([2, 0, 1], [[(0, 1), (1, 1), (2, 1)]], [2, 2, 3], [0], [None]),                    # (f) x = 2 twice, x >= 3: infeasible
    ([0, 1, 0], [[(0, 1)]], [3], [-1], [None]),                                        # (g) min -x, x <= 3: optimum -3
]
SMALL_KINDS = [relp_amd.INFEASIBLE, relp_amd.UNBOUNDED, relp_amd.UNBOUNDED, relp_amd.UNBOUNDED, relp_amd.UNBOUNDED, relp_amd.INFEASIBLE,
               relp_amd.FINITE_OPTIMUM]


def status_of(call, *args):
    with pytest.raises(relp_amd.RelpError) as info:
        call(*args)
    return info.value.status


def check_result(model, kind, witness, objective_text, who):
    """The checker on the witnesses of one certified result; `witness(which)` returns a dict.  Returns what it read."""
    got = {which: witness(which) for which in DEFINED[kind]}
    for which in set(range(3)) - set(DEFINED[kind]):  # the other combinations are refused
        assert status_of(witness, which) == ERR_STATE, (who, kind, which)
    try:
        if kind == relp_amd.FINITE_OPTIMUM:
            check_optimum(model, got[WITNESS_PRIMAL], got[WITNESS_DUAL], Fraction(objective_text))
        elif kind == relp_amd.INFEASIBLE:
            check_infeasible(model, got[WITNESS_DUAL], Fraction(objective_text))  # y'b is the value objective_exact returns
        else:
            assert objective_text == "-inf", who
            check_unbounded(model, got[WITNESS_PRIMAL], got[WITNESS_RAY])
    except WitnessError as error:
        raise AssertionError("%s (kind %d): %s" % (who, kind, error))
    for values in got.values():
        assert list(values) == sorted(values) and all(v != 0 for v in values.values()), who  # non-zero entries, ascending index
    return got


def check_many(many, models, kinds, certificates, who):
    """Every certified result of a `certify(..., witnesses=True)`; returns the witnesses per LP (None where not certified)."""
    out = []
    for i, (model, kind, c) in enumerate(zip(models, kinds, certificates)):
        if not c.certified:
            out.append(None)
            continue
        out.append(check_result(model, kind, lambda which: many.witness_exact(i, which), many.objective_exact(i), (who, i)))
    return out


def fields(many, certificates, i):
    c = certificates[i]
    try:
        exact = many.objective_exact(i)
    except relp_amd.RelpError:
        exact = None
    return (c.certified, c.path, c.fallback_reason, c.digits_primal, c.digits_dual, c.repair_pivots) + many.certificate_digits(i) + (exact,)


# ---- 4. the smallest shapes --------------------------------------------------------------------------------------------------
def test_the_smallest_shapes_pass_the_checker_on_both_paths():
    models = [model_of_case(case) for case in SMALL]
    many = relp_amd.Many(models)
    results = many.solve()
    assert [r.status for r in results] == [0] * 7 and [r.kind for r in results] == SMALL_KINDS
    batched = many.certify(mode=MANY_CERTIFY_ALL_KINDS, witnesses=True)
    assert [(c.certified, c.path) for c in batched] == [(1, 1)] * 7, [MANY_FALLBACK_NAMES[c.fallback_reason] for c in batched]
    from_batch = check_many(many, models, SMALL_KINDS, batched, "batched")
    assert Fraction(many.objective_exact(0)) == 1 and Fraction(many.objective_exact(5)) == 1  # the phase-one optima of (a) and (f)
    assert from_batch[2][WITNESS_PRIMAL] == {}                                   # (c): a zero right-hand side, x = 0
    assert from_batch[3][WITNESS_RAY] == {1: 1}                                  # (d): a column without entries, the ray is e_q alone
    assert any(v < 0 for v in many.basis(4)) and any(v < 0 for v in many.basis(5))  # (e), (f): an artificial stays basic ...
    assert all(0 <= j < models[i].nr_columns for i in (4, 5) for which, w in from_batch[i].items() if which != WITNESS_DUAL
               for j in w)  # ... and is never reported: the column witnesses name provider columns only
    assert from_batch[6] == {WITNESS_PRIMAL: {0: 3}, WITNESS_DUAL: {0: -1}}       # (g): x = 3, y = -1
    assert many.solution_exact(6) == {0: 3} and many.solution_exact(6, original=True) == {0: 3}
    serial = many.certify(mode=MANY_CERTIFY_SERIAL, witnesses=True)
    assert [(c.certified, c.path) for c in serial] == [(1, 2)] * 7
    from_serial = check_many(many, models, SMALL_KINDS, serial, "serial")
    for i, c in enumerate(serial):
        if c.repair_pivots == 0:
            assert from_serial[i] == from_batch[i], i
    many.close()


# ---- 5. the seeded population ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seeded():
    """The 240 LPs of tests/test_gpu_many_certify.py, solved once."""
    rng = random.Random(20261016)
    models = [model_of_case(random_lp(rng)) for _ in range(240)]
    many = relp_amd.Many(models)
    results = many.solve()
    assert all(r.status == 0 for r in results)
    yield {"models": models, "many": many, "kinds": [r.kind for r in results]}
    many.close()


@pytest.mark.parametrize("mode", [MANY_CERTIFY_ALL_KINDS, MANY_CERTIFY_OPTIMA])
def test_random_lps_every_certified_result_passes_the_checker_and_the_switch_changes_no_certificate(seeded, mode):
    many, models, kinds = seeded["many"], seeded["models"], seeded["kinds"]
    n = len(models)
    assert set(kinds) == {relp_amd.FINITE_OPTIMUM, relp_amd.INFEASIBLE, relp_amd.UNBOUNDED}
    without = many.certify(mode=mode)
    fields_without = [fields(many, without, i) for i in range(n)]
    assert status_of(many.witness_exact, 0, WITNESS_DUAL) == ERR_STATE and "relp_many_keep_witnesses" in many.last_error()
    kept = many.certify(mode=mode, witnesses=True)
    assert [fields(many, kept, i) for i in range(n)] == fields_without
    assert all(c.certified == 1 for c in kept)
    witnesses = check_many(many, models, kinds, kept, "mode %d" % mode)
    for i, kind in enumerate(kinds):
        if kind != relp_amd.FINITE_OPTIMUM:
            assert kept[i].path == (1 if mode == MANY_CERTIFY_ALL_KINDS else 2), (i, kind)
        else:
            structural = {j: v for j, v in witnesses[i][WITNESS_PRIMAL].items() if j < models[i].nr_structural}
            assert many.solution_exact(i) == structural, i


# ---- 6. both tiers of the batched certificate -----------------------------------------------------------------------------------
def test_golden_lps_of_both_tiers_pass_the_checker_and_equal_the_handle():
    names = ["AFIRO", "SC50A", "SC50B", "ADLITTLE", "SC205"]
    models = [netlib(name) for name in names]
    edge = relp_amd.lib().relp_many_certify_lds_rows()
    assert edge == 198 and [m.nr_rows <= edge for m in models] == [True, True, True, True, False] and models[0].nr_rows == 27
    many = relp_amd.Many(models)
    results = many.solve()
    certificates = many.certify(mode=MANY_CERTIFY_OPTIMA, witnesses=True)
    kinds = [r.kind for r in results]
    assert kinds == [relp_amd.FINITE_OPTIMUM] * 5
    assert [(c.certified, c.path) for c in certificates] == [(1, 1)] * 5, [MANY_FALLBACK_NAMES[c.fallback_reason] for c in certificates]
    witnesses = check_many(many, models, kinds, certificates, "golden")
    for i, model in enumerate(models):
        x = witnesses[i][WITNESS_PRIMAL]
        assert x and many.solution_exact(i) == {j: v for j, v in x.items() if j < model.nr_structural}, names[i]
    for i in range(3):
        solver = relp_amd.Solver(certify=1).load_model(models[i])
        result = solver.solve_relaxation()
        assert result.kind == relp_amd.FINITE_OPTIMUM and result.certified
        assert list(solver.basis()) == list(many.basis(i)), names[i]
        assert many.solution_exact(i, original=True) == solver.solution_exact(original=True), names[i]
        assert many.witness_exact(i, WITNESS_DUAL) == solver.witness_exact(WITNESS_DUAL), names[i]
        assert many.witness_exact(i, WITNESS_PRIMAL) == solver.witness_exact(WITNESS_PRIMAL), names[i]
        solver.close()
    many.close()


# ---- 7. the handle -----------------------------------------------------------------------------------------------------------
def test_a_handle_hands_out_the_witnesses_of_every_kind():
    lps = [("small %d" % i, model_of_case(case), kind) for i, (case, kind) in enumerate(zip(SMALL, SMALL_KINDS))]
    lps.append(("AFIRO", netlib("AFIRO"), relp_amd.FINITE_OPTIMUM))
    for name, model, kind in lps:
        solver = relp_amd.Solver(certify=1).load_model(model)
        assert status_of(solver.witness_exact, WITNESS_PRIMAL) == ERR_STATE, name  # nothing solved yet
        result = solver.solve_relaxation()
        assert result.kind == kind and result.certified == 1, (name, result.kind, result.certified)
        got = check_result(model, kind, solver.witness_exact, solver.objective_exact(), name)
        if kind == relp_amd.FINITE_OPTIMUM:
            assert solver.solution_exact() == {j: v for j, v in got[WITNESS_PRIMAL].items() if j < model.nr_structural}, name
        assert status_of(solver.witness_exact, 3) == ERR_ARGUMENT and status_of(solver.witness_exact, -1) == ERR_ARGUMENT, name
        solver.close()
    uncertified = relp_amd.Solver().load_model(lps[-1][1])
    assert uncertified.solve_relaxation().kind == relp_amd.FINITE_OPTIMUM
    assert status_of(uncertified.witness_exact, WITNESS_DUAL) == ERR_STATE
    uncertified.close()


# ---- 8. implicit bounds ------------------------------------------------------------------------------------------------------
def test_lps_solved_with_implicit_bounds_pass_the_checker_in_the_formulation_with_bound_rows():
    rng = random.Random(20261016)
    cases = [case for case in (random_lp(rng) for _ in range(240)) if any(u is not None for u in case[4])][:24]
    assert len(cases) == 24
    cases.append(([0, 0, 1], [[(0, 1)]], [3], [0], [2]))                # x >= 3 with x <= 2 as a bound: infeasible
    models = [model_of_case(case) for case in cases] + [netlib("KB2")]
    assert all(m.nr_rows > m.nr_constraints for m in models) and models[-1].nr_rows <= 198  # bound rows everywhere; KB2 in the LDS tier
    many = relp_amd.Many(models, bounded=True)
    results = many.solve()
    kinds = [r.kind for r in results]
    assert all(r.status == 0 for r in results) and set(kinds) == {relp_amd.FINITE_OPTIMUM, relp_amd.INFEASIBLE, relp_amd.UNBOUNDED}
    assert kinds[24:] == [relp_amd.INFEASIBLE, relp_amd.FINITE_OPTIMUM] and results[-1].inverse_in_lds == 1
    for mode in (MANY_CERTIFY_OPTIMA, MANY_CERTIFY_ALL_KINDS):
        certificates = many.certify(mode=mode, witnesses=True)
        witnesses = check_many(many, models, kinds, certificates, "bounded, mode %d" % mode)  # the models hold the bound rows and slacks
        for i, (kind, c) in enumerate(zip(kinds, certificates)):
            if kind == relp_amd.FINITE_OPTIMUM:
                assert c.certified == 1 and witnesses[i] is not None, i
            else:
                assert (c.certified, c.path) == (0, 0), i
                for which in range(3):
                    assert status_of(many.witness_exact, i, which) == ERR_STATE, (i, which)
                assert status_of(many.solution_exact, i) == ERR_STATE, i
    many.close()


# ---- 9. states and arguments ---------------------------------------------------------------------------------------------------
def test_states_and_arguments():
    import ctypes as C
    models = [model_of_case(SMALL[6]), model_of_case(SMALL[0]), model_of_case(SMALL[1])]  # optimum, infeasible, unbounded
    many = relp_amd.Many(models)
    assert status_of(many.witness_exact, 0, WITNESS_PRIMAL) == ERR_STATE  # before a solve
    many.solve()
    assert status_of(many.witness_exact, 0, WITNESS_PRIMAL) == ERR_STATE  # before any certify
    assert status_of(many.solution_exact, 0) == ERR_STATE
    many.certify(mode=MANY_CERTIFY_ALL_KINDS)
    assert status_of(many.witness_exact, 0, WITNESS_PRIMAL) == ERR_STATE and "relp_many_keep_witnesses" in many.last_error()
    assert status_of(many.solution_exact, 0) == ERR_STATE and "relp_many_keep_witnesses" in many.last_error()
    many.certify(mode=MANY_CERTIFY_ALL_KINDS, witnesses=True)
    for i, missing in ((0, WITNESS_RAY), (1, WITNESS_PRIMAL), (1, WITNESS_RAY), (2, WITNESS_DUAL)):
        assert status_of(many.witness_exact, i, missing) == ERR_STATE, (i, missing)
        assert "has no RELP_WITNESS_" in many.last_error(), many.last_error()
    assert status_of(many.solution_exact, 1) == ERR_STATE and status_of(many.solution_exact, 2) == ERR_STATE
    for index in (-1, 3):
        assert status_of(many.witness_exact, index, WITNESS_PRIMAL) == ERR_ARGUMENT, index
        assert status_of(many.solution_exact, index) == ERR_ARGUMENT, index
    for which in (-1, 3):
        assert status_of(many.witness_exact, 0, which) == ERR_ARGUMENT, which
    # the size query returns count and length without writing; a capacity that is too small is refused
    lib = relp_amd.lib()
    count, length = C.c_int32(-1), C.c_int64(-1)
    assert lib.relp_many_get_witness_exact(many._h, 0, WITNESS_PRIMAL, 0, C.byref(count), None, None, C.c_int64(0), C.byref(length)) == 0
    assert (count.value, length.value) == (1, len("3/1") + 1)
    index = (C.c_int32 * 1)(-7)
    buffer = C.create_string_buffer(b"#" * 8, 8)
    args = (many._h, 0, WITNESS_PRIMAL)
    assert lib.relp_many_get_witness_exact(*args, 0, C.byref(count), index, buffer, C.c_int64(8), C.byref(length)) == ERR_ARGUMENT
    assert lib.relp_many_get_witness_exact(*args, 1, C.byref(count), index, buffer, C.c_int64(3), C.byref(length)) == ERR_ARGUMENT
    assert lib.relp_many_get_witness_exact(*args, 1, C.byref(count), None, buffer, C.c_int64(8), C.byref(length)) == ERR_ARGUMENT
    assert index[0] == -7 and buffer.raw == b"#" * 8  # nothing was written
    assert lib.relp_many_get_witness_exact(*args, 1, C.byref(count), index, buffer, C.c_int64(4), C.byref(length)) == 0
    assert index[0] == 0 and buffer.raw[:4] == b"3/1\0"
    assert lib.relp_many_get_solution_exact(many._h, 0, 0, 0, C.byref(count), index, buffer, C.c_int64(8), C.byref(length)) == ERR_ARGUMENT
    assert lib.relp_many_keep_witnesses(many._h, 2) == ERR_ARGUMENT
    many.solve()  # a new solve: the witnesses of the old certificate are gone
    assert status_of(many.witness_exact, 0, WITNESS_PRIMAL) == ERR_STATE
    many.certify(mode=MANY_CERTIFY_ALL_KINDS, witnesses=True)
    assert many.witness_exact(0, WITNESS_PRIMAL) == {0: 3}
    many.certify(mode=MANY_CERTIFY_ALL_KINDS)  # ... and so are they after a certify with the switch off
    assert status_of(many.witness_exact, 0, WITNESS_PRIMAL) == ERR_STATE
    many.close()


# ---- 10. a negative control on device data -----------------------------------------------------------------------------------
def test_a_falsified_dual_of_afiro_is_rejected():
    model = netlib("AFIRO")
    many = relp_amd.Many([model])
    many.solve()
    assert many.certify(mode=MANY_CERTIFY_OPTIMA, witnesses=True)[0].certified == 1
    x, y, objective = many.witness_exact(0, WITNESS_PRIMAL), many.witness_exact(0, WITNESS_DUAL), Fraction(many.objective_exact(0))
    check_optimum(model, x, y, objective)
    assert objective == Fraction(-406659, 875)
    rhs = model.right_hand_side_exact()
    rows = [row for row in y if rhs[row] != 0]
    assert rows
    for row in rows:  # b_row != 0: the value y'b moves by b_row, unless a reduced cost turns negative first
        with pytest.raises(WitnessError):
            check_optimum(model, x, {**y, row: y[row] + 1}, objective)
    many.close()
