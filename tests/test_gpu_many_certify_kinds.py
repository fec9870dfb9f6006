"""``relp_many_certify`` mode 2: INFEASIBLE and UNBOUNDED results proved in the one launch ("The batched certificate").

The yardstick is always ``certify(mode=1)``, the serial certificate, which this feature leaves as it is."""
import random
from fractions import Fraction

import pytest

import relp_amd
from relp_amd.api import (ERR_ARGUMENT, ERR_STATE, MANY_CERTIFY_ALL_KINDS, MANY_CERTIFY_OPTIMA, MANY_CERTIFY_SERIAL, MANY_FALLBACK_KIND,
                          MANY_FALLBACK_NAMES, MANY_FALLBACK_NONE)
from relp_oracle import Infeasible, Unbounded
from test_gpu_many_certify import model_of_case, oracle_objective, random_lp

pytestmark = pytest.mark.gpu

KIND_OF = {Infeasible: relp_amd.INFEASIBLE, Unbounded: relp_amd.UNBOUNDED, Fraction: relp_amd.FINITE_OPTIMUM}


def exact_or_none(many, i):
    try:
        return many.objective_exact(i)
    except relp_amd.RelpError:
        return None


def proof(many, certificates, i):
    c = certificates[i]
    return (c.certified, c.path, c.fallback_reason) + many.certificate_digits(i) + (exact_or_none(many, i),)


# ---- 1. the smallest shapes ------------------------------------------------------------------------------------------------
def test_the_smallest_shapes_of_every_kind_in_one_launch():
    # (counts of =, <=, >= rows; columns; b; cost; upper) -- random_lp's notation; the last entry: a ray with entries is solved for
    cases = [
        (([0, 0, 1], [[(0, -1)]], [1], [0], [None]), False),                                      # (a) -x >= 1
        (([0, 0, 1], [[(0, 1)]], [1], [-1], [None]), True),                                       # (b) min -x, x >= 1
        (([0, 1, 0], [[(0, 1)], [(0, -1)]], [0], [-1, 0], [None, None]), True),                   # (c) min -x, x - y <= 0: b = 0
        (([0, 1, 0], [[(0, 1)], []], [3], [0, -1], [None, None]), False),                         # (d) min -z, z in no row
        (([2, 0, 0], [[(0, 1), (1, 1)], [(0, -1), (1, -1)]], [2, 2], [0, -1], [None, None]), True),  # (e) x - z = 2 twice, min -z
        (([2, 0, 1], [[(0, 1), (1, 1), (2, 1)]], [2, 2, 3], [0], [None]), False),                  # (f) x = 2 twice, x >= 3
        (([0, 1, 0], [[(0, 1)]], [3], [-1], [None]), False),                                      # (g) min -x, x <= 3
    ]
    many = relp_amd.Many([model_of_case(case) for case, _ in cases])
    results = many.solve()
    many.certify(mode=MANY_CERTIFY_SERIAL)
    serial_exact = [exact_or_none(many, i) for i in range(len(cases))]
    certificates = many.certify(mode=MANY_CERTIFY_ALL_KINDS)
    assert many.certify_device_seconds > 0
    for i, (case, has_ray) in enumerate(cases):
        expected = oracle_objective(case)
        assert results[i].status == 0 and results[i].kind == KIND_OF[type(expected)], (i, results[i].status, results[i].kind)
        c = certificates[i]
        assert (c.certified, c.path, c.fallback_reason) == (1, 1, MANY_FALLBACK_NONE), (i, MANY_FALLBACK_NAMES[c.fallback_reason], many.last_error())
        assert many.objective_exact(i) == serial_exact[i] and serial_exact[i] is not None, i
        if isinstance(expected, Unbounded):
            assert serial_exact[i] == "-inf", i
        elif isinstance(expected, Infeasible):
            assert Fraction(serial_exact[i]) > 0, i
        else:
            assert Fraction(serial_exact[i]) == expected, i
        digits = many.certificate_digits(i)
        assert digits[:2] == (c.digits_primal, c.digits_dual), i
        assert (digits[2] > 0) == has_ray, (i, digits)
    assert Fraction(serial_exact[0]) == 1 and Fraction(serial_exact[5]) == 1  # the phase-one optima of (a) and (f)
    assert many.certificate_digits(2)[0] == 0                                # (c): a zero right-hand side, nothing to lift for x
    assert any(v < 0 for v in many.basis(4)) and any(v < 0 for v in many.basis(5))  # (e), (f): an artificial stays basic
    many.close()


# ---- 2. the 240 seeded LPs -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seeded():
    """The 240 LPs of tests/test_gpu_many_certify.py, solved once; what the serial certificate says about each."""
    rng = random.Random(20261016)
    cases = [random_lp(rng) for _ in range(240)]
    models = [model_of_case(c) for c in cases]
    many = relp_amd.Many(models)
    results = many.solve()
    serial = many.certify(mode=MANY_CERTIFY_SERIAL)
    serial_exact = [exact_or_none(many, i) for i in range(len(cases))]
    yield {"models": models, "many": many, "kinds": [r.kind for r in results], "status": [r.status for r in results],
           "serial": [(c.certified, c.repair_pivots) for c in serial], "serial_exact": serial_exact}
    many.close()


def test_random_lps_every_infeasible_and_unbounded_verdict_is_proved_in_the_batch(seeded):
    many, kinds = seeded["many"], seeded["kinds"]
    n = len(kinds)
    assert set(kinds) == {relp_amd.FINITE_OPTIMUM, relp_amd.INFEASIBLE, relp_amd.UNBOUNDED} and all(s == 0 for s in seeded["status"])
    all_kinds = many.certify(mode=MANY_CERTIFY_ALL_KINDS)
    all_kinds_proofs = [proof(many, all_kinds, i) for i in range(n)]
    optima = many.certify(mode=MANY_CERTIFY_OPTIMA)
    optima_proofs = [proof(many, optima, i) for i in range(n)]
    for i in range(n):
        certified, path, reason, k_primal, k_dual, k_ray, exact = all_kinds_proofs[i]
        assert certified == seeded["serial"][i][0] == 1, (i, kinds[i], MANY_FALLBACK_NAMES[reason])
        assert exact == seeded["serial_exact"][i] and exact is not None, i
        if kinds[i] == relp_amd.FINITE_OPTIMUM:
            assert all_kinds_proofs[i] == optima_proofs[i] and k_ray == 0, i
        else:
            assert (path, reason) == (1, MANY_FALLBACK_NONE), (i, kinds[i], MANY_FALLBACK_NAMES[reason], many.last_error())
            assert exact == "-inf" if kinds[i] == relp_amd.UNBOUNDED else Fraction(exact) > 0, i
            assert k_ray == 0 or kinds[i] == relp_amd.UNBOUNDED, i
            assert 0 <= max(k_primal, k_dual, k_ray) <= 512, i
            # ... and mode 0 on the same handle hands them to the serial certificate again
            assert optima_proofs[i] == (1, 2, MANY_FALLBACK_KIND, 0, 0, 0, exact), i
    assert any(p[5] > 0 for p in all_kinds_proofs)  # rays were lifted


# ---- 3. both sides of the LDS boundary -----------------------------------------------------------------------------------------
def chain(m, unbounded):
    """x_i - x_{i+1} = 1 for i < m - 1, so x_0 = x_{m-1} + m - 1 >= m - 1; with x_0 <= m - 3 infeasible, with x_0 >= m and min -x_0
    unbounded.  m rows, m variables."""
    columns = [[] for _ in range(m)]
    for i in range(m - 1):
        columns[i].append((i, 1))
        columns[i + 1].append((i, -1))
    columns[0].append((m - 1, 1))
    columns = [sorted(column) for column in columns]
    kinds = ["Equal"] * (m - 1) + ["Greater" if unbounded else "Less"]
    b = [1] * (m - 1) + [m if unbounded else m - 3]
    cost = [-1 if unbounded and j == 0 else 0 for j in range(m)]
    return relp_amd.Model.from_general_form(columns, kinds, b, [(c, 0, None) for c in cost])


def test_chains_of_both_kinds_on_both_sides_of_the_lds_boundary():
    edge = relp_amd.lib().relp_many_certify_lds_rows()
    assert edge == 198
    shapes = [(m, unbounded) for m in (198, 199, 200) for unbounded in (False, True)]
    many = relp_amd.Many([chain(m, unbounded) for m, unbounded in shapes])
    results = many.solve()
    many.certify(mode=MANY_CERTIFY_SERIAL)
    serial_exact = [exact_or_none(many, i) for i in range(len(shapes))]
    certificates = many.certify(mode=MANY_CERTIFY_ALL_KINDS)
    tiers = set()
    for i, (m, unbounded) in enumerate(shapes):
        assert results[i].status == 0 and results[i].kind == (relp_amd.UNBOUNDED if unbounded else relp_amd.INFEASIBLE), (m, unbounded, results[i].kind)
        assert many._dimensions(i)[0] == m and results[i].inverse_in_lds == 0, (m, unbounded)  # (the solve's LDS tier ends at 139 rows)
        c = certificates[i]
        assert (c.certified, c.path, c.fallback_reason) == (1, 1, MANY_FALLBACK_NONE), (m, unbounded, MANY_FALLBACK_NAMES[c.fallback_reason], many.last_error())
        assert many.objective_exact(i) == serial_exact[i] and serial_exact[i] is not None, (m, unbounded)
        assert serial_exact[i] == ("-inf" if unbounded else "2/1"), (m, unbounded, serial_exact[i])  # x_0 - (m - 3) >= 2
        assert (many.certificate_digits(i)[2] > 0) == unbounded, (m, unbounded)
        tiers.add((m <= edge, unbounded))
    assert tiers == {(True, False), (True, True), (False, False), (False, True)}  # work matrix in LDS and in global memory, both kinds
    many.close()


# ---- 4. independence -----------------------------------------------------------------------------------------------------
def test_a_proof_of_either_kind_does_not_depend_on_the_other_lps_of_the_launch(seeded):
    kinds, models = seeded["kinds"], seeded["models"]
    unrepaired = [i for i, k in enumerate(kinds) if k == relp_amd.FINITE_OPTIMUM and seeded["serial"][i][1] == 0]
    chosen = [i for i, k in enumerate(kinds) if k == relp_amd.INFEASIBLE][:4] + [i for i, k in enumerate(kinds) if k == relp_amd.UNBOUNDED][:4]
    assert len(chosen) == 8 and len(unrepaired) >= 56
    alone = {}
    for i in chosen:
        many = relp_amd.Many([models[i]])
        many.solve()
        alone[i] = proof(many, many.certify(mode=MANY_CERTIFY_ALL_KINDS), 0)
        assert alone[i][:3] == (1, 1, MANY_FALLBACK_NONE) and alone[i][6] == seeded["serial_exact"][i], (i, alone[i])
        many.close()
    mixed = unrepaired[:56]
    first = [v for pair in zip(chosen, mixed[:8]) for v in pair] + mixed[8:]  # the eight spread among optima
    second = mixed[8:][::-1] + chosen[::-1] + mixed[:8]                       # ... and in a block, everything reversed
    assert sorted(first) == sorted(second) and len(first) == 64
    seen = []
    for order in (first, second):
        many = relp_amd.Many([models[i] for i in order])
        many.solve()
        certificates = many.certify(mode=MANY_CERTIFY_ALL_KINDS)
        proofs = {i: proof(many, certificates, slot) for slot, i in enumerate(order)}
        for i in chosen:
            assert proofs[i] == alone[i], i
        seen.append(proofs)
        many.close()
    assert seen[0] == seen[1]


# ---- 5. state and arguments -------------------------------------------------------------------------------------------------
def test_digits_need_a_certify_and_other_modes_are_refused_and_a_bounded_lp_keeps_path_0():
    infeasible = ([0, 0, 1], [[(0, 1)]], [3], [0], [2])  # x >= 3 with x <= 2 as a bound
    optimum = ([0, 1, 0], [[(0, 1)]], [3], [-1], [2])
    many = relp_amd.Many([model_of_case(infeasible), model_of_case(optimum)], bounded=True)
    with pytest.raises(relp_amd.RelpError) as info:
        many.certificate_digits(0)
    assert info.value.status == ERR_STATE
    results = many.solve()
    assert [r.status for r in results] == [0, 0] and [r.kind for r in results] == [relp_amd.INFEASIBLE, relp_amd.FINITE_OPTIMUM]
    with pytest.raises(relp_amd.RelpError) as info:
        many.certificate_digits(0)
    assert info.value.status == ERR_STATE
    for mode in (3, -1):
        with pytest.raises(relp_amd.RelpError) as info:
            many.certify(mode=mode)
        assert info.value.status == ERR_ARGUMENT, mode
    certificates = many.certify(mode=MANY_CERTIFY_ALL_KINDS)
    assert (certificates[0].certified, certificates[0].path, certificates[0].fallback_reason) == (0, 0, MANY_FALLBACK_NONE)
    assert exact_or_none(many, 0) is None and many.certificate_digits(0) == (0, 0, 0)
    assert certificates[1].certified == 1 and certificates[1].path in (1, 2) and Fraction(many.objective_exact(1)) == -2
    many.solve()  # a new solve: the digits of the old certificate are gone
    with pytest.raises(relp_amd.RelpError) as info:
        many.certificate_digits(1)
    assert info.value.status == ERR_STATE
    many.close()
