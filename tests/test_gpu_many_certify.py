"""``relp_many_certify``: the exact certificate of every LP of a launch in one further launch ("The batched certificate")."""
import json
import os
import random
from collections import Counter
from fractions import Fraction

import pytest

import relp_amd
from relp_amd.api import (ERR_ARGUMENT, ERR_STATE, MANY_FALLBACK_KIND, MANY_FALLBACK_NAMES, MANY_FALLBACK_NONE, MANY_FALLBACK_SINGULAR_MOD_P,
                          ManyCertificate)
from relp_oracle import FiniteOptimum, Infeasible, Unbounded, solve_relaxation
from relp_oracle.inverse_rows import BasisInverseRows
from relp_oracle.provider import MatrixData, Variable

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")


def golden_small(max_rows=512):
    """(name, fixture) of every golden LP of at most `max_rows` standard-form rows whose file is shipped, smallest first."""
    out = []
    for name in sorted(os.listdir(GOLDEN_DIR)):
        if not name.endswith(".json"):
            continue
        fixture = json.load(open(os.path.join(GOLDEN_DIR, name)))
        if not isinstance(fixture, dict) or "m" not in fixture or fixture.get("status") != "optimal":
            continue
        if fixture["m"] <= max_rows and os.path.exists(os.path.join(ROOT, fixture["file"])):
            out.append((name[:-5], fixture))
    return sorted(out, key=lambda item: (item[1]["m"], item[0]))


def netlib(name):
    return relp_amd.Model(os.path.join(ROOT, "data", "netlib", name + ".SIF"))


def random_lp(rng):
    """A x (=, <=, >=) b with b >= 0, 0 <= x <= u: infeasible, unbounded and rank-deficient cases among them."""
    n = rng.randint(2, 9)
    counts = [rng.randint(0, 3), rng.randint(0, 4), rng.randint(0, 3)]  # E, <=, >=
    if sum(counts) < 2:
        counts[1] += 2
    m = sum(counts)
    dense = [[rng.choice([0, 0, 1, 2, 3, -1, -2, 5]) for _ in range(n)] for _ in range(m)]
    b = [rng.randint(0, 12) for _ in range(m)]
    if rng.random() < 0.2 and m >= 2:  # a duplicated row: rank deficiency
        dense[1] = list(dense[0])
        b[1] = b[0]
    cost = [rng.randint(-5, 5) for _ in range(n)]
    upper = [rng.choice([None, None, rng.randint(1, 9)]) for _ in range(n)]
    columns = [[(i, dense[i][j]) for i in range(m) if dense[i][j] != 0] for j in range(n)]
    return counts, columns, b, cost, upper


def oracle(counts, columns, b, cost, upper):
    def data():
        return MatrixData(columns, b, [], counts[0], 0, counts[1], counts[2], [Variable(c, upper_bound=u) for c, u in zip(cost, upper)])
    if sum(counts) < 2:  # (the oracle's LU carry has no 1 x 1 update)
        return data(), solve_relaxation(data(), BasisInverseRows)
    try:
        return data(), solve_relaxation(data())
    except AssertionError:  # (the oracle's LU needs two rows left after removing redundant ones: its explicit carry takes one)
        return data(), solve_relaxation(data(), BasisInverseRows)


def oracle_objective(case):
    data, expected = oracle(*case)
    if not isinstance(expected, FiniteOptimum):
        return expected
    return sum((Fraction(case[3][j]) * v for j, v in data.reconstruct_solution(expected.solution)), Fraction(0))


def model_of_case(case):
    counts, columns, b, cost, upper = case
    kinds = ["Equal"] * counts[0] + ["Less"] * counts[1] + ["Greater"] * counts[2]
    return relp_amd.Model.from_general_form(columns, kinds, b, [(c, 0, u) for c, u in zip(cost, upper)])


def exact_or_none(many, i):
    try:
        return many.objective_exact(i)
    except relp_amd.RelpError:
        return None


def proof(many, certificates, i):
    c = certificates[i]
    return (c.certified, c.path, c.fallback_reason, c.digits_primal, c.digits_dual, exact_or_none(many, i))


# ---- 1. the smallest shapes ------------------------------------------------------------------------------------------------
def test_the_smallest_shapes_in_one_launch():
    big = 2147483647  # the first prime of the certificate: this 1 x 1 basis is singular modulo it
    cases = [
        ([0, 1, 0], [[(0, 1)]], [3], [-1], [None]),                                   # one row
        ([0, 1, 1], [[(0, 1), (1, 1)], [(0, 1), (1, -1)]], [4, 1], [-1, -2], [None, None]),  # two rows
        ([0, 1, 0], [[(0, big)]], [big], [-1], [None]),                               # min -x, 2147483647 x <= 2147483647
        ([2, 0, 0], [[(0, 1), (1, 1)], [(0, 1), (1, 1)]], [2, 2], [1, 2], [5, None]),  # a duplicated equality: an artificial stays basic
    ]
    many = relp_amd.Many([model_of_case(c) for c in cases])
    results = many.solve()
    certificates = many.certify(mode=0)
    for i, case in enumerate(cases):
        expected = oracle_objective(case)
        assert isinstance(expected, Fraction), i
        assert results[i].status == 0 and results[i].kind == relp_amd.FINITE_OPTIMUM, i
        assert certificates[i].certified == 1, (i, many.last_error())
        assert Fraction(many.objective_exact(i)) == expected, i
    assert Fraction(many.objective_exact(2)) == -1
    c = certificates[2]
    assert (c.path == 1 and c.fallback_reason == MANY_FALLBACK_NONE) or (c.path == 2 and c.fallback_reason == MANY_FALLBACK_SINGULAR_MOD_P), (c.path, c.fallback_reason)
    for i in (0, 1, 3):
        assert (certificates[i].path, certificates[i].fallback_reason) == (1, MANY_FALLBACK_NONE), i
    assert any(v < 0 for v in many.basis(3))  # an artificial stays basic: B of the last LP holds a unit column
    many.close()


# ---- 2. the 240 seeded LPs -------------------------------------------------------------------------------------------------
def test_random_lps_both_modes_agree_and_every_unrepaired_optimum_is_proved_in_the_batch():
    rng = random.Random(20261016)
    cases = [random_lp(rng) for _ in range(240)]
    many = relp_amd.Many([model_of_case(c) for c in cases])
    results = many.solve()
    serial = many.certify(mode=1)
    serial_exact = [exact_or_none(many, i) for i in range(len(cases))]
    assert many.certify_device_seconds == 0.0 and many.certify_wall_seconds > 0
    batched = many.certify(mode=0)
    batched_exact = [exact_or_none(many, i) for i in range(len(cases))]
    assert many.certify_device_seconds > 0 and many.certify_wall_seconds >= many.certify_device_seconds
    kinds = set()
    for i, (case, r) in enumerate(zip(cases, results)):
        expected = oracle_objective(case)
        assert r.status == 0, (i, many.last_error())
        a, b = serial[i], batched[i]
        assert a.certified == b.certified == 1, (i, r.kind, a.certified, b.certified, MANY_FALLBACK_NAMES[b.fallback_reason])
        assert serial_exact[i] == batched_exact[i] and batched_exact[i] is not None, i
        assert a.path == 2 and (a.digits_primal, a.digits_dual) == (0, 0), i
        if isinstance(expected, Fraction):
            assert r.kind == relp_amd.FINITE_OPTIMUM, i
            assert Fraction(batched_exact[i]) == expected, i
            if a.repair_pivots == 0:
                assert (b.path, b.fallback_reason) == (1, MANY_FALLBACK_NONE), (i, MANY_FALLBACK_NAMES[b.fallback_reason])
            if b.path == 1:
                assert 0 <= b.digits_primal <= 512 and 0 <= b.digits_dual <= 512 and b.repair_pivots == 0, i
        else:
            assert r.kind == (relp_amd.INFEASIBLE if isinstance(expected, Infeasible) else relp_amd.UNBOUNDED), i
            assert isinstance(expected, (Infeasible, Unbounded))
            assert (b.path, b.fallback_reason) == (2, MANY_FALLBACK_KIND), i
        kinds.add(r.kind)
    assert kinds == {relp_amd.FINITE_OPTIMUM, relp_amd.INFEASIBLE, relp_amd.UNBOUNDED}
    unrepaired = [i for i, r in enumerate(results) if r.kind == relp_amd.FINITE_OPTIMUM and serial[i].repair_pivots == 0]
    assert unrepaired and [i for i, c in enumerate(batched) if c.path == 1] == unrepaired
    many.close()


# ---- 3. golden LPs on both sides of the LDS boundary ---------------------------------------------------------------------------
def test_golden_lps_up_to_512_rows_are_proved_on_both_sides_of_the_lds_boundary():
    lps = golden_small()
    assert len(lps) >= 40
    edge = relp_amd.lib().relp_many_certify_lds_rows()
    assert edge == 198
    many = relp_amd.Many([relp_amd.Model(os.path.join(ROOT, f["file"])) for _, f in lps])
    results = many.solve()
    certificates = many.certify(mode=0)
    below, beyond = set(), set()
    for i, ((name, fixture), r, c) in enumerate(zip(lps, results, certificates)):
        assert r.status == 0 and r.kind == relp_amd.FINITE_OPTIMUM, (name, r.status, r.kind)
        assert c.certified == 1, (name, MANY_FALLBACK_NAMES[c.fallback_reason], many.last_error())
        assert many.objective_exact(i) == fixture["objective"], name
        assert c.path in (1, 2) and (c.path == 1) == (c.fallback_reason == MANY_FALLBACK_NONE), name
        if c.path == 1:
            (below if fixture["m"] <= edge else beyond).add(name)
    print("batched certificate, golden LPs: path 1 on %d of %d; fallbacks %s; largest K %d" % (
        len(below) + len(beyond), len(lps), dict(Counter(MANY_FALLBACK_NAMES[c.fallback_reason] for c in certificates if c.path == 2)),
        max(max(c.digits_primal, c.digits_dual) for c in certificates)))
    assert below and beyond, (sorted(below), sorted(beyond))
    many.close()


# ---- 4. independence -----------------------------------------------------------------------------------------------------
def test_a_proof_does_not_depend_on_the_other_lps_of_the_launch():
    alone = {}
    for name in ("AFIRO", "SC50A", "BLEND"):
        many = relp_amd.Many([netlib(name)])
        many.solve()
        alone[name] = proof(many, many.certify(mode=0), 0)
        assert alone[name][:3] == (1, 1, MANY_FALLBACK_NONE), (name, alone[name])
        many.close()
    names = ["AFIRO", "SC50A", "BLEND", "KB2", "SC105", "SHARE2B", "SCAGR7", "ADLITTLE"] * 8  # 64 LPs
    models = {name: netlib(name) for name in set(names)}
    seen = []
    for order in (names, names[::-1][3:] + names[::-1][:3]):
        many = relp_amd.Many([models[name] for name in order])
        many.solve()
        certificates = many.certify(mode=0)
        proofs = {}
        for i, name in enumerate(order):
            proofs.setdefault(name, set()).add(proof(many, certificates, i))
        assert all(len(p) == 1 for p in proofs.values()), {n: p for n, p in proofs.items() if len(p) > 1}
        for name in alone:
            assert proofs[name] == {alone[name]}, name
        seen.append(proofs)
        many.close()
    assert seen[0] == seen[1]


# ---- 5. state -------------------------------------------------------------------------------------------------------------
def test_certify_needs_a_solve_and_repeats_itself_and_leaves_a_stopped_lp_alone():
    names = ["AFIRO", "BLEND", "SC50A"]
    many = relp_amd.Many([netlib(n) for n in names], max_pivots=50)
    with pytest.raises(relp_amd.RelpError) as info:
        many.certify()
    assert info.value.status == ERR_STATE
    results = many.solve()
    assert results[1].kind == relp_amd.ITERATION_LIMIT and results[1].status == 0
    out = (ManyCertificate * 3)()
    out[0].struct_size = 24
    assert relp_amd.lib().relp_many_certify(many._h, 0, out, None, None) == ERR_ARGUMENT
    first = many.certify(mode=0)
    first_proofs = [proof(many, first, i) for i in range(3)]
    second = many.certify(mode=0)
    assert [proof(many, second, i) for i in range(3)] == first_proofs
    assert (first[1].certified, first[1].path, first[1].fallback_reason) == (0, 0, MANY_FALLBACK_NONE)
    assert exact_or_none(many, 1) is None
    golden = {n: json.load(open(os.path.join(GOLDEN_DIR, n + ".json")))["objective"] for n in names}
    for i in (0, 2):
        assert (first[i].certified, first[i].path) == (1, 1), names[i]
        assert many.objective_exact(i) == golden[names[i]], names[i]
    many.close()
