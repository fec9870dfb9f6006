"""``relp_many_*``: many small LPs solved in one launch, one workgroup per LP."""
import json
import os
import random
from fractions import Fraction

import numpy as np
import pytest

import relp_amd
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


def model_of(fixture):
    return relp_amd.Model(os.path.join(ROOT, fixture["file"]))


def netlib(name):
    return relp_amd.Model(os.path.join(ROOT, "data", "netlib", name + ".SIF"))


def signature(many, results, i):
    r = results[i]
    return (r.status, r.kind, r.pivots_phase_one, r.pivots_phase_two, np.float64(r.objective).tobytes(), tuple(many.basis(i)))


def test_golden_lps_up_to_512_rows_in_one_launch_are_certified_optima():
    lps = golden_small()
    assert len(lps) >= 40
    many = relp_amd.Many([model_of(f) for _, f in lps], certify=1)
    results = many.solve()
    assert many.kernel_seconds > 0
    tiers = set()
    for i, ((name, fixture), r) in enumerate(zip(lps, results)):
        assert r.status == 0 and r.kind == relp_amd.FINITE_OPTIMUM, (name, r.status, r.kind, many.last_error())
        assert r.certified == 1, (name, many.last_error())
        assert many.objective_exact(i) == fixture["objective"], name
        expected = float(Fraction(fixture["objective"]))
        assert abs(r.objective - expected) <= 1e-9 * max(1.0, abs(expected)), (name, r.objective, expected)
        assert r.inverse_in_lds == (1 if fixture["m"] <= 139 else 0), name
        assert r.reinversions >= 1 and r.max_residual < 1e-6
        tiers.add(r.inverse_in_lds)
    assert tiers == {0, 1}
    many.close()


# ---- seeded random LPs against the exact oracle --------------------------------------------------------------------------
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
    try:
        return data(), solve_relaxation(data())
    except AssertionError:  # (the oracle's LU needs two rows left after removing redundant ones: its explicit carry takes one)
        return data(), solve_relaxation(data(), BasisInverseRows)


def test_random_lps_in_one_launch_match_the_oracle():
    rng = random.Random(20261016)
    cases = [random_lp(rng) for _ in range(240)]
    models = []
    for counts, columns, b, cost, upper in cases:
        kinds = ["Equal"] * counts[0] + ["Less"] * counts[1] + ["Greater"] * counts[2]
        models.append(relp_amd.Model.from_general_form(columns, kinds, b, [(c, 0, u) for c, u in zip(cost, upper)]))
    many = relp_amd.Many(models, certify=1)
    results = many.solve()
    seen = set()
    for i, (case, r) in enumerate(zip(cases, results)):
        data, expected = oracle(*case)
        assert r.status == 0, (i, many.last_error())
        if isinstance(expected, Infeasible):
            assert r.kind == relp_amd.INFEASIBLE, i
        elif isinstance(expected, Unbounded):
            assert r.kind == relp_amd.UNBOUNDED, i
        else:
            assert isinstance(expected, FiniteOptimum)
            assert r.kind == relp_amd.FINITE_OPTIMUM, i
            cost = case[3]
            objective = sum((Fraction(cost[j]) * v for j, v in data.reconstruct_solution(expected.solution)), Fraction(0))
            assert Fraction(many.objective_exact(i)) == objective, i
            assert abs(r.objective - float(objective)) <= 1e-9 * max(1.0, abs(float(objective))), i
        assert r.certified == 1, (i, r.kind, many.last_error())
        seen.add(r.kind)
    assert seen == {relp_amd.FINITE_OPTIMUM, relp_amd.INFEASIBLE, relp_amd.UNBOUNDED}
    many.close()


# ---- independence and determinism --------------------------------------------------------------------------------------
def test_a_result_does_not_depend_on_the_other_lps_of_the_launch():
    names = ["AFIRO", "BLEND", "SC50A", "KB2", "SCAGR7", "BORE3D"]  # both tiers; BORE3D keeps zero-level artificials
    many = relp_amd.Many([netlib(n) for n in names])
    results = many.solve()
    mixed = [signature(many, results, i) for i in range(len(names))]
    many.close()
    reverse = relp_amd.Many([netlib(n) for n in reversed(names)])
    results = reverse.solve()
    reversed_signatures = [signature(reverse, results, i) for i in range(len(names))][::-1]
    reverse.close()
    assert reversed_signatures == mixed
    for i, name in enumerate(names):
        alone = relp_amd.Many([netlib(name)])
        results = alone.solve()
        assert signature(alone, results, 0) == mixed[i], name
        alone.close()
    assert all(s[1] == relp_amd.FINITE_OPTIMUM for s in mixed)


def test_a_thousand_copies_of_afiro_give_one_result():
    model = netlib("AFIRO")
    many = relp_amd.Many([model] * 1000)
    results = many.solve()
    first = signature(many, results, 0)
    assert first[1] == relp_amd.FINITE_OPTIMUM
    assert all(signature(many, results, i) == first for i in range(1000))
    assert abs(results[0].objective - float(Fraction(-406659, 875))) <= 1e-9 * 465
    many.close()


# ---- the basis is optimal for the existing path --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["AFIRO", "BLEND", "SC105", "E226"])
def test_the_returned_basis_is_optimal_for_a_solver_handle(name):
    path = os.path.join(ROOT, "data", "netlib", name + ".SIF")
    many = relp_amd.Many([relp_amd.Model(path)], certify=1)
    r = many.solve()[0]
    assert r.kind == relp_amd.FINITE_OPTIMUM and r.certified == 1
    basis = many.basis(0)
    solver = relp_amd.Solver(certify=1).load_mps(path)
    solver.set_basis(basis)
    done, reason = solver.iterate(1000)
    assert (done, reason) == (0, relp_amd.STOP_NO_ENTERING), name
    assert abs(solver.objective_function_value() + relp_amd.Model(path).fixed_cost() - r.objective) <= 1e-9 * max(1.0, abs(r.objective))
    solver.close()
    reference = relp_amd.Solver(certify=1).load_mps(path)
    assert reference.solve_relaxation().certified == 1
    assert reference.objective_exact() == many.objective_exact(0)
    x = many.solution(0)
    assert len(x) == relp_amd.Model(path).nr_structural
    reference.close()
    many.close()


# ---- the two tiers ------------------------------------------------------------------------------------------------------
def test_the_global_tier_gives_the_lds_tiers_certified_optima():
    names = ["AFIRO", "SC50A", "BLEND", "SHARE2B", "SC105"]
    lds = relp_amd.Many([netlib(n) for n in names], certify=1)
    forced = relp_amd.Many([netlib(n) for n in names], certify=1, switches=relp_amd.api.SW_MANY_GLOBAL_TIER)
    a, b = lds.solve(), forced.solve()
    for i, name in enumerate(names):
        assert a[i].inverse_in_lds == 1 and b[i].inverse_in_lds == 0, name
        assert a[i].certified == b[i].certified == 1, name
        assert lds.objective_exact(i) == forced.objective_exact(i), name
        assert (a[i].pivots_phase_one, a[i].pivots_phase_two) == (b[i].pivots_phase_one, b[i].pivots_phase_two), name
    lds.close()
    forced.close()


# ---- per-LP limits ------------------------------------------------------------------------------------------------------
def test_max_pivots_stops_only_the_lp_that_reaches_it():
    names = ["AFIRO", "BLEND", "SC50A"]
    free = relp_amd.Many([netlib(n) for n in names])
    unlimited = free.solve()
    assert unlimited[1].pivots_phase_one + unlimited[1].pivots_phase_two > 50
    assert all(r.pivots_phase_one + r.pivots_phase_two <= 50 for r in (unlimited[0], unlimited[2]))
    capped = relp_amd.Many([netlib(n) for n in names], max_pivots=50)
    limited = capped.solve()
    assert limited[1].kind == relp_amd.ITERATION_LIMIT and limited[1].status == 0
    assert limited[1].pivots_phase_one + limited[1].pivots_phase_two == 50
    for i in (0, 2):
        assert signature(capped, limited, i) == signature(free, unlimited, i), names[i]
    free.close()
    capped.close()


def test_dantzig_and_the_textbook_rule_reach_the_same_optima():
    names = ["AFIRO", "SC50A", "KB2", "SCAGR7"]
    golden = {n: json.load(open(os.path.join(GOLDEN_DIR, n + ".json")))["objective"] for n in names}
    for overrides in ({"pivot_rule": relp_amd.DANTZIG}, {"ratio_rule": relp_amd.api.RATIO_HARRIS}):
        many = relp_amd.Many([netlib(n) for n in names], certify=1, **overrides)
        for i, r in enumerate(many.solve()):
            assert r.kind == relp_amd.FINITE_OPTIMUM and r.certified == 1, (overrides, names[i])
            assert many.objective_exact(i) == golden[names[i]]
        many.close()
