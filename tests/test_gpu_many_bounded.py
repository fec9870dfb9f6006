"""``relp_amd.Many(models, bounded=True)``: implicit upper bounds inside the one-workgroup-per-LP kernel.

A bounded LP must walk the pivot sequence of ``Solver(implicit_bounds=1)`` with the explicit carry.  On the interval LPs of
``test_gpu_many_paths`` (consecutive-ones rows, small integer data; complementing a column keeps the matrix totally unimodular)
f64 is exact on both paths whatever the order of a sum, so kernel and handle must agree BIT FOR BIT: kind, iteration counts,
bound flips, the basis in the reference's formulation, objective and solution -- also after every prefix of k iterations.  On
other data the results are checked against the exact oracle and the exact certificate."""
import json
import os
import random
from fractions import Fraction

import numpy as np
import pytest

import relp_amd
from relp_oracle import FiniteOptimum, Infeasible, MatrixData, Unbounded, Variable, solve_relaxation
from test_gpu_bounded import bounded_lp
from test_gpu_many_paths import LP, RULES, checkpoints, interval, transportation

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# constraint rows: 1, 2, the edges of the three LDS launch groups (48, 96, the bounded cut-off 138), 63-65, 255-257, 511, 512
ROWS = (1, 2, 3, 48, 49, 63, 64, 65, 96, 97, 138, 139, 255, 256, 257, 511, 512)
BOUNDED_LDS_ROWS, PLAIN_LDS_ROWS = 138, 139


def standard_form_rows(r):
    """The largest m for which ``interval(m, ...)`` has r constraint rows (it adds u = m // 4 bounds beyond two rows)."""
    return max(m for m in range(r, 2 * r + 3) if m - (0 if m <= 2 else m // 4) == r)


def boxes():
    """Hand-made LPs of one and two constraint rows with a box on every variable (one of zero width), interval columns."""
    one = LP("box-1-row", [[(0, 1)], [(0, 1)], [(0, 1)], [(0, 1)]], ["Less"], [4],
             [(-2, 0, 1), (-1, 0, 2), (-1, 0, 3), (-3, 0, 0)], relp_amd.FINITE_OPTIMUM)
    two = LP("box-2-rows", [[(0, 1)], [(0, 1), (1, 1)], [(1, 1)], [(0, 1), (1, 1)], [(1, 1)]], ["Equal", "Greater"], [3, 2],
             [(1, 0, 2), (-2, 0, 1), (2, 0, 4), (-1, 0, 0), (-1, 0, 1)], relp_amd.FINITE_OPTIMUM)
    return [one, two]


def bounded_set():
    lps = boxes()
    others = ("unbounded", "infeasible")
    for k, r in enumerate(ROWS):
        m = standard_form_rows(r)
        plants = ["feasible"] if r >= 3 else [("feasible", "unbounded")[r - 1]]
        if r >= 3:
            plants.append(others[k % 2])
        for plant in plants:
            lp = interval(m, k, plant)
            assert lp.model.nr_constraints == r, (lp, lp.model.nr_constraints)
            lps.append(lp)
    return lps


_SET = None


def the_set():
    global _SET
    if _SET is None:
        _SET = bounded_set()
    return _SET


def has_bounds(model):
    return model.nr_rows > model.nr_constraints


def device_rows(model):
    return model.nr_constraints if has_bounds(model) else model.nr_rows


def handle_options(**extra):
    return dict(carry=relp_amd.api.CARRY_EXPLICIT, crash=0, implicit_bounds=1, **extra)


def many_options(**extra):
    return dict(carry=relp_amd.api.CARRY_EXPLICIT, crash=0, implicit_bounds=0, **extra)


def solver_run(lp, **options):
    solver = relp_amd.Solver(**handle_options(**options)).load_model(lp.model)
    r = solver.solve_relaxation()
    out = {"kind": r.kind, "pivots": (r.pivots_phase_one, r.pivots_phase_two), "flips": solver.bound_flips(),
           "objective": np.float64(r.objective).tobytes(), "basis": tuple(int(v) for v in solver.basis()),
           "solution": solver.solution().tobytes()}
    solver.close()
    return out


def many_view(many, r, i):
    return {"kind": r.kind, "pivots": (r.pivots_phase_one, r.pivots_phase_two), "flips": many.bound_flips(i),
            "objective": np.float64(r.objective).tobytes(), "basis": tuple(int(v) for v in many.basis(i)),
            "solution": many.solution(i).tobytes()}


def signature(many, r, i):
    return (r.status, r.kind, r.inverse_in_lds, r.pivots_phase_one, r.pivots_phase_two, many.bound_flips(i),
            np.float64(r.objective).tobytes(), tuple(int(v) for v in many.basis(i)), many.solution(i).tobytes())


def at_upper(model, basis):
    """Bounded columns that sit at their upper bound in a basis of the reference's formulation: basic on their own bound row."""
    return {b for b in basis[model.nr_constraints:] if 0 <= b < model.nr_columns - (model.nr_rows - model.nr_constraints)}


def leaves_at_an_upper_bound(lp, rule, total):
    """Whether some iteration of the solve takes a basic variable out of the basis AT its upper bound: seen between the bases
    after k and k + 1 iterations (one launch per k)."""
    previous = None
    for k in range(1, total):
        many = relp_amd.Many([lp.model], bounded=True, max_pivots=k, **many_options(**RULES[rule]))
        many.solve()
        basis = [int(v) for v in many.basis(0)]
        many.close()
        if previous is not None:
            gone = set(previous[:lp.model.nr_constraints]) - set(basis[:lp.model.nr_constraints])
            if gone & (at_upper(lp.model, basis) - at_upper(lp.model, previous)):
                return True
        previous = basis
    return False


# ---- 1. bit for bit with the Solver on exact data ---------------------------------------------------------------------------
_SOLVER = {}


def solver_results(rule):
    if rule not in _SOLVER:
        _SOLVER[rule] = [solver_run(lp, **RULES[rule]) for lp in the_set()]
    return _SOLVER[rule]


def test_the_set_covers_the_sizes_the_verdicts_and_the_three_classes_of_bounded_steps(capsys):
    lps = the_set()
    assert {lp.model.nr_constraints for lp in lps} == set(ROWS)
    assert {lp.expect for lp in lps} == {relp_amd.FINITE_OPTIMUM, relp_amd.INFEASIBLE, relp_amd.UNBOUNDED}
    wide = [lp for lp in lps if lp.model.nr_constraints <= 512 < lp.model.nr_rows]
    assert wide, "an LP of at most 512 constraint rows and more than 512 standard-form rows"
    fixed = [lp for lp in lps if any(u == 0 for _, _, u in lp.variables)]
    assert fixed, "an LP with a zero-width variable"
    many = relp_amd.Many([lp.model for lp in lps], bounded=True, **many_options(**RULES["steepest-textbook"]))
    results = many.solve()
    flips = [many.bound_flips(i) for i in range(len(lps))]
    many.close()
    assert any(f > 0 for f in flips), "an LP with a bound flip"
    leaving = None
    for lp, r in zip(lps, results):  # the small ones first: one launch per iteration
        if has_bounds(lp.model) and lp.model.nr_constraints <= 65 and r.kind == relp_amd.FINITE_OPTIMUM:
            if leaves_at_an_upper_bound(lp, "steepest-textbook", r.pivots_phase_one + r.pivots_phase_two + 1):
                leaving = lp
                break
    with capsys.disabled():
        print("\nbounded set: %d LPs, %d with flips (%d flips), %d with a fixed variable, leaving at an upper bound: %s"
              % (len(lps), sum(f > 0 for f in flips), sum(flips), len(fixed), leaving))
    assert leaving is not None, "an LP in which a variable leaves the basis at its upper bound"


@pytest.mark.parametrize("tier", ["lds", "global"])
@pytest.mark.parametrize("rule", list(RULES))
def test_final_result_is_the_bounded_solvers_bit_for_bit(rule, tier):
    lps = the_set()
    expected = solver_results(rule)
    switches = relp_amd.api.SW_MANY_GLOBAL_TIER if tier == "global" else 0
    many = relp_amd.Many([lp.model for lp in lps], bounded=True, **many_options(switches=switches, **RULES[rule]))
    results = many.solve()
    for i, (lp, r, want) in enumerate(zip(lps, results, expected)):
        assert many.basis(i).shape == (lp.model.nr_rows,), lp
        assert r.status == 0, (lp, many.last_error())
        assert r.kind == lp.expect, (lp, r.kind)
        cut_off = BOUNDED_LDS_ROWS if has_bounds(lp.model) else PLAIN_LDS_ROWS
        assert r.inverse_in_lds == (1 if tier == "lds" and device_rows(lp.model) <= cut_off else 0), lp
        got = many_view(many, r, i)
        for key in ("kind", "pivots", "flips", "basis", "solution"):
            assert got[key] == want[key], (lp, key, got[key] if key != "basis" else "", want[key] if key != "basis" else "")
        if r.kind == relp_amd.FINITE_OPTIMUM:
            assert got["objective"] == want["objective"], (lp, r.objective)
        assert r.max_residual == 0.0, (lp, r.max_residual)
    many.close()


# ---- 2. the path at checkpoints ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", ["steepest-textbook", "dantzig-textbook"])
def test_counts_flips_and_basis_after_k_iterations_are_the_solvers(rule, capsys):
    lps = [lp for lp in the_set() if lp.expect == relp_amd.FINITE_OPTIMUM]
    assert {lp.model.nr_constraints for lp in lps} >= set(ROWS) - {2}
    full = relp_amd.Many([lp.model for lp in lps], bounded=True, **many_options(**RULES[rule]))
    finals = full.solve()
    full.close()
    wanted = {}
    for idx, r in enumerate(finals):
        assert r.status == 0 and r.kind == relp_amd.FINITE_OPTIMUM, lps[idx]
        for k in checkpoints(r.pivots_phase_one, r.pivots_phase_one + r.pivots_phase_two):
            wanted.setdefault(k, []).append(idx)
    checked = 0
    for k, members in sorted(wanted.items()):
        many = relp_amd.Many([lps[i].model for i in members], bounded=True, max_pivots=k, **many_options(**RULES[rule]))
        results = many.solve()
        for slot, i in enumerate(members):
            lp = lps[i]
            solver = relp_amd.Solver(max_pivots=k, **handle_options(**RULES[rule])).load_model(lp.model)
            s = solver.solve_relaxation()
            r = results[slot]
            assert r.status == 0 and r.kind == s.kind == relp_amd.ITERATION_LIMIT, (lp, k, r.kind, s.kind)
            assert (r.pivots_phase_one, r.pivots_phase_two) == (s.pivots_phase_one, s.pivots_phase_two), (lp, k)
            assert r.pivots_phase_one + r.pivots_phase_two >= k, (lp, k)
            assert many.bound_flips(slot) == solver.bound_flips(), (lp, k)
            assert tuple(many.basis(slot)) == tuple(solver.basis()), (lp, k)
            solver.close()
            checked += 1
        many.close()
    with capsys.disabled():
        print("\n%s: %d checkpoints over %d bounded LPs" % (rule, checked, len(lps)))


# ---- 3. against the exact oracle --------------------------------------------------------------------------------------------
def test_random_bounded_lps_in_one_launch_match_the_oracle_exactly():
    cases = []
    for seed in range(100):
        rng = random.Random(5000 + seed)
        n, counts, columns, b, ranges, cost, upper = bounded_lp(rng)
        if seed >= 80:  # variables fixed at zero: never priced, resolved at the end
            upper = [0 if rng.random() < 0.35 else u for u in upper]
        data = MatrixData(columns, b, ranges, counts[0], counts[1], counts[2], counts[3],
                          [Variable(c, upper_bound=u) for c, u in zip(cost, upper)])
        try:
            expected = solve_relaxation(data)
        except AssertionError:
            continue  # the reference's LU cannot factor a 1 x 1 basis
        kinds = ["Equal"] * counts[0] + [("Range", r) for r in ranges] + ["Less"] * counts[2] + ["Greater"] * counts[3]
        model = relp_amd.Model.from_general_form(columns, kinds, b, [(c, 0, u) for c, u in zip(cost, upper)])
        assert (model.nr_rows, model.nr_columns, model.nr_constraints) == (data.nr_rows(), data.nr_columns(), sum(counts)), seed
        cases.append((seed, model, data, expected, cost, upper))
    assert len(cases) >= 90, len(cases)
    many = relp_amd.Many([c[1] for c in cases], bounded=True, certify=1)
    results = many.solve()
    for i, ((seed, model, data, expected, cost, upper), r) in enumerate(zip(cases, results)):
        assert r.status == 0, (seed, many.last_error())
        if isinstance(expected, Infeasible):
            assert r.kind == relp_amd.INFEASIBLE, seed
        elif isinstance(expected, Unbounded):
            assert r.kind == relp_amd.UNBOUNDED, seed
        else:
            assert isinstance(expected, FiniteOptimum)
            assert r.kind == relp_amd.FINITE_OPTIMUM, seed
            objective = sum((Fraction(cost[j]) * v for j, v in data.reconstruct_solution(expected.solution)), Fraction(0))
            assert abs(r.objective - float(objective)) <= 1e-9 * max(1.0, abs(float(objective))), seed
            assert r.certified == 1, (seed, many.last_error())
            assert Fraction(many.objective_exact(i)) == objective, seed
            x = many.solution(i)
            assert abs(float(np.dot(x, cost)) - float(objective)) <= 1e-8 * max(1.0, abs(float(objective))), seed
            for j, u in enumerate(upper):
                assert x[j] >= -1e-9 and (u is None or x[j] <= u + 1e-9), (seed, j)
    many.close()


# ---- 4. Netlib ---------------------------------------------------------------------------------------------------------------
NETLIB = ["BOEING1", "BOEING2", "BORE3D", "CAPRI", "ETAMACRO", "FINNIS", "KB2", "RECIPELP", "STAIR", "STANDATA", "STANDMPS",
          "VTP-BASE", "GROW7"]


def test_netlib_lps_with_bounds_in_one_bounded_launch(capsys):
    with open(os.path.join(ROOT, "tests", "golden", "netlib_expected.json")) as handle:
        expected = json.load(handle)
    models = [relp_amd.Model(os.path.join(ROOT, "data", "netlib", name + ".SIF")) for name in NETLIB]
    many = relp_amd.Many(models, bounded=True, certify=1)
    results = many.solve()
    lines = []
    for i, (name, model, r) in enumerate(zip(NETLIB, models, results)):
        lines.append("%-9s rows %3d -> %3d  status %d kind %d certified %d lds %d  iterations %d + %d, flips %d, objective %.10g"
                     % (name, model.nr_rows, model.nr_constraints, r.status, r.kind, r.certified, r.inverse_in_lds, r.pivots_phase_one,
                        r.pivots_phase_two, many.bound_flips(i), r.objective))
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    for i, (name, r) in enumerate(zip(NETLIB, results)):
        assert r.status == 0, (name, many.last_error())
        assert r.kind == relp_amd.FINITE_OPTIMUM, (name, r.kind)
        golden_path = os.path.join(ROOT, "tests", "golden", name + ".json")
        if name == "GROW7":
            # (no golden file.  The entry of netlib_expected.json carries the magnitude: GROW7 is a minimisation whose published
            # optimum is -4.7787811815e7, and the reference, which ignores this LP, lists it without the sign.)
            assert not os.path.exists(golden_path)
            assert expected[name]["ignored"] and expected[name]["expected"] > 0
            assert abs(r.objective - -expected[name]["expected"]) <= expected[name]["tolerance"], (name, r.objective)
            assert r.certified == 1, (name, many.last_error())
            assert abs(float(Fraction(many.objective_exact(i))) - -expected[name]["expected"]) <= expected[name]["tolerance"], name
            continue
        with open(golden_path) as handle:
            golden = json.load(handle)
        assert r.certified == 1, (name, many.last_error())
        assert Fraction(many.objective_exact(i)) == Fraction(golden["objective"]), name
    assert results[NETLIB.index("RECIPELP")].inverse_in_lds == 1 and results[NETLIB.index("KB2")].inverse_in_lds == 1
    many.close()


# ---- 5. launch composition ---------------------------------------------------------------------------------------------------
def test_a_result_does_not_depend_on_the_launch_and_a_bound_free_lp_runs_the_plain_kernel():
    bounded = [lp for lp in the_set() if has_bounds(lp.model) and lp.model.nr_constraints in (1, 2, 3, 48, 64, 97, 138, 139, 256, 512)]
    free = [transportation(63, 120, 3), transportation(64, 200, 4), transportation(140, 300, 8), interval(2, 1, "unbounded")]
    assert all(not has_bounds(lp.model) for lp in free) and len(bounded) >= 10
    options = many_options(**RULES["steepest-textbook"])
    alone = {}
    for lp in bounded + free:
        many = relp_amd.Many([lp.model], bounded=True, **options)
        alone[lp.label] = signature(many, many.solve()[0], 0)
        many.close()
    for lp in free:  # the same as without the mode: it ran the plain instantiation
        many = relp_amd.Many([lp.model], **options)
        assert signature(many, many.solve()[0], 0) == alone[lp.label], lp
        many.close()
    rng = random.Random(20)
    mixed = bounded + free + rng.sample(bounded, 4) + rng.sample(free, 2)
    rng.shuffle(mixed)
    many = relp_amd.Many([lp.model for lp in mixed], bounded=True, **options)
    first = many.solve()
    first_signatures = [signature(many, r, i) for i, r in enumerate(first)]
    for lp, got in zip(mixed, first_signatures):
        assert got == alone[lp.label], lp
    second = many.solve()  # from the start again: flipped, pos and b' are reset
    assert [signature(many, r, i) for i, r in enumerate(second)] == first_signatures
    many.close()
