"""``relp_many`` pivot for pivot against the ``Solver``, at every tier and launch-bucket edge.

On totally unimodular integer data every quantity both paths compute is an integer of modest size: B^-1 has entries in
{0, +-1} (Gauss-Jordan with +-1 pivots stays there), x_B, -pi and the steepest-edge weights are integers, and every ratio or
pricing key is a correctly rounded quotient of two exact integers.  f64 is then exact on both paths whatever the summation
order, so the kernel and the handle must agree BIT FOR BIT: kind, pivot counts, basis, objective and solution, and the basis
after every prefix of k pivots (``max_pivots = k``).  A wrong tie-break, a wrong weight update, a wrong index, leading dimension
or slab offset makes them part ways (or leaves a nonzero residual before a re-inversion) even where both still reach an optimum.

On real-valued data (section 4 of the tests) the f64 paths are not exact; there the results are checked against independent
references: the exact certificate of a separate launch and HiGHS (scipy) on the general form.
"""
import random
from fractions import Fraction

import numpy as np
import pytest

import relp_amd
from relp_oracle import BasisInverseRows, FiniteOptimum, LUDecomposition, MatrixData, SteepestDescentAlongObjective, Variable, solve_relaxation
from relp_oracle.solve import Infeasible, Unbounded
from test_gpu_ties import Trace, transportation as tied_transportation

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 139, 140, 255, 256, 257, 511, 512)  # standard-form rows
LDS_ROWS = 139


def bucket(m):
    """The launch group of an LP of m rows (many_host_lp): LDS tier m <= 48, <= 96, <= 139, then the global tier."""
    return 0 if m <= 48 else 1 if m <= 96 else 2 if m <= LDS_ROWS else 3


# ---- generators of exact-arithmetic LPs -------------------------------------------------------------------------------------
class LP:
    """A general-form LP, the model built from it and what it is meant to be."""

    def __init__(self, label, columns, kinds, b, variables, expect=None):
        self.label, self.columns, self.kinds, self.b, self.variables, self.expect = label, columns, kinds, b, variables, expect
        self.model = relp_amd.Model.from_general_form(columns, kinds, b, variables)
        self.m = self.model.nr_rows

    def __repr__(self):
        return self.label


def transportation(m, arcs, seed):
    """s sources, t sinks (s + t = m), `arcs` arcs: a spanning tree (source i - sink i - source i+1 ..., extra sinks on
    source j mod s) keeps the graph connected, random arcs fill up; a random integer flow on them sets supplies and demands
    (feasible by construction), costs from {1, 2, 3}.  Connected: exactly one redundant row, left to the zero-level drive-out."""
    rng = random.Random(1000 * m + seed)
    s = m // 2
    t = m - s
    tree = [(i, i) for i in range(s)] + [(i + 1, i) for i in range(s - 1)] + [(j % s, j) for j in range(s, t)]
    edges = set(tree)
    assert len(edges) == m - 1 <= arcs <= s * t
    while len(edges) < arcs:
        edges.add((rng.randrange(s), rng.randrange(t)))
    edges = sorted(edges)
    flow = {e: rng.choice([0, 0, 1, 2, 3]) for e in edges}
    for e in tree:  # every node carries flow: phase one has work to do
        flow[e] = max(flow[e], 1)
    supply, demand = [0] * s, [0] * t
    for (i, j), f in flow.items():
        supply[i] += f
        demand[j] += f
    columns = [[(i, 1), (s + j, 1)] for i, j in edges]
    variables = [(rng.choice([1, 2, 3]), 0, None) for _ in edges]
    lp = LP("transport-m%d-n%d" % (m, m + arcs), columns, ["Equal"] * m, supply + demand, variables, relp_amd.FINITE_OPTIMUM)
    lp.n = m + arcs  # every row is an equality: an artificial each, then the arcs
    return lp


def interval(m, seed, plant):
    """A consecutive-ones (interval) matrix over r rows, Less / Greater / Equal, plus u finite upper bounds (m = r + u
    standard-form rows; the bound rows keep the matrix TU).  Costs from {-2, -1, 1}, small integer b from a planted point.
    `plant`: "feasible" (every column with a negative cost is bounded), "infeasible" (a Greater row i+1 whose columns all
    cover the Less row i, with b_{i+1} = b_i + 1), or "unbounded" (a cost -1 column without an upper bound on one Greater row)."""
    rng = random.Random(7000 * m + seed)
    u = 0 if m <= 2 else m // 4
    r = m - u
    n = max(2, r + r // 2 + (1 if plant == "unbounded" else 0))
    kinds = ["Equal"] + [rng.choice(["Less", "Less", "Greater", "Equal"]) for _ in range(r - 1)]
    spans = []
    i = 0
    while i < r:  # a tiling first: every row is covered
        length = rng.randint(1, 3)
        spans.append((i, min(r, i + length) - 1))
        i += length
    while len(spans) < n:
        lo = rng.randrange(r)
        spans.append((lo, min(r - 1, lo + rng.randint(0, 5))))
    spans = spans[:n] if len(spans) > n else spans
    n = len(spans)
    cost = [rng.choice([-2, -1, 1]) for _ in range(n)]
    x0 = [rng.choice([0, 1, 1, 2]) for _ in range(n)]
    x0[0] = max(x0[0], 1)  # row 0 (Equal) has a positive right-hand side: phase one pivots
    if plant == "infeasible":
        assert r >= 3
        k = rng.randrange(1, r - 1)
        kinds[k], kinds[k + 1] = "Less", "Greater"
        spans = [(k, hi) if lo == k + 1 else (lo, hi) for lo, hi in spans]
    if plant == "unbounded":
        k = rng.randrange(1, r)
        kinds[k] = "Greater"
        spans[-1] = (k, k)
        cost[-1] = -1
    activity = [sum(x0[j] for j, (lo, hi) in enumerate(spans) if lo <= i <= hi) for i in range(r)]
    b = []
    for i in range(r):
        if kinds[i] == "Equal":
            b.append(activity[i])
        elif kinds[i] == "Less":
            b.append(activity[i] + rng.choice([0, 0, 1, 2]))
        else:
            b.append(max(0, activity[i] - rng.choice([0, 0, 1, 2])))
    if plant == "infeasible":
        b[k + 1] = b[k] + 1
    bounded_by_rows = [any(kinds[i] != "Greater" for i in range(lo, hi + 1)) for lo, hi in spans]
    candidates = [j for j in range(n) if not (plant == "unbounded" and j == n - 1)]
    rng.shuffle(candidates)
    upper = [None] * n
    for j in candidates[:u]:
        upper[j] = x0[j] + rng.choice([0, 1, 2])
    assert sum(v is not None for v in upper) == u
    if plant != "unbounded":  # no improving ray: a column on Greater rows only, without a bound, gets a positive cost
        for j in range(n):
            if upper[j] is None and not bounded_by_rows[j]:
                cost[j] = 1
    columns = [[(i, 1) for i in range(lo, hi + 1)] for lo, hi in spans]
    expect = {"feasible": relp_amd.FINITE_OPTIMUM, "infeasible": relp_amd.INFEASIBLE, "unbounded": relp_amd.UNBOUNDED}[plant]
    lp = LP("interval-m%d-%s" % (m, plant), columns, kinds, b, [(c, 0, v) for c, v in zip(cost, upper)], expect)
    return lp


# the columns of the transportation LPs: below 512, exactly 512 and 513 device columns (the pricing loop's stride), beyond 1024
TRANSPORT_ARCS = {2: 1, 63: 120, 64: 200, 65: 447, 127: 300, 128: 385, 129: 384, 139: 400, 140: 300, 255: 257, 256: 257,
                  257: 600, 511: 700, 512: 700}


def tu_set():
    lps = []
    for k, m in enumerate(SIZES):
        if m in TRANSPORT_ARCS:
            lps.append(transportation(m, TRANSPORT_ARCS[m], k))
        plant = "feasible" if m < 3 and k % 3 == 1 else ("feasible", "unbounded", "infeasible")[k % 3]
        if m == 2:
            plant = "unbounded"
        lps.append(interval(m, k, plant))
    return lps


_TU = None


def tu_lps():
    global _TU
    if _TU is None:
        _TU = tu_set()
    return _TU


def exact_options(**extra):
    """What both paths run with on the TU data: the explicit carry, no crash, no implicit bounds."""
    return dict(carry=relp_amd.api.CARRY_EXPLICIT, crash=0, implicit_bounds=0, **extra)


def solver_run(lp, **options):
    solver = relp_amd.Solver(**exact_options(**options)).load_model(lp.model)
    r = solver.solve_relaxation()
    out = {"m": solver.m, "n": solver.n, "kind": r.kind, "pivots": (r.pivots_phase_one, r.pivots_phase_two),
           "objective": np.float64(r.objective).tobytes(), "basis": tuple(int(v) for v in solver.basis()),
           "solution": solver.solution().tobytes(), "ratio_rule": solver.record()["ratio_rule"]}
    solver.close()
    return out


def many_view(many, r, i):
    return {"kind": r.kind, "pivots": (r.pivots_phase_one, r.pivots_phase_two), "objective": np.float64(r.objective).tobytes(),
            "basis": tuple(int(v) for v in many.basis(i)), "solution": many.solution(i).tobytes()}


def signature(many, r, i):
    return (r.status, r.kind, r.pivots_phase_one, r.pivots_phase_two, np.float64(r.objective).tobytes(), tuple(int(v) for v in many.basis(i)),
            many.solution(i).tobytes())


RULES = {
    "steepest-auto": dict(pivot_rule=relp_amd.STEEPEST_EDGE, ratio_rule=relp_amd.api.RATIO_AUTO),
    "steepest-textbook": dict(pivot_rule=relp_amd.STEEPEST_EDGE, ratio_rule=relp_amd.api.RATIO_TEXTBOOK),
    "dantzig-textbook": dict(pivot_rule=relp_amd.DANTZIG, ratio_rule=relp_amd.api.RATIO_TEXTBOOK),
}


def test_the_tu_set_covers_every_size_bucket_and_column_stride(capsys):
    """The generators hit what the issue of these tests asks for: every m of the sweep in standard form, n below 512, at 512 and
    513 and beyond 1024 device columns, at least two LPs per launch bucket, and all three verdicts planted."""
    lps = tu_lps()
    assert sorted({lp.m for lp in lps}) == sorted(SIZES)
    per_bucket = [sum(bucket(lp.m) == b for lp in lps) for b in range(4)]
    assert min(per_bucket) >= 2, per_bucket
    columns = {lp.n for lp in lps if hasattr(lp, "n")}
    assert {512, 513} <= columns and min(columns) < 512 and max(columns) > 1024, sorted(columns)
    assert {lp.expect for lp in lps} == {relp_amd.FINITE_OPTIMUM, relp_amd.INFEASIBLE, relp_amd.UNBOUNDED}
    with capsys.disabled():
        print("\nTU set: " + ", ".join("%s(bucket %d)" % (lp.label, bucket(lp.m)) for lp in lps))


# ---- 2. the final result is the Solver's, bit for bit ------------------------------------------------------------------
_SOLVER = {}


def solver_results(rule):
    if rule not in _SOLVER:
        _SOLVER[rule] = [solver_run(lp, **RULES[rule]) for lp in tu_lps()]
    return _SOLVER[rule]


@pytest.mark.parametrize("tier", ["lds", "global"])
@pytest.mark.parametrize("rule", list(RULES))
def test_final_result_is_the_solvers_bit_for_bit(rule, tier):
    lps = tu_lps()
    expected = solver_results(rule)
    # "global": every LP of m <= 139 forced to the global tier, next to the ones that are there anyway
    switches = relp_amd.api.SW_MANY_GLOBAL_TIER if tier == "global" else 0
    many = relp_amd.Many([lp.model for lp in lps], **exact_options(switches=switches, **RULES[rule]))
    results = many.solve()
    for i, (lp, r, want) in enumerate(zip(lps, results, expected)):
        assert want["m"] == lp.m and many.basis(i).shape == (lp.m,), lp
        if hasattr(lp, "n"):
            assert want["n"] == lp.n, lp
        assert r.status == 0, (lp, many.last_error())
        assert r.kind == lp.expect, (lp, r.kind)
        assert r.inverse_in_lds == (1 if tier == "lds" and lp.m <= LDS_ROWS else 0), lp
        got = many_view(many, r, i)
        for key in ("kind", "pivots", "basis", "solution"):
            assert got[key] == want[key], (lp, key, got[key] if key != "basis" else "", want[key] if key != "basis" else "")
        if r.kind == relp_amd.FINITE_OPTIMUM:
            assert got["objective"] == want["objective"], (lp, r.objective)
        assert r.max_residual == 0.0, (lp, r.max_residual)
        assert r.reinversions >= 1, lp
        if rule == "steepest-auto":
            assert want["ratio_rule"] == "textbook", lp
    if rule == "steepest-auto":  # AUTO resolves to the textbook rule on every LP of the launch, as on the handle
        textbook = relp_amd.Many([lp.model for lp in lps], **exact_options(switches=switches, **RULES["steepest-textbook"]))
        again = textbook.solve()
        assert [signature(textbook, r, i) for i, r in enumerate(again)] == [signature(many, r, i) for i, r in enumerate(results)]
        textbook.close()
    many.close()


# ---- 3. the path itself, at checkpoints ----------------------------------------------------------------------------------
def checkpoints(p1, total):
    """k in {1, 2, last of phase one, first of phase two, total - 1, a few in between} (p1: every pivot of phase one)."""
    ks = {1, 2, p1, p1 + 1, total - 1, total // 3, (2 * total) // 3, (p1 + total) // 2}
    return sorted(k for k in ks if 1 <= k < total)


def one_per_size():
    seen, out = set(), []
    for lp in tu_lps():
        if lp.m not in seen and lp.expect == relp_amd.FINITE_OPTIMUM:
            seen.add(lp.m)
            out.append(lp)
    return out


@pytest.mark.parametrize("rule", ["steepest-textbook", "dantzig-textbook"])
def test_the_basis_after_k_pivots_is_the_solvers(rule, capsys):
    lps = one_per_size()
    assert {lp.m for lp in lps} == set(SIZES)
    full = relp_amd.Many([lp.model for lp in lps], **exact_options(**RULES[rule]))
    finals = full.solve()
    full.close()
    wanted = {}  # k -> LPs checked at k
    for idx, r in enumerate(finals):
        assert r.status == 0 and r.kind == relp_amd.FINITE_OPTIMUM, lps[idx]
        for k in checkpoints(r.pivots_phase_one, r.pivots_phase_one + r.pivots_phase_two):
            wanted.setdefault(k, []).append(idx)
    checked = 0
    for k, members in sorted(wanted.items()):
        many = relp_amd.Many([lps[i].model for i in members], max_pivots=k, **exact_options(**RULES[rule]))
        results = many.solve()
        for slot, i in enumerate(members):
            lp = lps[i]
            solver = relp_amd.Solver(max_pivots=k, **exact_options(**RULES[rule])).load_model(lp.model)
            s = solver.solve_relaxation()
            r = results[slot]
            assert r.status == 0 and r.kind == s.kind == relp_amd.ITERATION_LIMIT, (lp, k, r.kind, s.kind)
            assert (r.pivots_phase_one, r.pivots_phase_two) == (s.pivots_phase_one, s.pivots_phase_two), (lp, k)
            assert r.pivots_phase_one + r.pivots_phase_two >= k, (lp, k)
            assert tuple(many.basis(slot)) == tuple(solver.basis()), (lp, k)
            solver.close()
            checked += 1
        many.close()
    with capsys.disabled():
        print("\n%s: %d checkpoints over %d LPs (m = %s)" % (rule, checked, len(lps), ", ".join(str(lp.m) for lp in lps)))


def initial_basis(model):
    """The starting basis as Solver::upload and many_host_lp build it, provider encoding: the reference's initial pivots, an
    artificial (-1 - k, k in row order) on every other row."""
    pivots = dict(model.pivot_element_indices())
    out, k = [], 0
    for row in range(model.nr_rows):
        if row in pivots:
            out.append(pivots[row])
        else:
            out.append(-1 - k)
            k += 1
    return out, k


def replay(start, n_art, pivots):
    """Bases after each prefix of an oracle trace ((phase, q, p, leaving) with phase-two columns not counting artificials)."""
    basis = list(start)
    out = [tuple(basis)]
    for phase, q, p, _ in pivots:
        device = q + (n_art if phase == 2 else 0)
        basis[p] = device - n_art if device >= n_art else -1 - device
        out.append(tuple(basis))
    return out


def small_oracle_lps():
    """The m <= 12 generators of test_gpu_ties: tied transportation LPs (compared through phase one: the reference then removes
    the redundant row) and 0/1 inequality LPs with independent rows (compared through both phases)."""
    out = []
    for seed in range(8):
        rng = random.Random(77 + seed)
        sources, sinks = rng.randint(3, 6), rng.randint(3, 7)
        columns, b, cost = tied_transportation(rng, sources, sinks, seed % 2 == 0)
        m = sources + sinks
        data = MatrixData(columns, b, [], m, 0, 0, 0, [Variable(c) for c in cost])
        trace = Trace()
        assert isinstance(solve_relaxation(data, BasisInverseRows, SteepestDescentAlongObjective, trace=trace), FiniteOptimum)
        model = relp_amd.Model.from_general_form(columns, ["Equal"] * m, b, [(c, 0, None) for c in cost])
        out.append(("tied-transport-%d" % seed, model, [t for t in trace.pivots if t[0] == 1]))
    for seed in range(6):
        rng = random.Random(500 + seed)
        m, n = rng.randint(4, 8), rng.randint(5, 10)
        dense = [[rng.choice([0, 0, 1, 1, 1]) for _ in range(n)] for _ in range(m)]
        for i in range(m):
            if not any(dense[i]):
                dense[i][rng.randrange(n)] = 1
        columns = [[(i, dense[i][j]) for i in range(m) if dense[i][j]] for j in range(n)]
        n_ge = rng.randint(1, 2)
        b = [rng.choice([1, 2, 2]) for _ in range(m)]
        cost = [rng.choice([-1, -1, -2, 1]) for _ in range(n)]
        data = MatrixData(columns, b, [], 0, 0, m - n_ge, n_ge, [Variable(c) for c in cost])
        trace = Trace()
        expected = solve_relaxation(data, LUDecomposition, SteepestDescentAlongObjective, trace=trace)
        pivots = [t for t in trace.pivots if t[0] == 1] if isinstance(expected, Infeasible) else list(trace.pivots)
        model = relp_amd.Model.from_general_form(columns, ["Less"] * (m - n_ge) + ["Greater"] * n_ge, b, [(c, 0, None) for c in cost])
        out.append(("tied-inequality-%d" % seed, model, pivots))
    return out


def test_the_basis_after_k_pivots_is_the_exact_oracles():
    lps = small_oracle_lps()
    expected = []
    for name, model, pivots in lps:
        start, n_art = initial_basis(model)
        expected.append(replay(start, n_art, pivots))
    longest = max(len(pivots) for _, _, pivots in lps)
    assert longest >= 5
    compared = 0
    options = exact_options(**RULES["steepest-textbook"])
    for k in range(1, longest + 1):
        members = [i for i, (_, _, pivots) in enumerate(lps) if len(pivots) >= k]
        many = relp_amd.Many([lps[i][1] for i in members], max_pivots=k, **options)
        results = many.solve()
        for slot, i in enumerate(members):
            r = results[slot]
            assert r.status == 0, (lps[i][0], k, many.last_error())
            done = r.pivots_phase_one + r.pivots_phase_two
            # k pivots, unless a zero-level drive-out (uncapped, as on the handle) ran past k at the end of phase one
            assert done >= k, (lps[i][0], k, done)
            if done < len(expected[i]):
                assert tuple(many.basis(slot)) == expected[i][done], (lps[i][0], k, done)
                compared += 1
        many.close()
    assert compared >= sum(len(p) for _, _, p in lps) // 2


# ---- 4. real-valued data, uncertified, against independent references ----------------------------------------------------
def fraction(rng, low, high, max_den=97):
    den = rng.randint(1, max_den)
    return Fraction(rng.randint(int(low * den), int(high * den)), den)


def real_lp(m, seed, kind):
    """A random sparse general-form LP with coefficients num/den (den <= 97) whose standard form has m rows.
    feasible: a planted point strictly inside every box, b from it; infeasible: two rows with the same coefficients, one <= beta,
    one >= beta + 1; unbounded: one variable without an upper bound, negative cost, on Greater rows with positive and on Less
    rows with negative coefficients only.  m = constraint rows + boxed variables."""
    rng = random.Random(31 * m + seed)
    if m <= 2:
        v, boxed = 2, 0
    else:
        v = max(2, m // 3)
        boxed = v - (1 if kind == "unbounded" else 0)
    r = m - boxed
    assert r >= 1
    ray = v - 1 if kind == "unbounded" else None
    # (bounds and the planted point in tenths: b = A x0 keeps denominators a 128-bit standard form can hold)
    lower = [Fraction(rng.randint(-20, 10), 10) for _ in range(v)]
    upper = [lower[j] + Fraction(rng.randint(10, 40), 10) if (boxed and j != ray) else None for j in range(v)]
    x0 = [lower[j] + Fraction(rng.randint(1, 9), 10) for j in range(v)]
    rows = [dict() for _ in range(r)]
    kinds = [rng.choice(["Equal", "Less", "Less", "Greater"]) for _ in range(r)]
    if boxed == 0:  # no boxes (m <= 2): row 0 is a budget row over every variable, positive coefficients
        kinds[0] = "Less"
        for j in range(v):
            rows[0][j] = fraction(rng, 1, 3) or Fraction(1)
    for j in range(v):
        for i in rng.sample(range(r), min(r, rng.randint(1, 3))):
            if boxed == 0 and i == 0:
                continue
            value = fraction(rng, -3, 3)
            if value != 0:
                rows[i][j] = value
    for i in range(r):
        if not rows[i]:
            rows[i][rng.randrange(v)] = fraction(rng, 1, 3) or Fraction(1)
    if ray is not None:  # the ray: only on rows that stay satisfied along +e_ray
        for i in range(r):
            if ray in rows[i]:
                if kinds[i] == "Equal" or (boxed == 0 and i == 0):
                    del rows[i][ray]
                elif kinds[i] == "Less":
                    rows[i][ray] = -abs(rows[i][ray])
                else:
                    rows[i][ray] = abs(rows[i][ray])
        if not any(ray in row for row in rows):
            i = rng.randrange(r)
            kinds[i] = "Greater" if kinds[i] == "Equal" else kinds[i]
            rows[i][ray] = abs(fraction(rng, 1, 3)) or Fraction(1)
            if kinds[i] == "Less":
                rows[i][ray] = -rows[i][ray]
    for i in range(r):
        if not rows[i]:
            rows[i][rng.choice([j for j in range(v) if j != ray])] = Fraction(1)
    b = []
    for i in range(r):
        act = sum(a * x0[j] for j, a in rows[i].items())
        gap = Fraction(rng.randint(1, 20), 10)
        b.append(act if kinds[i] == "Equal" else act + gap if kinds[i] == "Less" else act - gap)
    if kind == "infeasible":
        assert r >= 2
        i, k = 0, 1 if r > 1 else 0
        rows[k] = dict(rows[i])
        kinds[i], kinds[k] = "Less", "Greater"
        b[k] = b[i] + 1
    # (costs over denominators <= 16: the fixed cost sum c_j l_j has their least common multiple as its denominator)
    cost = [Fraction(rng.randint(-48, 48), rng.randint(1, 16)) for _ in range(v)]
    if ray is not None:
        cost[ray] = -abs(cost[ray]) - 1
    columns = [sorted((i, rows[i][j]) for i in range(r) if j in rows[i]) for j in range(v)]
    variables = [(cost[j], lower[j], upper[j]) for j in range(v)]
    expect = {"feasible": relp_amd.FINITE_OPTIMUM, "infeasible": relp_amd.INFEASIBLE, "unbounded": relp_amd.UNBOUNDED}[kind]
    lp = LP("real-m%d-%s" % (m, kind), columns, kinds, b, variables, expect)
    lp.x0 = x0
    return lp


_REAL = None


def real_lps():
    global _REAL
    if _REAL is None:
        _REAL = []
        for k, m in enumerate(SIZES):
            for kind in ("feasible", "infeasible", "unbounded"):
                if kind == "infeasible" and m < 2:
                    continue
                _REAL.append(real_lp(m, k, kind))
    return _REAL


def highs(lp):
    from scipy.optimize import linprog
    v = len(lp.variables)
    a_ub, b_ub, a_eq, b_eq = [], [], [], []
    dense = np.zeros((len(lp.b), v))
    for j, column in enumerate(lp.columns):
        for i, value in column:
            dense[i, j] = float(value)
    for i, kind in enumerate(lp.kinds):
        if kind == "Equal":
            a_eq.append(dense[i])
            b_eq.append(float(lp.b[i]))
        elif kind == "Less":
            a_ub.append(dense[i])
            b_ub.append(float(lp.b[i]))
        else:
            a_ub.append(-dense[i])
            b_ub.append(-float(lp.b[i]))
    res = linprog([float(c) for c, _, _ in lp.variables], A_ub=np.array(a_ub) if a_ub else None, b_ub=b_ub or None,
                  A_eq=np.array(a_eq) if a_eq else None, b_eq=b_eq or None,
                  bounds=[(float(lo), None if hi is None else float(hi)) for _, lo, hi in lp.variables], method="highs")
    kind = {0: relp_amd.FINITE_OPTIMUM, 2: relp_amd.INFEASIBLE, 3: relp_amd.UNBOUNDED}.get(res.status)
    return kind, res.fun, dense


def test_real_valued_lps_uncertified_against_the_certificate_and_highs(capsys):
    lps = real_lps()
    for lp in lps:
        assert lp.m in SIZES, lp
    assert sorted({lp.m for lp in lps}) == sorted(SIZES)
    fast = relp_amd.Many([lp.model for lp in lps], certify=0)
    results = fast.solve()
    proved = relp_amd.Many([lp.model for lp in lps], certify=1)
    certified = proved.solve()
    optima = 0
    for i, (lp, r, c) in enumerate(zip(lps, results, certified)):
        assert r.status == 0, (lp, fast.last_error())
        assert r.certified == 0
        assert signature(fast, r, i) == signature(proved, c, i), lp
        kind, fun, dense = highs(lp)
        assert r.kind == lp.expect == kind, (lp, r.kind, kind)
        assert c.certified == 1, (lp, proved.last_error())
        # (a verdict after a pivot is drawn from a re-inverted basis; an LP whose starting basis is optimal needs none)
        assert r.reinversions >= min(1, r.pivots_phase_one + r.pivots_phase_two) and r.max_residual < 1e-9, (lp, r.reinversions, r.max_residual)
        if r.kind != relp_amd.FINITE_OPTIMUM:
            continue
        optima += 1
        exact = Fraction(proved.objective_exact(i))
        assert abs(r.objective - float(exact)) <= 1e-9 * max(1.0, abs(float(exact))), (lp, r.objective, exact)
        assert abs(fun - float(exact)) <= 1e-7 * max(1.0, abs(float(exact))), (lp, fun, exact)
        # the solution, in the general form's variables (every variable has a finite lower bound: the standard form shifts it)
        x = fast.solution(i) + np.array([float(lo) for _, lo, _ in lp.variables])
        assert x.shape == (len(lp.variables),)
        activity = dense @ x
        scale = 1.0 + np.abs(dense).sum(axis=1) * np.abs(x).max()
        for row, kind_i in enumerate(lp.kinds):
            tol = 1e-9 * scale[row]
            if kind_i == "Equal":
                assert abs(activity[row] - float(lp.b[row])) <= tol, (lp, row)
            elif kind_i == "Less":
                assert activity[row] <= float(lp.b[row]) + tol, (lp, row)
            else:
                assert activity[row] >= float(lp.b[row]) - tol, (lp, row)
        for j, (_, lo, hi) in enumerate(lp.variables):
            assert x[j] >= float(lo) - 1e-9 * max(1.0, abs(float(lo))), (lp, j)
            assert hi is None or x[j] <= float(hi) + 1e-9 * max(1.0, abs(float(hi))), (lp, j)
        objective = sum(float(cj) * x[j] for j, (cj, _, _) in enumerate(lp.variables))
        assert abs(objective - r.objective) <= 1e-9 * max(1.0, abs(r.objective)), (lp, objective, r.objective)
        assert abs(lp.model.fixed_cost() - sum(float(cj * lo) for cj, lo, _ in lp.variables)) <= 1e-12 * max(1.0, abs(lp.model.fixed_cost()))
        # the basis is optimal for a handle
        solver = relp_amd.Solver().load_model(lp.model)
        solver.set_basis(fast.basis(i))
        assert solver.iterate(1000) == (0, relp_amd.STOP_NO_ENTERING), lp
        solver.close()
    assert optima >= len(SIZES)
    fast.close()
    proved.close()
    with capsys.disabled():
        print("\nreal-valued: " + ", ".join("%s(bucket %d, %d pivots)" % (lp.label, bucket(lp.m), r.pivots_phase_one + r.pivots_phase_two)
                                          for lp, r in zip(lps, results)))


# ---- 5. launch composition and reuse --------------------------------------------------------------------------------------
def test_a_mixed_launch_gives_every_lp_its_result_alone():
    """Every LP of sections 2 and 4 in one launch, some twice at different positions (the global tier's slab shared by many LPs),
    under the default options: each LP's signature is its signature alone."""
    lps = tu_lps() + real_lps()
    rng = random.Random(4242)
    order = list(range(len(lps)))
    duplicates = [i for i in order if lps[i].m > LDS_ROWS][::3] + [i for i in order if lps[i].m <= LDS_ROWS][::5]
    order += duplicates
    rng.shuffle(order)
    assert sum(lps[i].m > LDS_ROWS for i in order) >= 4
    mixed = relp_amd.Many([lps[i].model for i in order])
    results = mixed.solve()
    first = {}
    for slot, i in enumerate(order):
        s = signature(mixed, results[slot], slot)
        assert results[slot].status == 0, lps[i]
        assert first.setdefault(i, s) == s, lps[i]  # the duplicates agree
    sample = []
    for b in range(4):
        members = [i for i in first if bucket(lps[i].m) == b]
        sample += members[:2] + [i for i in members if i in duplicates][:1] + members[-1:]
    sample = list(dict.fromkeys(sample))
    assert len(sample) >= 12 and {bucket(lps[i].m) for i in sample} == {0, 1, 2, 3}
    for i in sample:
        alone = relp_amd.Many([lps[i].model])
        again = alone.solve()
        assert signature(alone, again[0], 0) == first[i], lps[i]
        alone.close()
    mixed.close()


def test_a_second_solve_on_the_same_handle_gives_the_same_results():
    """gamma and the column positions live in global memory: the second launch must not see the first's."""
    lps = tu_lps() + real_lps()[::2]
    many = relp_amd.Many([lp.model for lp in lps])
    one = many.solve()
    first = [signature(many, r, i) for i, r in enumerate(one)]
    two = many.solve()
    assert [signature(many, r, i) for i, r in enumerate(two)] == first
    many.close()


def test_polish_period_does_not_change_the_path_on_exact_data():
    lps = tu_lps()
    signatures = {}
    for period in (1, 7, 0, 100000):
        many = relp_amd.Many([lp.model for lp in lps], polish_period=period, **exact_options(**RULES["steepest-textbook"]))
        results = many.solve()
        signatures[period] = [signature(many, r, i) for i, r in enumerate(results)]
        for lp, r in zip(lps, results):
            assert r.status == 0 and r.kind == lp.expect and r.max_residual == 0.0, (lp, period)
            if period == 1:  # every pivot is followed by a re-inversion, except that the zero-level pivots of the drive-out share one
                driven_out = initial_basis(lp.model)[1]
                assert r.reinversions >= r.pivots_phase_two + 1, (lp, r.reinversions)
                assert r.reinversions >= r.pivots_phase_one + r.pivots_phase_two - driven_out, (lp, r.reinversions)
        many.close()
    assert signatures[1] == signatures[7] == signatures[0] == signatures[100000]
