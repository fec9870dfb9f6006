"""Inputs and the exact reference of the dual simplex tests (tests/test_dual_host.py, tests/test_gpu_dual.py,
tests/test_gpu_dual_state.py): a parent LP of the ``less`` family of tests/sparse_lps.py, cuts appended to it that its optimal vertex
violates, and a textbook dual simplex over ``Fraction`` that walks the child from the parent's optimal basis.

``cut_case`` builds the parent; ``CutCase.child(basis, x)`` takes the parent's optimal basis and vertex from the caller -- the oracle's
on the CPU, the certified device solve's on the GPU -- and appends ``n_cuts`` ``"Less"`` rows, each over 1 to 3 structural variables
that are positive at the vertex (so basic in every optimal basis), coefficients in +-{1, 2, 3}, right-hand side
``max(0, floor(a x*) - 1)``: never negative, so standardisation flips no row and keeps their order, and a row is drawn again until
``a x* > rhs``.  The child's basis is the parent's plus the slack of each new row, every slack named by
``child.pivot_element_indices()``.

``DualReference`` is the rule of relp_amd/csrc/dual.hip in exact arithmetic: the leaving row is the most negative ``x_B`` (ties: lowest
basic column, then lowest row), the entering column the minimum of ``d_j / |alpha_pj|`` over ``alpha_pj < 0`` (ties: lowest column).
It records every pivot and how far each of the two choices was ahead of its runner-up, so that a test only compares the device with
it pivot for pivot where f64 cannot have chosen otherwise.
"""
from fractions import Fraction

import numpy as np

import relp_amd
import sparse_lps

MIXED = sparse_lps.MIXES["mixed"]
# (seed, n_cuts) of the pivot-for-pivot cases, chosen on the CPU so that the reference alone meets test_dual_host's conditions: the
# child's exact optimum is the oracle's, at least 8 dual pivots (2 at m = 5), every selection won by a relative margin >= 1e-6.
# Measured there: 4, 16 and 12 pivots, smallest margins 0.18, 0.015 and 0.0041 (seed 1064 has ties in the ratio test: margin 0).
WALK_CASES = {5: (2005, 3), 64: (2064, 4), 65: (1065, 3)}
MIN_PIVOTS = {5: 2, 64: 8, 65: 8}
MARGIN = 1e-6
# (seed, n_cuts) of the state cases: the seeds of sparse_lps' ``less mixed`` cases; 24 violated cuts leave 16 dual pivots to make
# (each pivot repairs the row it leaves at; test_gpu_dual_state asserts that at least 8 of the 16 asked for were made).
STATE_CASES = {513: (1000 + 513, 24), 1025: (2000 + 1025, 24), 2049: (1000 + 2049, 24)}


class CutCase:
    """The parent of a cut case: its model, its data as ``Fraction`` (structural columns only) and the generator of its children."""

    def __init__(self, model, seed, n_cuts):
        self.parent, self.seed, self.n_cuts = model, seed, n_cuts
        self.m, self.n_structural = model.nr_rows, model.nr_structural
        self.columns = [[(i, Fraction(num, den)) for i, num, den in model.column_exact(j)] for j in range(self.n_structural)]
        self.cost = [model.cost_exact(j) for j in range(self.n_structural)]
        self.b = model.right_hand_side_exact()
        self.slack_row = {column: row for row, column in model.pivot_element_indices()}
        assert len(self.slack_row) == self.m and model.nr_columns == self.n_structural + self.m  # the `less` family: a slack per row

    def cuts(self, x):
        """``[(variables, coefficients, rhs)]`` for the vertex ``x`` (structural column -> ``Fraction``)."""
        rng = np.random.RandomState(self.seed + 7919)
        positive = sorted(j for j, v in x.items() if j < self.n_structural and v > 0)
        assert positive, "the parent's optimum is the origin: no cut can bite"
        rows = []
        while len(rows) < self.n_cuts:
            k = min(int(rng.randint(1, 4)), len(positive))
            variables = sorted(int(j) for j in rng.choice(positive, size=k, replace=False))
            coefficients = [int(v) for v in rng.randint(1, 4, size=k) * rng.choice((-1, 1), size=k)]
            activity = sum(a * x[j] for j, a in zip(variables, coefficients))
            rhs = max(0, activity.numerator // activity.denominator - 1)
            if activity > rhs:
                rows.append((variables, coefficients, rhs))
        return rows

    def child(self, basis, x):
        """``(model, basis, cuts)`` of the child: ``basis`` is the parent's optimal basis (provider columns by row, as
        ``Solver.basis()`` gives it), ``x`` its vertex over the structural columns."""
        x = {int(j): Fraction(v) for j, v in x.items()}
        cuts = self.cuts(x)
        columns = [list(column) for column in self.columns]
        for k, (variables, coefficients, _) in enumerate(cuts):
            for j, a in zip(variables, coefficients):
                columns[j].append((self.m + k, a))
        b = list(self.b) + [rhs for _, _, rhs in cuts]
        model = relp_amd.Model.from_general_form(columns, ["Less"] * len(b), b, [(c, 0, None) for c in self.cost])
        return model, extended_basis(self, model, basis), cuts


def extended_basis(case, child, basis):
    """The parent's basis in the child's columns, plus the slack of every row the child has beyond the parent's."""
    slack_of_row = {row: column for row, column in child.pivot_element_indices()}
    for column in range(child.nr_structural, child.nr_columns):  # a "Greater" row starts from an artificial: its surplus column
        entries = child.column_exact(column)
        if len(entries) == 1 and entries[0][0] not in slack_of_row:
            slack_of_row[entries[0][0]] = column
    assert len(slack_of_row) == child.nr_rows, "a row of the child has no slack of its own"
    out = []
    for column in (int(c) for c in basis):
        assert column >= 0, "an artificial in the parent's optimal basis"
        out.append(column if column < case.n_structural else slack_of_row[case.slack_row[column]])
    out += [slack_of_row[row] for row in range(case.m, child.nr_rows)]
    assert len(set(out)) == child.nr_rows
    return out


def cut_case(m, lengths, seed, n_cuts, decimal=False):
    """The parent ``sparse_lps.less_lp(m, 2 m, lengths, seed)``; ``decimal``: every matrix value divided by 10, so that the data do not
    count as small integers and the Harris rule runs."""
    model = sparse_lps.less_lp(m, 2 * m, lengths, seed)
    if decimal:
        whole = CutCase(model, seed, n_cuts)
        columns = [[(i, v / 10) for i, v in column] for column in whole.columns]
        model = relp_amd.Model.from_general_form(columns, ["Less"] * m, whole.b, [(c, 0, None) for c in whole.cost])
    return CutCase(model, seed, n_cuts)


def solved_parent(case):
    """``(basis, vertex)`` of the parent's certified optimum on the device."""
    solver = relp_amd.Solver(certify=1).load_model(case.parent)
    try:
        result = solver.solve_relaxation()
        assert result.kind == relp_amd.FINITE_OPTIMUM and result.certified
        return solver.basis(), solver.solution_exact()
    finally:
        solver.close()


def cold_objective(model):
    """``(exact objective, result)`` of a cold certified solve on the device."""
    solver = relp_amd.Solver(certify=1).load_model(model)
    try:
        result = solver.solve_relaxation()
        assert result.kind == relp_amd.FINITE_OPTIMUM and result.certified
        return solver.objective_exact(), result
    finally:
        solver.close()


def infeasible_child(case, basis, x):
    """A child that no point satisfies: over the two lowest structural variables that are positive at ``x``, ``x_j + x_k <= 0`` and
    ``x_j + x_k >= 1``.  The ``"Greater"`` row has a positive right-hand side, so it is not flipped and the rows keep their order."""
    positive = sorted(j for j, v in x.items() if j < case.n_structural and v > 0)
    j, k = positive[:2]
    columns = [list(column) for column in case.columns]
    for variable in (j, k):
        columns[variable] += [(case.m, 1), (case.m + 1, 1)]
    b = list(case.b) + [0, 1]
    model = relp_amd.Model.from_general_form(columns, ["Less"] * (case.m + 1) + ["Greater"], b, [(c, 0, None) for c in case.cost])
    return model, extended_basis(case, model, basis)


class DualReference:
    """The textbook dual simplex over ``Fraction`` on the exact data of ``model`` (``column_exact``, ``cost_exact``,
    ``right_hand_side_exact``) from ``basis`` (provider columns by row).  ``run()`` walks to the end and returns the stop reason of
    ``Solver.iterate_dual``; ``pivots``: ``(q, p, leaving)`` in provider columns; ``margins``: per pivot the relative lead of the
    leaving row's infeasibility and of the entering column's ratio over their runners-up (1 where there is none)."""

    def __init__(self, model, basis):
        provider = sparse_lps.Provider(model)
        self.m, self.n = provider.m, provider.n
        self.columns, self.cost, self.b = provider.columns, provider.cost, provider.b
        self.basis = [int(c) for c in basis]
        self.inverse = self._invert()
        self.x = [sum((row[i] * self.b[i] for i in range(self.m) if row[i]), Fraction(0)) for row in self.inverse]
        self.pivots, self.margins = [], []
        self.smallest_infeasibility = None

    def _invert(self):
        m = self.m
        work = [[Fraction(0)] * (2 * m) for _ in range(m)]
        for k, j in enumerate(self.basis):
            for i, v in self.columns[j]:
                work[i][k] = v
        for i in range(m):
            work[i][m + i] = Fraction(1)
        for k in range(m):
            p = next(i for i in range(k, m) if work[i][k] != 0)
            work[k], work[p] = work[p], work[k]
            pivot = work[k][k]
            work[k] = [v / pivot if v else v for v in work[k]]
            for i in range(m):
                factor = work[i][k]
                if i != k and factor:
                    work[i] = [a - factor * c if c else a for a, c in zip(work[i], work[k])]
        return [row[m:] for row in work]

    def objective(self):
        return sum((self.cost[j] * v for j, v in zip(self.basis, self.x)), Fraction(0))

    def reduced_costs(self):
        m = self.m
        y = [sum((self.cost[self.basis[k]] * self.inverse[k][i] for k in range(m) if self.inverse[k][i]), Fraction(0)) for i in range(m)]
        return [self.cost[j] - sum((v * y[i] for i, v in self.columns[j]), Fraction(0)) for j in range(self.n)]

    def step(self):
        """One dual pivot; returns ``None`` after it, or the stop reason (``STOP_NO_ENTERING`` / ``STOP_UNBOUNDED``)."""
        m = self.m
        infeasible = sorted(((-self.x[i], -self.basis[i], -i) for i in range(m) if self.x[i] < 0), reverse=True)
        if not infeasible:
            return relp_amd.STOP_NO_ENTERING
        worst = min(key for key, _, _ in infeasible)
        self.smallest_infeasibility = worst if self.smallest_infeasibility is None else min(worst, self.smallest_infeasibility)
        p = -infeasible[0][2]
        lead_row = 1.0 if len(infeasible) == 1 else float((infeasible[0][0] - infeasible[1][0]) / infeasible[0][0])
        rho = self.inverse[p]
        basic = set(self.basis)
        d = self.reduced_costs()
        ratios = []
        for j in range(self.n):
            if j in basic:
                continue
            alpha = sum((v * rho[i] for i, v in self.columns[j] if rho[i]), Fraction(0))
            if alpha < 0:
                assert d[j] >= 0, "the reference lost dual feasibility"
                ratios.append((d[j] / -alpha, j))
        if not ratios:
            return relp_amd.STOP_UNBOUNDED
        ratios.sort()
        q = ratios[0][1]
        lead_column = 1.0 if len(ratios) == 1 else (0.0 if ratios[1][0] == 0 else float((ratios[1][0] - ratios[0][0]) / ratios[1][0]))
        alpha_q = [sum((self.inverse[k][i] * v for i, v in self.columns[q] if self.inverse[k][i]), Fraction(0)) for k in range(m)]
        pivot = alpha_q[p]
        theta = self.x[p] / pivot
        new_row = [v / pivot if v else v for v in rho]
        for k in range(m):
            if k != p and alpha_q[k]:
                factor = alpha_q[k]
                self.inverse[k] = [a - factor * c if c else a for a, c in zip(self.inverse[k], new_row)]
                self.x[k] -= theta * factor
        self.inverse[p] = new_row
        self.x[p] = theta
        self.pivots.append((q, p, self.basis[p]))
        self.margins.append((lead_row, lead_column))
        self.basis[p] = q
        return None

    def run(self, limit=10000):
        for _ in range(limit):
            reason = self.step()
            if reason is not None:
                return reason
        return relp_amd.STOP_BUDGET

    def smallest_margin(self):
        return min((min(pair) for pair in self.margins), default=1.0)


def assert_walk_conditions(reference, m, reason):
    """What a walk must be like for the pivot-for-pivot comparison to say something (the conditions the constants above were chosen
    for): it ends primal feasible, is long enough, and f64 cannot have chosen otherwise at any step -- every selection is won by a
    relative margin of ``MARGIN``, and no infeasibility is as small as the threshold the device ignores rows under."""
    assert reason == relp_amd.STOP_NO_ENTERING, reason
    assert len(reference.pivots) >= MIN_PIVOTS.get(m, 8), len(reference.pivots)
    assert reference.smallest_margin() >= MARGIN, reference.margins
    assert reference.smallest_infeasibility >= MARGIN, reference.smallest_infeasibility
