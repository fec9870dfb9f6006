"""Inputs and the exact reference of the bounded dual simplex tests (tests/test_dual_bounded_host.py, tests/test_gpu_dual_bounded.py):
a parent LP of the ``less`` family of tests/sparse_lps.py with an upper bound on every second structural variable, a child that a
branching step and a cut loop would make of it, and the dual simplex on implicit upper bounds over ``Fraction``, in the
representation the device holds.

The parent (``parent_data``): the generator of ``sparse_lps.less_lp`` restated (``mixed`` lengths, n = 2 m, small integers), then
``u_j = x0_j + r``, ``r`` in 0..3, on every even structural variable -- ``x0`` is the point the right-hand side was built around, so
the parent stays feasible -- and ``u = 0`` on the first even variable with ``x0_j = 0``.

The child (``BoundedCase.child``), from the parent's optimal basis and vertex: ``n_cuts`` cuts as ``dual_lps.CutCase.cuts`` makes
them; ``n_tight`` bounded variables that are positive at the vertex get ``u_j = ceil(x_j*) - 1`` (0 where ``x_j* <= 1``: the fixed
case); and the lowest un-bounded variable that is positive at the vertex gets such a bound too, which adds a bound row to the
formulation.  Its basis is the parent's, column by column, plus the slack of every row the formulation gained.

``BoundedDualReference`` is the rule of the BOUNDED kernels of relp_amd/csrc/dual.hip in exact arithmetic: every column is held as
``x_j`` or as ``u_j - x_j``, every non-basic column sits at 0 in that form, ``rhs`` carries the shift of the complemented columns.
It takes the basis of the formulation (bound rows included) and reduces it as ``Solver::place_basis`` does.
"""
import functools
from fractions import Fraction

import numpy as np

import relp_amd
import relp_oracle
from relp_oracle.solve import FiniteOptimum, solve_relaxation_full_basis
import dual_lps
import sparse_lps

MIXED = sparse_lps.MIXES["mixed"]
MARGIN = dual_lps.MARGIN
# (seed, n_cuts, n_tight) of the pivot-for-pivot cases, chosen on the CPU (``search`` below) so that the reference alone meets
# ``assert_walk_conditions``.
WALK_CASES = {5: (46, 3, 1), 64: (2000, 4, 6), 65: (1006, 4, 4)}
MIN_PIVOTS = {5: 2, 64: 8, 65: 8}
MIN_PER_SIDE = {5: 1, 64: 2, 65: 2}
STATE_CASE = (513, 1000 + 513, 24, 8)  # m, seed, cuts, tightened bounds


def parent_data(m, seed, lengths=MIXED, decimal=False, every=2):
    """``(columns, b, cost, upper)`` of the parent: ``sparse_lps.less_lp(m, 2 m, lengths, seed)`` drawn again, then the bounds
    (``upper[j]`` is ``None`` without one).  ``every``: a bound on every ``every``-th variable; ``decimal``: matrix values / 10."""
    n = 2 * m
    rng = np.random.RandomState(seed)
    columns, activity, priced = [], np.zeros(m, dtype=np.int64), np.zeros(n, dtype=np.int64)
    x0 = rng.randint(0, 4, size=n)
    y = -rng.randint(0, 3, size=m)
    for j in range(n):
        k = min(int(lengths[j % len(lengths)]), m)
        rows = np.sort(rng.choice(m, size=k, replace=False))
        values = rng.randint(1, 4, size=k) * rng.choice((-1, 1), size=k)
        columns.append([(int(i), int(v)) for i, v in zip(rows, values)])
        activity[rows] += values * x0[j]
        priced[j] = int((values * y[rows]).sum())
    b = activity + np.maximum(0, -activity) + rng.randint(0, 5, size=m)
    cost = priced + rng.randint(0, 4, size=n)
    assert (b >= 0).all() and (cost < 0).any()
    room = rng.randint(0, 4, size=n)
    upper = [int(x0[j] + room[j]) if j % every == 0 else None for j in range(n)]
    at_zero = next(j for j in range(0, n, every) if x0[j] == 0)
    upper[at_zero] = 0
    if decimal:
        columns = [[(i, Fraction(v, 10)) for i, v in column] for column in columns]
    return columns, [int(v) for v in b], [int(c) for c in cost], upper


class Formulation:
    """One LP of the family in three forms: the device's ``relp_amd.Model``, the oracle's ``MatrixData`` and the constraint data as
    ``Fraction``.  All rows are ``"Less"`` with a non-negative right-hand side: the columns are the structurals, a slack per
    constraint row, a slack per bound row; the rows are the constraint rows, then a bound row per bounded variable in variable order."""

    def __init__(self, columns, b, cost, upper, n_greater=0):
        self.m, self.ns, self.n_greater = len(b), len(columns), n_greater  # (the last ``n_greater`` rows are ``"Greater"``: a surplus column each)
        self.columns = [[(i, Fraction(v)) for i, v in column] for column in columns]
        self.b, self.cost, self.upper = [Fraction(v) for v in b], [Fraction(c) for c in cost], list(upper)
        self.bounded = [j for j in range(self.ns) if upper[j] is not None]
        self.bound_row = {j: self.m + k for k, j in enumerate(self.bounded)}
        self.bound_slack = {j: self.ns + self.m + k for k, j in enumerate(self.bounded)}
        self.rows, self.n_device = self.m + len(self.bounded), self.ns + self.m

    @functools.cached_property
    def model(self):
        kinds = ["Less"] * (self.m - self.n_greater) + ["Greater"] * self.n_greater
        return relp_amd.Model.from_general_form(self.columns, kinds, self.b, [(c, 0, u) for c, u in zip(self.cost, self.upper)])

    @functools.cached_property
    def oracle(self):
        variables = [relp_oracle.provider.Variable(c, upper_bound=u) for c, u in zip(self.cost, self.upper)]
        return relp_oracle.provider.MatrixData(self.columns, self.b, [], 0, 0, self.m - self.n_greater, self.n_greater, variables)

    def device_column(self, j):
        """Column j of the device LP (constraint rows only): a structural, or the slack (surplus: -1) of row ``j - ns``."""
        return self.columns[j] if j < self.ns else [(j - self.ns, Fraction(-1 if j - self.ns >= self.m - self.n_greater else 1))]

    def solve(self):
        """The oracle's cold solve from the slack basis: ``FiniteOptimum`` with ``objective``, ``basis`` (by formulation row) and ``solution``."""
        return solve_relaxation_full_basis(self.oracle)


class BoundedCase:
    """A parent and the generator of its children."""

    def __init__(self, m, seed, n_cuts, n_tight, decimal=False, every=2):
        self.m, self.seed, self.n_cuts, self.n_tight = m, seed, n_cuts, n_tight
        self.data = parent_data(m, seed, decimal=decimal, every=every)
        self.parent = Formulation(*self.data)

    def cuts(self, x):
        """As ``dual_lps.CutCase.cuts``: rows over 1 to 3 structural variables positive at ``x``, violated by it."""
        rng = np.random.RandomState(self.seed + 7919)
        positive = sorted(j for j, v in x.items() if j < self.parent.ns and v > 0)
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

    def branches(self, x):
        """``{variable: new upper bound}``: ``n_tight`` bounded variables positive at ``x`` and the lowest un-bounded one (if any), each
        with ``ceil(x_j) - 1``, which ``x`` violates."""
        parent = self.parent
        rng = np.random.RandomState(self.seed + 104729)
        positive = sorted(j for j, v in x.items() if j < parent.ns and v > 0)
        with_bound = [j for j in positive if parent.upper[j] is not None]
        assert len(with_bound) >= self.n_tight, "too few bounded variables are positive at the parent's vertex"
        chosen = sorted(int(j) for j in rng.choice(with_bound, size=self.n_tight, replace=False)) if self.n_tight else []
        chosen += [j for j in positive if parent.upper[j] is None][:1]  # (none where every variable has a bound already)
        return {j: -(-x[j].numerator // x[j].denominator) - 1 for j in chosen}

    def child(self, basis, x, branches=None):
        """``(formulation, basis, cuts, branches)`` of the child.  ``basis``: the parent's optimal basis by formulation row, ``x``: its
        vertex over the structural columns."""
        parent = self.parent
        x = {int(j): Fraction(v) for j, v in x.items()}
        cuts = self.cuts(x) if self.n_cuts else []
        branches = self.branches(x) if branches is None else branches
        columns = [list(column) for column in parent.columns]
        for k, (variables, coefficients, _) in enumerate(cuts):
            for j, a in zip(variables, coefficients):
                columns[j].append((parent.m + k, Fraction(a)))
        upper = list(parent.upper)
        for j, u in branches.items():
            assert u >= 0 and (upper[j] is None or u <= upper[j])
            upper[j] = u
        child = Formulation(columns, list(parent.b) + [rhs for _, _, rhs in cuts], parent.cost, upper)
        return child, extended_basis(parent, child, basis), cuts, branches


def extended_basis(parent, child, basis):
    """The parent's basis in the child's columns and rows, plus the slack of every row the child's formulation gained (cuts behind the
    constraint rows, the bound row of a variable that had no bound)."""
    slack_of = {parent.bound_slack[j]: child.bound_slack[j] for j in parent.bounded}  # (structurals and row slacks keep their numbers)
    def column(c):
        c = int(c)
        assert c >= 0, "an artificial in the parent's optimal basis"
        return slack_of.get(c, c)
    out = [column(basis[i]) for i in range(parent.m)] + [child.ns + i for i in range(parent.m, child.m)]
    for j in child.bounded:
        out.append(column(basis[parent.bound_row[j]]) if j in parent.bound_row else child.bound_slack[j])
    assert len(out) == child.rows and len(set(out)) == child.rows
    return out


class BoundedDualReference:
    """The dual simplex on implicit upper bounds over ``Fraction`` from ``basis`` (by formulation row).  State, in the held
    representation: ``basis`` / ``pos`` (device columns: -1 at 0, -2 complemented at 0, -3 fixed), ``flipped``, ``inverse`` of the
    matrix whose column i is ``sgn a_basis[i]``, ``x`` and ``xub`` per row, ``rhs``.  ``pivots``: ``(q, p, leaving, side)``;
    ``margins``: per pivot the relative lead of the leaving row's key and of the entering column's ratio over their runners-up."""

    def __init__(self, form, basis):
        self.form, self.m, self.n = form, form.m, form.n_device
        m, n = self.m, self.n
        self.ub = [form.upper[j] if j < form.ns else None for j in range(n)]
        self.cost = [form.cost[j] if j < form.ns else Fraction(0) for j in range(n)]
        row_of = {int(c): i for i, c in enumerate(basis)}
        assert len(row_of) == form.rows and min(row_of) >= 0
        self.flipped = [0] * n
        for j in form.bounded:  # the bound slack is not basic: the variable sits at its upper bound, non-basic and complemented
            if form.bound_slack[j] not in row_of:
                assert j in row_of, "neither a bounded variable nor its bound slack is basic"
                self.flipped[j] = 1
                del row_of[j]
        device_basic = [(c, row_of[c]) for c in range(n) if c in row_of]
        assert len(device_basic) == m, "the basis does not reduce to a basis of the constraint rows"
        self.basis, homeless = [-1] * m, []
        for c, wanted in device_basic:
            if wanted < m and self.basis[wanted] < 0:
                self.basis[wanted] = c
            else:
                homeless.append(c)
        for i in range(m):
            if self.basis[i] < 0:
                self.basis[i] = homeless.pop(0)
        self.pos = [-1] * n
        for j in range(n):
            if self.ub[j] == 0:
                self.flipped[j] = 0
            self.pos[j] = -3 if self.ub[j] == 0 else (-2 if self.flipped[j] else -1)
        for i, c in enumerate(self.basis):
            self.pos[c] = i
        self.rhs = list(form.b)
        for j in range(n):
            if self.flipped[j]:
                for i, v in form.device_column(j):
                    self.rhs[i] -= self.ub[j] * v
        self.xub = [self.ub[c] for c in self.basis]
        self.inverse = self._invert()
        self.x = [sum((row[i] * self.rhs[i] for i in range(m) if row[i]), Fraction(0)) for row in self.inverse]
        self.pivots, self.margins = [], []
        self.smallest_violation = None
        self.fixed_cost_ties = 0  # steps at which a fixed column had the relative cost 0 exactly (``formulation_basis`` reads its sign)

    def sgn(self, j):
        return -1 if self.flipped[j] else 1

    def _invert(self):
        m = self.m
        work = [[Fraction(0)] * (2 * m) for _ in range(m)]
        for k, j in enumerate(self.basis):
            for i, v in self.form.device_column(j):
                work[i][k] = self.sgn(j) * v
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
        held = sum((self.sgn(j) * self.cost[j] * v for j, v in zip(self.basis, self.x)), Fraction(0))
        return held + sum((self.ub[j] * self.cost[j] for j in range(self.n) if self.flipped[j]), Fraction(0))

    def pi(self):
        m = self.m
        return [sum((self.sgn(self.basis[k]) * self.cost[self.basis[k]] * self.inverse[k][i] for k in range(m) if self.inverse[k][i]), Fraction(0))
                for i in range(m)]

    def relative_costs(self):
        """``c_j - pi a_j`` of every device column, un-signed: what ``Solver.relative_costs`` returns."""
        y = self.pi()
        return [self.cost[j] - sum((v * y[i] for i, v in self.form.device_column(j)), Fraction(0)) for j in range(self.n)]

    def signed_costs(self):
        """``d_j = sgn_j (c_j - pi a_j)`` on the priced columns (pos -1, -2), ``None`` elsewhere."""
        return [self.sgn(j) * c if self.pos[j] in (-1, -2) else None for j, c in enumerate(self.relative_costs())]

    def weights(self):
        return [sum((v * v for v in row if v), Fraction(0)) for row in self.inverse]

    def violation(self, i):
        """``(v_i, side)``: +1 below 0, -1 above ``xub``."""
        below = -self.x[i]
        above = self.x[i] - self.xub[i] if self.xub[i] is not None else None
        return (above, -1) if above is not None and above > below else (below, 1)

    def key(self, i, v):
        return v

    def solution(self):
        """The structural variables' values."""
        out = {j: Fraction(self.ub[j]) for j in range(self.form.ns) if self.pos[j] == -2}
        for i, j in enumerate(self.basis):
            if j < self.form.ns:
                out[j] = self.ub[j] - self.x[i] if self.flipped[j] else self.x[i]
        return out

    def formulation_basis(self):
        """``Solver::get_basis``: on a bound row the variable itself where it sits at its upper bound, else the bound slack; a fixed
        column counts as at its upper bound where its relative cost is negative."""
        form, costs = self.form, None
        out = list(self.basis)
        for j in form.bounded:
            position = self.pos[j]
            if position == -3:
                costs = costs or self.relative_costs()
                if costs[j] == 0:
                    self.fixed_cost_ties += 1
                position = -2 if costs[j] < 0 else -1
            out.append(j if position == -2 else form.bound_slack[j])
        return out

    def step(self):
        """One dual pivot; returns ``None`` after it, or the stop reason (``STOP_NO_ENTERING`` / ``STOP_UNBOUNDED``)."""
        m, form = self.m, self.form
        rows = []
        for i in range(m):
            v, side = self.violation(i)
            if v > 0:
                rows.append((self.key(i, v), -self.basis[i], -i, v, side))
        if not rows:
            return relp_amd.STOP_NO_ENTERING
        rows.sort(reverse=True)
        worst = min(v for _, _, _, v, _ in rows)
        self.smallest_violation = worst if self.smallest_violation is None else min(worst, self.smallest_violation)
        p, side = -rows[0][2], rows[0][4]
        lead_row = 1.0 if len(rows) == 1 else float((rows[0][0] - rows[1][0]) / rows[0][0])
        rho = self.inverse[p]
        d = self.signed_costs()
        ratios = []
        for j in range(self.n):
            if d[j] is None:
                continue
            abar = side * self.sgn(j) * sum((v * rho[i] for i, v in form.device_column(j) if rho[i]), Fraction(0))
            if abar < 0:
                assert d[j] >= 0, "the reference lost dual feasibility"
                ratios.append((d[j] / -abar, j))
        if not ratios:
            return relp_amd.STOP_UNBOUNDED
        ratios.sort()
        q = ratios[0][1]
        lead_column = 1.0 if len(ratios) == 1 else (0.0 if ratios[1][0] == 0 else float((ratios[1][0] - ratios[0][0]) / ratios[1][0]))
        alpha_q = [self.sgn(q) * sum((self.inverse[k][i] * v for i, v in form.device_column(q) if self.inverse[k][i]), Fraction(0)) for k in range(m)]
        pivot = alpha_q[p]
        assert side * pivot < 0
        theta = (self.x[p] - (self.xub[p] if side < 0 else 0)) / pivot
        assert theta >= 0
        new_row = [v / pivot if v else v for v in rho]
        for k in range(m):
            if k != p and alpha_q[k]:
                factor = alpha_q[k]
                self.inverse[k] = [a - factor * c if c else a for a, c in zip(self.inverse[k], new_row)]
                self.x[k] -= theta * factor
        self.inverse[p] = new_row
        self.x[p] = theta
        leaving = self.basis[p]
        if side < 0:  # the leaving column stops at its upper bound: complemented from now on
            for i, v in form.device_column(leaving):
                self.rhs[i] -= self.xub[p] * self.sgn(leaving) * v
            self.flipped[leaving] ^= 1
        self.pos[leaving] = -3 if self.ub[leaving] == 0 else (-2 if self.flipped[leaving] else -1)
        self.xub[p] = self.ub[q]
        self.pos[q] = p
        self.basis[p] = q
        self.pivots.append((q, p, leaving, side))
        self.margins.append((lead_row, lead_column))
        return None

    def run(self, limit=10000):
        for _ in range(limit):
            reason = self.step()
            if reason is not None:
                return reason
        return relp_amd.STOP_BUDGET

    def smallest_margin(self):
        return min((min(pair) for pair in self.margins), default=1.0)

    def feasible(self):
        return all(0 <= v and (u is None or v <= u) for v, u in zip(self.x, self.xub))


class SteepestBoundedDualReference(BoundedDualReference):
    """... with the steepest-edge key of the leaving row, ``v_i^2 / beta_i``."""

    def key(self, i, v):
        return v * v / sum((a * a for a in self.inverse[i] if a), Fraction(0))


class HeldState:
    """What ``residual_checks.assert_residuals`` reads -- a handle and the provider of its model -- for the HELD representation of a
    handle on implicit bounds, where the exact state is out of reach (m = 513): the LP whose column j is ``sgn_j a_j`` with the cost
    ``sgn_j c_j`` and whose right-hand side is ``b - sum u_j a_j`` over the complemented columns; in it the device's inverse, x_B and
    ``-pi`` are those of a plain basis, its relative costs are ``sgn_j`` times what ``relative_costs`` returns, and its objective is
    the device's minus ``sum u_j c_j``.  Which columns are complemented: a non-basic one where ``basis()`` has the variable itself
    on its bound row; a basic one by the sign of ``(row k of the device's inverse) . a_basis[k]``, which is +-1 up to rounding (only
    that sign is taken from the device; the residuals then check the inverse against the signed columns, every entry).  ``basis()``
    has the device's basis by position in its first m entries."""

    def __init__(self, solver, form):
        self.solver, self.form = solver, form
        self.m, self.n, self.n_art = form.m, form.n_device, 0
        assert solver.n_art == 0
        full = [int(c) for c in solver.basis()]
        self.held_basis = full[:self.m]
        assert len(full) == form.rows and all(0 <= c < self.n for c in self.held_basis)
        sgn = [1] * self.n
        for j in form.bounded:
            if full[form.bound_row[j]] == j:
                sgn[j] = -1
        self.inverse = [solver.basis_inverse_row(k)[:self.m] for k in range(self.m)]
        for k, j in enumerate(self.held_basis):
            diagonal = sum(float(v) * self.inverse[k][i] for i, v in form.device_column(j))
            assert abs(abs(diagonal) - 1) < 0.5, ("position", k, diagonal)
            sgn[j] = 1 if diagonal > 0 else -1
            assert sgn[j] > 0 or (j < form.ns and form.upper[j] is not None), ("an un-bounded column is held complemented", j)
        self.sgn = sgn
        upper = [form.upper[j] if j < form.ns and form.upper[j] is not None else 0 for j in range(self.n)]
        # the provider of the held LP
        self.columns = [[(i, sgn[j] * v) for i, v in form.device_column(j)] for j in range(self.n)]
        self.cost = [sgn[j] * (form.cost[j] if j < form.ns else 0) for j in range(self.n)]
        self.b = list(form.b)
        self.constant = Fraction(0)
        for j in range(self.n):
            if sgn[j] < 0:
                self.constant += upper[j] * form.cost[j]
                for i, v in form.device_column(j):
                    self.b[i] -= upper[j] * v
        self.complemented_basic = sum(1 for j in self.held_basis if sgn[j] < 0)

    # the handle
    def basis(self):
        return np.array(self.held_basis, dtype=np.int32)

    def basis_inverse_row(self, k):
        return self.inverse[k]

    def b_held(self):
        return self.solver.b()[:self.m]

    def objective_function_value(self):
        return self.solver.objective_function_value() - float(self.constant)

    def relative_costs(self):
        return self.solver.relative_costs()[:self.n] * np.array(self.sgn, dtype=np.float64)

    def right_multiply_by_basis_inverse(self, rows, values):
        return self.solver.right_multiply_by_basis_inverse(rows, values)[:self.m]


def held_pair(solver, form):
    """``(handle, provider)`` for ``assert_residuals``: two views of one ``HeldState`` (a handle's ``b()`` is x_B, a provider's ``b`` the right-hand side)."""
    state = HeldState(solver, form)

    class Handle:
        m, n, n_art = state.m, state.n, 0
        basis, basis_inverse_row = state.basis, state.basis_inverse_row
        objective_function_value, relative_costs = state.objective_function_value, state.relative_costs
        right_multiply_by_basis_inverse = state.right_multiply_by_basis_inverse
        b = staticmethod(state.b_held)

    class Provider:
        m, columns, cost, b = state.m, state.columns, state.cost, state.b
    return Handle, Provider, state


def walk(reference, collect_bases=False):
    """Walks ``reference`` to its end and gathers what the conditions ask about: ``(reason, facts)``."""
    widths, complemented_entering, bases = [], 0, []
    while True:
        flipped_before = list(reference.flipped)
        reason = reference.step()
        if reason is not None:
            break
        q, _, leaving, _ = reference.pivots[-1]
        complemented_entering += flipped_before[q]
        widths.append(reference.ub[leaving])
        bases.append(reference.formulation_basis())
    sides = [side for _, _, _, side in reference.pivots]
    facts = {"pivots": len(reference.pivots), "upper": sides.count(-1), "lower": sides.count(1), "complemented_entering": complemented_entering,
             "width_zero_leaving": sum(1 for w in widths if w == 0), "margin": reference.smallest_margin(),
             "smallest_violation": reference.smallest_violation, "fixed_cost_ties": reference.fixed_cost_ties}
    return reason, facts, bases


def assert_walk_conditions(reference, m, reason, facts):
    """What a walk must be like for the pivot-for-pivot comparison to say something: it ends primal feasible, is long enough, leaves on
    both sides, enters a complemented column, and f64 cannot have chosen otherwise at any step."""
    assert reason == relp_amd.STOP_NO_ENTERING and reference.feasible(), reason
    assert facts["pivots"] >= MIN_PIVOTS.get(m, 8), facts
    assert facts["upper"] >= MIN_PER_SIDE.get(m, 2) and facts["lower"] >= MIN_PER_SIDE.get(m, 2), facts
    assert facts["complemented_entering"] >= 1, facts
    assert facts["margin"] >= MARGIN and facts["smallest_violation"] >= MARGIN, facts
    assert facts["fixed_cost_ties"] == 0, facts  # (the sign of a fixed column's relative cost decides its row of the formulation basis)


@functools.lru_cache(maxsize=None)
def built(m, seed, n_cuts, n_tight, decimal=False, every=2):
    """``(case, parent optimum, child formulation, child basis, cuts, branches)``, built once per process: the parent's optimal basis
    and vertex are the oracle's."""
    case = BoundedCase(m, seed, n_cuts, n_tight, decimal=decimal, every=every)
    optimum = case.parent.solve()
    assert isinstance(optimum, FiniteOptimum)
    vertex = {j: v for j, v in optimum.solution if j < case.parent.ns}
    child, basis, cuts, branches = case.child(optimum.basis, vertex)
    return case, optimum, child, basis, cuts, branches


def infeasible_child(m=64):
    """``(case, parent optimum, child, basis)``: the two lowest bounded variables that are positive at the parent's vertex are fixed at 0
    by the branch, and the row ``x_j + x_k >= 1`` (a positive right-hand side: not flipped, the rows keep their order) contradicts
    that.  The row's basic column is its surplus."""
    case, optimum, _, _, _, _ = built(m, WALK_CASES[m][0], 0, 0)
    parent = case.parent
    vertex = {j: v for j, v in optimum.solution if j < parent.ns}
    j, k = [v for v in sorted(vertex) if vertex[v] > 0 and parent.upper[v] is not None][:2]
    columns = [list(column) for column in parent.columns]
    upper = list(parent.upper)
    for variable in (j, k):
        columns[variable].append((parent.m, Fraction(1)))
        upper[variable] = 0
    child = Formulation(columns, list(parent.b) + [1], parent.cost, upper, n_greater=1)
    return case, optimum, child, extended_basis(parent, child, optimum.basis)


def walk_case(m):
    return built(m, *WALK_CASES[m])


def search(m, seeds, shapes):
    """The first ``(seed, n_cuts, n_tight)`` whose walk meets the conditions, and its facts (a tool for choosing ``WALK_CASES``)."""
    for seed in seeds:
        for n_cuts, n_tight in shapes:
            try:
                _, _, child, basis, _, _ = built(m, seed, n_cuts, n_tight)
                reference = BoundedDualReference(child, basis)
                if min(d for d in reference.signed_costs() if d is not None) < 0:
                    continue
                reason, facts, _ = walk(reference)
                assert_walk_conditions(reference, m, reason, facts)
                if reference.objective() != child.solve().objective:
                    continue
                return (seed, n_cuts, n_tight), facts
            except (AssertionError, StopIteration):
                continue
    return None, None
