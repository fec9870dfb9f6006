"""An independent check of the exact witnesses behind a certified result (``Solver.witness_exact``, ``Many.witness_exact``).

Rational arithmetic on the model's exact data (``Model.column_exact``, ``cost_exact``, ``right_hand_side_exact``,
``fixed_cost_exact``) and nothing else: no call into the solver or the certificate, so a verdict of this library can be verified
without trusting the code that produced it.  The LP is the standard form of the model: min c'x subject to A x = b, x >= 0 over the
provider columns (the structural columns, then the slack columns), ``model.nr_rows`` rows and ``model.nr_columns`` columns.

A witness is a dict index -> ``Fraction`` of its non-zero entries.  Each check returns ``None`` or raises ``WitnessError`` naming
the first violated condition and its row or column.
"""
from fractions import Fraction


class WitnessError(AssertionError):
    """A witness does not prove what it claims.  ``condition``: which one failed; ``where``: its row or column (or None)."""

    def __init__(self, condition, where=None, detail=""):
        place = "" if where is None else " at %s %d" % where
        super().__init__("%s violated%s%s" % (condition, place, ": " + detail if detail else ""))
        self.condition = condition
        self.where = where


class _Form:
    """A, b, c and the fixed cost of a model, read once through its exact accessors."""

    def __init__(self, model):
        self.m, self.n = model.nr_rows, model.nr_columns
        self.columns = [[(i, Fraction(num, den)) for i, num, den in model.column_exact(j)] for j in range(self.n)]
        self.cost = [model.cost_exact(j) for j in range(self.n)]
        self.b = model.right_hand_side_exact()
        self.fixed = model.fixed_cost_exact()

    def vector(self, values, size, what, kind):
        """The dense form of a sparse witness; its indices must lie in the index space."""
        out = [Fraction(0)] * size
        for index, value in values.items():
            if not 0 <= index < size:
                raise WitnessError("%s: index inside the LP" % what, (kind, index))
            out[index] = Fraction(value)
        return out

    def times(self, x):
        """A x, by row."""
        out = [Fraction(0)] * self.m
        for j, column in enumerate(self.columns):
            if x[j]:
                for i, a in column:
                    out[i] += a * x[j]
        return out

    def priced(self, y, j):
        """y'a_j."""
        return sum((y[i] * a for i, a in self.columns[j]), Fraction(0))

    def dot_cost(self, x):
        return sum((c * v for c, v in zip(self.cost, x)), Fraction(0))

    def dot_b(self, y):
        return sum((v * b for v, b in zip(y, self.b)), Fraction(0))

    def feasible(self, x, what):
        """x >= 0 and A x = b."""
        for j, v in enumerate(x):
            if v < 0:
                raise WitnessError("%s >= 0" % what, ("column", j), str(v))
        for i, (lhs, rhs) in enumerate(zip(self.times(x), self.b)):
            if lhs != rhs:
                raise WitnessError("A %s = b" % what, ("row", i), "%s != %s" % (lhs, rhs))


def check_optimum(model, x, y, objective):
    """x is feasible, y is dual feasible over EVERY provider column, and both have the value ``objective``: by weak duality x is
    optimal and ``objective`` is the optimum (fixed cost included)."""
    form = _Form(model)
    objective = Fraction(objective)
    xs = form.vector(x, form.n, "x", "column")
    ys = form.vector(y, form.m, "y", "row")
    form.feasible(xs, "x")
    for j in range(form.n):
        reduced = form.cost[j] - form.priced(ys, j)
        if reduced < 0:
            raise WitnessError("c_j - y'a_j >= 0", ("column", j), str(reduced))
    primal = form.dot_cost(xs) + form.fixed
    if primal != objective:
        raise WitnessError("c'x + fixed cost = objective", None, "%s != %s" % (primal, objective))
    dual = form.dot_b(ys) + form.fixed
    if dual != objective:
        raise WitnessError("y'b + fixed cost = objective", None, "%s != %s" % (dual, objective))


def check_infeasible(model, y, value):
    """Farkas: y'a_j <= 0 for every provider column and y'b = ``value`` > 0, so no x >= 0 has A x = b (y'A x <= 0 < y'b)."""
    form = _Form(model)
    value = Fraction(value)
    ys = form.vector(y, form.m, "y", "row")
    for j in range(form.n):
        priced = form.priced(ys, j)
        if priced > 0:
            raise WitnessError("y'a_j <= 0", ("column", j), str(priced))
    yb = form.dot_b(ys)
    if yb != value:
        raise WitnessError("y'b = value", None, "%s != %s" % (yb, value))
    if yb <= 0:
        raise WitnessError("y'b > 0", None, str(yb))


def check_dual_bound(model, y, value):
    """Weak duality without a primal point: y is dual feasible over EVERY provider column and y'b + fixed cost = ``value``, so no
    feasible x costs less than ``value`` (c'x >= y'A x = y'b).  The witness of a ``CUTOFF`` result of the dual simplex, and of its
    ``ITERATION_LIMIT`` under ``Solver.set_dual_cutoff``."""
    form = _Form(model)
    value = Fraction(value)
    ys = form.vector(y, form.m, "y", "row")
    for j in range(form.n):
        reduced = form.cost[j] - form.priced(ys, j)
        if reduced < 0:
            raise WitnessError("c_j - y'a_j >= 0", ("column", j), str(reduced))
    dual = form.dot_b(ys) + form.fixed
    if dual != value:
        raise WitnessError("y'b + fixed cost = value", None, "%s != %s" % (dual, value))


def check_unbounded(model, x, ray):
    """x is feasible and d = ``ray`` has d >= 0, A d = 0 and c'd < 0: x + t d is feasible for every t >= 0 and its cost falls
    without bound."""
    form = _Form(model)
    xs = form.vector(x, form.n, "x", "column")
    d = form.vector(ray, form.n, "ray", "column")
    form.feasible(xs, "x")
    for j, v in enumerate(d):
        if v < 0:
            raise WitnessError("ray >= 0", ("column", j), str(v))
    for i, lhs in enumerate(form.times(d)):
        if lhs != 0:
            raise WitnessError("A ray = 0", ("row", i), str(lhs))
    slope = form.dot_cost(d)
    if slope >= 0:
        raise WitnessError("c'ray < 0", None, str(slope))
