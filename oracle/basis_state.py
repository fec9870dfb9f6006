"""The exact state of a simplex basis (oracle side; test infrastructure only -- nothing here imports ``relp_amd``).

Everything a handle holds after any number of pivots is a function of the current basis alone: the rows of ``B^-1``,
``x_B = B^-1 b``, the objective ``c_B' x_B``, the reduced costs ``c_j - c_B' B^-1 a_j`` and the steepest-edge weights
``gamma_j = 1 + |B^-1 a_j|^2`` (the recurrences that carry them are exact: pivot_rule.rs:243-296).  ``BasisState`` computes them
from the basis WITHOUT walking a pivot path, so that paths no step-by-step oracle can follow (batched launches, the deferred
product form, a polish inside the loop) are checked against the same truth.

Index spaces are those of the binding: a basis entry >= 0 is a provider column (for ``load_dense_le``: structurals, then the
slacks), ``-1 - k`` is artificial ``k``; every per-column result is indexed like ``Solver.relative_costs()`` -- the artificials
first, then the provider's columns.

``B^-1 = N / D`` comes from a fraction-free Gauss-Jordan elimination in Python integers (each step one rank-one update of a numpy
``object`` array; every division is exact).  Basic columns with a single entry -- slacks, artificials -- are eliminated by hand
first, so the elimination runs on the Schur block of the other columns only.  Each exact quantity ``q`` is returned as a pair of
f64 arrays ``hi = float(q)``, ``lo = float(q - hi)``; products with the columns of ``A`` are then formed in ``np.longdouble``
from ``hi + lo``.  Where ``longdouble`` is no wider than f64 (``EXTENDED`` false) the per-column quantities are exact integer dot
products instead, on the sample of columns that ``columns_to_check`` returns.

``BasisState`` holds dense (m, m) and (m, n) arrays: fine for the dense pipeline's few hundred rows.  ``SparseBasisState`` yields the
same numbers from the structure of that elimination alone -- the k x k Schur block and the sparse rows of the non-unit basic columns
-- for sparse LPs of thousands of rows (tests/test_gpu_sparse_state.py: 8193 rows, k = 100, well under a second and 22 MB).
"""
from fractions import Fraction
from math import gcd, lcm

import numpy as np

EXTENDED = np.finfo(np.longdouble).nmant > 52


def split(num, den):
    """``num / den`` (Python integers) as ``(hi, lo)``: the nearest f64 and the f64 nearest to what it leaves."""
    if num == 0:
        return 0.0, 0.0
    hi = num / den  # (int / int is correctly rounded)
    p, q = hi.as_integer_ratio()
    rest = num * q - p * den
    return hi, (rest / (den * q) if rest else 0.0)


def split_fraction(value):
    value = Fraction(value)
    return split(value.numerator, value.denominator)


def long_double(hi, lo):
    return np.asarray(hi, dtype=np.longdouble) + np.asarray(lo, dtype=np.longdouble)


class DenseLE:
    """The provider columns ``[A | I]`` of ``A x <= b`` as ``Solver.load_dense_le`` numbers them.  ``a``: (n, m) integers."""

    def __init__(self, a_columns):
        self.a = np.asarray(a_columns, dtype=np.int64)
        self.n, self.m = self.a.shape

    def __len__(self):
        return self.n + self.m

    def __getitem__(self, j):
        if j < self.n:
            return [(i, int(v)) for i, v in enumerate(self.a[j]) if v != 0]
        return [(j - self.n, 1)]

    def matrix(self):
        return np.concatenate([self.a.T, np.eye(self.m, dtype=np.int64)], axis=1)


def fraction_free_inverse(matrix):
    """``(N, D)`` with ``matrix^-1 = N / D``: Gauss-Jordan on ``[matrix | I]`` whose entries stay integers (after step k every entry
    is a minor of order k + 1, so the division by the previous pivot is exact).  ``matrix``: (s, s) ``object`` array of ints."""
    s = matrix.shape[0]
    if s == 0:
        return np.zeros((0, 0), dtype=object), 1
    work = np.concatenate([matrix.astype(object), np.array(np.eye(s, dtype=np.int64), dtype=object)], axis=1)
    previous = 1
    for k in range(s):
        p = next((i for i in range(k, s) if work[i, k] != 0), None)
        if p is None:
            raise ZeroDivisionError("singular basis")
        if p != k:
            work[[k, p]] = work[[p, k]]
        pivot = work[k, k]
        column = work[:, k].copy()
        column[k] = 0
        row = work[k, k:].copy()
        work[:, k:] = (work[:, k:] * pivot - np.outer(column, row)) // previous  # (columns before k are finished and not read again)
        work[k, k:] = row
        previous = pivot
    return work[:, s:], previous


_sparse_inverses = {}  # the components that ``sparse_inverse`` has inverted, by content: the bases of one walk share most of theirs
_SPARSE_INVERSES_KEPT = 1 << 20  # numerators (Python integers) kept at the most: beyond, the oldest results go first
_sparse_inverse_entries = [0]


def sparse_inverse(matrix):
    """``(N, D)`` with ``matrix^-1 = N / D`` and ``|D| = |det|``, as ``fraction_free_inverse`` returns them (the sign of D may differ, and N
    with it), for a SPARSE block: Gauss-Jordan on rows held as dicts of integers over one denominator per row (reduced by their gcd after
    every update), the pivot in the active column with the fewest active rows and there in the shortest row.  An arrow of 259 columns
    costs its 259^2 results, not 259^3 integer updates.  Results are kept by content."""
    s = matrix.shape[0]
    if s == 0:
        return np.zeros((0, 0), dtype=object), 1
    filled = [(int(i), int(j), int(matrix[i, j])) for i, j in zip(*np.nonzero(matrix != 0))]
    key = (s, tuple(filled))
    if key in _sparse_inverses:
        return _sparse_inverses[key]
    left, right, den = [{} for _ in range(s)], [{i: 1} for i in range(s)], [1] * s  # row r = (left[r] | right[r]) / den[r], integers
    in_column, count = [set() for _ in range(s)], [0] * s  # rows with an entry in the column; how many of them are active
    for i, j, v in filled:
        left[i][j] = v
        in_column[j].add(i)
        count[j] += 1
    active, active_columns, row_of, det = set(range(s)), set(range(s)), {}, Fraction(1)
    for _ in range(s):
        j = min(active_columns, key=lambda c: (count[c], c))
        if count[j] == 0:
            raise ZeroDivisionError("singular basis")
        i = min((r for r in in_column[j] if r in active), key=lambda r: (len(left[r]), r))
        pivot = left[i][j]
        det *= Fraction(pivot, den[i])
        den[i] = pivot  # the row over its pivot: (integers / den) / (pivot / den)
        for r in [r for r in in_column[j] if r != i]:
            factor = left[r][j]  # row r <- row r - (factor / den[r]) (row i / pivot) = (pivot row r - factor row i) / (den[r] pivot)
            row = {c: v * pivot for c, v in left[r].items()} if pivot != 1 else left[r]
            for c, v in left[i].items():
                had = c in row
                value = row.get(c, 0) - factor * v
                if value == 0:
                    if had:
                        del row[c]
                        in_column[c].discard(r)
                        count[c] -= r in active
                else:
                    row[c] = value
                    if not had:
                        in_column[c].add(r)
                        count[c] += r in active
            target = {c: v * pivot for c, v in right[r].items()} if pivot != 1 else right[r]
            for c, v in right[i].items():
                value = target.get(c, 0) - factor * v
                if value == 0:
                    target.pop(c, None)
                else:
                    target[c] = value
            den[r] *= pivot
            common = gcd(den[r], *row.values(), *target.values())
            if common > 1:
                row, target, den[r] = {c: v // common for c, v in row.items()}, {c: v // common for c, v in target.items()}, den[r] // common
            left[r], right[r] = row, target
        active.discard(i)
        active_columns.discard(j)
        for c in left[i]:
            count[c] -= 1
        row_of[j] = i
    assert det.denominator == 1
    numerators = np.zeros((s, s), dtype=object)
    for j in range(s):
        for c, v in right[row_of[j]].items():
            numerators[j, c], rest = divmod(v * det.numerator, den[row_of[j]])
            assert rest == 0
    _sparse_inverses[key] = numerators, det.numerator
    _sparse_inverse_entries[0] += s * s
    while _sparse_inverse_entries[0] > _SPARSE_INVERSES_KEPT and len(_sparse_inverses) > 1:
        oldest = next(iter(_sparse_inverses))  # (a dict keeps the order of insertion)
        _sparse_inverse_entries[0] -= oldest[0] * oldest[0]
        del _sparse_inverses[oldest]
    return numerators, det.numerator


class BasisState:
    def __init__(self, columns, b, cost, basis, artificial_rows=(), phase=2, extended=None):
        """``columns[j]``: provider column j as ``[(row, int or Fraction)]`` (a ``DenseLE``, or a list of such lists); ``b``, ``cost``:
        right-hand side and provider costs; ``basis``: as ``Solver.basis()``; ``artificial_rows[k]``: the row of artificial k;
        ``phase`` 1 prices the artificials at 1 and everything else at 0.  ``extended=False`` forces the exact integer path."""
        self.columns = columns
        self.m = len(b)
        self.b = [Fraction(int(v)) if not isinstance(v, Fraction) else v for v in b]
        self.artificial_rows = [int(r) for r in artificial_rows]
        self.n_art = len(self.artificial_rows)
        self.n = self.n_art + len(columns)
        if phase == 1:
            self.cost = [Fraction(1)] * self.n_art + [Fraction(0)] * len(columns)
        else:
            self.cost = [Fraction(0)] * self.n_art + [v if isinstance(v, Fraction) else Fraction(int(v)) for v in cost]
            self.cost += [Fraction(0)] * (self.n - len(self.cost))  # (`cost` may stop at the last structural: slacks cost nothing)
        self.basis = [self.n_art + int(c) if c >= 0 else -1 - int(c) for c in basis]
        assert len(self.basis) == self.m and len(set(self.basis)) == self.m
        self.extended = EXTENDED if extended is None else bool(extended)
        self.is_basic = np.zeros(self.n, dtype=bool)
        self.is_basic[self.basis] = True
        self._invert()
        self._vectors()
        self._matrix = None

    # ---- the columns ----------------------------------------------------------------------------
    def column(self, j):
        """Column j of ``[artificials | provider]`` as ``[(row, Fraction)]``."""
        if j < self.n_art:
            return [(self.artificial_rows[j], Fraction(1))]
        return [(int(i), Fraction(v)) for i, v in self.columns[j - self.n_art] if v != 0]

    def _integer_column(self, j):
        """``(rows, integer values, scale)`` with column = values / scale."""
        entries = self.column(j)
        scale = lcm(*[v.denominator for _, v in entries]) if entries else 1
        return [i for i, _ in entries], np.array([int(v * scale) for _, v in entries], dtype=object), scale

    def matrix(self):
        """All n columns as an (m, n) ``longdouble`` array (``hi + lo`` of every entry)."""
        if self._matrix is None:
            out = np.zeros((self.m, self.n), dtype=np.longdouble)
            for k, row in enumerate(self.artificial_rows):
                out[row, k] = 1
            if hasattr(self.columns, "matrix"):
                out[:, self.n_art:] = self.columns.matrix()
            else:
                for j in range(self.n_art, self.n):
                    for i, v in self.column(j):
                        hi, lo = split(v.numerator, v.denominator)
                        out[i, j] = np.longdouble(hi) + np.longdouble(lo)
            self._matrix = out
        return self._matrix

    def basis_matrix(self):
        """``B`` in f64 (every entry rounded once, as the device holds it)."""
        out = np.zeros((self.m, self.m))
        for k, j in enumerate(self.basis):
            for i, v in self.column(j):
                out[i, k] = float(v)
        return out

    # ---- B^-1 = num[k, :] / den[k] ----------------------------------------------------------------
    def _invert(self):
        m = self.m
        columns = [self.column(j) for j in self.basis]
        scale = []  # B' = B diag(scale) is an integer matrix whose single-entry columns are unit vectors
        for entries in columns:
            if not entries:
                raise ZeroDivisionError("singular basis")
            scale.append(1 / entries[0][1] if len(entries) == 1 else Fraction(lcm(*[v.denominator for _, v in entries])))
        unit = [k for k in range(m) if len(columns[k]) == 1]
        unit_row = [columns[k][0][0] for k in unit]
        if len(set(unit_row)) != len(unit_row):
            raise ZeroDivisionError("singular basis")
        other = [k for k in range(m) if len(columns[k]) != 1]
        taken = set(unit_row)
        rest = [i for i in range(m) if i not in taken]
        scaled = np.zeros((m, len(other)), dtype=object)
        for a, k in enumerate(other):
            for i, v in columns[k]:
                scaled[i, a] = int(v * scale[k])
        # rows `rest` hold nothing of the unit columns: B'[rest, other] is the Schur block, and
        #   x_other = B11^-1 y_rest,   x_u = y_row(u) - B'[row(u), other] x_other
        block, det = fraction_free_inverse(scaled[rest, :])
        num = np.zeros((m, m), dtype=object)
        if other:
            num[np.ix_(other, rest)] = block
            if unit:
                num[np.ix_(unit, rest)] = -scaled[unit_row, :].dot(block)
        for k, row in zip(unit, unit_row):
            num[k, row] = det
        den = []
        for k in range(m):
            d = det * scale[k].denominator
            if scale[k].numerator != 1:
                num[k, :] = num[k, :] * scale[k].numerator
            if d < 0:
                d = -d
                num[k, :] = -num[k, :]
            den.append(d)
        self.num, self.den = num, den
        self.inverse_hi = np.zeros((m, m))
        self.inverse_lo = np.zeros((m, m))
        for k in range(m):
            for i in np.flatnonzero(num[k, :] != 0):
                self.inverse_hi[k, i], self.inverse_lo[k, i] = split(num[k, i], den[k])

    def inverse_exact(self, k, i):
        return Fraction(self.num[k, i], self.den[k])

    def inverse_row(self, k):
        """Row k of ``B^-1`` as ``(hi, lo)``."""
        return self.inverse_hi[k], self.inverse_lo[k]

    def inverse_long(self):
        return long_double(self.inverse_hi, self.inverse_lo)

    # ---- x_B, the objective, pi --------------------------------------------------------------------
    def _vectors(self):
        m = self.m
        b_scale = lcm(*[v.denominator for v in self.b])
        b_int = np.array([int(v * b_scale) for v in self.b], dtype=object)
        x_num = self.num.dot(b_int)
        self.x_exact = [Fraction(int(x_num[k]), self.den[k] * b_scale) for k in range(m)]
        self.x_hi, self.x_lo = (np.array(v) for v in zip(*[split_fraction(x) for x in self.x_exact]))
        c_basic = [self.cost[j] for j in self.basis]
        self.objective_exact = sum((c * x for c, x in zip(c_basic, self.x_exact)), Fraction(0))
        common = lcm(*self.den)
        c_scale = lcm(*[c.denominator for c in c_basic])
        weights = np.array([int(c * c_scale) * (common // d) for c, d in zip(c_basic, self.den)], dtype=object)
        self.pi_num, self.pi_den = weights.dot(self.num), common * c_scale  # pi' = c_B' B^-1
        self.pi_hi, self.pi_lo = (np.array(v) for v in zip(*[split(int(p), self.pi_den) for p in self.pi_num]))

    def x_basic(self):
        return self.x_hi, self.x_lo

    def objective(self):
        return split_fraction(self.objective_exact)

    # ---- per-column quantities, exact ---------------------------------------------------------------
    def reduced_cost_exact(self, j):
        rows, values, scale = self._integer_column(j)
        return self.cost[j] - Fraction(int(self.pi_num[rows].dot(values)), self.pi_den * scale)

    def alpha_exact(self, j):
        """``B^-1 a_j`` as m Fractions."""
        rows, values, scale = self._integer_column(j)
        products = self.num[:, rows].dot(values)
        return [Fraction(int(products[k]), self.den[k] * scale) for k in range(self.m)]

    def gamma_exact(self, j):
        return 1 + sum((v * v for v in self.alpha_exact(j)), Fraction(0))

    # ---- per-column quantities over many columns: longdouble from hi + lo, or exact on a sample ------
    def columns_to_check(self, n_grouped=0, group=16, minimum=256):
        """Every column where ``longdouble`` is extended.  Otherwise a sample for the exact integer path: the first and the last column
        of every ``group`` of the first ``n_grouped`` provider columns, the whole last group, every single-entry column (their products
        cost nothing) and evenly spaced further ones up to ``minimum``."""
        if self.extended:
            return np.arange(self.n)
        first = self.n_art
        chosen = set(range(self.n_art))
        for start in range(0, n_grouped, group):
            chosen.add(first + start)
            chosen.add(first + min(start + group, n_grouped) - 1)
        chosen.update(range(first + max(0, (n_grouped - 1) // group * group), first + n_grouped))
        chosen.update(j for j in range(first + n_grouped, self.n) if len(self.columns[j - first]) == 1)
        target = min(self.n, minimum)
        if len(chosen) < target:
            for j in np.linspace(0, self.n - 1, target - len(chosen)).astype(int):
                chosen.add(int(j))
        j = 0
        while len(chosen) < target:
            chosen.add(j)
            j += 1
        return np.array(sorted(chosen))

    def reduced_costs(self, columns):
        if not self.extended:
            return np.array([float(self.reduced_cost_exact(int(j))) for j in columns], dtype=np.longdouble)
        cost = long_double(*zip(*[split_fraction(self.cost[int(j)]) for j in columns]))
        return cost - long_double(self.pi_hi, self.pi_lo) @ self.matrix()[:, columns]

    def alpha(self, j):
        if not self.extended:
            return np.array([float(v) for v in self.alpha_exact(j)], dtype=np.longdouble)
        return self.inverse_long() @ self.matrix()[:, j]

    def gammas(self, columns):
        if not self.extended:
            return np.array([float(self.gamma_exact(int(j))) for j in columns], dtype=np.longdouble)
        columns = np.asarray(columns)
        inverse = self.inverse_long()
        out = np.zeros(len(columns), dtype=np.longdouble)
        for start in range(0, len(columns), 512):
            alphas = inverse @ self.matrix()[:, columns[start:start + 512]]
            out[start:start + 512] = 1 + (alphas * alphas).sum(axis=0)
        return out

    def right_multiply(self, rows, values):
        """``v' B^-1`` for a sparse row ``v`` of small integers, as a ``longdouble`` vector (exact to its last bit or two)."""
        total = [Fraction(0)] * self.m
        for r, v in zip(rows, values):
            for i in np.flatnonzero(self.num[int(r), :] != 0):
                total[i] += int(v) * Fraction(self.num[int(r), i], self.den[int(r)])
        return long_double(*zip(*[split_fraction(t) for t in total]))


class Component:
    """One connected component of the Schur block of a ``SparseBasisState`` (``_invert_components``)."""


class SparseBasisState(BasisState):
    """The same state for a sparse LP of thousands of rows, held in the structure ``_invert`` finds and never as an (m, m) or (m, n)
    array.  With ``B' = B diag(scale)`` (integer; single-entry columns become unit vectors), ``unit`` the positions of those columns,
    ``other`` the k remaining ones, ``rest`` the k rows no unit column takes, ``S = B'[rest, other]`` and ``U = B'[unit rows, other]``:

        x = B'^-1 y:   x_other = S^-1 y_rest,                         x_u = y_row(u) - U[u, :] x_other
        z = w' B'^-1:  z_rest = (w_other - w_unit' U) S^-1,           z_row(u) = w_u

    so a row of the inverse has entries in ``rest`` and, for a unit position, at its own row.  ``S`` is inverted per CONNECTED COMPONENT
    of its row / column graph (``components``: a planted basis of 900 non-unit columns in blocks of at most 258 costs the sum of the
    blocks' cubes, not 900^3), each ``S_c^-1 = block_c / det_c`` in Python integers; ``det`` is the product of the ``det_c``, and
    ``den`` and ``row_exact`` are stated over it, so that they are the numbers of ``BasisState``.  Stored besides: ``S^-1`` as
    ``longdouble``, ``U`` as coordinate lists, the scales, and all n columns in compressed form.  The per-column quantities cost
    O(k nnz_j + nnz(U)) each.  Index spaces, ``den``, ``x_exact``, ``objective_exact``, ``reduced_cost_exact``, ``alpha_exact`` and
    ``gamma_exact`` are those of ``BasisState``; ``num`` is read a row at a time (``row_exact``)."""

    # ---- B^-1 --------------------------------------------------------------------------------------
    def _invert(self):
        m = self.m
        columns = [self.column(j) for j in self.basis]
        scale = []
        for entries in columns:
            if not entries:
                raise ZeroDivisionError("singular basis")
            scale.append(1 / entries[0][1] if len(entries) == 1 else Fraction(lcm(*[v.denominator for _, v in entries])))
        unit = [k for k in range(m) if len(columns[k]) == 1]
        unit_row = [columns[k][0][0] for k in unit]
        if len(set(unit_row)) != len(unit_row):
            raise ZeroDivisionError("singular basis")
        other = [k for k in range(m) if len(columns[k]) != 1]
        taken = set(unit_row)
        rest = [i for i in range(m) if i not in taken]
        k = len(other)
        rest_at = -np.ones(m, dtype=np.int64)  # row -> its place in `rest`, or -1
        rest_at[rest] = np.arange(k)
        unit_at = -np.ones(m, dtype=np.int64)  # row -> the place in `unit` of the unit column that takes it, or -1
        unit_at[unit_row] = np.arange(len(unit))
        schur = np.zeros((k, k), dtype=object)
        coo = []  # U: (place in `unit`, place in `other`, integer)
        for a, position in enumerate(other):
            for i, v in columns[position]:
                value = int(v * scale[position])
                if rest_at[i] >= 0:
                    schur[rest_at[i], a] = value
                else:
                    coo.append((int(unit_at[i]), a, value))
        self._invert_components(schur)
        self.k, self.scale = k, scale
        self.unit, self.unit_row, self.other, self.rest = (np.array(v, dtype=np.int64) for v in (unit, unit_row, other, rest))
        self.rest_at, self.unit_at = rest_at, unit_at
        coo.sort()
        self.coo_unit = np.array([c[0] for c in coo], dtype=np.int64)
        self.coo_other = np.array([c[1] for c in coo], dtype=np.int64)
        self.coo_value = [c[2] for c in coo]
        self.coo_long = np.array(self.coo_value, dtype=np.longdouble)  # (entries of B times an lcm of a few denominators: far below 2^64)
        self.coo_of_unit = {}  # place in `unit` -> [(place in `other`, integer)]
        for u, a, value in coo:
            self.coo_of_unit.setdefault(u, []).append((a, value))
        self.coo_of_other = {}  # place in `other` -> [(place in `unit`, integer)]
        for u, a, value in coo:
            self.coo_of_other.setdefault(a, []).append((u, value))
        self.place = np.zeros(m, dtype=np.int64)  # position -> its place in `unit` or in `other`
        self.place[self.unit] = np.arange(len(unit))
        self.place[self.other] = np.arange(k)
        self.in_other = np.zeros(m, dtype=bool)
        self.in_other[self.other] = True
        self.den, self.factor = [], []  # row `position` of B^-1 = factor * (row of det B'^-1) / den, den > 0 as in BasisState
        for position in range(m):
            d = self.det * scale[position].denominator
            self.den.append(abs(d))
            self.factor.append(scale[position].numerator * (-1 if d < 0 else 1))
        self.scale_long = long_double(*zip(*[split_fraction(s) for s in scale]))
        hi, lo = np.zeros((k, k)), np.zeros((k, k))
        for c in self.components:
            for a, row in zip(c.columns, c.block):
                for i, value in zip(c.rows, row):
                    hi[a, i], lo[a, i] = split(value, c.det)
        self.block_long = long_double(hi, lo)
        self._csc = None

    def _invert_components(self, schur):
        """``components``: the connected components of the graph that joins place i of ``rest`` with place a of ``other`` where
        ``schur[i, a] != 0``, each with ``rows`` (places in ``rest``), ``columns`` (places in ``other``), ``block[a, i]`` and ``det``:
        ``S_c^-1 = block / det``.  ``component_of[a]``, ``component_at[a]``: the component of place a of ``other`` and a's place in its
        ``columns``; ``row_component_of[i]``, ``row_component_at[i]``: the same for place i of ``rest``."""
        k = schur.shape[0]
        parent = list(range(2 * k))  # places of `rest`, then places of `other`

        def find(v):
            while parent[v] != v:
                parent[v] = parent[parent[v]]
                v = parent[v]
            return v
        for i, a in zip(*np.nonzero(schur != 0)):
            first, second = find(int(i)), find(k + int(a))
            if first != second:
                parent[second] = first
        members = {}
        for v in range(2 * k):
            members.setdefault(find(v), ([], []))[v >= k].append(v - k if v >= k else v)
        self.components = []
        self.component_of, self.component_at = np.zeros(k, dtype=np.int64), np.zeros(k, dtype=np.int64)
        self.row_component_of, self.row_component_at = np.zeros(k, dtype=np.int64), np.zeros(k, dtype=np.int64)
        self.det = 1
        for rows, columns in sorted(members.values()):
            if len(rows) != len(columns):
                raise ZeroDivisionError("singular basis")
            component = Component()
            component.rows, component.columns = np.array(rows, dtype=np.int64), np.array(columns, dtype=np.int64)
            component.block, component.det = sparse_inverse(schur[np.ix_(rows, columns)])
            self.component_of[columns], self.component_at[columns] = len(self.components), np.arange(len(columns))
            self.row_component_of[rows], self.row_component_at[rows] = len(self.components), np.arange(len(rows))
            self.components.append(component)
            self.det *= component.det
        for component in self.components:
            component.cofactor = self.det // component.det

    def _row_by_components(self, position):
        """Row ``position`` of ``det B'^-1`` before ``factor``: ``(columns, numerators)``, unsorted, zeros included."""
        if self.in_other[position]:
            a = self.place[position]
            c = self.components[self.component_of[a]]
            return self.rest[c.rows], c.block[self.component_at[a], :] * c.cofactor
        u = int(self.place[position])
        own = (np.array([self.unit_row[u]]), np.array([self.det], dtype=object))
        spread = {}  # component -> - U[u, columns of the component] block
        for a, value in self.coo_of_unit.get(u, ()):
            at = int(self.component_of[a])
            spread[at] = spread.get(at, 0) - value * self.components[at].block[self.component_at[a], :]
        parts = [(self.rest[self.components[at].rows], values * self.components[at].cofactor) for at, values in sorted(spread.items())]
        return np.concatenate([p[0] for p in parts] + [own[0]]), np.concatenate([p[1] for p in parts] + [own[1]])

    def row_exact(self, position):
        """Row ``position`` of ``B^-1`` as ``(columns, numerators)`` over ``den[position]``; zeros left out, columns ascending."""
        position = int(position)
        where, values = self._row_by_components(position)
        values = values * self.factor[position]
        keep = np.flatnonzero(values != 0)
        order = keep[np.argsort(where[keep], kind="stable")]
        return where[order], values[order]

    def inverse_exact(self, k, i):
        where, values = self.row_exact(k)
        at = np.flatnonzero(where == i)
        return Fraction(int(values[at[0]]), self.den[k]) if len(at) else Fraction(0)

    def inverse_row(self, k):
        hi, lo = np.zeros(self.m), np.zeros(self.m)
        where, values = self.row_exact(k)
        for i, value in zip(where, values):
            hi[i], lo[i] = split(int(value), self.den[k])
        return hi, lo

    def inverse_long(self):
        raise NotImplementedError("the structured state holds no (m, m) array: read inverse_row(k)")

    def matrix(self):
        raise NotImplementedError("the structured state holds no (m, n) array")

    def rows_that_may_not_be_unit(self):
        """Positions whose row of the inverse can have more than one entry (every other row is a multiple of a unit vector)."""
        return np.array(sorted(set(self.other.tolist()) | {int(self.unit[u]) for u in self.coo_of_unit}), dtype=np.int64)

    # ---- the two solves, exact --------------------------------------------------------------------------
    def _solve(self, rows, values):
        """``B^-1 y`` for the sparse ``y`` (Fractions) as ``{position: Fraction}``, zeros left out."""
        common = lcm(*[v.denominator for v in values]) if len(values) else 1
        ints = [int(v * common) for v in values]
        products = {}  # component -> common det_c S_c^-1 y_rows
        top = {}  # place in `unit` -> y_row(u) - U[u, :] x_other
        for i, v in zip(rows, ints):
            if v == 0:
                continue
            if self.rest_at[i] >= 0:
                at = int(self.row_component_of[self.rest_at[i]])
                products[at] = products.get(at, 0) + v * self.components[at].block[:, self.row_component_at[self.rest_at[i]]]
            else:
                top[int(self.unit_at[i])] = Fraction(v, common)
        out, solved = {}, {}  # solved: place in `other` -> x_other before the scale
        for at, product in products.items():
            c = self.components[at]
            for inside in np.flatnonzero(product != 0):
                a = int(c.columns[inside])
                solved[a] = Fraction(int(product[inside]), c.det * common)
                out[int(self.other[a])] = self.scale[self.other[a]] * solved[a]
        for a, x in solved.items():
            for u, value in self.coo_of_other.get(a, ()):
                top[u] = top.get(u, 0) - value * x
        for u, value in top.items():
            if value != 0:
                out[int(self.unit[u])] = self.scale[self.unit[u]] * value
        return out

    def _combine(self, weights):
        """``w' B^-1`` for ``{position: Fraction}`` as ``{row: Fraction}``, zeros left out."""
        scaled = {position: w * self.scale[position] for position, w in weights.items() if w != 0}
        out = {}
        reduced = [Fraction(0)] * self.k  # w_other - w_unit' U
        by_unit = {}
        for position, w in scaled.items():
            if self.in_other[position]:
                reduced[self.place[position]] += w
            else:
                by_unit[int(self.place[position])] = w
                out[int(self.unit_row[self.place[position]])] = w
        for u in by_unit.keys() & self.coo_of_unit.keys():
            for a, value in self.coo_of_unit[u]:
                reduced[a] -= by_unit[u] * value
        for c in self.components:
            mine = [reduced[a] for a in c.columns]
            if not any(mine):
                continue
            common = lcm(*[v.denominator for v in mine])
            product = np.array([int(v * common) for v in mine], dtype=object).dot(c.block)
            for i, value in zip(self.rest[c.rows].tolist(), product):
                if value != 0:
                    out[i] = Fraction(int(value), c.det * common)
        return out

    def _vectors(self):
        m = self.m
        x = self._solve(range(m), self.b)
        self.x_exact = [x.get(k, Fraction(0)) for k in range(m)]
        self.x_hi, self.x_lo = (np.array(v) for v in zip(*[split_fraction(v) for v in self.x_exact]))
        c_basic = [self.cost[j] for j in self.basis]
        self.objective_exact = sum((c * v for c, v in zip(c_basic, self.x_exact) if c != 0), Fraction(0))
        pi = self._combine({k: c for k, c in enumerate(c_basic)})
        self.pi_exact = [pi.get(i, Fraction(0)) for i in range(m)]  # pi' = c_B' B^-1
        self.pi_hi, self.pi_lo = (np.array(v) for v in zip(*[split_fraction(v) for v in self.pi_exact]))

    # ---- per-column quantities, exact ---------------------------------------------------------------
    def alpha_sparse_exact(self, j):
        entries = self.column(j)
        return self._solve([i for i, _ in entries], [v for _, v in entries])

    def alpha_exact(self, j):
        alpha = self.alpha_sparse_exact(j)
        return [alpha.get(k, Fraction(0)) for k in range(self.m)]

    def alpha_nnz(self, j):
        """The number of non-zeros of ``B^-1 a_j``, counted on the exact values."""
        return len(self.alpha_sparse_exact(j))

    def gamma_exact(self, j):
        return 1 + sum((v * v for v in self.alpha_sparse_exact(j).values()), Fraction(0))

    def reduced_cost_exact(self, j):
        return self.cost[j] - sum((self.pi_exact[i] * v for i, v in self.column(j)), Fraction(0))

    # ---- per-column quantities in longdouble from hi + lo --------------------------------------------------
    def compressed(self):
        """All n columns: ``(start, rows, longdouble values)``."""
        if self._csc is None:
            start, rows, hi, lo = [0], [], [], []
            for j in range(self.n):
                for i, v in self.column(j):
                    rows.append(i)
                    h, l = split(v.numerator, v.denominator)
                    hi.append(h)
                    lo.append(l)
                start.append(len(rows))
            self._csc = np.array(start, dtype=np.int64), np.array(rows, dtype=np.int64), long_double(hi, lo)
        return self._csc

    def _alpha_long(self, rows, values):
        """``(positions, longdouble values)`` of ``B^-1 a`` for a column given by rows and ``longdouble`` values."""
        at = self.rest_at[rows]
        inside = at >= 0
        if not inside.any():  # every entry lies in a row that a unit column takes: alpha is the column, scaled
            positions = self.unit[self.unit_at[rows]]
            return positions, self.scale_long[positions] * values
        out = np.zeros(self.m, dtype=np.longdouble)
        solved = self.block_long[:, at[inside]] @ values[inside]
        out[self.other] = solved
        top = np.zeros(len(self.unit), dtype=np.longdouble)
        top[self.unit_at[rows[~inside]]] = values[~inside]
        np.subtract.at(top, self.coo_unit, self.coo_long * solved[self.coo_other])
        out[self.unit] = top
        return np.arange(self.m), out * self.scale_long

    def alpha(self, j):
        if not self.extended:
            return np.array([float(v) for v in self.alpha_exact(j)], dtype=np.longdouble)
        start, rows, values = self.compressed()
        out = np.zeros(self.m, dtype=np.longdouble)
        positions, alpha = self._alpha_long(rows[start[j]:start[j + 1]], values[start[j]:start[j + 1]])
        out[positions] = alpha
        return out

    def alpha_nnz_estimates(self, columns):
        """Per column, how many entries of the ``longdouble`` alpha exceed 2^-40 of its largest: a guide to which columns have long
        and short alphas (``alpha_nnz`` is the exact count)."""
        start, rows, values = self.compressed()
        out = np.zeros(len(columns), dtype=np.int64)
        for at, j in enumerate(columns):
            _, alpha = self._alpha_long(rows[start[j]:start[j + 1]], values[start[j]:start[j + 1]])
            size = np.abs(alpha)
            out[at] = int((size > 2.0 ** -40 * size.max()).sum()) if len(size) else 0
        return out

    def gammas(self, columns):
        if not self.extended:
            return np.array([float(self.gamma_exact(int(j))) for j in columns], dtype=np.longdouble)
        start, rows, values = self.compressed()
        out = np.zeros(len(columns), dtype=np.longdouble)
        for at, j in enumerate(columns):
            _, alpha = self._alpha_long(rows[start[j]:start[j + 1]], values[start[j]:start[j + 1]])
            out[at] = 1 + (alpha * alpha).sum()
        return out

    def reduced_costs(self, columns):
        if not self.extended:
            return np.array([float(self.reduced_cost_exact(int(j))) for j in columns], dtype=np.longdouble)
        start, rows, values = self.compressed()
        out = long_double(*zip(*[split_fraction(c) for c in self.cost]))
        np.subtract.at(out, np.repeat(np.arange(self.n), np.diff(start)), long_double(self.pi_hi, self.pi_lo)[rows] * values)
        return out[np.asarray(columns)]

    def right_multiply(self, rows, values):
        weights = {}
        for r, v in zip(rows, values):
            weights[int(r)] = weights.get(int(r), Fraction(0)) + Fraction(int(v))
        total = self._combine(weights)
        return long_double(*zip(*[split_fraction(total.get(i, Fraction(0))) for i in range(self.m)]))


# ---- the f64 restatement of the Newton-Schulz inversion and polish (the yardstick for the device's error after either) ----------
def newton_schulz_inverse(B):
    """``Solver::invert_from_scratch`` in numpy f64: ``X0 = B' / (|B|_1 |B|_inf)``, ``X <- X + X (I - B X)``, its stop rule."""
    m = B.shape[0]
    identity = np.eye(m)
    X = B.T / (np.abs(B).sum(axis=0).max() * np.abs(B).sum(axis=1).max())
    previous = np.inf
    for it in range(200):
        R = identity - B @ X
        residual = np.abs(R).max()
        X = X + X @ R
        if residual < 1e-11:
            break
        if it > 60 and residual >= previous:
            break
        previous = residual
    return X


def newton_schulz_polish(B, X):
    """``Solver::polish`` in numpy f64: at most two steps from the drifted inverse ``X``, with its stop rule."""
    identity = np.eye(B.shape[0])
    X = np.array(X, dtype=np.float64)
    for _ in range(2):
        R = identity - B @ X
        residual = np.abs(R).max()
        if residual < 1e-12:
            break
        if residual >= 0.5:
            return newton_schulz_inverse(B)
        X = X + X @ R
        if residual < 1e-8:
            break
    return X


def polished_tolerance(reference, exact):
    """The bound on the device's error after a polish or a from-scratch inversion: 16 times the error of the numpy f64 restatement
    of the same iteration at the same basis (the matrix cores sum in another order than BLAS, and the restatement's error is one
    sample of rounding noise), and never below 8 ulps of the largest entry.  ``exact``: ``longdouble``.  Returns (bound, error of
    the restatement)."""
    exact = np.asarray(exact, dtype=np.longdouble)
    error = float(np.abs(np.asarray(reference, dtype=np.longdouble) - exact).max())
    return max(16.0 * error, 8.0 * 2.0 ** -53 * float(np.abs(exact).max())), error
