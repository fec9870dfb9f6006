"""Two seeded families of sparse integer LPs for the state tests of the sparse pivot paths (tests/test_gpu_sparse_state.py,
tests/test_oracle_basis_state.py), each built once per process, and the exact reference's view of the LP the device was given.

``equality``  ``integer_lp`` of tools/record_round_trip_cases.py: ``A x = A x0``, entries +-{1, 2, 3}, costs >= 0, n = 2 m.  Every row
              starts with its artificial; the walk is a phase-one walk.
``less``      ``A x <= b`` with ``b = A x0 + r >= 0`` and costs ``c = A'y + s`` with ``y <= 0``, ``s >= 0`` (dual feasible, so bounded;
              a cost is negative only through ``y``).  No artificial; the walk is a phase-two walk from the slack basis.

Column j has ``lengths[j % len(lengths)]`` entries.  ``short``: 1 .. 5, alphas on both sides of the 32 non-zeros at which update_kernel
changes its lane layout.  ``mixed``: 1 .. 5, 9, 25, 40 -- inside the padded width of 8, in the prefetched entries 8 .. 23, beyond them.
Seeds are 1000 + m unless ``SEEDS`` names another.  An LP must meet ``preconditions`` after 100 pivots; where 1000 + m does not (row
m - 1 of the inverse stays a unit vector), 2000 + m, 3000 + m, ... are tried in that order and the first that does is taken.  The
walk that decides is ``walk(..., textbook=True)``: the f64 model under the reference's ratio rule, which the device takes on these LPs
up to 8192 rows (small integers: RELP_RATIO_AUTO).  tests/test_oracle_basis_state.py re-checks the replaced seeds with it.

The reference reads the model (``column_exact``, ``cost_exact``, ``right_hand_side_exact``, ``pivot_element_indices``), never the
generator's arrays: standardisation may flip rows and appends the slacks.
"""
import importlib.util
import os
from fractions import Fraction

import numpy as np

import relp_amd
from basis_state import SparseBasisState

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_round_trip_cases", os.path.join(ROOT, "tools", "record_round_trip_cases.py"))
_recorder = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_recorder)
integer_lp = _recorder.integer_lp

MIXES = {"short": (1, 2, 3, 4, 5), "mixed": (1, 2, 3, 4, 5, 9, 25, 40)}
LENGTH_CLASSES = ((1, 8), (9, 24), (25, 40))  # the padded width, the prefetched entries, the CSC tail
SEEDS = {("equality", "mixed", 1024): 2000 + 1024, ("equality", "mixed", 4096): 4000 + 4096, ("less", "mixed", 1025): 2000 + 1025,
         ("less", "mixed", 4097): 2000 + 4097}
PIVOTS, BATCH = 100, 64  # what every case of tests/test_gpu_sparse_state.py walks: a batch of 64 and one of 36
_cases = {}


def btrans(m):
    """Three vectors with a small non-zero integer in EVERY row: a wrong entry in a row that nothing else reads still shows."""
    i = np.arange(m)
    rows = i.astype(np.int32)
    return [(rows, (1.0 + i % 7)), (rows, -(1.0 + i % 5)), (rows, (1.0 + (3 * i) % 9) * np.where(i % 2, -1.0, 1.0))]


def less_lp(m, n, lengths, seed):
    """min c x, A x <= A x0 + r, x >= 0 (docstring of the module)."""
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
    return relp_amd.Model.from_general_form(columns, ["Less"] * m, [int(v) for v in b], [(int(c), 0, None) for c in cost])


class Provider:
    """What the device was given, read once from the host model; also the ``MatrixProvider`` that ``f64_model.Model`` walks."""

    def __init__(self, model):
        self.m, self.n = model.nr_rows, model.nr_columns
        self.columns = [[(i, Fraction(num, den)) for i, num, den in model.column_exact(j)] for j in range(self.n)]
        self.cost = [model.cost_exact(j) for j in range(self.n)]
        self.b = model.right_hand_side_exact()
        self.pivots = model.pivot_element_indices()
        taken = {row for row, _ in self.pivots}
        self.artificial_rows = [i for i in range(self.m) if i not in taken]

    def nr_rows(self):
        return self.m

    def nr_columns(self):
        return self.n

    def column(self, j):
        return self.columns[j]

    def cost_value(self, j):
        return self.cost[j]

    def right_hand_side(self):
        return self.b

    def pivot_element_indices(self):
        return self.pivots

    def length_of(self, j):
        """Entries of column j of ``[artificials | provider]``."""
        n_art = len(self.artificial_rows)
        return 1 if j < n_art else len(self.columns[j - n_art])

    def state(self, basis, phase, cls=SparseBasisState, **options):
        """The exact state of ``basis`` (as ``Solver.basis()`` gives it) under the costs of ``phase``."""
        return cls(self.columns, self.b, self.cost, basis, artificial_rows=self.artificial_rows, phase=phase, **options)


def case(family, mix, m):
    """``(model, provider, phase)`` of one LP, built once."""
    key = (family, mix, m)
    if key not in _cases:
        build = integer_lp if family == "equality" else less_lp
        model = build(m, 2 * m, MIXES[mix], SEEDS.get(key, 1000 + m))
        _cases[key] = (model, Provider(model), 1 if family == "equality" else 2)
    return _cases[key]


def preconditions(exact, provider, mix):
    """What a basis must be like after the 100 pivots for a case to say something, asserted from its exact state ``exact``.  Returns (rows
    of the inverse that are not unit vectors, the columns whose FTRAN is checked, their exact nnz(alpha), entered columns in the basis)."""
    m, n_art = exact.m, exact.n_art
    initial = {n_art + column for _, column in provider.pivots}  # (the slacks the walk of the `less` family starts from)
    entered = {j for j in exact.basis if j >= n_art and j not in initial}
    structural = [j for j in entered if provider.length_of(j) > 1]
    assert exact.k <= 128 and exact.k == len(structural)
    # 100 pivots less the re-entries and the columns that left again.  The state alone cannot count those; the walks keep 97 .. 100
    # (counts per case: docstring of tests/test_gpu_sparse_state.py), and ten fewer than 100 is as far as a case may fall
    assert PIVOTS - 10 <= len(entered) <= PIVOTS, len(entered)
    not_unit = [int(k) for k in exact.rows_that_may_not_be_unit() if len(exact.row_exact(k)[0]) > 1]
    free = np.flatnonzero(~exact.is_basic)
    free = free[free >= n_art]
    lengths = np.array([provider.length_of(int(j)) for j in free])
    chosen = [int(free[np.flatnonzero(lengths == length)[0]]) for length in MIXES[mix]]
    estimates = exact.alpha_nnz_estimates(free)
    chosen += [int(free[np.argmax(estimates)]), int(free[np.argmin(estimates)])]
    chosen = sorted(set(chosen))
    nnz = [exact.alpha_nnz(q) for q in chosen]
    assert max(nnz) > 32, nnz  # (update_kernel changes its lane layout at 32 non-zeros of alpha)
    if mix == "mixed":
        basic_lengths = [provider.length_of(j) for j in structural]
        for low, high in LENGTH_CLASSES:
            assert any(low <= length <= high for length in basic_lengths), (low, high)
        stripes = {k // 512 for k in not_unit}
        assert stripes == set(range((m + 511) // 512)) and m - 1 in not_unit, sorted(stripes)
    else:
        assert min(nnz) <= 32, nnz
    return not_unit, chosen, nnz, len(entered)


def walk(provider, phase, pivots, textbook=False, basis=None):
    """``pivots`` steps of the numpy f64 model of the device's loop, never polished; returns the model (``basis_of`` reads its basis).
    ``textbook``: the reference's ratio test (the exact minimum ratio, ties to the lowest leaving column) in place of the Harris test.
    ``basis``: where to start (as ``Solver.set_basis`` takes it, no artificial) instead of the slack basis; inverted by numpy."""
    from f64_model import Model, Options

    class Textbook(Model):
        def ratio(self, alpha):
            rows = np.flatnonzero(alpha > self.opt.tol_pivot)
            if rows.size == 0:
                return None
            ratios = np.maximum(self.xB[rows], 0.0) / alpha[rows]
            ties = rows[ratios <= ratios.min()]
            return int(ties[np.argmin(self.basis[ties])])
    options = Options()
    options.polish_period = 1 << 30
    options.max_iters = pivots
    model = (Textbook if textbook else Model)(provider, options)
    assert (model.n_art > 0) == (phase == 1)
    if basis is not None:
        assert model.n_art == 0 and min(basis) >= 0
        model.basis = np.array(basis, dtype=np.int64)
        model.pos[:] = -1
        model.pos[model.basis] = np.arange(model.m)
        model.Binv = np.linalg.inv(model.A[:, model.basis].toarray())
        model.xB = model.Binv @ model.xB
    model.set_phase(model.cost1 if phase == 1 else model.cost2)
    assert model.run_phase(phase) == "iteration_limit"
    model.price()  # applies the weight update of the last pivot
    return model


def basis_of(model):
    """The basis of an ``f64_model.Model`` in the numbering of ``Solver.basis()``."""
    return [int(c) - model.n_art if c >= model.n_art else -1 - int(c) for c in model.basis]
