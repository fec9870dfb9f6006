"""Planted rows for the kernel edges of the long-step ratio test (tests/test_dual_planted_rows_host.py,
tests/test_gpu_dual_long_step_edges.py): LPs whose first dual pivot is made through an inverse that is exactly the identity (rows of
``+-e_i``) on small integers or dyadic fractions, so that every quantity ``dual_long_step_kernel`` and ``dual_pivot_kernel<true, true>``
(relp_amd/csrc/dual.hip) read at that pivot is exact in f64 and the device must take the exact reference's decision in a tie, at a
slot or flip limit, and at the slope floor, with no margin.

The construction (``planted``): every row is ``"Less"`` with ``b >= 0`` and the basis is every row slack, so ``Binv = I``, all basic
costs are 0, ``-pi = 0``, ``d_j = sgn_j c_j`` and ``alpha_row[j] = sgn_j a_pj``.  A boxed variable that starts at its upper bound is
listed on its own bound row of the start basis (the reference and ``Solver::place_basis`` read that as complemented), and moves the
right-hand side: ``x_B[p] = b_p - sum ub_j a_pj < 0`` plants the violation ``delta`` of row p on the lower side.  Dual feasibility
is ``c_j >= 0`` for a column held as ``x_j`` and ``c_j <= 0`` for a complemented one.  A column is a candidate of row p on either
side iff ``sgn_j a_pj < 0``; its ratio is ``|c_j| / |a_pj|`` and its drop ``ub_j |a_pj|``.  Because ``b_p >= 0``, every planted row
has a *ballast*: a complemented boxed candidate ``(a_p = +1, ub = BALLAST, cost = -BALLAST_RATIO)``, the last candidate of the
order, which makes any ``delta`` reachable.  It counts among the boxed candidates wherever a case states a number of them.
A violation on the upper side (``upper=u0``): the boxed singleton ``-e_p`` with cost 0 and the bound ``u0`` is basic in row p instead
of the slack (the row of the inverse is ``-e_p``, and the row's own slack is then no candidate on that side), ``x_B[p] = -rhs_p > u0``.

The other rows carry a large right-hand side (``ROOM``), so they stay feasible: a walk is the planted pivot and, where the cap or
the slot limit makes the entering variable overshoot its own bound (it always does when a candidate that could have been passed has
to enter), the pivots that bring that row back.  Those later pivots run through a non-identity inverse and meet the ``MARGIN``
leads of tests/dual_long_step_lps.py, which ``assert_conditions`` checks; only the planted pivot may hold a tie.

The constants of the kernels that the planted sizes are built around are restated here and compared with the source text by
tests/test_dual_planted_rows_host.py.
"""
import functools
from fractions import Fraction

import relp_amd
from relp_amd.api import RATIO_HARRIS, RATIO_TEXTBOOK, default_options
import dual_long_step_lps as lps
from dual_bounded_lps import BoundedDualReference, Formulation

MARGIN = lps.MARGIN
SLOTS = 2048       # DUAL_LONG_STEP_SLOTS (relp_amd/csrc/dual.hpp)
MAX_FLIPS = 32     # DUAL_MAX_FLIPS (relp_amd/csrc/dual.hpp)
SCAN = 8192        # DL_U * DL_THREADS (relp_amd/csrc/dual.hip): the columns of one trip of dual_long_step_kernel's scans
CHUNK = 1024       # DL_COL_CHUNK (relp_amd/csrc/dual.hip): entries of a column staged per pass of the pivot kernel's FTRANs
ROOM = 100000      # the right-hand side of the rows that are not planted
BALLAST, BALLAST_RATIO = 1000, 50000
ORACLE_MAX_ROWS, ORACLE_MAX_COLUMNS = 8, 100  # the final objective is compared with the oracle's up to these sizes


def handle_tolerances():
    """``(harris_delta, tol_dual, tol_pivot)`` of a handle's default options, as the exact values of the doubles."""
    options = default_options()
    return Fraction(options.harris_delta), Fraction(options.tol_dual), Fraction(options.tol_pivot)


def column(p, a, cost, ub=None, complemented=False, extra=()):
    """One column description: ``a`` in row p and ``extra`` entries ``(row, value)`` elsewhere."""
    assert all(row != p for row, _ in extra)
    return (sorted([(p, a)] + list(extra)), cost, ub, complemented)


def candidate(p, ratio, magnitude=1, ub=None, complemented=False, extra=()):
    """A candidate of row p (``sgn_j a_pj < 0``) with the given ratio: the cost and the coefficient get the signs of its held form."""
    sign = -1 if complemented else 1
    return column(p, -sign * magnitude, sign * Fraction(ratio) * magnitude, ub, complemented, extra)


def ballast(p, ratio=BALLAST_RATIO, extra=()):
    return candidate(p, ratio, 1, BALLAST, True, extra)


def planted(m, columns, deltas, upper=None, room=ROOM):
    """``(formulation, start basis)``.  ``columns``: ``(entries, cost, ub, complemented)`` per structural; ``deltas``: ``{row: violation}``
    of the planted rows; ``upper``: ``{row: u0}`` of the rows violated on the upper side, each through an appended basic column
    ``-e_row`` with that bound; ``room``: the right-hand side of the other rows."""
    upper = dict(upper or {})
    columns = list(columns) + [([(row, -1)], 0, u0, False) for row, u0 in sorted(upper.items())]
    basic_at = {row: len(columns) - len(upper) + k for k, row in enumerate(sorted(upper))}
    shift = [Fraction(0)] * m  # sum ub_j a_ij over the complemented columns
    for entries, cost, ub, complemented in columns:
        assert ub is not None or not complemented
        assert (cost <= 0) if complemented else (cost >= 0), "the start basis is not dual feasible"
        if complemented:
            for i, v in entries:
                shift[i] += Fraction(ub) * v
    b = []
    for i in range(m):
        if i not in deltas:
            b.append(room)
        elif i in upper:  # x_B = -rhs = shift - b = u0 + delta
            b.append(shift[i] - upper[i] - deltas[i])
        else:  # x_B = rhs = b - shift = -delta
            b.append(shift[i] - deltas[i])
        assert b[-1] >= 0, ("row %d needs more ballast" % i, b[-1])
    form = Formulation([entries for entries, _, _, _ in columns], b, [cost for _, cost, _, _ in columns], [ub for _, _, ub, _ in columns])
    basis = [basic_at.get(i, form.ns + i) for i in range(m)]
    for j in form.bounded:
        basis.append(j if columns[j][3] else form.bound_slack[j])
    return form, basis


class Case:
    """A planted LP, the reference that walks it and what the case is named for.  ``options``: of the ``Solver``; ``reference_class``
    and ``reference_options``: of its exact reference; ``check(reference)``: the conditions of this case alone on the finished walk
    (``reference.walks[0]`` is the planted pivot); ``harris``: signed costs may end at ``-tol_dual`` (the Harris rule's own slack);
    ``within_floor``: a row may end violated by ``harris_delta`` at most, which the device calls feasible."""

    def __init__(self, name, form, basis, check, options=None, reference_class=lps.LongStepBoundedDualReference, reference_options=None,
                 harris=False, within_floor=False):
        self.name, self.form, self.basis, self.check = name, form, basis, check
        self.options = dict(options or {})
        self.reference_class, self.reference_options = reference_class, dict(reference_options or {})
        self.harris, self.within_floor = harris, within_floor

    def reference(self):
        floor, tol_dual, tol_pivot = handle_tolerances()
        options = dict(max_flips=MAX_FLIPS, slots=SLOTS, slope_floor=floor)
        if self.harris:
            options.update(tol_dual=tol_dual, tol_pivot=tol_pivot)
        options.update(self.reference_options)
        return self.reference_class(self.form, self.basis, **options)


def spread(i, rows, p):
    """Two or three entries outside row p for column number i of a family, so that neighbours share rows."""
    others = [r for r in range(rows) if r != p]
    picked = [(others[i % len(others)], 1 + i % 3), (others[(i + 1) % len(others)], -1 - i % 2)]
    if i % 4 == 0 and len(others) > 2:
        picked.append((others[(i + 2) % len(others)], 2))
    return picked


def counts(walk):
    """``(boxed candidates, candidates without a bound)`` of one pivot."""
    return walk["boxed"], len(walk["candidates"]) - walk["boxed"]


# ---- A. the slots ---------------------------------------------------------------------------------------------------------------
def slots_case(boxed):
    """m = 4.  Row 0: ``boxed`` boxed candidates (the ballast among them) with the ratios 1, 2, 3 .. in a scattered column order and
    drop 1 (the one of ratio 3: 8), three candidates without a bound far behind, delta = 5/2.  Row 1, delta 5/4: a second planted
    row with four candidates of its own, whose columns reach into rows 0, 2, 3.
    ``boxed <= SLOTS``: the ratios 1 and 2 are passed and 3 enters; then row 1 flips one column and pivots through the eta column of
    the first pivot.  ``boxed > SLOTS``: the kernel falls back to the plain rule, the ratio 1 enters and overshoots its bound 1, so
    row 0 comes back on the upper side with the ``boxed - 1`` candidates that are left -- that pivot fits the slots again, flips the
    ratio 2 and enters 3 --, and row 1 follows as above: one skipped pivot in three."""
    m, p, prime = 4, 0, 2053
    columns = []
    for i in range(boxed - 1):
        ratio = 1 + (i * 7919) % prime  # distinct for i < 2053
        columns.append(candidate(p, ratio, 1, 8 if ratio == 3 else 1, i % 3 == 0, [(2 + i % 2, 1 + i % 3)] + ([(3 - i % 2, -1)] if i % 5 < 2 else [])))
    columns.append(ballast(p))
    columns += [candidate(p, 3000 + k, 1, None, False, [(2, 1)]) for k in range(3)]
    columns += [column(p, 2, 7, None, False, [(3, 1)]), column(p, -1, -4, 6, True, [(2, 1)])]  # not candidates: sgn a > 0
    # row 1: the entries in row 0 have sgn a > 0, so these are no candidates of row 0
    columns += [candidate(1, 1, 1, 1, False, [(0, 1), (2, 2)]), candidate(1, 3, 2, 1, True, [(0, -1), (2, 1), (3, 1)]),
                candidate(1, 5, 1, None, False, [(3, 2)]), ballast(1, extra=[(3, 1)])]
    form, basis = planted(m, columns, {0: Fraction(5, 2), 1: Fraction(5, 4)})

    def check(reference):
        first = reference.walks[0]
        assert (first["p"], first["side"]) == (0, 1) and counts(first) == (boxed, 3)
        if boxed <= SLOTS:
            assert not first["overflow"] and len(first["passed"]) == 2 and first["entered"] == 2 and reference.skipped == 0
            second = reference.walks[1]
        else:
            assert first["overflow"] and first["passed"] == [] and first["entered"] == 0 and reference.skipped == 1
            plain = BoundedDualReference(form, basis)
            assert plain.step() is None and plain.pivots[0] == reference.pivots[0]
            again, second = reference.walks[1], reference.walks[2]
            assert (again["p"], again["side"], again["boxed"]) == (0, -1, boxed - 1) and not again["overflow"] and len(again["passed"]) == 1
            assert not second["overflow"]
        assert second["p"] == 1 and len(second["candidates"]) == 4 and len(second["passed"]) >= 1  # few candidates, and it flips again
    return Case("slots, %d boxed candidates" % boxed, form, basis, check, options={"ratio_rule": RATIO_TEXTBOOK})


# ---- B. the cap -----------------------------------------------------------------------------------------------------------------
def cap_case(boxed, upper=False):
    """m = 6.  Row 0: ``boxed`` boxed candidates (the ballast last) with distinct ratios and drop 1, none without a bound,
    delta = 100: the slope never ends the walk.  F is the first min(boxed - 1, 32) of the order and the next candidate enters; where
    that is not the ballast it overshoots its bound 1 and row 0 is brought back by a second pivot on the upper side, which flips the
    candidates that were left.  ``upper``: row 0 leaves on the upper side at the planted pivot already."""
    m, p, prime = 6, 0, 41
    columns = [candidate(p, 1 + (i * 7) % prime, 1, 1, i % 2 == 1, spread(i, m, p)) for i in range(boxed - 1)]
    columns.append(ballast(p, extra=[(1, 1)]))
    columns += [column(p, 1, 3, None, False, [(2, 1)]), column(p, -2, -1, 4, True, [(4, 1)])]  # not candidates
    form, basis = planted(m, columns, {0: Fraction(100)}, {0: 5} if upper else None)
    in_f = min(boxed - 1, MAX_FLIPS)

    def check(reference):
        first = reference.walks[0]
        assert (first["p"], first["side"]) == (0, -1 if upper else 1) and counts(first) == (boxed, 0)
        assert len(first["passed"]) == in_f and first["entered"] == in_f and first["stopped_behind"] is None
        assert first["slope"] == 100 - in_f > 0
        assert 0 in first["forms"] and 1 in first["forms"], "F holds one held form only"
        lengths = [len(form.columns[j]) for j in first["passed"]]
        assert min(lengths) >= 2 and max(lengths) <= 4
        shared = [set(i for i, _ in form.columns[j]) - {p} for j in first["passed"]]
        assert any(a & b for k, a in enumerate(shared) for b in shared[k + 1:]), "no two columns of F share a row"
        if boxed - 1 > MAX_FLIPS:  # the cap ended the walk: the entering candidate could have been passed
            _, q, magnitude = first["candidates"][in_f]
            assert first["slope"] - reference.ub[q] * magnitude > reference.slope_floor
            assert len(reference.pivots) == 2 and reference.pivots[1][3] == -1 and len(reference.flips[1]) == boxed - 2 - MAX_FLIPS
        else:
            assert len(reference.pivots) == 1
    return Case("cap, %d boxed candidates%s" % (boxed, ", upper side" if upper else ""), form, basis, check, options={"ratio_rule": RATIO_TEXTBOOK})


# ---- C. beyond one trip of the scans --------------------------------------------------------------------------------------------
def wide_case(which):
    """m = 4, 8500 structural columns, row 0.  Columns 0 .. 8199 are the front, 8200 .. 8499 the back (all >= SCAN); most are
    no candidates.  (i) the passed candidates sit in the back; (ii) the candidate without a bound that ends the walk sits there;
    (iii) the entering column sits there while F lies in the front."""
    m, p, ns, back = 4, 0, 8500, 8200
    special = {}
    if which == "passed":
        special = {back + 7: candidate(p, 1, 1, 1, True, [(1, 2), (2, 1)]), back + 150: candidate(p, 2, 1, 1, False, [(2, -1), (3, 1)]),
                   back + 299: candidate(p, 3, 1, 1, False, [(1, 1)]), 40: candidate(p, 50, 1, 1, False, [(1, 1)]),
                   5000: candidate(p, 60, 1, None, False, [(2, 1)])}
        delta, want = Fraction(5, 2), ([back + 7, back + 150], back + 299)
    elif which == "unbounded":
        special = {17: candidate(p, 1, 1, 1, False, [(1, 2), (2, 1)]), 4000: candidate(p, 2, 2, 1, True, [(2, -1), (3, 1)]),
                   back + 99: candidate(p, 3, 1, None, False, [(1, 1), (3, 2)]), 8000: candidate(p, 4, 1, 1, False, [(1, 1)]),
                   900: candidate(p, 7, 1, None, False, [(2, 1)])}
        delta, want = Fraction(10), ([17, 4000], back + 99)
    else:
        special = {17: candidate(p, 1, 1, 1, False, [(1, 2), (2, 1)]), 4000: candidate(p, 2, 1, 1, True, [(2, -1), (3, 1)]),
                   back + 250: candidate(p, 3, 2, 1, False, [(1, 1), (3, 2)]), 8000: candidate(p, 4, 1, 1, False, [(1, 1)]),
                   900: candidate(p, 7, 1, None, False, [(2, 1)])}
        delta, want = Fraction(5, 2), ([17, 4000], back + 250)
    special[8100] = ballast(p)
    columns = []
    for j in range(ns):
        if j in special:
            columns.append(special[j])
        elif j % 3 == 0:
            columns.append(column(p, 1, 1 + j % 5, None, False, [(1 + j % 3, 1)]))  # sgn a > 0: no candidate
        else:
            columns.append(column(1 + j % 3, 1, j % 4, None, False))  # no entry in row 0
    form, basis = planted(m, columns, {0: delta})

    def check(reference):
        first = reference.walks[0]
        assert form.n_device >= SCAN + 300 and len(reference.pivots) == 1
        assert first["passed"] == want[0] and reference.pivots[0][0] == want[1]
        if which == "passed":
            assert min(first["passed"]) >= SCAN
        elif which == "unbounded":
            assert want[1] >= SCAN and reference.ub[want[1]] is None and max(first["passed"]) < SCAN
            unbounded = [(ratio, j) for ratio, j, _ in first["candidates"] if reference.ub[j] is None]
            assert min(unbounded)[1] == want[1] and any(j < SCAN for _, j in unbounded)
        else:
            assert want[1] >= SCAN and max(first["passed"]) < SCAN and first["stopped_behind"] is not None
    return Case("wide, %s" % which, form, basis, check, options={"ratio_rule": RATIO_TEXTBOOK})


# ---- D. ties (the textbook rule on integer data) --------------------------------------------------------------------------------
def tie_case(which):
    """m = 5, row 2; integer data throughout, so that the plan resolves ``RATIO_AUTO`` to the textbook rule."""
    m, p = 5, 2
    far = [candidate(p, 9, 1, 2, False, [(0, 1)]), candidate(p, 11, 1, None, False, [(4, 1)])]
    idle = [column(p, 1, 2, None, False, [(1, 1)]), column(0, 1, 1, 3, False, [(3, 1)])]
    cost_zero = False
    if which == "two boxed":  # equal ratios 2 = 2/1 = 4/2; the slope admits one: the lower column is passed, the higher enters
        columns = idle + [candidate(p, 2, 1, 1, False, [(0, 1), (3, 2)]), candidate(p, 2, 2, 1, True, [(0, -1), (1, 1)])] + far + [ballast(p)]
        delta, want = Fraction(2), ([2], 3)
    elif which == "unbounded lower":  # ratio 2 twice; the one without a bound has the lower column: it enters, F stops in front of it
        columns = idle + [candidate(p, 1, 1, 1, True, [(0, 1), (3, 2)]), candidate(p, 2, 3, None, False, [(0, -1), (1, 1)]),
                          candidate(p, 2, 1, 1, False, [(0, 2), (4, 1)])] + far + [ballast(p)]
        delta, want = Fraction(10), ([2], 3)
    elif which == "unbounded higher":  # ... the higher column: the boxed one is passed first
        columns = idle + [candidate(p, 1, 1, 1, True, [(0, 1), (3, 2)]), candidate(p, 2, 1, 1, False, [(0, 2), (4, 1)]),
                          candidate(p, 2, 3, None, False, [(0, -1), (1, 1)])] + far + [ballast(p)]
        delta, want = Fraction(10), ([2, 3], 4)
    elif which == "all zero":  # every cost is 0: the order is by column alone
        columns = [column(p, 1, 0, None, False, [(1, 1)]), candidate(p, 0, 2, 1, False, [(0, 1), (3, 2)]), column(0, 1, 0, 3, False, [(3, 1)]),
                   candidate(p, 0, 1, 1, True, [(0, -1), (1, 1)]), candidate(p, 0, 3, None, False, [(0, 2), (4, 1)]),
                   candidate(p, 0, 1, 1, False, [(1, 1)]), ballast(p, ratio=0)]
        delta, want, cost_zero = Fraction(10), ([1, 3], 4), True
    else:  # "width zero": ub = 0 (pos -3) with the most attractive ratio 1/4 in the lowest column; never a candidate
        columns = [column(p, -4, 1, 0, False, [(0, 1)])] + idle + [candidate(p, 2, 1, 1, False, [(0, 1), (3, 2)]),
                                                                   candidate(p, 3, 2, 1, True, [(0, -1), (1, 1)])] + far + [ballast(p)]
        delta, want = Fraction(2), ([3], 4)
    form, basis = planted(m, columns, {p: delta})

    def check(reference):
        first = reference.walks[0]
        assert len(reference.pivots) == 1 and first["passed"] == want[0] and reference.pivots[0][0] == want[1]
        ratios = {j: ratio for ratio, j, _ in first["candidates"]}
        if which == "two boxed":
            assert ratios[2] == ratios[3] and reference.ub[2] is not None and reference.ub[3] is not None
            assert first["stopped_behind"] is not None and first["stopped_behind"] < 0
        elif which in ("unbounded lower", "unbounded higher"):
            free, box = (3, 4) if which == "unbounded lower" else (4, 3)
            assert ratios[free] == ratios[box] and reference.ub[free] is None and reference.ub[box] is not None
            assert first["stopped_behind"] is None  # the candidate without a bound ended the walk, not the slope
        elif which == "all zero":
            assert cost_zero and all(ratio == 0 for ratio in ratios.values()) and len(ratios) == 5
            assert [j for _, j, _ in first["candidates"]] == sorted(ratios)
        else:
            assert reference.ub[0] == 0 and 0 not in ratios and first["costs"][0] is None
            assert Fraction(1, 4) < min(ratios.values())  # it would have come first
            assert reference.fixed_cost_ties == 0
    return Case("tie, %s" % which, form, basis, check)


# ---- E. the slope floor ---------------------------------------------------------------------------------------------------------
def floor_case(which):
    """m = 5, row 1, the textbook rule by option (the data are dyadic).  The first candidate has the drop ``1 - eps`` against the
    slope 1 (``zero``: two candidates of drop 1 against the slope 2, and ``zero, passed`` the slope 3 alongside)."""
    m, p = 5, 1
    floor, _, _ = handle_tolerances()
    eps = {"below": Fraction(1, 2 ** 40), "above": Fraction(1, 2 ** 20)}.get(which)
    rest = [candidate(p, 5, 1, 1, False, [(3, 1)]), candidate(p, 8, 1, None, False, [(4, 1)]), column(p, 1, 2, None, False, [(2, 1)]), ballast(p)]
    if eps is None:
        columns = [candidate(p, 1, 1, 1, True, [(0, 1), (3, 2)]), candidate(p, 2, 1, 1, False, [(0, -1), (2, 1)])] + rest
        delta = Fraction(2) if which == "zero" else Fraction(5, 2)
        want = ([0], 1) if which == "zero" else ([0, 1], 2)
    else:
        columns = [candidate(p, 1, 1, 1 - eps, True, [(0, 1), (3, 2)]), candidate(p, 2, 1, 1, False, [(0, -1), (2, 1)])] + rest
        delta = Fraction(1)
        want = ([], 0) if which == "below" else ([0], 1)
    form, basis = planted(m, columns, {p: delta}, room=1000)  # (1000 - 2^-40 is a double, ROOM - 2^-40 is not)

    def check(reference):
        first = reference.walks[0]
        assert len(reference.pivots) == 1 and first["passed"] == want[0] and reference.pivots[0][0] == want[1]
        behind = first["stopped_behind"]
        if which == "zero":
            assert behind == 0
        elif which == "below":
            assert 0 < behind == eps <= floor
            exact = lps.LongStepBoundedDualReference(form, basis)  # the floor 0 passes it: the case tells the two rules apart
            assert exact.step() is None and exact.flips[0] == [0]
        elif which == "above":
            assert behind < 0 and first["delta"] - reference.ub[0] == eps > floor
        else:
            assert behind < 0
    return Case("floor, %s" % which, form, basis, check, options={"ratio_rule": RATIO_TEXTBOOK}, within_floor=which == "below")


# ---- F. long columns ------------------------------------------------------------------------------------------------------------
LONG_ROWS, LONG_P = 1025, 512


def long_case():
    """m = 1025, row 512.  F = {a complemented column with an entry in every row (1024 + 1 entries: two chunks), a short one}; the
    entering column has an entry in every row too.  One pivot from the identity."""
    m, p = LONG_ROWS, LONG_P
    every = lambda scale: [(i, scale * (1 + i % 3)) for i in range(m) if i != p]
    columns = [column(0, 1, 2, None, False, [(5, 1)]), candidate(p, 1, 1, 1, True, every(1)), candidate(p, 2, 1, 1, False, [(0, 2), (1024, -1), (7, 1)]),
               candidate(p, 3, 2, 1, False, [(i, 1 + i % 2) for i in range(m) if i != p]), candidate(p, 6, 1, None, False, [(3, 1)]), ballast(p)]
    form, basis = planted(m, columns, {p: Fraction(5, 2)})

    def check(reference):
        first = reference.walks[0]
        assert len(reference.pivots) == 1 and first["passed"] == [1, 2] and reference.pivots[0][0] == 3
        assert len(form.columns[1]) == CHUNK + 1 and len(form.columns[2]) < CHUNK and len(form.columns[3]) > CHUNK
        assert first["forms"] == [1, 0]
    # (a column of more than 1024 entries sends the default plan to the multi-block FTRAN, which the dual loop refuses: the option
    # that moves that threshold keeps the plan on the single-workgroup kernels, whose chunk loops are what this case is about)
    return Case("long columns", form, basis, check, options={"ftran_min_nnz": 2 * CHUNK, "ratio_rule": RATIO_TEXTBOOK})


# ---- G. the Harris rule with flips ----------------------------------------------------------------------------------------------
def harris_case(which):
    """m = 5, row 3, ``ratio_rule = RATIO_HARRIS``, dyadic costs.  The lowest column (cost 0) is passed.  Behind it A (ratio 2^-34,
    |abar| 1) and B (ratio 2^-33, |abar| 4): ``theta_max = (2^-31 + tol_dual) / 4`` holds both ratios, pass 2 takes B; the textbook rule
    takes A.  ``free``: A has no bound and ends the walk; ``boxed``: A has a bound and a drop the slope does not admit -- it stays
    where it is, un-passed, beside the Harris choice."""
    m, p = 5, 3
    a_ub = None if which == "free" else 10
    columns = [candidate(p, 0, 1, 1, True, [(0, 1), (1, 2)]), candidate(p, Fraction(1, 2 ** 34), 1, a_ub, False, [(0, -1), (2, 1)]),
               candidate(p, Fraction(1, 2 ** 33), 4, None, False, [(0, 2), (4, 1)]), candidate(p, 1, 8, None, False, [(1, 1)]),
               column(p, 1, 2, None, False, [(2, 1)]), ballast(p)]
    form, basis = planted(m, columns, {p: Fraction(5, 2)})

    def check(reference):
        first = reference.walks[0]
        assert len(reference.pivots) == 1 and first["passed"] == [0] and reference.pivots[0][0] == 2
        assert first["candidates"][first["entered"]][1] == 2 and first["entered"] == 2  # behind A in the order, ahead in |abar|
        textbook = lps.LongStepBoundedDualReference(form, basis, slope_floor=reference.slope_floor)
        assert textbook.step() is None and textbook.flips[0] == [0] and textbook.pivots[0][0] == 1
        assert (first["stopped_behind"] is None) == (which == "free")
        assert min(reference.theta_margins) >= MARGIN
    return Case("harris, A %s" % which, form, basis, check, options={"ratio_rule": RATIO_HARRIS},
                reference_class=lps.HarrisLongStepBoundedDualReference, harris=True)


CASES = {
    "slots_2048": lambda: slots_case(SLOTS), "slots_2049": lambda: slots_case(SLOTS + 1),
    "cap_32": lambda: cap_case(32), "cap_33": lambda: cap_case(33), "cap_34": lambda: cap_case(34), "cap_40": lambda: cap_case(40),
    "cap_40_upper": lambda: cap_case(40, upper=True),
    "wide_passed": lambda: wide_case("passed"), "wide_unbounded": lambda: wide_case("unbounded"), "wide_entering": lambda: wide_case("entering"),
    "tie_two_boxed": lambda: tie_case("two boxed"), "tie_unbounded_lower": lambda: tie_case("unbounded lower"),
    "tie_unbounded_higher": lambda: tie_case("unbounded higher"), "tie_all_zero": lambda: tie_case("all zero"), "tie_width_zero": lambda: tie_case("width zero"),
    "floor_zero": lambda: floor_case("zero"), "floor_zero_passed": lambda: floor_case("zero, passed"),
    "floor_below": lambda: floor_case("below"), "floor_above": lambda: floor_case("above"),
    "long_columns": long_case,
    "harris_free": lambda: harris_case("free"), "harris_boxed": lambda: harris_case("boxed"),
}
TEXTBOOK_BY_DATA = [name for name in CASES if name.startswith("tie_")]  # the plan resolves RATIO_AUTO to the textbook rule on these


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def is_double(value):
    return Fraction(float(value)) == value


def is_signed_unit(row, i):
    return all((v == 0) if k != i else (v in (1, -1)) for k, v in enumerate(row))


@functools.lru_cache(maxsize=None)
def walked(name):
    """``(case, reference, reason, bases, start, costs)`` of a finished walk, made once per process and only read: ``bases[k]`` the
    formulation's basis after pivot k, ``start`` before the first; ``costs[0]`` the smallest signed cost at the start and ``costs[k + 1]``
    after pivot k.  The start is checked to be what the construction promises."""
    planted_case = case(name)
    reference = planted_case.reference()
    m = reference.m
    assert all(is_signed_unit(reference.inverse[i], i) for i in range(m)), "the start inverse is not rows of +-e_i"
    assert all(reference.cost[j] == 0 for j in reference.basis), "a basic cost is not 0"
    form = planted_case.form
    assert all(is_double(v) for v in reference.x + reference.rhs + form.b + form.cost), "a planted value is no double"
    assert all(is_double(v) for entries in form.columns for _, v in entries) and all(u is None or is_double(u) for u in form.upper)
    start = reference.formulation_basis()
    costs, bases = [min(c for c in reference.signed_costs() if c is not None)], []
    while True:
        reason = reference.step()
        if reason is not None:
            break
        bases.append(reference.formulation_basis())
        costs.append(min(c for c in reference.signed_costs() if c is not None))
        assert len(bases) <= 8, "the walk does not end"
    return planted_case, reference, reason, bases, start, costs


def assert_conditions(name):
    """What a planted case must be like on the reference alone for the device comparison to say something: the start is the identity
    with basic costs 0 (``walked``), dual feasible before and after every pivot, the walk ends primal feasible, every pivot behind the
    planted one keeps the ``MARGIN`` leads, and the case hits the branch it is named for (``Case.check``)."""
    planted_case, reference, reason, bases, start, costs = walked(name)
    floor, tol_dual, _ = handle_tolerances()
    assert reason == relp_amd.STOP_NO_ENTERING, reason
    assert costs[0] >= 0, "the start is not dual feasible"
    assert min(costs) >= (-tol_dual if planted_case.harris else 0), costs
    allowed = floor if planted_case.within_floor else 0
    assert all(-allowed <= v and (u is None or v <= u + allowed) for v, u in zip(reference.x, reference.xub)), "the walk ends primal infeasible"
    assert reference.walks[0]["delta"] > 1000 * floor
    for k in range(1, len(reference.pivots)):  # through a non-identity inverse: no ties there
        assert min(reference.margins[k]) >= MARGIN and reference.slope_margins[k] >= MARGIN, (k, reference.margins[k], reference.slope_margins[k])
    assert reference.fixed_cost_ties == 0
    planted_case.check(reference)
    return planted_case, reference


def kernel_walk_model(walk, ub, floor, slots=SLOTS, max_flips=MAX_FLIPS, column_breaks_ties=True):
    """The walk of ``dual_long_step_kernel`` restated step for step over the candidates of one recorded pivot (``reference.walks[k]``),
    as the kernel organises it and not as the reference does: the candidates without a bound only give their smallest ``(ratio, j)``,
    the boxed ones are peeled one arg-min per round, and the tests come in the kernel's order.  Returns ``(passed, overflow)``.
    ``column_breaks_ties=False`` leaves out the clause that lets a boxed candidate go first when a candidate without a bound has the
    same ratio and a higher column: the host tests use it to show which planted cases tell that rule from its absence."""
    boxed = [(ratio, j, ub[j] * magnitude) for ratio, j, magnitude in walk["candidates"] if ub[j] is not None]
    free = min(((ratio, j) for ratio, j, _ in walk["candidates"] if ub[j] is None), default=None)
    if not boxed:
        return [], False
    if len(boxed) > slots:
        return [], True
    slope, passed, left = walk["delta"], [], list(boxed)
    while len(passed) < max_flips and len(passed) + 1 < len(walk["candidates"]):
        if not left:
            break
        ratio, j, drop = min(left)
        if free is not None and (free[0] < ratio or (free[0] == ratio and (free[1] < j or not column_breaks_ties))):
            break
        behind = slope - drop
        if not behind > floor:
            break
        left.remove((ratio, j, drop))
        passed.append(j)
        slope = behind
    return passed, False
