"""The two inverse buffers and the two state copies of the fused pivot (relp_amd/csrc/kernels.hip `pivot_fused_kernel`,
`begin_batch_kernel`, `commit_kernel`) at every kind of batch edge.  Pivot k of a batch reads state copy k & 1 and the inverse buffer
``Ctl::t_buf`` names, and writes the other of each; in every launch that pivots the two agree (``t_buf`` is 0 at the start of a batch,
flips with every pivot, and a launch that makes no pivot leaves a status that stops the batch).  What can break that is the
bookkeeping around batches: batches that end at either parity (``commit_kernel`` copies back from the second buffer, the next batch
restarts at 0) and launches behind a stop inside a batch.  The kernel's column store (write-through) and a variant that took the buffer
from the batch parity were measured against these tests (profiles/fused_parity_ab.txt).

So the fused path is walked beside the three-kernel pivot (selected as in tests/test_gpu_fused.py), whose inverse is updated in place
and knows no parity, in pieces of every kind, and after EVERY ``iterate`` call the two handles must agree bit for bit: pivots made and
stop reason, basis, x_B, objective, the relative costs (that is -pi), the steepest-edge weights and rows of the inverse (all of them
up to 128 rows; above that a spread of rows after each call and all of them at the end).  With graph replay and without.  ``-m gpu``."""
import importlib.util
import os

import numpy as np
import pytest

import relp_amd

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_round_trip_cases", os.path.join(ROOT, "tools", "record_round_trip_cases.py"))
recorder = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(recorder)

GRAPH = pytest.mark.parametrize("use_graph", [1, 0], ids=["graph", "plain"])
ALL = 10 ** 6
_models = {}


def small_lp():
    """40 rows, 80 columns of 1-5 entries: feasible and bounded (tools/record_round_trip_cases.py), a few dozen pivots per phase."""
    if "small" not in _models:
        _models["small"] = recorder.integer_lp(40, 80, (1, 2, 3, 4, 5), 5040)
    return _models["small"]


def long_lp():
    """200 rows, 400 columns: phase one is longer than the batches of 64 and 65 pivots."""
    if "long" not in _models:
        _models["long"] = recorder.integer_lp(200, 400, (1, 2, 3, 4, 5), 5200)
    return _models["long"]


def unbounded_lp():
    """24 equality rows ``A x = A x0`` and 16 rows ``A x <= A x0 + 2`` over 80 columns with costs of both signs, and one column more
    with cost -1 and entries -1 .. -3 in the ``<=`` rows only: a ray of the feasible set along which the objective falls."""
    if "unbounded" not in _models:
        rng = np.random.RandomState(7040)
        m, n, m_eq = 40, 80, 24
        x0 = rng.randint(0, 4, size=n)
        b = np.zeros(m, dtype=np.int64)
        columns = []
        for j in range(n):
            rows = np.sort(rng.choice(m, size=1 + j % 5, replace=False))
            values = rng.randint(1, 4, size=len(rows)) * rng.choice((-1, 1), size=len(rows))
            columns.append([(int(i), int(v)) for i, v in zip(rows, values)])
            b[rows] += values * x0[j]
        b[m_eq:] += 2
        columns.append([(i, -int(rng.randint(1, 4))) for i in range(m_eq, m)])
        cost = [int(c) for c in rng.randint(-5, 6, size=n)] + [-1]
        _models["unbounded"] = relp_amd.Model.from_general_form(columns, ["Equal"] * m_eq + ["Less"] * (m - m_eq), [int(v) for v in b],
                                                                [(c, 0, None) for c in cost])
    return _models["unbounded"]


def load(model, fused, **options):
    if not fused:
        os.environ["RELP_NO_FUSED"] = "1"
    try:
        return relp_amd.Solver(certify=0, **options).load_model(model)
    finally:
        os.environ.pop("RELP_NO_FUSED", None)


class Pair:
    """The fused handle and the three-kernel handle of one LP, driven through the same calls."""

    def __init__(self, model, **options):
        plan = model.kernel_path(**options)
        assert plan["fused"] and plan["fused_rows"] == (2 if plan["m"] <= 1024 else 4)
        self.fused = load(model, True, **options)
        try:
            self.three = load(model, False, **options)
        except BaseException:
            self.fused.close()
            raise
        self.m = self.fused.m
        self.pivots = 0

    def close(self):
        self.fused.close()
        self.three.close()

    def __enter__(self):
        return self

    def __exit__(self, kind, value, trace):
        if kind is None:
            self.close()
        else:
            self.fused.close()
            self.three.close()

    def both(self, call):
        return call(self.fused), call(self.three)

    def rows(self, everything):
        if everything or self.m <= 128:
            return range(self.m)
        return sorted({0, 1, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, self.m - 2, self.m - 1} & set(range(self.m)) | set(range(0, self.m, self.m // 16)))

    def compare(self, what, everything=False):
        a, b = self.fused, self.three
        assert np.array_equal(a.basis(), b.basis()), what
        assert a.b().tobytes() == b.b().tobytes(), what
        assert float(a.objective_function_value()).hex() == float(b.objective_function_value()).hex(), what
        assert a.relative_costs().tobytes() == b.relative_costs().tobytes(), what
        assert a.gamma().tobytes() == b.gamma().tobytes(), what
        for i in self.rows(everything):
            assert a.basis_inverse_row(i).tobytes() == b.basis_inverse_row(i).tobytes(), (what, "row of the inverse", i)

    def begin(self, phase):
        self.both(lambda s: s.begin_phase_one() if phase == 1 else s.begin_phase_two())
        self.compare("begin of phase %d" % phase)

    def iterate(self, count, everything=False):
        got, want = self.both(lambda s: s.iterate(count))
        assert got == want, ("iterate(%d)" % count, got, want)
        self.pivots += got[0]
        self.compare("iterate(%d) -> %r after %d pivots" % (count, got, self.pivots), everything)
        return got

    def to_the_end_of_the_phase(self, step=ALL):
        """``iterate(step)`` until the phase stops; returns (pivots made, stop reason).  One call more after the stop: it must do nothing."""
        made = 0
        while True:
            done, reason = self.iterate(step)
            made += done
            assert made < 100000
            if reason != relp_amd.STOP_BUDGET:
                break
        assert self.iterate(step) == (0, reason)
        return made, reason

    def finish(self, step=ALL):
        """From somewhere in phase one through the hand-over to the end of phase two; returns the stop reason of phase two."""
        _, reason = self.to_the_end_of_the_phase(step)
        assert reason == relp_amd.STOP_NO_ENTERING
        self.begin(2)
        _, reason = self.to_the_end_of_the_phase(step)
        self.compare("the end", everything=True)
        return reason


def phase_lengths(model):
    """Pivots of phase one and of phase two, counted on the three-kernel path (no state copies, no parity)."""
    key = ("lengths", id(model))
    if key not in _models:
        solver = load(model, False)
        try:
            counts = []
            for phase in (1, 2):
                solver.begin_phase_one() if phase == 1 else solver.begin_phase_two()
                done, _ = solver.iterate(ALL)
                counts.append(done)
        finally:
            solver.close()
        _models[key] = tuple(counts)
    return _models[key]


def batch_length_for(pivots, odd):
    """A batch length L with a stop at in-batch index ``pivots % L`` of the wanted parity, and not at the batch's first launch."""
    for length in range(5, 40):
        index = pivots % length
        if index >= 1 and index % 2 == (1 if odd else 0):
            return length, index
    raise AssertionError("no batch length puts pivot %d at an %s index" % (pivots, "odd" if odd else "even"))


@GRAPH
@pytest.mark.parametrize("length", [1, 2, 3, 7, 64, 65])
def test_batches_of_every_length_end_at_both_parities(length, use_graph):
    """``pivots_per_launch`` = L: full batches end at parity L & 1; the calls below add pieces of L - 1, L + 1 and 1 pivots, so that
    ``commit_kernel`` copies back from the second buffer and from the first, and every next batch restarts at parity 0."""
    with Pair(small_lp() if length < 64 else long_lp(), pivots_per_launch=length, use_graph=use_graph) as pair:
        pair.begin(1)
        assert pair.iterate(length) == (length, relp_amd.STOP_BUDGET)  # (one full batch at the least)
        for count in (2 * length, max(1, length - 1), length + 1, 1, length):
            pair.iterate(count)
        assert pair.finish(step=3 * length + 1) == relp_amd.STOP_NO_ENTERING


@GRAPH
@pytest.mark.parametrize("odd", [True, False], ids=["odd", "even"])
def test_an_optimum_inside_a_batch(odd, use_graph):
    """Phase one ends (no entering column) at an odd / even launch of a full batch: the launches behind it in the batch make no pivot;
    then the hand-over and phase two, whose end falls inside a batch as well."""
    first, second = phase_lengths(small_lp())
    length, index = batch_length_for(first, odd)
    print("phase one: %d pivots, batches of %d: the stop is launch %d of its batch; phase two: %d pivots (launch %d)" % (first, length, index, second, second % length))
    with Pair(small_lp(), pivots_per_launch=length, use_graph=use_graph) as pair:
        pair.begin(1)
        assert pair.to_the_end_of_the_phase() == (first, relp_amd.STOP_NO_ENTERING)
        pair.begin(2)
        assert pair.to_the_end_of_the_phase() == (second, relp_amd.STOP_NO_ENTERING)
        pair.compare("the end", everything=True)


@GRAPH
@pytest.mark.parametrize("odd", [True, False], ids=["odd", "even"])
def test_an_unbounded_column_inside_a_batch(odd, use_graph):
    first, second = phase_lengths(unbounded_lp())
    assert second >= 2, "phase two of the unbounded LP stops at once: change its seed"
    length, index = batch_length_for(second, odd)
    print("phase two: %d pivots, then unbounded; batches of %d: the stop is launch %d of its batch" % (second, length, index))
    with Pair(unbounded_lp(), pivots_per_launch=length, use_graph=use_graph) as pair:
        pair.begin(1)
        assert pair.to_the_end_of_the_phase() == (first, relp_amd.STOP_NO_ENTERING)
        pair.begin(2)
        assert pair.to_the_end_of_the_phase() == (second, relp_amd.STOP_UNBOUNDED)
        pair.compare("the end", everything=True)


@GRAPH
@pytest.mark.parametrize("count", [3, 4], ids=["odd", "even"])
def test_a_budget_below_the_batch_length(count, use_graph):
    """``iterate(k)`` with k below the batch length of 64, again and again; then on through the hand-over to the end."""
    with Pair(small_lp(), use_graph=use_graph) as pair:
        pair.begin(1)
        for _ in range(4):
            assert pair.iterate(count) == (count, relp_amd.STOP_BUDGET)
        assert pair.finish() == relp_amd.STOP_NO_ENTERING


@GRAPH
@pytest.mark.parametrize("m", [1, 8, 9, 63, 64, 65, 512, 513, 1024, 1025, 2048])
def test_row_counts_where_the_load_code_changes_shape(m, use_graph):
    """Lanes and waves past m, a column workgroup with one column (m = 9), two and four rows per thread: batches of 16 (replayed as
    a graph), then pieces of 5 and 2 pivots -- a commit from the second buffer, then one from the first -- and a batch again."""
    with Pair(recorder.model("rows%d" % m), pivots_per_launch=16, use_graph=use_graph) as pair:
        pair.begin(1)
        if m <= 65:
            for count in (16, 5, 2, 16):
                pair.iterate(count)
            pair.finish(step=48)
        else:
            for count in (32, 5, 2):
                assert pair.iterate(count) == (count, relp_amd.STOP_BUDGET)
            assert pair.iterate(16, everything=True) == (16, relp_amd.STOP_BUDGET)
        assert pair.fused.stats().launches < pair.three.stats().launches  # (two launches per pivot against three: the paths differ)
