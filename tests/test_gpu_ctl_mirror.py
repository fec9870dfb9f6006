"""The host's view of the control block (relp_amd/csrc/solver.hip: `read_ctl`, `read_ctl_after_batch`, `write_ctl`).

The handle keeps a pinned, host-mapped mirror of the device's control block.  On the fused path `commit_kernel` stores the
committed block into the mirror itself and `iterate` reads it after synchronising the stream, with no copy enqueued; every other
reader copies into the mirror explicitly.  A mirror read too early -- before the batch that writes it has finished -- shows up as
a wrong `done`: `iterate(k)` must report exactly k pivots while the phase runs, whatever the sizes of the pieces, and a run in
pieces must end in the state of one `iterate` of the whole: stop reason, pivot counts, basis, the bits of the objective.

`stats().launches` counts a begin and a commit kernel per batch (2 + 2 b launches for a plain fused batch of b pivots, 1 + 3 b for
a captured one and for the three-kernel pivot), so a run in pieces cannot have the launch count of one long batch; what the
library must not do is add a launch anywhere, so the count of every run is checked against that closed form of its own batches
(``-m gpu``)."""
import itertools
import os

import numpy as np
import pytest

import relp_amd
from relp_amd import api
from relp_amd.workloads import max_flow_graph

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AFIRO = os.path.join(ROOT, "data", "netlib", "AFIRO.SIF")
BATCH = 64  # relp_options.pivots_per_launch, the default
PIECES = {"issue": [1, 63, 1, 64, 65, 2, 130, 7], "small": [1, 2, 1, 3, 5, 1, 4]}
CAP = 100000


def run_whole(solver):
    """Both phases, one `iterate` each (AFIRO leaves no zero-level artificial behind, tests/test_gpu_fused.py)."""
    calls = []
    solver.begin_phase_one()
    for phase in (1, 2):
        done, reason = solver.iterate(CAP)
        calls.append((CAP, done, reason))
        if phase == 1:
            solver.begin_phase_two()
    return calls


def run_pieces(solver, pieces):
    """The same in pieces; `done` must be what was asked for until the phase ends."""
    calls = []
    sizes = itertools.cycle(pieces)
    solver.begin_phase_one()
    for phase in (1, 2):
        while True:
            asked = next(sizes)
            done, reason = solver.iterate(asked)
            calls.append((asked, done, reason))
            assert len(calls) < CAP
            if reason == relp_amd.STOP_BUDGET:
                assert done == asked, (phase, calls)  # a stale control block reports another number
                continue
            assert done <= asked, (phase, calls)
            break
        if phase == 1:
            solver.begin_phase_two()
    return calls


def state(solver, calls):
    reasons = [reason for _, _, reason in calls if reason != relp_amd.STOP_BUDGET]
    per_phase, total = [], 0
    for _, done, reason in calls:
        total += done
        if reason != relp_amd.STOP_BUDGET:
            per_phase.append(total)
            total = 0
    return {"stop_reasons": reasons, "pivots": per_phase, "basis": [int(v) for v in solver.basis()],
            "objective": float(solver.objective_function_value()).hex()}


def expected_launches(calls, per_batch):
    """Launches of the batches `iterate` issued for `calls` = [(asked, done, reason)]: batches of min(what is left to do, BATCH)
    pivots until `done` pivots were made or a batch made fewer than it was given (the end of the phase)."""
    launches = 0
    for asked, done, _ in calls:
        made_so_far = 0
        while made_so_far < asked:
            batch = min(asked - made_so_far, BATCH)
            launches += per_batch(batch)
            made = min(batch, done - made_so_far)
            made_so_far += made
            if made < batch:
                break
    return launches


def fused_launches(use_graph):
    return lambda b: 1 + 3 * b if (use_graph and b == BATCH) else 2 + 2 * b


@pytest.mark.parametrize("pieces", sorted(PIECES))
@pytest.mark.parametrize("options", [{"use_graph": 1}, {"use_graph": 0}, {"use_graph": 1, "pivot_kernels": 1}, {"use_graph": 0, "pivot_kernels": 1}],
                         ids=["fused-graph", "fused-plain", "three-kernels-graph", "three-kernels-plain"])
def test_iterate_in_pieces_equals_one_iterate_of_the_whole(options, pieces):
    whole, parts = relp_amd.Solver(**options).load_mps(AFIRO), relp_amd.Solver(**options).load_mps(AFIRO)
    try:
        fused = "pivot_kernels" not in options
        calls_whole, calls_parts = run_whole(whole), run_pieces(parts, PIECES[pieces])
        a, b = state(whole, calls_whole), state(parts, calls_parts)
        assert a == b
        assert a["stop_reasons"] == [relp_amd.STOP_NO_ENTERING] * 2 and a["pivots"][0] > 0 and a["pivots"][1] > 0
        per_batch = fused_launches(options["use_graph"]) if fused else (lambda n: 1 + 3 * n)
        assert whole.stats().launches == expected_launches(calls_whole, per_batch)
        assert parts.stats().launches == expected_launches(calls_parts, per_batch)
    finally:
        whole.close()
        parts.close()


def test_the_whole_solve_is_what_the_pieces_reach():
    """`solve_relaxation` (phase setup, polish, feasibility check, result read-backs through the pinned buffers) against the pieces."""
    solved, parts = relp_amd.Solver().load_mps(AFIRO), relp_amd.Solver().load_mps(AFIRO)
    try:
        result = solved.solve_relaxation()
        calls = run_pieces(parts, PIECES["issue"])
        got = state(parts, calls)
        assert result.kind == relp_amd.FINITE_OPTIMUM
        assert got["pivots"] == [result.pivots_phase_one, result.pivots_phase_two]
        assert got["basis"] == [int(v) for v in solved.basis()]
        fixed = relp_amd.Model(AFIRO).fixed_cost()
        assert abs(parts.objective_function_value() + fixed - result.objective) <= 1e-12 * max(1.0, abs(result.objective))
        # twice on one handle: the mirror and the read-back buffers are reused
        again = solved.solve_relaxation()
        assert (again.objective, again.pivots_phase_one, again.pivots_phase_two) == (result.objective, result.pivots_phase_one, result.pivots_phase_two)
    finally:
        solved.close()
        parts.close()


@pytest.mark.parametrize("options", [{}, {"pivot_kernels": 1}, {"carry": api.CARRY_LU}], ids=["fused", "three-kernels", "lu"])
def test_duplicated_equality_row_is_driven_out_or_reported(options):
    """x0 + x1 = 2 twice and x1 + x2 = 3, min x0 + 2 x1 + 3 x2: phase one ends with an artificial basic at zero on one of the two
    equal rows; `drive_out_artificials` -- a write of the control block, a row scan, a read, per artificial row -- finds no column
    to pivot it out with and reports the row redundant.  Optimum x = (0, 2, 1), objective 7."""
    solver = relp_amd.Solver(**options)
    try:
        solver.load_matrix_data([0, 2, 5, 6], [0, 1, 0, 1, 2, 2], [1] * 6, [1] * 6, b=[2, 2, 3], cost=[1, 2, 3], counts=(3, 0, 0, 0))
        result = solver.solve_relaxation()
        assert result.kind == relp_amd.FINITE_OPTIMUM
        assert result.objective == 7.0
        assert np.array_equal(solver.solution(), [0.0, 2.0, 1.0])
        basis = [int(v) for v in solver.basis()]
        artificial_rows = [i for i, column in enumerate(basis) if column < 0]
        assert len(artificial_rows) == 1 and artificial_rows[0] in (0, 1), basis  # the redundant row keeps its artificial
        assert basis[2] >= 0
    finally:
        solver.close()


@pytest.mark.parametrize("options", [{"carry": api.CARRY_LU}, {"carry": api.CARRY_LU_INVERSE, "lu_refactor": 1}], ids=["lu-host", "lui-device"])
def test_lu_carry_in_pieces_through_refactorisations(options):
    options = dict(options, refactor_period=4)
    whole, parts, solved = (relp_amd.Solver(**options).load_mps(AFIRO) for _ in range(3))
    try:
        calls_whole, calls_parts = run_whole(whole), run_pieces(parts, PIECES["small"])
        a = state(whole, calls_whole)
        assert a == state(parts, calls_parts)
        # every four updates the kernel asks for a refactorisation and `iterate` goes on after it: more pivots than that in both phases
        assert min(a["pivots"]) > 4
        result = solved.solve_relaxation()  # (the solve of the same handle counts them)
        assert result.kind == relp_amd.FINITE_OPTIMUM and result.refactors > 0
    finally:
        whole.close()
        parts.close()
        solved.close()


def test_network_carry_in_pieces():
    """The 48-vertex max-flow LP of tools/record_kernel_paths.py under the spanning-forest carry."""
    nr_vertices = 48
    tail, head, capacity = max_flow_graph(nr_vertices, 192)
    keep = (head != 0) & (tail != nr_vertices - 1)
    model = relp_amd.Model.max_flow(nr_vertices, list(zip(tail[keep].tolist(), head[keep].tolist(), capacity[keep].tolist())), 0, nr_vertices - 1)
    options = {"carry": api.CARRY_NETWORK, "implicit_bounds": 1}
    whole, parts = relp_amd.Solver(**options).load_model(model), relp_amd.Solver(**options).load_model(model)
    try:
        calls_whole, calls_parts = run_whole(whole), run_pieces(parts, PIECES["issue"])
        a = state(whole, calls_whole)
        assert a == state(parts, calls_parts)
        assert sum(a["pivots"]) > 0
        assert whole.bound_flips() == parts.bound_flips()
    finally:
        whole.close()
        parts.close()
