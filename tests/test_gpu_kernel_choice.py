"""The instantiations the load-time plan names (``KernelPath``: ratio_kernel, fused_rows, update_kernel, price_kernel), run on each
side of every row count at which the plan takes another one: 1024 | 1025 (two / four rows per thread in the fused pivot and the
register-resident ratio test), 2048 | 2049 (the last fused size; four / eight rows per thread; the update reads whole columns /
predicates its loads), 4096 | 4097 (eight / sixteen rows per thread; pricing stages its vectors in LDS / gathers them), 8192 | 8193
(sixteen rows per thread / the ratio test across workgroups; generated columns at both).

The diagonal LP of tools/record_kernel_paths.py (row i: x_i - z_i = b_i, b_i = 1 on every 100th row, min sum x) has a closed form
for the first pivots of phase one.  Every x_i prices at cbar = -1 with the steepest-edge weight 2, so all keys are equal, and equal
keys go to the larger column (price_step.hpp): x_{m-1} enters first, on row m-1, the only row of its column, and the artificial of
that row leaves; no z_i is ever a candidate (its reduced cost is 1 while the artificial of its row is basic, 0 after).  After 100
pivots the basis is x_i on the rows i >= m - 100 and the artificial -1 - i on every other row, and the phase-one objective is the
sum of b_i over the rows that still hold their artificial.  100 pivots are a batch of 64 and one of 36, not replayed from a graph:
``stats().launches`` must be what the plan counts for them.

``CHOICE_CASES`` of tools/record_kernel_paths.py reach the instantiations that none of its ``CASES`` does; they are replayed as
tests/test_gpu_kernel_paths.py replays those, against fingerprints recorded before the plan named the instantiations."""
import importlib.util
import json
import os

import pytest

import relp_amd

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_kernel_paths", os.path.join(ROOT, "tools", "record_kernel_paths.py"))
recorder = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(recorder)
with open(os.path.join(ROOT, "tests", "golden", "kernel_choice_fingerprints.json")) as handle:
    GOLDEN = json.load(handle)
PIVOTS, BATCH = 100, 64


def test_the_golden_file_has_every_choice_case():
    assert sorted(GOLDEN) == sorted(case["name"] for case in recorder.CHOICE_CASES)


@pytest.mark.parametrize("case", recorder.CHOICE_CASES, ids=[case["name"] for case in recorder.CHOICE_CASES])
def test_choice_case_fingerprint(case):
    expected = dict(GOLDEN[case["name"]])
    assert "unstable" not in expected  # (no field differed between the two recordings)
    entry = recorder.run_case(case)
    assert sorted(entry) == sorted(expected)
    for level in expected:
        assert entry[level] == expected[level], level


@pytest.mark.parametrize("m", [1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193])
def test_diagonal_lp_on_each_side_of_every_edge(m):
    model = recorder._diagonal(m)
    options = dict(use_graph=0, pivots_per_launch=BATCH)
    plan = model.kernel_path(**options)
    solver = relp_amd.Solver(certify=0, **options)
    try:
        solver.load_model(model)
        solver.begin_phase_one()
        done, reason = solver.iterate(PIVOTS)
        objective = solver.objective_function_value()
        basis = [int(v) for v in solver.basis()]
        launches = int(solver.stats().launches)
    finally:
        solver.close()
    print("m = %d: %s / %s, fused_rows %d, %s, %s; done %d, reason %d, objective %r, launches %d" % (
        m, plan["ratio_kernel"], plan["ratio_kernel_no_change"], plan["fused_rows"], plan["update_kernel"], plan["price_kernel"], done, reason,
        objective, launches))
    assert (done, reason) == (PIVOTS, 3)  # the budget ran out: phase one has m - 100 pivots to go
    assert basis == [i if i >= m - PIVOTS else -1 - i for i in range(m)]
    assert objective == float(sum(1 for i in range(m - PIVOTS) if i % 100 == 0))  # (small integers: exact in f64)
    batches = [BATCH, PIVOTS - BATCH]
    assert launches == sum(plan["launches_per_batch"] + plan["launches_per_pivot"] * count for count in batches)
