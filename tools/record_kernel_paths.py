"""Fingerprints of every kernel path a loaded LP can take (tests/golden/kernel_path_fingerprints.json).

The host code that chooses the kernels of a handle (``plan_kernel_path``, relp_amd/csrc/kernel_path.hpp) is pinned from outside: a fixed
list of small cases, each reaching one branch of that choice, is loaded and driven through the public Python API only, so this file runs
unchanged before and after a change of the host code.  Per case:

  level A  straight after the load, from ``record()``: device rows, artificials, carry, ratio rule, where the LU refactorises, the bytes
           on the device and the two bytes-per-pivot figures;
  level B  after ``solve_relaxation()`` (the small LPs) or ``begin_phase_one()`` + ``iterate(100)`` (the diagonal LPs: that crosses a
           batch edge, an eta consolidation and an LU refactorisation): result kind, pivots per phase, polishes, refactors, kernel
           launches, device bytes, the objective as ``float.hex()`` and the basis (as a digest); for ``iterate`` also ``done`` and ``stop_reason``.

  python tools/record_kernel_paths.py record OUT.json        one run on the GPU
  python tools/record_kernel_paths.py table OUT.json         the load-time plan of every case (no device; written once the fingerprints
                                                             of a change match those recorded before it)
  python tools/record_kernel_paths.py merge A.json B.json OUT.json
        two runs of the same code into the golden file: level A must agree everywhere; a level-B field that differs between the two
        runs is named under "unstable" in its case and dropped from that case only.

tests/test_gpu_kernel_paths.py replays ``CASES`` against the golden file; tests/test_kernel_path_host.py plans the same cases without a device.
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import relp_amd  # noqa: E402
from relp_amd import api  # noqa: E402
from relp_amd.workloads import dense_lp, max_flow_graph  # noqa: E402

LEVEL_A = ("device_rows", "artificials", "carry", "ratio_rule", "lu_refactor", "device_bytes", "pricing_bytes_per_pivot", "inverse_bytes_per_pivot_bound")
LU, LU_INVERSE, NETWORK = api.CARRY_LU, api.CARRY_LU_INVERSE, api.CARRY_NETWORK
REFACTOR_DEVICE, REFACTOR_HOST, REFACTOR_DEVICE_ASYNC = 1, 2, 3

_models = {}


def _dense(m, n):
    a, b, c = dense_lp(m, n)  # A x <= b, min c x
    columns = [[(i, int(a[j, i])) for i in range(m)] for j in range(n)]
    return relp_amd.Model.from_general_form(columns, ["Less"] * m, [int(v) for v in b], [(int(v), 0, None) for v in c])


def _diagonal(m):
    """The LP of tests/test_gpu_large_rows.py without its upper bounds: row i is x_i - z_i = b_i, min sum x."""
    columns = [[(i, 1)] for i in range(m)] + [[(i, -1)] for i in range(m)]
    b = [1 if i % 100 == 0 else 0 for i in range(m)]
    return relp_amd.Model.from_general_form(columns, ["Equal"] * m, b, [(1, 0, None)] * m + [(0, 0, None)] * m)


def _max_flow():
    nr_vertices = 48
    tail, head, capacity = max_flow_graph(nr_vertices, 192)
    keep = (head != 0) & (tail != nr_vertices - 1)
    arcs = list(zip(tail[keep].tolist(), head[keep].tolist(), capacity[keep].tolist()))
    return relp_amd.Model.max_flow(nr_vertices, arcs, 0, nr_vertices - 1)


_BUILDERS = {
    "afiro": lambda: relp_amd.Model(os.path.join(ROOT, "data", "netlib", "AFIRO.SIF")),
    "kb2": lambda: relp_amd.Model(os.path.join(ROOT, "data", "netlib", "KB2.SIF")),  # variable bounds (tests/test_gpu_bounded.py)
    "dense64": lambda: _dense(64, 128),
    "dense65": lambda: _dense(65, 130),
    "diag1100": lambda: _diagonal(1100),
    "diag2100": lambda: _diagonal(2100),
    "diag7000": lambda: _diagonal(7000),
    "diag8400": lambda: _diagonal(8400),
    "maxflow": _max_flow,
}


def model(name):
    """The host model of a case, built once per process."""
    if name not in _models:
        _models[name] = _BUILDERS[name]()
    return _models[name]


def _case(name, lp, run="solve", **options):
    return {"name": name, "model": lp, "run": run, "options": options}


# run: "solve" = solve_relaxation(); "iterate" = begin_phase_one() + iterate(100); "load" = level A only (counters depend on timing);
#      "refused" = the load must fail (status and text recorded), then AFIRO loads and solves on the same handle (under
#                  RELP_CARRY_NETWORK, which refuses AFIRO itself, the max-flow LP);
#      "reload" = the case's LP, then AFIRO, on one handle.
CASES = [
    _case("afiro", "afiro"),
    _case("afiro-three-kernels", "afiro", pivot_kernels=1),
    _case("afiro-ftran-slices", "afiro", ftran_min_nnz=3),  # (AFIRO's longest column has 4 entries: multi-block FTRAN without a dense block)
    _case("afiro-crash", "afiro", crash=1),
    _case("afiro-harris", "afiro", ratio_rule=api.RATIO_HARRIS),
    _case("afiro-textbook", "afiro", ratio_rule=api.RATIO_TEXTBOOK),
    _case("afiro-auto", "afiro", ratio_rule=api.RATIO_AUTO),
    _case("afiro-lu-host", "afiro", carry=LU, lu_refactor=REFACTOR_HOST),
    _case("afiro-lu-device", "afiro", carry=LU, lu_refactor=REFACTOR_DEVICE),
    _case("afiro-lui-host", "afiro", carry=LU_INVERSE, lu_refactor=REFACTOR_HOST),
    _case("afiro-lui-device", "afiro", carry=LU_INVERSE, lu_refactor=REFACTOR_DEVICE),
    _case("afiro-lui-device-async", "afiro", run="load", carry=LU_INVERSE, lu_refactor=REFACTOR_DEVICE_ASYNC),
    _case("kb2-bounded", "kb2", implicit_bounds=1),
    _case("kb2-bounded-lu", "kb2", implicit_bounds=1, carry=LU),
] + [
    _case("dense64-storage%d-%s" % (storage, "rows" if switches else "lane"), "dense64", dense_storage=storage, switches=switches)
    for storage in (0, 1, 2) for switches in (0, api.SW_NO_DENSE_LANE)
] + [
    _case("dense64-eta", "dense64", ftran_min_nnz=16),
    _case("dense64-eta-no-slack-in-btran", "dense64", ftran_min_nnz=16, switches=api.SW_NO_SLACK_IN_BTRAN),
    _case("dense64-rank-one", "dense64", ftran_min_nnz=16, product_form=1),
    _case("dense65-odd", "dense65", ftran_min_nnz=16),
    _case("diag2100", "diag2100", run="iterate"),
    _case("diag7000-network", "diag7000", run="iterate", carry=NETWORK),
    _case("diag7000-no-generated-columns", "diag7000", run="iterate", switches=api.SW_NO_GENERATED_COLUMNS),
    _case("diag7000-no-rho-bits", "diag7000", run="iterate", switches=api.SW_NO_RHO_BITS),
    _case("diag7000-unit-pairs", "diag7000", run="iterate", switches=api.SW_PRICE_UNIT_PAIRS),
    _case("diag7000-ell-wide", "diag7000", run="iterate", switches=api.SW_ELL_WIDE),
    _case("diag8400", "diag8400", run="iterate"),
    _case("diag8400-k2-single", "diag8400", run="iterate", switches=api.SW_K2_SINGLE),
    _case("maxflow-network", "maxflow", carry=NETWORK, implicit_bounds=1),  # (the capacities are upper bounds)
    _case("refused-network-afiro", "afiro", run="refused", carry=NETWORK, implicit_bounds=1),  # (then the max-flow LP: AFIRO has no forest)
    _case("refused-lui-8400", "diag8400", run="refused", carry=LU_INVERSE),
    _case("refused-lu-8400", "diag8400", run="refused", carry=LU, refactor_period=63),  # (the default period of 31 fits up to about 8700 rows)
    _case("refused-textbook-8400", "diag8400", run="refused", ratio_rule=api.RATIO_TEXTBOOK),
    _case("reload-dense64-then-afiro", "dense64", run="reload"),
]
CASE_BY_NAME = {case["name"]: case for case in CASES}
# The kernel instantiations the plan names that no case above reaches (tests/golden/kernel_choice_fingerprints.json, recorded with the
# library of the commit before the plan named them; replayed by tests/test_gpu_kernel_choice.py).  They are in the table of plans too.
CHOICE_CASES = [
    _case("afiro-gemm-vector", "afiro", switches=api.SW_GEMM_VECTOR),  # (the polish GEMM on plain FMAs)
    _case("diag1100", "diag1100", run="iterate"),  # (between 1024 and 2048 rows: four rows per thread in the fused pivot and the ratio test)
    _case("diag2100-no-touched", "diag2100", run="iterate", switches=api.SW_NO_TOUCHED),  # (the predicated update on its plain grid)
]
REFUSED = [case for case in CASES if case["run"] == "refused"]


def _basis_digest(basis):
    """The basis (provider column per row, -1 - k for artificial k): verbatim below 100 rows, else its length and the SHA-256 of its text."""
    basis = [int(v) for v in basis]
    return basis if len(basis) < 100 else "%d:%s" % (len(basis), hashlib.sha256(",".join(map(str, basis)).encode()).hexdigest())


def _level_a(solver):
    record = solver.record()
    return {key: record[key] for key in LEVEL_A}


def _solve(solver):
    result = solver.solve_relaxation()
    record = solver.record()
    return {"result": int(result.kind), "pivots_phase_one": int(result.pivots_phase_one), "pivots_phase_two": int(result.pivots_phase_two),
            "polishes": int(result.polishes), "refactors": int(result.refactors), "kernel_launches": record["kernel_launches"],
            "device_bytes": record["device_bytes"], "objective": float(result.objective).hex(), "basis": _basis_digest(solver.basis())}


def _iterate(solver):
    solver.begin_phase_one()
    done, reason = solver.iterate(100)
    objective = solver.objective_function_value()
    record = solver.record()
    return {"done": int(done), "stop_reason": int(reason), "polishes": record["polishes"], "refactors": record["refactors"],
            "kernel_launches": int(solver.stats().launches), "device_bytes": record["device_bytes"], "objective": float(objective).hex(),
            "basis": _basis_digest(solver.basis())}


def run_case(case):
    """Drives one case on the GPU; returns its entry of the fingerprint file."""
    solver = relp_amd.Solver(certify=0, **case["options"])
    try:
        entry = {}
        if case["run"] == "refused":
            try:
                solver.load_model(model(case["model"]))
                entry["refusal"] = None
            except relp_amd.RelpError as error:
                entry["refusal"] = {"status": error.status, "message": api.lib().relp_last_error(solver._h).decode()}
            solver.load_model(model("maxflow" if case["options"].get("carry") == NETWORK else "afiro"))
            entry["A"] = _level_a(solver)
            entry["B"] = _solve(solver)
            return entry
        solver.load_model(model(case["model"]))
        entry["A"] = _level_a(solver)
        if case["run"] == "solve":
            entry["B"] = _solve(solver)
        elif case["run"] == "iterate":
            entry["B"] = _iterate(solver)
        elif case["run"] == "reload":
            entry["B"] = _solve(solver)
            solver.load_model(model("afiro"))
            entry["A_after_reload"] = _level_a(solver)
            entry["B_after_reload"] = _solve(solver)
        return entry
    finally:
        solver.close()


def _write(path, entries):
    """One case per line (the bases of the diagonal LPs are long)."""
    with open(path, "w") as handle:
        handle.write("{\n" + ",\n".join("%s: %s" % (json.dumps(name), json.dumps(entries[name], sort_keys=True, separators=(",", ":")))
                                       for name in sorted(entries)) + "\n}\n")


def record(path):
    import time
    out = {}
    try:  # (an error that is not the refusal a case expects ends the run: nothing more is started on the device after it)
        for case in CASES:
            t0 = time.time()
            out[case["name"]] = run_case(case)
            print("%-34s %.2f s" % (case["name"], time.time() - t0), flush=True)
    finally:
        _write(path, out)


def merge(path_a, path_b, path_out):
    with open(path_a) as handle:
        first = json.load(handle)
    with open(path_b) as handle:
        second = json.load(handle)
    assert sorted(first) == sorted(second) == sorted(CASE_BY_NAME)
    for name, entry in first.items():
        other = second[name]
        for key in entry:
            if not key.startswith("B"):
                assert entry[key] == other[key], "level A of %s differs between the two runs: %r / %r" % (name, entry[key], other[key])
        for key in [k for k in entry if k.startswith("B")]:
            unstable = sorted(field for field in entry[key] if entry[key][field] != other[key][field])
            for field in unstable:
                print("unstable: %s %s.%s: %r / %r" % (name, key, field, entry[key][field], other[key][field]))
                del entry[key][field]
            if unstable:
                entry.setdefault("unstable", []).extend(key + "." + field for field in unstable)
    _write(path_out, first)


def table(path):
    """The plan of every case that loads (tests/golden/kernel_path_table.json); needs no device."""
    _write(path, {case["name"]: model(case["model"]).kernel_path(**case["options"]) for case in CASES + CHOICE_CASES if case["run"] != "refused"})


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "record":
        record(sys.argv[2])
    elif len(sys.argv) == 3 and sys.argv[1] == "table":
        table(sys.argv[2])
    elif len(sys.argv) == 5 and sys.argv[1] == "merge":
        merge(*sys.argv[2:])
    else:
        sys.exit(__doc__)
