"""Fingerprints of small LPs that reach every load path of price_kernel, the k2f_* front half and pivot_fused_kernel
(tests/golden/round_trip_fingerprints.json).

The load phases of those kernels were regrouped so that each memory round trip is issued whole (clamped addresses, values dropped by
selects, entries 8 .. 23 of a long column fetched with the column).  Not one floating-point operation may change with that, and
tests/test_gpu_fused.py cannot tell: it compares two pivot paths that share the changed templates.  So the golden file was recorded
with the library of the commit BEFORE the regrouping (``RELP_AMD_LIB`` names it), twice, and tests/test_gpu_round_trips.py replays
the cases against it with the library of the tree.

The LPs are seeded integer programs through ``Model.from_general_form``: ``A x = b`` with ``b = A x0`` for an integer ``x0 >= 0``,
entries in +-{1, 2, 3}, costs >= 0 -- feasible and bounded by construction; ``record`` stops at a case that does not end at a finite
optimum.  Shapes (the smallest at which the new load code can go wrong):

  rows      m in ROWS, n = max(40, 2 m), columns of 1-5 entries: lanes and waves past m, waves without a column of the inverse,
            two / four rows per thread in the fused pivot, 2 / 4 / 8 per thread in the three-kernel ratio test
  length    m = 40, every column of length L in LENGTHS, and one LP whose columns cycle through 1, 9, 17, 25 entries so that every
            pricing wave holds them side by side: the padded width and each further eight
  blocks    m = 16, n chosen so that the plan's ``price_blocks`` is 1, 2, 128, 129, 512, 513 (asserted): inline candidate columns
            on / off, the second pass of the candidate loop; and 1024 with more columns than one pass prices
  each of them on the default path and with ``pivot_kernels=1``; one case of more than 64 pivots under graph replay and without.

  python tools/record_round_trip_cases.py record OUT.json         one run on the GPU
  python tools/record_round_trip_cases.py merge A.json B.json OUT.json
        two runs of the same library into the golden file; a field that differs between them is named under "unstable" in its case
        and not compared.
  python tools/record_round_trip_cases.py plan                    price_blocks of the `blocks` cases (no device)
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import relp_amd  # noqa: E402

ROWS = (1, 7, 8, 9, 63, 64, 65, 512, 513, 1024, 1025, 2047, 2048)
LENGTHS = (8, 9, 16, 17, 24, 25, 40)
MIXED = (1, 9, 17, 25)
BLOCKS = {1: 8, 2: 40, 128: 4072, 129: 4104, 512: 16360, 513: 16392}  # price_blocks -> n at m = 16 (`plan` prints them)
TWO_PASSES = 32808  # ... and n past the 1024 workgroups the plan stops at: some of them price a second set of columns

_models = {}


def integer_lp(m, n, lengths, seed):
    """min c x, A x = A x0, x >= 0: column j has lengths[j % len(lengths)] entries (at most m) in +-{1, 2, 3}, c >= 0, x0 in 0 .. 3."""
    rng = np.random.RandomState(seed)
    columns, b = [], np.zeros(m, dtype=np.int64)
    x0 = rng.randint(0, 4, size=n)
    for j in range(n):
        k = min(int(lengths[j % len(lengths)]), m)
        rows = np.sort(rng.choice(m, size=k, replace=False))
        values = rng.randint(1, 4, size=k) * rng.choice((-1, 1), size=k)
        columns.append([(int(i), int(v)) for i, v in zip(rows, values)])
        b[rows] += values * x0[j]
    cost = rng.randint(0, 10, size=n)
    return relp_amd.Model.from_general_form(columns, ["Equal"] * m, [int(v) for v in b], [(int(c), 0, None) for c in cost])


def _builders():
    out = {}
    for m in ROWS:
        out["rows%d" % m] = (m, max(40, 2 * m), (1, 2, 3, 4, 5), 1000 + m)
    for length in LENGTHS:
        out["length%d" % length] = (40, 80, (length,), 2000 + length)
    out["length-mixed"] = (40, 96, MIXED, 2999)
    for blocks, n in BLOCKS.items():
        out["blocks%d" % blocks] = (16, n, (1, 2, 3, 4, 5), 3000 + blocks)
    out["blocks1024-two-passes"] = (16, TWO_PASSES, (1, 2, 3, 4, 5), 3999)
    return out


BUILDERS = _builders()


def model(name):
    """The host model of a case, built once per process."""
    if name not in _models:
        _models[name] = integer_lp(*BUILDERS[name])
    return _models[name]


def _case(name, lp, **options):
    return {"name": name, "model": lp, "options": options}


CASES = [_case(lp + suffix, lp, **options) for lp in BUILDERS for suffix, options in (("", {}), ("-three-kernels", {"pivot_kernels": 1}))] + [
    _case("rows513-graph", "rows513", use_graph=1),  # (more than 64 pivots: the batch edge under graph replay, and without)
    _case("rows513-no-graph", "rows513", use_graph=0),
]
CASE_BY_NAME = {case["name"]: case for case in CASES}
MANY_PIVOTS = ("rows513-graph", "rows513-no-graph")


def _digest(array):
    return hashlib.sha256(np.ascontiguousarray(array).tobytes()).hexdigest()


def run_case(case):
    """Drives one case on the GPU; returns its entry of the fingerprint file."""
    solver = relp_amd.Solver(certify=0, **case["options"])
    try:
        solver.load_model(model(case["model"]))
        result = solver.solve_relaxation()
        record = solver.record()
        m = solver.m
        basis = [int(v) for v in solver.basis()]
        inverse = np.concatenate([solver.basis_inverse_row((k * (m - 1)) // 6) for k in range(7)])
        return {"result": int(result.kind), "pivots_phase_one": int(result.pivots_phase_one), "pivots_phase_two": int(result.pivots_phase_two),
                "objective": float(result.objective).hex(), "basis": "%d:%s" % (len(basis), hashlib.sha256(",".join(map(str, basis)).encode()).hexdigest()),
                "solution": _digest(solver.solution()), "inverse_rows": _digest(inverse),
                "kernel_launches": record["kernel_launches"], "device_bytes": record["device_bytes"]}
    finally:
        solver.close()


def _write(path, entries):
    with open(path, "w") as handle:
        handle.write("{\n" + ",\n".join("%s: %s" % (json.dumps(name), json.dumps(entries[name], sort_keys=True, separators=(",", ":")))
                                       for name in sorted(entries)) + "\n}\n")


def record(path):
    import time
    out = {}
    try:  # (an error ends the run: nothing more is started on the device after it)
        for case in CASES:
            t0 = time.time()
            entry = out[case["name"]] = run_case(case)
            print("%-28s %.2f s  pivots %d + %d" % (case["name"], time.time() - t0, entry["pivots_phase_one"], entry["pivots_phase_two"]), flush=True)
            if entry["result"] != relp_amd.FINITE_OPTIMUM:
                raise SystemExit("%s does not end at a finite optimum: %r" % (case["name"], entry))
            if case["name"] in MANY_PIVOTS and entry["pivots_phase_one"] + entry["pivots_phase_two"] <= 64:
                raise SystemExit("%s makes no more than 64 pivots" % case["name"])
    finally:
        _write(path, out)


def merge(path_a, path_b, path_out):
    with open(path_a) as handle:
        first = json.load(handle)
    with open(path_b) as handle:
        second = json.load(handle)
    assert sorted(first) == sorted(second) == sorted(CASE_BY_NAME)
    for name, entry in first.items():
        unstable = sorted(field for field in entry if entry[field] != second[name][field])
        for field in unstable:
            print("unstable: %s.%s: %r / %r" % (name, field, entry[field], second[name][field]))
            del entry[field]
        if unstable:
            entry["unstable"] = unstable
    _write(path_out, first)


def plan():
    for name in BUILDERS:
        if name.startswith("blocks"):
            print(name, BUILDERS[name][1], model(name).kernel_path()["price_blocks"], model(name).kernel_path(pivot_kernels=1)["price_blocks"])


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "record":
        record(sys.argv[2])
    elif len(sys.argv) == 5 and sys.argv[1] == "merge":
        merge(*sys.argv[2:])
    elif len(sys.argv) == 2 and sys.argv[1] == "plan":
        plan()
    else:
        sys.exit(__doc__)
