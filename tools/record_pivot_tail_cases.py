"""Fingerprints of small LPs at the ends of a pivot that tests/test_gpu_round_trips.py does not reach
(tests/golden/pivot_tail_fingerprints.json).

The fused pivot kernel gave the bookkeeping of a pivot to a workgroup that owns no column of the inverse, its column-owning workgroups
stopped waiting for the pivot row's broadcast, the combined reduction of the k2f_* front half lost a ladder and a barrier, and the
arg-max of the entering column and of Harris pass 2 their opening barriers.  Not one bit of a result may move with that, and
tests/test_gpu_fused.py cannot tell where both pivot paths share the change.  So the golden file was recorded with the library of the commit BEFORE the change
(``RELP_AMD_LIB`` names it), twice, and tests/test_gpu_pivot_tail.py replays the cases against it with the library of the tree.

Seeded integer LPs through ``Model.from_general_form``, each on the default path and with ``pivot_kernels=1``:

  endings   m = 9, n = 40: what only the writer handles.  `unbounded`: a feasible LP plus one column that negates another one, of a
            cost that makes the pair a ray of negative cost.  `infeasible`: the first row once more, with another right-hand side.
            Both through ``solve_relaxation``.
  budget    the `rows65` LP of tools/record_round_trip_cases.py, whose first phase takes 77 pivots: ``begin_phase_one()``, then
            ``iterate(k)``, for each k in BUDGETS from the start; with graph replay and with ``use_graph=0``.  After the call: pivots
            made, stop reason, basis, the bits of x_B and of the objective.  1, 63, 64 and 65 use their budget up on either side of
            the edge of a batch of 64 -- the hand-on of a used-up budget, the control block's passage through both state copies --
            and 129 ends the phase inside its second batch, whose remaining launches hand the state on untouched.
  ties      m = 8, n = 96: columns in identical twins (same entries, same cost), which keep equal reduced costs and weights until one
            of them enters; the twin of column j stands 1, 8 or 32 columns behind it -- the neighbouring lane group of a pricing
            wave, another wave, another pricing workgroup -- under steepest edge and under Dantzig, whose tie rules are opposite.
            One pivot per ``iterate(1)``; the fingerprint is the basis after every pivot.  `twin_ties` counts the pivots whose
            entering column had its twin non-basic at that moment (worked out here, on the host, from the bases): `record` tries
            seeds until there is one, and keeps the seed in SEEDS below.

  python tools/record_pivot_tail_cases.py record OUT.json         one run on the GPU
  python tools/record_pivot_tail_cases.py merge A.json B.json OUT.json
        two runs of the same library into the golden file; a field that differs between them is named under "unstable" in its case
        and not compared.
"""
import hashlib
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import relp_amd  # noqa: E402

_spec = importlib.util.spec_from_file_location("record_round_trip_cases", os.path.join(ROOT, "tools", "record_round_trip_cases.py"))
round_trip = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(round_trip)

BUDGETS = (1, 63, 64, 65, 129)
DISTANCES = (1, 8, 32)
RULES = {"steepest": relp_amd.STEEPEST_EDGE, "dantzig": relp_amd.DANTZIG}
TIE_M, TIE_N = 8, 96
END_M, END_N = 9, 40
MAX_PIVOTS = 2000
# the seed of each tie LP: the first of 5000 + 100 d, ... at which some entering column has its twin non-basic under both rules and on
# both paths (`record` asserts it, and prints the seed to put here when it has to move on)
SEEDS = {1: 5100, 8: 5800, 32: 8200}

_models = {}


def _columns(rng, m, n, lengths=(1, 2, 3, 4, 5)):
    columns = []
    for j in range(n):
        k = min(int(lengths[j % len(lengths)]), m)
        rows = np.sort(rng.choice(m, size=k, replace=False))
        values = rng.randint(1, 4, size=k) * rng.choice((-1, 1), size=k)
        columns.append([(int(i), int(v)) for i, v in zip(rows, values)])
    return columns


def _right_hand_side(m, columns, x0):
    b = [0] * m
    for column, x in zip(columns, x0):
        for i, v in column:
            b[i] += v * int(x)
    return b


def _general_form(m, columns, b, cost):
    return relp_amd.Model.from_general_form(columns, ["Equal"] * m, [int(v) for v in b], [(int(c), 0, None) for c in cost])


def unbounded_lp():
    """A x = A x0 over 39 columns, and a 40th that negates column 0 at a cost below -c_0: x_0 and x_39 grow together for ever."""
    rng = np.random.RandomState(4001)
    columns = _columns(rng, END_M, END_N - 1)
    x0 = rng.randint(0, 4, size=END_N - 1)
    cost = [int(c) for c in rng.randint(0, 10, size=END_N - 1)]
    b = _right_hand_side(END_M, columns, x0)
    columns.append([(i, -v) for i, v in columns[0]])
    cost.append(-cost[0] - 1)
    return _general_form(END_M, columns, b, cost)


def infeasible_lp():
    """A x = A x0 over eight rows, and row 0 once more with a right-hand side one larger."""
    rng = np.random.RandomState(4002)
    columns = _columns(rng, END_M - 1, END_N)
    x0 = rng.randint(0, 4, size=END_N)
    cost = rng.randint(0, 10, size=END_N)
    b = _right_hand_side(END_M - 1, columns, x0)
    columns = [column + [(END_M - 1, v) for i, v in column if i == 0] for column in columns]
    return _general_form(END_M, columns, b + [b[0] + 1], cost)


def twin_of(j, distance, n=TIE_N):
    """The column with the entries and the cost of column j, or None: whole groups of 2 d columns pair j with j + d, the rest stand alone."""
    if j >= (n // (2 * distance)) * 2 * distance:
        return None
    return j + distance if j % (2 * distance) < distance else j - distance


def tie_lp(distance, seed):
    rng = np.random.RandomState(seed)
    columns, cost = [None] * TIE_N, [0] * TIE_N
    for j in range(TIE_N):
        twin = twin_of(j, distance)
        if twin is not None and twin < j:
            columns[j], cost[j] = list(columns[twin]), cost[twin]
        else:
            columns[j], cost[j] = _columns(rng, TIE_M, 1, lengths=(int(rng.randint(1, 6)),))[0], int(rng.randint(0, 10))
    x0 = rng.randint(0, 4, size=TIE_N)
    return _general_form(TIE_M, columns, _right_hand_side(TIE_M, columns, x0), cost)


BUILDERS = {"unbounded": unbounded_lp, "infeasible": infeasible_lp, "rows65": lambda: round_trip.model("rows65")}
for _d in DISTANCES:
    BUILDERS["twins%d" % _d] = (lambda d: lambda: tie_lp(d, SEEDS[d]))(_d)


def model(name):
    """The host model of a case, built once per process."""
    if name not in _models:
        _models[name] = BUILDERS[name]()
    return _models[name]


def _case(name, kind, lp, **options):
    return {"name": name, "kind": kind, "model": lp, "options": options}


PATHS = (("", {}), ("-three-kernels", {"pivot_kernels": 1}))
CASES = [_case(lp + suffix, "ending", lp, **options) for lp in ("unbounded", "infeasible") for suffix, options in PATHS] + [
    _case("budget-%s%s" % (graph, suffix), "budget", "rows65", use_graph=flag, **options)
    for graph, flag in (("graph", 1), ("no-graph", 0)) for suffix, options in PATHS] + [
    _case("twins%d-%s%s" % (d, rule, suffix), "ties", "twins%d" % d, pivot_rule=RULES[rule], **options)
    for d in DISTANCES for rule in sorted(RULES) for suffix, options in PATHS]
CASE_BY_NAME = {case["name"]: case for case in CASES}
ENDING_KIND = {"unbounded": relp_amd.UNBOUNDED, "infeasible": relp_amd.INFEASIBLE}


def _digest(array):
    return hashlib.sha256(np.ascontiguousarray(array).tobytes()).hexdigest()


def _basis(solver):
    return " ".join(str(int(v)) for v in solver.basis())


def _run_ending(solver):
    result = solver.solve_relaxation()
    record = solver.record()
    return {"result": int(result.kind), "pivots_phase_one": int(result.pivots_phase_one), "pivots_phase_two": int(result.pivots_phase_two),
            "basis": _basis(solver), "x_B": _digest(solver.b()), "objective": float(solver.objective_function_value()).hex(),
            "kernel_launches": record["kernel_launches"], "device_bytes": record["device_bytes"]}


def _run_budget(case):
    calls, launches = [], []
    for asked in BUDGETS:  # each from the start of phase one, in a solver of its own
        solver = relp_amd.Solver(certify=0, **case["options"])
        try:
            solver.load_model(model(case["model"]))
            solver.begin_phase_one()
            done, reason = solver.iterate(asked)
            calls.append({"asked": asked, "done": int(done), "reason": int(reason), "basis": _digest(solver.basis()),
                          "x_B": _digest(solver.b()), "objective": float(solver.objective_function_value()).hex()})
            launches.append(solver.record()["kernel_launches"])
        finally:
            solver.close()
    return {"calls": calls, "kernel_launches": launches}


def twin_ties(bases, entered, n_art, distance):
    """How many pivots brought in a column whose twin was non-basic in the basis the pivot started from (columns: device index space,
    the artificial ones first)."""
    count = 0
    for before, q in zip(bases, entered):
        twin = twin_of(q - n_art, distance) if q >= n_art else None
        if twin is not None and twin + n_art not in before:
            count += 1
    return count


def _run_ties(solver, distance):
    solver.begin_phase_one()
    bases, entered = [[int(v) for v in solver.basis()]], []
    for phase in (1, 2):
        while True:
            done, reason = solver.iterate(1)
            if done == 0:
                break
            entered.append(int(solver.last_pivot()[1]))
            bases.append([int(v) for v in solver.basis()])
            if len(entered) >= MAX_PIVOTS:
                raise SystemExit("more than %d pivots" % MAX_PIVOTS)
        if phase == 1:
            if reason != relp_amd.STOP_NO_ENTERING or abs(solver.objective_function_value()) > 1e-9:
                break
            solver.begin_phase_two()
    return {"bases": [" ".join(map(str, basis)) for basis in bases], "last_reason": int(reason),
            "objective": float(solver.objective_function_value()).hex(),
            "seed": SEEDS[distance], "twin_ties": twin_ties(bases, entered, solver.n_art, distance)}


def run_case(case):
    """Drives one case on the GPU; returns its entry of the fingerprint file."""
    if case["kind"] == "budget":
        return _run_budget(case)
    solver = relp_amd.Solver(certify=0, **case["options"])
    try:
        solver.load_model(model(case["model"]))
        if case["kind"] == "ending":
            return _run_ending(solver)
        assert solver.n_provider == TIE_N and solver.m == TIE_M
        return _run_ties(solver, int(case["model"][len("twins"):]))
    finally:
        solver.close()


def _write(path, entries):
    with open(path, "w") as handle:
        handle.write("{\n" + ",\n".join("%s: %s" % (json.dumps(name), json.dumps(entries[name], sort_keys=True, separators=(",", ":")))
                                       for name in sorted(entries)) + "\n}\n")


def _find_seeds():
    """Moves SEEDS[d] on to the first seed at which every case of distance d has a tie between twins."""
    for d in DISTANCES:
        for seed in range(SEEDS[d], SEEDS[d] + 50):
            SEEDS[d] = seed
            _models.pop("twins%d" % d, None)
            ties = [run_case(case)["twin_ties"] for case in CASES if case["model"] == "twins%d" % d]
            print("twins%d seed %d: twin ties %r" % (d, seed, ties), flush=True)
            if min(ties) > 0:
                break
        else:
            raise SystemExit("no seed with a tie between twins at distance %d" % d)
    print("SEEDS = %r" % SEEDS, flush=True)


def record(path):
    import time
    out = {}
    try:  # (an error ends the run: nothing more is started on the device after it)
        _find_seeds()
        for case in CASES:
            t0 = time.time()
            entry = out[case["name"]] = run_case(case)
            print("%-32s %.2f s" % (case["name"], time.time() - t0), flush=True)
            if case["kind"] == "ending" and entry["result"] != ENDING_KIND[case["model"]]:
                raise SystemExit("%s ends as %r" % (case["name"], entry))
            if case["kind"] == "budget":
                print("    " + ", ".join("%d: %d (%d)" % (call["asked"], call["done"], call["reason"]) for call in entry["calls"]))
                if [call["reason"] for call in entry["calls"]] != [relp_amd.STOP_BUDGET] * 4 + [relp_amd.STOP_NO_ENTERING]:
                    raise SystemExit("%s: 1, 63, 64 and 65 must use their budget up and 129 end the phase" % case["name"])
            if case["kind"] == "ties" and entry["twin_ties"] == 0:
                raise SystemExit("%s: no entering column had its twin non-basic" % case["name"])
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


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "record":
        record(sys.argv[2])
    elif len(sys.argv) == 5 and sys.argv[1] == "merge":
        merge(*sys.argv[2:])
    else:
        sys.exit(__doc__)
