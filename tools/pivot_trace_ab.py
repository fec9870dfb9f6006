"""Same pivots, same bits: a record of what one build of the library computes on the smallest inputs that reach every kernel that
prices a column or chooses the entering one, and the comparison of two such records.  A diagnostic for refactors that must not move a
bit (relp_amd/csrc/pivot_step.hpp, price_step.hpp), not a test.

    python tools/pivot_trace_ab.py record --lib relp_amd/librelp_amd.so --out profiles/<name>/result.json
    python tools/pivot_trace_ab.py compare profiles/<name>/parent.json profiles/<name>/result.json

`record` runs the cases in a fresh child process with RELP_AMD_LIB set to the library (the binding loads one library per process).
Solver cases step with iterate(1) / last_pivot() and keep (phase, q, p, leaving) of the first 300 pivots, then the pivot counts per phase
and float.hex of the objective; Many cases keep per LP the status, kind, iterations, bound flips, basis and the objective's bits.
`compare` prints the first difference of every case that differs and exits 1 if there is one.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACE_CAP = 300
NETLIB4 = ("AFIRO", "ADLITTLE", "SHARE2B", "BLEND")
STORAGE = {"bytes, column per lane": {}, "bytes, vectors in LDS": {"RELP_NO_DENSE_LANE": "1"},  # tests/test_gpu_dense.py::STORAGE
           "f32, column per lane": {"RELP_DENSE_F32": "1"}, "f32, vectors in LDS": {"RELP_DENSE_F32": "1", "RELP_NO_DENSE_LANE": "1"},
           "f64, column per lane": {"RELP_DENSE_F64": "1"}, "f64, vectors in LDS": {"RELP_DENSE_F64": "1", "RELP_NO_DENSE_LANE": "1"}}


def solver_record(solver):
    """The device loop one pivot at a time while the trace is short, in batches after that."""
    import relp_amd
    pivots, counts, outcome = [], [0, 0], "optimal"
    solver.begin_phase_one()
    for phase in (1, 2):
        while True:
            done, reason = solver.iterate(1 if len(pivots) < TRACE_CAP else 4096)
            counts[phase - 1] += done
            if done == 1 and len(pivots) < TRACE_CAP:
                pivots.append(list(solver.last_pivot()))
            if reason == relp_amd.STOP_UNBOUNDED:
                outcome = "unbounded"
                break
            if reason == relp_amd.STOP_NO_ENTERING:
                break
            assert counts[phase - 1] < 10 ** 7
        if outcome != "optimal":
            break
        if phase == 1:
            if solver.n_art > 0 and abs(solver.objective_function_value()) > 1e-9:  # (no artificials: phase one ran on the costs)
                outcome = "infeasible"
                break
            solver.begin_phase_two()
    return {"outcome": outcome, "pivots_phase_one": counts[0], "pivots_phase_two": counts[1], "bound_flips": solver.bound_flips(),
            "objective": float(solver.objective_function_value()).hex(), "trace": pivots}


def many_record(models, names, **options):
    import numpy as np
    import relp_amd
    many = relp_amd.Many(models, **options)
    results = many.solve()
    out = {}
    for i, name in enumerate(names):
        r = results[i]
        out[name] = {"status": r.status, "kind": r.kind, "pivots_phase_one": r.pivots_phase_one, "pivots_phase_two": r.pivots_phase_two,
                     "bound_flips": many.bound_flips(i), "basis": [int(x) for x in many.basis(i)], "objective": float(np.float64(r.objective)).hex()}
    many.close()
    return out


def cases():
    """(name, environment, run) of every case; `run` builds the handle after the environment is set."""
    import relp_amd
    from relp_amd import api
    from relp_amd.workloads import dense_lp, max_flow_graph

    def netlib(name, **options):
        return lambda: solver_record(relp_amd.Solver(**options).load_mps(os.path.join(ROOT, "data", "netlib", name + ".SIF")))

    out = []
    for name in NETLIB4:
        out.append(("netlib %s, fused pivot" % name, {}, netlib(name)))
        out.append(("netlib %s, three-kernel pivot" % name, {}, netlib(name, pivot_kernels=1)))
        out.append(("netlib %s, pricing without LDS" % name, {}, netlib(name, price_lds_max=1)))
    for name in ("AFIRO", "BLEND"):
        for rule in range(4):
            out.append(("netlib %s, pivot rule %d" % (name, rule), {}, netlib(name, pivot_rule=rule)))
        out.append(("netlib %s, LU carry" % name, {}, netlib(name, carry=api.CARRY_LU)))
        out.append(("netlib %s, LU carry through the inverse triangles" % name, {}, netlib(name, carry=api.CARRY_LU_INVERSE)))
    for name in ("KB2", "BORE3D"):
        out.append(("netlib %s, implicit bounds" % name, {}, netlib(name, implicit_bounds=1)))
    for m, n in ((64, 128), (256, 512)):
        for storage in sorted(STORAGE):
            for long_columns in (False, True):
                env = dict(STORAGE[storage], **({"RELP_FTRAN_MIN_NNZ": "16"} if long_columns else {}))
                out.append(("dense %dx%d, %s%s" % (m, n, storage, ", multi-block FTRAN" if long_columns else ""), env,
                            lambda m=m, n=n: solver_record(relp_amd.Solver().load_dense_le(*dense_lp(m, n)))))
    graphs = {}

    def max_flow(nr_vertices, nr_arcs):  # as tests/test_network.py builds it; once per size
        if (nr_vertices, nr_arcs) not in graphs:
            tail, head, capacity = max_flow_graph(nr_vertices, nr_arcs)
            keep = (head != 0) & (tail != nr_vertices - 1)
            arcs = list(zip(tail[keep].tolist(), head[keep].tolist(), capacity[keep].tolist()))
            graphs[(nr_vertices, nr_arcs)] = relp_amd.Model.max_flow(nr_vertices, arcs, 0, nr_vertices - 1)
        return graphs[(nr_vertices, nr_arcs)]

    def flow(nr_vertices, nr_arcs, **options):
        return lambda: solver_record(relp_amd.Solver(**options).load_model(max_flow(nr_vertices, nr_arcs)))

    out.append(("max flow 16384 vertices, generated columns", {}, flow(16384, 131072, implicit_bounds=1)))
    out.append(("max flow 16384 vertices, RELP_NO_RHO_BITS", {"RELP_NO_RHO_BITS": "1"}, flow(16384, 131072, implicit_bounds=1)))
    out.append(("max flow 16384 vertices, RELP_PRICE_UNIT_PAIRS", {"RELP_PRICE_UNIT_PAIRS": "1"}, flow(16384, 131072, implicit_bounds=1)))
    out.append(("max flow 16384 vertices, SW_NO_GENERATED_COLUMNS", {}, flow(16384, 131072, implicit_bounds=1, switches=api.SW_NO_GENERATED_COLUMNS)))
    out.append(("max flow 16384 vertices, CARRY_NETWORK", {}, flow(16384, 131072, implicit_bounds=1, carry=api.CARRY_NETWORK)))
    out.append(("max flow 1024 vertices, 9190 rows (multi-workgroup ratio test)", {}, flow(1024, 8192)))

    def many_netlib(**options):
        def run():
            names = []
            for entry in sorted(os.listdir(os.path.join(ROOT, "tests", "golden"))):
                if entry.endswith(".json"):
                    fixture = json.load(open(os.path.join(ROOT, "tests", "golden", entry)))
                    if isinstance(fixture, dict) and fixture.get("file", "").startswith("data/netlib/") and fixture.get("m", 1 << 30) <= 128 \
                            and os.path.exists(os.path.join(ROOT, fixture["file"])):
                        names.append((entry[:-5], fixture["file"]))
            return many_record([relp_amd.Model(os.path.join(ROOT, f)) for _, f in names], [n for n, _ in names], **options)
        return run

    for bounded in (False, True):
        for rule, rule_name in ((relp_amd.STEEPEST_EDGE, "steepest edge"), (relp_amd.DANTZIG, "Dantzig")):
            out.append(("many, %s, %s" % ("bounded" if bounded else "plain", rule_name), {}, many_netlib(bounded=bounded, pivot_rule=rule)))
    return out


def child(out_path, only):
    sys.path.insert(0, ROOT)
    import relp_amd
    record = {"library": relp_amd.lib().relp_version().decode(), "cases": {}}
    for name, env, run in cases():
        if only and only not in name:
            continue
        os.environ.update(env)
        try:
            record["cases"][name] = run()
        finally:
            for key in env:
                del os.environ[key]
        print("recorded", name, flush=True)
        write_record(record, out_path)  # (after every case: a fault leaves what was recorded)


def write_record(record, path):
    """Valid JSON with one line per case.  A trace that an earlier case (by name) of the same record also walked is written as
    {"same_as": that case}: the storage forms, launch paths and carries mostly make the same pivots, and a committed record stays short."""
    lines, first = [], {}
    for name in sorted(record["cases"]):
        case = dict(record["cases"][name])
        if "trace" in case:
            key = json.dumps(case["trace"])
            if key in first:
                case["trace"] = {"same_as": first[key]}
            first.setdefault(key, name)
        lines.append('  %s: %s' % (json.dumps(name), json.dumps(case, sort_keys=True, separators=(",", ":"))))
    with open(path, "w") as f:
        f.write('{"library": %s, "cases": {\n%s\n}}\n' % (json.dumps(record["library"]), ",\n".join(lines)))


def read_record(path):
    record = json.load(open(path))
    for case in record["cases"].values():
        if isinstance(case.get("trace"), dict):
            case["trace"] = record["cases"][case["trace"]["same_as"]]["trace"]
    return record


def first_difference(a, b, path=""):
    if type(a) is not type(b):
        return "%s: %r against %r" % (path, a, b)
    if isinstance(a, dict):
        for key in sorted(set(a) | set(b)):
            if key not in a or key not in b:
                return "%s/%s: only in %s" % (path, key, "the first" if key in a else "the second")
            d = first_difference(a[key], b[key], path + "/" + str(key))
            if d:
                return d
        return None
    if isinstance(a, list):
        for k, (x, y) in enumerate(zip(a, b)):
            d = first_difference(x, y, "%s[%d]" % (path, k))
            if d:
                return d
        return None if len(a) == len(b) else "%s: %d entries against %d" % (path, len(a), len(b))
    return None if a == b else "%s: %r against %r" % (path, a, b)


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = parser.add_subparsers(dest="mode", required=True)
    rec = sub.add_parser("record")
    rec.add_argument("--lib", required=True)
    rec.add_argument("--out", required=True)
    rec.add_argument("--only", default="", help="cases whose name contains this")
    rec.add_argument("--in-child", action="store_true", help=argparse.SUPPRESS)
    cmp_ = sub.add_parser("compare")
    cmp_.add_argument("first")
    cmp_.add_argument("second")
    args = parser.parse_args()
    if args.mode == "record":
        if args.in_child:
            return child(args.out, args.only)
        env = dict(os.environ, RELP_AMD_LIB=os.path.abspath(args.lib))
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        return subprocess.call([sys.executable, os.path.abspath(__file__), "record", "--lib", args.lib, "--out", args.out, "--only", args.only, "--in-child"], env=env)
    a, b = read_record(args.first), read_record(args.second)
    differing = 0
    for name in sorted(set(a["cases"]) | set(b["cases"])):
        if name not in a["cases"] or name not in b["cases"]:
            print("%s: only in %s" % (name, args.first if name in a["cases"] else args.second))
            differing += 1
            continue
        d = first_difference(a["cases"][name], b["cases"][name])
        if d:
            print("%s: first difference at %s" % (name, d))
            differing += 1
    print("%d cases compared, %d differ" % (len(set(a["cases"]) | set(b["cases"])), differing))
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main())
