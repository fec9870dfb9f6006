"""relp_many (one workgroup per LP, one launch) against relp_batch_run (host threads, one handle per LP, bench.py's four LPs in
flight per GPU) on the same lists, certificate off in both.  LPs/s and pivots/s of each, for
  (a) 1024 LPs cycling through the golden Netlib LPs of at most 128 standard-form rows,
  (b) 256 LPs cycling through the golden Netlib LPs of 129 to 512 rows,
  (c) 4096 seeded random LPs of 16 to 128 rows.  relp_batch keeps one handle per model and worker, so it is timed on the first
      128 of them (each a model of its own, 512 handles); its LPs/s are per LP all the same.
Every figure is from the second of two runs (the first loads the code objects and builds the handles' graphs).  The kernel's
resource usage (hipcc -Rpass-analysis=kernel-resource-usage, profiles/many_kernel_resource_usage.txt) is copied into the output.

    python tools/many_probe.py [--out profiles/many_small_lps_mi355x.json]
"""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import relp_amd  # noqa: E402

WORKERS = 4  # bench.py --concurrency default


def netlib_golden(low, high):
    names = []
    for entry in sorted(os.listdir(os.path.join(ROOT, "tests", "golden"))):
        if not entry.endswith(".json"):
            continue
        fixture = json.load(open(os.path.join(ROOT, "tests", "golden", entry)))
        if isinstance(fixture, dict) and fixture.get("file", "").startswith("data/netlib/") and low <= fixture["m"] <= high:
            names.append(entry[:-5])
    return names


def random_model(rng):
    m = int(rng.integers(16, 129))
    n = int(rng.integers(m, 2 * m + 1))
    greater = int(m * 0.2)
    kinds = ["Less"] * (m - greater) + ["Greater"] * greater
    columns = []
    for _ in range(n):  # every column has a positive entry in a <= row: x >= 0 stays bounded without bound rows
        rows = set(rng.choice(m, size=int(rng.integers(0, min(m, 5) + 1)), replace=False).tolist()) | {int(rng.integers(0, m - greater))}
        columns.append([(int(i), int(rng.integers(1, 10))) for i in sorted(rows)])
    b = [int(rng.integers(20, 100)) for _ in range(m - greater)] + [int(rng.integers(1, 10)) for _ in range(greater)]
    variables = [(int(rng.integers(-9, 2)), 0, None) for _ in range(n)]
    return relp_amd.Model.from_general_form(columns, kinds, b, variables)


def run_many(models):
    many = relp_amd.Many(models, certify=0)
    many.solve()  # warm-up
    t0 = time.perf_counter()
    results = many.solve()
    wall = time.perf_counter() - t0
    kernel = many.kernel_seconds
    many.close()
    pivots = sum(r.pivots_phase_one + r.pivots_phase_two for r in results)
    kinds = {}
    for r in results:
        key = "status_%d" % r.status if r.status else {1: "optimal", 2: "infeasible", 3: "unbounded", 4: "iteration_limit"}.get(r.kind, "none")
        kinds[key] = kinds.get(key, 0) + 1
    return {"lps": len(models), "kernel_seconds": kernel, "solve_wall_seconds": wall, "lps_per_second": len(models) / kernel,
            "pivots": pivots, "pivots_per_second": pivots / kernel, "max_pivots_of_one_lp": max(r.pivots_phase_one + r.pivots_phase_two for r in results),
            "lds_tier": sum(r.inverse_in_lds for r in results), "global_tier": sum(1 - r.inverse_in_lds for r in results),
            "results": kinds, "mean_reinversions": float(np.mean([r.reinversions for r in results]))}


def run_batch(models, schedule):
    batch = relp_amd.Batch(models, devices=(0,), workers_per_device=WORKERS, certify=0)
    batch.run(schedule)  # warm-up
    entries, _, makespan = batch.run(schedule)
    batch.close()
    pivots = sum(e.result.pivots_phase_one + e.result.pivots_phase_two for e in entries)
    return {"lps": len(schedule), "workers": WORKERS, "makespan_seconds": makespan, "lps_per_second": len(schedule) / makespan,
            "pivots": pivots, "pivots_per_second": pivots / makespan, "failed": sum(1 for e in entries if e.status != 0)}


def resource_usage():
    path = os.path.join(ROOT, "profiles", "many_kernel_resource_usage.txt")
    if not os.path.exists(path):
        return None
    out, current = {}, None
    for line in open(path):
        name = re.search(r"Function Name: (\S+)", line)
        if name:
            flags = re.search(r"ILb(\d)ELb(\d)E", name.group(1))  # many_kernel<LDS_INVERSE, BOUNDED>
            current = ("lds_tier" if flags.group(1) == "1" else "global_tier") + ("_bounded" if flags.group(2) == "1" else "")
            out[current] = {"symbol": name.group(1)}
            continue
        field = re.search(r"remark:\s+([A-Za-z][^:\[]*?)\s*(?:\[[^\]]*\])?:\s*(\d+)", line)
        if current and field:
            out[current][field.group(1).strip()] = int(field.group(2))
    return out


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "many_small_lps_mi355x.json"))
    args = parser.parse_args()
    report = {"device": "MI355X (gfx950)", "certify": 0, "kernel_resource_usage": resource_usage(), "cases": {}}
    small, medium = netlib_golden(1, 128), netlib_golden(129, 512)
    for label, names, count in (("a_netlib_up_to_128_rows", small, 1024), ("b_netlib_129_to_512_rows", medium, 256)):
        models = [relp_amd.Model(os.path.join(ROOT, "data", "netlib", name + ".SIF")) for name in names]
        schedule = [k % len(models) for k in range(count)]
        many = run_many([models[k] for k in schedule])
        batch = run_batch(models, schedule)
        report["cases"][label] = {"models": names, "relp_many": many, "relp_batch_run": batch,
                                  "lps_per_second_ratio": many["lps_per_second"] / batch["lps_per_second"]}
        print(label, json.dumps(report["cases"][label]["lps_per_second_ratio"]), flush=True)
    rng = np.random.default_rng(0x5EED0C)
    models = [random_model(rng) for _ in range(4096)]
    many = run_many(models)
    batch = run_batch(models[:128], list(range(128)))
    report["cases"]["c_random_16_to_128_rows"] = {"seed": 0x5EED0C, "relp_many": many, "relp_batch_run_first_128": batch,
                                                   "lps_per_second_ratio": many["lps_per_second"] / batch["lps_per_second"]}
    print("c_random_16_to_128_rows", report["cases"]["c_random_16_to_128_rows"]["lps_per_second_ratio"], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print(json.dumps(report, indent=1))


if __name__ == "__main__":
    main()
