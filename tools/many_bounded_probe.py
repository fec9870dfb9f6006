"""relp_many with implicit upper bounds (``Many(models, bounded=True)``) against the same launch with the bounds as rows
(``bounded=False``), certificate off, every figure from the second of two solves of a handle:
  (d) 1024 LPs cycling through the shipped Netlib LPs that have bounds and at most 512 standard-form rows,
  (e) 4096 seeded random boxed LPs: 16 to 64 constraint rows r, n between r and 2 r variables, a box on every variable.
LPs/s, iterations/s, iterations and bound flips of both modes go to ``--out``.

``--plain-lists LABEL`` times instead the relp_many side of the lists (a)-(c) of tools/many_probe.py and stores it under
``plain_lists[LABEL]`` of ``--out``: run it on two builds (``RELP_AMD_LIB``) to see whether the plain instantiations moved, and twice
on one build for the run-to-run noise.

    python tools/many_bounded_probe.py [--out profiles/many_bounded_mi355x.json] [--plain-lists LABEL]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import relp_amd  # noqa: E402
from many_probe import netlib_golden, random_model  # noqa: E402

NETLIB_WITH_BOUNDS = ["BOEING2", "BORE3D", "CAPRI", "GROW7", "KB2", "RECIPELP", "STAIR", "STANDATA", "VTP-BASE"]
KINDS = {1: "optimal", 2: "infeasible", 3: "unbounded", 4: "iteration_limit"}


def boxed_model(rng):
    r = int(rng.integers(16, 65))
    n = int(rng.integers(r, 2 * r + 1))
    greater = int(r * 0.2)
    kinds = ["Less"] * (r - greater) + ["Greater"] * greater
    columns = []
    for _ in range(n):
        rows = set(rng.choice(r, size=int(rng.integers(1, min(r, 5) + 1)), replace=False).tolist())
        columns.append([(int(i), int(rng.integers(1, 10))) for i in sorted(rows)])
    b = [int(rng.integers(20, 100)) for _ in range(r - greater)] + [int(rng.integers(1, 10)) for _ in range(greater)]
    variables = [(int(rng.integers(-9, 2)), 0, int(rng.integers(1, 11))) for _ in range(n)]
    return relp_amd.Model.from_general_form(columns, kinds, b, variables)


def run(models, bounded):
    many = relp_amd.Many(models, bounded=bounded, certify=0) if bounded else relp_amd.Many(models, certify=0)
    many.solve()  # warm-up
    results = many.solve()
    kernel = many.kernel_seconds
    flips = sum(many.bound_flips(i) for i in range(len(models))) if bounded else 0
    many.close()
    iterations = sum(r.pivots_phase_one + r.pivots_phase_two for r in results)
    kinds = {}
    for r in results:
        key = "status_%d" % r.status if r.status else KINDS.get(r.kind, "none")
        kinds[key] = kinds.get(key, 0) + 1
    return {"lps": len(models), "kernel_seconds": kernel, "lps_per_second": len(models) / kernel, "iterations": iterations,
            "iterations_per_second": iterations / kernel, "bound_flips": flips, "lds_tier": sum(r.inverse_in_lds for r in results),
            "global_tier": sum(1 - r.inverse_in_lds for r in results), "results": kinds,
            "mean_reinversions": float(np.mean([r.reinversions for r in results]))}


def both_modes(models):
    rows = [(m.nr_rows, m.nr_constraints) for m in models]
    out = {"mean_standard_form_rows": float(np.mean([a for a, _ in rows])), "mean_constraint_rows": float(np.mean([b for _, b in rows])),
           "bounds_as_rows": run(models, False), "implicit_bounds": run(models, True)}
    out["lps_per_second_ratio"] = out["implicit_bounds"]["lps_per_second"] / out["bounds_as_rows"]["lps_per_second"]
    return out


def plain_lists():
    out = {}
    for label, names, count in (("a_netlib_up_to_128_rows", netlib_golden(1, 128), 1024), ("b_netlib_129_to_512_rows", netlib_golden(129, 512), 256)):
        models = [relp_amd.Model(os.path.join(ROOT, "data", "netlib", name + ".SIF")) for name in names]
        out[label] = run([models[k % len(models)] for k in range(count)], False)
    rng = np.random.default_rng(0x5EED0C)
    out["c_random_16_to_128_rows"] = run([random_model(rng) for _ in range(4096)], False)
    return out


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "many_bounded_mi355x.json"))
    parser.add_argument("--plain-lists", default=None, metavar="LABEL")
    args = parser.parse_args()
    report = {"device": "MI355X (gfx950)", "certify": 0, "cases": {}, "plain_lists": {}}
    if os.path.exists(args.out):
        with open(args.out) as f:
            report = json.load(f)
    if args.plain_lists:
        report.setdefault("plain_lists", {})[args.plain_lists] = plain_lists()
        for label, case in report["plain_lists"][args.plain_lists].items():
            print(args.plain_lists, label, "%.1f LPs/s" % case["lps_per_second"], flush=True)
    else:
        models = [relp_amd.Model(os.path.join(ROOT, "data", "netlib", name + ".SIF")) for name in NETLIB_WITH_BOUNDS]
        report["cases"]["d_netlib_with_bounds"] = dict(models=NETLIB_WITH_BOUNDS, **both_modes([models[k % len(models)] for k in range(1024)]))
        print("d_netlib_with_bounds", report["cases"]["d_netlib_with_bounds"]["lps_per_second_ratio"], flush=True)
        rng = np.random.default_rng(0xB0C5ED)
        report["cases"]["e_random_boxed_16_to_64_rows"] = dict(seed=0xB0C5ED, **both_modes([boxed_model(rng) for _ in range(4096)]))
        print("e_random_boxed_16_to_64_rows", report["cases"]["e_random_boxed_16_to_64_rows"]["lps_per_second_ratio"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print(json.dumps(report, indent=1))


if __name__ == "__main__":
    main()
