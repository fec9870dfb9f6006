"""What the exact certificate of a relp_many launch costs: `Many.certify(mode=1)` (the serial certificate, LP after LP, what
options.certify does) against `Many.certify(mode=0)` (one further launch for all LPs, the host stage on at most 16 threads, the
serial certificate per LP for what the batch does not take), on the same handle in the same process, for the lists of
tools/many_probe.py:
  (a) 1024 LPs cycling through the golden Netlib LPs of at most 128 standard-form rows,
  (b) 256 LPs cycling through the golden Netlib LPs of 129 to 512 rows (--skip-b leaves it out),
  (c) 4096 seeded random LPs of 16 to 128 rows,
and once for every golden LP of at most 512 rows (the per-reason counts of tests/test_gpu_many_certify.py).
Per list: the launch time of the solve (second of two solves), then per mode one warm-up call and `--runs` timed calls (at least
three) with their minimum, median and maximum, the LPs per path and per fallback reason, and the largest digit count K.
`--kinds` adds `Many.certify(mode=2)` (INFEASIBLE and UNBOUNDED results in the same launch: a third solve per ray) as a third mode
in the same process, with the LPs per verdict, the rays lifted and the host seconds per path (launch, host stage and fallbacks
apart), and a fifth list, since the four above hold no UNBOUNDED result:
  (d) 4096 seeded random LPs as in (c), each with one more column of cost -1 and negative entries in <= rows only, so that every
      feasible one is unbounded along it.

    python tools/many_certify_probe.py [--out profiles/many_certify_mi355x.json]
    python tools/many_certify_probe.py --kinds [--out profiles/many_certify_kinds_mi355x.json]
"""
import argparse
import json
import os
import statistics
import sys
from collections import Counter

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import relp_amd  # noqa: E402
from many_probe import netlib_golden, random_model  # noqa: E402
from relp_amd.api import MANY_FALLBACK_NAMES  # noqa: E402


def random_unbounded_model(rng):
    """random_model's LP (tools/many_probe.py) with one more column: cost -1, entries -1 .. -9 in up to five <= rows."""
    m = int(rng.integers(16, 129))
    n = int(rng.integers(m, 2 * m + 1))
    greater = int(m * 0.2)
    kinds = ["Less"] * (m - greater) + ["Greater"] * greater
    columns = []
    for _ in range(n):
        rows = set(rng.choice(m, size=int(rng.integers(0, min(m, 5) + 1)), replace=False).tolist()) | {int(rng.integers(0, m - greater))}
        columns.append([(int(i), int(rng.integers(1, 10))) for i in sorted(rows)])
    rows = sorted(set(rng.choice(m - greater, size=int(rng.integers(1, 6)), replace=False).tolist()))
    columns.append([(int(i), -int(rng.integers(1, 10))) for i in rows])
    b = [int(rng.integers(20, 100)) for _ in range(m - greater)] + [int(rng.integers(1, 10)) for _ in range(greater)]
    variables = [(int(rng.integers(-9, 2)), 0, None) for _ in range(n)] + [(-1, 0, None)]
    return relp_amd.Model.from_general_form(columns, kinds, b, variables)


def spread(values):
    return {"runs": values, "min": min(values), "median": statistics.median(values), "max": max(values)}


def probe(label, models, runs, kinds=False):
    many = relp_amd.Many(models, certify=0)
    many.solve()  # warm-up
    results = many.solve()
    report = {"lps": len(models), "kernel_seconds": many.kernel_seconds,
              "optimal": sum(1 for r in results if r.status == 0 and r.kind == relp_amd.FINITE_OPTIMUM)}
    modes = [(1, "serial_mode_1"), (0, "batched_mode_0")]
    if kinds:
        modes.append((2, "batched_all_kinds_mode_2"))
        report["infeasible"] = sum(1 for r in results if r.status == 0 and r.kind == relp_amd.INFEASIBLE)
        report["unbounded"] = sum(1 for r in results if r.status == 0 and r.kind == relp_amd.UNBOUNDED)
    for mode, key in modes:
        many.certify(mode=mode)  # warm-up
        wall, device, host = [], [], []
        for _ in range(runs):
            certificates = many.certify(mode=mode)
            wall.append(many.certify_wall_seconds)
            device.append(many.certify_device_seconds)
            host.append(sum(c.host_seconds for c in certificates))
        entry = {"wall_seconds": spread(wall), "host_seconds_summed_over_lps": spread(host),
                 "certified": sum(c.certified for c in certificates),
                 "paths": {str(k): v for k, v in sorted(Counter(c.path for c in certificates).items())},
                 "repair_pivots": int(sum(c.repair_pivots for c in certificates))}
        if kinds:  # (of the last timed call)
            entry["host_seconds_by_path"] = {str(path): sum(c.host_seconds for c in certificates if c.path == path) for path in (1, 2)}
        if mode == 2:
            digits = [many.certificate_digits(i) for i in range(len(models))]
            entry["rays_lifted"] = sum(1 for d in digits if d[2] > 0)
            entry["largest_K_ray"] = max(d[2] for d in digits)
            entry["ray_digits_summed"] = int(sum(d[2] for d in digits))
        if mode != 1:
            entry["device_seconds"] = spread(device)
            entry["fallback_reasons"] = dict(Counter(MANY_FALLBACK_NAMES[c.fallback_reason] for c in certificates if c.path == 2))
            entry["largest_K"] = max(max(c.digits_primal, c.digits_dual) for c in certificates)
            entry["digits_summed"] = int(sum(c.digits_primal + c.digits_dual for c in certificates))
        report[key] = entry
        print(label, key, json.dumps(entry["wall_seconds"]), flush=True)
    report["wall_ratio_serial_over_batched"] = report["serial_mode_1"]["wall_seconds"]["median"] / report["batched_mode_0"]["wall_seconds"]["median"]
    if kinds:
        report["wall_ratio_mode_0_over_mode_2"] = report["batched_mode_0"]["wall_seconds"]["median"] / report["batched_all_kinds_mode_2"]["wall_seconds"]["median"]
    many.close()
    return report


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--out", default=None)
    parser.add_argument("--kinds", action="store_true", help="time certify(mode=2) as a third mode")
    parser.add_argument("--runs", type=int, default=3)
    parser.add_argument("--skip-b", action="store_true")
    args = parser.parse_args()
    runs = max(3, args.runs)
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "many_certify_kinds_mi355x.json" if args.kinds else "many_certify_mi355x.json")
    report = {"device": "MI355X (gfx950)", "timed_runs_per_mode": runs, "cases": {}}
    lists = [("a_netlib_up_to_128_rows", netlib_golden(1, 128), 1024)]
    if not args.skip_b:
        lists.append(("b_netlib_129_to_512_rows", netlib_golden(129, 512), 256))
    for label, names, count in lists:
        models = [relp_amd.Model(os.path.join(ROOT, "data", "netlib", name + ".SIF")) for name in names]
        report["cases"][label] = dict(probe(label, [models[k % len(models)] for k in range(count)], runs, args.kinds), models=names)
    rng = np.random.default_rng(0x5EED0C)
    report["cases"]["c_random_16_to_128_rows"] = dict(probe("c_random_16_to_128_rows", [random_model(rng) for _ in range(4096)], runs, args.kinds), seed=0x5EED0C)
    if args.kinds:
        rng = np.random.default_rng(0x5EED0D)
        report["cases"]["d_random_with_an_unbounded_column"] = dict(
            probe("d_random_with_an_unbounded_column", [random_unbounded_model(rng) for _ in range(4096)], runs, True), seed=0x5EED0D)
    names = netlib_golden(1, 512)
    models = [relp_amd.Model(os.path.join(ROOT, "data", "netlib", name + ".SIF")) for name in names]
    report["cases"]["golden_up_to_512_rows_once_each"] = dict(probe("golden_up_to_512_rows_once_each", models, runs, args.kinds), models=names)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print(json.dumps(report, indent=1))


if __name__ == "__main__":
    main()
