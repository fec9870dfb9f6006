"""The spanning-forest carry (RELP_CARRY_NETWORK) on BASELINE config 5 (V = 65 536, E = 1 048 576, implicit bounds), from the
reference start and from the crash basis:
  * a whole solve: pivots, seconds, pivots per second, device bytes;
  * the same solve with RELP_SW_NETWORK_STATS (same pivots): row depth, subtree cut off by the leaving arc and path of the entering
    arc, averaged over EVERY pivot (the record's "network_tree");
  * per-kernel times in a third run (profile_kernel 0 pricing, 1 entering column + tree path + ratio test, 2 forest update, each
    launch bracketed by events outside the captured batches, so with launch gaps).  profile_kernel advances that run by the pivots
    it times, so its pivot path is not the solve's; the times are per launch at the sampled states.

    python tools/network_carry_probe.py [--samples 16] [--out profiles/network_carry_probe_mi355x.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import relp_amd  # noqa: E402
from relp_amd.api import CARRY_NETWORK, SW_NETWORK_STATS  # noqa: E402
from relp_amd.workloads import max_flow_graph  # noqa: E402

NR_VERTICES, NR_ARCS = 65536, 1048576


def probe(model, crash, samples):
    out = {"start": "crash" if crash else "reference"}
    solver = relp_amd.Solver(carry=CARRY_NETWORK, implicit_bounds=1, crash=crash).load_model(model)
    result = solver.solve_relaxation()
    record = solver.record()
    pivots = result.pivots_phase_one + result.pivots_phase_two
    out.update(pivots=pivots, solve_seconds=result.solve_seconds, pivots_per_second=pivots / result.solve_seconds,
               objective=result.objective, device_bytes=record["device_bytes"], carry=record["carry"], ratio_rule=record["ratio_rule"])
    solver.close()
    solver = relp_amd.Solver(carry=CARRY_NETWORK, implicit_bounds=1, crash=crash, switches=SW_NETWORK_STATS).load_model(model)
    counted = solver.solve_relaxation()
    assert counted.pivots_phase_one + counted.pivots_phase_two == pivots
    out["forest_per_pivot"] = solver.record()["network_tree"]
    solver.close()
    solver = relp_amd.Solver(carry=CARRY_NETWORK, implicit_bounds=1, crash=crash).load_model(model)
    solver.begin_phase_one()
    every = max(1, pivots // max(1, samples))
    times = {0: [], 1: [], 2: []}
    phase = 1
    while True:
        for which in (0, 1, 2):
            try:
                times[which].append(solver.profile_kernel(which, 4))
            except relp_amd.RelpError:
                pass
        done, reason = solver.iterate(every)
        if done == 0 or reason != relp_amd.STOP_BUDGET:
            if phase == 2 or solver.objective_function_value() > 0:
                break
            phase = 2
            solver.begin_phase_two()
    solver.close()
    out["kernel_us"] = {name: 1e6 * float(np.mean(times[k])) if times[k] else None
                        for k, name in ((0, "price"), (1, "path_and_ratio"), (2, "forest_update"))}
    out["kernel_samples"] = len(times[0])
    return out


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--samples", type=int, default=16)
    parser.add_argument("--out", default=None)
    args = parser.parse_args()
    tail, head, capacity = max_flow_graph(NR_VERTICES, NR_ARCS)
    model = relp_amd.Model.max_flow(NR_VERTICES, list(zip(tail.tolist(), head.tolist(), capacity.tolist())), 0, NR_VERTICES - 1)
    results = [probe(model, crash, args.samples) for crash in (0, 1)]
    text = json.dumps({"workload": "BASELINE config 5, implicit bounds", "results": results}, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
