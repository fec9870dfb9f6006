"""The ends of a pivot against the library of the commit before the writer workgroup and the barrier-saving reductions of the
k2f_* front half: what only the writer of pivot_fused_kernel handles (an unbounded and an infeasible LP, budgets
that run out at, before and after the edge of a batch, with graph replay and without) and exact ties between identical columns in
one pricing wave, in two waves and in two pricing workgroups, under both tie rules -- replayed field for field against fingerprints
recorded with that library (tools/record_pivot_tail_cases.py: the cases, the fields, how the golden file was made)."""
import importlib.util
import json
import os

import pytest

import relp_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_pivot_tail_cases", os.path.join(ROOT, "tools", "record_pivot_tail_cases.py"))
recorder = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(recorder)
with open(os.path.join(ROOT, "tests", "golden", "pivot_tail_fingerprints.json")) as handle:
    GOLDEN = json.load(handle)
FIELDS = {"ending": ("result", "pivots_phase_one", "pivots_phase_two", "basis", "x_B", "objective", "kernel_launches", "device_bytes"),
          "budget": ("calls", "kernel_launches"),
          "ties": ("bases", "last_reason", "objective", "seed", "twin_ties")}


def test_the_golden_file_has_every_case():
    assert sorted(GOLDEN) == sorted(recorder.CASE_BY_NAME)
    for name, entry in GOLDEN.items():
        case = recorder.CASE_BY_NAME[name]
        assert sorted(set(entry) - {"unstable"} | set(entry.get("unstable", []))) == sorted(FIELDS[case["kind"]]), name


def test_the_endings_are_the_writers():
    for name, entry in GOLDEN.items():
        case = recorder.CASE_BY_NAME[name]
        if case["kind"] == "ending":
            assert entry["result"] == recorder.ENDING_KIND[case["model"]], name
            plan = recorder.model(case["model"]).kernel_path(**case["options"])
            assert plan["m"] == recorder.END_M == 9 and plan["n"] - plan["sparse_first"] == recorder.END_N == 40
        if case["kind"] == "budget":
            calls = entry["calls"]
            assert [call["asked"] for call in calls] == [1, 63, 64, 65, 129], name
            for call in calls[:4]:  # a used-up budget reports what was asked for ...
                assert call["reason"] == relp_amd.STOP_BUDGET and call["done"] == call["asked"], name
            # ... and the last call ends the phase inside its second batch of 64: the launches behind that pivot are no-ops
            assert calls[4]["reason"] == relp_amd.STOP_NO_ENTERING and 64 < calls[4]["done"] < 128, name


@pytest.mark.parametrize("distance", recorder.DISTANCES)
def test_the_tie_cases_hold_twins_and_met_a_tie_between_them(distance):
    lp = recorder.model("twins%d" % distance)
    twins = 0
    for j in range(recorder.TIE_N):
        twin = recorder.twin_of(j, distance)
        if twin is None:
            continue
        twins += 1
        assert recorder.twin_of(twin, distance) == j and abs(twin - j) == distance
        (rows_j, values_j), (rows_t, values_t) = lp.column(j), lp.column(twin)
        assert list(rows_j) == list(rows_t) and list(values_j) == list(values_t) and lp.cost_value(j) == lp.cost_value(twin)
    assert twins >= 64
    for options in ({}, {"pivot_kernels": 1}):
        plan = lp.kernel_path(**options)
        assert plan["m"] == recorder.TIE_M == 8 and plan["n"] - plan["sparse_first"] == recorder.TIE_N == 96
        assert plan["ell_w"] == 8 and plan["price_blocks"] >= 2  # 32 columns per pricing workgroup: 32 apart is another workgroup
    for name, entry in GOLDEN.items():
        if recorder.CASE_BY_NAME[name]["model"] == "twins%d" % distance:
            # at least one pivot's entering column had its twin non-basic: the arg-max met an exact tie
            assert entry["twin_ties"] > 0 and entry["seed"] == recorder.SEEDS[distance], name
            assert len(entry["bases"]) > 1, name


@pytest.mark.gpu
@pytest.mark.parametrize("name", [case["name"] for case in recorder.CASES])
def test_pivot_tail_fingerprint(name):
    expected = dict(GOLDEN[name])
    unstable = expected.pop("unstable", [])  # fields that differed between two runs of the same library: named, not compared
    entry = recorder.run_case(recorder.CASE_BY_NAME[name])
    for field in unstable:
        entry.pop(field)
    print(name, entry)
    assert entry == expected
