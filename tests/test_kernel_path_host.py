"""The load-time plan (``plan_kernel_path``, relp_amd/csrc/kernel_path.hpp) without a device: ``Model.kernel_path`` over the cases of
tools/record_kernel_paths.py."""
import importlib.util
import json
import os

import pytest

import relp_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_kernel_paths", os.path.join(ROOT, "tools", "record_kernel_paths.py"))
recorder = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(recorder)
with open(os.path.join(ROOT, "tests", "golden", "kernel_path_table.json")) as handle:
    TABLE = json.load(handle)
with open(os.path.join(ROOT, "tests", "golden", "kernel_path_fingerprints.json")) as handle:
    FINGERPRINTS = json.load(handle)
PLANNED = [case for case in recorder.CASES if case["run"] != "refused"]


@pytest.fixture(scope="module")
def plans():
    return {case["name"]: recorder.model(case["model"]).kernel_path(**case["options"]) for case in PLANNED}


def test_plans_match_the_golden_table(plans):
    assert sorted(TABLE) == sorted(plans)
    for name, plan in plans.items():
        assert plan == TABLE[name], name


def test_cases_cover_every_flag_and_storage_form(plans):
    flags = [key for key, value in next(iter(plans.values())).items() if isinstance(value, bool)]
    assert len(flags) == 16  # every bool of KernelPath
    for flag in flags:
        assert {plan[flag] for plan in plans.values()} == {False, True}, flag
    assert any(plan["ftran_slices"] > 0 and plan["n_dense"] == 0 for plan in plans.values())  # multi-block FTRAN without a dense block
    assert {plan["dense_storage"] for plan in plans.values()} == {"NONE", "I8_LANE", "F32_LANE", "F64_LANE", "I8_PERMUTED", "F32_ROWS", "F64_ROWS"}


def test_invariants_between_the_decisions(plans):
    for name, p in plans.items():
        if p["fused"]:
            assert not (p["lu_mode"] or p["network"] or p["bounded"] or p["eta_mode"] or p["track_touched"]), name
            assert p["n_dense"] == 0 and p["ftran_slices"] == 0 and p["ell_w"] == 8, name
        if p["eta_mode"]:
            assert p["n_dense"] > 0 and p["m"] % 2 == 0 and p["m"] <= 4096 and p["ftran_slices"] > 0, name
        if p["slack_in_btran"]:
            assert p["eta_mode"] and p["slack_of_row_length"] == p["m"], name
        if p["generated_columns"]:
            assert p["ell_w"] == 2, name


@pytest.mark.parametrize("case", recorder.REFUSED, ids=[case["name"] for case in recorder.REFUSED])
def test_refused_loads_are_refused_by_the_plan(case):
    with pytest.raises(relp_amd.RelpError) as info:
        recorder.model(case["model"]).kernel_path(**case["options"])
    recorded = FINGERPRINTS[case["name"]]["refusal"]  # what a load on the device answered before the plan existed
    assert info.value.status == relp_amd.api.ERR_ARGUMENT == recorded["status"]
    assert str(info.value) == "relp_amd status %d: %s" % (recorded["status"], recorded["message"])
