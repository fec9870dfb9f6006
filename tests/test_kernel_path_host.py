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
PLANNED = [case for case in recorder.CASES + recorder.CHOICE_CASES if case["run"] != "refused"]


REGISTERS = {"REGISTERS_2": 2, "REGISTERS_4": 4, "REGISTERS_8": 8, "REGISTERS_16": 16}
RATIO_KERNELS = set(REGISTERS) | {"MULTI_WORKGROUP", "ONE_WORKGROUP"}
PRICE_KERNELS = {"UNIT_PAIRS", "GENERATED", "WIDTH_2", "LDS", "GATHER"}
ENUMS = {"price_kernel": PRICE_KERNELS, "price_kernel_fused": PRICE_KERNELS, "ratio_kernel": RATIO_KERNELS,
         "ratio_kernel_no_change": RATIO_KERNELS - {"MULTI_WORKGROUP"}, "update_kernel": {"EAGER", "PREDICATED", "PREDICATED_SPLIT_GRID"},
         "polish_gemm": {"MFMA", "VECTOR"}}
PRICE_LDS_CONFIGURED = 160 * 1024 - 1024  # what configure_lds lets a pricing workgroup ask for


def check_kernel_choice(name, p):
    """What must hold between the instantiations the plan names and the sizes it was given (kernel_limits.hpp: 512 threads hold the rows)."""
    for field, values in ENUMS.items():
        assert p[field] in values, (name, field)
    if p["ftran_slices"] > 0:  # alpha comes preselected: only the register-resident kernel reads it
        assert p["ratio_kernel"] in REGISTERS, name
    for field in ("ratio_kernel", "ratio_kernel_no_change"):
        if p[field] in REGISTERS:
            assert REGISTERS[p[field]] * 512 >= p["m"], (name, field)
            assert REGISTERS[p[field]] == 2 or REGISTERS[p[field]] * 256 < p["m"], (name, field)  # ... and the smallest that does
    assert p["ratio_kernel_no_change"] != "MULTI_WORKGROUP", name
    assert p["multi_workgroup_ratio"] == (p["ratio_kernel"] == "MULTI_WORKGROUP"), name
    assert (p["fused_rows"] > 0) == p["fused"], name
    if p["fused"]:
        assert p["fused_rows"] in (2, 4) and p["fused_rows"] * 512 >= p["m"], name
    for field in ("price_kernel", "price_kernel_fused"):
        if p[field] == "LDS":
            assert p["price_lds"] <= PRICE_LDS_CONFIGURED and p["ell_w"] == 8, (name, field)
    if p["price_kernel"] == "LDS":
        assert p["dense_blocks"] == 0, name
    assert (p["price_kernel"] in ("UNIT_PAIRS", "GENERATED")) == p["generated_columns"], name
    assert (p["update_kernel"] == "EAGER") == (p["m"] <= 2048), name
    assert p["launches_per_batch"] == (2 if p["fused"] else 1), name
    assert p["launches_per_pivot_forced"] == (p["launches_per_pivot"] if not p["fused"] else 3), name


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
    for field, values in ENUMS.items():  # every instantiation the plan can name is named by a case
        assert {plan[field] for plan in plans.values()} == values, field
    assert {plan["fused_rows"] for plan in plans.values()} == {0, 2, 4}


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
        check_kernel_choice(name, p)


@pytest.mark.parametrize("case", recorder.REFUSED, ids=[case["name"] for case in recorder.REFUSED])
def test_refused_loads_are_refused_by_the_plan(case):
    with pytest.raises(relp_amd.RelpError) as info:
        recorder.model(case["model"]).kernel_path(**case["options"])
    recorded = FINGERPRINTS[case["name"]]["refusal"]  # what a load on the device answered before the plan existed
    assert info.value.status == relp_amd.api.ERR_ARGUMENT == recorded["status"]
    assert str(info.value) == "relp_amd status %d: %s" % (recorded["status"], recorded["message"])


# The diagonal LP on each side of every row count at which the plan takes another instantiation: 512 threads hold 2 / 4 / 8 / 16 rows
# each in the register-resident ratio test (1024, 2048, 4096, 8192 rows; beyond: across workgroups), 2 / 4 in the fused pivot (1024;
# 2048 is its last size), the update reads whole columns up to 2048 rows, and pricing stages 3 m doubles in LDS up to 96 KB (4096).
# (m, options) -> ratio_kernel, ratio_kernel_no_change, fused_rows, update_kernel, price_kernel, launches per batch / pivot / forced / replayed
THREE = {"pivot_kernels": 1}
EDGES = [
    (1024, {}, "REGISTERS_2", "REGISTERS_2", 2, "EAGER", "LDS", (2, 2, 3, 3)),
    (1025, {}, "REGISTERS_4", "REGISTERS_4", 4, "EAGER", "LDS", (2, 2, 3, 3)),
    (2048, {}, "REGISTERS_4", "REGISTERS_4", 4, "EAGER", "LDS", (2, 2, 3, 3)),
    (2049, {}, "REGISTERS_8", "REGISTERS_8", 0, "PREDICATED_SPLIT_GRID", "LDS", (1, 3, 3, 3)),
    (4096, {}, "REGISTERS_8", "REGISTERS_8", 0, "PREDICATED_SPLIT_GRID", "LDS", (1, 3, 3, 3)),
    (4097, {}, "REGISTERS_16", "REGISTERS_16", 0, "PREDICATED_SPLIT_GRID", "GATHER", (1, 3, 3, 3)),
    (8192, {}, "REGISTERS_16", "REGISTERS_16", 0, "PREDICATED_SPLIT_GRID", "GENERATED", (1, 3, 3, 3)),
    (8193, {}, "MULTI_WORKGROUP", "ONE_WORKGROUP", 0, "PREDICATED_SPLIT_GRID", "GENERATED", (1, 3, 3, 3)),
    (1024, THREE, "REGISTERS_2", "REGISTERS_2", 0, "EAGER", "LDS", (1, 3, 3, 3)),
    (1025, THREE, "REGISTERS_4", "REGISTERS_4", 0, "EAGER", "LDS", (1, 3, 3, 3)),
    (2048, THREE, "REGISTERS_4", "REGISTERS_4", 0, "EAGER", "LDS", (1, 3, 3, 3)),
    (8193, {"switches": relp_amd.api.SW_K2_SINGLE}, "ONE_WORKGROUP", "ONE_WORKGROUP", 0, "PREDICATED_SPLIT_GRID", "GENERATED", (1, 3, 3, 3)),
    (8192, {"carry": recorder.NETWORK}, "REGISTERS_16", "REGISTERS_16", 0, "PREDICATED", "GENERATED", (1, 5, 5, 5)),
    (8193, {"carry": recorder.NETWORK}, "MULTI_WORKGROUP", "ONE_WORKGROUP", 0, "PREDICATED", "GENERATED", (1, 7, 7, 7)),
]


@pytest.fixture(scope="module")
def diagonal():
    models = {}

    def get(m):
        if m not in models:
            models[m] = recorder._diagonal(m)
        return models[m]
    return get


@pytest.mark.parametrize("edge", EDGES, ids=["%d-%s" % (e[0], "-".join("%s=%s" % kv for kv in e[1].items()) or "default") for e in EDGES])
def test_instantiations_on_each_side_of_every_edge(diagonal, edge):
    m, options, ratio, no_change, fused_rows, update, price, launches = edge
    p = diagonal(m).kernel_path(**options)
    assert p["m"] == m
    assert (p["ratio_kernel"], p["ratio_kernel_no_change"]) == (ratio, no_change)
    assert p["fused_rows"] == fused_rows and p["fused"] == (fused_rows > 0)
    assert p["update_kernel"] == update and p["price_kernel"] == price
    assert (p["launches_per_batch"], p["launches_per_pivot"], p["launches_per_pivot_forced"], p["launches_per_pivot_replayed"]) == launches
    check_kernel_choice("diagonal %d %r" % (m, options), p)
