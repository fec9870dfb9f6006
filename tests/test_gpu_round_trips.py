"""The regrouped load phases of price_kernel, the k2f_* front half and pivot_fused_kernel against the library of the commit before
them: small seeded integer LPs at every shape where the new load code takes another path, replayed field for field against
fingerprints recorded with that library (tools/record_round_trip_cases.py: the cases, the fields, how the golden file was made).
Equal pivots, objective bits, basis, solution bytes and rows of the inverse say that not one floating-point operation changed;
equal launches and device bytes that no launch and no buffer did."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_round_trip_cases", os.path.join(ROOT, "tools", "record_round_trip_cases.py"))
recorder = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(recorder)
with open(os.path.join(ROOT, "tests", "golden", "round_trip_fingerprints.json")) as handle:
    GOLDEN = json.load(handle)
FIELDS = ("result", "pivots_phase_one", "pivots_phase_two", "objective", "basis", "solution", "inverse_rows", "kernel_launches", "device_bytes")


def test_the_golden_file_has_every_case():
    assert sorted(GOLDEN) == sorted(recorder.CASE_BY_NAME)
    for name, entry in GOLDEN.items():
        assert sorted(set(entry) - {"unstable"} | set(entry.get("unstable", []))) == sorted(FIELDS), name
        assert entry["result"] == 1, name  # relp_amd.FINITE_OPTIMUM
    for name in recorder.MANY_PIVOTS:
        assert GOLDEN[name]["pivots_phase_one"] + GOLDEN[name]["pivots_phase_two"] > 64


@pytest.mark.parametrize("blocks", sorted(recorder.BLOCKS))
def test_the_block_cases_reach_their_number_of_pricing_workgroups(blocks):
    lp = recorder.model("blocks%d" % blocks)
    assert lp.kernel_path()["price_blocks"] == blocks
    assert lp.kernel_path(pivot_kernels=1)["price_blocks"] == blocks


def test_the_two_pass_case_has_more_columns_than_one_pass_prices():
    plan = recorder.model("blocks1024-two-passes").kernel_path()
    assert plan["price_blocks"] == 1024 and plan["n"] - plan["sparse_first"] > 1024 * (256 // plan["ell_w"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", [case["name"] for case in recorder.CASES])
def test_round_trip_fingerprint(name):
    expected = dict(GOLDEN[name])
    unstable = expected.pop("unstable", [])  # fields that differed between two runs of the same library: named, not compared
    entry = recorder.run_case(recorder.CASE_BY_NAME[name])
    for field in unstable:
        entry.pop(field)
    print(name, entry)
    assert entry == expected
