"""Every kernel path a load can choose, replayed against fingerprints recorded before the load-time plan moved into
``plan_kernel_path`` (tools/record_kernel_paths.py: the cases, what is recorded and how the golden file was made).  Equality field
for field: the device bytes say that the same buffers exist with the same sizes, the pivots, launches, objective bits and the basis
that the same kernels ran."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_kernel_paths", os.path.join(ROOT, "tools", "record_kernel_paths.py"))
recorder = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(recorder)
with open(os.path.join(ROOT, "tests", "golden", "kernel_path_fingerprints.json")) as handle:
    GOLDEN = json.load(handle)


def test_the_golden_file_has_every_case():
    assert sorted(GOLDEN) == sorted(recorder.CASE_BY_NAME)


@pytest.mark.parametrize("name", [case["name"] for case in recorder.CASES])
def test_kernel_path_fingerprint(name):
    expected = dict(GOLDEN[name])
    unstable = expected.pop("unstable", [])  # fields that differed between two runs of the same library: named, not compared
    entry = recorder.run_case(recorder.CASE_BY_NAME[name])
    for field in unstable:
        level, key = field.split(".")
        entry[level].pop(key)
    assert sorted(entry) == sorted(expected)
    for level in expected:
        assert entry[level] == expected[level], level
