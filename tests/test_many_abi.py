"""``relp_many_*`` on a machine without a GPU: the struct mirrors agree, and every refusal happens before the device is touched."""
import ctypes as C
import os

import pytest

import relp_amd
from relp_amd.api import ERR_ARGUMENT, ERR_DEVICE, ManyResult
from test_struct_layouts import c_struct, ctypes_struct, rust_struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def netlib(name):
    return relp_amd.Model(os.path.join(ROOT, "data", "netlib", name + ".SIF"))


def no_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")


def create(models, **overrides):
    """relp_many_create through ctypes: (status, error text)."""
    options = relp_amd.default_options(**overrides)
    handles = (C.c_void_p * len(models))(*[m._h for m in models])
    out = C.c_void_p()
    error = C.create_string_buffer(512)
    status = relp_amd.lib().relp_many_create(handles, len(models), C.byref(options), C.byref(out), error, 512)
    if status == 0:
        relp_amd.lib().relp_many_free(out)
    return status, error.value.decode()


def test_many_result_layouts_match_the_header_ctypes_and_integration_md():
    header = c_struct("relp_many_result")
    assert [f[0] for f in header][:4] == ["status", "kind", "certified", "inverse_in_lds"]
    assert ctypes_struct(ManyResult) == header
    assert rust_struct("RelpManyResult") == header
    assert C.sizeof(ManyResult) == sum(width * count for _, _, width, count in header)


def test_many_symbols_are_exported():
    names = [s for s in relp_amd.SYMBOLS if s.startswith("relp_many_")]
    assert {"relp_many_create", "relp_many_solve", "relp_many_get_basis", "relp_many_get_solution",
            "relp_many_get_objective_exact", "relp_many_free"} <= set(names)
    assert all(hasattr(relp_amd.lib(), s) for s in names)


def test_without_a_device_create_reports_a_device_error():
    no_gpu()
    status, message = create([netlib("AFIRO"), netlib("BLEND")])
    assert status == ERR_DEVICE, message
    with pytest.raises(relp_amd.RelpError) as info:
        relp_amd.Many([netlib("AFIRO")])
    assert info.value.status == ERR_DEVICE


def test_a_model_over_512_rows_is_refused_by_index_before_the_device():
    models = [netlib("AFIRO"), netlib("SC50A"), netlib("25FV47")]  # 25FV47: 821 rows in standard form
    status, message = create(models)
    assert status == ERR_ARGUMENT
    assert "model 2" in message and "821" in message and "512" in message


@pytest.mark.parametrize("overrides,needle", [
    ({"carry": relp_amd.api.CARRY_LU}, "carry"),
    ({"carry": relp_amd.api.CARRY_NETWORK}, "carry"),
    ({"implicit_bounds": 1}, "implicit_bounds"),
    ({"crash": 1}, "crash"),
    ({"pivot_rule": relp_amd.FIRST_PROFITABLE}, "DANTZIG"),
    ({"switches": relp_amd.api.SW_PRICE_UNIT_PAIRS}, "generated"),
])
def test_options_the_path_cannot_honour_are_refused_before_the_device(overrides, needle):
    status, message = create([netlib("AFIRO")], **overrides)
    assert status == ERR_ARGUMENT and needle in message, message


def test_dantzig_and_the_ratio_rules_are_accepted_up_to_the_device():
    no_gpu()
    for overrides in ({"pivot_rule": relp_amd.DANTZIG}, {"ratio_rule": relp_amd.api.RATIO_TEXTBOOK},
                      {"switches": relp_amd.api.SW_MANY_GLOBAL_TIER}):
        status, message = create([netlib("AFIRO")], **overrides)
        assert status == ERR_DEVICE, (overrides, message)


def test_bad_arguments():
    lib = relp_amd.lib()
    out = C.c_void_p()
    assert lib.relp_many_create(None, 1, None, C.byref(out), None, 0) == ERR_ARGUMENT
    models = (C.c_void_p * 1)(None)
    error = C.create_string_buffer(256)
    assert lib.relp_many_create(models, 1, None, C.byref(out), error, 256) == ERR_ARGUMENT
    assert b"model 0" in error.value
    assert lib.relp_many_solve(None, None, None) == ERR_ARGUMENT
    assert lib.relp_many_free(None) == ERR_ARGUMENT
