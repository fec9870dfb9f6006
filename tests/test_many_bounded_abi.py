"""``relp_many_create_with`` / ``relp_many_config.implicit_bounds`` on a machine without a GPU: the struct mirrors agree, the new
symbols are exported, and what the mode accepts and refuses is decided before the device is touched (so a model it accepts gets
as far as ``RELP_ERR_DEVICE`` here)."""
import ctypes as C
import os

import pytest

import relp_amd
from relp_amd.api import ERR_ARGUMENT, ERR_DEVICE, ManyConfig
from test_struct_layouts import c_struct, ctypes_struct, rust_struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def netlib(name):
    return relp_amd.Model(os.path.join(ROOT, "data", "netlib", name + ".SIF"))


def no_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")


def create_with(models, config, **overrides):
    """relp_many_create_with through ctypes: (status, error text).  ``config``: a ManyConfig, or None for NULL."""
    options = relp_amd.default_options(**overrides)
    handles = (C.c_void_p * len(models))(*[m._h for m in models])
    out = C.c_void_p()
    error = C.create_string_buffer(512)
    status = relp_amd.lib().relp_many_create_with(handles, len(models), C.byref(options), C.byref(config) if config is not None else None,
                                                  C.byref(out), error, 512)
    if status == 0:
        relp_amd.lib().relp_many_free(out)
    return status, error.value.decode()


def create(models, **overrides):
    options = relp_amd.default_options(**overrides)
    handles = (C.c_void_p * len(models))(*[m._h for m in models])
    out = C.c_void_p()
    error = C.create_string_buffer(512)
    status = relp_amd.lib().relp_many_create(handles, len(models), C.byref(options), C.byref(out), error, 512)
    if status == 0:
        relp_amd.lib().relp_many_free(out)
    return status, error.value.decode()


def bounded_config():
    return ManyConfig(C.sizeof(ManyConfig), 1)


def test_many_config_layouts_match_the_header_ctypes_and_integration_md():
    header = c_struct("relp_many_config")
    assert [f[0] for f in header] == ["struct_size", "implicit_bounds"]
    assert ctypes_struct(ManyConfig) == header
    assert rust_struct("RelpManyConfig") == header
    assert C.sizeof(ManyConfig) == sum(width * count for _, _, width, count in header) == 8


def test_the_three_symbols_are_exported_and_documented():
    names = {"relp_many_create_with", "relp_many_get_bound_flips", "relp_get_bound_flips"}
    assert names <= set(relp_amd.SYMBOLS)
    assert all(hasattr(relp_amd.lib(), s) for s in names)
    with open(os.path.join(ROOT, "include", "relp_amd.h")) as handle:
        header = handle.read()
    with open(os.path.join(ROOT, "INTEGRATION.md")) as handle:
        integration = handle.read()
    for name in names:
        assert "int32_t %s(" % name in header, name
        assert "fn %s(" % name in integration, name


def test_boeing1_is_taken_by_its_constraint_rows_and_refused_by_its_standard_form_rows():
    no_gpu()
    boeing1 = netlib("BOEING1")
    assert (boeing1.nr_rows, boeing1.nr_constraints) == (596, 351)
    status, message = create_with([netlib("AFIRO"), boeing1], bounded_config())
    assert status == ERR_DEVICE, message  # accepted by every check that comes before the device
    status, message = create([netlib("AFIRO"), boeing1])
    assert status == ERR_ARGUMENT and "model 1" in message and "596" in message and "512" in message, message


def test_over_512_constraint_rows_is_refused_by_index_before_the_device():
    gfrd = netlib("GFRD-PNC")
    assert gfrd.nr_constraints == 616
    status, message = create_with([netlib("AFIRO"), netlib("KB2"), gfrd], bounded_config())
    assert status == ERR_ARGUMENT, message
    assert "model 2" in message and "616" in message and "512" in message and "constraint rows" in message, message


@pytest.mark.parametrize("size", [0, 4, 12, 16, -8])
def test_a_struct_size_the_header_never_had_is_an_argument_error(size):
    status, message = create_with([netlib("AFIRO")], ManyConfig(size, 1))
    assert status == ERR_ARGUMENT and "struct_size" in message, message
    status, message = create_with([netlib("AFIRO")], ManyConfig(size, 0))
    assert status == ERR_ARGUMENT and "struct_size" in message, message


def test_an_implicit_bounds_value_other_than_0_and_1_is_refused():
    status, message = create_with([netlib("AFIRO")], ManyConfig(C.sizeof(ManyConfig), 2))
    assert status == ERR_ARGUMENT and "implicit_bounds" in message, message


def test_a_null_config_refuses_and_accepts_what_relp_many_create_does():
    no_gpu()
    cases = [
        ([netlib("AFIRO"), netlib("BLEND")], {}),
        ([netlib("AFIRO"), netlib("SC50A"), netlib("25FV47")], {}),
        ([netlib("BOEING1")], {}),
        ([netlib("AFIRO")], {"implicit_bounds": 1}),
        ([netlib("AFIRO")], {"crash": 1}),
        ([netlib("AFIRO")], {"pivot_rule": relp_amd.DANTZIG}),
    ]
    for models, overrides in cases:
        assert create_with(models, None, **overrides) == create(models, **overrides), overrides
        # a config that leaves the mode off changes nothing either
        assert create_with(models, ManyConfig(C.sizeof(ManyConfig), 0), **overrides) == create(models, **overrides), overrides


def test_the_options_field_stays_refused_in_the_bounded_mode_too():
    status, message = create_with([netlib("AFIRO")], bounded_config(), implicit_bounds=1)
    assert status == ERR_ARGUMENT and "implicit_bounds" in message, message


def test_python_many_bounded_reaches_the_device():
    no_gpu()
    with pytest.raises(relp_amd.RelpError) as info:
        relp_amd.Many([netlib("BOEING1")], bounded=True)
    assert info.value.status == ERR_DEVICE
    with pytest.raises(relp_amd.RelpError) as info:
        relp_amd.Many([netlib("BOEING1")])
    assert info.value.status == ERR_ARGUMENT


def test_bad_arguments():
    lib = relp_amd.lib()
    flips = C.c_int64()
    assert lib.relp_many_get_bound_flips(None, 0, C.byref(flips)) == ERR_ARGUMENT
    assert lib.relp_get_bound_flips(None, C.byref(flips)) == ERR_ARGUMENT
    out = C.c_void_p()
    config = bounded_config()
    assert lib.relp_many_create_with(None, 1, None, C.byref(config), C.byref(out), None, 0) == ERR_ARGUMENT
