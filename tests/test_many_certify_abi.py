"""``relp_many_certify`` on a machine without a GPU: the struct mirrors agree, the symbols exist, bad arguments are refused before the device."""
import ctypes as C

import relp_amd
from relp_amd.api import ERR_ARGUMENT, ManyCertificate
from test_struct_layouts import c_struct, ctypes_struct, rust_struct


def test_many_certificate_layouts_match_the_header_ctypes_and_integration_md():
    header = c_struct("relp_many_certificate")
    assert [f[0] for f in header] == ["struct_size", "certified", "path", "fallback_reason", "digits_primal", "digits_dual",
                                      "repair_pivots", "host_seconds"]
    assert ctypes_struct(ManyCertificate) == header
    assert rust_struct("RelpManyCertificate") == header
    assert C.sizeof(ManyCertificate) == sum(width * count for _, _, width, count in header) == 40


def test_the_fallback_reasons_of_the_header_are_the_ones_python_names():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "relp_amd.h")).read()
    found = dict((name, int(value)) for name, value in re.findall(r"RELP_MANY_FALLBACK_([A-Z_]+) = (\d+)", text))
    assert found == {name: value for value, name in enumerate(relp_amd.api.MANY_FALLBACK_NAMES)}
    assert relp_amd.api.MANY_FALLBACK_NAMES == ["NONE", "KIND", "WIDTH", "SINGULAR_MOD_P", "DIGITS", "SIGN"]


def test_the_symbols_are_exported():
    for name in ("relp_many_certify", "relp_many_certify_lds_rows"):
        assert name in relp_amd.SYMBOLS and hasattr(relp_amd.lib(), name)
    # 4 m^2 bytes of work matrix beside 28 m bytes of vectors and 1 KiB of scalars in the 160 KiB of a CU
    rows = relp_amd.lib().relp_many_certify_lds_rows()
    assert 4 * rows * rows + 28 * rows + 1024 <= 160 * 1024 < 4 * (rows + 1) ** 2 + 28 * (rows + 1) + 1024
    assert rows == 198


def test_bad_arguments_are_refused_without_a_device():
    lib = relp_amd.lib()
    out = (ManyCertificate * 1)()
    out[0].struct_size = C.sizeof(ManyCertificate)
    device, wall = C.c_double(-1.0), C.c_double(-1.0)
    assert lib.relp_many_certify(None, 0, out, C.byref(device), C.byref(wall)) == ERR_ARGUMENT  # NULL handle
    assert (device.value, wall.value) == (0.0, 0.0)
    fake = C.c_void_p(C.addressof(C.create_string_buffer(8)))  # never dereferenced: `out` and its size are looked at first
    assert lib.relp_many_certify(fake, 0, None, None, None) == ERR_ARGUMENT  # NULL out
    out[0].struct_size = C.sizeof(ManyCertificate) - 8
    assert lib.relp_many_certify(fake, 0, out, None, None) == ERR_ARGUMENT  # a size no header ever had
    out[0].struct_size = 0
    assert lib.relp_many_certify(fake, 1, out, None, None) == ERR_ARGUMENT
