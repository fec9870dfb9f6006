"""``relp_many_certify`` mode 2 and ``relp_many_get_certificate_digits`` on a machine without a GPU: the symbol, the mode enum, the
arguments refused before the device, and the certificate struct at the size it has always had."""
import ctypes as C
import os
import re

import relp_amd
from relp_amd.api import ERR_ARGUMENT, MANY_CERTIFY_ALL_KINDS, MANY_CERTIFY_MODE_NAMES, MANY_CERTIFY_OPTIMA, MANY_CERTIFY_SERIAL, ManyCertificate
from test_struct_layouts import c_struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_digits_accessor_is_exported_listed_and_documented():
    name = "relp_many_get_certificate_digits"
    assert name in relp_amd.SYMBOLS and hasattr(relp_amd.lib(), name)
    with open(os.path.join(ROOT, "include", "relp_amd.h")) as handle:
        assert "int32_t %s(const relp_many* many, int32_t model, int32_t digits[3]);" % name in handle.read()
    with open(os.path.join(ROOT, "INTEGRATION.md")) as handle:
        assert "fn %s(" % name in handle.read()
    digits = (C.c_int32 * 3)(7, 7, 7)
    assert relp_amd.lib().relp_many_get_certificate_digits(None, 0, digits) == ERR_ARGUMENT  # NULL handle
    assert tuple(digits) == (7, 7, 7)


def test_the_modes_of_the_header_are_the_ones_python_names():
    with open(os.path.join(ROOT, "include", "relp_amd.h")) as handle:
        text = handle.read()
    body = re.search(r"typedef enum relp_many_certify_mode \{(.*?)\} relp_many_certify_mode;", text, flags=re.S).group(1)
    found = dict((name, int(value)) for name, value in re.findall(r"RELP_MANY_CERTIFY_([A-Z_]+) = (\d+)", body))
    assert found == {name: value for value, name in enumerate(MANY_CERTIFY_MODE_NAMES)}
    assert (MANY_CERTIFY_OPTIMA, MANY_CERTIFY_SERIAL, MANY_CERTIFY_ALL_KINDS) == (0, 1, 2)
    assert MANY_CERTIFY_MODE_NAMES == ["OPTIMA", "SERIAL", "ALL_KINDS"]
    assert not re.search(r"RELP_MANY_FALLBACK_[A-Z_]+", body)  # (that prefix belongs to the reasons)
    with open(os.path.join(ROOT, "INTEGRATION.md")) as handle:
        integration = handle.read()
    for name, value in found.items():
        assert re.search(r"\b%s = %d\b" % ("".join(part.capitalize() for part in name.split("_")), value), integration), name


def test_mode_2_refuses_bad_arguments_without_a_device():
    lib = relp_amd.lib()
    out = (ManyCertificate * 1)()
    out[0].struct_size = C.sizeof(ManyCertificate)
    device, wall = C.c_double(-1.0), C.c_double(-1.0)
    assert lib.relp_many_certify(None, MANY_CERTIFY_ALL_KINDS, out, C.byref(device), C.byref(wall)) == ERR_ARGUMENT  # NULL handle
    assert (device.value, wall.value) == (0.0, 0.0)
    fake = C.c_void_p(C.addressof(C.create_string_buffer(8)))  # never dereferenced: `out`, its size and the mode are looked at first
    assert lib.relp_many_certify(fake, MANY_CERTIFY_ALL_KINDS, None, None, None) == ERR_ARGUMENT  # NULL out
    for mode in (3, -1):
        assert lib.relp_many_certify(fake, mode, out, None, None) == ERR_ARGUMENT  # not a mode
    out[0].struct_size = C.sizeof(ManyCertificate) + 8
    assert lib.relp_many_certify(fake, MANY_CERTIFY_ALL_KINDS, out, None, None) == ERR_ARGUMENT  # a size no header ever had


def test_the_certificate_struct_keeps_its_40_bytes():
    header = c_struct("relp_many_certificate")
    assert [f[0] for f in header] == ["struct_size", "certified", "path", "fallback_reason", "digits_primal", "digits_dual",
                                      "repair_pivots", "host_seconds"]
    assert C.sizeof(ManyCertificate) == sum(width * count for _, _, width, count in header) == 40
