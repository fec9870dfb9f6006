"""``relp_set_dual_farkas`` on a machine without a GPU: the header declares it, the library exports it, bad arguments are refused before
the device, and the Python entry points of the dual loop take the keyword."""
import inspect
import os
import re

import relp_amd
from relp_amd.api import ERR_ARGUMENT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_header_declares_the_setter_beside_its_sibling():
    text = open(os.path.join(ROOT, "include", "relp_amd.h")).read()
    assert re.search(r"^int32_t relp_set_dual_farkas\(relp_handle\* handle, int32_t on\);$", text, re.M)
    assert text.index("int32_t relp_set_dual_long_step(") < text.index("int32_t relp_set_dual_farkas(")
    for key in ('"dual_farkas"', '"dual_farkas_row"'):
        assert key in text


def test_the_symbol_is_exported():
    assert "relp_set_dual_farkas" in relp_amd.SYMBOLS and hasattr(relp_amd.lib(), "relp_set_dual_farkas")


def test_bad_arguments_are_refused_without_a_device():
    lib = relp_amd.lib()
    for on in (0, 1, 2):  # a NULL handle: what the sibling setter answers (a handle needs a device: tests/test_gpu_dual_farkas.py has the range)
        assert lib.relp_set_dual_farkas(None, on) == lib.relp_set_dual_long_step(None, on) == ERR_ARGUMENT


def test_the_four_solves_take_the_keyword_and_none_keeps_the_setting():
    for name in ("solve_dual", "solve_dual_from", "solve_dual_bounded", "solve_dual_bounded_from"):
        parameter = inspect.signature(getattr(relp_amd.Solver, name)).parameters["farkas"]
        assert parameter.default is None and parameter.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD, name
    for name in ("solve_dual_bounded", "solve_dual_bounded_from"):  # behind the keyword they had
        assert list(inspect.signature(getattr(relp_amd.Solver, name)).parameters)[-2:] == ["long_step", "farkas"], name
    assert "relp_set_dual_farkas" in inspect.getdoc(relp_amd.Solver.set_dual_farkas)
