"""The layering of relp_amd/csrc (CPU; no library needed): which files reach the host class ``Solver``, which headers stay clear of
the host model and the host Markowitz factorisation, which headers compile without HIP, and where the launch boilerplate lives."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "relp_amd", "csrc")
FILES = sorted(name for name in os.listdir(CSRC) if name.endswith((".hpp", ".hip", ".cpp")))
TEXT = {name: open(os.path.join(CSRC, name)).read() for name in FILES}
INCLUDES = {name: [i for i in re.findall(r'^\s*#\s*include\s+"([^"]+)"', text, flags=re.M) if i in TEXT] for name, text in TEXT.items()}

# the files that name `Solver` (batch.cpp may join them when it needs the class)
MAY_REACH_SOLVER = {"solver.hpp", "solver.hip", "capi.cpp", "many.hip", "dual.hip", "network_carry.hip", "batch.cpp"}
DEVICE_LAYER = ["wave_ops.hpp", "pivot_step.hpp", "price_step.hpp", "kernels.hpp", "device_lp.hpp", "launch.hpp"]
HOST_ONLY = ["options.hpp", "kernel_path.hpp", "kernel_limits.hpp"]


def reachable(name):
    """Every file of csrc that `name` includes, directly or through other files of csrc (itself included)."""
    seen, stack = {name}, [name]
    while stack:
        for included in INCLUDES[stack.pop()]:
            if included not in seen:
                seen.add(included)
                stack.append(included)
    return seen


def test_the_walk_sees_the_includes():
    assert "kernel_limits.hpp" in reachable("kernels.hip") and "solver.hpp" in reachable("solver.hip")
    assert len(FILES) > 40 and all(name in TEXT for name in DEVICE_LAYER + HOST_ONLY)


def test_solver_hpp_is_reached_only_by_the_files_that_name_solver():
    reaching = {name for name in FILES if "solver.hpp" in reachable(name)}
    assert reaching <= MAY_REACH_SOLVER, sorted(reaching - MAY_REACH_SOLVER)


@pytest.mark.parametrize("header", DEVICE_LAYER)
def test_device_layer_headers_do_not_reach_the_host_model(header):
    assert not reachable(header) & {"model.hpp", "lu_host.hpp", "solver.hpp"}, sorted(reachable(header))


def host_compiler():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    candidates = [shutil.which("clang++"), os.path.join(rocm, "llvm", "bin", "clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++")]
    found = [c for c in candidates if c and os.path.exists(c)]
    assert found, "no clang++ on PATH or under %s" % rocm
    return found[0]


@pytest.mark.parametrize("header", HOST_ONLY)
def test_host_only_headers_compile_without_hip(header, tmp_path):
    source = tmp_path / "one_line.cpp"
    source.write_text('#include "%s"\n' % header)
    # a plain C++ translation unit: no -x hip, no HIP include path
    run = subprocess.run([host_compiler(), "-std=c++17", "-fsyntax-only", "-I", CSRC, str(source)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert not any("hip" in included for name in reachable(header) for included in re.findall(r"#\s*include\s+<([^>]+)>", TEXT[name]))


def test_the_dynamic_lds_opt_in_is_written_once():
    assert [name for name in FILES if "hipFuncAttributeMaxDynamicSharedMemorySize" in TEXT[name]] == ["launch.hpp"]


def test_no_reproducer_flavour_is_left():
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert "REPRO" not in makefile
    assert [name for name in FILES if "REPRO" in TEXT[name]] == []
