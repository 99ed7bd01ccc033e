"""CPU-side checks of the importance-sampling entry points (ag2_detect_importance and friends): declared, exported,
bound by the harness, struct layouts equal to the header's as a C compiler lays them out, and the C++ driver of the
device opt-in compiles against the mirror headers."""
import ctypes
import os
import subprocess

import pytest

import __graft_entry__ as entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "agile_grasp2_amd", "csrc", "libag2hip.so")
HOST_DIR = os.path.join(ROOT, "agile_grasp2_amd", "host")
CSRC_DIR = os.path.join(ROOT, "agile_grasp2_amd", "csrc")

NEW = ["ag2_default_importance_params", "ag2_detect_importance", "ag2_importance_sample",
       "ag2_get_importance_rounds", "ag2_get_importance_info"]


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(LIB):
        entry.build()
    return LIB


def test_importance_symbols_declared_exported_and_bound(built):
    from agile_grasp2_amd import capi
    declared = entry.declared_symbols()
    exported = entry.exported_symbols(built)
    for s in NEW:
        assert s in declared and s in exported and s in capi.SYMBOLS, s


def _c_layout(tmp, struct, fields):
    """sizeof and offsetof of `fields` of `struct`, as gcc lays out include/ag2_c.h."""
    src = os.path.join(tmp, "layout.c")
    body = "".join(f'  printf("%zu\\n", offsetof({struct}, {f}));\n' for f in fields)
    open(src, "w").write("#include <stddef.h>\n#include <stdio.h>\n#include \"ag2_c.h\"\nint main(void) {\n"
                         f'  printf("%zu\\n", sizeof({struct}));\n{body}  return 0;\n}}\n')
    exe = os.path.join(tmp, "layout")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
    vals = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    return vals[0], dict(zip(fields, vals[1:]))


@pytest.mark.parametrize("name", ["ImportanceParams", "ImportanceInfo"])
def test_importance_struct_layouts_match_header(tmp_path, name):
    from agile_grasp2_amd import capi
    mirror = getattr(capi, name)
    struct = {"ImportanceParams": "ag2_importance_params", "ImportanceInfo": "ag2_importance_info"}[name]
    fields = [f for f, _ in mirror._fields_]
    size, offs = _c_layout(str(tmp_path), struct, fields)
    assert ctypes.sizeof(mirror) == size
    for f in fields:
        assert getattr(mirror, f).offset == offs[f], f


def test_importance_params_defaults(built):
    """importance_sampling.cpp:9-15: 5 rounds of 50 samples, 30 % random, radius 0.02, MAX."""
    from agile_grasp2_amd import capi
    p = capi.default_importance_params()
    assert (p.num_iterations, p.num_samples, p.prob_rand_samples, p.radius, p.method) == (5, 50, 0.3, 0.02, capi.IS_MAX)
    assert capi.IS_SUM == 1 and capi.IMPORTANCE_MAX_ROUNDS == 64


def build_importance_driver(tmp):
    subprocess.check_call(["make", "-C", CSRC_DIR, "-s", "-j", "8"])
    subprocess.check_call(["make", "-C", HOST_DIR, "-s"])
    exe = os.path.join(tmp, "importance_device")
    subprocess.check_call([
        "g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "importance_device.cpp"), "-o", exe,
        "-L", HOST_DIR, "-lag2host", "-L", CSRC_DIR, "-lag2hip",
        f"-Wl,-rpath,{HOST_DIR}", f"-Wl,-rpath,{CSRC_DIR}"])
    return exe


def test_importance_driver_builds(tmp_path):
    exe = build_importance_driver(str(tmp_path))
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr   # nothing touched the GPU
