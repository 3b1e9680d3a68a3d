"""Stand-alone sanitizer check of the histogram arithmetic.

tests/native/lathist_check.cpp includes only _native/lathist.h and has
its own main(); it is built with AddressSanitizer and UBSan and run as an
ordinary program (nothing is loaded into Python).
"""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "lathist_check.cpp")
INC = os.path.join(ROOT, "cueball_amd", "_native")


def find_compiler():
    for name in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if name:
            path = shutil.which(name)
            if path:
                return path
    return None


def test_header_is_python_free():
    with open(os.path.join(INC, "lathist.h")) as f:
        includes = [ln for ln in f if ln.lstrip().startswith("#include")]
    assert includes and not any("Python.h" in ln for ln in includes)


def test_lathist_check_under_sanitizers(tmp_path):
    cxx = find_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "lathist_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
            "-fno-sanitize-recover=undefined", "-I", INC, SRC, "-o", exe]
    # Link the sanitizer runtimes into the program where the toolchain
    # has them as archives (gcc needs the flags, clang does so by
    # default): it then runs the same whatever else the environment
    # loads into processes.  Fall back to the toolchain's default.
    build = None
    for extra in (["-static-libasan", "-static-libubsan"], []):
        build = subprocess.run(base + extra, capture_output=True,
                               text=True, timeout=170)
        if build.returncode == 0:
            break
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "lathist ok" in run.stdout
