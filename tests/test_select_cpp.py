"""csrc/dif_select.h, the run-time value -> compile-time constant selectors of every launcher, checked by a stand-alone host
program (tests/cpp/select_test.cpp, its own main) built with AddressSanitizer and UndefinedBehaviorSanitizer.  The program runs
as a child process and is never loaded into Python.  No GPU, no HIP."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "cpp", "select_test.cpp")


def host_compiler():
    for name in (os.environ.get("CXX"), "g++", "clang++", "c++", "/opt/rocm/lib/llvm/bin/clang++"):
        path = name and shutil.which(name)
        if path:
            return path
    return None


def test_selectors_reach_exactly_the_asked_instantiation(tmp_path):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "select_test")
    # the sanitizer runtimes are linked statically: the program runs whatever else the loader brings in first
    clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static = ["-static-libsan"] if clang else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-g", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined"] + static + [SOURCE, "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "select_test OK" in run.stdout, run.stdout + run.stderr


def test_the_selector_header_needs_no_hip():
    text = open(os.path.join(ROOT, "difformer_amd", "csrc", "dif_select.h")).read()
    assert "#include <hip" not in text and "__device__" not in text and "__global__" not in text
