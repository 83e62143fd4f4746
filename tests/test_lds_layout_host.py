"""CPU: the dynamic-LDS layouts of the one-workgroup-per-spectrum kernels (csrc/lds_layout.hpp: one function per kernel, called by the
kernel for its pointers and by the launcher for the size) under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone
program with its own main (tests/c/lds_layout_host.cpp) that carves a heap buffer of exactly the requested size with every layout.
Nothing of it is loaded into this process and nothing touches a GPU."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_lds_layouts_under_sanitizers(tmp_path):
    cxx = next((c for c in ("g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "lds_layout_host")
    # (the sanitizers' runtimes are linked statically: clang's default, asked of gcc)
    static = [] if "clang" in cxx else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static,
                    "-I", os.path.join(ROOT, "hybrid-drt_amd", "csrc"), os.path.join(ROOT, "tests", "c", "lds_layout_host.cpp"),
                    "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "lds layouts ok" in run.stdout
