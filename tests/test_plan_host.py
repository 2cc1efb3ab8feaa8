"""The host-only construction helpers (iqlpref_amd/csrc/host_plan.h: workspace planner, dropout constants)
checked by a stand-alone C++ program, tests/c_abi/plan_check.cpp: system compiler, no HIP, no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_workspace_plan_and_dropout_constants(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler on this box")
    exe = str(tmp_path / "plan_check")
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", os.path.join(ROOT, "tests", "c_abi", "plan_check.cpp"),
                    "-I", os.path.join(ROOT, "iqlpref_amd", "csrc"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout + run.stderr
