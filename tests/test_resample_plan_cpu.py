"""CPU: the sample-rate conversion planner (csrc/fs_resample_plan.h) under its host check (tools/resample_plan_check.cpp: hand-computed output
lengths and values of both definitions, the tap tables of the six rate pairs, and a seeded random walk over chunk lengths that asserts the
stream book's invariants after every step), built with the host compiler and run.  No sanitizer flags here -- the suite also runs on GPU
machines; the ASan / UBSan build is the command in the program's header, run by hand."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_resample_plan_host_check(tmp_path):
    cxx = shutil.which("c++") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "resample_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tools", "resample_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout
    assert r.stdout.splitlines()[-1:] == ["resample_plan_check ok"], r.stdout
