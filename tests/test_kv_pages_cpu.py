"""CPU: the KV page book (csrc/fs_kv_pages.h) under its host check (tools/kv_pages_check.cpp: scripted sessions and a seeded random walk,
check() and a page-id-by-page-id comparison with a naive model after every operation), built with the host compiler and run.  No
sanitizer flags here -- the suite also runs on GPU machines; the ASan / UBSan build is the command in the program's header, run by hand."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kv_pages_host_check(tmp_path):
    cxx = shutil.which("c++") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "kv_pages_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tools", "kv_pages_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout
    assert r.stdout.splitlines()[-1:] == ["kv_pages_check ok"], r.stdout
