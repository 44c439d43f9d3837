"""CPU: the collector slots' bookkeeping (csrc/fs_slot_book.h) under its host check (tools/slot_book_check.cpp: both instantiations, the
in-hand rule, every allocation freed at exit), built with the host compiler and run.  No sanitizer flags here -- the suite also runs on
GPU machines; the ASan / UBSan build is the command in the program's header, run by hand."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_slot_book_host_check(tmp_path):
    cxx = shutil.which("c++") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "slot_book_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tools", "slot_book_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout
    assert r.stdout.splitlines()[-1:] == ["slot_book_check ok"], r.stdout
