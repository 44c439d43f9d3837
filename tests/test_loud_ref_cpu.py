"""CPU: the loudness definition without the device.  (1) Known answers of the numpy referee the GPU tests lean on (tests/loud_refs.py): a
997 Hz sine of amplitude 1 measures -3.01 LUFS, and the coefficient construction reproduces the 48 kHz table of ITU-R BS.1770.  (2) The
planner and host evaluator (csrc/fs_loud_plan.h) under their host check (tools/loud_plan_check.cpp), built with the host compiler and run --
no sanitizer flags here, the ASan / UBSan build is the command in the program's header, run by hand.  (3) The admission rule of the case
table: no block of any case lies within 0.01 LU of either gate, so no device-against-referee comparison hinges on a gate flipping.  (4)
Teeth: the referee with a gate disabled moves L by more than 1 LU where that gate is at work.  The gap case is built so that BOTH gates
decide it (the absolute gate drops the silent blocks, which lifts the relative gate over the second burst); the quiet-passage case is the
relative gate's -- a signal of two levels, both above -70 LUFS, has no block the absolute gate could drop, so that fourth combination has
nothing to show and is asserted to be exactly that."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import loud_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_loud_plan_host_check(tmp_path):
    cxx = shutil.which("c++") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "loud_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tools", "loud_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout
    assert r.stdout.splitlines()[-1:] == ["loud_plan_check ok"], r.stdout


def test_full_scale_997_hz_sine_is_minus_3_01_lufs():
    x = R.signal("sine", 3 * 44100, 44100)
    assert np.abs(x).max() > 0.9999
    r = R.measure(x, 44100)
    assert abs(r["lufs"] - (-3.01)) <= 0.01, r["lufs"]
    assert r["blocks_total"] == 27 and r["blocks_kept"] == 27 and r["peak"] == np.abs(x).max()


def test_48_khz_coefficients_are_the_table_of_bs1770():
    (b0, b1, b2, a1, a2), (d1, d2) = R.coefs(48000)
    got = (b0, b1, b2, a1, a2, d1, d2)
    want = (1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585, -1.99004745483398, 0.99007225036621)
    assert all(abs(g - w) <= 1e-12 for g, w in zip(got, want)), got


def test_hops_and_blocks_at_the_edges():
    assert [R.hop(r) for r in (8000, 8004, 8005, 11025, 44100, 48000)] == [800, 800, 801, 1103, 4410, 4800]
    for rate in R.RATES:
        h = R.hop(rate)
        x = R.signal("mix", 5 * h, rate, 1)
        assert [R.measure(x[:n], rate)["blocks_total"] for n in (4 * h - 1, 4 * h, 4 * h + 1, 5 * h - 1, 5 * h)] == [0, 1, 1, 1, 2]
        r = R.measure(x[:4 * h - 1], rate)
        assert r["lufs"] == -math.inf and R.gain(r["lufs"], r["peak"], R.TARGET) == np.float32(1.0)


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_no_case_has_a_block_near_a_gate(case):
    r = R.reference(case)
    l = r["l"][~np.isnan(r["l"])]
    assert np.all(np.abs(l + 70.0) > 0.01), np.abs(l + 70.0).min()
    if not math.isnan(r["gamma"]):
        assert np.all(np.abs(l - r["gamma"]) > 0.01), np.abs(l - r["gamma"]).min()
    assert r["blocks_total"] == max(case[1] // R.hop(case[2]) - 3, 0)


def test_cases_reach_every_clause():
    kinds = {c[0]: R.reference(c) for c in R.SIGNALS[:7]}
    g = {k: (10.0 ** ((R.TARGET - r["lufs"]) / 20.0), 10.0 ** (R.MAX_GAIN_DB / 20.0), 10.0 ** (R.PEAK_DB / 20.0) / float(r["peak"])) for k, r in kinds.items()}
    assert min(g["spike"]) == g["spike"][2] and g["spike"][2] < 0.5 * min(g["spike"][:2])   # the peak clause decides
    assert min(g["under"]) == g["under"][1] and abs(kinds["under"]["lufs"] - (R.TARGET - 50.0)) < 0.05  # 50 LU under: max_gain_db decides
    assert min(g["mix"]) == g["mix"][0]                                                         # the target decides
    assert 0 < kinds["nan"]["blocks_kept"] < kinds["nan"]["blocks_total"] and kinds["nan"]["peak"] > 0 and math.isfinite(kinds["nan"]["lufs"])
    assert 0 < kinds["gap"]["blocks_kept"] < kinds["gap"]["blocks_total"] and 0 < kinds["quiet"]["blocks_kept"] < kinds["quiet"]["blocks_total"]
    # lengths: one that is no multiple of the chunk or the span, rows of several workgroups
    assert all(n % R.CHUNK and n % R.SPAN and n > R.SPAN for n in (R.edge_lengths(r)[-1] for r in R.RATES)) and R.LONG > 8 * R.SPAN


def test_teeth_a_skipped_gate_moves_the_loudness_by_more_than_1_lu():
    kind, n, rate, seed = R.GAP
    x, L = R.reference(R.GAP)["x"], R.reference(R.GAP)["lufs"]
    assert abs(R.measure(x, rate, absolute=False)["lufs"] - L) > 1.0
    assert abs(R.measure(x, rate, relative=False)["lufs"] - L) > 1.0
    kind, n, rate, seed = R.QUIET
    x, L = R.reference(R.QUIET)["x"], R.reference(R.QUIET)["lufs"]
    assert abs(R.measure(x, rate, relative=False)["lufs"] - L) > 1.0
    assert R.reference(R.QUIET)["l"].min() > -70.0 and R.measure(x, rate, absolute=False)["lufs"] == L  # (docstring: nothing for it to drop)
    # the quiet passage is 15 LU under the loud one
    l = R.reference(R.QUIET)["l"]
    assert abs((l[0] - l[-1]) - 15.0) < 0.1


def test_the_hop_bound_is_small_and_not_vacuous():
    # what 1e-4 LU of L allows a block's energy is 2.3e-5 relative; the derived bound of an audible hop is far inside it at every rate
    for case in R.CASES:
        r = R.reference(case)
        s, b = r["s"], r["bound"]
        fin = np.isfinite(s)
        loud = fin & (np.where(fin, s, 0.0) > 1e-12 * (s[fin].max() if fin.any() else 1.0))
        if loud.any():
            assert (b[loud] / s[loud]).max() < 2e-6, (case, (b[loud] / s[loud]).max())
            assert (b[loud] / s[loud]).min() > 100 * R.U
