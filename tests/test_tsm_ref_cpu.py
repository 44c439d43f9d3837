"""CPU: the time-stretch definition without the device.  (1) The planner and host evaluator (csrc/fs_tsm_plan.h) under their host check
(tools/tsm_plan_check.cpp: hand-computed lengths, positions and tie-rule chains), built with the host compiler and run -- no sanitizer flags
here, the ASan / UBSan build is the command in the program's header, run by hand.  (2) The numpy referee the GPU tests lean on
(tests/tsm_refs.py): the consequences the header states, the tiers of the case table, and teeth -- the referee tells a contracted
overlap-add and a wrong tie rule apart from the right ones on the listed cases."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import tsm_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tsm_plan_host_check(tmp_path):
    cxx = shutil.which("c++") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "tsm_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tools", "tsm_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout
    assert r.stdout.splitlines()[-1:] == ["tsm_plan_check ok"], r.stdout


def test_plan_lengths_and_nominal_positions():
    # worked by hand (the same pairs as tools/tsm_plan_check.cpp)
    assert R.plan(0, 1.25)[:2] == (0, 0) and R.plan(100, 0.5)[:2] == (200, 1) and R.plan(1280, 1.25)[:2] == (1024, 2)
    assert R.plan(1281, 1.25)[:2] == (1025, 3) and R.plan(10, 4.0)[0] == 3 and R.plan(1, 4.0)[0] == 0
    assert R.plan(1000, 0.77)[2].tolist() == [0, 394, 788] and R.plan(4608, 3.0)[2].tolist() == [0, 1536, 3072]


def test_speed_one_is_the_identity_chain():
    x = R.signal("voiced", 9000, 3)
    pos, ties = R.chain64(x, 1.0)
    assert pos.tolist() == [512 * k for k in range(len(pos))] and len(pos) == 18 and not ties.any()
    y = R.ola_f32(x, pos, 1.0)
    assert y.shape == x.shape and np.array_equal(y[:512], x[:512])
    assert np.all(np.abs(y - x) <= 2.4e-7 * np.abs(x))  # w[i] + w[i + Hs] is 1 up to an ulp, and so are the two roundings


def test_silence_picks_lag_zero_and_periodic_the_smaller_lag():
    for kind, n, seed, speed in R.CRAFTED:
        x = R.signal(kind, n, seed)
        pos, ties = R.chain_of(kind, n, seed, speed)
        _, K, q = R.plan(n, speed)
        assert not ties.any(), (kind, speed)  # (the GPU test compares these chains bit for bit)
        d = pos - q
        if kind == "silence_gap":
            # frames whose template and whole search region lie inside the gap: every error is 0
            lo, hi = n // 2 - 1500, n // 2 + 1500
            inside = [k for k in range(1, K) if pos[k - 1] + 512 >= lo and pos[k - 1] + 1536 <= hi and q[k] - 512 >= lo and q[k] + 1536 <= hi]
            assert inside and all(d[k] == 0 for k in inside), (speed, inside)
        else:
            # frames that read no sample outside [0, n): the lags a period apart tie at exactly 0; the one nearest 0 wins
            full = [k for k in range(1, K) if q[k] - 512 >= 0 and q[k] + 1536 <= n and pos[k - 1] + 1536 <= n]
            assert len(full) >= 3
            for k in full:
                e = R.errors64(x, int(pos[k - 1]), int(q[k]))
                zeros = np.flatnonzero(e == 0.0) - 512
                assert len(zeros) >= 6 and set(np.diff(zeros)) == {147} and abs(d[k]) == np.abs(zeros).min() <= 73, (speed, k)
            assert any(d[k] != R.first_min(R.errors64(x, int(pos[k - 1]), int(q[k]))) for k in full)


@pytest.mark.parametrize("case", R.EXACT, ids=lambda c: "%s-%d-%d-%g" % c)
def test_exact_tier_has_no_near_tie_frame(case):
    kind, n, seed, speed = case
    pos, ties = R.chain_of(kind, n, seed, speed)
    assert len(pos) >= 8 and not ties.any(), np.flatnonzero(ties).tolist()


@pytest.mark.parametrize("case", R.REFEREED, ids=lambda c: "%s-%d-%d-%g" % c)
def test_refereed_tier_has_near_ties_within_the_cap(case):
    kind, n, seed, speed = case
    pos, ties = R.chain_of(kind, n, seed, speed)
    assert 1 <= int(ties.sum()) <= R.cap_of(len(pos) - 1), (int(ties.sum()), len(pos))
    # the reference chain replayed along itself: every pick admitted, none differs
    r = R.replay(R.signal(kind, n, seed), speed, pos)
    assert r["admitted"] and r["differ"] == 0 and r["stray"] == 0 and r["worst"] == 0.0


def test_teeth_contracted_ola_and_first_minimum_tie_rule_differ():
    fused = chains = 0
    for kind, n, seed, speed in R.EXACT + R.CRAFTED:
        x = R.signal(kind, n, seed)
        pos, _ = R.chain_of(kind, n, seed, speed)
        fused += not np.array_equal(R.ola_f32(x, pos, speed), R.ola_f32(x, pos, speed, fused=True))
    for kind, n, seed, speed in R.CRAFTED:
        x = R.signal(kind, n, seed)
        wrong, _ = R.chain64(x, speed, pick=R.first_min)
        chains += not np.array_equal(wrong, R.chain_of(kind, n, seed, speed)[0])
    assert fused >= 1 and chains >= 1, (fused, chains)
    # and the replay refuses a chain that is off by one sample somewhere
    kind, n, seed, speed = R.EXACT[3]
    pos = R.chain_of(kind, n, seed, speed)[0].copy()
    pos[5] += 1
    r = R.replay(R.signal(kind, n, seed), speed, pos)
    assert not r["admitted"] or r["stray"] >= 1
