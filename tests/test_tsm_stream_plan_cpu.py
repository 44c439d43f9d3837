"""CPU: the chunked time stretch without the device.  (1) The emission rule, the carry start, the derived carry bound and the chunk-by-chunk
evaluator of csrc/fs_tsm_plan.h under their host check (tools/tsm_stream_plan_check.cpp), built with the host compiler and run -- no
sanitizer flags here, the ASan / UBSan build is the command in the program's header, run by hand.  The program prints every step of every
sequence it walks; the numpy restatement the GPU tests lean on (tests/tsm_stream_refs.py) is held to those lines, so the two cannot drift
apart.  (2) The restatement's own sweep: monotone emission, no emitted frame reads at or beyond n or below the carry, the carry within the
bound, the totals equal out_len(n).  (3) fishrt.SessionStreamer's speed arguments against a fake session and a fake codec."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import tsm_refs as R
import tsm_stream_refs as S
from fishrt.stream import SessionStreamer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_lines(tmp_path_factory):
    cxx = shutil.which("c++") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("tsm_stream") / "tsm_stream_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tools", "tsm_stream_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-2000:]
    return r.stdout.splitlines()


def test_tsm_stream_plan_host_check(host_lines):
    assert host_lines[-1:] == ["tsm_stream_plan_check ok"], host_lines[-5:]


def test_numpy_rule_equals_the_header_step_by_step(host_lines):
    cases = [ln for ln in host_lines if ln.startswith("case ")]
    assert len(cases) >= 8 * 5 * 6
    seen, one_sample_chunks = set(), 0
    for ln in cases:
        head, steps = ln[5:].split(" :")
        speed, N, D, bound = head.split()
        speed, N, D, bound = float(speed), int(N), int(D), int(bound)
        seen.add((speed, N, D))
        assert bound == S.carry_bound(speed, N, D), ln[:80]
        rows = [tuple(int(v) for v in st.split(",")) for st in steps.split()]
        assert rows and all(r[1] == (i + 1 == len(rows)) for i, r in enumerate(rows))
        one_sample_chunks += sum(r[0] == 1 for r in rows)
        mine = S.walk([r[0] for r in rows], speed, N, D)
        for r, m in zip(rows, mine):
            assert (r[2], r[3], r[4], r[5]) == (m["k0"], m["k1"], m["n_emit"], m["carry_start"]), (ln[:60], r, m)
    assert seen == {(s, N, D) for s in S.SPEEDS for N, D in S.PARAMS}
    assert one_sample_chunks > 100


@pytest.mark.parametrize("N,D", S.PARAMS)
def test_rule_sweep(N, D):
    hs = N // 2
    for speed in S.SPEEDS:
        n = int(np.ceil(speed * hs * 9.3)) + 2 * D + 17
        bound = S.carry_bound(speed, N, D)
        lists = [[n], S.ragged(n, 3, 1, 2 * N), S.even(n, 300), S.ragged(n, 4, 1, 3) + [0]]
        if N <= 256:
            lists.append([1] * n)
        for chunks in lists:
            steps = S.walk(chunks, speed, N, D)
            cs_in = 0
            for st in steps[:-1]:
                # a prefix: every frame below k1 is emittable at n, none of the next ones
                assert all(S.emittable(k, st["n"], speed, N, D) == (k < st["k1"]) for k in range(st["k1"] + 12)), (speed, st)
                for k in range(st["k0"], st["k1"]):
                    lo, hi = S.reads(k, speed, N, D)
                    assert hi <= st["n"] and lo >= cs_in, (speed, k, lo, hi, st, cs_in)
                assert st["n"] - st["carry_start"] <= bound and st["carry_start"] >= cs_in, (speed, st, bound)
                cs_in = st["carry_start"]
            assert sum(st["n_emit"] for st in steps) == S.out_len(n, speed) == R.plan(n, speed, N)[0]
            assert steps[-1]["k1"] == R.plan(n, speed, N)[1]
    # the first clause is needed: at speed 4.0 with the defaults (D + N) / speed = 384 < Hs
    if (N, D) == (R.FRAME, R.RADIUS):
        n = S.q_of(3, 4.0) + D + N
        assert n >= S.hi_of(2, 4.0) + hs + N and 4 * hs > S.out_len(n, 4.0) and not S.emittable(3, n, 4.0)
        assert S.carry_bound(4.0) == 4098 and S.carry_bound(0.25) == 2433


def test_edge_lengths_and_an_empty_stream():
    for speed in S.SPEEDS:
        for n in (0, 1, 511, 512, 513):
            for chunks in ([n], [n, 0], [n // 2, n - n // 2], [1] * n or [0]):
                assert sum(S.emitted(chunks, speed)) == S.out_len(n, speed)
    assert S.emitted([0], 1.25) == [0] and S.emitted([0, 0], 0.5) == [0, 0]
    # Hs input samples do not make frame 0 emittable when speed > 1: it is not yet a whole frame of the final length
    assert S.emitted([512, 0], 2.0) == [0, 256] and S.emitted([512, 0], 0.5) == [512, 512]


# ---- SessionStreamer(speed=) against fakes
SPF = 4


class FakeCodec:
    def __init__(self):
        self.opened, self.open, self.calls = [], {}, []

    def streams_open(self, **kw):
        self.opened.append(kw)
        self.open[len(self.opened) - 1] = kw
        return len(self.opened) - 1

    def streams_close(self, sid):
        del self.open[sid]

    def streams_decode_ragged(self, ids, chunks, final=None):
        self.calls.append(([int(i) for i in ids], [c.shape[1] for c in chunks], None if final is None else [bool(f) for f in final]))
        # a speed stream holds everything back until its final item
        out = []
        for i, c, f in zip(ids, chunks, final if final is not None else [False] * len(ids)):
            held = self.open[i].setdefault("_held", 0) + c.shape[1]
            if "speed" in self.open[i] and not f:
                self.open[i]["_held"] = held
                out.append(np.zeros(0, np.float32))
            else:
                self.open[i]["_held"] = 0
                out.append(np.zeros(held * SPF if "speed" in self.open[i] else c.shape[1] * SPF, np.float32))
        return out


class FakeSession:
    """a request is reported done one step after its last frame arrived, so a request whose length is a multiple of the chunk finishes
    with no frames left"""

    def __init__(self, lengths):
        self.lengths, self.slots = lengths, {}

    def add(self, prompt, max_new_tokens):
        slot = len(self.slots)
        self.slots[slot] = [int(prompt), 0, False]
        return slot

    def step(self, k):
        for st in self.slots.values():
            st[2] = st[1] == self.lengths[st[0]]
            st[1] = min(st[1] + k, self.lengths[st[0]])
        return sum(not st[2] for st in self.slots.values())

    def poll(self, slot, codes=True):
        i, n, done = self.slots[slot]
        return (np.zeros((8, n), np.uint32), done) if codes else (n, done)

    def release(self, slot):
        del self.slots[slot]


def test_session_streamer_speed_needs_ragged():
    with pytest.raises(ValueError, match="ragged=True"):
        SessionStreamer(FakeSession([8]), FakeCodec(), chunk=16, first_chunk=16, speed=1.25)
    ss = SessionStreamer(FakeSession([8]), FakeCodec(), chunk=16, first_chunk=16)
    with pytest.raises(ValueError, match="ragged=True"):
        ss.add(0, 0, speed=1.25)
    assert ss.codec.opened == [] and ss.live == {}  # refused before anything was opened


def test_session_streamer_passes_speeds_and_always_flushes():
    codec, sess = FakeCodec(), FakeSession([8, 8, 8, 5])
    got = {i: [] for i in range(4)}
    ss = SessionStreamer(sess, codec, chunk=4, first_chunk=4, ragged=True, speed=0.8, sample_rate=24000,
                         on_audio=lambda tag, pcm, final: got[tag].append((len(pcm), final)))
    ss.add(0, 0, tag=0)
    ss.add(1, 0, tag=1, speed=1.5)
    assert [kw.get("speed") for kw in codec.opened] == [0.8, 1.5] and all(kw["sample_rate"] == 24000 for kw in codec.opened)
    plain = SessionStreamer(sess, codec, chunk=4, first_chunk=4, ragged=True, on_audio=lambda tag, pcm, final: got[tag].append((len(pcm), final)))
    plain.add(2, 0, tag=2)
    plain.add(3, 0, tag=3, speed=2.0)
    assert "speed" not in codec.opened[2] and codec.opened[3] == dict(speed=2.0)
    for _ in range(3):
        ss.step(4)
        plain.step(0)
    # requests 0 and 1 are reported done with no frames left: the speed streams still get their flush item (T = 0, final); the plain
    # request 2 ends with its last 4 frames, and never sees an empty item
    flushes = [(i, T) for ids, Ts, fin in codec.calls if fin for i, T, f in zip(ids, Ts, fin) if f]
    assert sorted(flushes) == [(0, 0), (1, 0), (2, 4), (3, 1)], codec.calls
    assert all(not (i == 2 and T == 0) for ids, Ts, _ in codec.calls for i, T in zip(ids, Ts))
    assert got[0][-1] == (8 * SPF, True) and got[1][-1] == (8 * SPF, True) and got[3][-1] == (5 * SPF, True)
    assert codec.open == {} and sorted(ss.results) == [0, 1] and sorted(plain.results) == [2, 3]
