"""CPU: the server's use of shared session prefixes (fishrt/server.py `AppState(session_prefixes=True)`) and SessionStreamer's pass-through,
against stand-in LM / session objects that record how they are driven.  A prefix is created once per voice and session and hit afterwards,
the per-session map is an LRU of Scheduler.PREFIX_LRU, a prefix the KV pool cannot hold falls back to the full prompt, the map dies with
the session, and every request still gets the codes of its own full prompt."""
import threading

import numpy as np

from fishrt import server
from fishrt.stream import SessionStreamer


def _codes_of(prompt):
    """what the fake generates for a full prompt: frames depend on the whole prompt"""
    n = 3 + int(prompt[0].sum()) % 4
    return np.full((8, n), int(prompt[0].sum()) % 997, np.uint32)


class FakeLM:
    def __init__(self, prefix_capacity=100):
        self.cfg = dict(num_codebooks=8)
        self.max_batch, self.calls, self.lock, self.prefix_capacity = 4, [], threading.Lock(), prefix_capacity
        self.gate, self.entered = threading.Event(), threading.Event()  # entered: a batch-1 call has started
        self.gate.set()

    def clear_slow_layer_caches(self):
        pass

    def clear_slow_caches_until(self, pos):
        pass

    def curr_kv_size(self):
        return 0

    def generate_blocking(self, prompt, max_new_tokens, **kw):
        self.entered.set()
        self.gate.wait(10)
        self.calls.append(("single", prompt.shape[1]))
        return _codes_of(prompt)

    def session(self, **kw):
        return FakeSession(self)


class FakeSession:
    def __init__(self, lm):
        assert lm.lock.acquire(blocking=False)
        self.lm, self.slots, self.prefixes, self.next_pid = lm, {}, {}, 0
        lm.calls.append(("session",))

    def close(self):
        self.lm.calls.append(("session_end", len(self.prefixes)))
        self.lm.lock.release()

    def add_prefix(self, prompt):
        if len(self.prefixes) >= self.lm.prefix_capacity:
            self.lm.calls.append(("add_prefix_full",))
            return None
        pid = self.next_pid
        self.next_pid += 1
        self.prefixes[pid] = np.array(prompt)
        self.lm.calls.append(("add_prefix", pid, prompt.shape[1]))
        return pid

    def release_prefix(self, pid):
        del self.prefixes[pid]
        self.lm.calls.append(("release_prefix", pid))

    def add(self, prompt, max_new_tokens, prefix=None):
        free = [i for i in range(4) if i not in self.slots]
        if not free:
            return None
        full = prompt if prefix is None else np.concatenate([self.prefixes[prefix], prompt], 1)
        self.slots[free[0]] = [_codes_of(full), 0]
        self.lm.calls.append(("add", prefix, prompt.shape[1]))
        return free[0]

    def step(self, n):
        for v in self.slots.values():
            v[1] = min(v[0].shape[1], v[1] + n)
        return sum(v[1] < v[0].shape[1] for v in self.slots.values())

    def poll(self, slot, codes=True):
        full, n = self.slots[slot]
        return (full[:, :n].copy(), n == full.shape[1]) if codes else (n, n == full.shape[1])

    def release(self, slot):
        del self.slots[slot]


class Tok:
    def encode(self, text):
        return list(text.encode())

    def token_to_id(self, token):
        return {"<|semantic:0|>": 1000, "<|semantic|>": 5}.get(token)


def _voice(k, n=20):
    c = np.zeros((9, n), np.uint32)
    c[0] = 100 + k + np.arange(n)
    return c


def _body(i, n=6):
    b = np.zeros((9, n), np.uint32)
    b[0] = 7 * i + np.arange(n)
    return b


def _run(jobs, session_prefixes=True, prefix_capacity=100):
    """jobs: list of (voice index or None, body index); all queued behind a blocker so that they take the session path"""
    lm = FakeLM(prefix_capacity)
    ls = server.LMState(lm, Tok(), {}, None, max_new_tokens=64, max_batch=4)
    sch = server.Scheduler(ls, 0.0, True, session_prefixes=session_prefixes)
    lm.gate.clear()
    blocker = sch.submit(None, _body(999), 0, True)  # lone job: the batch-1 path, held at the gate while the rest is queued
    assert lm.entered.wait(10), "the blocker did not take the batch-1 path"
    futs = []
    for v, b in jobs:
        cond = None if v is None else _voice(v)
        futs.append((sch.submit(cond, _body(b), 0 if cond is None else cond.shape[1], True), cond, _body(b)))
    lm.gate.set()
    blocker.result(10)
    for f, cond, body in futs:
        full = body if cond is None else np.concatenate([cond, body], 1)
        assert np.array_equal(f.result(10), _codes_of(full))
    sch.close()
    return sch, lm


def test_prefixes_are_created_once_per_voice_and_hit_afterwards():
    jobs = [(0, 1), (1, 2), (0, 3), (0, 4), (1, 5), (None, 6), (0, 7)]
    sch, lm = _run(jobs)
    created = [c for c in lm.calls if c[0] == "add_prefix"]
    assert [c[2] for c in created] == [20, 20] and len(created) == 2
    adds = [c for c in lm.calls if c[0] == "add"]
    assert len(adds) == len(jobs)
    assert sum(c[1] is not None for c in adds) == 6 and all(c[2] == 6 for c in adds if c[1] is not None)
    assert sch.stats["session_prefix_hits"] == 4 and sch.stats["session_prefix_tokens_saved"] == 4 * 20
    assert not sch.prefixes  # the map is dropped with the session


def test_lru_evicts_the_least_recently_used_prefix():
    n = server.Scheduler.PREFIX_LRU
    jobs = [(v, v) for v in range(n + 2)] + [(0, 50)]
    sch, lm = _run(jobs)
    released = [c[1] for c in lm.calls if c[0] == "release_prefix"]
    assert released == [0, 1, 2]  # voices 0 and 1 were the oldest; voice 0 comes back as a new prefix and evicts voice 2
    created = [c for c in lm.calls if c[0] == "add_prefix"]
    assert len(created) == n + 3
    assert sch.stats["session_prefix_hits"] == 0


def test_a_prefix_the_pool_cannot_hold_falls_back_to_the_full_prompt():
    jobs = [(0, 1), (1, 2), (1, 3)]
    sch, lm = _run(jobs, prefix_capacity=1)
    adds = [c for c in lm.calls if c[0] == "add"]
    assert adds[0][1] == 0 and adds[1][1] is None and adds[1][2] == 26 and adds[2][1] is None
    assert ("add_prefix_full",) in lm.calls


def test_option_off_never_touches_prefixes():
    sch, lm = _run([(0, 1), (0, 2), (1, 3)], session_prefixes=False)
    assert not any(c[0] in ("add_prefix", "release_prefix", "add_prefix_full") for c in lm.calls)
    assert all(c[1] is None and c[2] == 26 for c in lm.calls if c[0] == "add")
    assert "session_prefix_hits" not in sch.stats


def test_app_state_option_reaches_the_scheduler():
    lm = FakeLM()
    ls = server.LMState(lm, Tok(), {}, None, max_new_tokens=64, max_batch=4)
    st = server.AppState(ls, None, session_prefixes=True)
    assert st.scheduler.session_prefixes
    st.scheduler.close()
    st = server.AppState(ls, None)
    assert not st.scheduler.session_prefixes
    st.scheduler.close()


class _RecSession:
    def __init__(self):
        self.adds = []

    def add(self, prompt, max_new_tokens, prefix=None):
        self.adds.append((prompt, max_new_tokens, prefix))
        return len(self.adds) - 1


class _Codec:
    def __init__(self):
        self.n = 0

    def streams_open(self):
        self.n += 1
        return self.n

    def streams_close(self, sid):
        pass


def test_session_streamer_passes_the_prefix_through():
    sess = _RecSession()
    st = SessionStreamer(sess, _Codec())
    assert st.add("body", 30, prefix=3) == 0
    assert st.add("plain", 31) == 1
    assert sess.adds == [("body", 30, 3), ("plain", 31, None)]
