"""CPU: prefix KV blobs without a GPU.  (a) fishrt.prefix_blob_info on hand-packed headers (include/fishrt.h: fs_kv_blob_header): the good
one and every bad field, each refused with a ValueError that names the field.  (b) the scheduler's host cache of blobs
(fishrt/server.py `AppState(session_prefixes=True, prefix_host_cache_bytes=N)`) against the stand-in LM / session objects of
test_session_prefix_cpu.py, extended with export_prefix / import_prefix: a voice is imported, not prefilled again, after its session has
closed or after the per-session LRU evicted it; every prefix is exported once; the byte budget drops the least recently used blob; an
import the KV pool cannot hold falls back to the full prompt; with the option off the sessions are driven exactly as before."""
import struct

import numpy as np
import pytest

import fishrt
from fishrt import server
from test_session_prefix_cpu import FakeLM, FakeSession, Tok, _body, _codes_of, _voice

HDR = struct.Struct("<8sIIiiiiIIQQQ")
GOOD = dict(magic=b"FSKVPFX1", version=1, kv_dtype=1, n_layer=2, n_local_heads=2, head_dim=32, P=65, header_bytes=64, reserved=0,
            weights_fingerprint=0x0123456789ABCDEF, payload_bytes=2 * 2 * 65 * 2 * 32 * 2, reserved2=0)


def _blob(payload=None, **over):
    f = dict(GOOD, **over)
    body = bytes(GOOD["payload_bytes"] if payload is None else payload)
    return HDR.pack(*[f[k] for k in GOOD]) + body


def test_header_is_64_bytes_and_matches_the_ctypes_mirror():
    import ctypes
    from fishrt import _ffi
    assert HDR.size == 64 == ctypes.sizeof(_ffi.KvBlobHeader)
    h = _ffi.KvBlobHeader.from_buffer_copy(_blob()[:64])
    assert (h.magic, h.version, h.kv_dtype, h.n_layer, h.n_local_heads, h.head_dim, h.P, h.header_bytes) == (b"FSKVPFX1", 1, 1, 2, 2, 32, 65, 64)
    assert h.weights_fingerprint == GOOD["weights_fingerprint"] and h.payload_bytes == GOOD["payload_bytes"]


def test_prefix_blob_info_reads_a_good_header():
    info = fishrt.prefix_blob_info(_blob())
    for k, v in GOOD.items():
        assert info[k] == (v.decode() if k == "magic" else v), k
    assert info["bytes"] == 64 + GOOD["payload_bytes"]
    assert fishrt.prefix_blob_info(bytearray(_blob()))["P"] == 65
    # f32 KV storage: 4 bytes per element
    assert fishrt.prefix_blob_info(_blob(kv_dtype=0, payload_bytes=2 * GOOD["payload_bytes"], payload=2 * GOOD["payload_bytes"]))["kv_dtype"] == 0


@pytest.mark.parametrize("blob,field", [
    (_blob(magic=b"FSKVPFX2"), "magic"),
    (_blob(version=2), "version"),
    (_blob(header_bytes=128), "header_bytes"),
    (_blob()[:-1], r"bytes = \d+ != 64 \+ payload_bytes"),
    (_blob() + b"\0", r"bytes = \d+ != 64 \+ payload_bytes"),
    (_blob()[:40], "bytes"),
    (_blob(kv_dtype=2), "kv_dtype"),
    (_blob(n_layer=0), "n_layer"),
    (_blob(n_local_heads=-2), "n_local_heads"),
    (_blob(head_dim=36), "head_dim"),
    (_blob(P=0), "P = 0"),
    (_blob(n_layer=3), "payload_bytes"),
    (_blob(P=64), "payload_bytes"),
], ids=["magic", "version", "header_bytes", "truncated", "padded", "short", "kv_dtype", "n_layer", "n_local_heads", "head_dim", "P", "dims-n_layer",
        "dims-P"])
def test_prefix_blob_info_names_the_bad_field(blob, field):
    with pytest.raises(ValueError, match=field):
        fishrt.prefix_blob_info(blob)


# ---- the scheduler's host cache

BLOB_BYTES = 9 * 20 * 4  # a stand-in blob is the voice's prompt (20 columns) as bytes


class BlobLM(FakeLM):
    def __init__(self, prefix_capacity=100, import_capacity=100):
        super().__init__(prefix_capacity)
        self.import_capacity = import_capacity

    def session(self, **kw):
        return BlobSession(self)


class BlobSession(FakeSession):
    def export_prefix(self, pid):
        self.lm.calls.append(("export_prefix", pid))
        return self.prefixes[pid].astype(np.uint32).tobytes()

    def import_prefix(self, blob):
        if len(self.prefixes) >= self.lm.import_capacity:
            self.lm.calls.append(("import_prefix_full",))
            return None
        pid = self.next_pid
        self.next_pid += 1
        self.prefixes[pid] = np.frombuffer(blob, np.uint32).reshape(9, -1).copy()
        self.lm.calls.append(("import_prefix", pid, self.prefixes[pid].shape[1]))
        return pid


def _scheduler(lm, **kw):
    ls = server.LMState(lm, Tok(), {}, None, max_new_tokens=64, max_batch=4)
    return server.Scheduler(ls, 0.0, True, session_prefixes=True, **kw)


def _burst(sch, lm, jobs):
    """one burst of (voice, body) jobs through ONE session: queued behind a lone blocker job (the batch-1 path, held at the gate), so
    that all of them take the session path; returns once every job has its codes.  The session closes at the lull that follows."""
    n0 = len(lm.calls)
    lm.entered.clear()
    lm.gate.clear()
    blocker = sch.submit(None, _body(999), 0, True)
    assert lm.entered.wait(10), "the blocker did not take the batch-1 path"
    futs = [(sch.submit(_voice(v), _body(b), 20, True), np.concatenate([_voice(v), _body(b)], 1)) for v, b in jobs]
    lm.gate.set()
    blocker.result(10)
    for f, full in futs:
        assert np.array_equal(f.result(10), _codes_of(full))
    return n0


def _names(calls, *which):
    return [c for c in calls if c[0] in which]


def test_a_voice_is_imported_after_its_session_has_closed_and_exported_once():
    lm = BlobLM()
    sch = _scheduler(lm, prefix_host_cache_bytes=10_000)
    _burst(sch, lm, [(0, 1), (0, 2)])
    n1 = _burst(sch, lm, [(0, 3), (0, 6)])  # (a burst is two jobs at least: a lone job takes the batch-1 path)
    n2 = _burst(sch, lm, [(0, 4), (0, 5)])
    sch.close()
    assert len(_names(lm.calls, "session")) == 3  # every burst had a session of its own
    assert len(_names(lm.calls, "add_prefix")) == 1 and len(_names(lm.calls, "export_prefix")) == 1
    # the export comes when the first session is about to close
    i_exp, i_end = lm.calls.index(_names(lm.calls, "export_prefix")[0]), lm.calls.index(_names(lm.calls, "session_end")[0])
    assert i_exp < i_end and not _names(lm.calls[i_exp:i_end], "add", "session")
    assert n1 < n2 and not _names(lm.calls[n1:], "add_prefix", "export_prefix")
    assert [c[2] for c in _names(lm.calls, "import_prefix")] == [20, 20]
    assert all(c[1] is not None and c[2] == 6 for c in _names(lm.calls, "add"))  # every job prefilled its body only
    assert sch.stats["session_prefix_imports"] == 2 and sch.stats["session_prefix_import_tokens"] == 40
    assert sch.stats["prefix_host_cache_bytes"] == BLOB_BYTES
    assert sch.stats["session_prefix_hits"] == 3  # (the second job of every burst: the prefix was in the session's map; an import is no hit)


def test_a_voice_evicted_from_the_session_lru_is_imported():
    n = server.Scheduler.PREFIX_LRU
    lm = BlobLM()
    sch = _scheduler(lm, prefix_host_cache_bytes=100_000)
    _burst(sch, lm, [(v, v) for v in range(n + 2)] + [(0, 50)])
    sch.close()
    assert len(_names(lm.calls, "add_prefix")) == n + 2  # voice 0 is NOT created a second time
    imp = _names(lm.calls, "import_prefix")
    assert len(imp) == 1 and imp[0][2] == 20
    # voices 0 and 1 were exported when the LRU dropped them, right before their release; the others when the session closed; each once
    exported = [c[1] for c in _names(lm.calls, "export_prefix")]
    assert sorted(exported) == list(range(n + 2)) and exported[:2] == [0, 1]
    for pid in (0, 1):
        i = lm.calls.index(("export_prefix", pid))
        assert lm.calls[i + 1] == ("release_prefix", pid)
    assert sch.stats["session_prefix_imports"] == 1
    assert sch.stats["prefix_host_cache_bytes"] == (n + 2) * BLOB_BYTES


def test_the_byte_budget_drops_the_least_recently_used_blob():
    lm = BlobLM()
    sch = _scheduler(lm, prefix_host_cache_bytes=2 * BLOB_BYTES + 100)
    _burst(sch, lm, [(0, 1), (1, 2), (2, 3)])
    assert sch.stats["prefix_host_cache_bytes"] == 2 * BLOB_BYTES and len(sch.host_blobs) == 2
    n1 = _burst(sch, lm, [(1, 4), (1, 8)])    # voice 1 becomes the most recently used blob
    n2 = _burst(sch, lm, [(0, 5), (0, 9)])    # voice 0 had been dropped: created again; its new blob drops voice 2
    n3 = _burst(sch, lm, [(2, 6), (1, 7)])
    sch.close()
    assert _names(lm.calls[n1:n2], "import_prefix") and not _names(lm.calls[n1:n2], "add_prefix")
    assert _names(lm.calls[n2:n3], "add_prefix") and not _names(lm.calls[n2:n3], "import_prefix")
    last = lm.calls[n3:]
    assert len(_names(last, "add_prefix")) == 1 and len(_names(last, "import_prefix")) == 1  # voice 2 prefilled, voice 1 imported
    assert sch.stats["prefix_host_cache_bytes"] <= 2 * BLOB_BYTES + 100
    # a blob larger than the whole budget is not kept at all
    lm2 = BlobLM()
    sch2 = _scheduler(lm2, prefix_host_cache_bytes=BLOB_BYTES - 1)
    _burst(sch2, lm2, [(0, 1), (0, 3)])
    _burst(sch2, lm2, [(0, 2), (0, 4)])
    sch2.close()
    assert len(_names(lm2.calls, "add_prefix")) == 2 and not _names(lm2.calls, "import_prefix") and sch2.stats["prefix_host_cache_bytes"] == 0


def test_an_import_the_pool_cannot_hold_falls_back_to_the_full_prompt():
    lm = BlobLM()
    sch = _scheduler(lm, prefix_host_cache_bytes=10_000)
    _burst(sch, lm, [(0, 1), (0, 3)])
    lm.import_capacity = 0
    n1 = _burst(sch, lm, [(0, 2), (0, 4)])
    sch.close()
    burst = lm.calls[n1:]
    assert ("import_prefix_full",) in burst and not _names(burst, "add_prefix", "import_prefix")
    adds = _names(burst, "add")
    assert len(adds) == 2 and all(a[1] is None and a[2] == 26 for a in adds)
    assert sch.stats["session_prefix_imports"] == 0 and sch.stats["prefix_host_cache_bytes"] == BLOB_BYTES  # the blob stays cached


def test_a_refused_blob_is_dropped_and_the_voice_prefilled_again():
    class Refusing(BlobSession):
        def import_prefix(self, blob):
            raise RuntimeError("prefix blob: weights_fingerprint differs from this handle's")

    lm = BlobLM()
    sch = _scheduler(lm, prefix_host_cache_bytes=10_000)
    _burst(sch, lm, [(0, 1), (0, 3)])
    lm.session = lambda **kw: Refusing(lm)
    n1 = _burst(sch, lm, [(0, 2), (0, 4)])
    assert len(_names(lm.calls[n1:], "add_prefix")) == 1
    sch.close()
    assert len(_names(lm.calls, "export_prefix")) == 2  # the new session's prefix replaces the refused blob


def test_a_prefix_is_not_exported_while_its_creating_job_is_still_prefilling():
    lm = BlobLM()
    sch = _scheduler(lm, prefix_host_cache_bytes=10_000)
    try:
        sess = BlobSession(lm)
        j = server._Job(_voice(0), _body(1), 20, True)
        sch.prefixes.clear()
        slot, hit = sch._session_add(sess, j)
        assert slot is not None and not hit and sch.prefix_makers[j.cond_key] is j
        pid = sch.prefixes[j.cond_key]
        sch._stash(sess, j.cond_key, pid)  # no frame yet: the slot is still prefilling
        assert not _names(lm.calls, "export_prefix") and not sch.host_blobs
        sess.step(8)
        sch._stash(sess, j.cond_key, pid)
        sch._stash(sess, j.cond_key, pid)
        assert len(_names(lm.calls, "export_prefix")) == 1 and list(sch.host_blobs) == [j.cond_key]
        sess.close()
    finally:
        sch.close()


def test_option_off_drives_the_session_exactly_as_before():
    jobs = [(0, 1), (1, 2), (0, 3)] + [(v, 10 + v) for v in range(2, server.Scheduler.PREFIX_LRU + 2)] + [(0, 30)]
    runs = []
    for kw in (dict(), dict(prefix_host_cache_bytes=0)):
        lm = BlobLM()
        sch = _scheduler(lm, **kw)
        _burst(sch, lm, jobs)
        _burst(sch, lm, [(0, 40), (1, 41)])
        sch.close()
        runs.append((lm.calls, sch.stats))
    # the same jobs against the stand-ins WITHOUT export / import methods: nothing of the feature is touched
    lm = FakeLM()
    sch = _scheduler(lm)
    _burst(sch, lm, jobs)
    _burst(sch, lm, [(0, 40), (1, 41)])
    sch.close()
    runs.append((lm.calls, sch.stats))
    for calls, stats in runs:
        assert calls == runs[2][0] and stats == runs[2][1]
        assert not _names(calls, "export_prefix", "import_prefix", "import_prefix_full")
        assert not {"session_prefix_imports", "session_prefix_import_tokens", "prefix_host_cache_bytes"} & set(stats)
    assert len(_names(runs[0][0], "add_prefix")) == server.Scheduler.PREFIX_LRU + 5  # (every burst and every eviction prefills again)


def test_app_state_option_reaches_the_scheduler_and_needs_session_prefixes():
    lm = BlobLM()
    ls = server.LMState(lm, Tok(), {}, None, max_new_tokens=64, max_batch=4)
    st = server.AppState(ls, None, session_prefixes=True, prefix_host_cache_bytes=4096)
    assert st.scheduler.host_budget == 4096 and st.scheduler.stats["prefix_host_cache_bytes"] == 0
    st.scheduler.close()
    st = server.AppState(ls, None, session_prefixes=True)
    assert st.scheduler.host_budget == 0 and "session_prefix_imports" not in st.scheduler.stats
    st.scheduler.close()
    with pytest.raises(ValueError, match="session_prefixes"):
        server.AppState(ls, None, prefix_host_cache_bytes=4096)
