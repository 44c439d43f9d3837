"""GPU: prefix KV blobs (fs_lm_weights_fingerprint / fs_lm_session_prefix_export / fs_lm_session_prefix_import, include/fishrt.h).
Import restores the cache bytes, so no comparison here has a tolerance: a blob's payload IS the cache rows of a slot on the prefix, an
imported prefix gives the codes and the KV rows of the created one bit for bit (on a pool that held other data before, and with a
one-column body admitted in the same host step), a blob moves between session kinds and between handles with equal weights, every
malformed or foreign blob is refused by field name with the pool untouched, and an export changes nothing in a running session."""
import ctypes as C
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bench
import fishrt
from fishrt import _ffi
from fishrt import config as fcfg

SEED = 0xF15E5EED
MID = dict(fcfg.TINY, dim=256, n_head=4, n_local_heads=2, head_dim=64, intermediate_size=1024)
TOK15 = fcfg.FISH_1_5_TOKENS
CONFIGS = pytest.mark.parametrize("cfg,dtype", [(fcfg.TINY, "bf16"), (MID, "bf16"), (MID, "fp8")], ids=["hd32", "hd64", "hd64-fp8"])
PS = (1, 63, 64, 65, 130)  # one row, both sides of a page boundary, three pages with a partly filled last one
BODIES = (1, 7, 40)
GREEDY = dict(temp=0.0, top_p=1.0, top_k=0, seed=42, ignore_eos=True)
HDR = struct.Struct("<8sIIiiiiIIQQQ")
FIELDS = ("magic", "version", "kv_dtype", "n_layer", "n_local_heads", "head_dim", "P", "header_bytes", "reserved", "weights_fingerprint",
          "payload_bytes", "reserved2")


def _prompt(rng, L):
    p = np.zeros((9, L), np.uint32)
    p[0] = rng.randint(0, 400, L)
    k = min(L - 1, 5)
    if k > 0:  # a VQ span so that codebook embeddings take part
        p[0, 1 : 1 + k] = fcfg.TINY_TOKENS["semantic_start_id"] + rng.randint(0, 64, k)
        p[1:, 1 : 1 + k] = rng.randint(0, 64, (8, k))
    return p


def _prompt15(L, seed):
    p = np.zeros((9, L), np.uint32)
    p[0] = np.random.RandomState(seed).randint(0, TOK15["im_end_id"], L)
    return p


def _lm(cfg, dtype, seed=SEED, max_batch=4):
    return fishrt.DualARTransformer(cfg, fcfg.TINY_TOKENS, 0, dtype, max_batch=max_batch).load_synthetic(seed)


def _pages(n):
    return (n + 63) // 64


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _payload_f32(blob, cfg, P):
    """the payload [n_layer][2][P][n_local_heads][head_dim] of bf16 elements -> f32"""
    pay = np.frombuffer(blob, np.uint16, offset=64).reshape(cfg["n_layer"], 2, P, cfg["n_local_heads"], cfg["head_dim"])
    return (pay.astype(np.uint32) << 16).view(np.float32)


def _drain(s, live):
    out = {}
    while live:
        s.step(8)
        for slot in list(live):
            if s.poll(slot, codes=False)[1]:
                out[live.pop(slot)] = s.poll(slot)[0]
                s.release(slot)
    return out


def _rewrite(blob, payload=None, **over):
    f = dict(zip(FIELDS, HDR.unpack_from(blob, 0)), **over)
    return HDR.pack(*[f[k] for k in FIELDS]) + (blob[64:] if payload is None else payload)


@CONFIGS
def test_payload_equals_the_cache(cfg, dtype):
    lm = _lm(cfg, dtype)
    fp = lm.weights_fingerprint()
    rng = np.random.RandomState(11)
    with lm.session(**GREEDY) as s:
        for P in PS:
            pid = s.add_prefix(_prompt(rng, P))
            slot = s.add(_prompt(rng, 3), P + 3 + 4, prefix=pid)
            s.step(1)
            before = s.info()
            blob = s.export_prefix(pid)
            assert s.info() == before
            h = fishrt.prefix_blob_info(blob)
            nbytes = cfg["n_layer"] * 2 * P * cfg["n_local_heads"] * cfg["head_dim"] * 2
            assert h == dict(magic="FSKVPFX1", version=1, kv_dtype=1, n_layer=cfg["n_layer"], n_local_heads=cfg["n_local_heads"],
                             head_dim=cfg["head_dim"], P=P, header_bytes=64, reserved=0, weights_fingerprint=fp, payload_bytes=nbytes,
                             reserved2=0, bytes=64 + nbytes), (P, h)
            pay = _payload_f32(blob, cfg, P)
            for layer in range(cfg["n_layer"]):
                k, v = lm.debug_read_kv(layer, 0, P, slot=slot)
                assert np.array_equal(_bits(pay[layer, 0]), _bits(k)) and np.array_equal(_bits(pay[layer, 1]), _bits(v)), (P, layer)
                assert np.abs(k).max() > 0 and np.abs(v).max() > 0
            s.release(slot)
            s.release_prefix(pid)


def _run_on_prefix(lm, s, P, bodies, make_prefix, check_import=False):
    """the prefix (make_prefix(s) -> id) and a one-column body in the SAME host step, step() right after; then the other bodies.
    -> (codes per body, K/V rows [0, P) of the one-column slot per layer, prefix id)"""
    cfg = lm.cfg
    before = s.info()
    pid = make_prefix(s)
    assert pid is not None
    if check_import:
        assert s.info()["free_pages"] == before["free_pages"] - _pages(P), P
    live = {s.add(bodies[0], P + bodies[0].shape[1] + 6, prefix=pid): 0}
    s.step(1)
    if check_import:  # no slow-transformer pass ran for the import, and the one-column body prefills nothing
        after = s.info()
        assert (after["prefill_passes"], after["tokens_prefilled"]) == (before["prefill_passes"], before["tokens_prefilled"]), (P, before, after)
    slot0 = next(iter(live))
    kv = [lm.debug_read_kv(layer, 0, P, slot=slot0) for layer in range(cfg["n_layer"])]
    for i in (1, 2):
        live[s.add(bodies[i], P + bodies[i].shape[1] + 6, prefix=pid)] = i
    assert None not in live
    return _drain(s, live), kv, pid


@CONFIGS
def test_import_equals_create_bit_for_bit(cfg, dtype):
    lm = _lm(cfg, dtype)
    rng = np.random.RandomState(23)
    prefixes = {P: _prompt(rng, P) for P in PS}
    bodies = {P: [_prompt(rng, n) for n in BODIES] for P in PS}
    ref, blobs = {}, {}
    with lm.session(**GREEDY) as a:
        for P in PS:
            codes, kv, pid = _run_on_prefix(lm, a, P, bodies[P], lambda s: s.add_prefix(prefixes[P]))
            blobs[P] = a.export_prefix(pid)
            a.release_prefix(pid)
            ref[P] = (codes, kv)
    with lm.session(**GREEDY) as b:
        # dirty the pool: unrelated slots over every page, released again, so that imported pages hold stale rows
        live = {b.add(_prompt(rng, 150), 150 + 35): i for i in range(4)}
        assert None not in live
        _drain(b, live)
        free0 = b.info()["free_pages"]
        for P in PS:
            codes, kv, pid = _run_on_prefix(lm, b, P, bodies[P], lambda s: s.import_prefix(blobs[P]), check_import=True)
            for i in range(len(BODIES)):
                assert codes[i].shape == ref[P][0][i].shape and codes[i].shape[1] >= 6
                assert np.array_equal(codes[i], ref[P][0][i]), (P, BODIES[i])
            for layer, ((k, v), (kr, vr)) in enumerate(zip(kv, ref[P][1])):
                assert np.array_equal(_bits(k), _bits(kr)) and np.array_equal(_bits(v), _bits(vr)), (P, layer)
            assert b.export_prefix(pid) == blobs[P]  # and an imported prefix exports the bytes it was made of
            b.release_prefix(pid)
            assert b.info()["free_pages"] == free0, P
        assert b.info()["live_prefixes"] == 0


@pytest.fixture(scope="module")
def full15():
    """two Fish-1.5-sized bf16 handles with the same synthetic weights"""
    lms = [fishrt.DualARTransformer(fcfg.FISH_1_5, TOK15, 0, "bf16", max_batch=4).load_synthetic(SEED) for _ in range(2)]
    yield lms
    for lm in lms:
        lm.close()


def test_blobs_move_between_session_kinds_and_handles(full15):
    lm1, lm2 = full15
    assert lm1.weights_fingerprint() == lm2.weights_fingerprint()
    P, F = 100, 8
    pre, body = _prompt15(P, 700), _prompt15(12, 701)
    mnt = P + 12 + F - 2
    with lm1.session(**GREEDY) as s:
        pid = s.add_prefix(pre)
        blob = s.export_prefix(pid)  # (waits for the prefix's own pass)
    sampled = dict(sampling=dict(temp=0.7, top_p=0.8, top_k=50, repetition_penalty=1.2), seed=1234)
    with lm2.session(temp=0.7, top_p=0.8, top_k=50, seed=9, ignore_eos=True, per_slot=True) as s:
        own = s.add_prefix(pre)
        imp = s.import_prefix(blob)
        live = {s.add(body, mnt, prefix=own, **sampled): "own", s.add(body, mnt, prefix=imp, **sampled): "imp"}
        out = _drain(s, live)
        assert out["own"].shape == (8, F) and np.array_equal(out["own"], out["imp"])
        assert s.export_prefix(own) == blob and s.export_prefix(imp) == blob  # both handles export the same bytes
    with lm2.session(temp=0.0, top_p=1.0, top_k=0, seed=5, ignore_eos=True, rows=True, repetition_penalty=1.2) as s:
        own = s.add_prefix(pre)
        out_own = _drain(s, {s.add(body, mnt, prefix=own): 0})[0]
    with lm2.session(temp=0.0, top_p=1.0, top_k=0, seed=5, ignore_eos=True, rows=True, repetition_penalty=1.2) as s:
        imp = s.import_prefix(blob)
        before = s.info()
        out_imp = _drain(s, {s.add(body, mnt, prefix=imp): 0})[0]
        assert s.info()["prefill_passes"] - before["prefill_passes"] == 1  # the body's pass only
    assert out_own.shape == (8, F) and np.array_equal(out_own, out_imp)


def test_fullsize_default_voice_import_equals_create(full15):
    """Fish 1.5 bf16 shapes, FS_SESSION_ROWS: the default voice's conditioning (system + user text + the voice's VQ span + <|im_end|>) as the
    prefix, the request text as the body, 12 greedy frames: import in a second session == create in the first"""
    lm = full15[0]
    p = bench.default_voice_prompt(TOK15)
    P = 12 + 48 + 4 + 274 + 1
    pre, body = np.ascontiguousarray(p[:, :P]), np.ascontiguousarray(p[:, P:])
    assert int(pre[0, -1]) == TOK15["im_end_id"] and body.shape[1] == 28
    kw = dict(temp=0.0, top_p=1.0, top_k=0, seed=5, ignore_eos=True, rows=True, repetition_penalty=1.2)
    mnt = p.shape[1] + 12 - 2
    with lm.session(**kw) as s:
        pid = s.add_prefix(pre)
        created = _drain(s, {s.add(body, mnt, prefix=pid): 0})[0]
        blob = s.export_prefix(pid)
    c = fcfg.FISH_1_5
    assert fishrt.prefix_blob_info(blob)["payload_bytes"] == c["n_layer"] * 2 * P * c["n_local_heads"] * c["head_dim"] * 2
    with lm.session(**kw) as s:
        pid = s.import_prefix(blob)
        imported = _drain(s, {s.add(body, mnt, prefix=pid): 0})[0]
        info = s.info()
        assert info["prefill_passes"] == 1 and info["tokens_prefilled"] == body.shape[1] - 1, info
    assert created.shape == (8, 12) and np.array_equal(created, imported)


def test_refusals_name_the_field_and_leave_the_pool_alone():
    lm = _lm(MID, "bf16", max_batch=2)
    other = _lm(MID, "bf16", seed=SEED + 1, max_batch=2)
    fp8 = _lm(MID, "fp8", max_batch=2)
    rng = np.random.RandomState(5)
    pre = _prompt(rng, 65)
    msl = MID["max_seq_len"]

    def blob_of(h):
        with h.session(**GREEDY) as s:
            return s.export_prefix(s.add_prefix(pre))

    good, foreign = blob_of(lm), blob_of(other)
    row = MID["n_layer"] * 2 * MID["n_local_heads"] * MID["head_dim"] * 2  # payload bytes per position
    bad = [
        (_rewrite(good, magic=b"FSKVPFX0"), "magic"),
        (_rewrite(good, version=2), "version"),
        (good[:-1], "bytes"),
        (_rewrite(good, header_bytes=60), "header_bytes"),
        (_rewrite(good, kv_dtype=0), "kv_dtype"),
        (_rewrite(good, n_layer=MID["n_layer"] + 1), "n_layer"),
        (_rewrite(good, n_local_heads=1), "n_local_heads"),
        (_rewrite(good, head_dim=32), "head_dim"),
        (_rewrite(good, P=msl, payload_bytes=row * msl, payload=bytes(row * msl)), "P "),
        (_rewrite(good, P=0, payload_bytes=0, payload=b""), "P "),
        (_rewrite(good, P=64), "payload_bytes"),
        (foreign, "weights_fingerprint"),
    ]
    with lm.session(**GREEDY) as s:
        free0 = s.info()["free_pages"]
        for blob, field in bad:
            with pytest.raises(RuntimeError, match=field):
                s.import_prefix(blob)
            assert s.info()["free_pages"] == free0 and s.info()["live_prefixes"] == 0, field
        pid = s.import_prefix(good)  # the session is fine afterwards
        assert pid is not None and s.info()["free_pages"] == free0 - 2
        with pytest.raises(RuntimeError, match="capacity"):  # cap too small
            buf, n = C.create_string_buffer(64), C.c_size_t(0)
            _ffi.check(_ffi.lib().fs_lm_session_prefix_export(lm._h, pid, buf, C.c_size_t(64), C.byref(n)))
        s.release_prefix(pid)
        with pytest.raises(RuntimeError, match="prefix id"):
            s.export_prefix(pid)
        # a pool with too few free pages: None, not an error
        ids = []
        while len(ids) < 64:
            free = s.info()["free_pages"]
            ids.append(s.import_prefix(good))
            if ids[-1] is None:
                break
            assert s.info()["free_pages"] == free - 2
        assert ids[-1] is None and len(ids) > 1 and free < 2 and s.info()["free_pages"] == free
    with fp8.session(**GREEDY) as s:  # a bf16 blob into an fp8 handle of the same checkpoint: other arena, other K/V
        free0 = s.info()["free_pages"]
        with pytest.raises(RuntimeError, match="weights_fingerprint"):
            s.import_prefix(good)
        assert s.info()["free_pages"] == free0
    # fingerprints: a function of (weights, storage type), stable, recomputed after a reload
    twin = _lm(MID, "bf16", max_batch=1)
    f = lm.weights_fingerprint()
    assert f == lm.weights_fingerprint() == twin.weights_fingerprint()
    assert f == fishrt.prefix_blob_info(good)["weights_fingerprint"]
    assert len({f, other.weights_fingerprint(), fp8.weights_fingerprint()}) == 3
    twin.load_synthetic(SEED + 1)
    assert twin.weights_fingerprint() == other.weights_fingerprint() != f
    pid, n = C.c_int(0), C.c_size_t(0)
    with pytest.raises(RuntimeError, match="no open session"):
        _ffi.check(_ffi.lib().fs_lm_session_prefix_import(lm._h, good, C.c_size_t(len(good)), C.byref(pid)))
    with pytest.raises(RuntimeError, match="no open session"):
        _ffi.check(_ffi.lib().fs_lm_session_prefix_export(lm._h, 0, None, C.c_size_t(0), C.byref(n)))


def test_export_is_inert():
    lm = _lm(MID, "bf16")
    rng = np.random.RandomState(8)
    pre, bodies = _prompt(rng, 100), [_prompt(rng, 9), _prompt(rng, 1)]
    sampled = dict(temp=0.8, top_p=0.9, top_k=40, repetition_penalty=1.2)
    runs = []
    for export in (False, True):
        with lm.session(temp=0.8, top_p=0.9, top_k=40, seed=3, ignore_eos=True, per_slot=True) as s:
            pid = s.add_prefix(pre)
            slots = [s.add(b, 100 + b.shape[1] + 20, prefix=pid, sampling=sampled, seed=100 + i) for i, b in enumerate(bodies)]
            blobs = []
            for _ in range(4):
                s.step(3)
                if export:
                    before = s.info()
                    blobs.append(s.export_prefix(pid))
                    assert s.info() == before
            while s.step(8):
                pass
            runs.append([s.poll(sl)[0] for sl in slots])
            assert not export or (len(set(blobs)) == 1 and len(blobs) == 4)
    for a, b in zip(*runs):
        assert a.shape[1] >= 20 and np.array_equal(a, b)
