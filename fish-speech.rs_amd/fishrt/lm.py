"""Host-side mirror of the reference's LM surface over the C ABI.

`DualARTransformer` mirrors fish_speech_core::lm::DualARTransformer (dual_ar.rs:443-713) +
generate_blocking / generate_static_batch (generate/*.rs); `LM` mirrors the PyO3 class
(fish_speech_python/src/lm.rs:23-199) minus tokenisation (the caller supplies token ids: SURVEY.md §2 row 7)."""
import ctypes as C
import struct

import numpy as np

from . import _ffi, config

DTYPES = {"f32": 0, "bf16": 1, "fp8": 2}


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


KV_BLOB_MAGIC = b"FSKVPFX1"
_KV_BLOB_HEADER = struct.Struct("<8sIIiiiiIIQQQ")  # fs_kv_blob_header (include/fishrt.h), little-endian, 64 bytes
_KV_BLOB_FIELDS = ("magic", "version", "kv_dtype", "n_layer", "n_local_heads", "head_dim", "P", "header_bytes", "reserved",
                   "weights_fingerprint", "payload_bytes", "reserved2")
_KV_ELEM_BYTES = {0: 4, 1: 2}  # fs_dtype of the KV storage -> bytes per element (FS_F32, FS_BF16; fp8 handles keep a bf16 cache)


def prefix_blob_info(blob):
    """Parse and check the header of a prefix KV blob (Session.export_prefix; include/fishrt.h: fs_kv_blob_header) without a GPU.
    -> dict of the header fields plus "bytes" (the blob's length).  Raises ValueError naming the field that is wrong: magic, version,
    header_bytes, bytes (!= 64 + payload_bytes), kv_dtype, the dimensions, payload_bytes (against the dimensions).  What only a handle
    can judge -- the dimensions against the model, P < max_seq_len, weights_fingerprint -- is left to Session.import_prefix."""
    blob = bytes(blob) if not isinstance(blob, (bytes, bytearray, memoryview)) else blob
    n = len(blob)
    if n < _KV_BLOB_HEADER.size:
        raise ValueError(f"prefix blob: bytes = {n} is smaller than the 64-byte header")
    h = dict(zip(_KV_BLOB_FIELDS, _KV_BLOB_HEADER.unpack_from(blob, 0)))
    if h["magic"] != KV_BLOB_MAGIC:
        raise ValueError(f"prefix blob: wrong magic {h['magic']!r} (not {KV_BLOB_MAGIC!r})")
    if h["version"] != 1:
        raise ValueError(f"prefix blob: unsupported version {h['version']} (this package reads version 1)")
    if h["header_bytes"] != _KV_BLOB_HEADER.size:
        raise ValueError(f"prefix blob: header_bytes = {h['header_bytes']}, not 64")
    if n != _KV_BLOB_HEADER.size + h["payload_bytes"]:
        raise ValueError(f"prefix blob: bytes = {n} != 64 + payload_bytes = {64 + h['payload_bytes']} (truncated or padded blob)")
    if h["kv_dtype"] not in _KV_ELEM_BYTES:
        raise ValueError(f"prefix blob: kv_dtype = {h['kv_dtype']} is no KV storage type (0 f32, 1 bf16)")
    for k in ("n_layer", "n_local_heads", "head_dim", "P"):
        if h[k] < 1:
            raise ValueError(f"prefix blob: {k} = {h[k]} must be >= 1")
    if h["head_dim"] % 8:
        raise ValueError(f"prefix blob: head_dim = {h['head_dim']} is no multiple of 8")
    want = h["n_layer"] * 2 * h["P"] * h["n_local_heads"] * h["head_dim"] * _KV_ELEM_BYTES[h["kv_dtype"]]
    if h["payload_bytes"] != want:
        raise ValueError(f"prefix blob: payload_bytes = {h['payload_bytes']} does not match the dimensions "
                         f"(n_layer * 2 * P * n_local_heads * head_dim elements = {want} bytes)")
    h["magic"] = h["magic"].decode()
    h["bytes"] = n
    return h


class DualARTransformer:
    def __init__(self, model_args=None, token_cfg=None, device=0, dtype="bf16", max_batch=1):
        if dtype not in DTYPES:
            raise ValueError(f"Unsupported dtype: {dtype}")  # fish_speech_python/src/utils.rs:25-40
        self.cfg = dict(model_args or config.FISH_1_5)
        self.tok = dict(token_cfg or config.FISH_1_5_TOKENS)
        self.dtype = dtype
        ma = _ffi.ModelArgs(**{k: self.cfg[k] for k, _ in _ffi.ModelArgs._fields_})
        tc = _ffi.TokenCfg(**self.tok)
        h = C.c_void_p()
        _ffi.check(_ffi.lib().fs_lm_create(C.byref(ma), C.byref(tc), int(device), DTYPES[dtype], int(max_batch), C.byref(h)))
        self._h = h
        self.max_batch = max_batch

    def close(self):
        if getattr(self, "_h", None) and _ffi is not None and getattr(_ffi, "lib", None):  # (module globals are gone at interpreter exit)
            _ffi.lib().fs_lm_destroy(self._h)
            self._h = None

    __del__ = close

    # ---- weights
    def load_synthetic(self, seed):
        _ffi.check(_ffi.lib().fs_lm_load_synthetic(self._h, C.c_uint64(seed)))
        return self

    def load_safetensors(self, path):
        _ffi.check(_ffi.lib().fs_lm_load_safetensors(self._h, str(path).encode()))
        return self

    # ---- DualARTransformer methods
    def forward_generate(self, inp, input_pos, want_logits=True):
        """dual_ar.rs:574-635.  inp: u32 (B, C+1, L) or (C+1, L).  Returns (logits (B, V), hidden (B, dim))."""
        inp = _u32(inp)
        if inp.ndim == 2:
            inp = inp[None]
        if inp.ndim != 3 or inp.shape[1] != self.cfg["num_codebooks"] + 1:
            raise ValueError("Input tokens must have num_codebooks + 1 codebooks!")  # dual_ar.rs:535-538
        B, _, L = inp.shape
        logits = np.empty((B, self.cfg["vocab_size"]), np.float32) if want_logits else None
        hidden = np.empty((B, self.cfg["dim"]), np.float32)
        _ffi.check(_ffi.lib().fs_lm_forward_generate(
            self._h, inp.ctypes.data_as(C.POINTER(C.c_uint32)), B, L, int(input_pos),
            logits.ctypes.data_as(C.POINTER(C.c_float)) if want_logits else None,
            hidden.ctypes.data_as(C.POINTER(C.c_float))))
        return logits, hidden

    def forward_generate_fast(self, x, input_pos):
        """dual_ar.rs:638-673.  x: f32 (B, dim).  Returns logits (B, codebook_size)."""
        x = np.ascontiguousarray(x, np.float32).reshape(-1, self.cfg["dim"])
        out = np.empty((x.shape[0], self.cfg["codebook_size"]), np.float32)
        _ffi.check(_ffi.lib().fs_lm_forward_generate_fast(self._h, x.ctypes.data_as(C.POINTER(C.c_float)), x.shape[0],
                                                          int(input_pos), out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def fast_embeddings(self, ids):
        ids = _u32(ids).reshape(-1)
        out = np.empty((ids.size, self.cfg["dim"]), np.float32)
        _ffi.check(_ffi.lib().fs_lm_fast_embed(self._h, ids.ctypes.data_as(C.POINTER(C.c_uint32)), ids.size,
                                               out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def clear_fast_layer_caches(self):
        _ffi.check(_ffi.lib().fs_lm_clear_fast_layer_caches(self._h))

    def clear_slow_layer_caches(self):
        _ffi.check(_ffi.lib().fs_lm_clear_slow_layer_caches(self._h))

    def clear_slow_caches_until(self, pos):
        _ffi.check(_ffi.lib().fs_lm_clear_slow_caches_until(self._h, int(pos)))

    def curr_kv_size(self):
        n = _ffi.lib().fs_lm_curr_kv_size(self._h)
        if n < 0:
            raise RuntimeError(_ffi.lib().fs_last_error().decode())
        return n

    # ---- generation drivers
    def generate_blocking(self, prompt, max_new_tokens, temp=0.7, top_p=0.9, top_k=50, repetition_penalty=1.2, seed=0,
                          ignore_eos=False, on_frame=None, persistent=True, time_kernels=False):
        """generate/single_batch.rs:308-324.  prompt u32 (C+1, L) -> codes u32 (C, n_frames).
        persistent=False sets FS_GEN_NO_PERSIST (per-node graph path; see include/fishrt.h); time_kernels=True sets FS_GEN_TIME_KERNELS
        (measurement mode: HIP events around each persistent kernel, last_stats()["slow_kernel_us" / "fast_kernel_us"])."""
        prompt = _u32(prompt)
        Cb = self.cfg["num_codebooks"]
        if prompt.ndim != 2 or prompt.shape[0] != Cb + 1:
            raise ValueError("Input tokens must have num_codebooks + 1 codebooks!")
        L = prompt.shape[1]
        cap = max(1, max_new_tokens - L + 2) + 1
        out = np.zeros((Cb, cap), np.uint32)
        n = C.c_size_t(0)
        s = _ffi.Sampling(float(temp), float(top_p), int(top_k), float(repetition_penalty))
        cb = _ffi.FRAME_CB(lambda user, idx, codes: int(bool(on_frame(idx, [codes[i] for i in range(Cb)])))) if on_frame \
            else C.cast(None, _ffi.FRAME_CB)
        _ffi.check(_ffi.lib().fs_lm_generate(self._h, prompt.ctypes.data_as(C.POINTER(C.c_uint32)), L, int(max_new_tokens),
                                             C.byref(s), C.c_uint64(seed), (1 if ignore_eos else 0) | (0 if persistent else 2) | (4 if time_kernels else 0),
                                             out.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_size_t(cap), C.byref(n), cb, None))
        return out[:, : n.value].copy()

    def generate_blocking_with_hidden(self, prompt, max_new_tokens, collect_hidden_states=True, temp=0.7, top_p=0.9, top_k=50,
                                      repetition_penalty=1.2, seed=0, ignore_eos=False, persistent=True):
        """generate/single_batch.rs:217-306 -> (codes u32 (C, n_frames), hidden f32 (n_iterations, 1, dim) or None)."""
        prompt = _u32(prompt)
        Cb, D = self.cfg["num_codebooks"], self.cfg["dim"]
        if prompt.ndim != 2 or prompt.shape[0] != Cb + 1:
            raise ValueError("Input tokens must have num_codebooks + 1 codebooks!")
        L = prompt.shape[1]
        cap = max(1, max_new_tokens - L + 2) + 1
        out = np.zeros((Cb, cap), np.uint32)
        hid = np.zeros((cap, D), np.float32) if collect_hidden_states else None
        n, nh = C.c_size_t(0), C.c_size_t(0)
        s = _ffi.Sampling(float(temp), float(top_p), int(top_k), float(repetition_penalty))
        _ffi.check(_ffi.lib().fs_lm_generate_with_hidden(
            self._h, prompt.ctypes.data_as(C.POINTER(C.c_uint32)), L, int(max_new_tokens), C.byref(s), C.c_uint64(seed),
            (1 if ignore_eos else 0) | (0 if persistent else 2), out.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_size_t(cap), C.byref(n),
            hid.ctypes.data_as(C.POINTER(C.c_float)) if collect_hidden_states else None, C.c_size_t(cap), C.byref(nh),
            C.cast(None, _ffi.FRAME_CB), None))
        return out[:, : n.value].copy(), (hid[: nh.value].reshape(nh.value, 1, D).copy() if collect_hidden_states else None)

    def generate_static_batch(self, prompts, max_new_tokens, temp=0.7, top_p=0.9, top_k=50, repetition_penalty=1.2,
                              seed=42, ignore_eos=False, audio_only=True, return_is_audio=False):
        """generate/static_batch.rs:282-390.  prompts: list of u32 (C+1, L_i) -> list of (C, n_i); return_is_audio=True: the reference's full
        return value (codes, is_audio) with is_audio a list of bool arrays (n_i,) -- through fs_lm_generate_static_batch."""
        if return_is_audio or not audio_only:
            return self._generate_static_batch_full(prompts, max_new_tokens, temp, top_p, top_k, repetition_penalty, seed, ignore_eos, audio_only)
        Cb = self.cfg["num_codebooks"]
        ps = [_u32(p) for p in prompts]
        lens = np.array([p.shape[1] for p in ps], np.int32)
        flat = np.concatenate([p.reshape(-1) for p in ps])
        cap = max(1, max_new_tokens - int(lens.max()) + 2) + 1
        out = np.zeros((len(ps), Cb, cap), np.uint32)
        nf = (C.c_size_t * len(ps))()
        s = _ffi.Sampling(float(temp), float(top_p), int(top_k), float(repetition_penalty))
        _ffi.check(_ffi.lib().fs_lm_generate_batch(self._h, flat.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                   lens.ctypes.data_as(C.POINTER(C.c_int)), len(ps), int(max_new_tokens),
                                                   C.byref(s), C.c_uint64(seed), 1 if ignore_eos else 0,
                                                   out.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_size_t(cap), nf))
        return [out[i, :, : nf[i]].copy() for i in range(len(ps))]

    def _generate_static_batch_full(self, prompts, max_new_tokens, temp, top_p, top_k, repetition_penalty, seed, ignore_eos, audio_only):
        Cb = self.cfg["num_codebooks"]
        ps = [_u32(p) for p in prompts]
        lens = np.array([p.shape[1] for p in ps], np.int32)
        flat = np.concatenate([p.reshape(-1) for p in ps])
        cap = max(1, max_new_tokens - int(lens.max()) + 2) + 1
        out = np.zeros((len(ps), Cb, cap), np.uint32)
        isa = np.zeros((len(ps), cap), np.uint8)
        nf = (C.c_size_t * len(ps))()
        s = _ffi.Sampling(float(temp), float(top_p), int(top_k), float(repetition_penalty))
        _ffi.check(_ffi.lib().fs_lm_generate_static_batch(self._h, flat.ctypes.data_as(C.POINTER(C.c_uint32)), lens.ctypes.data_as(C.POINTER(C.c_int)),
                                                          len(ps), int(max_new_tokens), 1 if audio_only else 0, C.byref(s), C.c_uint64(seed),
                                                          1 if ignore_eos else 0, out.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_size_t(cap), nf,
                                                          isa.ctypes.data_as(C.POINTER(C.c_uint8))))
        return [out[i, :, : nf[i]].copy() for i in range(len(ps))], [isa[i, : nf[i]].astype(bool) for i in range(len(ps))]

    def generate_multi(self, prompts, max_new_tokens, temp=0.0, top_p=1.0, top_k=0, repetition_penalty=1.2, seeds=None,
                       ignore_eos=False, persistent=True):
        """R concurrent generate_blocking requests on this handle (fishrt.h: fs_lm_generate_multi): prompts = list of u32 (C+1, L_i);
        max_new_tokens / temp / top_p / top_k / repetition_penalty: one value for all requests or one per request -> list of (C, n_i)."""
        Cb = self.cfg["num_codebooks"]
        ps = [_u32(p) for p in prompts]
        n = len(ps)
        per = lambda v: list(v) if isinstance(v, (list, tuple, np.ndarray)) else [v] * n
        mnt, temps, tps, tks, rps = per(max_new_tokens), per(temp), per(top_p), per(top_k), per(repetition_penalty)
        lens = np.array([p.shape[1] for p in ps], np.int32)
        flat = np.concatenate([p.reshape(-1) for p in ps])
        mn = np.array(mnt, np.int32)
        cap = max(max(1, int(m) - int(l) + 2) for m, l in zip(mnt, lens)) + 1
        out = np.zeros((n, Cb, cap), np.uint32)
        nf = (C.c_size_t * n)()
        ss = (_ffi.Sampling * n)(*[_ffi.Sampling(float(temps[i]), float(tps[i]), int(tks[i]), float(rps[i])) for i in range(n)])
        sd = np.array(list(seeds) if seeds is not None else [0] * n, np.uint64)
        _ffi.check(_ffi.lib().fs_lm_generate_multi(self._h, flat.ctypes.data_as(C.POINTER(C.c_uint32)), lens.ctypes.data_as(C.POINTER(C.c_int)), n,
                                                   mn.ctypes.data_as(C.POINTER(C.c_int)), ss, sd.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                   (1 if ignore_eos else 0) | (0 if persistent else 2),
                                                   out.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_size_t(cap), nf))
        return [out[i, :, : nf[i]].copy() for i in range(n)]

    def rows_supported(self, n, temp=0.0, top_p=1.0, top_k=0, repetition_penalty=1.2):
        """fishrt.h fs_lm_rows_supported: would generate_multi serve n requests with these settings on the request-row kernels?"""
        per = lambda v: list(v) if isinstance(v, (list, tuple, np.ndarray)) else [v] * n
        temps, tps, tks, rps = per(temp), per(top_p), per(top_k), per(repetition_penalty)
        ss = (_ffi.Sampling * n)(*[_ffi.Sampling(float(temps[i]), float(tps[i]), int(tks[i]), float(rps[i])) for i in range(n)])
        ok = C.c_int(0)
        _ffi.check(_ffi.lib().fs_lm_rows_supported(self._h, int(n), ss, C.byref(ok)))
        return bool(ok.value)

    def weights_arena(self):
        """(device pointer, bytes) of the handle's weight arena (fishrt.h: fs_lm_weights_arena) -- for fanout.broadcast_weights"""
        ptr, n = C.c_void_p(), C.c_size_t(0)
        _ffi.check(_ffi.lib().fs_lm_weights_arena(self._h, C.byref(ptr), C.byref(n)))
        return int(ptr.value), int(n.value)

    def adopt_weights(self):
        _ffi.check(_ffi.lib().fs_lm_weights_adopt(self._h))
        return self

    def weights_fingerprint(self):
        """64-bit fingerprint of the weight arena (fishrt.h: fs_lm_weights_fingerprint): equal for handles with the same weights in the
        same storage type, which may exchange prefix KV blobs (Session.export_prefix / import_prefix).  Cached until the next load."""
        out = C.c_uint64(0)
        _ffi.check(_ffi.lib().fs_lm_weights_fingerprint(self._h, C.byref(out)))
        return int(out.value)

    def session(self, temp=0.7, top_p=0.9, top_k=50, seed=42, ignore_eos=False, rows=False, repetition_penalty=1.2, per_slot=False, wide=False,
                score=False, trace=False, alts=0):
        """continuous batching over this handle's max_batch slots (fishrt.h: fs_lm_session_*): `with lm.session(...) as s:`
        per_slot=True: FS_SESSION_PER_SLOT -- every slot samples like its own generate_blocking call (own settings, seed, repetition penalty).
        wide=True (with per_slot=True): FS_SESSION_WIDE_SAMPLER -- slots may also sample nucleus-only (top_k == 0) or with top_k > 256.
        score=True (with per_slot=True): FS_SESSION_SCORE -- the session also takes scoring slots (Session.add_scored / poll_scores).
        trace=True (with per_slot=True, score=True): FS_SESSION_TRACE -- the session also takes traced slots (Session.add(..., trace=True) /
        poll_trace): generating slots that record the log-probs of the tokens they pick.
        alts=N (1 .. 16, with per_slot=True, score=True; 0 = off): FS_SESSION_ALTS -- every scoring and traced slot also records the N most
        likely candidates and the entropy of each decision (Session.poll_alts).
        Fish <= 1.4 token configs (no semantic range) take per_slot=True only; plain and rows sessions raise and say so."""
        return Session(self, temp, top_p, top_k, seed, ignore_eos, rows, repetition_penalty, per_slot, wide, score, trace, alts)

    def generate_turns(self, cond, bodies, max_new_tokens, between=None, temp=0.7, top_p=0.9, top_k=50, repetition_penalty=1.2, seed=42,
                       ignore_eos=False, step_frames=8):
        """The bodies as the turns of ONE conversation (upstream Fish-Speech's long-form mode: the earlier segments -- text and generated
        codes -- stay in the context of the next one), through a per-slot session: turn 0 is add(concat(cond, bodies[0])), turn i + 1 is
        Session.continue_from(turn i's slot, concat(between, bodies[i + 1])), so nothing of the history is ever prefilled again and its
        rows are the very rows that produced the audio.  cond: u32 [C+1, n] or None; bodies[i]: u32 [C+1, L_i] (encode_text("user", chunk)
        + encode_vq(None)); between: u32 [C+1, k] columns that close an assistant turn (the tokens of "<|im_end|>"; None = nothing).
        Every turn gets the frame budget it would have had on cond alone: max_new_tokens raised by what its history adds to its prompt.
        Turn i samples with seed + i.  When history + body + budget no longer fit max_seq_len (or no KV page is free) the turn starts over on cond alone,
        as upstream drops old segments.  -> the list of per-turn codes u32 [C, n_i]."""
        C1 = self.cfg["num_codebooks"] + 1
        empty = np.zeros((C1, 0), np.uint32)
        cond = empty if cond is None else _u32(cond)
        between = empty if between is None else _u32(between)
        bodies = [_u32(b) for b in bodies]
        for what, a in [("cond", cond), ("between", between)] + [(f"bodies[{i}]", b) for i, b in enumerate(bodies)]:
            if a.ndim != 2 or a.shape[0] != C1 or (what.startswith("bodies") and a.shape[1] < 1):
                raise ValueError(f"{what} must be u32 [{C1}, n], got {a.shape}")
        if int(max_new_tokens) < 1:
            raise ValueError("max_new_tokens must be >= 1")
        out = []
        with self.session(temp=temp, top_p=top_p, top_k=top_k, seed=seed, ignore_eos=ignore_eos, per_slot=True,
                          repetition_penalty=repetition_penalty) as s:
            prev, hist = None, 0  # the previous turn's slot (kept until the next one is queued) and its token history
            for i, body in enumerate(bodies):
                sd = (int(seed) + i) & (2**64 - 1)
                slot = None
                if prev is not None:
                    tail = np.concatenate([between, body], 1)
                    Lh, Lc = hist + 1 + tail.shape[1], cond.shape[1] + body.shape[1]
                    if Lh + max(0, int(max_new_tokens) - Lc + 1) <= self.cfg["max_seq_len"]:  # the frames it would have had on cond alone fit
                        slot, _ = s.continue_from(prev, tail, int(max_new_tokens) + (Lh - Lc), seed=sd)
                    s.release(prev)
                if slot is None:  # the first turn, or a history that no longer fits: the conditioning alone
                    full = np.ascontiguousarray(np.concatenate([cond, body], 1))
                    slot = s.add(full, int(max_new_tokens), seed=sd)
                    if slot is None:
                        raise RuntimeError("generate_turns: the session has no room for the turn")
                    L = full.shape[1]
                else:
                    L = hist + 1 + tail.shape[1]
                while not s.poll(slot, codes=False)[1]:
                    s.step(step_frames)
                codes, _ = s.poll(slot)
                out.append(codes)
                prev, hist = slot, L + codes.shape[1] - 1
            if prev is not None:
                s.release(prev)
        return out

    def generate_traced(self, prompts, max_new_tokens, samplings=None, seeds=None, collect_hidden=False, top_n=0):
        """Generate behind every prompts[i] (u32 [C+1, L_i]) and return, with the codes, the log-probs the model gave the tokens it picked
        -- one pass, no teacher-forced second one.  max_new_tokens: one int or one per prompt; samplings[i] (dict / SamplingArgs-like) and
        seeds[i]: the request's own settings / StdRng seed, None = the session's (temp 0.7, top_p 0.9, top_k 50, penalty 1.2; seed 42 +
        admission number).  Opens one per-slot trace session (wide when a setting needs it), admits the requests as slots free up and
        returns one dict per prompt: codes u32 [C, n_frames], the arrays of Session.poll_trace (tokens, logprob, top_logprob, top,
        eos_logprob, n_decisions), total = the sum of the log-probs of the decisions made (f64), plus hidden f32 [n, dim] with
        collect_hidden.  top_n > 0 (<= 16): an alts=top_n session, and each dict also holds Session.poll_alts' alt_index, alt_logprob
        and entropy."""
        n = len(prompts)
        budgets = [int(max_new_tokens)] * n if np.ndim(max_new_tokens) == 0 else [int(m) for m in max_new_tokens]
        samplings = [None] * n if samplings is None else list(samplings)
        seeds = [None] * n if seeds is None else list(seeds)
        if not (len(budgets) == len(samplings) == len(seeds) == n):
            raise ValueError(f"generate_traced: {n} prompts for {len(budgets)} budgets, {len(samplings)} samplings, {len(seeds)} seeds")
        alts = dict(alts=Session._alts(top_n, "top_n")) if top_n else {}

        def is_wide(sp):
            if sp is None:
                return False
            get = sp.get if isinstance(sp, dict) else (lambda k, d: getattr(sp, k, d))
            return float(get("temp", 0.7)) > 0.0 and not 0 < int(get("top_k", 50)) <= 256

        out = [None] * n
        with self.session(per_slot=True, score=True, trace=True, wide=any(is_wide(sp) for sp in samplings), **alts) as s:
            todo = [(i, s._prompt(p)) for i, p in enumerate(prompts)]  # (every shape is checked first)
            for sp in samplings:
                if sp is not None:
                    s._sampling(sp)
            live = {}
            while todo or live:
                while todo:
                    i, p = todo[0]
                    slot = s.add(p, budgets[i], sampling=samplings[i], seed=seeds[i], collect_hidden=collect_hidden, trace=True)
                    if slot is None:
                        if not live:
                            raise RuntimeError(f"generate_traced: request {i} does not fit an empty session (KV page pool too small)")
                        break
                    live[slot] = i
                    todo.pop(0)
                s.step(8)
                for slot in list(live):
                    codes, done = s.poll(slot)
                    if not done:
                        continue
                    r = s.poll_trace(slot)
                    r["codes"] = codes
                    r["total"] = float(np.nansum(r["logprob"], dtype=np.float64))
                    if alts:
                        r.update(s.poll_alts(slot))
                    if collect_hidden:
                        r["hidden"] = s.poll_hidden(slot)
                    out[live.pop(slot)] = r
                    s.release(slot)
        return out

    def score(self, prompts, frames, collect_hidden=False, top_n=0):
        """Teacher-forced log-probabilities of given code sequences: sequence i is frames[i] (u32 [C+1, N_i]: row 0 the slow tokens, rows
        1..C the codes) behind prompts[i] (u32 [C+1, L_i]).  Opens a greedy per-slot score session, feeds the sequences through the
        handle's max_batch slots -- admitting the next one as slots free up, so the weights are streamed once per step for all of them --
        and returns one dict per sequence: logprob / top_logprob f32 [N, C+1], top u32 [N, C+1], eos_logprob f32 [N]
        (Session.poll_scores), total = logprob.sum() (f64), plus hidden f32 [N, dim] with collect_hidden.  top_n > 0 (<= 16): an
        alts=top_n session, and each dict also holds Session.poll_alts' alt_index u32 / alt_logprob f32 [N, C+1, top_n] and entropy
        f32 [N, C+1]."""
        if len(prompts) != len(frames):
            raise ValueError(f"score: {len(prompts)} prompts for {len(frames)} frame arrays")
        alts = dict(alts=Session._alts(top_n, "top_n")) if top_n else {}
        out = [None] * len(prompts)
        with self.session(temp=0.0, top_p=1.0, top_k=0, seed=0, repetition_penalty=1.0, per_slot=True, score=True, **alts) as s:
            todo = [(i, s._prompt(p), s._frames(f)) for i, (p, f) in enumerate(zip(prompts, frames))]  # (every shape is checked first)
            live = {}
            while todo or live:
                while todo:
                    i, p, f = todo[0]
                    slot = s.add_scored(p, f, collect_hidden=collect_hidden)
                    if slot is None:
                        if not live:
                            raise RuntimeError(f"score: sequence {i} does not fit an empty session (KV page pool too small)")
                        break
                    live[slot] = i
                    todo.pop(0)
                s.step(8)
                for slot in [k for k in live if s.poll(k, codes=False)[1]]:
                    r = s.poll_scores(slot)
                    r["total"] = float(r["logprob"].sum(dtype=np.float64))
                    if alts:
                        r.update(s.poll_alts(slot))
                    if collect_hidden:
                        r["hidden"] = s.poll_hidden(slot)
                    out[live.pop(slot)] = r
                    s.release(slot)
        return out

    def last_stats(self):
        st = _ffi.GenStats()
        _ffi.check(_ffi.lib().fs_lm_last_stats(self._h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in _ffi.GenStats._fields_}

    def selftest(self, what="persist"):
        """fs_lm_selftest: the persistent decode kernels of this build against the per-node kernels on the loaded weights (raises on a mismatch)"""
        _ffi.check(_ffi.lib().fs_lm_selftest(self._h, what.encode()))

    def debug_capture(self, n_frames):
        """test hook: record what the 9 decisions of each of the first n_frames iterations saw and picked (persistent path only)"""
        _ffi.check(_ffi.lib().fs_lm_debug_capture(self._h, int(n_frames)))

    def debug_read(self, n_frames):
        out = np.zeros((int(n_frames), 9, 2048), np.float32)
        _ffi.check(_ffi.lib().fs_lm_debug_read(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), int(n_frames)))
        return out

    def debug_read_kv(self, layer, t0, n, slot=0):
        """test hook: cached K / V rows [t0, t0 + n) of one slow layer as f32 (n, n_local_heads, head_dim) each"""
        sh = (int(n), self.cfg["n_local_heads"], self.cfg["head_dim"])
        k, v = np.zeros(sh, np.float32), np.zeros(sh, np.float32)
        _ffi.check(_ffi.lib().fs_lm_debug_read_kv(self._h, int(slot), int(layer), int(t0), int(n), k.ctypes.data_as(C.POINTER(C.c_float)),
                                                  v.ctypes.data_as(C.POINTER(C.c_float))))
        return k, v

    def debug_read_row(self, row, n_frames):
        """the capture of request `row` of the last generate_multi call"""
        out = np.zeros((int(n_frames), 9, 2048), np.float32)
        _ffi.check(_ffi.lib().fs_lm_debug_read_row(self._h, int(row), out.ctypes.data_as(C.POINTER(C.c_float)), int(n_frames)))
        return out

    def stream(self):
        return _ffi.lib().fs_lm_stream(self._h)

    def bench_kernel(self, kind, kv_len=495, reps=50):
        """us per launch of one batch-1 decode kernel (0 qkv, 1 attention, 2 wo, 3 ffn_up, 4 ffn_down) as a graph node (measurement hook)."""
        us = C.c_float(0)
        _ffi.check(_ffi.lib().fs_lm_bench_kernel(self._h, int(kind), int(kv_len), int(reps), C.byref(us)))
        return float(us.value)


class Session:
    """Request slots over the static-batch step (no reference counterpart).  add() -> slot or None when full;
    step(n) runs up to n frames for all live slots and returns how many are still generating; poll(slot) -> (codes (C, n), done);
    release(slot) frees the slot.  A slot generates what a one-prompt generate_static_batch would (no repetition penalty)."""

    SAMPLING_KEYS = ("temp", "top_p", "top_k", "repetition_penalty")

    def __init__(self, lm, temp, top_p, top_k, seed, ignore_eos, rows=False, repetition_penalty=1.2, per_slot=False, wide=False, score=False,
                 trace=False, alts=0):
        """rows=True: FS_SESSION_ROWS -- the slots run on the request-row persistent kernels with batch-1 semantics (repetition penalty, own
        sampler stream per slot); max_batch <= 8.
        per_slot=True: FS_SESSION_PER_SLOT -- the slots stay on the static-batch step (any max_batch, bf16 / fp8) and every slot samples like
        its own generate_blocking call, with the settings and seed of its add() (default: the session's, seed + admission number).  The
        only session kind of a Fish <= 1.4 handle: its slow token is the 2-way {pad, im_end} draw, one stream word per frame even when greedy
        wide=True: FS_SESSION_WIDE_SAMPLER, per_slot sessions only -- the session's and every add()'s settings may be greedy or any
        temp > 0 with any top_k >= 0 (0 = no top-k) and any top_p; settings inside the 0 < top_k <= 256 limit give the same codes as without it
        score=True: FS_SESSION_SCORE, per_slot sessions only (Fish 1.5 token layout) -- add_scored() admits slots that are forced along a given
        code sequence and record its log-probabilities (poll_scores); generating slots of the session are unaffected
        trace=True: FS_SESSION_TRACE, per_slot + score sessions only -- add(..., trace=True) admits generating slots that leave the score
        record of the tokens they pick (poll_trace); every other slot of the session is unaffected
        alts=N (1 .. 16; 0 = off): FS_SESSION_ALTS | FS_SESSION_ALTS_N(N), per_slot + score sessions only -- every scoring and traced slot
        also records the N most likely candidates and the entropy of each of its decisions (poll_alts); codes and records are unaffected"""
        self.lm, self._open = lm, False
        alts = self._alts(alts)
        if rows and per_slot:
            raise ValueError("rows and per_slot exclude each other (a row session's slots already sample per slot)")
        if wide and not per_slot:
            raise ValueError("wide=True needs per_slot=True (FS_SESSION_WIDE_SAMPLER is valid only together with FS_SESSION_PER_SLOT)")
        if score and not per_slot:
            raise ValueError("score=True needs per_slot=True (FS_SESSION_SCORE is valid only together with FS_SESSION_PER_SLOT)")
        if trace and not (per_slot and score):
            raise ValueError("trace=True needs per_slot=True and score=True (FS_SESSION_TRACE is valid only together with "
                             "FS_SESSION_PER_SLOT | FS_SESSION_SCORE)")
        if alts and rows:
            raise ValueError("alts needs per_slot=True and score=True (FS_SESSION_ALTS is valid only together with "
                             "FS_SESSION_PER_SLOT | FS_SESSION_SCORE: not with rows=True)")
        if alts and not (per_slot and score):
            raise ValueError("alts needs per_slot=True and score=True (FS_SESSION_ALTS is valid only together with "
                             "FS_SESSION_PER_SLOT | FS_SESSION_SCORE)")
        self.rows, self.per_slot, self.wide, self.score, self.trace = bool(rows), bool(per_slot), bool(wide), bool(score), bool(trace)
        self.alts = alts
        self.sampling = dict(temp=float(temp), top_p=float(top_p), top_k=int(top_k), repetition_penalty=float(repetition_penalty))
        s = _ffi.Sampling(float(temp), float(top_p), int(top_k), float(repetition_penalty) if (rows or per_slot) else 1.0)
        flags = (_ffi.FS_GEN_IGNORE_EOS if ignore_eos else 0) | (_ffi.FS_SESSION_ROWS if rows else 0) | (_ffi.FS_SESSION_PER_SLOT if per_slot else 0)
        flags |= _ffi.FS_SESSION_WIDE_SAMPLER if wide else 0
        flags |= _ffi.FS_SESSION_SCORE if score else 0
        flags |= _ffi.FS_SESSION_TRACE if trace else 0
        flags |= (_ffi.FS_SESSION_ALTS | _ffi.FS_SESSION_ALTS_N(alts)) if alts else 0
        _ffi.check(_ffi.lib().fs_lm_session_begin(lm._h, C.byref(s), C.c_uint64(seed), flags))
        self._open = True

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        if self._open:
            self._open = False
            _ffi.check(_ffi.lib().fs_lm_session_end(self.lm._h))

    @staticmethod
    def _alts(n, what="alts"):
        """the N of an alts session: an integer in 0 .. FS_ALTS_MAX (0 = off)"""
        if isinstance(n, bool) or int(n) != n or not 0 <= int(n) <= _ffi.FS_ALTS_MAX:
            raise ValueError(f"{what} must be an integer in 0 .. {_ffi.FS_ALTS_MAX} (alternatives per decision; 0 = off), got {n!r}")
        return int(n)

    def _prompt(self, prompt, what="prompt"):
        p = _u32(prompt)
        if p.ndim != 2 or p.shape[0] != self.lm.cfg["num_codebooks"] + 1 or p.shape[1] < 1:  # the C side reads (C + 1) * L words
            raise ValueError(f"{what} must be u32 [{self.lm.cfg['num_codebooks'] + 1}, L >= 1], got {p.shape}")
        return p

    def _sampling(self, sampling):
        """dict or SamplingArgs-like (temp / top_p / top_k / repetition_penalty; missing entries: the session's) -> _ffi.Sampling"""
        if isinstance(sampling, dict):
            unknown = set(sampling) - set(self.SAMPLING_KEYS)
            if unknown:
                raise ValueError(f"unknown sampling settings {sorted(unknown)} (known: {', '.join(self.SAMPLING_KEYS)})")
            get = sampling.get
        else:
            if not any(hasattr(sampling, k) for k in self.SAMPLING_KEYS):
                raise ValueError("sampling must be a dict or an object with temp / top_p / top_k / repetition_penalty")
            get = lambda k, d: getattr(sampling, k, d)
        v = {k: get(k, self.sampling[k]) for k in self.SAMPLING_KEYS}
        if not (float(v["temp"]) >= 0.0) or int(v["top_k"]) < 0:
            raise ValueError("sampling: temp and top_k must not be negative")
        return _ffi.Sampling(float(v["temp"]), float(v["top_p"]), int(v["top_k"]), float(v["repetition_penalty"]))

    def add(self, prompt, max_new_tokens, prefix=None, sampling=None, seed=None, collect_hidden=False, trace=False):
        """prefix (an add_prefix id): `prompt` is the request's BODY -- the slot generates what add(concat(prefix prompt, body)) would,
        reading the prefix's K/V from its shared pages and prefilling the body only.
        sampling (dict or SamplingArgs-like) / seed: the slot's own sampler settings / StdRng seed (fs_lm_session_add_ex) -- per_slot and rows
        sessions only; a plain session has one lock-step sampler and refuses them.
        collect_hidden=True (fs_lm_session_add_hidden, any session kind): the slot also keeps the slow transformer's pre-norm hidden state
        of every iteration it runs -> poll_hidden(slot); its codes are those of the same add without it
        trace=True (fs_lm_session_add_traced, trace=True sessions): the slot also records the log-probs of the tokens it picks ->
        poll_trace(slot); its codes are those of the same add without it"""
        if trace and not self.trace:
            raise ValueError("add(trace=True) needs lm.session(per_slot=True, score=True, trace=True)")
        p = self._prompt(prompt, "prompt" if prefix is None else "body")
        slot = C.c_int(-1)
        if trace:
            sp = C.byref(self._sampling(sampling)) if sampling is not None else None
            if seed is not None and not 0 <= int(seed) < 2**64:
                raise ValueError("seed must fit an unsigned 64-bit integer")
            sd = C.byref(C.c_uint64(int(seed))) if seed is not None else None
            _ffi.check(_ffi.lib().fs_lm_session_add_traced(self.lm._h, -1 if prefix is None else int(prefix), p.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                           int(p.shape[1]), int(max_new_tokens), sp, sd, 1 if collect_hidden else 0, C.byref(slot)))
        elif sampling is not None or seed is not None or collect_hidden:
            if (sampling is not None or seed is not None) and not (self.rows or self.per_slot):
                raise ValueError("per-slot sampling / seed need lm.session(per_slot=True) or lm.session(rows=True)")
            sp = C.byref(self._sampling(sampling)) if sampling is not None else None
            if seed is not None and not 0 <= int(seed) < 2**64:
                raise ValueError("seed must fit an unsigned 64-bit integer")
            sd = C.byref(C.c_uint64(int(seed))) if seed is not None else None
            fn = _ffi.lib().fs_lm_session_add_hidden if collect_hidden else _ffi.lib().fs_lm_session_add_ex
            _ffi.check(fn(self.lm._h, -1 if prefix is None else int(prefix), p.ctypes.data_as(C.POINTER(C.c_uint32)),
                          int(p.shape[1]), int(max_new_tokens), sp, sd, C.byref(slot)))
        elif prefix is None:
            _ffi.check(_ffi.lib().fs_lm_session_add(self.lm._h, p.ctypes.data_as(C.POINTER(C.c_uint32)), int(p.shape[1]), int(max_new_tokens),
                                                    C.byref(slot)))
        else:
            _ffi.check(_ffi.lib().fs_lm_session_add_prefixed(self.lm._h, int(prefix), p.ctypes.data_as(C.POINTER(C.c_uint32)), int(p.shape[1]),
                                                             int(max_new_tokens), C.byref(slot)))
        return None if slot.value < 0 else int(slot.value)

    def add_prefix(self, prompt):
        """prefill a conditioning prefix (system text + voice prompt) once into pages of this session -> prefix id, or None when the KV
        page pool cannot hold it right now.  Slots admitted with add(body, ..., prefix=id) share its pages."""
        p = self._prompt(prompt, "prefix")
        pid = C.c_int(-1)
        _ffi.check(_ffi.lib().fs_lm_session_prefix_create(self.lm._h, p.ctypes.data_as(C.POINTER(C.c_uint32)), int(p.shape[1]), C.byref(pid)))
        return None if pid.value < 0 else int(pid.value)

    def release_prefix(self, prefix):
        """drop the session's reference; the pages go back once no slot uses them any more"""
        _ffi.check(_ffi.lib().fs_lm_session_prefix_release(self.lm._h, int(prefix)))

    def prefix_from_slot(self, slot, n_positions=None):
        """a prefix out of the first P cached positions of `slot` (fs_lm_session_prefix_from_slot): nothing is prefilled, the slot's full
        pages are shared and its partly filled page copied.  n_positions None: all T = L + n_frames - 1 positions the slot has (the column
        of its last emitted frame is not among them: last_frame); else 1 <= n_positions <= T.  -> (prefix id, P); (None, P) when the one
        page a cut inside a page needs is not free right now.  The slot goes on as if nothing had happened; plain and per_slot sessions."""
        if self.rows:
            raise ValueError("prefix_from_slot needs a plain or per_slot session (FS_SESSION_ROWS sessions are not supported)")
        if n_positions is not None and (isinstance(n_positions, bool) or int(n_positions) != n_positions or int(n_positions) < 1):
            raise ValueError(f"n_positions must be None (the slot's whole history) or an integer >= 1, got {n_positions!r}")
        pid, P = C.c_int(-1), C.c_int(0)
        _ffi.check(_ffi.lib().fs_lm_session_prefix_from_slot(self.lm._h, int(slot), -1 if n_positions is None else int(n_positions), C.byref(pid),
                                                              C.byref(P)))
        return (None if pid.value < 0 else int(pid.value)), int(P.value)

    def last_frame(self, slot):
        """u32 (C + 1,): the input column [slow token, c0..] of the slot's last emitted frame, as the engine would feed it next
        (fs_lm_session_last_frame); an error before the slot's first frame.  For a cut at an earlier frame take the slow token from a traced
        slot's poll_trace()["tokens"] or from the frames a scoring slot was forced along."""
        out = np.zeros(self.lm.cfg["num_codebooks"] + 1, np.uint32)
        _ffi.check(_ffi.lib().fs_lm_session_last_frame(self.lm._h, int(slot), out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    def continue_from(self, slot, body, max_new_tokens, **add_kwargs):
        """the next turn of `slot`: its whole history becomes a prefix, and a new slot is admitted on it with body = [last_frame(slot),
        body...] (body u32 [C+1, n >= 0]; what follows the slot's last frame) -> (new slot, prefix id), or (None, None) when the pool or
        the slots are short right now (nothing is kept then).  The session's reference on the prefix is dropped as soon as the add is
        queued, so its pages go when the new slot -- and the source -- are released; the id is returned for the record only.
        max_new_tokens and add_kwargs (sampling, seed, collect_hidden, trace) are add()'s: the budget counts from the new slot's whole
        prompt, history included."""
        if "prefix" in add_kwargs:
            raise ValueError("continue_from admits on the prefix it makes: no prefix argument")
        b = _u32(body)
        C1 = self.lm.cfg["num_codebooks"] + 1
        if b.ndim != 2 or b.shape[0] != C1:
            raise ValueError(f"body must be u32 [{C1}, n >= 0], got {b.shape}")
        col = self.last_frame(slot)
        pid, _ = self.prefix_from_slot(slot)
        if pid is None:
            return None, None
        try:
            new = self.add(np.concatenate([col[:, None], b], axis=1), max_new_tokens, prefix=pid, **add_kwargs)
        finally:
            self.release_prefix(pid)
        return (new, pid) if new is not None else (None, None)

    def export_prefix(self, prefix):
        """the K/V rows of a live prefix as bytes (fishrt.h: fs_lm_session_prefix_export; header: prefix_blob_info).  Waits for the
        prefix's own pass if that is still queued or in flight; changes nothing in the session."""
        n = C.c_size_t(0)
        _ffi.check(_ffi.lib().fs_lm_session_prefix_export(self.lm._h, int(prefix), None, C.c_size_t(0), C.byref(n)))
        buf = C.create_string_buffer(int(n.value))
        _ffi.check(_ffi.lib().fs_lm_session_prefix_export(self.lm._h, int(prefix), buf, C.c_size_t(n.value), C.byref(n)))
        return buf.raw[: n.value]

    def import_prefix(self, blob):
        """a prefix from a blob of export_prefix -- of this handle or of one with the same weights_fingerprint(), in any session kind --
        without a prefill pass -> prefix id, or None when the KV page pool cannot hold it right now.  A blob that does not fit the handle
        raises RuntimeError naming the header field.  Afterwards the prefix is a created one in every respect."""
        blob = bytes(blob)
        pid = C.c_int(-1)
        _ffi.check(_ffi.lib().fs_lm_session_prefix_import(self.lm._h, blob, C.c_size_t(len(blob)), C.byref(pid)))
        return None if pid.value < 0 else int(pid.value)

    INFO_KEYS = ("free_pages", "shared_pages", "live_prefixes", "prefill_passes", "tokens_prefilled", "prefix_tokens_reused",
                 "tail_pages_copied", "prefill_us")

    def info(self):
        """KV page pool and prefill counters of this session (fs_lm_session_info)"""
        out = (C.c_int64 * 8)()
        _ffi.check(_ffi.lib().fs_lm_session_info(self.lm._h, out))
        return dict(zip(self.INFO_KEYS, (int(v) for v in out)))

    def step(self, n_frames=8):
        act = C.c_int(0)
        _ffi.check(_ffi.lib().fs_lm_session_step(self.lm._h, int(n_frames), C.byref(act)))
        return int(act.value)

    def poll(self, slot, codes=True):
        n, done = C.c_size_t(0), C.c_int(0)
        _ffi.check(_ffi.lib().fs_lm_session_poll(self.lm._h, int(slot), None, C.c_size_t(0), C.byref(n), C.byref(done)))
        if not codes:
            return int(n.value), bool(done.value)
        cap = max(1, int(n.value))
        out = np.zeros((self.lm.cfg["num_codebooks"], cap), np.uint32)
        _ffi.check(_ffi.lib().fs_lm_session_poll(self.lm._h, int(slot), out.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_size_t(cap), C.byref(n),
                                                 C.byref(done)))
        return out[:, : n.value].copy(), bool(done.value)

    def poll_hidden(self, slot, first=0):
        """hidden-state rows [first, rows so far) of a slot admitted with collect_hidden=True -> f32 (n, dim).  One row per iteration the
        slot ran, the terminating <|im_end|> one included: the slot has n_frames or n_frames + 1 rows (fs_lm_session_poll_hidden)"""
        if int(first) < 0:
            raise ValueError("first must not be negative")
        n = C.c_size_t(0)
        _ffi.check(_ffi.lib().fs_lm_session_poll_hidden(self.lm._h, int(slot), C.c_size_t(0), None, C.c_size_t(0), C.byref(n)))
        rows = max(0, int(n.value) - int(first))
        out = np.zeros((max(1, rows), self.lm.cfg["dim"]), np.float32)
        if rows:
            _ffi.check(_ffi.lib().fs_lm_session_poll_hidden(self.lm._h, int(slot), C.c_size_t(int(first)), out.ctypes.data_as(C.POINTER(C.c_float)),
                                                            C.c_size_t(rows), C.byref(n)))
        return out[:rows].copy()

    def _frames(self, frames):
        f = np.asarray(frames)
        C1 = self.lm.cfg["num_codebooks"] + 1
        if f.dtype != np.uint32 or f.ndim != 2 or f.shape[0] != C1 or f.shape[1] < 1:  # the C side reads (C + 1) * N words
            raise ValueError(f"frames must be a u32 array [{C1}, N >= 1] (row 0 the slow tokens, rows 1.. the codes), got {f.dtype} {f.shape}")
        return np.ascontiguousarray(f)

    def add_scored(self, prompt, frames, prefix=None, collect_hidden=False):
        """a scoring slot (fs_lm_session_add_scored; score=True sessions): its N iterations are forced to frames[:, i] (u32 [C+1, N]) behind
        `prompt` (or behind prefix + body, as add) and scored -> poll_scores(slot).  The slot emits frames[1:] as its codes and is done after
        N iterations.  -> slot, or None when no slot / KV pages are free right now.  collect_hidden=True: also poll_hidden(slot)."""
        if not self.score:
            raise ValueError("add_scored needs lm.session(per_slot=True, score=True)")
        p = self._prompt(prompt, "prompt" if prefix is None else "body")
        f = self._frames(frames)
        slot = C.c_int(-1)
        _ffi.check(_ffi.lib().fs_lm_session_add_scored(self.lm._h, -1 if prefix is None else int(prefix), p.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                       int(p.shape[1]), f.ctypes.data_as(C.POINTER(C.c_uint32)), int(f.shape[1]),
                                                       1 if collect_hidden else 0, C.byref(slot)))
        return None if slot.value < 0 else int(slot.value)

    def poll_scores(self, slot, first=0):
        """records [first, iterations so far) of a scoring slot -> dict(logprob f32 [n, C+1], top_logprob f32 [n, C+1], top u32 [n, C+1],
        eos_logprob f32 [n]): per iteration and decision (0 the slow token, 1 + c codebook c) the log-softmax of the raw row at the forced
        token and at its maximum, the greedy pick (a candidate index for decision 0: token - (semantic_start_id - 1), 0 = <|im_end|>; the
        code otherwise), and the log-probability of <|im_end|> at the slow decision (-inf in an ignore_eos session)"""
        if int(first) < 0:
            raise ValueError("first must not be negative")
        L, C1 = _ffi.lib(), self.lm.cfg["num_codebooks"] + 1
        n = C.c_size_t(0)
        _ffi.check(L.fs_lm_session_poll_scores(self.lm._h, int(slot), C.c_size_t(0), None, None, None, None, C.c_size_t(0), C.byref(n)))
        rows = max(0, int(n.value) - int(first))
        cap = max(1, rows)
        lp, tlp = np.zeros((cap, C1), np.float32), np.zeros((cap, C1), np.float32)
        top, eos = np.zeros((cap, C1), np.uint32), np.zeros(cap, np.float32)
        if rows:
            fp = C.POINTER(C.c_float)
            _ffi.check(L.fs_lm_session_poll_scores(self.lm._h, int(slot), C.c_size_t(int(first)), lp.ctypes.data_as(fp), tlp.ctypes.data_as(fp),
                                                   top.ctypes.data_as(C.POINTER(C.c_uint32)), eos.ctypes.data_as(fp), C.c_size_t(rows), C.byref(n)))
        return dict(logprob=lp[:rows].copy(), top_logprob=tlp[:rows].copy(), top=top[:rows].copy(), eos_logprob=eos[:rows].copy())

    def poll_trace(self, slot, first=0):
        """records [first, iterations so far) of a traced slot (add(..., trace=True)) -> dict(tokens u32 [n, C+1], logprob f32 [n, C+1],
        top_logprob f32 [n, C+1], top u32 [n, C+1], eos_logprob f32 [n], n_decisions i32 [n]): poll_scores' figures, taken at the token the
        slot PICKED (tokens[:, 0] the slow token id, tokens[:, 1 + c] the code; tokens.T feeds add_scored).  One row per iteration the slot
        ran, the terminating <|im_end|> one included (n_decisions 1: its codebook entries are NaN / 0xFFFFFFFF / 0)"""
        if not self.trace:
            raise ValueError("poll_trace needs lm.session(per_slot=True, score=True, trace=True)")
        if int(first) < 0:
            raise ValueError("first must not be negative")
        L, C1 = _ffi.lib(), self.lm.cfg["num_codebooks"] + 1
        n = C.c_size_t(0)
        _ffi.check(L.fs_lm_session_poll_trace(self.lm._h, int(slot), C.c_size_t(0), None, None, None, None, None, None, C.c_size_t(0), C.byref(n)))
        rows = max(0, int(n.value) - int(first))
        cap = max(1, rows)
        tok, top = np.zeros((cap, C1), np.uint32), np.zeros((cap, C1), np.uint32)
        lp, tlp = np.zeros((cap, C1), np.float32), np.zeros((cap, C1), np.float32)
        eos, nd = np.zeros(cap, np.float32), np.zeros(cap, np.int32)
        if rows:
            fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
            _ffi.check(L.fs_lm_session_poll_trace(self.lm._h, int(slot), C.c_size_t(int(first)), tok.ctypes.data_as(up), lp.ctypes.data_as(fp),
                                                  tlp.ctypes.data_as(fp), top.ctypes.data_as(up), eos.ctypes.data_as(fp),
                                                  nd.ctypes.data_as(C.POINTER(C.c_int)), C.c_size_t(rows), C.byref(n)))
        return dict(tokens=tok[:rows].copy(), logprob=lp[:rows].copy(), top_logprob=tlp[:rows].copy(), top=top[:rows].copy(),
                    eos_logprob=eos[:rows].copy(), n_decisions=nd[:rows].copy())

    def poll_alts(self, slot, first=0):
        """alternatives [first, iterations so far) of a scoring or traced slot of an alts=N session (fs_lm_session_poll_alts) ->
        dict(alt_index u32 [n, C+1, N], alt_logprob f32 [n, C+1, N], entropy f32 [n, C+1]): per iteration and decision the N most likely
        candidates of the raw row, the most likely first (alt_index[..., 0] == top; among equal values the higher index first; padding
        0xFFFFFFFF / NaN where a decision has fewer than N candidates or was skipped), and the entropy of the decision in nats"""
        if not self.alts:
            raise ValueError("poll_alts needs lm.session(per_slot=True, score=True, alts=N)")
        if int(first) < 0:
            raise ValueError("first must not be negative")
        L, C1 = _ffi.lib(), self.lm.cfg["num_codebooks"] + 1
        n, na = C.c_size_t(0), C.c_int(0)
        _ffi.check(L.fs_lm_session_poll_alts(self.lm._h, int(slot), C.c_size_t(0), None, None, None, C.c_size_t(0), C.byref(n), C.byref(na)))
        rows, N = max(0, int(n.value) - int(first)), int(na.value) or self.alts
        cap = max(1, rows)
        idx, lp, ent = np.zeros((cap, C1, N), np.uint32), np.zeros((cap, C1, N), np.float32), np.zeros((cap, C1), np.float32)
        if rows:
            fp = C.POINTER(C.c_float)
            _ffi.check(L.fs_lm_session_poll_alts(self.lm._h, int(slot), C.c_size_t(int(first)), idx.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                 lp.ctypes.data_as(fp), ent.ctypes.data_as(fp), C.c_size_t(rows), C.byref(n), C.byref(na)))
        return dict(alt_index=idx[:rows].copy(), alt_logprob=lp[:rows].copy(), entropy=ent[:rows].copy())

    def release(self, slot):
        _ffi.check(_ffi.lib().fs_lm_session_release(self.lm._h, int(slot)))


class LM:
    """fish_speech_python `LM` (lm.rs:23-199) with token-id inputs: __call__(list of prompts (C+1, L_i) for successive
    text chunks, speaker_prompt) -> u32 (1, C, sum T).  Conditioning tokens stay cached across chunks exactly as
    lm.rs:94-135: clear cache, generate per chunk, clear_slow_caches_until(n_conditioning_tokens)."""

    def __init__(self, model_args=None, token_cfg=None, device=0, dtype="bf16"):
        self.model = DualARTransformer(model_args, token_cfg, device, dtype)

    def __call__(self, chunk_prompts, n_conditioning_tokens=0, temp=0.7, top_p=0.9, top_k=50, repetition_penalty=1.2,
                 max_new_tokens=1024, seed=0):
        self.model.clear_slow_layer_caches()
        outs = []
        for i, p in enumerate(chunk_prompts):
            outs.append(self.model.generate_blocking(p, max_new_tokens, temp, top_p, top_k, repetition_penalty, seed + i))
            self.model.clear_slow_caches_until(n_conditioning_tokens)
        self.model.clear_slow_layer_caches()
        return np.concatenate(outs, axis=1)[None]
