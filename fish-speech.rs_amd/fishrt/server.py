"""OpenAI-compatible serving shim over the fishrt hot path: the request / response surface of the reference server
(`server/src/main.rs:60-72`: POST /v1/audio/speech, POST /v1/audio/encoding, GET /v1/voices) with a request SCHEDULER in place of the
reference's global `tokio::Mutex` around the model (`server/lib/state.rs:13`, `handlers/speech.rs:26,77`).

What is mirrored (file:line in the reference):
  * `GenerateRequest` {model, voice, input, response_format, batch_size, speaker_prompt} and the voice lookup with the default-voice
    fallback / "unconditioned" (`handlers/speech.rs:238-297`); system prompt "Speak out the provided text." for Fish 1.5 (:283-289);
  * chunked generation with the conditioning prefix kept in the KV cache between the chunks of a request (`encode_sequence(.., true)`,
    `clear_slow_caches_until(n_conditioning_tokens)`, :40), the one-shot re-roll when a chunk runs into `max_new_tokens` (:41-61), codes - 1
    for Fish <= 1.4 (:63-68), opt-in internal batching over `generate_static_batch` (`batch_size`, :72-96,141-151);
  * WAV body `audio/wav` written as `audio/wav.rs:27-58` (:168-176); errors as HTTP 500 with the message string (`handlers/error.rs:17-31`);
  * `/v1/voices` -> list of names (`handlers/supported_voices.rs`), `/v1/audio/encoding` -> `.npy` of the (8, T) codes, optional `id` +
    `prompt` query registering the voice, duplicate id -> error (`handlers/encode_speech.rs:36-94`).
What is NOT: Opus / Ogg streaming (`audio/opus.rs`; out of scope) -- `response_format: "opus"` answers 501 unless the
caller supplies an encoder; audio decoding other than WAV; the text cleaner is a compact restatement (`preprocess_text`, pluggable).
Sample rates (opt-in, `AppState(device_resample=None | "linear" | "sinc", opus_rate=None)`): with `device_resample` the codec converts on
the device -- `/v1/audio/speech` takes a `sample_rate` field for its WAV and `pcm` answers (rejected with a message otherwise) and
`/v1/audio/encoding` downmixes and resamples an upload through `codec.encode(..., sample_rate=sr)` ("linear" is the reference's
`functional.rs::resample`, `speech.rs:184-216` / `encode_speech.rs:50-54`) instead of scipy on the host; with `opus_rate` (the reference:
24000) the Opus hook gets PCM at that rate, and that rate.
Speed (opt-in, `AppState(device_speed=False)`): the `speed` field of the OpenAI schema.  With the option off (the default) the field is
ignored, as it always was: normal-rate audio, no message.  With it on, `speed` must be a real number in 0.25 .. 4.0 (a JSON number, not a
string or a boolean; anything else answers 422 with a message) and every vocoded chunk is time-stretched on the device
(`codec.decode(..., speed=)`: WSOLA, the pitch stays; include/fishrt.h fs_codec_decode_speed) BEFORE it is resampled and formatted -- for the
WAV, `pcm` and Opus-hook answers alike, with and without `sample_rate` / `opus_rate`.  A request without the field makes the codec calls it
made before.
Loudness (opt-in, `AppState(device_loudness=False)`): a request field `loudness`, the level the answer is to have in LUFS (ITU-R BS.1770
integrated loudness; include/fishrt.h fs_codec_decode_loud).  It must be a real number in -40 .. -5, else 422 with a message; with the
option off the field answers 422 saying so (a level a client asked for is not dropped silently).  Integrated loudness is a property of the
whole signal, so the field goes with the WAV answers, which are whole: the request's chunks are vocoded in ONE `codec.decode(...,
loudness=)` call over their codes in order, measured, scaled (never above a sample peak of -1 dBFS), then stretched (`speed`) and
resampled / packed (`sample_rate`) on the device.  The `pcm` and Opus answers stream chunk by chunk and refuse the field with a 422 that
says why.  A request without the field makes the calls it made before.

Scheduler.  One worker thread per LM handle (= per GPU) drains a queue of chunk jobs.  A job whose conditioning prefix equals the one
sitting in the handle's KV cache skips the prefix (the reference's `assume_kv_cache`); jobs of different voices simply invalidate it
(the reference's single mutex serialises requests and would reuse a stale prefix only by construction of one request at a time).  When
several jobs are in flight (or a request asks for `batch_size`) on a `max_batch > 1` handle, they share the static-batch decode step
(the weights are streamed once per step for all rows) through CONTINUOUS batching: the handle's rows are request slots of a session
(`fs_lm_session_*`), a job joins as soon as a slot is free and leaves when it is done -- token-level admission, no lock-step batches.
A lone job takes the batch-1 path with its persistent decode kernels.  `Scheduler(continuous=False)` keeps the lock-step variant
(jobs waiting together go through one `generate_static_batch` call).

Per-request sampling (`Scheduler(per_slot_sampling=True)`, off by default).  A session that cannot take the request-row kernels is opened
with FS_SESSION_PER_SLOT instead of the lock-step sampler (on a Fish <= 1.4 `model_type` it is the only session kind the handle takes, so
this switch is what gives such a deployment continuous batching at all): every job is admitted with the server's settings (repetition penalty included)
and a sampler seed of its own, so what a job generates no longer depends on its slot or on the other jobs, and every chunk may join the
session without `batch_size`.  Requests may then carry `temperature`, `top_p`, `top_k`, `repetition_penalty` and `seed` (an extension:
the reference's `GenerateRequest` has none).  They are honoured on the batch-1 path and in per-slot / row sessions; a job that carries
any of them never enters a lock-step sampler path -- it runs alone instead -- and a job with a `seed` always runs in the session on a
`max_batch > 1` handle, alone or not, so that the same request gives the same audio whatever else the server is doing.

Wide sampling (`Scheduler(per_slot_sampling=True, wide_sampling=True)`, off by default).  Per-slot sessions are opened with
FS_SESSION_WIDE_SAMPLER as well, so a slot may sample nucleus-only (`top_k == 0`, what upstream Fish-Speech does) or with `top_k > 256`:
such a request joins the per-slot session instead of waiting for it to drain and running alone, and a server whose DEFAULT settings are
nucleus-only gets a per-slot session at all.  Handles whose sessions take the request-row kernels (2 / 4 / 8 slots, Fish 1.5) keep their
limit: a job outside it still runs alone.

Host cache of prefix blobs (`Scheduler(session_prefixes=True, prefix_host_cache_bytes=N)`, off by default).  A session prefix dies with its
session, and the session is closed at every lull, before every batch-1 job and after every error.  With a byte budget the scheduler keeps
an LRU `cond_key -> blob` of its own (`Session.export_prefix`): a prefix is exported once, when the per-session LRU evicts it or its
session is about to close -- not while the job that created it has no frame yet, and not from a session that failed -- and a voice that
misses the session's map but hits the cache is imported (`Session.import_prefix`: one copy and a scatter) instead of prefilled.  No pages
for the import falls back to the full prompt, as for a creation; a blob the handle refuses (weights reloaded) is dropped.

Chunk history (`AppState(chunk_history=True)`, off by default: it changes what a client hears; needs the continuous scheduler with
`per_slot_sampling`).  Upstream Fish-Speech keeps the earlier segments of a long text -- their text and their generated codes -- in the
context of the next one, so prosody carries over; the reference, and this shim by default, generate every chunk on the conditioning
prefix alone.  With the option the chunks of ONE request run as the turns of a conversation: chunk i + 1 is admitted when chunk i's slot
is done, on a prefix made of that slot's whole history (`Session.continue_from`: `fs_lm_session_prefix_from_slot`, nothing is prefilled
again), with the body [the last frame's column, the tokens of "<|im_end|>", encode_text("user", chunk), encode_vq(None)] -- the columns
`PromptEncoder` puts between one assistant turn and the next.  The chunk keeps the frame budget it would have had without history
(`max_new_tokens` raised by what the history adds to its prompt); when history + body + budget would not fit `max_seq_len`, or the
session has no room right now, it falls back to the conditioning prefix alone, as upstream drops old segments.  Chunks of different
requests still share the session, and responses keep their shape (a streamed chunk is sent when its turn is done, as before).

Hidden states (`generate_hidden_states`, `handlers/send_hidden_states.rs`: body {text, speaker_id, return_audio} -> a stored zip of
`hidden_states.npy`, optional `audio.wav`, `metadata.json`).  Its chunk jobs go through the same scheduler with `collect_hidden` set: in a
session the slot is admitted with `add(..., collect_hidden=True)` and read with `poll_hidden`, outside one the job calls
`generate_blocking_with_hidden`; a collecting job never enters a lock-step `generate_static_batch` (the reference's static batch returns
no hidden states) -- it runs alone instead.  The reference's router (`server/src/main.rs:60-72`) does not mount that handler; the shim
serves it as POST /v1/audio/hidden_states.
"""
import collections
import hashlib
import io
import json
import queue
import zipfile
import secrets
import threading
import time
from concurrent.futures import Future

import numpy as np

from . import prompt as fprompt
from . import wav as fwav

FISH15_SYSPROMPT = "Speak out the provided text."


class SamplingArgs:  # sampling/mod.rs:29-34; defaults of server/lib/utils/load.rs:116-125
    def __init__(self, temp=0.7, top_p=0.8, top_k=256, repetition_penalty=1.4):
        self.temp, self.top_p, self.top_k, self.repetition_penalty = temp, top_p, top_k, repetition_penalty

    def kw(self):
        return dict(temp=self.temp, top_p=self.top_p, top_k=self.top_k, repetition_penalty=self.repetition_penalty)


# ---- text/clean.rs (compact restatement: symbol map, sentence split, combine short / split long by script-independent Latin thresholds)
_SYMBOLS = {"“": '"', "”": '"', "‘": "'", "’": "'", "…": "...", "«": '"', "»": '"', "​": "", "‌": "", "‍": "", "﻿": "",
            "。": ".", "、": ", ", "！": "!", "？": "?", "「": '"', "」": '"', "『": '"', "』": '"', "・": "", "：": ",", "；": ",",
            "（": "", "）": "", "【": "", "】": ""}


def preprocess_text(text, combine=150, split=400):
    t = text.strip()
    for a, b in _SYMBOLS.items():
        t = t.replace(a, b)
    t = "".join(c for c in t if not (0x1F300 <= ord(c) <= 0x1F9FF))
    t = t.replace(" - ", "—")
    sents, cur = [], ""
    for i, ch in enumerate(t):
        cur += ch
        if ch in ".!?\n" and (i + 1 == len(t) or t[i + 1] not in ".!?") and cur.strip():  # a run of marks ("...", "?!") ends ONE sentence
            sents.append(cur.strip())
            cur = ""
    if cur.strip():
        sents.append(cur.strip())
    chunks, acc = [], ""
    for s in sents:
        while len(s) > split:  # a sentence longer than the split threshold is cut at the last space before it
            cut = s.rfind(" ", 0, split)
            cut = cut if cut > 0 else split
            (chunks.append(acc) if acc else None)
            acc = ""
            chunks.append(s[:cut].strip())
            s = s[cut:].strip()
        if acc and len(acc) + 1 + len(s) > combine:
            chunks.append(acc)
            acc = s
        else:
            acc = (acc + " " + s).strip()
    if acc:
        chunks.append(acc)
    return chunks


class LMState:  # server/lib/state.rs:12-21
    def __init__(self, lm, tokenizer, voices, default_voice, model_type=fprompt.FISH_1_5, default_sampling_args=None, max_new_tokens=1792,
                 max_batch=1, seed_source=None):
        self.lm, self.tokenizer, self.voices, self.default_voice, self.model_type = lm, tokenizer, dict(voices), default_voice, model_type
        self.default_sampling_args = default_sampling_args or SamplingArgs(repetition_penalty=1.4 if model_type == fprompt.FISH_1_5 else 1.2)
        self.max_new_tokens, self.max_batch = max_new_tokens, max_batch
        self.voices_lock = threading.Lock()
        # single_batch.rs:46: every generate call draws a fresh sampler seed (`rand::random::<u64>()`); tests pass a deterministic source
        self.seed_source = seed_source or (lambda: secrets.randbits(64))


class AppState:  # server/lib/state.rs:23-29
    def __init__(self, lm_state, codec, sample_rate=44100, opus_encoder=None, preprocess=preprocess_text, batch_window_s=0.002,
                 continuous=True, auto_batch=False, session_prefixes=False, per_slot_sampling=False, wide_sampling=False,
                 prefix_host_cache_bytes=0, chunk_history=False, device_resample=None, opus_rate=None, device_speed=False,
                 device_loudness=False):
        self.lm, self.codec, self.sample_rate, self.opus_encoder, self.preprocess = lm_state, codec, sample_rate, opus_encoder, preprocess
        # device_resample (None | "linear" | "sinc", off by default): the codec converts sample rates on the device (FireflyCodec.decode /
        # encode with sample_rate=): /v1/audio/speech takes a `sample_rate` field for WAV and `pcm` answers, and /v1/audio/encoding resamples
        # an upload with the codec ("linear" = the reference's resample, bit for bit) instead of scipy on the host.
        # opus_rate (None | Hz; the reference uses 24000, speech.rs:184-216): the opus_encoder hook gets PCM at that rate, and that rate
        # (converted in the device_resample mode, "sinc" when that is off), instead of 44.1 kHz PCM
        if device_resample not in (None, "linear", "sinc"):
            raise ValueError('device_resample must be None, "linear" or "sinc"')
        self.device_resample, self.opus_rate = device_resample, (None if opus_rate is None else int(opus_rate))
        # device_speed (off by default: the `speed` field is ignored, as ever): requests may carry `speed` (0.25 .. 4.0) and the codec
        # time-stretches every chunk on the device before it resamples and formats it (FireflyCodec.decode(speed=))
        self.device_speed = bool(device_speed)
        # device_loudness (off by default: a `loudness` field answers 422): WAV requests may carry `loudness` (LUFS, -40 .. -5) and the codec
        # measures and scales the whole answer on the device (FireflyCodec.decode(loudness=))
        self.device_loudness = bool(device_loudness)
        self.codec_lock = threading.Lock()  # a codec handle takes one call at a time (include/fishrt.h); requests vocode from their own threads
        self.auto_batch = auto_batch  # True: every chunk may join the batching session (batch sampling semantics) without `batch_size`
        # session_prefixes (off by default): session jobs share their voice's conditioning prefix (Session.add_prefix) instead of prefilling
        # it per chunk.  A prefix prefilled on its own may round differently from the full prompt and flip a near-tie, so it stays opt-in.
        # per_slot_sampling (off by default): per-request sampler semantics in sessions + request-level sampling fields (module docstring)
        # wide_sampling (off by default; needs per_slot_sampling): per-slot sessions also take nucleus-only / top_k > 256 settings
        # prefix_host_cache_bytes (0 = off; needs session_prefixes): the scheduler keeps the K/V of conditioning prefixes as host blobs
        # (Session.export_prefix) across sessions, up to this many bytes, and imports them instead of prefilling the voice again.  An imported
        # prefix carries the bits of a created one, so the caveat of session_prefixes is unchanged.
        # chunk_history (off by default; needs continuous and per_slot_sampling): the chunks of one request run as turns of one conversation,
        # each on the history of the one before (module docstring).  It changes what a client hears.
        self.chunk_history = bool(chunk_history)
        self.scheduler = Scheduler(lm_state, batch_window_s, continuous, session_prefixes=session_prefixes, per_slot_sampling=per_slot_sampling,
                                   wide_sampling=wide_sampling, prefix_host_cache_bytes=prefix_host_cache_bytes, chunk_history=chunk_history)


class _Job:
    def __init__(self, cond, body, n_cond, allow_batch, sampling=None, seed=None, collect_hidden=False):
        self.cond, self.body, self.n_cond, self.allow_batch, self.future = cond, body, n_cond, allow_batch, Future()
        self.collect_hidden = bool(collect_hidden)  # the future then resolves to (codes, hidden f32 (iterations, dim)) instead of codes
        self.sampling, self.seed = sampling, seed  # request-level SamplingArgs / sampler seed (None: the server's / a fresh one)
        self.cond_key = hashlib.sha1(cond.tobytes()).hexdigest() if cond is not None else None
        # chunk_history: the job of the request's next chunk (submitted when this one is done) and the columns that close this turn
        self.next, self.sep = None, None

    def full_prompt(self):
        return self.body if self.cond is None else np.ascontiguousarray(np.concatenate([self.cond, self.body], 1))


_STOP = object()  # Scheduler.close() sentinel


class Scheduler:
    """Replaces `state.lm.model.lock().await`: chunk jobs from all requests in one queue, one worker per handle."""

    PREFIX_LRU = 8  # conditioning prefixes kept per session (session_prefixes)

    def __init__(self, lm_state, batch_window_s=0.002, continuous=True, step_frames=8, session_prefixes=False, per_slot_sampling=False,
                 wide_sampling=False, prefix_host_cache_bytes=0, chunk_history=False):
        if chunk_history and not (continuous and per_slot_sampling):
            raise ValueError("chunk_history=True needs continuous=True and per_slot_sampling=True (a turn is a slot of a per-slot session)")
        if wide_sampling and not per_slot_sampling:
            raise ValueError("wide_sampling=True needs per_slot_sampling=True (FS_SESSION_WIDE_SAMPLER is a per-slot session flag)")
        if prefix_host_cache_bytes and not session_prefixes:
            raise ValueError("prefix_host_cache_bytes needs session_prefixes=True (it keeps the blobs of session prefixes)")
        if prefix_host_cache_bytes < 0:
            raise ValueError("prefix_host_cache_bytes must not be negative")
        self.s, self.q, self.window = lm_state, queue.Queue(), batch_window_s
        self.continuous, self.step_frames = continuous, step_frames
        self.session_prefixes = session_prefixes
        self.per_slot_sampling = per_slot_sampling
        self.wide_sampling = bool(wide_sampling)
        self.chunk_history = bool(chunk_history)
        self.sess_mode = None  # "rows" | "per_slot" | "plain" while a session is open
        self.prefixes = collections.OrderedDict()  # session_prefixes: cond_key -> prefix id of the open session (LRU order)
        # prefix_host_cache_bytes: cond_key -> blob (LRU order, bounded by the byte budget).  It belongs to the scheduler, not to a
        # session: blobs outlive every session.close().  prefix_makers: cond_key -> the job whose admission created the prefix of the
        # open session (a prefix is not exported while that job is still prefilling)
        self.host_budget = int(prefix_host_cache_bytes)
        self.host_blobs = collections.OrderedDict()
        self.prefix_makers = {}
        self.cached_key = None
        self.stats = dict(jobs=0, single=0, batched_rows=0, batches=0, prefix_hits=0, rerolls=0)
        if session_prefixes:
            self.stats.update(session_prefix_hits=0, session_prefix_tokens_saved=0)
        if self.host_budget:
            self.stats.update(session_prefix_imports=0, session_prefix_import_tokens=0, prefix_host_cache_bytes=0)
        if per_slot_sampling:
            self.stats.update(per_slot_sessions=0)
        if wide_sampling:
            self.stats.update(wide_sessions=0)
        if chunk_history:
            self.stats.update(history_turns=0, history_fallbacks=0)
        self._stop = False
        self.th = threading.Thread(target=self._run, daemon=True)
        self.th.start()

    def submit(self, cond, body, n_cond, allow_batch, sampling=None, seed=None, collect_hidden=False):
        j = _Job(cond, body, n_cond, allow_batch, sampling, seed, collect_hidden)
        self.q.put(j)
        return j.future

    def submit_turns(self, cond, bodies, n_cond, allow_batch, sep, sampling=None, seeds=None, collect_hidden=False):
        """chunk_history: the chunks of one request as a chain of jobs -> their futures.  Only the first is queued; each of the others
        is admitted when the one before it is done, on that one's history (`_turn_add`) or, failing that, like any job.  sep: the
        columns that close an assistant turn (the tokens of "<|im_end|>")."""
        jobs = [_Job(cond, b, n_cond, allow_batch, sampling, None if seeds is None else seeds[i], collect_hidden) for i, b in enumerate(bodies)]
        for a, b in zip(jobs, jobs[1:]):
            a.next, a.sep = b, sep
        if jobs:
            self.q.put(jobs[0])
        return [j.future for j in jobs]

    @staticmethod
    def _fail(j, e):
        """the job's future gets the error, and so does every later chunk of its request (nothing will ever submit them)"""
        while j is not None:
            if not j.future.done():
                j.future.set_exception(e)
            j = getattr(j, "next", None)

    def _after(self, j):
        """job j is done outside a turn hand-over: the next chunk of its request joins the queue like any job (conditioning alone)"""
        nxt = getattr(j, "next", None)
        if nxt is not None:
            j.next = None
            if self._stop:
                self._fail(nxt, RuntimeError("the scheduler is shutting down; the rest of the request was dropped"))
            else:
                self.stats["history_fallbacks"] = self.stats.get("history_fallbacks", 0) + 1
                self.q.put(nxt)

    def _turn_add(self, sess, slot, j, codes):
        """chunk_history: job j's slot is done with `codes`; admit the next chunk of its request on the slot's history -> its slot, or
        None (no next chunk / it would not fit max_seq_len / no room right now: the caller lets it fall back)"""
        nxt = getattr(j, "next", None)
        if nxt is None or self.sess_mode != "per_slot" or getattr(j, "sess_L", None) is None or not self._session_ok(nxt):
            return None
        hist = j.sess_L + int(codes.shape[1]) - 1  # the slot's history: its prompt and its frames but the last one's column
        tail = np.ascontiguousarray(np.concatenate([j.sep, nxt.body], 1))
        L_turn, L_plain = hist + 1 + tail.shape[1], (nxt.cond.shape[1] if nxt.cond is not None else 0) + nxt.body.shape[1]
        # the frames the chunk would have had on the conditioning alone must fit behind history + body
        if L_turn + max(0, self.s.max_new_tokens - L_plain + 1) > self.s.lm.cfg["max_seq_len"]:
            return None
        sa = nxt.sampling or self.s.default_sampling_args
        kw = dict(sampling=sa.kw(), seed=(nxt.seed if nxt.seed is not None else self.s.seed_source()) & (2**64 - 1))
        if nxt.collect_hidden:
            kw["collect_hidden"] = True
        new, _ = sess.continue_from(slot, tail, self.s.max_new_tokens + (L_turn - L_plain), **kw)
        if new is None:
            return None
        j.next = None
        nxt.sess_slot, nxt.sess_L = new, L_turn
        self.stats["history_turns"] = self.stats.get("history_turns", 0) + 1
        return new

    @staticmethod
    def _own(j):
        return getattr(j, "sampling", None) is not None or getattr(j, "seed", None) is not None

    def _session_ok(self, j):
        """may job j join a session?  Jobs without request-level settings: always.  With: only where a slot samples per request
        (per_slot_sampling) and with settings inside the per-slot samplers' limit -- greedy, or temp > 0 with 0 < top_k <= 256; on handles
        whose sessions take the request-row kernels (2 / 4 / 8 slots) additionally greedy like the server's default or sampled like it.
        wide_sampling: in per-slot session mode any temp >= 0 with any top_k >= 0 (the sessions carry FS_SESSION_WIDE_SAMPLER); the
        row-session handles keep the limit above."""
        if not self._own(j):
            return True
        if not self.per_slot_sampling:
            return False
        sa, d = j.sampling or self.s.default_sampling_args, self.s.default_sampling_args
        if not (sa.temp == 0 or (sa.temp > 0 and 0 < sa.top_k <= 256)):
            if not (self.wide_sampling and sa.temp >= 0 and sa.top_k >= 0):
                return False
            if self.sess_mode != "per_slot" and getattr(self.s.lm, "max_batch", 0) in (2, 4, 8) and not self._legacy_tokens():
                return False  # (a row session's slots stay inside the row kernels' samplers)
        # (a Fish <= 1.4 handle never opens a row session: its sessions are per-slot ones, whatever max_batch is)
        if (getattr(self.s.lm, "max_batch", 0) in (2, 4, 8) and self.sess_mode != "per_slot" and not self._legacy_tokens()
                and (sa.temp == 0) != (d.temp == 0)):
            return False
        return True

    def _legacy_tokens(self):
        """Fish <= 1.4 token layout (2-way slow token): of the session kinds only FS_SESSION_PER_SLOT takes such a handle (fishrt.h)"""
        return self.s.model_type != fprompt.FISH_1_5

    def close(self):
        self._stop = True
        self.q.put(_STOP)
        self.th.join(timeout=10)

    # -- worker
    def _run(self):
        if self.s.max_batch > 1 and self.continuous and hasattr(self.s.lm, "session"):
            return self._run_continuous()
        while True:
            j = self.q.get()
            if j is _STOP or self._stop:
                return
            batch = [j]
            if self.s.max_batch > 1 and j.allow_batch:  # gather what else is waiting (or arrives within the window), up to max_batch rows
                deadline = time.perf_counter() + self.window
                while len(batch) < self.s.max_batch:
                    try:
                        n = self.q.get(timeout=max(0.0, deadline - time.perf_counter()))
                    except queue.Empty:
                        break
                    if n is _STOP:
                        self.q.put(_STOP)
                        break
                    batch.append(n)  # (a job that must not be batched still shares the gather; it runs alone below)
            # (a job with request-level sampling settings never enters the lock-step sampler: it runs alone; so does a job that collects
            # hidden states -- the static batch returns none)
            runs_alone = [b for b in batch if not b.allow_batch or self._own(b) or b.collect_hidden]
            together = [b for b in batch if b.allow_batch and not self._own(b) and not b.collect_hidden]
            try:
                if len(together) >= 2:
                    self._batched(together)
                else:
                    runs_alone = together + runs_alone
                for b in runs_alone:
                    self._single(b)
            except BaseException as e:  # every waiting request gets the error (AppError -> HTTP 500)
                for b in batch:
                    if not b.future.done():
                        b.future.set_exception(e)

    def _run_continuous(self):
        """Continuous batching (fishrt.h fs_lm_session_*): the handle's max_batch rows are request slots; a chunk job joins as soon as a slot
        is free (its prompt is prefilled between two decode steps) and leaves when it samples <|im_end|> or runs out of budget -- no job waits
        for a batch to form or for the slowest row of its batch.  A lone job (nothing else live or waiting) takes the batch-1 path instead:
        persistent decode kernels, repetition penalty, conditioning-prefix reuse.  Jobs that must not be batched drain the session first."""
        lm, sess, live, held = self.s.lm, None, {}, None

        def fail_all(e):
            for jb in list(live.values()) + ([held] if held is not None else []):
                self._fail(jb, e)
            live.clear()

        stopping = False
        while True:
            try:
                # ---- intake: one job at a time is held until a slot (or the drained handle) is free for it
                if held is None and not stopping:
                    if live:
                        try:
                            held = self.q.get_nowait()
                        except queue.Empty:
                            pass
                    else:
                        if sess is not None:  # idle: give the handle back (its other entry points work between bursts)
                            self._stash_prefixes(sess)
                            sess.close()
                            sess = None
                            self.prefixes.clear()
                        held = self.q.get()
                    if held is _STOP:
                        held, stopping = None, True
                if stopping and not live:
                    if sess is not None:
                        self._stash_prefixes(sess)
                        sess.close()
                        self.prefixes.clear()
                    return
                if held is not None:
                    joins = held.allow_batch and self._session_ok(held)
                    # (per_slot_sampling: a job with a seed of its own runs in the session even when it is alone -- same kernels, same audio)
                    # (chunk_history: a job with chunks behind it runs in the session too -- its history is a slot's)
                    lone = not live and self.q.empty() and not (self.per_slot_sampling and joins and
                                                                (held.seed is not None or getattr(held, "next", None) is not None))
                    if not joins or lone:
                        if not live:  # drain first; then the batch-1 path
                            if sess is not None:
                                self._stash_prefixes(sess)
                                sess.close()
                                sess = None
                                self.prefixes.clear()
                            j, held = held, None
                            self._single(j)
                            continue
                    else:
                        if sess is None:
                            sa = self.s.default_sampling_args
                            seed = self.s.seed_source() & (2**64 - 1)
                            # handles with 2 / 4 / 8 slots and the request-row kernels: the slots keep the batch-1 semantics of _single
                            # (repetition penalty, one LogitsProcessor stream per job) while they share every decode launch (FS_SESSION_ROWS)
                            # (not on Fish <= 1.4 handles: row and plain sessions refuse them; with per_slot_sampling they get a per-slot
                            # session below -- every slot its own generate_blocking call, 2-way slow draw included)
                            rows = (getattr(lm, "max_batch", 0) in (2, 4, 8) and hasattr(lm, "rows_supported")
                                    and not (self.per_slot_sampling and self._legacy_tokens())
                                    and lm.rows_supported(lm.max_batch, **sa.kw()))
                            try:
                                sess = lm.session(temp=sa.temp, top_p=sa.top_p, top_k=sa.top_k, seed=seed, rows=True,
                                                  repetition_penalty=sa.repetition_penalty) if rows else None
                            except Exception:  # (f32 / fp8 / Fish <= 1.4 handles, or the device's persistent kernels are taken)
                                sess = None
                            if sess is not None:
                                self.stats["row_sessions"] = self.stats.get("row_sessions", 0) + 1
                                self.sess_mode = "rows"
                            elif self.per_slot_sampling:
                                try:
                                    wide = dict(wide=True) if self.wide_sampling else {}
                                    sess = lm.session(temp=sa.temp, top_p=sa.top_p, top_k=sa.top_k, seed=seed, per_slot=True,
                                                      repetition_penalty=sa.repetition_penalty, **wide)
                                except Exception:  # (no per-slot session on this handle / with these defaults: never the lock-step sampler instead)
                                    j, held = held, None
                                    self._single(j)
                                    continue
                                self.stats["per_slot_sessions"] += 1
                                if self.wide_sampling:
                                    self.stats["wide_sessions"] += 1
                                self.sess_mode = "per_slot"
                            else:
                                sess = lm.session(temp=sa.temp, top_p=sa.top_p, top_k=sa.top_k, seed=seed)
                                self.sess_mode = "plain"
                            self.cached_key = None
                            self.prefixes.clear()
                        try:
                            slot, hit = self._session_add(sess, held)
                        except BaseException as e:  # a bad request (prompt longer than max_seq_len, ...) fails ALONE: the live slots go on
                            self._fail(held, e)
                            held = None
                            continue
                        if slot is not None:
                            if hit:
                                self.stats["session_prefix_hits"] += 1
                                self.stats["session_prefix_tokens_saved"] += int(held.cond.shape[1])
                            live[slot] = held
                            held = None
                            self.stats["jobs"] += 1
                            self.stats["batched_rows"] += 1
                            self.stats["peak_live"] = max(self.stats.get("peak_live", 0), len(live))
                            continue  # admit more before stepping
                        if not live:  # nothing will ever free a slot / KV pages for it: the batch-1 path (or its error) instead of spinning
                            self._stash_prefixes(sess)
                            sess.close()
                            sess = None
                            self.prefixes.clear()
                            j, held = held, None
                            self._single(j)
                            continue
                # ---- one scheduling quantum of decode steps for every live slot
                if live:
                    sess.step(self.step_frames)
                    self.stats["batches"] += 1
                    for slot in list(live):
                        n, done = sess.poll(slot, codes=False)
                        if done:
                            codes, _ = sess.poll(slot)
                            hidden = sess.poll_hidden(slot) if live[slot].collect_hidden else None
                            failed = codes.shape[1] >= self.s.max_new_tokens
                            # chunk_history: the next chunk of the request takes this slot's history before the slot goes
                            nxt = getattr(live[slot], "next", None)
                            turn = None if failed or stopping else self._turn_add(sess, slot, live[slot], codes)
                            sess.release(slot)
                            jb = live.pop(slot)
                            jb.sess_slot = None
                            if turn is not None:  # (the old slot's pages the turn shares stay until the turn's slot is released)
                                live[turn] = nxt
                                self.stats["jobs"] += 1
                                self.stats["batched_rows"] += 1
                            try:  # (jb has left `live`: from here on fail_all no longer sees it, so its future is resolved right here)
                                if codes.shape[1] >= self.s.max_new_tokens:  # speech.rs:41-61 "Failed generation suspected. Rerolling once":
                                    self.stats["rerolls"] += 1               # the re-roll takes the batch-1 path once the session has drained
                                    jb.allow_batch, jb.reroll = False, True
                                    if stopping:  # nothing takes jobs off the queue any more: fail it instead of orphaning its future
                                        raise RuntimeError("the scheduler is shutting down; the re-roll of a failed generation was dropped")
                                    self.q.put(jb)
                                else:
                                    jb.future.set_result(self._result(jb, codes, hidden))
                                    self._after(jb)  # (chunk_history: a next chunk that could not take the history joins like any job)
                            except BaseException as e:
                                self._fail(jb, e)
            except BaseException as e:  # every in-flight request gets the error (AppError -> HTTP 500); the session is rebuilt
                fail_all(e)
                held = None
                try:
                    if sess is not None:
                        sess.close()
                except BaseException:
                    pass
                sess = None
                self.prefixes.clear()  # (no export from a session that failed: its device state is not trusted)
                self.prefix_makers.clear()

    # -- host cache of prefix blobs (prefix_host_cache_bytes)
    def _settled(self, sess, key):
        """has the prefix's own pass long finished?  Not while the job whose admission created it is still prefilling (no frame yet)"""
        jm = self.prefix_makers.get(key)
        if jm is None or jm.future.done():
            return True
        slot = getattr(jm, "sess_slot", None)
        return slot is not None and sess.poll(slot, codes=False)[0] > 0

    def _stash(self, sess, key, pid):
        """export prefix `pid` of the open session into the host cache -- at most once per voice: a voice that is cached (exported
        earlier, or imported from the cache) is not exported again"""
        if not self.host_budget or key in self.host_blobs or not self._settled(sess, key):
            return
        blob = sess.export_prefix(pid)
        if len(blob) > self.host_budget:
            return
        self.host_blobs[key] = blob
        self.stats["prefix_host_cache_bytes"] += len(blob)
        while self.stats["prefix_host_cache_bytes"] > self.host_budget:
            _, old = self.host_blobs.popitem(last=False)
            self.stats["prefix_host_cache_bytes"] -= len(old)

    def _stash_prefixes(self, sess):
        """the session is about to close: keep its prefixes (least recently used first, so that the byte budget drops those first)"""
        if self.host_budget:
            for key, pid in list(self.prefixes.items()):
                self._stash(sess, key, pid)
        self.prefix_makers.clear()

    def _import_prefix(self, sess, j):
        """the job's voice from the host cache -> prefix id, or None (not cached, no KV pages right now, or a blob this handle refuses --
        weights reloaded since: dropped)"""
        blob = self.host_blobs.get(j.cond_key) if self.host_budget else None
        if blob is None:
            return None
        self.host_blobs.move_to_end(j.cond_key)
        try:
            pid = sess.import_prefix(blob)
        except RuntimeError:
            del self.host_blobs[j.cond_key]
            self.stats["prefix_host_cache_bytes"] -= len(blob)
            return None
        if pid is not None:
            self.stats["session_prefix_imports"] += 1
            self.stats["session_prefix_import_tokens"] += int(j.cond.shape[1])
        return pid

    def _session_add(self, sess, j):
        """admit job j into the session -> (slot or None, whether it joined on an existing prefix).  session_prefixes: the job's
        conditioning prefix is prefilled once per session (LRU of PREFIX_LRU) and the job prefills its body only; a prefix the KV pool
        cannot hold falls back to the full prompt"""
        kw = {}
        if self.per_slot_sampling and self.sess_mode in ("rows", "per_slot"):  # the job's own settings and seed, else the server's and a fresh seed
            sa = j.sampling or self.s.default_sampling_args
            kw = dict(sampling=sa.kw(), seed=(j.seed if j.seed is not None else self.s.seed_source()) & (2**64 - 1))
        if j.collect_hidden:  # any session kind (fs_lm_session_add_hidden); the rows come back through poll_hidden
            kw["collect_hidden"] = True
        j.sess_L = (j.cond.shape[1] if j.cond is not None else 0) + j.body.shape[1]  # (chunk_history: the slot's prompt length)
        if not self.session_prefixes or j.cond is None or j.cond.shape[1] < 1 or j.body.shape[1] < 1:
            return sess.add(j.full_prompt(), self.s.max_new_tokens, **kw), False
        pid = self.prefixes.get(j.cond_key)
        hit = pid is not None and not getattr(j, "made_prefix", False)  # (a job retried while the slots were full created its own)
        if pid is not None:
            self.prefixes.move_to_end(j.cond_key)
        else:
            cached = self.host_budget and j.cond_key in self.host_blobs
            pid = self._import_prefix(sess, j) if cached else None
            if pid is None and cached and j.cond_key in self.host_blobs:  # (no KV pages for the import: as for a creation)
                return sess.add(j.full_prompt(), self.s.max_new_tokens, **kw), False
            if pid is None:
                pid = sess.add_prefix(j.cond)
                if pid is None:
                    return sess.add(j.full_prompt(), self.s.max_new_tokens, **kw), False
                if self.host_budget:
                    self.prefix_makers[j.cond_key] = j
            self.prefixes[j.cond_key] = pid
            j.made_prefix = True
            while len(self.prefixes) > self.PREFIX_LRU:  # (slots still on an evicted prefix keep its pages until they are released)
                key, old = self.prefixes.popitem(last=False)
                self._stash(sess, key, old)
                self.prefix_makers.pop(key, None)
                sess.release_prefix(old)
        slot = sess.add(j.body, self.s.max_new_tokens, prefix=pid, **kw)
        j.sess_slot = slot
        return slot, hit

    def _codes_out(self, codes):
        if self.s.model_type != fprompt.FISH_1_5:  # speech.rs:63-68: Fish <= 1.4 codes are shifted by one
            if (codes == 0).any():  # the reference's u32 subtraction would wrap and its codebook gather then fails: surface it the same way
                raise RuntimeError("Fish <= 1.4 generation produced code 0 (no codebook entry -1)")
            codes = codes - np.uint32(1)
        return codes

    def _result(self, j, codes, hidden):
        """what job j's future resolves to: codes, or (codes, hidden f32 (iterations, dim)) for a collecting job"""
        codes = self._codes_out(codes)
        if not j.collect_hidden:
            return codes
        hidden = np.asarray(hidden, np.float32)
        return codes, np.ascontiguousarray(hidden.reshape(hidden.shape[0], hidden.shape[-1]))

    def _single(self, j):
        try:
            lm, sa = self.s.lm, getattr(j, "sampling", None) or self.s.default_sampling_args
            hidden = None
            if j.collect_hidden:  # generate_blocking_with_hidden (speech.rs:27-48): same call, plus the hidden rows
                def gen(prompt, seed):
                    nonlocal hidden
                    codes, hidden = lm.generate_blocking_with_hidden(prompt, self.s.max_new_tokens, True, seed=seed, **sa.kw())
                    return codes
            else:
                gen = lambda prompt, seed: lm.generate_blocking(prompt, self.s.max_new_tokens, seed=seed, **sa.kw())
            own_seed = getattr(j, "seed", None)
            draw = (lambda: own_seed) if own_seed is not None else self.s.seed_source
            self.stats["jobs"] += 1
            self.stats["single"] += 1
            if j.cond_key is not None and j.cond_key == self.cached_key and lm.curr_kv_size() == j.n_cond:
                prompt = j.body  # the conditioning prefix is in the KV cache (encode_sequence(.., assume_kv_cache = true))
                self.stats["prefix_hits"] += 1
            else:
                lm.clear_slow_layer_caches()
                prompt = j.full_prompt()
            codes = gen(prompt, draw())
            lm.clear_slow_caches_until(j.n_cond)  # speech.rs:40
            self.cached_key = j.cond_key if j.cond is not None else None
            if codes.shape[1] == self.s.max_new_tokens and getattr(j, "reroll", False):  # this WAS the re-roll of a session job
                raise RuntimeError("Encoded input failed for second time. Bailing")
            if codes.shape[1] == self.s.max_new_tokens:  # speech.rs:41-61: "Failed generation suspected. Rerolling once"
                self.stats["rerolls"] += 1
                lm.clear_slow_layer_caches()
                codes2 = gen(j.full_prompt(), self.s.seed_source())
                lm.clear_slow_caches_until(j.n_cond)
                if codes2.shape[1] == self.s.max_new_tokens:
                    raise RuntimeError("Encoded input failed for second time. Bailing")
                codes = codes2
            j.future.set_result(self._result(j, codes, hidden))
            self._after(j)
        except BaseException as e:
            self.cached_key = None
            self._fail(j, e)

    def _batched(self, jobs):
        assert not any(j.collect_hidden for j in jobs), "a job that collects hidden states never joins a lock-step batch"
        lm, sa = self.s.lm, self.s.default_sampling_args
        self.stats["jobs"] += len(jobs)
        self.stats["batches"] += 1
        self.stats["batched_rows"] += len(jobs)
        kw = sa.kw()
        # (only where the C side really takes the row kernels: on any other handle / sampler setting fs_lm_generate_multi would run the jobs
        # one after the other -- N times the latency of ONE lock-step generate_static_batch, which streams the weights once per step)
        if (2 <= len(jobs) <= 8 and len(jobs) <= getattr(lm, "max_batch", 0) and hasattr(lm, "generate_multi")
                and hasattr(lm, "rows_supported") and lm.rows_supported(len(jobs), **kw)):
            # request rows (fishrt.h fs_lm_generate_multi): every job keeps the batch-1 semantics of _single -- its own repetition-penalty
            # window and sampler stream -- while one persistent launch serves all of them
            self.stats["row_batches"] = self.stats.get("row_batches", 0) + 1
            outs = lm.generate_multi([j.full_prompt() for j in jobs], self.s.max_new_tokens, seeds=[self.s.seed_source() & (2**64 - 1) for _ in jobs], **kw)
            lm.clear_slow_layer_caches()
            self.cached_key = None
            for j, o in zip(jobs, outs):
                j.future.set_result(self._codes_out(o))
            return
        kw.pop("repetition_penalty")  # the batch path's repetition penalty is a no-op in the reference (static_batch.rs:204-206)
        outs = lm.generate_static_batch([j.full_prompt() for j in jobs], self.s.max_new_tokens, **kw)
        lm.clear_slow_layer_caches()  # speech.rs:88
        self.cached_key = None
        for j, o in zip(jobs, outs):
            j.future.set_result(self._codes_out(o))


# ---- request handling (framework-free core; `make_app` wraps it in FastAPI)
class AppError(Exception):  # handlers/error.rs:17-31 -> HTTP 500 with the message
    pass


def _prompts_for_request(state, req, unconditioned=True):
    s = state.lm
    voice = req.get("voice")
    if voice == "unconditioned" and unconditioned:
        emb = None
    else:
        with s.voices_lock:
            emb = s.voices.get(voice, s.default_voice)
    chunks = state.preprocess(req.get("input", ""))
    enc = fprompt.PromptEncoder(s.tokenizer, s.lm.cfg["num_codebooks"], s.model_type)
    sysprompt = req.get("speaker_prompt") or (FISH15_SYSPROMPT if s.model_type == fprompt.FISH_1_5 else None)
    n_cond, _ = enc.encode_sequence(chunks, sysprompt, emb, True)
    sys_arr = enc.encode_text("system", sysprompt) if sysprompt is not None else None
    parts = [p for p in (sys_arr, emb) if p is not None]
    cond = np.ascontiguousarray(np.concatenate(parts, 1)) if parts else None
    assistant = enc.encode_vq(None)
    bodies = [np.ascontiguousarray(np.concatenate([enc.encode_text("user", c), assistant], 1)) for c in chunks]
    return n_cond, cond, bodies


_REQ_SAMPLING = (("temperature", "temp", float), ("top_p", "top_p", float), ("top_k", "top_k", int), ("repetition_penalty", "repetition_penalty", float))


def _request_sampling(state, req):
    """the optional request-level sampling fields (per_slot_sampling servers only; an extension, the reference's GenerateRequest has none)
    -> (SamplingArgs or None, seed or None)"""
    if not getattr(state.scheduler, "per_slot_sampling", False):
        return None, None
    sa, d = None, state.lm.default_sampling_args
    if any(req.get(k) is not None for k, _, _ in _REQ_SAMPLING):
        kw = {name: conv(req[k]) if req.get(k) is not None else getattr(d, name) for k, name, conv in _REQ_SAMPLING}
        if not (kw["temp"] >= 0.0) or kw["top_k"] < 0 or not (kw["repetition_penalty"] > 0.0):
            raise AppError("temperature and top_k must not be negative, repetition_penalty must be positive")
        sa = SamplingArgs(**kw)
    seed = req.get("seed")
    if seed is not None:
        seed = int(seed)
        if not 0 <= seed < 2**64:
            raise AppError("seed must fit an unsigned 64-bit integer")
    return sa, seed


def generate_speech(state, req):
    """POST /v1/audio/speech -> (status, content_type, body bytes | iterator of bytes)"""
    for k in ("model", "voice", "input"):
        if k not in req:
            return 422, "application/json", json.dumps({"detail": f"missing field `{k}`"}).encode()
    try:
        n_cond, cond, bodies = _prompts_for_request(state, req)
        fmt = req.get("response_format")
        if fmt == "opus":
            if state.opus_encoder is None:
                return 501, "application/json", json.dumps({"detail": "Opus / Ogg streaming is outside this shim (audio/opus.rs); use the default WAV "
                                                                      "response or response_format 'pcm'"}).encode()
        out_rate = req.get("sample_rate")
        if out_rate is not None:
            if getattr(state, "device_resample", None) is None:
                return 422, "application/json", json.dumps({"detail": "`sample_rate` needs a server started with device_resample (the codec "
                                                                      f"answers at {state.sample_rate} Hz otherwise)"}).encode()
            if fmt == "opus":
                return 422, "application/json", json.dumps({"detail": "`sample_rate` goes with the WAV and 'pcm' answers; Opus runs at the "
                                                                      "server's opus_rate"}).encode()
            if isinstance(out_rate, bool) or not isinstance(out_rate, int) or not 1000 <= out_rate <= 384000:
                return 422, "application/json", json.dumps({"detail": "`sample_rate` must be an integer number of Hz in 1000 .. 384000"}).encode()
        speed = req.get("speed") if getattr(state, "device_speed", False) else None  # (option off: the field is ignored)
        if speed is not None:
            if isinstance(speed, bool) or not isinstance(speed, (int, float)) or not 0.25 <= speed <= 4.0:  # (NaN fails the comparison)
                return 422, "application/json", json.dumps({"detail": "`speed` must be a number in 0.25 .. 4.0"}).encode()
            speed = float(speed)
        loud = req.get("loudness")
        if loud is not None:
            if not getattr(state, "device_loudness", False):
                return 422, "application/json", json.dumps({"detail": "`loudness` needs a server started with device_loudness"}).encode()
            if isinstance(loud, bool) or not isinstance(loud, (int, float)) or not -40.0 <= loud <= -5.0:  # (NaN fails the comparison)
                return 422, "application/json", json.dumps({"detail": "`loudness` must be a number of LUFS in -40 .. -5"}).encode()
            if fmt in ("pcm", "opus"):
                return 422, "application/json", json.dumps({"detail": f"`loudness` goes with the WAV answer: '{fmt}' streams chunk by chunk, and "
                                                                      "integrated loudness needs the whole signal"}).encode()
            loud = float(loud)
        # like the reference (speech.rs:72-96) chunks are batched only when the request asks for it (`batch_size` > 1): the batch paths sample
        # with BatchedLogitsProcessor semantics and no repetition penalty, so what a client hears must not depend on the server's load.
        # `auto_batch` (server option, off by default) lets every chunk join the continuous-batching session when other work is in flight.
        # With per_slot_sampling a session slot samples like the batch-1 path (own stream, repetition penalty), so every chunk may join.
        sa, seed = _request_sampling(state, req)
        per_slot = getattr(state.scheduler, "per_slot_sampling", False)
        want_batch = int(req.get("batch_size") or 1) > 1 or getattr(state, "auto_batch", False) or per_slot
        if getattr(state, "chunk_history", False) and len(bodies) > 1:  # the chunks as turns of one conversation (module docstring)
            enc = fprompt.PromptEncoder(state.lm.tokenizer, state.lm.lm.cfg["num_codebooks"], state.lm.model_type)
            seeds = None if seed is None else [(seed + i) & (2**64 - 1) for i in range(len(bodies))]
            futs = state.scheduler.submit_turns(cond, bodies, n_cond, state.lm.max_batch > 1 and want_batch, enc.tokenize_text("<|im_end|>"),
                                                sampling=sa, seeds=seeds)
        elif sa is None and seed is None:
            futs = [state.scheduler.submit(cond, b, n_cond, state.lm.max_batch > 1 and want_batch) for b in bodies]
        else:  # (chunk i of a seeded request draws from seed + i, as fishrt.lm.LM does)
            futs = [state.scheduler.submit(cond, b, n_cond, state.lm.max_batch > 1 and want_batch, sampling=sa,
                                           seed=None if seed is None else (seed + i) & (2**64 - 1)) for i, b in enumerate(bodies)]

        def pcm_chunks(**spec):  # spec: sample_rate / resample / dtype of FireflyCodec.decode (converted on the device); none = as ever
            if speed is not None:  # stretched on the device, before the conversion
                spec = dict(spec, speed=speed)
            for f in futs:
                codes = f.result()
                with state.codec_lock:
                    pcm = state.codec.decode(np.ascontiguousarray(codes[None]), **spec)[0, 0]  # (an out-of-range code is an error, as in the reference)
                yield pcm

        def pcm_whole(empty, **spec):  # `loudness`: one codec call over the request's codes in order, measured and scaled as one signal
            if speed is not None:
                spec = dict(spec, speed=speed)
            codes = [f.result() for f in futs]
            if not codes:
                return np.zeros(0, empty)
            with state.codec_lock:
                return state.codec.decode(np.ascontiguousarray(np.concatenate(codes, axis=-1)[None]), loudness=loud, **spec)[0, 0]

        s16 = dict(sample_rate=out_rate, resample=state.device_resample, dtype="s16") if out_rate is not None else None
        if fmt == "pcm":  # extension: chunked little-endian s16 PCM at the codec rate (or `sample_rate`), one HTTP chunk per text chunk
            if s16:
                return 200, "audio/pcm", (np.ascontiguousarray(p, "<i2").tobytes() for p in pcm_chunks(**s16))
            return 200, "audio/pcm", (fwav.pcm_to_i16(p).tobytes() for p in pcm_chunks())
        if fmt == "opus":
            enc = state.opus_encoder
            opus_rate = getattr(state, "opus_rate", None)
            if opus_rate is not None:
                spec = dict(sample_rate=opus_rate, resample=getattr(state, "device_resample", None) or "sinc", dtype="f32")
                return 200, "audio/ogg", (b for p in pcm_chunks(**spec) for b in enc(p, opus_rate))
            return 200, "audio/ogg", (b for p in pcm_chunks() for b in enc(p, state.sample_rate))
        if s16:
            if loud is not None:
                all_pcm = pcm_whole(np.int16, **s16)
            else:
                all_pcm = np.concatenate(list(pcm_chunks(**s16))) if futs else np.zeros(0, np.int16)
            buf = io.BytesIO()
            fwav.write_pcm_as_wav(buf, all_pcm, out_rate)
            return 200, "audio/wav", buf.getvalue()
        if loud is not None:
            all_pcm = pcm_whole(np.float32)
        else:
            all_pcm = np.concatenate(list(pcm_chunks())) if futs else np.zeros(0, np.float32)
        buf = io.BytesIO()
        fwav.write_pcm_as_wav(buf, all_pcm, state.sample_rate)
        return 200, "audio/wav", buf.getvalue()
    except BaseException as e:
        return 500, "text/plain", f"Something went wrong: {e}".encode()


HIDDEN_FRAME_RATE = 21.535  # send_hidden_states.rs:114


def generate_hidden_states(state, req):
    """POST /v1/audio/hidden_states (handlers/send_hidden_states.rs:15-126): {text, speaker_id, return_audio} -> (status, content_type, body).
    The body is a stored (uncompressed) zip: hidden_states.npy = f32 [frames, dim], the slow transformer's pre-norm hidden state of every
    generator iteration of every text chunk in order (:52-69,82-96); audio.wav when return_audio (:98-104); metadata.json =
    {frame_count, frame_rate, hidden_dim} (:106-117).  Server default sampling, default-voice fallback (:26-33)."""
    for k in ("text", "speaker_id", "return_audio"):
        if k not in req:
            return 422, "application/json", json.dumps({"detail": f"missing field `{k}`"}).encode()
    try:
        want_audio = bool(req["return_audio"])
        n_cond, cond, bodies = _prompts_for_request(state, dict(voice=req["speaker_id"], input=req["text"]), unconditioned=False)
        # chunk jobs like a speech request's: they may join a session wherever a speech chunk without `batch_size` may
        want_batch = getattr(state, "auto_batch", False) or getattr(state.scheduler, "per_slot_sampling", False)
        futs = [state.scheduler.submit(cond, b, n_cond, state.lm.max_batch > 1 and want_batch, collect_hidden=True) for b in bodies]
        hidden, pcm = [], []
        for f in futs:
            codes, hid = f.result()
            hidden.append(hid)
            if want_audio:
                with state.codec_lock:
                    pcm.append(state.codec.decode(np.ascontiguousarray(codes[None]))[0, 0])
        if not hidden:
            raise AppError("Failed to concatenate hidden states")  # (:82-83: no text chunk, nothing to concatenate)
        hs = np.ascontiguousarray(np.concatenate(hidden, 0), np.float32)
        buf = io.BytesIO()
        with zipfile.ZipFile(buf, "w", zipfile.ZIP_STORED) as z:
            npy = io.BytesIO()
            np.lib.format.write_array(npy, hs, version=(1, 0))
            z.writestr("hidden_states.npy", npy.getvalue())
            if want_audio:
                wav = io.BytesIO()
                fwav.write_pcm_as_wav(wav, np.concatenate(pcm), state.sample_rate)
                z.writestr("audio.wav", wav.getvalue())
            z.writestr("metadata.json", json.dumps({"frame_count": int(hs.shape[0]), "frame_rate": HIDDEN_FRAME_RATE, "hidden_dim": int(hs.shape[1])}))
        return 200, "application/zip", buf.getvalue()
    except BaseException as e:
        return 500, "text/plain", f"Something went wrong: {e}".encode()


def supported_voices(state):
    with state.lm.voices_lock:
        return list(state.lm.voices.keys())


def _read_wav(data):
    """RIFF/WAVE PCM16 / PCM32 / float32 -> (f32 (channels, n), sample_rate); other containers are outside the shim"""
    import struct
    if data[:4] != b"RIFF" or data[8:12] != b"WAVE":
        raise AppError("only RIFF/WAVE uploads are decoded by this shim")
    pos, fmt, pcm = 12, None, None
    while pos + 8 <= len(data):
        cid, size = data[pos:pos + 4], struct.unpack("<I", data[pos + 4:pos + 8])[0]
        body = data[pos + 8:pos + 8 + size]
        if cid == b"fmt ":
            fmt = struct.unpack("<HHIIHH", body[:16])
        elif cid == b"data":
            pcm = body
        pos += 8 + size + (size & 1)
    if fmt is None or pcm is None:
        raise AppError("malformed WAV upload")
    tag, ch, sr, _, _, bits = fmt
    if tag == 1 and bits == 16:
        a = np.frombuffer(pcm, "<i2").astype(np.float32) / 32768.0
    elif tag == 1 and bits == 32:
        a = np.frombuffer(pcm, "<i4").astype(np.float32) / 2147483648.0
    elif tag == 3 and bits == 32:
        a = np.frombuffer(pcm, "<f4").astype(np.float32)
    else:
        raise AppError(f"unsupported WAV encoding (format {tag}, {bits} bits)")
    n = a.size // ch
    return a[: n * ch].reshape(n, ch).T.copy(), sr


def encode_speaker(state, file_bytes, params):
    """POST /v1/audio/encoding (handlers/encode_speech.rs:36-94) -> (status, content_type, body)"""
    try:
        audio, sr = _read_wav(file_bytes)
        if getattr(state, "device_resample", None) is not None:
            # downmix, resample and encode on the device (fs_codec_encode_pcm): "linear" is the reference's arithmetic (encode_speech.rs:50-54)
            codes = state.codec.encode(np.ascontiguousarray(audio[None], np.float32), sample_rate=int(sr), resample=state.device_resample)[0]
        else:
            if audio.shape[0] > 1:
                audio = audio.mean(0, keepdims=True)
            if sr != state.sample_rate:
                from math import gcd
                from scipy.signal import resample_poly
                g = gcd(int(sr), int(state.sample_rate))
                audio = resample_poly(audio, state.sample_rate // g, sr // g, axis=1).astype(np.float32)
            codes = state.codec.encode(np.ascontiguousarray(audio[None], np.float32))[0]  # (8, T)
        vid, text = params.get("id"), params.get("prompt")
        if vid is not None and text is not None:
            s = state.lm
            enc = fprompt.PromptEncoder(s.tokenizer, s.lm.cfg["num_codebooks"], s.model_type)
            with s.voices_lock:
                if vid in s.voices:
                    raise AppError(f"ID already exists on server: {vid}")
                s.voices[vid] = enc.encode_conditioning_prompt(text, codes.astype(np.uint32))
        buf = io.BytesIO()
        np.save(buf, codes)
        return 200, "application/x-npy", buf.getvalue()
    except BaseException as e:
        return 500, "text/plain", f"Something went wrong: {e}".encode()


def _multipart_first_file(content_type, body):
    import email.parser
    msg = email.parser.BytesParser().parsebytes(b"Content-Type: " + content_type.encode() + b"\r\n\r\n" + body)
    if not msg.is_multipart():
        raise AppError("No file provided")
    for part in msg.get_payload():
        payload = part.get_payload(decode=True)
        if payload:
            return payload
    raise AppError("No file provided")


def make_app(state):
    """FastAPI application with the reference's three routes (server/src/main.rs:60-72) and its hidden-states handler (module docstring)."""
    from fastapi import FastAPI, Request
    from fastapi.responses import JSONResponse, Response, StreamingResponse

    app = FastAPI(title="fishrt")

    @app.post("/v1/audio/speech")
    async def speech(request: Request):
        import asyncio
        try:
            req = await request.json()
        except Exception:
            return JSONResponse({"detail": "body must be a JSON object"}, status_code=422)
        status, ctype, body = await asyncio.get_event_loop().run_in_executor(None, generate_speech, state, req)
        if isinstance(body, (bytes, bytearray)):
            return Response(content=body, status_code=status, media_type=ctype)
        return StreamingResponse(body, status_code=status, media_type=ctype)

    @app.post("/v1/audio/hidden_states")
    async def hidden_states(request: Request):
        import asyncio
        try:
            req = await request.json()
        except Exception:
            return JSONResponse({"detail": "body must be a JSON object"}, status_code=422)
        status, ctype, body = await asyncio.get_event_loop().run_in_executor(None, generate_hidden_states, state, req)
        return Response(content=body, status_code=status, media_type=ctype)

    @app.post("/v1/audio/encoding")
    async def encoding(request: Request):
        import asyncio
        body = await request.body()
        try:
            data = _multipart_first_file(request.headers.get("content-type", ""), body)
        except AppError as e:
            return Response(content=f"Something went wrong: {e}".encode(), status_code=500, media_type="text/plain")
        status, ctype, out = await asyncio.get_event_loop().run_in_executor(None, encode_speaker, state, data, dict(request.query_params))
        return Response(content=out, status_code=status, media_type=ctype)

    @app.get("/v1/voices")
    async def voices():
        return JSONResponse(supported_voices(state))

    return app
