"""Long-form streaming: overlap the Firefly vocoder with LM generation (BASELINE configs[4]).

The reference vocodes a whole utterance after generation finishes (server/lib/handlers/speech.rs:98-129; SURVEY.md §3c:
"no LM/vocoder overlap and no frame-streaming in the reference").  Every convolution of the 1.4+/1.5 codec is causal
(codec/utils/mod.rs:53-62,110-122), so the PCM of frames [a, b) depends only on codes [a - R, b) with a finite receptive
field R: chunks can be vocoded while the LM is still generating, bit-identically to one-shot decoding.

R in frames (2048 samples): conv_post 12/2048 + per HiFi-GAN stage 180 samples (k=11 branch: 2 convs x 10 taps x (1+3+5))
at 2048, 1024, 512, 256 and 32 samples/frame + conv_pre 12/4 + ConvNeXt depthwise 6/4 + 6/2  ~= 14.5 frames; HALO = 24.
"""
import queue
import threading
import time

import numpy as np

HALO = 24


def decode_chunk(codec, codes, a, b, halo=HALO):
    """PCM of frames [a, b) of `codes` (8, T): decode [a - halo, b) and keep the tail."""
    lo = max(0, a - halo)
    pcm = codec.decode(np.ascontiguousarray(codes[None, :, lo:b]))[0, 0]
    return pcm[2048 * (a - lo):]


class StreamingSynth:
    """generate_blocking + FireflyCodec.decode with the vocoder running in a worker thread on its own HIP stream.

    chunk: frames per vocoder call once the stream is under way; first_chunk: size of the first call (time to first audio).  Every call
    re-decodes `halo` frames of left context (all convolutions are causal), so larger steady-state chunks cost less: 24 / 64 = 37 % extra
    vocoder work at chunk 64, 9 % at 256.  The codes live in one preallocated (C, cap) array that the frame callback fills column by
    column (no per-chunk rebuild).  stats: frames, lm_s, vocoder_busy_s, total_s, overlap_efficiency, first_audio_s (time from the call
    to the first PCM chunk)."""

    def __init__(self, lm, codec, chunk=256, halo=HALO, first_chunk=32, inline=False, stateful=None):
        """inline: vocode a chunk inside the frame callback (the LM pauses for the 3-4 ms of a 256-frame chunk) instead of in the worker
        thread.  On ONE device the persistent decode kernels hold every CU, so a concurrent vocoder only advances one kernel per LM kernel
        boundary and both sides pay for the switching; time-slicing at chunk granularity costs the vocoder's own time and no more."""
        self.lm, self.codec, self.chunk, self.halo, self.first_chunk = lm, codec, chunk, halo, min(first_chunk, chunk)
        self.inline = inline
        # stateful: the codec carries the convolutions' left context between chunks on the device (fs_codec_stream_*): no frame is decoded
        # twice; chunks shorter than 16 frames (a stream's tail) still take the halo path.  Default: whenever the codec offers it.
        # (stateful=True: required; None: used when the codec can open a stream -- the reduced test topology and the f32 mode cannot)
        self.stateful = stateful

    def __call__(self, prompt, max_new_tokens, **gen_kw):
        Cb = self.lm.cfg["num_codebooks"]
        cap = max(1, max_new_tokens - np.asarray(prompt).shape[1] + 2) + 1
        codes = np.zeros((Cb, cap), np.uint32)
        n_frames = [0]
        q, pcm_parts, errors = queue.Queue(), [], []
        t_busy, t_first = [0.0], [None]
        t0 = time.perf_counter()

        min_frames = getattr(self.codec, "STREAM_MIN_FRAMES", 16)
        stateful = bool(self.stateful) or (self.stateful is None and hasattr(self.codec, "stream_decode"))
        if stateful:
            try:
                self.codec.stream_begin()
            except Exception:
                if self.stateful:
                    raise
                stateful = False
        # A stateful stream advances the device-side left context only through stream_decode, which needs >= min_frames frames: a NON-final
        # chunk below that would have to take the stateless halo path and the next stateful chunk would start from a stale context (wrong,
        # discontinuous PCM).  So the chunk sizes of a stateful stream are raised to min_frames; only the final tail may be shorter (it is
        # decoded with a halo from the codes, and nothing follows it).
        first_chunk = max(self.first_chunk, min_frames) if stateful else self.first_chunk
        chunk = max(self.chunk, min_frames) if stateful else self.chunk

        def vocode(a, b, final=False):
            t1 = time.perf_counter()
            if stateful and b - a >= min_frames:
                pcm_parts.append(self.codec.stream_decode(np.ascontiguousarray(codes[:, a:b])))
            else:
                assert final or not stateful, "a non-final chunk of a stateful stream below the codec's minimum chunk"
                pcm_parts.append(decode_chunk(self.codec, codes, a, b, self.halo))
            t_busy[0] += time.perf_counter() - t1
            if t_first[0] is None:
                t_first[0] = time.perf_counter() - t0

        inline_upto = [0]

        def worker():
            try:
                done_upto = 0
                while True:
                    n = q.get()
                    final = n is None
                    if final:
                        if errors:
                            return
                        n = n_frames[0]
                        done_upto = max(done_upto, inline_upto[0])
                    while True:  # vocode every complete chunk available so far (the first one is shorter)
                        step = first_chunk if done_upto == 0 else chunk
                        if done_upto + step > n:
                            break
                        vocode(done_upto, done_upto + step)
                        done_upto += step
                    if final:
                        if n > done_upto:
                            vocode(done_upto, n, final=True)  # tail
                        return
            except BaseException as e:  # surfaced by the caller after join
                errors.append(e)

        th = threading.Thread(target=worker, daemon=True)
        th.start()

        def on_frame(idx, fr):
            codes[:, idx] = fr
            n_frames[0] = idx + 1
            done = idx + 1
            if done == first_chunk or (done > first_chunk and (done - first_chunk) % chunk == 0):
                if self.inline:
                    step = first_chunk if done == first_chunk else chunk
                    try:
                        vocode(done - step, done)
                        inline_upto[0] = done
                    except BaseException as e:  # (an exception must not escape a ctypes callback: record it, stop generating)
                        errors.append(e)
                else:
                    q.put(done)
            return bool(errors)  # stop generating if the vocoder thread died

        try:
            out = self.lm.generate_blocking(prompt, max_new_tokens, on_frame=on_frame, **gen_kw)
            t_lm = time.perf_counter() - t0
        finally:
            q.put(None)  # the worker always gets its sentinel, also when generate_blocking raises
            th.join()
            if stateful:
                try:
                    self.codec.stream_end()
                except Exception:
                    pass
        if errors:
            raise errors[0]
        t_all = time.perf_counter() - t0
        assert out.shape[1] == n_frames[0] and Cb == out.shape[0] and np.array_equal(out, codes[:, : n_frames[0]])
        pcm = np.concatenate(pcm_parts) if pcm_parts else np.zeros(0, np.float32)
        self.stats = dict(stateful=stateful, frames=n_frames[0], lm_s=t_lm, vocoder_busy_s=t_busy[0], total_s=t_all, first_audio_s=t_first[0],
                          overlap_efficiency=(t_lm + t_busy[0] - t_all) / max(t_busy[0], 1e-9))
        return out, pcm


class SessionStreamer:
    """Streams the PCM of every request of a continuous-batching session (lm.Session, fs_lm_session_*) while it generates, through the
    codec's multi-stream decode (FireflyCodec.streams_*: one stateful stream per request, many streams per vocoder call).

    Every request gets its own codec stream when it is added.  After each step(k) of the session, every live request with at least
    `chunk` frames not yet vocoded (`first_chunk` for its first piece) contributes exactly that many frames to ONE streams_decode call: one
    call per distinct chunk length, T uniform within a call.  A request that has finished is flushed: its remaining frames go through
    streams_decode with n = 1 when there are >= 16 of them, else through decode_chunk's halo path; then its stream is closed and its slot
    released.  Per request, the PCM pieces concatenated are bit-identical to codec.decode of its final codes.

    The vocoder runs inline, on the thread that steps the session, between two steps: rows sessions hold every CU for their persistent
    kernels (see StreamingSynth.inline), so a vocoder in another thread would only interleave at kernel boundaries.  Keep k <= chunk: a
    request contributes one chunk per step, so frames beyond that wait for the next step.

    on_audio(tag, pcm, final) is called for every PCM piece, in order per request; step() also returns the pieces as (tag, pcm, final).
    stats[tag]: frames, first_audio_s (add() to its first PCM piece), vocoder_s (wall time of the vocoder calls that carried its audio; a
    shared call counts in full for each request in it), chunks.  calls: one record per vocoder call (quantum, kind, n, T).

    ragged=True (FireflyCodec.streams_decode_ragged): at most ONE vocoder call per step().  Every request that is due -- its first piece of
    `first_chunk` frames, a steady piece of `chunk` frames, or whatever is left of a finished request, down to one frame -- is an item of the
    same call, so the kinds "tail" and "halo" never occur (the call is recorded as kind "ragged", its T = the longest item) and `chunk` /
    `first_chunk` may be any value >= 1.  The codec runs the items of a ragged call at the stride of the longest one: a call costs about
    n x the longest item, so one long item next to many short ones (a 64-frame chunk next to 31 one-frame tails) is paid 32 x 64 frames of
    work for 95 frames of audio.  Chunk sizes near each other keep that waste small; the one-call rule holds whatever the mix."""

    def __init__(self, session, codec, chunk=64, first_chunk=32, halo=HALO, on_audio=None, clock=time.perf_counter, ragged=False,
                 sample_rate=None, resample="sinc", pcm_dtype="f32", speed=None):
        """sample_rate / pcm_dtype (ragged=True only): every request's stream is opened with that PCM spec (FireflyCodec.streams_open), so
        its pieces arrive at sample_rate Hz as f32 or int16, converted on the device by `resample` ("sinc" or "linear").  Every item carries
        its final flag: a piece holds the samples whose input exists, so pieces vary in length (the first one of a sinc stream is short),
        and a finished request with no frames left still gets a flush item, which delivers the samples held back.  Per request the pieces
        concatenated equal codec.decode(final codes, sample_rate=, resample=, dtype=), bit for bit.  stats[tag]["samples"] counts them.
        speed (ragged=True only; 0.25 .. 4.0, None = none): the default speed of every request; add(speed=) sets a request's own.  Such a
        request's stream time-stretches its PCM on the device chunk by chunk (FireflyCodec.streams_open(speed=)), before sample_rate /
        pcm_dtype apply: a piece holds the whole stretch frames whose input exists (the first pieces of a request may be empty), the
        finished request always gets its flush item, and per request the pieces concatenated equal codec.decode(final codes, speed=,
        sample_rate=, resample=, dtype=), bit for bit."""
        if speed is not None and not ragged:
            raise ValueError("speed needs ragged=True (the uniform vocoder calls return f32 at the codec rate)")
        self.speed = speed
        self.pcm_spec = None
        if sample_rate is not None or pcm_dtype != "f32":
            if not ragged:
                raise ValueError("sample_rate / pcm_dtype need ragged=True (the uniform vocoder calls return f32 at the codec rate)")
            self.pcm_spec = dict(sample_rate=sample_rate, resample=resample, dtype=pcm_dtype)
        min_frames = 1 if ragged else getattr(codec, "STREAM_MIN_FRAMES", 16)
        if chunk < min_frames or first_chunk < min_frames:
            raise ValueError(f"chunk and first_chunk must be >= {min_frames} frames (the codec's minimum streamed chunk)")
        self.session, self.codec, self.chunk, self.first_chunk, self.halo = session, codec, int(chunk), int(first_chunk), halo
        self.min_frames, self.on_audio, self.clock, self.ragged = min_frames, on_audio, clock, bool(ragged)
        self.live = {}       # slot -> request record
        self.results = {}    # tag -> final codes (C, n) of every finished request
        self.stats = {}      # tag -> per-request numbers
        self.calls = []      # (quantum, kind: "chunk" | "tail" | "halo" | "ragged", n, T)
        self.quantum = 0
        self.n_active = 0
        self._admitted = 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def add(self, prompt, max_new_tokens, tag=None, prefix=None, sampling=None, seed=None, speed=None):
        """admit a request: -> its session slot, or None when the session is full (nothing is opened then).  tag: the name its audio and
        stats are reported under (default: the admission number 0, 1, 2, ...).  prefix: a Session.add_prefix id -- `prompt` is then the
        request's body (Session.add).  sampling / seed: the request's own sampler settings / seed (Session.add; per_slot and rows sessions).  speed: the request's own speed (ragged=True only; None: the streamer's default)"""
        if speed is not None and not self.ragged:
            raise ValueError("speed needs ragged=True (the uniform vocoder calls return f32 at the codec rate)")
        if speed is None:
            speed = self.speed
        if tag is None:
            tag = self._admitted
        if tag in self.stats:
            raise ValueError(f"tag {tag!r} is already in use")
        okw = dict(self.pcm_spec) if self.pcm_spec else {}
        if speed is not None:
            okw["speed"] = speed
        sid = self.codec.streams_open(**okw)
        try:
            kw = {}
            if prefix is not None:
                kw["prefix"] = prefix
            if sampling is not None:
                kw["sampling"] = sampling
            if seed is not None:
                kw["seed"] = seed
            slot = self.session.add(prompt, max_new_tokens, **kw)
        except BaseException:
            self.codec.streams_close(sid)
            raise
        if slot is None:
            self.codec.streams_close(sid)
            return None
        self._admitted += 1
        self.live[slot] = dict(tag=tag, sid=sid, done_upto=0, t_add=self.clock(), flush=bool(self.pcm_spec) or speed is not None)
        self.stats[tag] = dict(frames=0, first_audio_s=None, vocoder_s=0.0, chunks=0, samples=0)
        return slot

    def step(self, n_frames=8):
        """one session step of up to n_frames frames, then the vocoder calls it makes due -> list of (tag, pcm, final).  self.n_active = the
        session's slots still generating afterwards"""
        self.n_active = self.session.step(n_frames)
        self.quantum += 1
        if self.ragged:
            return self._step_ragged()
        out = []
        groups, finished = {}, []
        for slot, r in self.live.items():
            n, done = self.session.poll(slot, codes=False)
            r["n"] = n
            if done:
                finished.append(slot)
                continue
            T = self.first_chunk if r["done_upto"] == 0 else self.chunk
            if n - r["done_upto"] >= T:
                groups.setdefault(T, []).append(slot)
        for T in sorted(groups):
            slots = groups[T]
            codes = np.stack([self._codes(s)[:, self.live[s]["done_upto"]:self.live[s]["done_upto"] + T] for s in slots])
            t1 = self.clock()
            pcm = self.codec.streams_decode([self.live[s]["sid"] for s in slots], codes)
            self._account([self.live[s] for s in slots], "chunk", T, self.clock() - t1)
            for i, s in enumerate(slots):
                out.append(self._deliver(self.live[s], pcm[i], T, False))
        for slot in finished:
            out.extend(self._finish(slot))
        return out

    def _step_ragged(self):
        """every due request -- first piece, steady piece, or the rest of a finished one -- in ONE streams_decode_ragged call"""
        due, finished = [], []  # due: (slot, frames, final)
        for slot, r in self.live.items():
            n, done = self.session.poll(slot, codes=False)
            r["n"] = n
            left = n - r["done_upto"]
            if done:
                finished.append(slot)
                if left > 0 or r["flush"]:  # (a spec or speed stream holds samples back until its final item: flush it even with no frames left)
                    due.append((slot, left, True))
                continue
            T = self.first_chunk if r["done_upto"] == 0 else self.chunk
            if left >= T:
                due.append((slot, T, False))
        out = []
        try:
            if due:
                chunks = []
                for slot, T, _ in due:
                    a = self.live[slot]["done_upto"]
                    chunks.append(np.ascontiguousarray(self._codes(slot)[:, a:a + T]))
                t1 = self.clock()
                if self.pcm_spec or any(self.live[s]["flush"] for s, _, _ in due):
                    pcm = self.codec.streams_decode_ragged([self.live[s]["sid"] for s, _, _ in due], chunks, final=[f for _, _, f in due])
                else:
                    pcm = self.codec.streams_decode_ragged([self.live[s]["sid"] for s, _, _ in due], chunks)
                self._account([self.live[s] for s, _, _ in due], "ragged", max(T for _, T, _ in due), self.clock() - t1)
                for (slot, T, final), p in zip(due, pcm):
                    out.append(self._deliver(self.live[slot], p, T, final))
            for slot in finished:
                r = self.live[slot]
                if r["done_upto"] == r["n"] and not any(s == slot for s, _, _ in due) and self.on_audio is not None:
                    self.on_audio(r["tag"], np.zeros(0, np.float32), True)  # nothing left: the last piece was already delivered; signal the end
                self.results[r["tag"]] = self._codes(slot)[:, :r["n"]].copy()
        finally:
            for slot in finished:
                r = self.live.pop(slot)
                self.codec.streams_close(r["sid"])
                self.session.release(slot)
        return out

    def close(self):
        """close the codec streams of requests still in flight (their slots stay with the session)"""
        for r in self.live.values():
            try:
                self.codec.streams_close(r["sid"])
            except Exception:
                pass
        self.live = {}

    # ---- internals
    def _codes(self, slot):
        r = self.live[slot]
        if r.get("codes") is None or r["codes"].shape[1] < r["n"]:
            r["codes"], _ = self.session.poll(slot)
        return r["codes"]

    def _account(self, recs, kind, T, dt):
        self.calls.append((self.quantum, kind, len(recs), T))
        for r in recs:
            self.stats[r["tag"]]["vocoder_s"] += dt

    def _deliver(self, r, pcm, T, final):
        r["done_upto"] += T
        st = self.stats[r["tag"]]
        st["frames"] = r["done_upto"]
        st["chunks"] += 1
        st["samples"] += int(np.asarray(pcm).shape[-1])
        if st["first_audio_s"] is None:
            st["first_audio_s"] = self.clock() - r["t_add"]
        if self.on_audio is not None:
            self.on_audio(r["tag"], pcm, final)
        return (r["tag"], pcm, final)

    def _finish(self, slot):
        r = self.live[slot]
        out = []
        try:
            codes = self._codes(slot)
            a, b = r["done_upto"], r["n"]
            t1 = self.clock()
            if b - a >= self.min_frames:
                pcm = self.codec.streams_decode([r["sid"]], np.ascontiguousarray(codes[None, :, a:b]))[0]
                self._account([r], "tail", b - a, self.clock() - t1)
                out.append(self._deliver(r, pcm, b - a, True))
            elif b > a:
                pcm = decode_chunk(self.codec, codes, a, b, self.halo)
                self._account([r], "halo", b - a, self.clock() - t1)
                out.append(self._deliver(r, pcm, b - a, True))
            elif self.on_audio is not None:  # nothing left: the last piece was already delivered; signal the end
                self.on_audio(r["tag"], np.zeros(0, np.float32), True)
            self.results[r["tag"]] = codes[:, :b].copy()
        finally:
            del self.live[slot]
            self.codec.streams_close(r["sid"])
            self.session.release(slot)
        return out
