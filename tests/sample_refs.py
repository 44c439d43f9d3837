"""Frame-by-frame definitions for the production sampler launches of csrc/lm_sample.hip (fs_selftest_sample_frames, include/fishrt.h).

What is defined HERE (plain Python state machines, one per generator):
  * the single sequence  (k_sample_slow / k_sample_fast;            semantics: generate/single_batch.rs)
  * the static batch     (k_sample_*_rows, k_rows_rng_words + _par; semantics: generate/static_batch.rs)
  * the session slot     (k_sample_*_slots<WIDE>; the single sequence + the freeze rule)
i.e. the repetition-penalty window and mask, the emit / freeze / `done` transitions, prev / have_prev, the pos / frame / n_out counters, the
token layout, and which word of which StdRng stream every decision takes.  What is NOT restated here: a decision itself.  Picks come from
the oracle's entry points -- orc_sampler_sample (LogitsProcessor: one persistent stream per request / slot), orc_batched_sample with
call_index (BatchedLogitsProcessor: the child stream of (call, row)) -- the stream words from orc_rng_stream, the next slow input from
gemv_refs' `embed` definition and the prep fragments from gemm_refs' `prep` definition and bound.  tests/test_sample_ref_cpu.py pins the
machines against independent code: the window against orc_reppen_*, the whole single-sequence and static-batch machines against
OracleLM.generate / generate_batch.

Every comparison with the device is EXACT (integers; floats bit for bit, compared as uint32) except the prep fragments, which are held to
the bound gemm_refs derives for k_prep's normalised row: |hi + lo - n| <= (((D / 256 + 16) / 2 + 3) u + 2^-17) |n|, n = v / rms(v) * g in
float64 (block_prep_row sums 4 fma terms per thread, a 6-step wave tree and 3 adds: fewer roundings than the k_prep chain the bound was
derived for).  The bound is not re-measured here; profiles/sample_nodes_parity.txt records the worst |err| / tol.

Stream bookkeeping (RngState::consumed): a LogitsProcessor decision takes exactly one u32 word when WeightedIndex has a positive total
and none otherwise (rand 0.8.5 WeightedIndex::new fails on an all-zero total before anything is drawn; the reference falls to index 0).
After top-k the kept probabilities are positive, so the total is zero only without top-k (top_k == 0 or >= n) and top_p <= 0, where
sample_topp zeroes every entry: such a stream never draws.  A greedy decision draws nothing; a Fish <= 1.4 slow decision always draws
one word (legacy_softmax_sample), greedy slots included, and k_sample_slow draws it on replays after termination as well.

Logit rows are crafted so that the scripted events certainly happen (module functions scripted_row / probe_row / tie_rows): a scripted
row is noise in [-1, 0) with the scripted candidate at +2 (2 / 1.5 > 0: it survives every penalty used); a probe row holds a = 1.0 and
b = 0.9 (or a = -1.0, b = -0.9 over noise in [-3, -2)): with penalty >= 1.2 the pick is b iff a is penalised (a iff penalised, for the
negative pair: the division RAISES a negative logit).  NaN logits are out of scope: neither ArgMax rule of fishrt.h defines them and no
case contains one.
"""
import ctypes as C
import functools
import types

import numpy as np

import gemm_refs
import gemv_refs

F32, F64, U32, I32 = np.float32, np.float64, np.uint32, np.int32
POISON = 0xFFFFFFFF
FAMILIES = ("single", "single_batchrow", "rows", "rows_par", "slots", "slots_wide")
# family -> the production kernels its cases launch; test_sample_ref_cpu checks the union against PRODUCTION_KERNELS
FAMILY_KERNELS = {
    "single": ("k_sample_slow", "k_sample_fast"),
    "single_batchrow": ("k_sample_slow", "k_sample_fast"),
    "rows": ("k_sample_slow_rows", "k_sample_fast_rows"),
    "rows_par": ("k_rows_rng_words", "k_sample_slow_rows_par", "k_sample_fast_rows_par"),
    "slots": ("k_sample_slow_slots<false>", "k_sample_fast_slots<false>"),
    "slots_wide": ("k_sample_slow_slots<true>", "k_sample_fast_slots<true>"),
}
PRODUCTION_KERNELS = ("k_sample_slow", "k_sample_fast", "k_sample_slow_rows", "k_sample_fast_rows", "k_rows_rng_words", "k_sample_slow_rows_par",
                      "k_sample_fast_rows_par", "k_sample_slow_slots<false>", "k_sample_slow_slots<true>", "k_sample_fast_slots<false>",
                      "k_sample_fast_slots<true>")
WINDOW = 16
ST_WORDS = 40  # SeqState as int32 words: pos, rope_off, frame, done, n_out, have_prev, step, prompt_L, cur[16], prev[16]
POS, ROPE, FRAME, DONE, NOUT, HAVE, STEP, PL, CUR, PREV = 0, 1, 2, 3, 4, 5, 6, 7, 8, 24
FISH15 = dict(im_end_id=10, pad_id=5, semantic_start_id=11, semantic_end_id=2100, has_semantic_end=1)
# generic DualAR layout: <|im_end|> not adjacent to the range and BEHIND it, so a terminating row counts as "audio" at static_batch.rs:229
GENERIC = dict(im_end_id=70, pad_id=5, semantic_start_id=4, semantic_end_id=60, has_semantic_end=1)
GENERIC_LOW = dict(im_end_id=2, pad_id=5, semantic_start_id=20, semantic_end_id=90, has_semantic_end=1)
ONE_SEM = dict(im_end_id=10, pad_id=5, semantic_start_id=11, semantic_end_id=11, has_semantic_end=1)  # sem_lo == sem_hi
LEGACY = dict(im_end_id=4, pad_id=5, semantic_start_id=5, semantic_end_id=0, has_semantic_end=0)  # Fish <= 1.4: pad_id == the semantic id


def _orc():
    from oracle import oracle as orc
    return orc


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


# ------------------------------------------------------------------------------------------------------------------ oracle entry points
class Stream:
    """one LogitsProcessor with its persistent StdRng stream (orc_sampler_*)"""

    def __init__(self, seed, temp, top_p, top_k):
        self.L = _orc().lib()
        self.h = C.c_void_p(self.L.orc_sampler_create(C.c_uint64(seed), C.c_double(float(F32(temp))), C.c_double(top_p), C.c_uint64(top_k)))

    def sample(self, row):
        row = np.ascontiguousarray(row, F32)
        return int(self.L.orc_sampler_sample(self.h, _p(row, C.c_float), C.c_uint64(row.size)))

    def __del__(self):
        if getattr(self, "h", None):
            self.L.orc_sampler_destroy(self.h)
            self.h = None


def batched_pick(seed, temp, top_p, top_k, rows, call_index):
    """BatchedLogitsProcessor::sample number call_index of a request on rows [B][n] -> picks [B]"""
    rows = np.ascontiguousarray(rows, F32)
    out = np.zeros(rows.shape[0], U32)
    _orc().lib().orc_batched_sample(C.c_uint64(seed), C.c_double(float(F32(temp))), C.c_double(top_p), C.c_uint64(top_k), _p(rows, C.c_float),
                                    rows.shape[0], rows.shape[1], int(call_index), _p(out, C.c_uint32))
    return out


def stream_words(seed, n):
    out = np.zeros(max(n, 1), U32)
    _orc().lib().orc_rng_stream(C.c_uint64(seed), int(n), _p(out, C.c_uint32), 0, None)
    return out[:n]


def stream_u64(seed, n):
    out = np.zeros(max(n, 1), np.uint64)
    _orc().lib().orc_rng_stream(C.c_uint64(seed), 0, None, int(n), _p(out, C.c_uint64))
    return out[:n]


def seed_key(seed):
    key = np.zeros(8, U32)
    _orc().lib().orc_rng_seed_key(C.c_uint64(seed), _p(key, C.c_uint32))
    return key


def child_word(master_seed, n64):
    """word 0 of the child StdRng seeded with u64 number n64 of the master stream (sampling/mod.rs:93-95)"""
    return int(stream_words(int(stream_u64(master_seed, n64 + 1)[n64]), 1)[0])


def total_key(v):
    """f32::total_cmp as a signed integer key"""
    b = np.ascontiguousarray(v, F32).view(I32).astype(np.int64)
    return np.where(b < 0, b ^ 0x7FFFFFFF, b)


def legacy_u(word):
    return F32(int(word) >> 8) * F32(1.0 / 16777216.0)


def legacy_p_pad(pad, eos):
    pad, eos = F32(pad), F32(eos)
    m = max(pad, eos)
    e_pad, e_eos = np.exp(F32(pad - m)), np.exp(F32(eos - m))
    return F32(e_pad / F32(e_pad + e_eos))


# ------------------------------------------------------------------------------------------------------------------ the window (rep_pen.rs:37-65)
class PenWindow:
    """SingleBatchedRepPenProcessor: the 16-deep deque, tokens_seen and the mask.  The reference's `entry(tok).or_insert(1)` never counts
    above 1, so the mask entry of a token is reset when ANY instance of it leaves the window -- the older of two included -- and a token
    pushed in the very call that drops its older instance ends unpenalised (`last == dropped`).  The device keeps the deque as a 17-slot
    ring: ring()/meta() give that representation (head moves down by one per push, len saturates at 16, unwritten slots hold 0)."""

    def __init__(self, vocab, amt, mut=None):
        self.mask = np.ones(vocab, F32)
        self.amt = F32(amt)
        self.ctx = []       # front = index 0
        self.seen = {}
        self.depth = {"win15": 15, "win17": 17}.get(mut, WINDOW)
        self.refcount = mut == "reset_when_none"
        self.ring_ = np.zeros(17, I32)
        self.head, self.len = 0, 0

    def push(self, tok):
        tok = int(tok)
        if self.refcount and tok in self.seen:
            self.seen[tok] += 1
        else:
            self.seen.setdefault(tok, 1)
        if self.seen[tok] == 1 or not self.refcount:
            self.mask[tok] = self.amt
        self.ctx.insert(0, tok)
        if len(self.ctx) > self.depth:
            d = self.ctx.pop()
            if d in self.seen:
                self.seen[d] -= 1
                if self.seen[d] == 0:
                    del self.seen[d]
                    self.mask[d] = F32(1.0)
        self.head = (self.head + 16) % 17
        self.ring_[self.head] = tok
        self.len = min(self.len + 1, 16)

    def apply(self, row, mut=None):
        row = np.ascontiguousarray(row, F32)
        if mut == "neg_multiply":
            return np.where(row < 0, row * self.mask, row / self.mask).astype(F32)
        return (row / self.mask).astype(F32)


# ------------------------------------------------------------------------------------------------------------------ cases
@functools.lru_cache(maxsize=None)
def tables(dim, n_cb, cb_size, tok_rows, wt):
    r = np.random.RandomState(dim * 31 + cb_size)
    mk = lambda n: (r.standard_normal((n, dim)) * 0.5).astype(F32)
    t = [mk(tok_rows), mk(n_cb * cb_size), mk(cb_size), (1.0 + 0.1 * r.standard_normal(dim)).astype(F32)]
    if wt == "bf16":
        t[:3] = [gemm_refs.bf16_rne(a) for a in t[:3]]
    return tuple(t)


class Case:
    """one hook call.  cfgs: list of dicts(temp, top_p, top_k, rep_pen, seed, ignore_eos) -- B of them for the slot families, else 1.
    logits: list over frames of (slow [B][n_slow], fast [n_cb][B][cb_size]); x: [F][B][dim]; state0: int32 [B][40]."""

    def __init__(self, name, family, cfgs, logits, B=1, n_cb=2, cb_size=64, n_slow=40, ld=None, dim=128, out_cap=64, wt="bf16", tokens=FISH15,
                 prep=False, hid=False, session=0, cap_frames=0, batch_rows=0, batch_row=0, state0=None, eps=1e-5):
        self.name, self.family, self.cfgs, self.B, self.n_cb, self.cb_size, self.n_slow = name, family, cfgs, B, n_cb, cb_size, n_slow
        self.ld = ld if ld is not None else n_slow + 3
        self.dim, self.out_cap, self.wt, self.tokens, self.prep, self.hid, self.session = dim, out_cap, wt, dict(tokens), prep, hid, session
        self.cap_frames, self.batch_rows, self.batch_row, self.eps = cap_frames, batch_rows, batch_row, eps
        self.logits = logits
        self.F = len(logits)
        self.legacy = not self.tokens["has_semantic_end"]
        self.audio_base = self.tokens["im_end_id"] if self.legacy else self.tokens["semantic_start_id"] - 1
        self.tok_rows = max(self.audio_base + n_slow, self.tokens["im_end_id"] + 1, self.tokens["pad_id"] + 1)
        self.state0 = np.zeros((B, ST_WORDS), I32) if state0 is None else np.ascontiguousarray(state0, I32)
        self.x = (np.random.RandomState(zlib_seed(name)).standard_normal((self.F, B, dim)) * 2).astype(F32)

    # token layout as SampleCfg has it
    @property
    def im_end(self):
        return self.tokens["im_end_id"]

    @property
    def sem_lo(self):
        return self.tokens["semantic_start_id"]

    @property
    def sem_hi(self):
        return self.tokens["semantic_end_id"] if self.tokens["has_semantic_end"] else self.tokens["semantic_start_id"]

    def tables(self):
        return tables(self.dim, self.n_cb, self.cb_size, self.tok_rows, self.wt)

    @property
    def slots(self):
        return self.family in ("slots", "slots_wide")

    @property
    def rows(self):
        return self.family in ("rows", "rows_par")

    @property
    def single(self):
        return self.family in ("single", "single_batchrow")

    @property
    def Lf(self):
        return (1 if self.family == "rows_par" else 0) + 1 + self.n_cb

    @property
    def R(self):
        return self.B if self.slots else (1 if self.single else 0)

    def kernels(self):
        return FAMILY_KERNELS[self.family]

    def ffi(self, plan_only=False, **over):
        """-> (fs_sample_case, keep-alive list)"""
        from fishrt import _ffi
        c = _ffi.SampleCase()
        tok, cb, fast, g = self.tables()
        sam = (_ffi.Sampling * len(self.cfgs))(*[_ffi.Sampling(float(k["temp"]), float(k["top_p"]), int(k["top_k"]), float(k.get("rep_pen", 1.0)))
                                                 for k in self.cfgs])
        seeds = np.array([k["seed"] for k in self.cfgs], np.uint64)
        ign = np.array([int(k.get("ignore_eos", 0)) for k in self.cfgs], I32)
        flat = np.concatenate([np.concatenate([np.ascontiguousarray(s, F32).reshape(-1), np.ascontiguousarray(f, F32).reshape(-1)]) for s, f in self.logits])
        keep = [sam, seeds, ign, flat, self.state0, self.x, tok, cb, fast, g]
        c.family, c.wt, c.plan_only, c.B = _ffi.SAMPLE_FAMILIES[self.family], _ffi.GEMV_WT[self.wt], int(plan_only), self.B
        c.F, c.n_cb, c.cb_size, c.n_slow, c.ld, c.dim, c.out_cap, c.tok_rows = self.F, self.n_cb, self.cb_size, self.n_slow, self.ld, self.dim, self.out_cap, self.tok_rows
        c.prep, c.hid, c.session, c.cap_frames, c.batch_rows, c.batch_row, c.n_cfg = int(self.prep), int(self.hid), self.session, self.cap_frames, self.batch_rows, self.batch_row, len(self.cfgs)
        c.eps = self.eps
        c.tokens = _ffi.TokenCfg(*[self.tokens[k] for k in ("im_end_id", "pad_id", "semantic_start_id", "semantic_end_id", "has_semantic_end")])
        c.samplings, c.seeds, c.ignore_eos, c.state0 = sam, _p(seeds, C.c_uint64), _p(ign, C.c_int32), _p(self.state0, C.c_int32)
        c.tok_emb, c.cb_emb, c.fast_emb, c.prep_g, c.x, c.logits = (_p(a, C.c_float) for a in (tok, cb, fast, g, self.x, flat))
        for k, v in over.items():
            setattr(c, k, v)
        return c, keep

    def run(self):
        """the hook on the GPU -> dict of arrays [L, ...] in the shapes of reference()"""
        from fishrt import _ffi
        c, keep = self.ffi(plan_only=True)
        o = _ffi.SampleOut()
        _ffi.check(_ffi.lib().fs_selftest_sample_frames(0, C.byref(c), C.byref(o)))
        bufs = [np.zeros(max(int(o.need[i]), 1), np.uint8) for i in range(len(_ffi.SAMPLE_OUTS))]
        for i, b in enumerate(bufs):
            o.buf[i] = b.ctypes.data if o.need[i] else None
            o.cap[i] = int(o.need[i])
        c.plan_only = 0
        _ffi.check(_ffi.lib().fs_selftest_sample_frames(0, C.byref(c), C.byref(o)))
        out = {n: bufs[i][: int(o.need[i])].view(U32) for i, n in enumerate(_ffi.SAMPLE_OUTS) if n != "PREP"}
        out["PREP"] = bufs[_ffi.SAMPLE_OUTS.index("PREP")][: int(o.need[_ffi.SAMPLE_OUTS.index("PREP")])].view(np.uint16)
        out["guard_ok"], out["L"] = bool(o.guard_ok), int(o.n_launches)
        return out


def zlib_seed(name):
    import zlib
    return zlib.crc32(name.encode()) & 0x7FFFFFFF


# ------------------------------------------------------------------------------------------------------------------ the machines
class Machine:
    """runs a case launch by launch; reference() collects the state after every launch"""

    def __init__(self, case, mut=None):
        c = self.c = case
        self.mut = mut
        B, C_, dim = c.B, c.n_cb, c.dim
        self.st = c.state0.astype(np.int64).copy()
        self.tok, self.cb, self.fast, self.g = c.tables()
        self.X = np.full((B, dim), POISON, U32)
        self.XF = np.full((B, dim), POISON, U32)
        self.codes = np.full((B, C_, c.out_cap), POISON, U32)
        self.win = [[PenWindow(c.cb_size, (1.0 if c.rows else k.get("rep_pen", 1.0)), mut) for _ in range(C_)] for k in (c.cfgs if c.slots else c.cfgs[:1])] \
            if c.R else []
        self.consumed = [0] * len(c.cfgs)
        if c.slots or c.family == "single":
            self.streams = [Stream(k["seed"], k["temp"], k["top_p"], k["top_k"]) for k in c.cfgs]
            self.words = [stream_words(k["seed"], c.F * (C_ + 1) + 4) for k in c.cfgs]
        self.ahead_at = np.full((B, 16), 0xFFFFFFFFFFFFFFFF, np.uint64)
        self.ahead_word = np.full((B, 16), POISON, U32)
        self.wtab = np.full((B, 16), POISON, U32)
        self.prep_n = np.full((32, dim), np.nan)
        self.epoch = np.zeros(2, U32)
        self.hid_rows = (int(c.state0[:, FRAME].max()) + c.F) if c.hid else 0
        self.hid = np.full((self.hid_rows, dim), POISON, U32)
        self.cap = np.full((B, c.cap_frames, 4), POISON, U32)

    # ---- pieces
    def audio_tok(self, idx):
        return self.c.audio_base + idx if idx > 0 else self.c.im_end

    def embed(self, cur):
        c = self.c
        ns = types.SimpleNamespace(op="embed", prompt=False, step=0, prompt_L=1, tokens=np.asarray(cur[: c.n_cb + 1], U32), tok=self.tok, cb=self.cb,
                                   n_cb=c.n_cb, cb_size=c.cb_size, sem_lo=c.sem_lo, sem_hi=c.sem_hi)
        return gemv_refs._embed_reference(ns, None)["Y"][0].astype(F32).view(U32)

    def prep_row(self, b):
        if not self.c.prep:
            return
        v = self.XF[b].view(F32).astype(F64)
        d = np.sqrt((v * v).sum() / self.c.dim + F64(F32(self.c.eps)))
        self.prep_n[b] = v / d * self.g.astype(F64)

    def greedy_last(self, row, stream):
        if self.mut == "first_for_last":
            k = total_key(row)
            return int(np.argmax(k))
        return stream.sample(row)  # (temp == 0: the oracle's host ArgMax)

    def batch_pick(self, rows, cfg, frame_of_row, call, B_total, row_of):
        """picks of the static-batch rule for `rows` [R][n]; row r is batch row row_of[r] of B_total at frame frame_of_row[r]"""
        c = self.c
        out = np.zeros(len(rows), np.int64)
        calls = c.n_cb + 1
        for fr in sorted(set(int(f) for f in frame_of_row)):
            sel = [r for r in range(len(rows)) if int(frame_of_row[r]) == fr]
            full = np.zeros((B_total, rows.shape[1]), F32)
            for r in sel:
                full[row_of[r]] = rows[r]
            ci = fr * calls + call
            if self.mut == "child_swap":    # B and calls swapped in the child index
                ci = None
            if self.mut == "fast_call_off" and call > 0:
                ci = fr * calls + call - 1
            if F32(cfg["temp"]) <= F32(1e-7) and self.mut == "last_for_first":
                for r in sel:
                    k = rows[r]
                    out[r] = len(k) - 1 - int(np.argmax(k[::-1]))
                continue
            if ci is None:  # child of master u64 number (frame * B + row) * calls + call: call index n64 of a one-row batch
                for r in sel:
                    n64 = (fr * B_total + row_of[r]) * calls + call
                    out[r] = batched_pick(cfg["seed"], cfg["temp"], cfg["top_p"], cfg["top_k"], rows[r][None], n64)[0]
                continue
            got = batched_pick(cfg["seed"], cfg["temp"], cfg["top_p"], cfg["top_k"], full, ci)
            for r in sel:
                out[r] = got[row_of[r]]
        return out

    def draws(self, cfg, n):
        """does a sampled LogitsProcessor decision over n candidates take a stream word? (module docstring)"""
        no_topk = cfg["top_k"] == 0 or cfg["top_k"] >= n
        drew = not (no_topk and F32(cfg["top_p"]) <= 0)
        return True if self.mut == "count_nodraw" else drew

    def emit(self, b, cur):
        st, c = self.st[b], self.c
        o = int(st[NOUT])
        if o < c.out_cap:
            self.codes[b, :, o] = cur[1: c.n_cb + 1]
        elif self.mut == "past_cap":  # no capacity check: column o of [n_cb][out_cap] rows spills into what lies behind them
            flat = self.codes.reshape(-1)
            for cc in range(c.n_cb):
                at = (b * c.n_cb + cc) * c.out_cap + o
                if at < flat.size:
                    flat[at] = cur[1 + cc]
        st[NOUT] = o + 1

    # ---- single sequence
    def single_slow(self, f):
        c, st, cfg = self.c, self.st[0], self.c.cfgs[0]
        lg = np.array(c.logits[f][0][0], F32)
        self.XF[0] = c.x[f, 0].view(U32)
        if c.hid and st[DONE] == 0:
            self.hid[int(st[FRAME])] = c.x[f, 0].view(U32)
        if c.family == "single_batchrow":
            if cfg.get("ignore_eos"):
                lg[0] = -np.inf
            idx = int(self.batch_pick(lg[None], cfg, [st[FRAME]], 0, c.batch_rows, [c.batch_row])[0])
        elif c.legacy:
            w = self.words[0][self.consumed[0]]
            self.consumed[0] += 1
            if F32(cfg["temp"]) != 0:
                self.streams[0].sample(np.zeros(2, F32))  # (the oracle stream moves on by the same word)
            is_pad = bool(legacy_u(w) < legacy_p_pad(lg[0], lg[1])) or bool(cfg.get("ignore_eos"))
            tok = c.tokens["pad_id"] if is_pad else c.im_end
            idx = None
        else:
            if cfg.get("ignore_eos"):
                lg[0] = -np.inf
            if F32(cfg["temp"]) == 0:
                idx = self.greedy_last(lg, self.streams[0])
            else:
                idx = self.streams[0].sample(lg)
                self.consumed[0] += int(self.draws(cfg, len(lg)))
        if idx is not None:
            tok = self.audio_tok(idx)
        if st[DONE]:
            tok = c.im_end
        st[CUR] = tok
        if tok == c.im_end and st[DONE] == 0:
            st[DONE] = 1

    def single_fast(self, f, cb):
        c, st, cfg = self.c, self.st[0], self.c.cfgs[0]
        eos = st[CUR] == c.im_end
        code = 0
        bm = c.family == "single_batchrow"
        if not eos:
            lg = np.array(c.logits[f][1][cb][0], F32)
            if st[HAVE] and self.mut != "no_have_prev":
                w = self.win[0][cb]
                w.push(st[PREV + cb + 1])
                lg = w.apply(lg, self.mut)
            if bm:
                code = int(self.batch_pick(lg[None], cfg, [st[FRAME]], 1 + cb, c.batch_rows, [c.batch_row])[0])
            elif F32(cfg["temp"]) == 0:
                code = self.greedy_last(lg, self.streams[0])
            else:
                code = self.streams[0].sample(lg)
                self.consumed[0] += int(self.draws(cfg, len(lg)))
        st[CUR + cb + 1] = code
        if cb != c.n_cb - 1:
            if not eos:
                self.XF[0] = self.fast[code].view(U32)
            return
        cur = st[CUR: CUR + c.n_cb + 1].copy()
        if st[DONE] != 2:
            frame = int(st[FRAME])
            if st[DONE] == 1 and self.mut != "done_never_2":
                st[DONE] = 2
            emit = frame == 0 or cur[0] != c.im_end
            if self.mut == "no_frame0_emit":
                emit = cur[0] != c.im_end
            if self.mut == "emit_terminating":
                emit = True
            if emit:
                self.emit(0, cur)
            st[PREV: PREV + c.n_cb + 1] = cur
            st[HAVE] = 1
            st[POS] += 1
            st[FRAME] = frame + 1
        self.X[0] = self.embed(cur)

    # ---- the end of a frame of the row families and the slots (rows_frame_commit)
    def commit(self, b, code, take_code, freeze):
        c, st = self.c, self.st[b]
        cur = st[CUR: CUR + c.n_cb + 1].copy()
        if take_code:
            cur[c.n_cb] = code
        if cur[0] < c.sem_lo and self.mut != "keep_nonaudio_codes":
            cur[1:] = 0
        frame = int(st[FRAME])
        frozen = freeze and st[DONE] != 0 and frame > 0
        if self.mut == "frozen_advances":
            frozen = False
        if not frozen:
            emit = frame == 0 or not st[DONE]
            if self.mut == "no_frame0_emit":
                emit = not st[DONE]
            if self.mut == "emit_terminating":
                emit = True
            if emit:
                if frame == 0 and cur[0] < c.sem_lo:
                    st[STEP] = -1
                self.emit(b, cur)
            st[PREV: PREV + c.n_cb + 1] = cur
            st[CUR: CUR + c.n_cb + 1] = cur
            st[HAVE] = 1
            st[POS] += 1
            st[FRAME] = frame + 1
        self.X[b] = self.embed(cur)

    # ---- static batch
    def rows_words(self, f):
        c, cfg = self.c, self.c.cfgs[0]
        calls = c.n_cb + 1
        for b in range(c.B):
            for k in range(calls):
                n64 = (int(self.st[b][FRAME]) * calls + k) * c.B + b
                if self.mut == "child_swap":
                    n64 = (int(self.st[b][FRAME]) * c.B + b) * calls + k
                if self.mut == "fast_call_off" and k > 0:
                    n64 = (int(self.st[b][FRAME]) * calls + k - 1) * c.B + b
                self.wtab[b, k] = child_word(cfg["seed"], n64)

    def rows_slow(self, f):
        c, cfg = self.c, self.c.cfgs[0]
        lg = np.array(c.logits[f][0], F32)
        self.XF[:] = c.x[f].view(U32)
        if cfg.get("ignore_eos"):
            lg[:, 0] = -np.inf
        idx = self.batch_pick(lg, cfg, self.st[:, FRAME], 0, c.B, list(range(c.B)))
        for b in range(c.B):
            tok = self.audio_tok(int(idx[b]))
            self.st[b][CUR] = tok
            if tok == c.im_end:
                self.st[b][DONE] = 1
            self.prep_row(b)
        if c.prep:
            self.epoch[0] += 1

    def rows_fast(self, f, cb):
        c, cfg = self.c, self.c.cfgs[0]
        lg = np.array(c.logits[f][1][cb], F32)
        code = self.batch_pick(lg, cfg, self.st[:, FRAME], 1 + cb, c.B, list(range(c.B)))
        for b in range(c.B):
            self.st[b][CUR + cb + 1] = code[b]
            if cb != c.n_cb - 1:
                self.XF[b] = self.fast[int(code[b])].view(U32)
                self.prep_row(b)
            else:
                self.commit(b, int(code[b]), True, bool(c.session))

    # ---- session slots
    def look_ahead(self, b, decision, used=1):
        at = self.consumed[b] + used
        self.ahead_at[b, decision] = at
        self.ahead_word[b, decision] = self.words[b][at]

    def slots_slow(self, f):
        c = self.c
        self.XF[:] = c.x[f].view(U32)
        for b in range(c.B):
            st, cfg = self.st[b], c.cfgs[b]
            live = st[DONE] == 0
            temp = F32(cfg["temp"])
            lg = np.array(c.logits[f][0][b], F32)
            if live and temp != 0:
                self.look_ahead(b, 1)
            if live and c.legacy:
                w = self.words[b][self.consumed[b]]
                self.consumed[b] += 1
                if temp != 0:
                    self.streams[b].sample(np.zeros(2, F32))
                u = legacy_u(w)
                is_pad = bool(u < legacy_p_pad(lg[0], lg[1])) or bool(cfg.get("ignore_eos"))
                tok = c.tokens["pad_id"] if is_pad else c.im_end
                st[CUR] = tok
                if tok == c.im_end:
                    st[DONE] = 1
                if c.cap_frames and st[FRAME] < c.cap_frames:
                    self.cap[b, int(st[FRAME])] = np.array([lg[0], lg[1], u, 0.0 if is_pad else 1.0], F32).view(U32)
            elif live:
                if cfg.get("ignore_eos"):
                    lg[0] = -np.inf
                if temp == 0:
                    idx = self.greedy_last(lg, self.streams[b])
                else:
                    idx = self.streams[b].sample(lg)
                    self.consumed[b] += int(self.draws(cfg, len(lg)))
                tok = self.audio_tok(idx)
                st[CUR] = tok
                if tok == c.im_end:
                    st[DONE] = 1
            self.prep_row(b)
        if c.prep:
            self.epoch[0] += 1

    def slots_fast(self, f, cb):
        c = self.c
        last = cb == c.n_cb - 1
        for b in range(c.B):
            st, cfg = self.st[b], c.cfgs[b]
            live = st[DONE] == 0
            temp = F32(cfg["temp"])
            if live and temp != 0:
                self.look_ahead(b, 0 if last else cb + 2)
            elif live and last and c.legacy:
                self.look_ahead(b, 0, 0)
            code = 0
            if live:
                lg = np.array(c.logits[f][1][cb][b], F32)
                if st[HAVE] and self.mut != "no_have_prev":
                    w = self.win[b][cb]
                    w.push(st[PREV + cb + 1])
                    lg = w.apply(lg, self.mut)
                if temp == 0:
                    code = self.greedy_last(lg, self.streams[b])
                else:
                    code = self.streams[b].sample(lg)
                    self.consumed[b] += int(self.draws(cfg, len(lg)))
                st[CUR + cb + 1] = code
            if not last:
                self.XF[b] = self.fast[code].view(U32)
                self.prep_row(b)
            else:
                self.commit(b, code, bool(live), True)

    # ---- the trace
    def snapshot(self):
        c = self.c
        s = {"STATES": self.st.astype(I32).view(U32).copy(), "XF": self.XF.copy(), "X": self.X.copy(), "CODES": self.codes.copy()}
        if c.R:
            s["RING"] = np.stack([np.stack([w.ring_ for w in row]) for row in self.win]).view(U32).copy()
            s["META"] = np.array([[[w.head, w.len] for w in row] for row in self.win], I32).view(U32)
            s["MASK"] = np.stack([np.stack([w.mask for w in row]) for row in self.win]).view(U32).copy()
        if c.slots:
            r = np.zeros((c.B, 58), U32)
            for b in range(c.B):
                r[b, :8] = seed_key(c.cfgs[b]["seed"])
                r[b, 8], r[b, 9] = self.consumed[b] & 0xFFFFFFFF, self.consumed[b] >> 32
                r[b, 10:42] = self.ahead_at[b].view(U32)
                r[b, 42:58] = self.ahead_word[b]
            s["RNG"] = r
        else:
            r = np.zeros(10, U32)
            r[:8] = seed_key(c.cfgs[0]["seed"])
            r[8] = self.consumed[0]
            s["RNG"] = r
        if c.family == "rows_par":
            s["WORDS"] = self.wtab.copy()
        if c.prep:
            s["PREP_N"] = self.prep_n.copy()
            s["EPOCH"] = self.epoch.copy()
        if c.hid:
            s["HID"] = self.hid.copy()
        if c.cap_frames:
            s["CAP"] = self.cap.copy()
        return s

    def run(self):
        c = self.c
        snaps = []
        for f in range(c.F):
            self.X[:] = c.x[f].view(U32)  # (the hidden rows the slow transformer left)
            if c.family == "rows_par":
                self.rows_words(f)
                snaps.append(self.snapshot())
            (self.single_slow if c.single else self.rows_slow if c.rows else self.slots_slow)(f)
            snaps.append(self.snapshot())
            for cb in range(c.n_cb):
                (self.single_fast if c.single else self.rows_fast if c.rows else self.slots_fast)(f, cb)
                snaps.append(self.snapshot())
        return {k: np.stack([s[k] for s in snaps]) for k in snaps[0]}


_REF_CACHE = {}


def reference(case, mut=None):
    """the expected state after every launch: dict name -> array [L, ...] (uint32 views of every exact output; PREP_N float64 [L][32][dim],
    NaN = a row the launches have not written).  Computed once per (case, mutation) and shared; callers must not modify it."""
    key = (case.name, mut)
    if key not in _REF_CACHE:
        _REF_CACHE[key] = Machine(case, mut).run()
    return _REF_CACHE[key]


def prep_planes(case, raw):
    """PREP output uint16 [L][2 * 32 * dim] -> (hi, lo) float64 [L][32][dim] and the raw words [L][32][dim][2]"""
    D = case.dim
    m, k = np.meshgrid(np.arange(32), np.arange(D), indexing="ij")
    raw = raw.reshape(-1, 2 * 32 * D)
    w = np.stack([raw[:, gemm_refs.frag_off(m, k, p, D)] for p in (0, 1)], -1)
    f = (w.astype(U32) << 16).view(F32).astype(F64)
    return f[..., 0], f[..., 1], w


def prep_tol(case, n):
    return (((case.dim / 256 + 16) / 2 + 3) * gemm_refs.U + 2.0 ** -17) * np.abs(n)


def compare(case, ref, got):
    """-> (list of mismatch strings (empty = the traces agree), worst prep |err| / tol)"""
    bad, worst = [], 0.0
    for name, e in ref.items():
        if name == "PREP_N":
            hi, lo, w = prep_planes(case, got["PREP"])
            written = ~np.isnan(e)
            err = np.abs(np.where(written, hi + lo - np.where(written, e, 0), 0))
            tol = np.where(written, prep_tol(case, np.where(written, e, 1)), 1)
            ratio = float((err / np.maximum(tol, 1e-300)).max())
            worst = max(worst, ratio)
            if not (err <= tol).all():
                bad.append(f"PREP: worst |err| / tol = {ratio:.3f} at {np.unravel_index(np.argmax(err / np.maximum(tol, 1e-300)), err.shape)}")
            if not (w[~written] == 0xFFFF).all():
                bad.append("PREP: a row no launch has written is not poison any more")
            continue
        g = got[name].reshape(e.shape)
        if not np.array_equal(g, e.astype(U32)):
            at = np.argwhere(g != e.astype(U32))[0]
            bad.append(f"{name}: first mismatch at launch {at[0]} (frame {at[0] // case.Lf}, node {at[0] % case.Lf}) index {tuple(at[1:])}: "
                       f"got {g[tuple(at)]:#x}, expected {int(e[tuple(at)]):#x}")
    return bad, worst


def traces_differ(a, b):
    return any(not np.array_equal(a[k], b[k], equal_nan=True) if a[k].dtype.kind == "f" else not np.array_equal(a[k], b[k]) for k in a)


# ------------------------------------------------------------------------------------------------------------------ crafted rows
def noise(r, n, lo=-1.0):
    return (lo + r.random_sample(n)).astype(F32)


def scripted_row(r, n, cand):
    v = noise(r, n)
    v[cand] = 2.0
    return v


def probe_row(r, n, a, b, negative=False):
    v = noise(r, n, -3.0 if negative else -1.0)
    v[a], v[b] = (-1.0, -0.9) if negative else (1.0, 0.9)
    return v


def tie_rows(r, n, ept):
    """greedy tie rows over n candidates for a kernel whose thread owns `ept` consecutive candidates (1: the strided 1024-thread kernels)"""
    rows = []

    def pair(i, j, v=1.0):
        if 0 <= i < j < n:
            w = noise(r, n)
            w[i] = w[j] = v
            rows.append(w)
    pair(5, 6); pair(7, 71); pair(9, 9 + 1024); pair(0, n - 1); pair(n - 2, n - 1)
    pair(3 * ept + ept - 1, 3 * ept + ept); pair(63 * ept + ept - 1, 64 * ept); pair(1023, 1024)
    rows.append(np.full(n, 0.5, F32))                       # all candidates equal
    w = np.full(n, -np.inf, F32); w[n // 2 + 1] = 0.0       # -inf everywhere but one
    rows.append(w)
    for i, j in ((5, 70 % n if 70 % n > 5 else n - 1), (1, 2)):  # +0 and -0 at the maximum, both orders, every other candidate negative
        for zi, zj in ((0.0, -0.0), (-0.0, 0.0)):
            w = noise(r, n, -2.0)
            w[i], w[j] = zi, zj
            rows.append(w)
    w = noise(r, n); w[0] = 1.0                             # the maximum at candidate 0 (<|im_end|> of a slow row): last
    rows.append(w)
    return rows


# window scripts: per codebook a list over frames of ("pick", tok) | ("probe", a, b, negative) | ("pentie", a, b); fillers are distinct
A, Bq = 40, 41  # the probed pair; fillers come from 0 .. 39 and 42 ..


def _fill(F, events):
    used = iter([t for t in range(2, 64) if t not in (A, Bq)])
    return [events.get(f) or ("pick", next(used)) for f in range(F)]


def window_scripts(F=24):
    return [
        _fill(F, {0: ("pick", A), 2: ("pentie", None, None), 15: ("probe", A, Bq, False)}),                    # age 15: penalised
        _fill(F, {0: ("pick", A), 16: ("probe", A, Bq, False)}),                                                # age 16: the last penalised age
        _fill(F, {0: ("pick", A), 17: ("probe", A, Bq, False)}),                                                # age 17: out of the window
        _fill(F, {0: ("pick", A), 5: ("pick", A), 17: ("probe", A, Bq, False)}),                                # twice; the OLDER instance has just left
        _fill(F, {0: ("pick", A), 5: ("pick", A), 22: ("probe", A, Bq, False)}),                                # twice; the younger one has left as well
        _fill(F, {0: ("pick", A), 16: ("pick", A), 17: ("probe", A, Bq, False)}),                               # last == dropped
        _fill(F, {0: ("pick", A), 16: ("probe", A, Bq, True)}),                                                 # negative pair, penalised: a wins
        _fill(F, {0: ("pick", A), 17: ("probe", A, Bq, True)}),                                                 # negative pair, not penalised: b wins
    ]


def script_rows(r, n, script, f, rep_pen, prev_pick):
    ev = script[f]
    if ev[0] == "pick":
        return scripted_row(r, n, ev[1])
    if ev[0] == "probe":
        return probe_row(r, n, ev[1], ev[2], ev[3])
    # a tie created only by the division: the previous pick holds exactly the penalty, a LATER candidate holds 1.0
    v = noise(r, n)
    v[prev_pick] = F32(rep_pen)
    v[n - 1] = 1.0
    return v


def window_case(name, family, rep_pens, wt="bf16", n_cb=8, F=24):
    B = len(rep_pens)
    r = np.random.RandomState(zlib_seed(name))
    scripts = window_scripts(F)
    cfgs = [dict(temp=0.0, top_p=1.0, top_k=0, rep_pen=p, seed=7 + i, ignore_eos=1) for i, p in enumerate(rep_pens)]
    logits = []
    for f in range(F):
        slow = np.stack([scripted_row(r, 40, 3 + (f + b) % 30) for b in range(B)])
        fast = np.stack([np.stack([script_rows(r, 64, scripts[(cb + b) % 8], f, rep_pens[b], scripts[(cb + b) % 8][f - 1][1] if f else 0)
                                   for b in range(B)]) for cb in range(n_cb)])
        logits.append((slow, fast))
    return Case(name, family, cfgs, logits, B=B, n_cb=n_cb, cb_size=64, n_slow=40, dim=128, wt=wt, out_cap=F + 2)


def tie_case(name, family, n_slow, cb_size, ignore_eos, B=1, n_cb=2, dim=128, wt="bf16", **kw):
    r = np.random.RandomState(zlib_seed(name))
    slots = family.startswith("slots")
    ts, tf = tie_rows(r, n_slow, 4 if slots else 1), tie_rows(r, cb_size, 2 if slots else 1)
    F = len(ts)
    temp = 0.0
    cfgs = [dict(temp=temp, top_p=1.0, top_k=0, rep_pen=1.0, seed=3 + i, ignore_eos=ignore_eos) for i in range(B if slots else 1)]
    logits = []
    for f in range(F):
        slow = np.stack([ts[(f + b) % F] if (f + b) % F != F - 1 or f == F - 1 else ts[0] for b in range(B)])
        fast = np.stack([np.stack([tf[(f + cb + b) % len(tf)] for b in range(B)]) for cb in range(n_cb)])
        logits.append((slow, fast))
    return Case(name, family, cfgs, logits, B=B, n_cb=n_cb, cb_size=cb_size, n_slow=n_slow, ld=2048 if n_slow > 1024 else None, dim=dim, wt=wt,
                out_cap=F + 2, **kw)


def _slow_row(r, n, pick):
    """a slow row whose greedy pick is candidate `pick` under either tie rule"""
    return scripted_row(r, n, pick)


def term_case(name, family, term_frames, B, F, ignore_eos=0, tokens=FISH15, session=0, out_cap=64, state0=None, n_cb=2, n_slow=40, hid=False,
              cfgs=None, **kw):
    """row b's slow pick is candidate 0 (<|im_end|>) at frame term_frames[b] (None: never), an audio candidate otherwise"""
    r = np.random.RandomState(zlib_seed(name))
    slots = family.startswith("slots")
    if cfgs is None:
        cfgs = [dict(temp=0.0, top_p=1.0, top_k=0, rep_pen=1.2, seed=11 + i, ignore_eos=ignore_eos) for i in range(B if slots else 1)]
    logits = []
    for f in range(F):
        slow = np.stack([_slow_row(r, n_slow, 0 if term_frames[b] == f else 1 + (5 * f + b) % (n_slow - 1)) for b in range(B)])
        fast = np.stack([np.stack([scripted_row(r, 64, (7 * f + 3 * cb + b) % 64) for b in range(B)]) for cb in range(n_cb)])
        logits.append((slow, fast))
    return Case(name, family, cfgs, logits, B=B, n_cb=n_cb, cb_size=64, n_slow=n_slow, dim=128, tokens=tokens, session=session, out_cap=out_cap,
                state0=state0, hid=hid, **kw)


def random_case(name, family, cfgs, B, F, n_slow, cb_size, n_cb, dim, prep=False, scale=3.0, **kw):
    r = np.random.RandomState(zlib_seed(name))
    logits = [((r.standard_normal((B, n_slow)) * scale).astype(F32), (r.standard_normal((n_cb, B, cb_size)) * scale).astype(F32)) for _ in range(F)]
    return Case(name, family, cfgs, logits, B=B, n_cb=n_cb, cb_size=cb_size, n_slow=n_slow, ld=2048 if n_slow > 1024 else None, dim=dim, prep=prep,
                out_cap=F + 2, **kw)


def legacy_pair(u, above):
    """(pad, eos) with p_pad a few f32 ulps above / below u: as close as the one-ulp freedom of the exponential allows -- p_pad is
    e / (e + 1) or 1 / (1 + e) with e = expf(d) known to one ulp, which moves p_pad by at most p (1 - p) 2^-23 <= half an ulp of p for
    p >= 1/2 and at most one ulp below; the pair is searched so that the float64 value of p_pad lies 3 .. 9 ulps of u on the wanted side"""
    u = float(u)
    ulp = float(np.spacing(F32(max(u, 2.0 ** -20))))
    want = u + (6 * ulp if above else -6 * ulp)
    want = min(max(want, 1e-6), 1 - 1e-6)
    d = F32(np.log(1.0 / want - 1.0))  # eos - pad
    for _ in range(4096):
        p = 1.0 / (1.0 + np.exp(np.float64(d)))
        off = (p - u) / ulp
        if (3 <= off <= 9) if above else (-9 <= off <= -3):
            return F32(0.0), d
        d = np.nextafter(d, F32(-np.inf) if (off < 3 if above else off < -9) else F32(np.inf)).astype(F32)
    raise AssertionError("no (pad, eos) pair found")


def legacy_case(name, family, temps, ignore_eos=0, cap_frames=0, F=4):
    """2-row slow logits around the host-computed draws of each stream: frame f sits just above u (pad), the last frame just below (im_end)"""
    B = len(temps)
    r = np.random.RandomState(zlib_seed(name))
    n_cb = 2
    cfgs = [dict(temp=t, top_p=0.8, top_k=16, rep_pen=1.2, seed=100 + i, ignore_eos=ignore_eos) for i, t in enumerate(temps)]
    words = [stream_words(k["seed"], F * (n_cb + 1) + 4) for k in cfgs]
    logits = []
    for f in range(F):
        slow = np.zeros((B, 2), F32)
        for b in range(B):
            # the slow word of frame f: sampled streams draw 1 + n_cb words per live frame, greedy ones only the slow word
            at = f * (n_cb + 1) if temps[b] != 0 else f
            slow[b] = legacy_pair(legacy_u(words[b][at]), above=(f + b) % F != F - 1)
        fast = (r.standard_normal((n_cb, B, 64)) * 3).astype(F32)
        logits.append((slow, fast))
    return Case(name, family, cfgs, logits, B=B, n_cb=n_cb, cb_size=64, n_slow=2, ld=8, dim=128, tokens=LEGACY, cap_frames=cap_frames, out_cap=F + 2)


PROD = dict(temp=0.7, top_p=0.8, top_k=256, rep_pen=1.2)
OTHER = dict(temp=1.0, top_p=0.9, top_k=40, rep_pen=1.5)


@functools.lru_cache(maxsize=None)
def all_cases():
    cs = []
    # ---- window scripts (families with a penalty)
    cs.append(window_case("window/single/1.2", "single", [1.2]))
    cs.append(window_case("window/single/1.5/f32", "single", [1.5], wt="f32"))
    cs.append(window_case("window/single/1.0", "single", [1.0]))
    cs.append(window_case("window/slots", "slots", [1.2, 1.5, 1.0]))
    cs.append(window_case("window/slots_wide", "slots_wide", [1.5, 1.0, 1.2, 1.2]))
    # ---- ties, both rules, every family
    for fam, kw in (("single", {}), ("single_batchrow", dict(batch_rows=3, batch_row=1)), ("rows", dict(B=3)), ("slots", dict(B=3)),
                    ("slots_wide", dict(B=2))):
        cs.append(tie_case(f"ties/{fam}/2037x1024", fam, 2037, 1024, 1, **kw))
        cs.append(tie_case(f"ties/{fam}/2048x64/eos", fam, 2048, 64, 0, **kw))
    cs.append(tie_case("ties/rows/session", "rows", 40, 64, 0, B=2, session=1))
    # ---- termination and emission
    cs.append(term_case("term/single/frame0+2replays", "single", [0], 1, 3, hid=True))
    cs.append(term_case("term/single/frame0/ignore_eos", "single", [0], 1, 3, ignore_eos=1, hid=True))
    cs.append(term_case("term/single/frame2+2replays/out_cap2", "single", [2], 1, 5, out_cap=2, hid=True))
    cs.append(term_case("term/single/out_cap3", "single", [None], 1, 5, out_cap=3))
    cs.append(term_case("term/single/generic", "single", [3], 1, 5, tokens=GENERIC))
    cs.append(term_case("term/single/one_sem", "single", [None], 1, 3, tokens=ONE_SEM, n_slow=8))
    cs.append(term_case("term/single_batchrow", "single_batchrow", [2], 1, 4, batch_rows=3, batch_row=2))
    for sess in (0, 1):
        cs.append(term_case(f"term/rows/session{sess}", "rows", [0, 2, None, 1], 4, 5, session=sess, out_cap=3))
        cs.append(term_case(f"term/rows/generic/session{sess}", "rows", [1, None, 0], 3, 4, session=sess, tokens=GENERIC))
    cs.append(term_case("term/rows/generic_low", "rows", [0, None], 2, 3, tokens=GENERIC_LOW))
    cs.append(term_case("term/rows/one_sem", "rows", [None, 1], 2, 3, tokens=ONE_SEM, n_slow=8))
    cs.append(term_case("term/rows/ignore_eos", "rows", [0, 1], 2, 3, ignore_eos=1))
    parked = np.zeros((4, ST_WORDS), I32)
    parked[1, [POS, FRAME, DONE, NOUT, HAVE]] = [30, 7, 2, 7, 1]   # a parked slot next to live ones
    parked[1, CUR] = FISH15["im_end_id"]; parked[1, CUR + 1: CUR + 3] = [5, 6]; parked[1, PREV: PREV + 3] = [13, 5, 6]
    parked[2, [POS, FRAME, NOUT, HAVE]] = [12, 3, 3, 1]             # a slot in mid-flight: the window starts with its previous codes
    parked[2, PREV: PREV + 3] = [14, 9, 9]
    parked[3, CUR + 1: CUR + 3] = [7, 8]                            # stale codes under a frame-0 <|im_end|>: emitted as zeros
    for fam in ("slots", "slots_wide"):
        cs.append(term_case(f"term/{fam}/mix", fam, [None, None, 1, 0], 4, 4, state0=parked, out_cap=4))
        cs.append(term_case(f"term/{fam}/ignore_eos+generic", fam, [0, 1], 2, 3, ignore_eos=1, tokens=GENERIC))
    # ---- RNG numbering: child indices, the words table, consumed, look-ahead tags
    for B in (1, 3, 9):
        s = dict(temp=0.8, top_p=0.9, top_k=16, seed=42 + B)
        cs.append(random_case(f"rng/rows/B{B}", "rows", [s], B, 3, 40, 64, 2, 128))
        cs.append(random_case(f"rng/rows_par/B{B}", "rows_par", [s], B, 3, 40, 64, 2, 128, prep=True))
        cs.append(random_case(f"rng/single_batchrow/B{B}", "single_batchrow", [dict(s, rep_pen=1.0)], 1, 3, 40, 64, 2, 128, batch_rows=B, batch_row=B // 2))
    cs.append(random_case("rng/rows/session1/B3", "rows", [dict(temp=0.8, top_p=0.9, top_k=0, seed=5)], 3, 4, 40, 64, 2, 128, session=1, scale=1.0))
    cs.append(random_case("rng/slots_wide/nodraw", "slots_wide",
                          [dict(temp=0.9, top_p=0.0, top_k=0, rep_pen=1.2, seed=1), dict(temp=0.9, top_p=0.7, top_k=0, rep_pen=1.2, seed=2),
                           dict(temp=0.0, top_p=1.0, top_k=0, rep_pen=1.2, seed=3), dict(temp=0.9, top_p=0.9, top_k=300, rep_pen=1.0, seed=4, ignore_eos=1),
                           dict(temp=0.6, top_p=0.9, top_k=16, rep_pen=1.2, seed=5, ignore_eos=1)], 5, 4, 2037, 1024, 2, 128, scale=2.0))
    cs.append(random_case("rng/slots/mixed", "slots", [dict(temp=0.0, top_p=1.0, top_k=0, rep_pen=1.2, seed=8, ignore_eos=1),
                                                       dict(temp=0.7, top_p=0.8, top_k=16, rep_pen=1.2, seed=9, ignore_eos=1)], 2, 4, 40, 64, 8, 128, prep=True))
    cs.append(random_case("rng/single/general_path", "single", [dict(temp=0.9, top_p=0.9, top_k=0, rep_pen=1.2, seed=77, ignore_eos=1)], 1, 3, 2037, 1024,
                          2, 128))
    # ---- Fish <= 1.4 slow decision
    cs.append(legacy_case("legacy/single/sampled", "single", [0.7]))
    cs.append(legacy_case("legacy/single/greedy", "single", [0.0]))
    cs.append(legacy_case("legacy/single/ignore_eos", "single", [0.7], ignore_eos=1))
    cs.append(legacy_case("legacy/slots/mix+capture", "slots", [0.7, 0.0, 0.9], cap_frames=3))
    cs.append(legacy_case("legacy/slots_wide/ignore_eos", "slots_wide", [0.0, 0.7], ignore_eos=1, cap_frames=5))
    # ---- production wiring in volume: 8 rows x 24 frames of random rows at n = 2037 / 1024, production settings and one other
    for tag, s in (("prod", PROD), ("other", OTHER)):
        cs.append(random_case(f"volume/single/{tag}", "single", [dict(s, seed=1000, ignore_eos=1)], 1, 24, 2037, 1024, 8, 1024))
        cs.append(random_case(f"volume/single_batchrow/{tag}", "single_batchrow", [dict(s, rep_pen=1.0, seed=1001, ignore_eos=1)], 1, 24, 2037, 1024, 8,
                              1024, batch_rows=8, batch_row=5))
        cs.append(random_case(f"volume/rows/{tag}", "rows", [dict(s, seed=1002)], 8, 24, 2037, 1024, 8, 1024, prep=True))
        cs.append(random_case(f"volume/rows_par/{tag}", "rows_par", [dict(s, seed=1003)], 8, 24, 2037, 1024, 8, 1024, prep=True))
        cs.append(random_case(f"volume/slots/{tag}", "slots", [dict(s, seed=1100 + i, ignore_eos=int(i != 3)) for i in range(8)], 8, 24, 2037, 1024, 8,
                              1024, prep=True))
    cs.append(random_case("volume/slots_wide/mix", "slots_wide",
                          [dict([PROD, OTHER, dict(temp=0.8, top_p=0.7, top_k=0, rep_pen=1.2), dict(temp=1.0, top_p=0.95, top_k=400, rep_pen=1.2)][i % 4],
                                seed=1200 + i, ignore_eos=int(i != 6)) for i in range(8)], 8, 24, 2037, 1024, 8, 1024, prep=True))
    names = [c.name for c in cs]
    assert len(set(names)) == len(names)
    return tuple(cs)


def case_by_name(name):
    return next(c for c in all_cases() if c.name == name)


# ------------------------------------------------------------------------------------------------------------------ mutations
# mutation of the REFERENCE machines -> the listed cases whose expected trace it must change (at least one; test_sample_ref_cpu checks)
MUTATIONS = {
    "win15": ("window/single/1.2", "window/slots"),                  # window depth 15: the age-16 probe is no longer penalised
    "win17": ("window/single/1.2", "window/slots"),                  # window depth 17: the age-17 probe still is
    "reset_when_none": ("window/single/1.2", "window/slots_wide"),   # a correct count: the mask survives the older instance's exit
    "neg_multiply": ("window/single/1.2", "window/slots"),           # a negative logit is multiplied (the HF rule), not divided
    "first_for_last": ("ties/single/2037x1024", "ties/slots/2037x1024", "ties/slots_wide/2048x64/eos"),
    "last_for_first": ("ties/rows/2037x1024", "ties/single_batchrow/2048x64/eos"),
    "no_frame0_emit": ("term/single/frame0+2replays", "term/rows/session0", "term/slots/mix"),
    "emit_terminating": ("term/single/frame2+2replays/out_cap2", "term/rows/session0"),  # (a slot's terminating frame is held back by the freeze: frozen_advances)
    "done_never_2": ("term/single/frame0+2replays",),
    "no_have_prev": ("window/single/1.2", "window/slots"),           # have_prev left unset: the window never fills
    "frozen_advances": ("term/slots/mix", "term/rows/session1"),
    "keep_nonaudio_codes": ("term/rows/session0", "term/slots/mix"),
    "child_swap": ("rng/rows/B3", "rng/rows_par/B9", "rng/single_batchrow/B3"),
    "fast_call_off": ("rng/rows/B3", "rng/rows_par/B3", "rng/single_batchrow/B9"),
    "count_nodraw": ("rng/slots_wide/nodraw",),
    "past_cap": ("term/single/out_cap3", "term/rows/session0"),
}
# No waivers: every mutation must change every case listed for it, except that B = 1 makes child_swap the identity (no B1 case is listed).


# ------------------------------------------------------------------------------------------------------------------ rejected cases
def rejected_cases():
    """(label, case, field overrides, substring of the error) -- the hook must refuse each before any device call"""
    base = lambda fam="rows", **kw: random_case("rej/" + fam, fam, [dict(temp=0.8, top_p=0.9, top_k=16, seed=1)] * (2 if fam.startswith("slots") else 1),
                                                 2 if not fam.startswith("single") else 1, 1, 40, 64, 2, 128, **kw)
    return [
        ("n_cb + 1 > 16", base(), dict(n_cb=16), "n_cb + 1 <= 16"),
        ("slow capacity", base("single"), dict(n_slow=4097, ld=4100), "larger than the sampler capacity"),
        ("slot slow capacity", base("slots"), dict(n_slow=2049, ld=2049), "per-slot sampler capacity"),
        ("slot codebook capacity", base("slots_wide"), dict(cb_size=1025), "per-slot sampler capacity"),
        ("ld < n", base(), dict(ld=39), "n_slow <= ld"),
        ("rows_par greedy", random_case("rej/par0", "rows_par", [dict(temp=0.0, top_p=1.0, top_k=16, seed=1)], 2, 1, 40, 64, 2, 128), {}, "rows_par_sampler_ok"),
        ("rows_par top_k", random_case("rej/par1", "rows_par", [dict(temp=0.8, top_p=1.0, top_k=64, seed=1)], 2, 1, 40, 64, 2, 128), {}, "rows_par_sampler_ok"),
        ("narrow slot, nucleus only", random_case("rej/s0", "slots", [dict(temp=0.8, top_p=0.9, top_k=0, seed=1)] * 2, 2, 1, 40, 64, 2, 128), {},
         "0 < top_k <= 256"),
        ("narrow slot, top_k 300", random_case("rej/s1", "slots", [dict(temp=0.8, top_p=0.9, top_k=300, seed=1)] * 2, 2, 1, 2037, 1024, 2, 128), {},
         "0 < top_k <= 256"),
        ("prep dim", base(prep=True), dict(dim=2048), "dim <= 1024"),
        ("prep dim % 4", base(prep=True), dict(dim=126), "dim <= 1024"),
        ("single with B = 2", base("single"), dict(B=2), "one row"),
        ("batch_row outside", base("single_batchrow", batch_rows=3, batch_row=1), dict(batch_row=3), "batch_row"),
        ("legacy rows", base(tokens=LEGACY), {}, "token layout"),
        ("tables too short", base(), dict(tok_rows=20), "outside tok_emb"),
        ("n_cfg", base("slots"), dict(n_cfg=1), "n_cfg"),
    ]


def call_rejected(case, over):
    """plan_only = 0 on purpose: the refusal must come before any device call (this runs on machines without a GPU)"""
    from fishrt import _ffi
    c, keep = case.ffi(plan_only=False, **over)
    o = _ffi.SampleOut()
    rc = _ffi.lib().fs_selftest_sample_frames(0, C.byref(c), C.byref(o))
    return rc, _ffi.lib().fs_last_error().decode()
