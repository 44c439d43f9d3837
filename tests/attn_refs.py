"""Float64 definitions of the attention the kernels of csrc/lm_attn.hip (and k_wo's merge prologues) implement, the input builders of the
per-launcher attention tests, the per-element error bound, and the ctypes wrapper of fs_selftest_attn.  Shared by test_attn_ref_cpu.py (CPU:
pins these definitions, the plan names and the teeth of every case) and test_attn_paths_gpu.py (GPU).

Definitions (dual_ar.rs:252-279): row m of length T attends over tokens [0, T) of its sequence's paged cache; query head h reads kv head
g = h // n_rep; s_t = (q . k_t) / sqrt(Dh), w = softmax(s), o = sum_t w_t v_t.  A partial over a token range is {o = sum_t exp(s_t - m) v_t,
m = max s_t, l = sum_t exp(s_t - m)}; partials merge as o = sum_c exp(m_c - M) o_c / sum_c exp(m_c - M) l_c.

Bound per output element (row, head, dim d), from the reference's own quantities: A_t = scale sum_i |q_i k_ti|, R_t = max s - s_t,
B_d = sum_t w_t |v_td|, u = 2^-24, delta = (Dh + 2) eps_q max_t A_t, eps_exp(x) = 4 c (|x| + 1) u with c = EXPF_C = 1.203 the measured
constant of the device's __expf (4 = this project's margin for device functions):
    tol_d = 2 sum_t w_t (2 delta + eps_exp(R_t) + eps_p) |v_td| + (T + 64) u B_d + eps_out |o_d|
eps_q = eps_p = u for the VALU kernels, 2^-16 for the MFMA prefill (q and p travel as bf16 hi + lo); eps_out = 2^-17 for hi + lo outputs, u
for f32 outputs.  (T + 64) u B_d holds for any summation order.  For an un-normalised partial the same expression with p_t = exp(s_t - m) in
place of w_t bounds o, with |v| = 1 it bounds l, and m is held to delta + u |m|."""
import ctypes as C

import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
KV_PAGE = 64
STALE = 2.0 ** 100
# measured on an MI355X by test_attn_paths_gpu.test_expf_constant (printed there): max |rel err| / ((|x| + 1) u) of __expf against float64 exp
# over every x of [-88, 0] whose e^x is a normal float (x >= EXPF_NORMAL_MIN = ln 2^-126).  Below that -- the last 0.66 of the interval -- the
# true value is subnormal and the device returns 0 (flushed: an absolute error below 2^-126, asserted there as such).  No case of these tests
# has a score more than 80 below its maximum, so the flush never enters a bound.
EXPF_C = 1.203
EXPF_FINDING = 8.0
EXPF_NORMAL_MIN = -87.33654475

GEOMS = {"TINY": (4, 2, 32), "MID": (4, 2, 64), "FISH": (16, 2, 64)}  # (H, Hk, Dh)
WT = {"f32": 0, "bf16": 1, "fp8": 2}
OPS = {"DECODE": 0, "DECODE_WO": 1, "WO_FUSED": 2, "ROWS": 3, "EXPF": 4}


def chunk_of(wt):
    return 64 if wt == "f32" else 128


def bf16_rne(x):
    """f32 -> nearest bf16 (ties to even), returned as f32"""
    b = np.ascontiguousarray(x, F32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) >> 16 << 16
    return (b & 0xFFFFFFFF).astype(np.uint32).view(F32).reshape(np.shape(x))


def kv_round(x, wt):
    return np.asarray(x, F32) if wt == "f32" else bf16_rne(x)


def rope_i(x, cos, sin):
    """interleaved RoPE (dual_ar.rs:239-249) of x [..., Dh] with cos / sin [Dh / 2]: pairs (2j, 2j + 1)"""
    x = np.asarray(x, F64)
    a, b = x[..., 0::2], x[..., 1::2]
    out = np.empty_like(x)
    out[..., 0::2] = a * cos - b * sin
    out[..., 1::2] = a * sin + b * cos
    return out


def gather(pool, table_row, n_tok, g):
    """tokens [0, n_tok) of kv head g of the sequence whose page-table row is table_row, from a pool [n_pages][Hk][64][Dh] -> [n_tok][Dh]"""
    t = np.arange(n_tok)
    return pool[np.asarray(table_row)[t // KV_PAGE], g, t % KV_PAGE]


def partial(q, k, v, eps_q=U, eps_p=U, dup=None):
    """one query head q [Dh] over tokens k, v [T][Dh] in float64 -> dict with the un-normalised partial {o, m, l}, the weights p = exp(s - m) and
    the absolute bounds on o, m, l (module docstring).  dup = (a, b): tokens [a, b) counted twice (a mutation)"""
    q, k, v = np.asarray(q, F64), np.asarray(k, F64), np.asarray(v, F64)
    Dh, T = q.shape[0], k.shape[0]
    scale = 1.0 / np.sqrt(float(Dh))
    s = (k @ q) * scale
    A = (np.abs(k) @ np.abs(q)) * scale
    m = s.max()
    R = m - s
    p = np.exp(-R)
    if dup is not None:
        p = p.copy()
        p[dup[0]:dup[1]] *= 2.0
    delta = (Dh + 2) * eps_q * A.max()
    e_t = 2 * delta + 4 * EXPF_C * (R + 1) * U + eps_p
    o = p @ v
    l = p.sum()
    tol_o = 2 * ((p * e_t) @ np.abs(v)) + (T + 64) * U * (p @ np.abs(v))
    tol_l = 2 * (p * e_t).sum() + (T + 64) * U * l
    return dict(o=o, m=m, l=l, p=p, tol_o=tol_o, tol_l=tol_l, tol_m=delta + U * abs(m), s=s)


def attend(q, k, v, eps_q=U, eps_p=U, eps_out=U, dup=None):
    """normalised attention of one head -> (o [Dh], tol [Dh], w [T])"""
    r = partial(q, k, v, eps_q, eps_p, dup)
    o = r["o"] / r["l"]
    return o, r["tol_o"] / r["l"] + eps_out * np.abs(o), r["p"] / r["l"]


def merge(parts):
    """merge of {o, m, l} partials (each o [Dh]) -> normalised o"""
    M = max(p["m"] for p in parts)
    L = sum(p["l"] * np.exp(p["m"] - M) for p in parts)
    return sum(p["o"] * np.exp(p["m"] - M) for p in parts) / L


def hadamard(n):
    i = np.arange(n)
    bits = i[:, None] & i[None, :]
    pc = np.zeros_like(bits)
    while bits.any():
        pc += bits & 1
        bits >>= 1
    return (1 - 2 * (pc & 1)).astype(F64)


def edge_tokens(T, wt):
    """0, T - 1 and both sides of the 16 / 64 / CH / 8 CH edge nearest to T - 1 (inside [0, T))"""
    out = [0, T - 1]
    for e in (16, 64, chunk_of(wt), 8 * chunk_of(wt)):
        b = max(e, (T - 1) // e * e)
        out += [b - 1, b]
    seen, res = set(), []
    for t in out:
        if 0 <= t < T and t not in seen:
            seen.add(t)
            res.append(t)
    return res


# ---------------------------------------------------------------------------------------------------------------------------- cases
class Case:
    """One fs_selftest_attn call and what the reference needs to restate it.  seq_L: tokens of each sequence that hold data; rows: (sequence
    index, T) per activation row; Ts: the lengths as the case table gives them (decode: [T]; prefill / chunked rows: [M]).  kind: 'decode' | 'decode_wo' | 'fused' | 'rows' (pos_step 0 / -1) | 'prefill' | 'group'
    | 'small' | 'tbl'."""

    def __init__(self, cid, kind, wt, geom, tier, expect, Ts, nc_launch=0, n_chunks_max=0, pos_step=0, seed=0, **kw):
        self.id, self.kind, self.wt, self.geom, self.tier, self.expect = cid, kind, wt, geom, tier, expect
        self.H, self.Hk, self.Dh = GEOMS[geom]
        self.n_rep = self.H // self.Hk
        self.K = self.H * self.Dh
        self.Ts = list(Ts)
        self.nc_launch, self.n_chunks_max, self.pos_step = nc_launch, n_chunks_max or nc_launch, pos_step
        self.seed = seed
        self.flags = {k: kw.pop(k, 0) for k in ("no_flash", "chunked_attn", "small_attn", "identity_pages")}
        self.seq_rows = kw.pop("seq_rows", 0)     # group prefill: rows per sequence
        self.seq_pos = kw.pop("seq_pos", None)    # group prefill: first position per sequence
        self.pos0 = kw.pop("pos0", 0)             # prefill: first position
        self.wo_kind = kw.pop("wo", "identity")   # decode_wo / fused: 'identity' (x0 = 0) or 'random'
        self.stale_part = kw.pop("stale_part", STALE)
        self.pt_extra = kw.pop("pt_extra", 1)
        assert not kw, kw
        self.CH = chunk_of(wt)
        self._build()

    # ---- layout: which activation row reads which sequence at which length
    def _layout(self):
        k = self.kind
        if k in ("decode", "decode_wo", "fused"):
            return [self.Ts[0]], [(0, self.Ts[0])]
        if k == "prefill":
            M = self.Ts[0]
            return [self.pos0 + M], [(0, self.pos0 + m + 1) for m in range(M)]
        if k == "group":
            n_seq = len(self.seq_pos)
            return [p + self.seq_rows for p in self.seq_pos], [(s, self.seq_pos[s] + j + 1) for s in range(n_seq) for j in range(self.seq_rows)]
        if self.pos_step == 1:  # chunked rows of one sequence
            M = self.Ts[0]
            return [self.pos0 + M], [(0, self.pos0 + m + 1) for m in range(M)]
        return list(self.Ts), [(m, T) for m, T in enumerate(self.Ts)]  # rows are sequences

    def _build(self):
        rng = np.random.RandomState(0xA77 + self.seed)
        H, Hk, Dh, wt = self.H, self.Hk, self.Dh, self.wt
        self.seq_L, self.rows = self._layout()
        self.M = len(self.rows)
        n_seq = len(self.seq_L)
        launched = self.nc_launch * self.CH // KV_PAGE if self.kind in ("decode", "decode_wo") or self.flags["chunked_attn"] or \
            (self.kind == "rows" and self.pos_step == 1) else 0
        slots = [max(L // KV_PAGE + 1, launched, -(-(-(-L // self.CH) * self.CH) // KV_PAGE)) for L in self.seq_L]
        if self.kind in ("small", "tbl", "fused"):
            slots = [1] * n_seq
        self.pt_len = max(slots) + self.pt_extra
        # physical pages: a random permutation (non-monotone), sequence 1 shares sequence 0's first page when both fill it
        share = n_seq >= 2 and min(self.seq_L[0], self.seq_L[1]) >= KV_PAGE and self.kind not in ("small", "tbl")
        n_own = sum(slots) - (1 if share else 0)
        if self.flags["identity_pages"] or self.kind == "fused":
            self.n_pages = n_seq + 1
            perm = list(range(n_seq)) + [n_seq]
        else:
            self.n_pages = n_own + 2
            perm = list(rng.permutation(self.n_pages))
        stale_page = perm.pop()
        self.table = np.full((n_seq, self.pt_len), stale_page, np.int32)
        owner = {}
        for s in range(n_seq):
            for j in range(slots[s]):
                if share and s == 1 and j == 0:
                    self.table[1, 0] = self.table[0, 0]
                    continue
                self.table[s, j] = perm.pop(0)
                owner[int(self.table[s, j])] = (s, j)
        # pools: everything stale (+-2^100, finite) until a sequence's own tokens are written
        shape = (self.n_pages, Hk, KV_PAGE, Dh)
        self.k = (STALE * rng.choice([-1.0, 1.0], shape)).astype(F32)
        self.v = (STALE * rng.choice([-1.0, 1.0], shape)).astype(F32)
        had = hadamard(Dh)
        self.dirs = had[1 + np.arange(Hk)]  # +-1 direction per kv head (range / equal tiers)
        self.plant = []
        for s in range(n_seq):
            L = self.seq_L[s]
            if self.tier == "random" or self.tier == "planted":
                ks, vs = rng.randn(Hk, L, Dh), rng.randn(Hk, L, Dh)
                if self.tier == "planted":  # edge token j of the sequence carries 2 x Hadamard row j: mutually orthogonal, norm^2 = 4 Dh;
                    # every other row is random in the complement of all planted directions (up to the rounding to the KV type)
                    P = had[sorted(set((3 + j + o) % Dh for j in range(10) for o in (0, 20)))]
                    ks -= (ks @ P.T / Dh) @ P
                    ed = edge_tokens(L, wt)
                    if share and s == 1:  # the shared page holds sequence 0's rows: its own planted tokens lie behind it (and token 0, common)
                        ed = [t for t in ed if t >= KV_PAGE or t == 0]
                    for j, t in enumerate(ed):
                        ks[:, t] = 2.0 * had[(3 + j + (20 if share and s == 1 and t else 0)) % Dh]
                    vs[:, :, 0] = np.abs(vs[:, :, 0])  # dim 0 of the output is carried by the OTHER tokens, without cancellation: a planted
                    vs[:, ed, 0] = 0.0                 # token counted twice moves it by half
                    self.plant.append(ed)
            elif self.tier == "equal":
                ks = np.broadcast_to(self.dirs[:, None, :] * 0.5, (Hk, L, Dh)).copy()
                vs = rng.randint(-16, 17, (Hk, L, Dh)) / 8.0
            else:  # range_first / range_last: the maximum in the first / last chunk, every other score 60..80 below it
                c = -(60.0 + 0.5 * rng.randint(0, 41, L))
                c[0 if self.tier == "range_first" else L - 1] = 0.0
                ks = self.dirs[:, None, :] * c[None, :, None]
                vs = rng.randn(Hk, L, Dh)
            ks, vs = kv_round(ks, wt), kv_round(vs, wt)
            t = np.arange(L)
            for j in range(-(-L // KV_PAGE)):
                if share and s == 1 and j == 0:
                    continue
                sel = t[(t // KV_PAGE) == j]
                self.k[self.table[s, j], :, sel % KV_PAGE] = ks[:, sel].transpose(1, 0, 2)
                self.v[self.table[s, j], :, sel % KV_PAGE] = vs[:, sel].transpose(1, 0, 2)
        # queries, per tier, from what the pool holds
        self.q = np.zeros((self.M, H, Dh), F32)
        scale = 1.0 / np.sqrt(float(Dh))
        # planted: q = beta k* / 2 gives s* = 2 beta scale Dh = ln(99 L) + 0.5 against ~0 for every other row: weight >= 0.99 and no larger a
        # score than that needs -- the bound grows with max |score| (delta)
        beta_of = lambda L: (np.log(99.0 * L) + 0.5) / (scale * 2 * Dh)
        self.tstar = np.full((self.M, H), -1)
        for m, (s, T) in enumerate(self.rows):
            if self.tier == "random" or self.tier == "equal":
                self.q[m] = rng.randn(H, Dh)
            elif self.tier == "planted":
                pass  # below
            else:
                for h in range(H):
                    self.q[m, h] = self.dirs[h // self.n_rep] / (scale * Dh)
        if self.tier == "planted":  # a row aligns head h with one of the sequence's planted tokens below its own length
            for m, (s, T) in enumerate(self.rows):
                ok = [t for t in self.plant[s] if t < T]
                for h in range(H):
                    t = ok[(h + m) % len(ok)]
                    self.tstar[m, h] = t
                    self.q[m, h] = 0.5 * beta_of(self.seq_L[s]) * gather(self.k, self.table[s], t + 1, h // self.n_rep)[t]
        self.q_ref, self.k_ref, self.v_ref = self.q.astype(F64), self.k, self.v
        if self.kind == "tbl":
            self._build_tbl(rng)
        # the first stale row of every activation row: K aligned with the query of the group's first head (an unmasked read takes over)
        for m, (s, T) in enumerate(self.rows):
            if T == self.seq_L[s] and T < self.pt_len * KV_PAGE:
                page = self.table[s, T // KV_PAGE]
                if (s, T // KV_PAGE) == owner.get(int(page), None) or page == stale_page:
                    for g in range(Hk):
                        sg = np.where(self.q_ref[m, g * self.n_rep] < 0, -1.0, 1.0)
                        self.k[page, g, T % KV_PAGE] = STALE * sg
                        self.k_ref[page, g, T % KV_PAGE] = STALE * sg
        # Wo, x for the wo ops
        if self.kind in ("decode_wo", "fused"):
            if self.wo_kind == "identity":
                self.wo, self.x0 = np.eye(self.K, dtype=F32), np.zeros(self.K, F32)
            else:
                self.wo = (rng.randn(self.K, self.K) / np.sqrt(self.K)).astype(F32)
                self.wo = bf16_rne(self.wo) if wt != "f32" else self.wo
                self.x0 = rng.randn(self.K).astype(F32)

    def _build_tbl(self, rng):
        """k_attn_small_rows_tbl: q / k / v of the row's own token come from row codes[m] of a qkv table; position T - 1 of the page is stale until
        the launch appends bf16_rne(rope_i(k)), bf16_rne(v) there.  Table values carry bf16 precision and the 'cos / sin' tables are dyadic, so
        the rotation is exact in f32 whatever the contraction: the appended row is defined bit for bit."""
        H, Hk, Dh = self.H, self.Hk, self.Dh
        qd, kd = H * Dh, Hk * Dh
        self.tbl_rows, self.rope_rows, self.rope_off, self.code_slot = 12, 16, 3, 2
        self.tbl = bf16_rne(rng.randn(self.tbl_rows, qd + 2 * kd).astype(F32))
        self.codes = rng.randint(0, self.tbl_rows, self.M).astype(np.uint32)
        cs, sn = np.array([1, .5, -.75, .25, -1, 0]), np.array([0, .5, .25, -1, .75, 1])
        idx = rng.randint(0, 6, (self.rope_rows, Dh // 2))
        self.cos_t, self.sin_t = cs[idx].astype(F32), sn[idx].astype(F32)
        self.k_ref, self.v_ref = self.k.copy(), self.v.copy()
        self.appended = []
        for m, (s, T) in enumerate(self.rows):
            pos, row, rp = T - 1, self.tbl[self.codes[m]].astype(F64), T - 1 + self.rope_off
            page = self.table[s, 0]
            self.q_ref[m] = rope_i(row[:qd].reshape(H, Dh), self.cos_t[rp].astype(F64), self.sin_t[rp].astype(F64))
            kn = rope_i(row[qd:qd + kd].reshape(Hk, Dh), self.cos_t[rp].astype(F64), self.sin_t[rp].astype(F64))
            assert np.array_equal(kn.astype(F32).astype(F64), kn)
            self.k[page, :, pos] = STALE * rng.choice([-1.0, 1.0], (Hk, Dh))
            self.v[page, :, pos] = STALE * rng.choice([-1.0, 1.0], (Hk, Dh))
            self.k_ref[page, :, pos] = bf16_rne(kn.astype(F32))
            self.v_ref[page, :, pos] = bf16_rne(row[qd + kd:].reshape(Hk, Dh).astype(F32))
            self.appended.append((int(page), pos))
        self.q[:] = 0

    # ---- the call
    def ffi_case(self, plan_only=0):
        from fishrt import _ffi
        c = _ffi.AttnCase()
        keep = []

        def ptr(a, ct):
            a = np.ascontiguousarray(a)
            keep.append(a)
            return a.ctypes.data_as(C.POINTER(ct))
        k = self.kind
        c.op = {"decode": 0, "decode_wo": 1, "fused": 2}.get(k, 3)
        c.wt = WT[self.wt]
        c.H, c.Hk, c.Dh, c.dim = self.H, self.Hk, self.Dh, self.K
        c.M = self.M
        c.n_pages, c.pt_rows, c.pt_len = self.n_pages, self.table.shape[0], self.pt_len
        c.page_table = ptr(self.table, C.c_int32)
        c.k, c.v, c.q = ptr(self.k, C.c_float), ptr(self.v, C.c_float), ptr(self.q, C.c_float)
        c.n_chunks_max, c.nc_launch, c.part_rows = self.n_chunks_max, self.nc_launch, self.M
        c.plan_only = plan_only
        c.stale_part = self.stale_part
        for f, val in self.flags.items():
            setattr(c, f, val)
        if k in ("decode", "decode_wo"):
            c.pos, c.pos_step, c.pt_stride = self.Ts[0] - 1, 0, 0
        elif k == "fused":
            c.fused_T, c.pos = self.Ts[0], self.Ts[0] - 1
        elif k == "prefill" or (k == "rows" and self.pos_step == 1):
            c.pos, c.pos_step, c.pt_stride = self.pos0, 1, 0
        elif k == "group":
            c.pos, c.pos_step, c.pt_stride, c.seq_rows = 0, 1, self.pt_len, self.seq_rows
            c.seq_pos = ptr(np.asarray(self.seq_pos, np.int32), C.c_int32)
        else:
            c.pt_stride = self.pt_len
            c.pos_step = self.pos_step
            if self.pos_step < 0:
                c.row_pos = ptr(np.asarray([T - 1 for _, T in self.rows], np.int32), C.c_int32)
            else:
                assert len(set(self.Ts)) == 1
                c.pos = self.Ts[0] - 1
        if k in ("decode_wo", "fused"):
            c.wo, c.x = ptr(self.wo, C.c_float), ptr(self.x0, C.c_float)
        if k == "tbl":
            c.tbl0, c.code_slot, c.tbl_rows, c.rope_rows, c.rope_off = 1, self.code_slot, self.tbl_rows, self.rope_rows, self.rope_off
            c.tbl, c.cos_t, c.sin_t = ptr(self.tbl, C.c_float), ptr(self.cos_t, C.c_float), ptr(self.sin_t, C.c_float)
            c.codes = ptr(self.codes, C.c_uint32)
        c._keep = keep
        return c

    def plan_name(self):
        from fishrt import _ffi
        c = self.ffi_case(plan_only=1)
        name = C.create_string_buffer(96)
        n_out, ok = C.c_size_t(0), C.c_int(0)
        _ffi.check(_ffi.lib().fs_selftest_attn(0, C.byref(c), None, 0, C.byref(n_out), None, None, name, 96, C.byref(ok)))
        return name.value.decode()

    def out_size(self):
        if self.kind == "decode":
            return self.H * self.n_chunks_max * (self.Dh + 2)
        if self.kind in ("decode_wo", "fused"):
            return self.K
        return 2 * (-(-self.M // 32) * 32) * self.K

    def run(self):
        """-> (out f32, k_after, v_after, variant, guard_ok)"""
        from fishrt import _ffi
        c = self.ffi_case()
        out = np.zeros(self.out_size(), F32)
        ka, va = np.zeros_like(self.k), np.zeros_like(self.v)
        name = C.create_string_buffer(96)
        n_out, ok = C.c_size_t(0), C.c_int(0)
        fp = C.POINTER(C.c_float)
        _ffi.check(_ffi.lib().fs_selftest_attn(0, C.byref(c), out.ctypes.data_as(fp), out.size, C.byref(n_out), ka.ctypes.data_as(fp),
                                               va.ctypes.data_as(fp), name, 96, C.byref(ok)))
        assert n_out.value == out.size, (n_out.value, out.size)
        return out, ka, va, name.value.decode(), bool(ok.value)

    # ---- the reference.  mut: None | 'drop' (T - 1) | 'extra' (T + 1: the first stale row) | 'g+1' | 'g-1' | 'dup' (the last wave tile twice)
    def _head(self, m, h, mut, lo=0, hi=None):
        s, T = self.rows[m]
        g = h // self.n_rep
        if mut == "g+1":
            g = (g + 1) % self.Hk
        elif mut == "g-1":
            g = (g - 1) % self.Hk
        if mut == "drop":
            T -= 1
        elif mut == "extra":
            T += 1
        hi = T if hi is None else min(hi, T)
        kk = gather(self.k_ref, self.table[s], hi, g)[lo:]
        vv = gather(self.v_ref, self.table[s], hi, g)[lo:]
        a = (self.rows[m][1] - 1) // 16 * 16  # 'dup': the row's last 16-token wave tile [a, T) is counted twice
        dup = (max(a, lo) - lo, hi - lo) if mut == "dup" and hi > max(a, lo) else None
        return self.q_ref[m, h], kk, vv, dup

    def eps(self):
        if self.kind in ("prefill", "group"):
            return dict(eps_q=2.0 ** -16, eps_p=2.0 ** -16, eps_out=2.0 ** -17)
        if self.kind in ("decode", "decode_wo", "fused"):
            return dict(eps_q=U, eps_p=U, eps_out=U)
        return dict(eps_q=U, eps_p=U, eps_out=2.0 ** -17)

    def reference(self, mut=None):
        """normalised attention of every (row, head) -> (o [M][H][Dh], tol, wmax [M][H] = weight of the planted token or the largest weight)"""
        o = np.zeros((self.M, self.H, self.Dh))
        tol = np.zeros_like(o)
        wst = np.zeros((self.M, self.H))
        e = self.eps()
        for m in range(self.M):
            for h in range(self.H):
                if mut == "drop" and self.rows[m][1] == 1:
                    o[m, h], tol[m, h] = np.nan, 0.0
                    continue
                q, kk, vv, dup = self._head(m, h, mut)
                o[m, h], tol[m, h], w = attend(q, kk, vv, dup=dup, **e)
                wst[m, h] = w[self.tstar[m, h]] if self.tstar[m, h] >= 0 and mut is None else w.max()
        return o, tol, wst

    def partial_ranges(self, tpb=1):
        """token ranges of the partial slots a decode launch produces"""
        T, span = self.Ts[0], self.CH * tpb
        return [(z * span, min(T, (z + 1) * span)) for z in range(-(-T // span))]

    def reference_partials(self, tpb=1, mut=None):
        """[H][n_chunks_max][Dh + 2] expected partials (NaN where nothing is written) and their bounds"""
        ref = np.full((self.H, self.n_chunks_max, self.Dh + 2), np.nan)
        tol = np.zeros_like(ref)
        Tm = self.Ts[0] + (1 if mut == "extra" else -1 if mut == "drop" else 0)
        span = self.CH * tpb
        for z in range(-(-Tm // span)):
            for h in range(self.H):
                q, kk, vv, dup = self._head(0, h, mut, z * span, (z + 1) * span)
                r = partial(q, kk, vv, dup=dup)
                ref[h, z, :self.Dh], ref[h, z, self.Dh], ref[h, z, self.Dh + 1] = r["o"], r["m"], r["l"]
                tol[h, z, :self.Dh], tol[h, z, self.Dh], tol[h, z, self.Dh + 1] = r["tol_o"] + U * np.abs(r["o"]), r["tol_m"], r["tol_l"] + U * r["l"]
        return ref, tol

    def reference_x(self, mut=None):
        """x0 + Wo . attention, and its bound: the attention's bound through |Wo|, the GEMV's (dim + 2) u sum |w a|, the add's rounding"""
        o, tol, _ = self.reference(mut)
        a, ta = o.reshape(-1), tol.reshape(-1)
        W = self.wo.astype(F64)
        x = self.x0.astype(F64) + W @ a
        t = np.abs(W) @ ta + (self.K + 2) * U * (np.abs(W) @ np.abs(a)) + U * (np.abs(x) + np.abs(self.x0))
        return x, t


def run_expf(x):
    from fishrt import _ffi
    x = np.ascontiguousarray(x, F32)
    c = _ffi.AttnCase()
    c.op, c.n_expf = OPS["EXPF"], x.size
    c.expf_x = x.ctypes.data_as(C.POINTER(C.c_float))
    out = np.zeros(x.size, F32)
    name = C.create_string_buffer(96)
    n_out, ok = C.c_size_t(0), C.c_int(0)
    _ffi.check(_ffi.lib().fs_selftest_attn(0, C.byref(c), out.ctypes.data_as(C.POINTER(C.c_float)), out.size, C.byref(n_out), None, None, name, 96,
                                           C.byref(ok)))
    return out


# ---------------------------------------------------------------------------------------------------------------------------- the case table
DECODE_CFGS = (("TINY", "f32", "decode/f32/32/2"), ("TINY", "bf16", "decode/bf16/32/2"), ("MID", "bf16", "decode/bf16/64/2"),
               ("FISH", "bf16", "decode/bf16/64/2/hs4"), ("FISH", "f32", "decode/f32/64/8"))
DECODE_TS = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129)


def _nc(T, wt, nc=None):
    return nc or -(-T // chunk_of(wt))


def decode_cases():
    out = []
    for geom, wt, name in DECODE_CFGS:
        for i, T in enumerate(DECODE_TS):
            for tier in ("planted", ("random", "equal", "range_first", "range_last")[(i + len(geom)) % 4]):
                nc = max(_nc(T, wt), 2 if T > 64 else 1)
                out.append(Case(f"decode-{geom}-{wt}-T{T}-{tier}", "decode", wt, geom, tier, name, [T], nc_launch=nc, n_chunks_max=nc + 1, seed=T))
        for T in (130, 700):
            if wt == "bf16" or T == 130:
                nc = 8 if wt == "bf16" else 8
                out.append(Case(f"decode-{geom}-{wt}-T{T}-nc8", "decode", wt, geom, "planted", name, [T], nc_launch=nc, n_chunks_max=8, seed=T))
    # super-chunks (Fish geometry, bf16 KV): nc_launch > 8 -> k_attn_rows<.., PART> over tpb chunks per block
    for wt in ("bf16", "fp8"):
        for T, nc, tpb in ((1024, 8, 1), (1025, 16, 2), (1100, 16, 2), (2048, 16, 2), (2049, 32, 4), (4100, 64, 8)):
            name = "decode/bf16/64/2/hs4" if tpb == 1 else f"decode/part/tpb{tpb}"
            for tier in (("planted", "range_last") if wt == "bf16" else ("planted",)):
                out.append(Case(f"decode-FISH-{wt}-T{T}-nc{nc}-{tier}", "decode", wt, "FISH", tier, name, [T], nc_launch=nc, n_chunks_max=nc + (tpb == 1), seed=T))
    return out


def decode_wo_cases():
    out = []
    mk = lambda cid, wt, geom, tier, name, T, nc, **kw: out.append(Case(cid, "decode_wo", wt, geom, tier, name, [T], nc_launch=nc, n_chunks_max=kw.pop("ncm", nc), seed=T, **kw))
    # register merge of <= 8 partials
    for T, nc in ((100, 1), (200, 2), (1000, 8), (300, 8)):
        mk(f"wo-reg-FISH-bf16-T{T}-nc{nc}", "bf16", "FISH", "planted", "decode/bf16/64/2/hs4+wo/reg", T, nc, ncm=max(nc, 4))
    mk("wo-reg-TINY-bf16-T129-nc2", "bf16", "TINY", "planted", "decode/bf16/32/2+wo/reg", 129, 2)
    mk("wo-reg-MID-bf16-T300-random-wo", "bf16", "MID", "random", "decode/bf16/64/2+wo/reg", 300, 4, wo="random")
    mk("wo-reg-TINY-f32-T130-nc8", "f32", "TINY", "range_last", "decode/f32/32/2+wo/reg", 130, 8)
    # super-chunk partials merged in registers
    mk("wo-part-FISH-bf16-T1100-nc16", "bf16", "FISH", "planted", "decode/part/tpb2+wo/reg", 1100, 16)
    mk("wo-part-FISH-bf16-T4100-nc64", "bf16", "FISH", "range_first", "decode/part/tpb8+wo/reg", 4100, 64)
    # general LDS merge: f32 KV (64-token chunks), including H * nc_launch > 256
    for T, nc in ((513, 9), (600, 16), (1100, 18)):
        mk(f"wo-lds-FISH-f32-T{T}-nc{nc}", "f32", "FISH", "planted", "decode/f32/64/8+wo/lds", T, nc)
    mk("wo-lds-TINY-f32-T600-nc10", "f32", "TINY", "range_last", "decode/f32/32/2+wo/lds", 600, 10)
    # fp8 weights: identity Wo, scale 1
    mk("wo-reg-FISH-fp8-T300-nc4", "fp8", "FISH", "planted", "decode/bf16/64/2/hs4+wo/reg", 300, 4)
    return out


def fused_cases():
    out = []
    for geom, wt in (("FISH", "bf16"), ("MID", "bf16"), ("TINY", "bf16"), ("TINY", "f32")):
        for T in range(1, 9):
            tier = ("planted", "random", "equal")[T % 3]
            out.append(Case(f"fused-{geom}-{wt}-T{T}", "fused", wt, geom, tier, f"wo/fused/{GEOMS[geom][2]}", [T], seed=T,
                            wo="random" if T == 5 else "identity"))
    return out


def rows_cases():
    out = []
    R = lambda cid, geom, tier, name, Ts, **kw: out.append(Case(cid, kw.pop("kind", "rows"), kw.pop("wt", "bf16"), geom, tier, name, Ts, seed=len(out), **kw))
    rngT = np.random.RandomState(7)
    ragged = lambda M: [1, 300, 128, 129, 16, 17, 64, 65, 127, 255, 256, 257][:M] + list(rngT.randint(1, 301, max(0, M - 12)))
    # one-node k_attn_rows: per-row positions (pos_step -1) and lock-step rows (pos_step 0)
    for M, name in ((3, "rows/bf16/64/2/hs4"), (4, "rows/bf16/64/2/hs4/remap"), (33, "rows/bf16/64/4/hs2"), (36, "rows/bf16/64/4/hs2/remap"),
                    (128, "rows/bf16/64/8")):
        R(f"rows-FISH-M{M}-ragged", "FISH", "planted", name, ragged(M), pos_step=-1)
    R("rows-FISH-M4-step0", "FISH", "range_last", "rows/bf16/64/2/hs4/remap", [257] * 4, pos_step=0)
    R("rows-FISH-M3-fp8", "FISH", "planted", "rows/bf16/64/2/hs4", [129, 1, 300], pos_step=-1, wt="fp8")
    for geom, d in (("MID", 64), ("TINY", 32)):
        R(f"rows-{geom}-M5-ragged", geom, "planted", f"rows/bf16/{d}/2", ragged(5), pos_step=-1)
        R(f"rows-{geom}-M3-step0", geom, "equal", f"rows/bf16/{d}/2", [130] * 3, pos_step=0)
        R(f"rows-{geom}-M4-random", geom, "random", f"rows/bf16/{d}/2", [300, 17, 128, 2], pos_step=-1)
    # chunked + combine: prefill rows of head_dim 32 / no_flash (pos_step 1, M = 129 crosses a chunk) and rows-are-sequences with chunked_attn
    R("chunked-TINY-M129", "TINY", "planted", "rows/chunked/32", [129], pos_step=1, nc_launch=2, n_chunks_max=3)
    R("chunked-MID-M129-noflash", "MID", "planted", "rows/chunked/64", [129], pos_step=1, nc_launch=2, n_chunks_max=2, no_flash=1)
    R("chunked-TINY-step0", "TINY", "range_first", "rows/chunked/32", [200] * 3, pos_step=0, nc_launch=2, n_chunks_max=4, chunked_attn=1)
    R("chunked-FISH-step0", "FISH", "planted", "rows/chunked/64", [129] * 2, pos_step=0, nc_launch=2, n_chunks_max=2, chunked_attn=1)
    # <= 8 tokens in one page
    for geom, d in (("FISH", 64), ("TINY", 32)):
        for ident in (0, 1):
            R(f"small-{geom}-ident{ident}", geom, "planted", f"small/{d}" + ("/ident" if ident else ""), list(range(1, 9)), pos_step=-1, kind="small",
              small_attn=1, identity_pages=ident)
        R(f"small-{geom}-step0", geom, "random", f"small/{d}", [5] * 3, pos_step=0, kind="small", small_attn=1)
    # ... with q / k / v of the row's own token from the qkv table (pos 0..7), appended by the node itself
    R("tbl-FISH-pos0-7", "FISH", "random", "small_tbl/64", list(range(1, 9)), pos_step=-1, kind="tbl", small_attn=1)
    R("tbl-FISH-ident", "FISH", "random", "small_tbl/64", [8, 1, 4, 5], pos_step=-1, kind="tbl", small_attn=1, identity_pages=1)
    R("tbl-MID-step0", "MID", "random", "small_tbl/64", [3] * 5, pos_step=0, kind="tbl", small_attn=1)
    # causal MFMA prefill: one sequence, and a group pass
    for pos0 in (0, 5, 64, 130):
        for M in (2, 15, 16, 17, 65):
            R(f"prefill-MID-pos{pos0}-M{M}", "MID", "planted", "prefill_mfma/seq", [M], pos0=pos0, kind="prefill", pos_step=1)
    R("prefill-MID-pos64-M16-random", "MID", "random", "prefill_mfma/seq", [16], pos0=64, kind="prefill", pos_step=1)
    R("prefill-FISH-pos5-M17", "FISH", "planted", "prefill_mfma/seq", [17], pos0=5, kind="prefill", pos_step=1)
    R("prefill-FISH-pos130-M65-range", "FISH", "range_first", "prefill_mfma/seq", [65], pos0=130, kind="prefill", pos_step=1)
    R("prefill-group-MID", "MID", "planted", "prefill_mfma/group", [], kind="group", pos_step=1, seq_rows=17, seq_pos=[0, 70, 130], pt_extra=3)
    R("prefill-group-FISH", "FISH", "random", "prefill_mfma/group", [], kind="group", pos_step=1, seq_rows=17, seq_pos=[64, 0, 5], pt_extra=2)
    return out


# every plan name lm_attn.hip can produce with the default environment -> the kernel instantiation behind it.  (k_attn_decode<.., 64, 4> and
# <bf16, 64, 1> are reached only with FISHRT_ATTN_HSPLIT = 2 / 8, k_attn_decode<float, 64, 4> by nothing: dispatch_attn instantiates them.)
PLAN_TABLE = {
    "decode/f32/32/2": "k_attn_decode<float,32,2>", "decode/bf16/32/2": "k_attn_decode<bf16,32,2>", "decode/bf16/64/2": "k_attn_decode<bf16,64,2>",
    "decode/bf16/64/2/hs4": "k_attn_decode<bf16,64,2> hsplit 4", "decode/f32/64/8": "k_attn_decode<float,64,8>",
    "decode/part/tpb2": "k_attn_rows<bf16,64,2,true> tpb 2", "decode/part/tpb4": "k_attn_rows<bf16,64,2,true> tpb 4",
    "decode/part/tpb8": "k_attn_rows<bf16,64,2,true> tpb 8",
    "rows/bf16/64/2/hs4": "k_attn_rows<bf16,64,2> hsplit 4", "rows/bf16/64/2/hs4/remap": "k_attn_rows<bf16,64,2> hsplit 4, XCD remap",
    "rows/bf16/64/4/hs2": "k_attn_rows<bf16,64,4> hsplit 2", "rows/bf16/64/4/hs2/remap": "k_attn_rows<bf16,64,4> hsplit 2, XCD remap",
    "rows/bf16/64/8": "k_attn_rows<bf16,64,8>", "rows/bf16/64/2": "k_attn_rows<bf16,64,2>", "rows/bf16/32/2": "k_attn_rows<bf16,32,2>",
    "rows/chunked/32": "k_attn_decode<bf16,32,2> on rows + k_attn_combine<32>",
    "rows/chunked/64": "k_attn_decode<bf16,64,2|8> on rows + k_attn_combine<64>",
    "small/64": "k_attn_small_rows<64>", "small/64/ident": "k_attn_small_rows<64> identity pages",
    "small/32": "k_attn_small_rows<32>", "small/32/ident": "k_attn_small_rows<32> identity pages", "small_tbl/64": "k_attn_small_rows_tbl<64>",
    "prefill_mfma/seq": "k_attn_prefill_mfma", "prefill_mfma/group": "k_attn_prefill_mfma group",
    "wo/fused/64": "k_wo<FUSED, 64>", "wo/fused/32": "k_wo<FUSED, 32>",
}


def all_cases():
    return decode_cases() + decode_wo_cases() + fused_cases() + rows_cases()


def rejected_cases():
    """(label, ffi case, text the error must contain): every one is refused by the hook's validation, before any device call"""
    out = []

    def bad(label, case, text, **fields):
        c = case.ffi_case()
        for f, val in fields.items():
            setattr(c, f, val)
        out.append((label, c, text))
    dec = Case("rej-dec", "decode", "bf16", "FISH", "random", "", [130], nc_launch=2, n_chunks_max=2)
    t = dec.table.copy(); t[0, 1] = dec.n_pages
    bad("page id == n_pages", dec, "page id", page_table=t.ctypes.data_as(C.POINTER(C.c_int32))); out[-1][1]._keep.append(t)
    t2 = dec.table.copy(); t2[0, 0] = -1
    bad("page id < 0", dec, "page id", page_table=t2.ctypes.data_as(C.POINTER(C.c_int32))); out[-1][1]._keep.append(t2)
    bad("table shorter than the launched chunks", dec, "page-table slot", pt_len=3, nc_launch=2, pos=129)
    bad("T > pt_len * 64", dec, "page-table slot", pt_len=2)
    bad("launched chunks do not cover T", dec, "do not cover", nc_launch=1)
    bad("nc_launch > n_chunks_max", dec, "nc_launch", nc_launch=3)
    bad("n_chunks_max > 128", dec, "n_chunks_max", n_chunks_max=129)
    bad("H not a multiple of Hk", dec, "multiple of Hk", Hk=3)
    bad("unsupported geometry", dec, "head_dim", Dh=48, dim=16 * 48)
    bad("dim != H * Dh", dec, "dim must equal", dim=512)
    bad("decode with M = 2", dec, "M == 1", M=2)
    bad("negative position", dec, "position", pos=-1)
    bad("unknown op", dec, "unknown op", op=9)
    bad("unknown weight type", dec, "weight type", wt=5)
    bad("no pools", dec, "n_pages", n_pages=0)
    sm = Case("rej-small", "small", "bf16", "FISH", "random", "", [8, 3], pos_step=-1, small_attn=1)
    rp = np.asarray([8, 2], np.int32)
    bad("small_attn with T = 9", sm, "<= 8 tokens", row_pos=rp.ctypes.data_as(C.POINTER(C.c_int32))); out[-1][1]._keep.append(rp)
    tz = np.zeros_like(sm.table)
    bad("identity pages with more rows than pages", sm, "identity pages", identity_pages=1, n_pages=1, page_table=tz.ctypes.data_as(C.POINTER(C.c_int32)))
    out[-1][1]._keep.append(tz)
    bad("rows with M = 0", sm, "1 <= M", M=0)
    bad("rows with f32 weights", sm, "bf16 or fp8", wt=0)
    fu = Case("rej-fused", "fused", "bf16", "FISH", "random", "", [8])
    bad("fused_T = 9", fu, "fused_T", fused_T=9)
    bad("fused wo without Wo", fu, "wo and x", wo=None)
    tb = Case("rej-tbl", "tbl", "bf16", "FISH", "random", "", [2, 3], pos_step=-1, small_attn=1)
    cd = np.asarray([1, 12], np.uint32)
    bad("code outside the table", tb, "code", codes=cd.ctypes.data_as(C.POINTER(C.c_uint32))); out[-1][1]._keep.append(cd)
    bad("RoPE row outside the tables", tb, "RoPE row", rope_off=14)
    tt = tb.table.copy(); tt[1, 0] = tt[0, 0]
    bad("two rows append to one page", tb, "same page", page_table=tt.ctypes.data_as(C.POINTER(C.c_int32))); out[-1][1]._keep.append(tt)
    ch = Case("rej-chunked", "rows", "bf16", "TINY", "random", "", [129], pos_step=1, nc_launch=2, n_chunks_max=2)
    bad("more rows than the partials hold", ch, "partials buffer", part_rows=100)
    gr = Case("rej-group", "group", "bf16", "MID", "random", "", [], pos_step=1, seq_rows=17, seq_pos=[0, 70], pt_extra=1)
    bad("group prefill with a ragged last sequence", gr, "multiple of seq_rows", M=33)
    bad("group prefill past the table", gr, "page-table slot", pt_len=1)
    return out


def call_rejected(c):
    """-> (status, message) of one call that must be refused"""
    from fishrt import _ffi
    out = np.zeros(1 << 16, F32)
    name = C.create_string_buffer(96)
    n_out, ok = C.c_size_t(0), C.c_int(0)
    rc = _ffi.lib().fs_selftest_attn(0, C.byref(c), out.ctypes.data_as(C.POINTER(C.c_float)), out.size, C.byref(n_out), None, None, name, 96, C.byref(ok))
    return rc, _ffi.lib().fs_last_error().decode()
