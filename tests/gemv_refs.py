"""Float64 definitions of what the batch-1 node kernels of csrc/lm_kernels.hip compute (k_qkv, k_ffn_up, k_ffn_down, k_head, the GEMV body of
k_wo, k_embed, k_fast_embed), the case table of the per-launch tests, the error bounds, and the ctypes wrapper of fs_selftest_gemv.  Shared by
test_gemv_ref_cpu.py (CPU: pins these definitions, plans every case, proves the teeth) and test_gemv_paths_gpu.py (GPU).

Definitions.  RMSNorm: xn = x / sqrt(mean(x^2) + eps) g.  GEMV: y[r] = s[r] sum_k W[r, k] xn[k] (s = 1 without fp8).  QKV: interleaved RoPE of
the q and k pairs (2j, 2j + 1) of a head with the factors of row pos + rope_off, q to f32, k and v rounded once to KVT<WT> (bf16 for bf16 and
fp8 weights, f32 for f32) and stored at ((page_table[pos >> 6] Hk + g) 64 + (pos & 63)) Dh + d.  FFN up: silu(a) b on the interleaved rows
(2r, 2r + 1).  FFN down and the wo body: x + s sum_k (no norm).  Head: rows [0, n_rows).  Embed: tok_emb[t0] + sum_c mask cb_emb[c cb_size +
t_{c + 1}], mask = (sem_lo <= t0 <= sem_hi), summed in order with separately rounded f32 additions -- mirrored exactly.  Fast embed: a gather.

Tier A -- exact, zero tolerance.  W in {0, +-1/2, +-1}; fp8 scales 2^((5 r mod 8) - 4): powers of two, distinct within any 8 consecutive rows
(so between the rows of every pair), and at most 2^7 apart, which keeps a RoPE pair's sum inside 24 bits; g and the RoPE factors in {0, +-1/2,
+-1}.  x has K / 4 entries +-2^j, K / 8 entries +-2^(j + 1) and zeros elsewhere, eps = 4^j / 4: sum x^2 is a sum of multiples of 4^j (exact in
any order), mean(x^2) = 3/4 4^j, mean + eps = 4^j, d = 2^j, so xn is in {0, +-1/2, +-1, +-2} exactly.  The inputs of the two GEMVs without a
norm (down, wo) are in that set directly; residuals lie on the grid 2^-7 with |.| <= 4.  Every product w xn is then a multiple of G = 1/4
and S = sum_k |w xn| <= 2 K <= 2^13 < 2^24 G: every partial sum in any order (lane chains, the DPP tree, the KS slices of k_ffn_down) is an
f32 value.  What follows are single operations on exact values -- a power-of-two scale, one RoPE fma pair, one residual addition -- exact
iff the result is an f32 value, which check_tier_a() asserts on the reference itself, per case, together with the grids and the S bound.
The f32 outputs then equal the float64 reference, the bf16 cache rows equal it rounded once (RNE).  SwiGLU outputs are not exact (the device
exp): they are held to the Tier B allowance with exact a and b.

Tier B -- derived bound, normal data: W ~ N(0, 1 / K) in the weight type (fp8: e4m3fn values with non-power-of-two row scales spread over
[2^-6, 2^3]), x ~ N(0, 1) times 1e-3, 1 or 30, one case per norm op with an all-zero x (d = sqrt(eps)), eps = 1e-5.  u = 2^-23 (one f32
rounding, taken at twice the unit roundoff).  |y - ref| <= (K + c) u S, S = |s| sum_k |w xn|:  K stands for the fma chain (a lane's chain is
only NX = ceil(K / (64 EPL)) EPL long; K is the bound of any summation order), and c counts what else lies on the path:
  7   the wave reduction: four DPP additions and the three additions of the four row sums
  1   the multiplication by the row scale
  (NX + 9) / 4 + 2, rounded up: the relative error of xn[k] in units of u, from the NX fmas + 7 additions of sum x^2, / K, + eps (NX + 9
      roundings, in half units of u, halved again by the square root), the square root, x / d and the multiplication by g (half a unit each,
      counted whole)  -- norm ops only
  KS  k_ffn_down: the KS - 1 additions of the wave slices, and the product t sc fused or not into the residual addition
Epilogue terms, the ones gemm_refs states: RoPE a c - b s: the operands' bounds through |c|, |s| plus 2 u (|a c| + |b s|); residual: one
addition, u (|x0| + |s sum|); bf16 cache rows: half an ulp of 8 significant bits, 2^-8 (|v| + t).  The only device-function allowance is
a / (1 + __expf(-a)) of k_ffn_up: gemm_refs.SILU_C_BOUND (|a| + 1) 2^-24 |v| + 2 u |v| + 2^-120, and the whole |v| where a < -87 (e^-a at the
edge of the f32 range: the quotient becomes -0) -- the row path's constant and range rule, nothing fitted here.  Tier B up cases plant rows
with a near +90, -90 and -87.3.

Tier C -- bit identity the code promises: cache_resident true == false; the state position source == the static one at the same position;
HEAD with n_rows = 2037 == the first 2037 rows of n_rows = 2040; QKV leaves every pool element outside the 2 Hk Dh written ones bit-identical
(asserted in every QKV comparison: the reference pools carry tolerance 0 there).

Shapes: every K in {128, 256, 1024, 4096} a launcher accepts, for f32, bf16 and fp8 (k_wo: dim <= 1024).  A dim = 4096 QKV matrix has at least
(H + 2) Dh x 4096 > 16 M elements, over the 8 M the other cases keep to: one geometry (H 64, Hk 2, Dh 64) per weight type is run all the same.

Worst |err| / tol on an MI355X over all 137 cases (profiles/gemv_paths_parity.txt; f32 / bf16 / fp8 weights): qkv q 0.0016 / 0.0017 / 0.0028,
cache rows 0.0021 (f32 KV) and 0.913 / 0.904 (bf16 KV: a half-ulp bound of the format, reached by construction); up 0.119 / 0.160 / 0.228
(the device-function allowance); down 0.0009 / 0.0028 / 0.0019; head 0.0014 / 0.0005 / 0.0037; wo body 0.0023 / 0.0029 / 0.0064; embed and
fast embed equal; every Tier A comparison exact.  No ratio above 1: no kernel had to change.

Teeth (test_gemv_ref_cpu): each mutation of MUTATIONS must move every applicable Tier A case by at least one grid step (2^-7, the coarsest
grid any exact output lies on) and every applicable Tier B case by 10 x the moved element's bound.  What a mutation cannot apply to is listed
in WAIVED, by (mutation, reason), with the number of cases; the CPU test recomputes that table."""
import ctypes as C
import functools
import zlib

import numpy as np

from attn_refs import GEOMS as ATTN_GEOMS
from gemm_refs import SILU_C_BOUND, bf16_rne, e4m3_values, rope_i, silu64, e4m3_nearest, EXP_OVERFLOW_A, ABS_FLOOR

F32, F64 = np.float32, np.float64
U = 2.0 ** -23
KV_PAGE = 64
GRID_A = 2.0 ** -7
EPS_B = 1e-5
WTS = ("f32", "bf16", "fp8")
EPL = {"f32": 4, "bf16": 8, "fp8": 16}
GEOMS = dict(ATTN_GEOMS, BIG=(64, 2, 64))  # (H, Hk, Dh); BIG: the one dim = 4096 geometry (module docstring)
OPS = ("qkv", "up", "down", "head", "wo", "embed", "fast_embed")
NORM_OPS = ("qkv", "up", "head")
FLAG_OPS = ("qkv", "wo", "up", "down")  # the launchers with a cache_resident flag
ROW_WAVES = {"qkv": 2, "wo": 4, "up": 4, "head": 4}
DOWN_KS = 4
SYM = np.float32([0, 0.5, -0.5, 1, -1])


def kv_round(x, wt):
    """one rounding to KVT<WT>: bf16 for bf16 and fp8 weights, f32 for f32"""
    x = np.asarray(x, F64).astype(F32)
    return (x if wt == "f32" else bf16_rne(x)).astype(F64)


def to_wt(x, wt):
    """nearest value of the weight type, as f32"""
    x = np.asarray(x, F32)
    return x if wt == "f32" else (bf16_rne(x) if wt == "bf16" else e4m3_nearest(x))


def nx_of(K, wt):
    ch = 64 * EPL[wt]
    return -(-K // ch) * EPL[wt]


def c_ops(op, K, wt):
    """the c of (K + c) u S: module docstring"""
    c = 7 + 1
    if op in NORM_OPS:
        c += int(np.ceil((nx_of(K, wt) + 9) / 4 + 2))
    if op == "down":
        c += DOWN_KS
    return c


# ---------------------------------------------------------------------------------------------------------------------------- cases
class Case:
    """One fs_selftest_gemv call.  op: one of OPS; wt: 'f32' | 'bf16' | 'fp8'; tier 'A' | 'B'."""

    def __init__(self, cid, op, wt, tier, K=0, rows=0, geom=None, resident=False, xs=1.0, **kw):
        self.id, self.op, self.wt, self.tier = cid, op, wt, tier
        self.K, self.rows, self.geom, self.resident, self.xs, self.kw = K, rows, geom, bool(resident), xs, kw
        self.fp8 = wt == "fp8"
        self.kvt = "f32" if wt == "f32" else "bf16"
        if geom:
            self.H, self.Hk, self.Dh = GEOMS[geom]
            self.K = self.H * self.Dh
            self.qdim, self.kdim = self.H * self.Dh, self.Hk * self.Dh
            self.rows = (self.H + 2 * self.Hk) * self.Dh if op == "qkv" else self.K
        self.w_rows = 2 * self.rows if op == "up" else self.rows   # up: rows = inter
        self.pos, self.rope_off, self.use_state = kw.get("pos", 0), kw.get("rope_off", 0), kw.get("use_state", True)
        self.eps = EPS_B
        self._built = False

    def __repr__(self):
        return self.id

    @property
    def expect(self):
        """the plan name and grid this call must have: the launchers' dispatch written out"""
        if self.op in ("embed", "fast_embed"):
            return f"{self.op}/{self.kvt}", (1 if self.op == "embed" else self.kw["n_ids"], 1, 1)
        pol = "res" if self.resident else "nt"
        if self.op == "down":
            return f"down/{self.wt}/K{self.K}/ks{DOWN_KS}/{pol}", (self.rows, 1, 1)
        w = ROW_WAVES[self.op]
        grid = (-(-self.rows // w), 1, 1)
        if self.op == "head":
            return f"head/{self.wt}/K{self.K}/w{w}", grid
        if self.op == "wo":
            return f"wo/{self.wt}/K{self.K}/w{w}/dh{self.Dh}/{pol}", grid
        return f"{self.op}/{self.wt}/K{self.K}/w{w}/{pol}", grid

    @property
    def n_weights(self):
        return self.w_rows * self.K

    # ---- inputs, deterministic per id
    def build(self):
        if self._built:
            return self
        self._built = True
        rng = np.random.RandomState(zlib.crc32(self.id.encode()) & 0x7FFFFFFF)
        if self.op in ("embed", "fast_embed"):
            return self._build_embed(rng)
        A = self.tier == "A"
        K, N = self.K, self.w_rows
        norm = self.op in NORM_OPS
        if A:
            j = int(rng.randint(-3, 3))
            if norm:
                x = np.zeros(K)
                idx = rng.permutation(K)
                x[idx[:K // 4]] = 2.0 ** j
                x[idx[K // 4:K // 4 + K // 8]] = 2.0 ** (j + 1)
                self.x = (x * rng.choice([-1.0, 1.0], K)).astype(F32)
                self.eps = float(4.0 ** j / 4)
                self.g = rng.choice(SYM, K, p=[0.1, 0.2, 0.2, 0.25, 0.25]).astype(F32)
            else:
                self.x = rng.choice(np.float32([0, 0.5, -0.5, 1, -1, 2, -2]), K).astype(F32)
            self.w = rng.choice(SYM, (N, K)).astype(F32)
            self.wscale = (2.0 ** ((5 * np.arange(N)) % 8 - 4)).astype(F32)
            self.y0 = (rng.randint(-512, 513, self.rows) / 128.0).astype(F32)
        else:
            self.x = (rng.randn(K) * self.xs).astype(F32)
            self.g = (1.0 + 0.1 * rng.randn(K)).astype(F32)
            if self.fp8:
                self.w = e4m3_nearest(rng.randn(N, K) * (4.0 / np.sqrt(K)))
                self.wscale = (2.0 ** rng.uniform(-6.0, 3.0, N)).astype(F32)
                self.wscale[:2] = np.float32([2.0 ** -6 * 1.37, 2.0 ** 3 * 0.77])[:N]  # both ends of the range, not powers of two
            else:
                self.w = to_wt(rng.randn(N, K) / np.sqrt(K), self.wt)
            self.y0 = (rng.randn(self.rows) * max(self.xs, 1e-3)).astype(F32)  # (a residual stream of the update's own magnitude)
            if self.op == "up" and self.xs > 0 and self.rows >= 6:
                self._plant_silu_rows()
        if not self.fp8:
            self.wscale = None
        if not norm:
            self.g = None
        if self.op == "qkv":
            self._build_qkv(rng, A)
        return self

    def xn(self, eps=None):
        """the GEMV input in float64: RMSNorm(x) for the norm ops, x itself otherwise"""
        x = self.x.astype(F64)
        if self.op not in NORM_OPS:
            return x
        eps = self.eps if eps is None else eps
        with np.errstate(all="ignore"):
            return x / np.sqrt((x * x).mean() + eps) * self.g.astype(F64)

    def _plant_silu_rows(self):
        """weight rows aimed at chosen dot products (the values stay in the weight type): w1 rows 1, 2, 3 at a = +90, -90, -87.3, the edges of
        the device exp's range; pair 0 at (a, b) = (1.5, -3), where silu is far from linear and both S equal |a|, |b| -- the one pair whose
        output moves by 10 bounds at every depth when its two scales are swapped (silu(a) b is invariant under the swap where silu is linear)"""
        xn = self.xn()
        for row, t in ((2, 90.0), (4, -90.0), (6, -87.3), (0, 1.5), (1, -3.0)):
            v = t * xn / (xn @ xn)
            if self.fp8:
                sc = np.float32(np.abs(v).max() / 400.0)
                self.wscale[row] = sc
                self.w[row] = e4m3_nearest(v / sc)
            else:
                self.w[row] = to_wt(v, self.wt)

    def _build_qkv(self, rng, A):
        half = self.Dh // 2
        self.pt_len = self.pos // KV_PAGE + 1
        self.n_pages = self.pt_len + 2
        self.table = (np.arange(self.pt_len) + 1 + (rng.randint(2))).astype(np.int32)  # never the identity
        self.rope_rows = self.pos + self.rope_off + 2
        if A:
            self.cos_t = rng.choice(SYM, (self.rope_rows, half)).astype(F32)
            self.sin_t = rng.choice(SYM, (self.rope_rows, half)).astype(F32)
        else:
            th = np.arange(self.rope_rows)[:, None] * (1e4 ** (-np.arange(half) / half))[None, :]
            self.cos_t, self.sin_t = np.cos(th).astype(F32), np.sin(th).astype(F32)
        shape = (self.n_pages, self.Hk, KV_PAGE, self.Dh)
        self.k0 = to_wt(rng.randn(*shape) * 100, self.kvt)  # stale rows: must come back untouched
        self.v0 = to_wt(rng.randn(*shape) * 100, self.kvt)

    def _build_embed(self, rng):
        kw = self.kw
        self.dim, self.tok_rows = kw["dim"], kw.get("tok_rows", 40)
        self.tok = to_wt(rng.randn(self.tok_rows, self.dim), self.kvt)
        if self.op == "fast_embed":
            self.ids = rng.randint(0, self.tok_rows, kw["n_ids"]).astype(np.uint32)
            self.ids[0], self.ids[-1] = self.tok_rows - 1, 0
            return self
        self.n_cb, self.cb_size = kw.get("n_cb", 8), kw.get("cb_size", 11)
        self.cb = to_wt(rng.randn(self.n_cb * self.cb_size, self.dim), self.kvt)
        self.sem_lo, self.sem_hi = kw.get("sem_lo", 10), kw.get("sem_hi", 30)
        self.prompt = kw["source"] == "prompt"
        self.prompt_L, self.step = (kw.get("prompt_L", 7), kw.get("step", 3)) if self.prompt else (0, 0)
        if self.prompt:
            toks = rng.randint(0, self.cb_size, (self.n_cb + 1, self.prompt_L)).astype(np.uint32)
            toks[0] = rng.randint(0, self.tok_rows, self.prompt_L)
            for c in range(1, self.n_cb + 1):  # the neighbouring column holds another code in every row
                toks[c, (self.step + 1) % self.prompt_L] = (toks[c, self.step] + 1 + c % 3) % self.cb_size
            toks[0, self.step] = kw["t0"]
            self.tokens = toks.reshape(-1)
        else:
            toks = rng.randint(0, self.cb_size, self.n_cb + 1).astype(np.uint32)
            toks[0] = kw["t0"]
            self.tokens = toks
        return self

    # ---- the call
    def ffi_case(self, plan_only=0):
        from fishrt import _ffi
        self.build()
        c = _ffi.GemvCase()
        keep = []

        def ptr(a, ct=C.c_float, dt=F32):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dt)
            keep.append(a)
            return a.ctypes.data_as(C.POINTER(ct))
        c.op, c.wt, c.plan_only, c.cache_resident = _ffi.GEMV_OPS[{"qkv": "QKV", "up": "FFN_UP", "down": "FFN_DOWN", "head": "HEAD", "wo": "WO_BODY",
                                                                   "embed": "EMBED", "fast_embed": "FAST_EMBED"}[self.op]], _ffi.GEMV_WT[self.wt], plan_only, int(self.resident)
        c.eps = self.eps
        if self.op in ("embed", "fast_embed"):
            c.dim, c.tok_rows, c.tok_emb = self.dim, self.tok_rows, ptr(self.tok)
            if self.op == "fast_embed":
                c.n_ids, c.ids = len(self.ids), ptr(self.ids, C.c_uint32, np.uint32)
            else:
                c.n_cb, c.cb_size, c.cb_emb, c.sem_lo, c.sem_hi = self.n_cb, self.cb_size, ptr(self.cb), self.sem_lo, self.sem_hi
                c.use_prompt, c.prompt_L, c.step = int(self.prompt), self.prompt_L, self.step
                c.n_tokens, c.tokens = len(self.tokens), ptr(self.tokens, C.c_uint32, np.uint32)
            c._keep = keep
            return c
        c.x, c.norm_w, c.w, c.wscale = ptr(self.x), ptr(self.g), ptr(self.w), ptr(self.wscale)
        if self.op in ("down", "wo"):
            c.y = ptr(self.y0)
        if self.op == "down":
            c.dim, c.inter = self.rows, self.K
        elif self.op == "up":
            c.dim, c.inter = self.K, self.rows
        else:
            c.dim, c.n_rows = self.K, self.rows
        if self.geom:
            c.H, c.Hk, c.Dh = self.H, self.Hk, self.Dh
        if self.op == "qkv":
            c.pos, c.rope_off, c.use_state = self.pos, self.rope_off, int(self.use_state)
            c.n_pages, c.pt_len, c.rope_rows = self.n_pages, self.pt_len, self.rope_rows
            c.cos_t, c.sin_t, c.k, c.v = ptr(self.cos_t), ptr(self.sin_t), ptr(self.k0), ptr(self.v0)
            c.page_table = ptr(self.table, C.c_int32, np.int32)
        c._keep = keep
        return c

    def _call(self, c, o):
        from fishrt import _ffi
        name = C.create_string_buffer(96)
        o.variant, o.variant_cap = C.cast(name, C.c_char_p), 96
        rc = _ffi.lib().fs_selftest_gemv(0, C.byref(c), C.byref(o))
        return rc, name

    def plan(self):
        """-> (plan name, grid) by validation alone (plan_only: no device)"""
        from fishrt import _ffi
        o = _ffi.GemvOut()
        rc, name = self._call(self.ffi_case(plan_only=1), o)
        _ffi.check(rc)
        return name.value.decode(), tuple(o.grid), o

    def run(self):
        """-> dict: name, grid, guard_ok, Y and (QKV) the pools K, V after the call"""
        from fishrt import _ffi
        _, _, probe = self.plan()
        o = _ffi.GemvOut()
        fp = C.POINTER(C.c_float)
        y = np.zeros(probe.n_y, F32)
        o.y, o.y_cap = y.ctypes.data_as(fp), y.size
        ka = va = None
        if self.op == "qkv":
            ka, va = np.zeros(self.k0.shape, F32), np.zeros(self.v0.shape, F32)
            o.k, o.v, o.pool_cap = ka.ctypes.data_as(fp), va.ctypes.data_as(fp), ka.size
        rc, name = self._call(self.ffi_case(), o)
        _ffi.check(rc)
        if self.op == "fast_embed":
            y = y.reshape(len(self.ids), self.dim)
        return dict(name=name.value.decode(), grid=tuple(o.grid), guard_ok=bool(o.guard_ok), Y=y, K=ka, V=va)


# ---------------------------------------------------------------------------------------------------------------------------- the reference
def _embed_reference(case, mut):
    if case.op == "fast_embed":
        y = case.tok.astype(F64)[case.ids.astype(int)]
        return {"Y": (y, np.zeros_like(y))}
    stride = case.prompt_L if case.prompt else 1
    base = case.step if case.prompt else 0
    if mut == "embed_stride1":
        stride = 1
    t = case.tokens.astype(int)
    t0 = t[base]
    hi_ok = t0 < case.sem_hi if mut == "embed_hi_excl" else t0 <= case.sem_hi
    m = np.float32(1.0 if (t0 >= case.sem_lo and hi_ok) else 0.0)
    acc = np.float32(0.0) + case.tok[t0]
    for c in range(case.n_cb):  # k_embed's own order, one separately rounded f32 addition per codebook: mirrored exactly
        code = t[base + (c + 1) * stride] % case.cb_size
        acc = (acc + (case.cb[c * case.cb_size + code] * m).astype(F32)).astype(F32)
    y = acc.astype(F64)
    return {"Y": (y, np.zeros_like(y))}


def reference(case, mut=None):
    """-> dict output name -> (ref, tol): float64 arrays in the hook's output shapes; tol == 0 means equality with ref (already rounded once to
    the output format).  mut: one of MUTATIONS."""
    case.build()
    if case.op in ("embed", "fast_embed"):
        return _embed_reference(case, mut)
    A = case.tier == "A"
    op, K, wt = case.op, case.K, case.wt
    xn = case.xn(0.0 if mut == "eps_drop" else None)
    W = case.w.astype(F64)
    sc = case.wscale.astype(F64) if case.fp8 else np.ones(case.w_rows)
    if mut == "scale_next":      # the scale of the neighbouring row
        sc = np.roll(sc, -1)
    if mut == "s13_swap":        # the scales of w1[r] and w3[r] swapped
        sc = sc.reshape(-1, 2)[:, ::-1].reshape(-1)
    if mut == "down_slices":     # wave w's weight slice against wave w + 1's activation slice
        xn = np.roll(xn.reshape(DOWN_KS, -1), -1, axis=0).reshape(-1)
    with np.errstate(all="ignore"):
        acc = (W @ xn) * sc
        S = (np.abs(W) @ np.abs(np.nan_to_num(xn))) * np.abs(sc)
    tol = np.zeros_like(S) if A else (K + c_ops(op, K, wt)) * U * S
    if op == "head":
        return {"Y": (acc, tol)}
    if op in ("down", "wo"):
        y0 = np.zeros(case.rows) if mut == "resid_missing" else case.y0.astype(F64)
        return {"Y": (y0 + acc, tol if A else tol + U * (np.abs(y0) + np.abs(acc)))}
    if op == "up":
        a, b, ta, tb = acc[0::2], acc[1::2], tol[0::2], tol[1::2]
        v = silu64(a) * b
        tv = 1.1 * ta * np.abs(b) + np.abs(silu64(a)) * tb + (SILU_C_BOUND * (np.abs(a) + 1) * 2.0 ** -24 + 2 * U) * np.abs(v) + ABS_FLOOR
        tv = tv + np.where(a < EXP_OVERFLOW_A, np.abs(v), 0.0)  # e^-a beyond the f32 range: the device's quotient is -0
        return {"Y": (v, tv), "_ab": (a, b)}
    return _reference_qkv(case, acc, tol, mut)


def _reference_qkv(case, acc, tol, mut):
    A = case.tier == "A"
    Dh, half, qd, kd, Hk = case.Dh, case.Dh // 2, case.qdim, case.kdim, case.Hk
    rpos = case.pos if mut == "rope_no_off" else case.pos + case.rope_off
    pair = np.arange((qd + kd) // 2)
    j = pair if mut == "rope_pair_row" else pair % half          # pair index inside the head: (row % Dh) / 2
    flat = (rpos * half + j) % case.cos_t.size                   # (the mutated index runs on into the following rows of the table)
    cs, sn = case.cos_t.astype(F64).reshape(-1)[flat], case.sin_t.astype(F64).reshape(-1)[flat]
    a, b = acc[:qd + kd:2], acc[1:qd + kd:2]
    ta, tb = tol[:qd + kd:2], tol[1:qd + kd:2]
    o0, o1 = rope_i(a, b, cs, sn)
    r0 = ta * np.abs(cs) + tb * np.abs(sn) + 2 * U * (np.abs(a * cs) + np.abs(b * sn))
    r1 = ta * np.abs(sn) + tb * np.abs(cs) + 2 * U * (np.abs(a * sn) + np.abs(b * cs))
    rot = np.stack([o0, o1], -1).reshape(-1)
    trot = np.zeros_like(rot) if A else np.stack([r0, r1], -1).reshape(-1)
    out = {"Y": (rot[:qd], trot[:qd])}
    Kp, Vp = case.k0.astype(F64).copy(), case.v0.astype(F64).copy()
    TK, TV = np.zeros_like(Kp), np.zeros_like(Vp)

    def cache(val, t):
        if A:
            return kv_round(val, case.wt), np.zeros_like(val)
        return val, t + (2.0 ** -8 * (np.abs(val) + t) if case.kvt == "bf16" else 0.0)
    page = case.pos // KV_PAGE if mut == "pt_ignored" else int(case.table[case.pos // KV_PAGE])
    slot = (case.pos + {"kv_slot_m1": -1, "kv_slot_p1": 1}.get(mut, 0)) % KV_PAGE
    heads = (np.arange(Hk) + (1 if mut == "kv_head" else 0)) % Hk
    kk, tk = cache(rot[qd:], trot[qd:])
    vv, tv = cache(acc[qd + kd:], np.zeros(kd) if A else tol[qd + kd:])
    Kp[page, heads, slot], TK[page, heads, slot] = kk.reshape(Hk, Dh), tk.reshape(Hk, Dh)
    Vp[page, heads, slot], TV[page, heads, slot] = vv.reshape(Hk, Dh), tv.reshape(Hk, Dh)
    out["K"], out["V"] = (Kp, TK), (Vp, TV)
    return out


def check_tier_a(case):
    """the exactness arithmetic of the module docstring, per case: inputs on their grids, S below 2^24 grid steps, and every exact output of
    the reference an f32 value"""
    case.build()
    assert case.tier == "A"
    sym = lambda a: np.isin(np.asarray(a, F64), [0, 0.5, -0.5, 1, -1]).all()
    if case.op in ("embed", "fast_embed"):
        assert np.array_equal(to_wt(case.tok, case.kvt), case.tok) and (case.op == "fast_embed" or np.array_equal(to_wt(case.cb, case.kvt), case.cb))
        return
    assert sym(case.w) and case.K <= 4096
    xn = case.xn()
    if case.op in NORM_OPS:
        x = case.x.astype(F64)
        j = np.log2(case.eps * 4) / 2
        assert j == int(j) and case.eps > 0
        assert np.isin(np.abs(x), [0, 2.0 ** j, 2.0 ** (j + 1)]).all() and sym(case.g)
        assert (x * x).mean() + case.eps == 4.0 ** j      # an exact power of 4 with a non-zero eps
        assert np.sqrt((x * x).mean() + case.eps) == 2.0 ** j
    assert np.isin(np.abs(xn), [0, 0.5, 1, 2]).all()
    G = 0.25
    S = np.abs(case.w.astype(F64)) @ np.abs(xn)
    assert S.max() < 2 ** 24 * G, (case.id, float(S.max()))   # every partial sum in any order is a multiple of G below 2^24 G
    if case.fp8:
        e = np.log2(case.wscale.astype(F64))
        assert np.array_equal(e, np.round(e)) and (np.diff(e) != 0).all() and e.max() - e.min() <= 7
    if case.op in ("down", "wo"):
        assert np.array_equal(np.round(case.y0.astype(F64) * 128) / 128, case.y0.astype(F64)) and np.abs(case.y0).max() <= 4
    if case.op == "qkv":
        assert sym(case.cos_t) and sym(case.sin_t)
        assert np.array_equal(to_wt(case.k0, case.kvt), case.k0) and np.array_equal(to_wt(case.v0, case.kvt), case.v0)
    ref = reference(case)
    if case.op != "up":   # (SwiGLU: a and b are exact, the output is held to the device-function allowance)
        y = ref["Y"][0]
        assert np.array_equal(y.astype(F32).astype(F64), y), case.id
        assert (ref["Y"][1] == 0).all()
    else:
        a, b = ref["_ab"]
        assert np.array_equal(a.astype(F32).astype(F64), a) and np.array_equal(b.astype(F32).astype(F64), b)


# ---------------------------------------------------------------------------------------------------------------------------- the case table
POSITIONS = (0, 63, 64, 200)
XS = (1e-3, 1.0, 30.0)


@functools.lru_cache(maxsize=None)
def all_cases():
    cs = []
    add = lambda *a, **k: cs.append(Case(*a, **k))
    i = 0
    # QKV: TINY (K 128), MID (256), FISH (1024) x weight type x tier; positions, RoPE offsets, position sources and load policies cycle
    for geom in ("TINY", "MID", "FISH"):
        for wt in WTS:
            for tier in "AB":
                pos, ro, st, res = POSITIONS[i % 4], (0, 7)[(i // 2) % 2], bool((i // 3) % 2), bool((i // 4 + i) % 2)
                add(f"qkv-{geom}-{wt}-pos{pos}-ro{ro}-{'state' if st else 'static'}-{'res' if res else 'nt'}-{tier}", "qkv", wt, tier, geom=geom,
                    pos=pos, rope_off=ro, use_state=st, resident=res, xs=XS[i % 3])
                i += 1
    for n, wt in enumerate(WTS):  # dim = 4096 (module docstring: over the 8 M elements the other cases keep to)
        add(f"qkv-BIG-{wt}-pos64-ro7-{'AB'[n == 0]}", "qkv", wt, "AB"[n == 0], geom="BIG", pos=64, rope_off=7, use_state=n != 1, resident=n == 2, xs=1.0)
    add("qkv-MID-bf16-zero-x-B", "qkv", "bf16", "B", geom="MID", pos=63, rope_off=7, xs=0.0)
    # every other GEMV: K in {128, 256, 1024, 4096} x weight type x tier
    for K in (128, 256, 1024, 4096):
        for wt in WTS:
            for tier in "AB":
                res = bool((i // 2 + i) % 2)
                inter = (6, 130)[(i // 2) % 2]     # not multiples of the 4 rows of a block
                add(f"up-K{K}-{wt}-inter{inter}-{'res' if res else 'nt'}-{tier}", "up", wt, tier, K=K, rows=inter, resident=res, xs=XS[i % 3])
                dim = (5, 131)[(i // 2 + 1) % 2]
                add(f"down-K{K}-{wt}-dim{dim}-{'nt' if res else 'res'}-{tier}", "down", wt, tier, K=K, rows=dim, resident=not res, xs=XS[(i + 1) % 3])
                n = (1, 5, 2037)[(i + i // 6) % 3]
                add(f"head-K{K}-{wt}-n{n}-{tier}", "head", wt, tier, K=K, rows=n, xs=XS[(i + 2) % 3])
                i += 1
    for wt in WTS:   # n_rows = 2037 for every weight type (the Tier C pair 2037 / 2040 runs on these)
        add(f"head-K1024-{wt}-n2037-tail-B", "head", wt, "B", K=1024, rows=2037, xs=1.0)
    add("up-K256-fp8-zero-x-B", "up", "fp8", "B", K=256, rows=6, xs=0.0)
    add("head-K128-f32-zero-x-B", "head", "f32", "B", K=128, rows=5, xs=0.0)
    # the GEMV body of k_wo: dim <= 1024
    for geom in ("TINY", "MID", "FISH"):
        for wt in WTS:
            for tier in "AB":
                res = bool((i // 2) % 2)
                add(f"wo-{geom}-{wt}-{'res' if res else 'nt'}-{tier}", "wo", wt, tier, geom=geom, resident=res, xs=XS[i % 3])
                i += 1
    # k_embed: table type x token source x t0 at the edges of the mask range (sem_lo 10, sem_hi 30); dim 1000: four passes of the 256 threads
    for wt in ("bf16", "f32"):
        for source in ("prompt", "cur"):
            for t0 in (9, 10, 30, 31):
                add(f"embed-{wt}-{source}-t{t0}", "embed", wt, "A", source=source, t0=t0, dim=(128, 1000)[t0 % 2])
    add("embed-fp8-prompt-t30", "embed", "fp8", "A", source="prompt", t0=30, dim=256, prompt_L=5, step=4)
    for wt, n in (("bf16", 1), ("f32", 9), ("fp8", 3)):
        add(f"fast_embed-{wt}-n{n}", "fast_embed", wt, "A", n_ids=n, dim=(1000, 128, 1024)[n % 3])
    return tuple(cs)


# the ways these kernels go wrong (reference(case, mut)), the ops each is about ...
MUTATIONS = {
    "s13_swap": ("up",),                    # s_13 pair swapped: 2r against 2r + 1
    "eps_drop": NORM_OPS,                   # eps dropped from the RMSNorm
    "rope_pair_row": ("qkv",),              # RoPE pair index from the row instead of row % Dh
    "rope_no_off": ("qkv",),                # RoPE row pos instead of pos + rope_off
    "kv_slot_m1": ("qkv",),                 # KV slot pos - 1
    "kv_slot_p1": ("qkv",),                 # KV slot pos + 1
    "pt_ignored": ("qkv",),                 # page table ignored
    "kv_head": ("qkv",),                    # kv head index wrong
    "down_slices": ("down",),               # k_ffn_down's wave slices permuted
    "resid_missing": ("down", "wo"),        # residual missing
    "embed_hi_excl": ("embed",),            # upper embed bound exclusive
    "embed_stride1": ("embed",),            # embed stride 1 instead of prompt_L
    "scale_next": ("qkv", "up", "down", "head", "wo"),  # row scale of the neighbouring row
}


def waived(case, mut):
    """None where the mutation applies to the case; else the reason it cannot (the key of WAIVED)"""
    case.build()
    assert case.op in MUTATIONS[mut]
    if mut in ("s13_swap", "scale_next") and not case.fp8:
        return "no row scales without fp8"
    if case.op != "embed" and case.tier == "B" and case.xs == 0.0 and mut in ("s13_swap", "scale_next", "rope_pair_row", "rope_no_off", "kv_head"):
        return "all-zero x: every value is 0 whatever scales, rotates or permutes it"
    if mut == "scale_next" and case.w_rows == 1:
        return "one row: there is no neighbouring row"
    if mut == "eps_drop" and case.tier == "B" and case.xs >= 1.0:
        return "eps <= 1e-5 mean(x^2): below one rounding of the norm"
    if mut == "rope_no_off" and case.rope_off == 0:
        return "rope_off == 0"
    if mut == "embed_hi_excl" and case.tokens[case.step if case.prompt else 0] != case.sem_hi:
        return "t0 != sem_hi"
    if mut == "embed_stride1":
        if not case.prompt:
            return "cur source: the stride is 1"
        if not case.sem_lo <= case.tokens[case.step] <= case.sem_hi:
            return "mask 0: no code is read into the sum"
    return None


# ... and what each is waived for: (mutation, reason) -> number of cases (test_gemv_ref_cpu recomputes this table from the cases)
WAIVED = {
    ("s13_swap", "no row scales without fp8"): 16,
    ("s13_swap", "all-zero x: every value is 0 whatever scales, rotates or permutes it"): 1,
    ("scale_next", "no row scales without fp8"): 78,
    ("scale_next", "all-zero x: every value is 0 whatever scales, rotates or permutes it"): 1,
    ("scale_next", "one row: there is no neighbouring row"): 2,
    ("eps_drop", "eps <= 1e-5 mean(x^2): below one rounding of the norm"): 26,
    ("rope_no_off", "rope_off == 0"): 10,
    ("rope_no_off", "all-zero x: every value is 0 whatever scales, rotates or permutes it"): 1,
    ("rope_pair_row", "all-zero x: every value is 0 whatever scales, rotates or permutes it"): 1,
    ("kv_head", "all-zero x: every value is 0 whatever scales, rotates or permutes it"): 1,
    ("embed_hi_excl", "t0 != sem_hi"): 12,
    ("embed_stride1", "cur source: the stride is 1"): 8,
    ("embed_stride1", "mask 0: no code is read into the sum"): 4,
}


def rejected_cases():
    """(label, case, attribute overrides on the ffi struct, text of the validation message)"""
    q = lambda **k: Case("rej", "qkv", k.pop("wt", "bf16"), "A", geom="MID", pos=70, rope_off=1, **k)
    return [
        ("width", Case("rej", "head", "bf16", "A", K=128, rows=5), {"dim": 384}, "unsupported GEMV width"),
        ("width-down", Case("rej", "down", "f32", "A", K=128, rows=5), {"inter": 512}, "unsupported GEMV width"),
        ("width-qkv", q(), {"dim": 384, "H": 6}, "unsupported GEMV width"),
        ("dim", q(), {"H": 2}, "dim must equal H * Dh"),
        ("dim-wo", Case("rej", "wo", "bf16", "A", geom="MID"), {"dim": 128}, "dim must equal H * Dh"),
        ("odd-dh", q(), {"Dh": 63}, "head_dim must be even"),
        ("table", q(), {"pt_len": 1}, "page table does not cover pos"),
        ("fp8-scales", Case("rej", "up", "fp8", "A", K=128, rows=6), {"wscale": None}, "fp8 weights need their row scales"),
        ("page", q(), {"n_pages": 1}, "page id is outside the pool"),
        ("rope", q(), {"rope_rows": 71}, "RoPE row"),
        ("grid", Case("rej", "head", "bf16", "A", K=128, rows=5), {"_w": 1.0 + 2.0 ** -10}, "not a bf16 value"),
        ("wo-wide", Case("rej", "wo", "bf16", "A", geom="BIG"), {}, "wo: 1 <= Hk <= H <= 16"),
        ("code", Case("rej", "embed", "bf16", "A", source="cur", t0=10, dim=128), {"cb_size": 1}, "outside its codebook"),
    ]


def call_rejected(case, over):
    from fishrt import _ffi
    c = case.ffi_case()
    for k, v in over.items():
        if k == "_w":
            case.w[0, 0] = v
            c = case.ffi_case()
        elif v is None:
            setattr(c, k, C.POINTER(C.c_float)())
        else:
            setattr(c, k, v)
    o = _ffi.GemvOut()
    rc, _ = case._call(c, o)
    return rc, _ffi.lib().fs_last_error().decode()
