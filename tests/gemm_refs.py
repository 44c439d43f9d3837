"""Float64 definitions of what the row-path GEMM family of csrc/lm_gemm.hip computes (k_prep, k_gemm3, k_gemm_big, k_gemm_down and every
epilogue), the case table of the per-launch tests, the error bounds, and the ctypes wrapper of fs_selftest_gemm.  Shared by
test_gemm_ref_cpu.py (CPU: pins these definitions, plans every case, proves the teeth) and test_gemm_paths_gpu.py (GPU).

Operation: Y[m, n] = sum_k W[n, k] (hi + lo)[m, k], where hi = bf16_rne(x), lo = bf16_rne(x - hi) is the split every GEMM input goes through
(split_bf16, lm_dev.h); fp8 weights are e4m3fn values times one f32 scale per row, applied to the K-summed accumulator.  The epilogues:
STORE (one slab per K range), RESIDUAL (y += a), RESIDUAL_NORM (y += a; split(y g); per-(block, row) sum of squares), SWIGLU on interleaved
(w1, w3) rows (silu(a) b, split), QKV (interleaved RoPE of the q and k pairs, q to Y, k / v as bf16 into the paged cache, optionally the
one-token attention output o1), and the *_RMS forms that first divide by rms[m] = sqrt(sum_b ss[m, b] / K + eps).

Tier A -- exact, zero tolerance.  X lies on the grid 2^-10 with |X| <= 1: 11 significant bits, so hi + lo == X exactly, hi and lo are both
multiples of 2^-10, and lo != 0 for about half of the entries.  W is in {0, +-1/2, +-1} (exact in bf16 and e4m3), fp8 scales are powers of two, g and the
RoPE factors are in {0, +-1/2, +-1}, residuals lie on the grid 2^-11 with |.| <= 4, and the *_RMS partials make sum / K + eps an exact power
of 4.  Every product is then a multiple of G = 2^-11, and S = sum_k |w x| bounds every partial sum in any order; S < 2^24 G = 2^13 (K <= 4096)
means every partial sum is an integer multiple of G below 2^24 G, i.e. exact in f32 whatever the summation order and inside the MFMA.  The
epilogues then apply single operations to exact values (a power-of-two scale or rms, one RoPE fma pair, one residual addition), exact iff
the result is an f32 value.  check_tier_a() asserts the grids, the S bound and that last condition on the reference, per case.
The f32 outputs then equal the float64 reference, the bf16 outputs equal it rounded once (RNE), the hi / lo planes equal the mirrored split.
The sum-of-squares partials and the SwiGLU outputs are not exact (v^2 needs more than 24 bits; the device exp): they are held to bounds.

Tier B -- derived bound, normal data: W ~ N(0, 1/K) in the weight type, X ~ N(0, 1) times a per-row scale of 0.1, 1 or 30.  u = 2^-23 (one
f32 rounding, taken at twice the unit roundoff for the MFMA's internal accumulation).  With S = sum_k |w (hi + lo)| over the element's K
range and n = 2 K_range + 4 (+ 1 with an fp8 scale) f32 additions and multiplications on the path to it (both parts through the MFMA, the
quarter / half sums), |y - ref| <= n u S for the reference that sums w (hi + lo) in float64; against the UNSPLIT x the bound grows by
2^-17 S (the file header's claim: hi + lo = x to 2^-17 relative).  Epilogue terms, from their f32 operation counts:
  rms division   tot = nblk / 8 + 3 additions, / K, + eps, sqrtf, then one division: (nblk / 8 + 7) u |y|
  RoPE           a c - b s: two roundings, 2 u (|a c| + |b s|), and the operands' own bounds through |c|, |s|
  residual       one addition: u (|y0| + |a|)
  split output   hi + lo = v (1 + 2^-17): 2^-17 |v|; bf16 output (K / V rows): half an ulp of 8 significant bits, 2^-8 |v|
  ss partial     ROWS / 2 fmas + log2 adds of squares: (ROWS + 2) u sum v^2, and 2 |v| tol_v + tol_v^2 from the operands
  k_prep         slab sum: separately rounded f32 additions in slab order, mirrored exactly (no bound); norm: sum of squares over D in (D / 256 + 12) steps, / D, + eps, sqrtf, / d, * w: relative
                 ((D / 256 + 16) / 2 + 3) u on x / d * w, then the split
  k_gemm_down    ksplit additions of the partials and the residual: ksplit u (|y0| + S)
The only device-function allowance is a / (1 + __expf(-a)) in the two SwiGLU epilogues: SILU_C (|a| + 1) 2^-24 |v| with SILU_C measured on
Tier A inputs (a, b exact) against the float64 expression, as max over elements of (|hi + lo - ref| - 2^-8 |lo|) / ((|a| + 1) 2^-24 |ref|) --
2^-8 |lo| bounds the half ulp of the lo part, the only other rounding between v and the planes.  Asserted: 4 x the measured value (the ulp
error of __expf varies with its argument); SILU_C_MEASURED / SILU_C_BOUND below.  Range: an absolute 2^-120 is added wherever the device
function can flush a subnormal, and for a < -87 (e^-a at the edge of the f32 range or beyond: the quotient becomes -0) the whole |v| <
|a b| 2^-125.  Measured on an MI355X over the 16 Tier A SwiGLU cases: SILU_C = 1.588 (a = -0.0190, where (|a| + 1) 2^-24 is half an f32 ulp:
the quotient's and the product's own roundings are part of what is measured); asserted 6.352.
Worst |err| / tol on an MI355X over all cases (profiles/gemm_paths_parity.txt): f32 outputs of k_gemm3 0.0114 against the split operand and
0.0475 against the unsplit x, k_gemm_big 0.0005 / 0.0023, k_gemm_down's X 0.0029; ss partials 0.066 / 0.016 / 0.075; the bf16 cache rows
0.962 and the hi + lo planes 0.925 (both are half-ulp bounds of their format, reached by construction); k_prep with a norm 0.84; every
Tier A comparison exact.

Tier C -- bit identity the code promises: HALF at M = 16 == full at M = 17 on the 16 common rows; another gridDim.z (via N) gives the same
rows; the `pre` path of a first panel (RESIDUAL's residual slot; QKV / QKV_RMS's RoPE slot with lock-step rows, pos_step 0) == the same rows
computed in the block's later panel; k_gemm_big == k_gemm3 on Tier A.  (test_gemm_paths_gpu.)

Teeth (test_gemm_ref_cpu): the loose n u S of a deep Tier B case cannot see a lo-plane error (2^-9 relative of one operand against
2 K u sqrt(K) of all); the Tier A twin of every shape does, at one grid step.  Each mutation must move every applicable Tier A case by at
least one grid step and every applicable Tier B case by 10 x the element's bound -- except that the two lo-plane mutations are asked of
Tier B only at depth 128."""
import ctypes as C
import functools
import zlib

import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -23
KV_PAGE = 64
PF_M = 32
GRID_A = 2.0 ** -11
ABS_FLOOR = 2.0 ** -120
# measured on an MI355X by test_gemm_paths_gpu.test_swiglu_allowance (printed there, profiles/gemm_paths_parity.txt): see the module docstring
# 1.588 at a = -0.01904, b = 5.7729 (g3-SWIGLU_RMS-panels-N6400-A, row 49, column 2656), over the 16 Tier A SwiGLU cases
SILU_C_MEASURED = 1.588
SILU_C_BOUND = 4.0 * SILU_C_MEASURED
# a below this: e^-a is within a factor e^1.7 of FLT_MAX = e^88.72 or beyond it, 1 + __expf(-a) may be +inf and the quotient -0, where the
# true |v| = |a b| / (1 + e^-a) < |a b| 2^-125 is still a normal float: the whole value is allowed to be flushed there (f32 range, not a fit)
EXP_OVERFLOW_A = -87.0

EPI = {n: i for i, n in enumerate(("STORE", "RESIDUAL", "SWIGLU", "QKV", "RESIDUAL_NORM", "SWIGLU_RMS", "QKV_RMS", "STORE_RMS", "QKV_SEQ"))}
EPI_RT = {"STORE": 1, "RESIDUAL": 1, "SWIGLU": 2, "QKV": 1, "RESIDUAL_NORM": 1, "SWIGLU_RMS": 2, "QKV_RMS": 1, "STORE_RMS": 1, "QKV_SEQ": 1}
RMS_EPIS = ("SWIGLU_RMS", "QKV_RMS", "STORE_RMS")
QKV_EPIS = ("QKV", "QKV_RMS", "QKV_SEQ")
# k_gemm_big is instantiated for every epilogue launch_gemm3 is: the engine sends the first seven there; QKV_RMS and STORE_RMS (folded decode
# steps, M <= 32 in the engine) reach it through gemm_plan from 128 rows at depth 1024 all the same, so they are listed and run too
BIG_EPIS = ("STORE", "RESIDUAL", "SWIGLU", "QKV", "RESIDUAL_NORM", "SWIGLU_RMS", "QKV_SEQ", "QKV_RMS", "STORE_RMS")
GEOMS = {"MID": (4, 2, 64), "FISH": (16, 2, 64), "TINY": (4, 2, 32)}  # (H, Hk, Dh)


# ------------------------------------------------------------------------------------------------------------------------ number formats
def bf16_rne(x):
    """f32 -> nearest bf16 (ties to even), returned as f32"""
    b = np.ascontiguousarray(x, F32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) >> 16 << 16
    return (b & 0xFFFFFFFF).astype(np.uint32).view(F32).reshape(np.shape(x))


def split(x):
    """split_bf16 of lm_dev.h: hi = rne(x), lo = rne(x - hi), both f32"""
    x = np.ascontiguousarray(x, F32)
    hi = bf16_rne(x)
    return hi, bf16_rne(x - hi)


@functools.lru_cache(maxsize=None)
def e4m3_values():
    """the 254 finite values of OCP e4m3fn by byte (NaN bytes 0x7F / 0xFF left out), ascending and unique"""
    vals = []
    for b in range(256):
        if (b & 0x7F) == 0x7F:
            continue
        e, m = (b >> 3) & 15, b & 7
        v = m * 2.0 ** -9 if e == 0 else (1 + m / 8.0) * 2.0 ** (e - 7)
        vals.append(-v if b & 0x80 else v)
    return np.unique(np.asarray(vals, F64))


def e4m3_nearest(x):
    """nearest e4m3fn value (saturating); ties go to either neighbour -- only membership of the result matters here"""
    v = e4m3_values()
    x = np.clip(np.asarray(x, F64), v[0], v[-1])
    i = np.clip(np.searchsorted(v, x), 1, len(v) - 1)
    return np.where(np.abs(x - v[i - 1]) <= np.abs(v[i] - x), v[i - 1], v[i]).astype(F32)


def frag_off(m, k, part, K):
    """lm_dev.h frag_off: element (row m, depth k, part) of a fragment-major [rows][K] matrix, in bf16 elements"""
    m, k = np.asarray(m), np.asarray(k)
    p, mt, lr, kk, lq, e = m >> 5, (m >> 4) & 1, m & 15, k >> 5, (k >> 3) & 3, k & 7
    return (((((p * (K >> 5) + kk) * 2 + part) * 2 + mt) * 64 + (lq * 16 + lr)) * 8 + e)


def rope_i(a, b, cs, sn):
    return a * cs - b * sn, a * sn + b * cs


def silu64(a):
    a = np.asarray(a, F64)
    with np.errstate(over="ignore"):
        return a / (1.0 + np.exp(-a))


# ---------------------------------------------------------------------------------------------------------------------------- cases
class Case:
    """One fs_selftest_gemm call.  op: 'prep' | 'rows' | 'down'; tier 'A' | 'B'; expect: the plan name it must reach."""

    def __init__(self, cid, op, tier, expect, M, N=0, K=0, epi=None, fp8=False, ksplit=1, geom=None, ld=0, big_min_m=0, grid=None, **kw):
        self.id, self.op, self.tier, self.expect = cid, op, tier, expect
        self.M, self.N, self.K, self.epi, self.fp8, self.ksplit = M, N, K, epi, bool(fp8), ksplit
        self.geom, self.big_min_m, self.grid = geom, big_min_m, grid
        self.Mcap = -(-M // PF_M) * PF_M if op != "down" else PF_M
        self.kw = kw
        self.rt = EPI_RT.get(epi, 1)
        self.qkv = epi in QKV_EPIS
        self.rms = epi in RMS_EPIS
        if self.qkv:
            self.H, self.Hk, self.Dh = GEOMS[geom]
            self.qdim, self.kdim = self.H * self.Dh, self.Hk * self.Dh
            self.N = (self.H + 2 * self.Hk) * self.Dh
        self.ldy = ld or (self.qdim if self.qkv else self.N)
        self.D, self.S = kw.get("D", 0), kw.get("S", 0)
        self.norm, self.want_frag = kw.get("norm", False), kw.get("want_frag", True)
        self.n_launches = kw.get("n_launches", 1)
        self.o1 = kw.get("o1", False)
        self.eps = 0.0 if tier == "A" else 1e-5
        self._built = False

    def __repr__(self):
        return self.id

    # ---- inputs, deterministic per id
    def build(self):
        if self._built:
            return self
        self._built = True
        rng = np.random.RandomState(zlib.crc32(self.id.encode()) & 0x7FFFFFFF)
        A = self.tier == "A"
        M = self.M
        sym = np.float32([0, 0.5, -0.5, 1, -1])

        def acts(rows, cols):
            if A:
                return (rng.randint(-1024, 1025, (rows, cols)) / 1024.0).astype(F32)
            scale = np.float32([0.1, 1.0, 30.0])[np.arange(rows) % 3][:, None]
            return (rng.randn(rows, cols) * scale).astype(F32)

        def resid(rows, cols):
            return (rng.randint(-8192, 8193, (rows, cols)) / 2048.0).astype(F32) if A else rng.randn(rows, cols).astype(F32)

        def gains(n):
            return rng.choice(sym[1:], n).astype(F32) if A else (1.0 + 0.1 * rng.randn(n)).astype(F32)

        if self.op == "prep":
            D = self.D
            self.x = resid(M, D) if A else acts(M, D)
            self.p = np.stack([resid(M, D) for _ in range(self.S)]) if self.S else np.zeros((0, M, D), F32)
            self.norm_w = gains(D) if self.norm else None
            self.eps = 1e-5
            return self
        K, N = self.K, self.N
        self.x = acts(M, K)
        self.x2 = acts(M, K)
        if A:
            self.w = rng.choice(sym, (N, K), p=[0.2, 0.2, 0.2, 0.2, 0.2]).astype(F32)
            self.wscale = rng.choice(np.float32([0.5, 1, 2]), N).astype(F32)
        elif self.fp8:
            self.w = e4m3_nearest(rng.randn(N, K) * 8.0)
            self.wscale = ((0.5 + 1.5 * rng.rand(N)) / (8.0 * np.sqrt(K))).astype(F32)  # NOT the quantiser's amax / 448
        else:
            self.w = bf16_rne((rng.randn(N, K) / np.sqrt(K)).astype(F32))
            self.wscale = None
        if not self.fp8:
            self.wscale = None
        self.y0 = resid(M, self.ldy)
        self.g = gains(N)
        if self.rms or self.kw.get("nblk"):
            self.nblk = self.kw.get("nblk", 8)
            if A:  # sum / K + 0 = 4^j exactly: rms in {1/2, 1, 2}
                j = np.float64([0.25, 1.0, 4.0])[np.arange(M) % 3]
                self.ss = np.repeat((j * K / self.nblk)[:, None], self.nblk, 1).astype(F32)
            else:
                rs = np.float64([0.1, 1.0, 30.0])[np.arange(M) % 3] ** 2
                self.ss = (rs[:, None] * K / self.nblk * (0.5 + rng.rand(M, self.nblk))).astype(F32)
        if self.qkv:
            self._build_qkv(rng, A, sym)
        return self

    def _build_qkv(self, rng, A, sym):
        kw, M, half = self.kw, self.M, self.Dh // 2
        self.pos_step, self.seq_rows = kw.get("pos_step", 1), kw.get("seq_rows", 0)
        self.pos, self.rope_off = kw.get("pos", 0), kw.get("rope_off", 0)
        self.row_pos, self.seq_pos = kw.get("row_pos"), kw.get("seq_pos")
        n_seq = M // self.seq_rows if self.seq_rows else (M if self.pos_step <= 0 else 1)
        # positions as gemm_epilogue derives them
        sq = np.arange(M) // self.seq_rows if self.seq_rows else np.arange(M)
        j = np.arange(M) - sq * self.seq_rows if self.seq_rows else np.zeros(M, int)
        pos = self.pos + (j if self.seq_rows else np.arange(M) * self.pos_step)
        rpos = pos + self.rope_off
        self.row_rope_off = self.seq_rope_off = None
        if self.pos_step < 0:
            pos = np.asarray(self.row_pos)
            self.row_rope_off = (np.arange(M) % 3).astype(np.int32) if self.rope_off else None
            rpos = pos + (self.row_rope_off if self.row_rope_off is not None else 0)
        if self.epi == "QKV_SEQ":
            pos = np.asarray(self.seq_pos)[sq] + j
            self.seq_rope_off = (2 * np.arange(n_seq) % 5).astype(np.int32) if self.rope_off else None
            rpos = pos + (self.seq_rope_off[sq] if self.seq_rope_off is not None else 0)
        self.rpos_, self.pos_, self.sq_ = rpos.astype(int), pos.astype(int), sq
        self.pt_len = int(pos.max()) // KV_PAGE + 1
        one_table = self.pos_step == 1 and not self.seq_rows
        self.pt_rows = 1 if one_table else n_seq
        self.pt_stride = 0 if one_table else self.pt_len + 1  # (a stride that is not the row length)
        n_slots = (self.pt_rows - 1) * self.pt_stride + self.pt_len if not one_table else self.pt_len
        self.n_pages = n_slots + 2
        self.table = rng.permutation(self.n_pages)[:n_slots].astype(np.int32)  # non-identity
        self.table_shape = (1, n_slots)
        self.rope_rows = int(rpos.max()) + 2
        if A:
            self.cos_t = rng.choice(sym, (self.rope_rows, half)).astype(F32)
            self.sin_t = rng.choice(sym, (self.rope_rows, half)).astype(F32)
        else:
            th = np.arange(self.rope_rows)[:, None] * (1e4 ** (-np.arange(half) / half))[None, :]
            self.cos_t, self.sin_t = np.cos(th).astype(F32), np.sin(th).astype(F32)
        shape = (self.n_pages, self.Hk, KV_PAGE, self.Dh)
        self.k0 = bf16_rne(rng.randn(*shape).astype(F32) * 100)  # stale rows: must come back untouched
        self.v0 = bf16_rne(rng.randn(*shape).astype(F32) * 100)

    def page_of(self, sq, pos):
        return self.table[sq * self.pt_stride + pos // KV_PAGE]

    # ---- the call
    def ffi_case(self, plan_only=0):
        from fishrt import _ffi
        self.build()
        c = _ffi.GemmCase()
        keep = []

        def ptr(a, ct=C.c_float, dt=F32):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dt)
            keep.append(a)
            return a.ctypes.data_as(C.POINTER(ct))
        c.op = {"prep": 0, "rows": 1, "down": 2}[self.op]
        c.M, c.plan_only, c.eps = self.M, plan_only, self.eps
        if self.op == "prep":
            c.D, c.S, c.want_frag = self.D, self.S, int(self.want_frag)
            c.x, c.p, c.norm_w = ptr(self.x), ptr(self.p) if self.S else None, ptr(self.norm_w)
            c._keep = keep
            return c
        c.fp8, c.N, c.K, c.ksplit, c.big_min_m = int(self.fp8), self.N, self.K, self.ksplit, self.big_min_m
        c.x, c.w, c.wscale = ptr(self.x), ptr(self.w), ptr(self.wscale)
        if self.op == "down":
            c.x2, c.y, c.g = ptr(self.x2), ptr(self.y0), ptr(self.g)
            c.n_launches, c.epoch, c.node_id = self.n_launches, self.kw.get("epoch", 3), self.kw.get("node_id", 7)
            c.stale_tag = self.kw.get("stale_tag", c.epoch * 4096 + c.node_id - 1)
            c._keep = keep
            return c
        c.epi, c.rt, c.ldy, c.ldo = EPI[self.epi], self.kw.get("rt", self.rt), self.ldy, self.kw.get("ldo", 0)
        if self.epi in ("RESIDUAL", "RESIDUAL_NORM"):
            c.y, c.g = ptr(self.y0), ptr(self.g)
        if self.rms:
            c.ss, c.nblk = ptr(self.ss), self.nblk
        if self.qkv:
            c.H, c.Hk, c.Dh = self.H, self.Hk, self.Dh
            c.pos, c.rope_off, c.pos_step, c.pt_stride, c.seq_rows = self.pos, self.rope_off, self.pos_step, self.pt_stride, self.seq_rows
            c.pt_rows, c.pt_len, c.n_pages, c.rope_rows, c.o1 = self.table_shape[0], self.table_shape[1], self.n_pages, self.rope_rows, int(self.o1)
            c.cos_t, c.sin_t, c.k, c.v = ptr(self.cos_t), ptr(self.sin_t), ptr(self.k0), ptr(self.v0)
            c.page_table = ptr(self.table, C.c_int32, np.int32)
            if self.pos_step < 0:
                c.row_pos = ptr(self.row_pos, C.c_int32, np.int32)
                c.row_rope_off = ptr(self.row_rope_off, C.c_int32, np.int32)
            if self.epi == "QKV_SEQ":
                c.seq_pos = ptr(self.seq_pos, C.c_int32, np.int32)
                c.seq_rope_off = ptr(self.seq_rope_off, C.c_int32, np.int32)
        c._keep = keep
        return c

    def _probe(self):
        from fishrt import _ffi
        c = self.ffi_case(plan_only=1)
        o = _ffi.GemmOut()
        name = C.create_string_buffer(96)
        o.variant, o.variant_cap = C.cast(name, C.c_char_p), 96
        _ffi.check(_ffi.lib().fs_selftest_gemm(0, C.byref(c), C.byref(o)))
        return name.value.decode(), o

    def plan(self):
        """-> (plan name, grid) by validation alone (plan_only: no device)"""
        name, o = self._probe()
        return name, tuple(o.grid)

    def run(self):
        """-> dict: name, grid, guard_ok, and the outputs as arrays (Y, hi, lo, ss, K, V, epoch1) in the shapes of include/fishrt.h"""
        from fishrt import _ffi
        name0, probe = self._probe()
        c = self.ffi_case()
        o = _ffi.GemmOut()
        name = C.create_string_buffer(96)
        o.variant, o.variant_cap = C.cast(name, C.c_char_p), 96
        fp = C.POINTER(C.c_float)
        y, planes, ss = np.zeros(probe.n_y, F32), np.zeros(probe.n_planes, F32), np.zeros(probe.n_ss, F32)
        e1 = np.full(2, 0xFFFFFFFF, np.uint32)
        o.y, o.y_cap, o.planes, o.planes_cap, o.ss, o.ss_cap = y.ctypes.data_as(fp), y.size, planes.ctypes.data_as(fp), planes.size, ss.ctypes.data_as(fp), ss.size
        o.epoch1 = e1.ctypes.data_as(C.POINTER(C.c_uint32))
        ka = va = None
        if self.qkv:
            ka, va = np.zeros_like(self.k0), np.zeros_like(self.v0)
            o.k, o.v, o.pool_cap = ka.ctypes.data_as(fp), va.ctypes.data_as(fp), ka.size
        _ffi.check(_ffi.lib().fs_selftest_gemm(0, C.byref(c), C.byref(o)))
        assert name.value.decode() == name0
        res = dict(name=name.value.decode(), grid=tuple(o.grid), guard_ok=bool(o.guard_ok), K=ka, V=va)
        Mc = self.Mcap
        if self.op == "prep":
            res["Y"] = y.reshape(self.M, self.D)
            if self.want_frag:
                res["hi"], res["lo"] = planes.reshape(2, Mc, self.D)
        elif self.op == "down":
            L = self.n_launches
            res["Y"] = y.reshape(L, PF_M, self.N)
            pl = planes.reshape(L, 2, PF_M, self.N)
            res["hi"], res["lo"] = pl[:, 0], pl[:, 1]
            res["ss"] = ss.reshape(L, PF_M, self.N // 16)
            res["epoch1"] = e1[:L]
        else:
            if y.size:
                res["Y"] = y.reshape(self.ksplit, Mc, self.ldy) if self.epi in ("STORE", "STORE_RMS") else y.reshape(Mc, self.ldy)
            if planes.size:
                res["hi"], res["lo"] = planes.reshape(2, Mc, -1)
            if ss.size:
                res["ss"] = ss.reshape(Mc, -1)
        return res


# ---------------------------------------------------------------------------------------------------------------------------- the reference
def _operand(case, x, mut):
    """the activation operand hi + lo in float64, with the operand mutations applied; rows >= M do not exist (NaN)"""
    hi, lo = split(x)
    hi, lo = hi.astype(F64), lo.astype(F64)
    K = x.shape[1]
    if mut == "lo_drop":       # the lo plane dropped for row tile 0
        lo[:16] = 0.0
    elif mut == "lo_kstep":    # the lo plane read from the neighbouring k-step
        lo = np.roll(lo, -32, axis=1)
    xs = hi + lo
    if mut == "tile_swap":     # row tiles 0..15 and 16..31 of the first panel swapped
        full = np.full((max(32, xs.shape[0]), K), np.nan)
        full[:xs.shape[0]] = xs
        full[:32] = np.concatenate([full[16:32], full[:16]])
        xs = full[:x.shape[0]]
    return xs


def _gemm(case, x, mut=None):
    """-> (acc, tol, unsplit) each [ksplit][M][N] float64: the K-range sums of w (hi + lo) with the fp8 scale applied, their bound n u S,
    and the same sums of the unsplit x with the bound grown by 2^-17 S"""
    case.build()
    W = case.w.astype(F64)
    ks = case.ksplit if case.op == "rows" else 1
    Kr = case.K // ks
    xs = _operand(case, x, mut)
    xa = np.abs(np.nan_to_num(xs))
    if mut == "k_quarter":     # one K quarter (a wave's share) of the first range skipped
        xs = xs.copy()
        xs[:, Kr // 4:Kr // 2] = 0.0
    sc = case.wscale.astype(F64) if case.fp8 else np.ones(case.N)
    if mut == "scale_shift":   # the scale of row r used for r + 1
        sc = np.roll(sc, 1)
    acc = np.stack([xs[:, s * Kr:(s + 1) * Kr] @ W[:, s * Kr:(s + 1) * Kr].T for s in range(ks)]) * sc
    S = np.stack([xa[:, s * Kr:(s + 1) * Kr] @ np.abs(W[:, s * Kr:(s + 1) * Kr]).T for s in range(ks)]) * np.abs(sc)
    n = 2 * Kr + 4 + (1 if case.fp8 else 0)
    uns = np.stack([x.astype(F64)[:, s * Kr:(s + 1) * Kr] @ W[:, s * Kr:(s + 1) * Kr].T for s in range(ks)]) * sc
    return acc, n * U * S, uns, S


def _rms(case):
    """rms[m] and the relative bound of dividing by it"""
    ss = case.ss.astype(F64)
    return np.sqrt(ss.sum(1) / case.K + case.eps), (case.nblk / 8 + 7) * U


def _planes(v, tol, exact):
    """expected hi / lo planes of split(v): exact -> the mirrored split, compared plane by plane; else hi + lo against v"""
    if exact:
        hi, lo = split(v.astype(F32))
        return hi.astype(F64), lo.astype(F64), None
    return None, None, tol + 2.0 ** -17 * np.abs(v)


def reference(case, mut=None):
    """-> dict output name -> (ref, tol): float64 arrays in the hook's output shapes, NaN where the launch writes nothing; tol == 0 means bit
    equality with ref rounded once to the output format (done here).  'sum' entries: (ref, tol) of hi + lo where the planes are not exact.
    mut: one of MUTATIONS."""
    case.build()
    A = case.tier == "A"
    M, N, Mc = case.M, case.N, case.Mcap
    out = {}
    if case.op == "prep":
        return _reference_prep(case, mut)
    if case.op == "down":
        return _reference_down(case, mut)
    acc, tol, uns, S = _gemm(case, case.x, mut)
    tol_split = tol  # (the bound against the unsplit x keeps n u S at every tier)
    if A:
        tol = np.zeros_like(tol)  # exact sums: what is left is each epilogue's own rounding
    if case.rms:
        dn, rel = _rms(case)
        acc, uns = acc / dn[None, :, None], uns / dn[None, :, None]
        rel = 0.0 if A else rel
        tol = tol / dn[None, :, None] + rel * np.abs(acc)
        S = S / dn[None, :, None]
    epi = case.epi
    if epi in ("STORE", "STORE_RMS"):
        Y = np.full((case.ksplit, Mc, case.ldy), np.nan)
        T = np.zeros_like(Y)
        Y[:, :M, :N], T[:, :M, :N] = acc, (0.0 if A else tol)
        out["Y"] = (Y, T)
        Yu, Tu = Y.copy(), T.copy()
        Yu[:, :M, :N], Tu[:, :M, :N] = uns, tol + (rel * np.abs(uns) if case.rms else 0.0) + 2.0 ** -17 * S
        out["Y_unsplit"] = (Yu, Tu)
        return out
    acc, tol, uns, S = acc[0], tol[0], uns[0], S[0]
    if epi in ("RESIDUAL", "RESIDUAL_NORM"):
        y0 = case.y0.astype(F64)
        Y = np.full((Mc, case.ldy), np.nan)
        T = np.zeros_like(Y)
        Y[:M] = y0
        v = y0[:, :N] + acc
        tv = np.zeros_like(v) if A else tol + U * (np.abs(y0[:, :N]) + np.abs(acc))
        Y[:M, :N], T[:M, :N] = v, tv
        out["Y"] = (Y, T)
        if epi == "RESIDUAL_NORM":
            g = case.g.astype(F64)
            vg = v * g
            hi, lo, tsum = _planes(vg, tv * np.abs(g) + U * np.abs(vg), A)
            _put_planes(out, hi, lo, vg, tsum, Mc, N, M, N)
            rows = 64 if case.expect.startswith("big") else 16
            nb = N // rows
            sq = (v * v).reshape(M, nb, rows).sum(2)
            tss = (2 * np.abs(v) * tv + tv * tv).reshape(M, nb, rows).sum(2) + (rows + 2) * U * sq
            if mut == "ss_next":  # the partial of block b + 1
                sq = np.roll(sq, -1, axis=1)
            SS = np.full((Mc, nb), np.nan)
            TS = np.zeros_like(SS)
            SS[:M], TS[:M] = sq, tss
            out["ss"] = (SS, TS)
        return out
    if epi in ("SWIGLU", "SWIGLU_RMS"):
        a, b, ta, tb = acc[:, 0::2], acc[:, 1::2], tol[:, 0::2], tol[:, 1::2]
        v = silu64(a) * b
        tv = 1.1 * ta * np.abs(b) + np.abs(silu64(a)) * tb + (SILU_C_BOUND * (np.abs(a) + 1) * 2.0 ** -24 + 2 * U) * np.abs(v) + ABS_FLOOR
        tv = tv + np.where(a < EXP_OVERFLOW_A, np.abs(v), 0.0)  # e^-a beyond the f32 range: the device's quotient is -0
        ldo = case.kw.get("ldo", 0) or N // 2
        _put_planes(out, None, None, v, tv + 2.0 ** -17 * np.abs(v), Mc, ldo, M, N // 2)
        out["_swiglu_ab"] = (a, b)
        return out
    return _reference_qkv(case, acc, tol, mut, out)


def _put_planes(out, hi, lo, v, tsum, Mc, C, M, n):
    if hi is not None:
        for name, p in (("hi", hi), ("lo", lo)):
            P = np.full((Mc, C), np.nan)
            P[:M, :n] = p
            out[name] = (P, np.zeros_like(P))
    else:
        P = np.full((Mc, C), np.nan)
        T = np.zeros_like(P)
        P[:M, :n], T[:M, :n] = v, tsum
        out["sum"] = (P, T)


def _reference_qkv(case, acc, tol, mut, out):
    A = case.tier == "A"
    M, Mc, Dh, half, qd, kd = case.M, case.Mcap, case.Dh, case.Dh // 2, case.qdim, case.kdim
    cs = case.cos_t.astype(F64)[case.rpos_][:, None, :]
    sn = case.sin_t.astype(F64)[case.rpos_][:, None, :]
    qk = acc[:, :qd + kd].reshape(M, -1, half, 2)
    tq = tol[:, :qd + kd].reshape(M, -1, half, 2)
    a, b = qk[..., 0], qk[..., 1]
    o0, o1 = (a, b) if mut == "rope_norot" else rope_i(a, b, cs, sn)
    r0 = tq[..., 0] * np.abs(cs) + tq[..., 1] * np.abs(sn) + 2 * U * (np.abs(a * cs) + np.abs(b * sn))
    r1 = tq[..., 0] * np.abs(sn) + tq[..., 1] * np.abs(cs) + 2 * U * (np.abs(a * sn) + np.abs(b * cs))
    rot = np.stack([o0, o1], -1).reshape(M, qd + kd)
    trot = np.zeros_like(rot) if A else np.stack([r0, r1], -1).reshape(M, qd + kd)
    Y = np.full((Mc, case.ldy), np.nan)
    T = np.zeros_like(Y)
    Y[:M, :qd], T[:M, :qd] = rot[:, :qd], trot[:, :qd]
    out["Y"] = (Y, T)
    Kp, Vp = case.k0.astype(F64).copy(), case.v0.astype(F64).copy()
    TK, TV = np.zeros_like(Kp), np.zeros_like(Vp)
    vv, tvv = acc[:, qd + kd:], (np.zeros_like(acc[:, qd + kd:]) if A else tol[:, qd + kd:])

    def cache(val, t):
        if A:
            return bf16_rne(val.astype(F32)).astype(F64), np.zeros_like(val)
        return val, t + 2.0 ** -8 * (np.abs(val) + t)
    n_seq = int(case.sq_.max()) + 1
    for m in range(M):
        sq, pos = int(case.sq_[m]), int(case.pos_[m])
        if mut == "pt_neighbor":  # the neighbouring sequence's page table
            sq = (sq + 1) % n_seq
        page = case.page_of(sq, pos)
        kpos = pos - 1 if mut == "kpos-1" else pos
        kpage = case.page_of(sq, kpos) if kpos >= 0 else page
        Kp[kpage, :, kpos % KV_PAGE], TK[kpage, :, kpos % KV_PAGE] = [z.reshape(case.Hk, Dh) for z in cache(rot[m, qd:], trot[m, qd:])]
        Vp[page, :, pos % KV_PAGE], TV[page, :, pos % KV_PAGE] = [z.reshape(case.Hk, Dh) for z in cache(vv[m], tvv[m])]
    out["K"], out["V"] = (Kp, TK), (Vp, TV)
    if case.o1:  # attention over one token is the identity on V: hi = the cached bf16 value of the row's kv group, lo = 0
        n_rep = case.H // case.Hk
        vb = bf16_rne(vv.astype(F32)).astype(F64).reshape(M, case.Hk, 1, Dh)
        hi = np.broadcast_to(vb, (M, case.Hk, n_rep, Dh)).reshape(M, qd)
        _put_planes(out, hi, np.zeros_like(hi), None, None, Mc, qd, M, qd)
    return out


def _reference_prep(case, mut):
    A = case.tier == "A"
    M, Mc, D = case.M, case.Mcap, case.D
    S = case.S - 1 if (mut == "slab_missing" and case.S) else case.S
    v32 = case.x.copy()
    for s in range(S):  # k_prep's own order, one separately rounded f32 addition per slab: mirrored exactly at every tier
        v32 = v32 + case.p[s]
    v = v32.astype(F64)
    tv = np.zeros_like(v)
    out = {"Y": (v, tv)}
    if not case.want_frag:
        return out
    if case.norm:
        d = np.sqrt((v * v).sum(1, keepdims=True) / D + case.eps)
        n = v / d * case.norm_w.astype(F64)
        rel = ((D / 256 + 16) / 2 + 3) * U
        _put_planes(out, None, None, n, tv / d * np.abs(case.norm_w) * 1.01 + (rel + 2.0 ** -17) * np.abs(n), Mc, D, M, D)
    else:  # a deterministic split of an f32 value: exact on normal data too
        hi, lo = split(v32)
        _put_planes(out, hi.astype(F64), lo.astype(F64), None, None, Mc, D, M, D)
    return out


def _reference_down(case, mut):
    A = case.tier == "A"
    M, N, L = case.M, case.N, case.n_launches
    ks = int(case.expect.split("/ks")[1].split("/")[0])
    Y = np.full((L, PF_M, N), np.nan)
    TY = np.zeros_like(Y)
    HI, LO, SUM, TSUM = Y.copy(), Y.copy(), Y.copy(), TY.copy()
    SS = np.full((L, PF_M, N // 16), np.nan)
    TSS = np.zeros_like(SS)
    g = case.g.astype(F64)
    y = case.y0.astype(F64)
    ty = np.zeros_like(y)
    for l in range(L):
        x = case.x if l == 0 else case.x2
        acc, tol, _, S = _gemm(case, x, mut if mut != "slab_missing" else None)
        acc, tol, S = acc[0], tol[0], S[0]
        if mut == "slab_missing":  # one source block's partial left out of the owner's sum
            Kr = case.K // ks
            xs = _operand(case, x, None)
            sc = case.wscale.astype(F64) if case.fp8 else 1.0
            acc = acc - (xs[:, Kr:2 * Kr] @ case.w.astype(F64)[:, Kr:2 * Kr].T) * sc
        v = y + acc
        tv = np.zeros_like(v) if A else ty + tol + ks * U * (np.abs(y) + S)
        Y[l, :M], TY[l, :M] = v, tv
        vg = v * g
        if A:
            h, lo = split(vg.astype(F32))
            HI[l, :M], LO[l, :M] = h, lo
        SUM[l, :M], TSUM[l, :M] = vg, tv * np.abs(g) + (U + 2.0 ** -17) * np.abs(vg)
        sq = (v * v).reshape(M, N // 16, 16).sum(2)
        if mut == "ss_next":
            sq = np.roll(sq, -1, axis=1)
        SS[l, :M] = sq
        TSS[l, :M] = (2 * np.abs(v) * tv + tv * tv).reshape(M, N // 16, 16).sum(2) + 18 * U * (v * v).reshape(M, N // 16, 16).sum(2)
        y, ty = v, tv
    out = {"Y": (Y, TY), "ss": (SS, TSS)}
    if A:
        out["hi"], out["lo"] = (HI, np.zeros_like(HI)), (LO, np.zeros_like(LO))
    else:
        out["sum"] = (SUM, TSUM)
    return out


def check_tier_a(case):
    """the exactness arithmetic of the module docstring, per case: inputs on their grids, and S (+ residual) below 2^24 grid steps"""
    case.build()
    assert case.tier == "A"
    on = lambda a, g: np.array_equal(np.round(np.asarray(a, F64) / g) * g, np.asarray(a, F64))
    sym = lambda a: np.isin(np.asarray(a, F64), [0, 0.5, -0.5, 1, -1]).all()
    if case.op == "prep":
        assert on(case.x, GRID_A) and on(case.p, GRID_A) and np.abs(case.x).max() <= 4
        assert (np.abs(case.x.astype(F64)) + np.abs(case.p.astype(F64)).sum(0)).max() < 2 ** 24 * GRID_A
        return
    assert on(case.x, 2.0 ** -10) and np.abs(case.x).max() <= 1 and sym(case.w)
    hi, lo = split(case.x)
    assert np.array_equal(hi.astype(F64) + lo.astype(F64), case.x.astype(F64)) and (lo != 0).mean() > 0.3
    assert on(hi, 2.0 ** -10) and on(lo, 2.0 ** -10)
    # the GEMM stage: every product a multiple of 2^-11, every partial sum bounded by S < 2^24 2^-11
    S = np.abs(case.x.astype(F64)) @ np.abs(case.w.astype(F64)).T
    if case.op == "down":
        S = np.maximum(S, np.abs(case.x2.astype(F64)) @ np.abs(case.w.astype(F64)).T)
    assert case.K <= 4096 and S.max() < 2 ** 24 * GRID_A, (case.id, float(S.max()))
    # the epilogue stage: power-of-two scales and rms, factors in {0, +-1/2, +-1}, residuals on the grid -- single operations on exact
    # values, so the result is exact iff it is an f32 value: checked on the reference itself
    if case.fp8:
        assert np.isin(case.wscale, [0.5, 1, 2]).all()
    if case.op == "down" or case.epi in ("RESIDUAL", "RESIDUAL_NORM"):
        assert on(case.y0, GRID_A) and np.abs(case.y0).max() <= 4 and sym(case.g)
    if case.rms:
        assert np.isin(case.ss.astype(F64).sum(1) / case.K, [0.25, 1.0, 4.0]).all() and case.eps == 0.0
    if case.qkv:
        assert sym(case.cos_t) and sym(case.sin_t)
    ref = reference(case)
    for name in ("Y",):
        if name in ref:
            y = ref[name][0]
            live = ~np.isnan(y)
            assert np.array_equal(y[live].astype(F32).astype(F64), y[live]), (case.id, name)


# ---------------------------------------------------------------------------------------------------------------------------- the case table
def _wt(fp8):
    return "fp8" if fp8 else "bf16"


def _g3(epi, nks, fp8, half):
    return f"gemm3/{epi}/nks{nks}/rt{EPI_RT[epi]}/{_wt(fp8)}" + ("/half" if half else "")


def listed_variants():
    """the dispatch of launch_gemm3 / launch_gemm_down written out branch for branch: every name a launch can have"""
    names = set()
    for epi in EPI:                       # k_gemm3: depth per K range / 128 in {1, 2, 8} x weight type x (M <= 16)
        for nks in (1, 2, 8):
            for fp8 in (False, True):
                for half in (False, True):
                    names.add(_g3(epi, nks, fp8, half))
    for epi in BIG_EPIS:                  # k_gemm_big: 1024 per K range from GB_MIN_M rows, every epilogue
        for fp8 in (False, True):
            names.add(f"big/{epi}/{_wt(fp8)}")
    for nks, ks in ((8, 4), (2, 4), (1, 2)):  # k_gemm_down: K in {4096, 1024, 256}
        for fp8 in (False, True):
            names.add(f"down/nks{nks}/ks{ks}/{_wt(fp8)}")
    names |= {"prep/one", "prep/reread"}
    return names


def _qkv_kw(epi, M, i):
    """position layouts of the QKV epilogues, cycled over the cases: prefill across a page boundary, lock-step rows (the `pre` path), per-row
    states, group rows"""
    if epi == "QKV_SEQ":
        sr = 3 if M % 3 == 0 else 1
        n = M // sr
        return dict(pos_step=1, seq_rows=sr, seq_pos=[(0, 63, 130, 7, 64, 191)[s % 6] + 200 * (s // 6) for s in range(n)], rope_off=i % 2)
    k = i % 3
    if k == 0:
        return dict(pos_step=1, pos=62, rope_off=3 * (i % 2))
    if k == 1:
        return dict(pos_step=0, pos=5 + 59 * (i % 2), rope_off=i % 2)
    return dict(pos_step=-1, row_pos=[(63, 0, 64, 130, 7)[m % 5] for m in range(M)], rope_off=i % 2)


@functools.lru_cache(maxsize=None)
def all_cases():
    cs = []
    add = lambda *a, **k: cs.append(Case(*a, **k))
    MS_HALF, MS_FULL = (1, 15, 16), (17, 31, 32, 33, 65)
    i = 0
    # every k_gemm3 instantiation, smallest shapes: K = 128 nks, one K range
    for epi in EPI:
        for nks in (1, 2, 8):
            for fp8 in (False, True):
                for half in (True, False):
                    M = (MS_HALF if half else MS_FULL)[i % (3 if half else 5)]
                    tier = "AB"[i % 2]
                    kw = {}
                    N = 48
                    if epi in QKV_EPIS:
                        if epi == "QKV_SEQ" and M % 3:
                            M = {1: 3, 16: 15, 17: 18, 31: 33, 32: 33, 65: 66}.get(M, M)
                        kw = dict(geom=("MID", "TINY", "FISH")[i % 3] if nks < 8 else ("MID", "TINY")[i % 2], **_qkv_kw(epi, M, i))
                    elif epi == "RESIDUAL_NORM":
                        N = 128
                    elif epi in ("SWIGLU", "SWIGLU_RMS"):
                        N = 128 if i % 2 else 64
                    elif epi in ("STORE", "STORE_RMS"):
                        N, kw = ((37, dict(ld=48)), (40, {}), (48, dict(ld=56)))[i % 3]
                    else:
                        N = (40, 48)[i % 2]
                    add(f"g3-{epi}-nks{nks}-{_wt(fp8)}-M{M}-{tier}", "rows", tier, _g3(epi, nks, fp8, half), M, N, 128 * nks, epi=epi, fp8=fp8, **kw)
                    i += 1
    # both tiers of the shapes the issue names: split-K STORE slabs, the panel loop with gridDim.z < panels, o1, fp8 RESIDUAL_NORM
    for K, nks in ((512, 1), (1024, 2), (4096, 8)):
        for tier in "AB":
            add(f"g3-STORE-ks4-K{K}-{tier}", "rows", tier, _g3("STORE", nks, tier == "B", False), 33, 40, K, epi="STORE", ksplit=4, fp8=tier == "B")
    for tier in "AB":
        add(f"g3-STORE-panels-N6400-{tier}", "rows", tier, _g3("STORE", 1, False, False), 97, 6400, 128, epi="STORE", grid=(400, 1, 2))
        add(f"g3-RESIDUAL-panels-N6400-{tier}", "rows", tier, _g3("RESIDUAL", 1, False, False), 97, 6400, 128, epi="RESIDUAL", grid=(400, 1, 2))
    # QKV epilogues in a block's second panel: FISH has 80 tiles, 1024 / 80 = 12 < 13 panels, so block z = 0 runs panels 0 and 12; lock-step rows
    # (pos_step 0: the `pre` slot of the first panel), the *_RMS form also rewrites s_rms behind the panel barrier
    for tier in "AB":
        add(f"g3-QKV-panels-pre-M416-{tier}", "rows", tier, _g3("QKV", 1, False, False), 416, 0, 128, epi="QKV", geom="FISH", pos_step=0, pos=5,
            rope_off=2, grid=(80, 1, 12))
        add(f"g3-QKV_RMS-panels-pre-M416-{tier}", "rows", tier, _g3("QKV_RMS", 1, tier == "A", False), 416, 0, 128, epi="QKV_RMS", fp8=tier == "A",
            geom="FISH", pos_step=0, pos=70, grid=(80, 1, 12))
        # ... and the RT = 2 SwiGLU epilogue with the rms: 200 tiles, 1024 / 200 = 5 < 6 panels
        add(f"g3-SWIGLU_RMS-panels-N6400-{tier}", "rows", tier, _g3("SWIGLU_RMS", 1, False, False), 161, 6400, 128, epi="SWIGLU_RMS", grid=(200, 1, 5))
        add(f"g3-STORE_RMS-panels-N6400-{tier}", "rows", tier, _g3("STORE_RMS", 1, tier == "B", False), 97, 6400, 128, epi="STORE_RMS", fp8=tier == "B",
            grid=(400, 1, 2))
    add("g3-QKV-o1-pos0-M4-A", "rows", "A", _g3("QKV", 2, False, True), 4, 0, 256, epi="QKV", geom="MID", pos_step=0, pos=0, o1=True)
    add("g3-QKV_RMS-o1-pos0-M17-A", "rows", "A", _g3("QKV_RMS", 1, True, False), 17, 0, 128, epi="QKV_RMS", fp8=True, geom="FISH", pos_step=-1,
        row_pos=[0] * 17, o1=True)
    add("g3-QKV-rowstates-M65-A", "rows", "A", _g3("QKV", 1, False, False), 65, 0, 128, epi="QKV", geom="FISH", pos_step=-1,
        row_pos=[5 + m // 32 for m in range(65)])
    add("g3-QKV_SEQ-pages-M9-B", "rows", "B", _g3("QKV_SEQ", 2, False, True), 9, 0, 256, epi="QKV_SEQ", geom="TINY", pos_step=1, seq_rows=3,
        seq_pos=[0, 63, 130], rope_off=1)
    # k_gemm_big: K = 1024 per range
    j = 0
    for epi in BIG_EPIS:
        for fp8 in (False, True):
            tier = "AB"[j % 2]
            M, N = ((512, 64), (513, 72), (545, 136))[j % 3]
            kw = {}
            if epi in QKV_EPIS:
                kw = dict(geom="MID", pos_step=1, pos=(0, 30)[j % 2], rope_off=j % 2)
                if epi == "QKV_SEQ":
                    M, kw = 513, dict(geom="MID", pos_step=1, seq_rows=171, seq_pos=[0, 63, 130], rope_off=1)
            elif epi == "RESIDUAL_NORM":
                N = 512
            elif epi in ("SWIGLU", "SWIGLU_RMS"):
                N = (64, 128)[j % 2]
            elif epi == "RESIDUAL":
                N = (64, 72, 136)[j % 3]
            add(f"big-{epi}-{_wt(fp8)}-M{M}-{tier}", "rows", tier, f"big/{epi}/{_wt(fp8)}", M, N, 1024, epi=epi, fp8=fp8, **kw)
            j += 1
    add("big-STORE-M129-N4096-B", "rows", "B", "big/STORE/bf16", 129, 4096, 1024, epi="STORE", grid=(64, 1, 5))
    add("big-STORE-M129-ks4-A", "rows", "A", "big/STORE/bf16", 129, 1024, 4096, epi="STORE", ksplit=4, grid=(16, 4, 5))
    add("big-RESIDUAL-M289-N4096-xpanel-A", "rows", "A", "big/RESIDUAL/fp8", 289, 4096, 1024, epi="RESIDUAL", fp8=True, grid=(64, 1, 8))
    # k_gemm_down
    j = 0
    for K, nks, ks in ((256, 1, 2), (1024, 2, 4), (4096, 8, 4)):
        for fp8 in (False, True):
            for M in (1, 16, 17, 32):
                tier = "AB"[(j + j // 4) % 2]
                N = (128, 256)[(j // 2 + j // 8) % 2]
                add(f"down-K{K}-{_wt(fp8)}-M{M}-N{N}-{tier}", "down", tier, f"down/nks{nks}/ks{ks}/{_wt(fp8)}", M, N, K,
                    fp8=fp8, n_launches=2 if M in (17, 32) else 1)
                j += 1
    # k_prep
    j = 0
    for D in (256, 384, 1024, 2048):
        for S in (0, 1, 4):
            for norm in (False, True):
                tier = "B" if norm else "AB"[j % 2]
                add(f"prep-D{D}-S{S}-{'norm' if norm else 'split'}-{tier}", "prep", tier, "prep/one" if D <= 1024 else "prep/reread", (1, 33, 5)[j % 3],
                    D=D, S=S, norm=norm)
                j += 1
    add("prep-D1024-S4-nofrag-A", "prep", "A", "prep/one", 3, D=1024, S=4, want_frag=False)
    add("prep-D2048-S1-nofrag-B", "prep", "B", "prep/reread", 2, D=2048, S=1, want_frag=False)
    return tuple(cs)


# the ways these kernels go wrong, and the cases each applies to
MUTATIONS = ("lo_drop", "lo_kstep", "tile_swap", "k_quarter", "scale_shift", "rope_norot", "kpos-1", "pt_neighbor", "ss_next", "slab_missing")


def mutation_applies(case, mut):
    if case.op == "prep":
        return mut == "slab_missing" and case.S > 0
    if mut in ("lo_drop", "lo_kstep", "k_quarter", "tile_swap"):
        return True
    if mut == "scale_shift":
        return case.fp8
    if mut in ("rope_norot", "kpos-1"):
        return case.qkv
    if mut == "pt_neighbor":
        return case.qkv and case.pt_stride > 0 and case.M > 1 and (case.seq_rows == 0 or case.M > case.seq_rows)
    if mut == "ss_next":
        return case.op == "down" or case.epi == "RESIDUAL_NORM"
    return case.op == "down"  # slab_missing


def rejected_cases():
    """(label, case, attribute overrides on the ffi struct, text of the validation message)"""
    base = lambda **k: Case("rej", "rows", "A", "", 4, 48, 128, **k)
    return [
        ("pair", base(epi="SWIGLU", rt=1), {}, "not a pair"),
        ("pair2", base(epi="STORE", rt=2), {}, "not a pair"),
        ("depth", base(epi="STORE"), {"K": 384}, "unsupported GEMM depth"),
        ("ksplit", base(epi="RESIDUAL"), {"ksplit": 2, "K": 256}, "only the STORE epilogues"),
        ("ldy", base(epi="STORE"), {"ldy": 40}, "ldy must cover N"),
        ("bf16", base(epi="STORE"), {"_w": 1.0 + 2.0 ** -10}, "not a bf16 value"),
        ("e4m3", base(epi="STORE", fp8=True), {"_w": 1.0 + 2.0 ** -4}, "not an e4m3fn value"),
        ("oddN", base(epi="RESIDUAL"), {"N": 37, "ldy": 48}, "even N"),
        ("page", Case("rej", "rows", "A", "", 4, 0, 128, epi="QKV", geom="MID", pos_step=1, pos=62), {"n_pages": 1}, "page id is outside the pool"),
        ("rope", Case("rej", "rows", "A", "", 4, 0, 128, epi="QKV", geom="MID", pos_step=1, pos=62), {"rope_rows": 3}, "RoPE row"),
        ("slot", Case("rej", "rows", "A", "", 4, 0, 128, epi="QKV", geom="MID", pos_step=0, pos=5), {"pt_stride": 0}, "same cache row"),
        ("o1big", Case("rej", "rows", "A", "", 512, 0, 1024, epi="QKV", geom="MID", pos_step=1, pos=0, o1=True), {}, "o1 needs the k_gemm3 path"),
        ("downM", Case("rej", "down", "A", "", 33, 128, 256), {}, "k_gemm_down does not take"),
        ("downK", Case("rej", "down", "A", "", 4, 128, 512), {}, "k_gemm_down does not take"),
        ("downN", Case("rej", "down", "A", "", 4, 64, 256), {"N": 64}, "k_gemm_down does not take"),
        ("stale", Case("rej", "down", "A", "", 4, 128, 256, stale_tag=3 * 4096 + 7), {}, "stale_tag equals"),
        ("prepD", Case("rej", "prep", "A", "", 4, D=100), {}, "multiple of 32"),
    ]


def call_rejected(case, over):
    from fishrt import _ffi
    c = case.ffi_case()
    for k, v in over.items():
        if k == "_w":
            case.w[0, 0] = v
            c = case.ffi_case()
        else:
            setattr(c, k, v)
    o = _ffi.GemmOut()
    name = C.create_string_buffer(96)
    o.variant, o.variant_cap = C.cast(name, C.c_char_p), 96
    rc = _ffi.lib().fs_selftest_gemm(0, C.byref(c), C.byref(o))
    return rc, _ffi.lib().fs_last_error().decode()
