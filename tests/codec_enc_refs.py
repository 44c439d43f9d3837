"""float64 numpy references of the encoder-side / ConvNeXt / FSQ kernels (csrc/codec_kernels.hip), the planted and searched inputs of their
GPU tests, and the ctypes wrapper of fs_selftest_codec_op.  Shared by test_codec_encoder_ops_gpu.py, test_codec_encoder_stages_gpu.py (GPU)
and test_codec_encoder_ref_cpu.py, which pins every reference here against the CPU oracle and the golden fixture without a GPU.

Nothing here is the oracle's f32 code or a kernel's expression: every function is the operation's definition in float64."""
import ctypes

import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24  # unit roundoff of f32
LEVELS, BASIS = (8, 5, 5, 5), (1, 8, 40, 200)
N_FFT, HOP, N_MELS = 2048, 512, 160


# ------------------------------------------------------------------------------------------------------------------------- references
def ref_space_to_depth(x, s):
    """y[c * s + k][t] = x[c][t * s + k]; the last T % s columns are dropped"""
    C, T = x.shape
    To = T // s
    return np.ascontiguousarray(x[:, : To * s].reshape(C, To, s).transpose(0, 2, 1).reshape(C * s, To))


def n_frames(n, n_fft=N_FFT, hop=HOP):
    """frames the streaming STFT emits for an n-sample clip: one per hop once n_fft samples are in, plus one for a partial last hop"""
    Lp = n + (n_fft - hop)
    full, rem = divmod(Lp, hop)
    F = max(0, full - (n_fft // hop - 1))
    return F + (1 if rem > 0 and Lp >= n_fft else 0)


def ref_stft_frames(pcm, T, n_fft=N_FFT, hop=HOP):
    """the T windowed frames in float64, [T][n_fft]: reflect pad that repeats the edge sample, zeros behind the padded signal, periodic Hann"""
    x = np.asarray(pcm, F64)
    pad = (n_fft - hop) // 2
    padded = np.concatenate([x[:pad][::-1], x, x[x.size - pad:][::-1]])
    need = (T - 1) * hop + n_fft
    if padded.size < need:
        padded = np.concatenate([padded, np.zeros(need - padded.size)])
    win = 0.5 * (1.0 - np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft))
    return np.stack([padded[f * hop: f * hop + n_fft] * win for f in range(T)])


def ref_stft_mag(pcm, T, n_fft=N_FFT, hop=HOP):
    """-> (|rfft| float64 [n_fft/2+1][T] WITHOUT the + 1e-6, the L2 norm of each windowed frame [T])"""
    fr = ref_stft_frames(pcm, T, n_fft, hop)
    return np.abs(np.fft.rfft(fr, axis=1)).T.copy(), np.sqrt((fr * fr).sum(1))


def stft_expected_f32(mag64):
    """what the kernel stores for an exact magnitude: (f32)|.| + 1e-6f in f32 arithmetic"""
    return (mag64.astype(F32) + F32(1e-6)).astype(F32)


def ref_mel_sum(lin, fb):
    """float64 sum_k lin[k][f] * fb[k][m] -> [n_mels][F]"""
    return np.asarray(fb, F64).T @ np.asarray(lin, F64)


def mel_chain_f32(lin, fb):
    """the ascending-k chain of separately rounded f32 products and sums the kernel promises (__fadd_rn(__fmul_rn)), [n_mels][F] f32"""
    lin, fb = np.asarray(lin, F32), np.asarray(fb, F32)
    acc = np.zeros((fb.shape[1], lin.shape[1]), F32)
    for k in range(lin.shape[0]):
        acc = (acc + (fb[k][:, None] * lin[k][None, :]).astype(F32)).astype(F32)
    return acc


def ref_log_clamp(s):
    """log(clamp(s, 1e-5f, 100)) in float64 (the clamp constants are the f32 ones)"""
    return np.log(np.clip(np.asarray(s, F64), float(F32(1e-5)), 100.0))


def ref_log_mel(pcm, fb):
    """the whole front-end in float64 (only the table and the stored magnitude are f32) -> [n_mels][F]"""
    T = n_frames(len(pcm))
    mag, _ = ref_stft_mag(pcm, T)
    return ref_log_clamp(ref_mel_sum(stft_expected_f32(mag), fb))


def ref_layernorm_cf(x, w, b, eps=1e-6):
    """per time step over the channels (axis -2), biased variance -> y, and the pieces the bounds need"""
    x = np.asarray(x, F64)
    m = x.mean(-2, keepdims=True)
    d = x - m
    v = (d * d).mean(-2, keepdims=True)
    sd = np.sqrt(v + eps)
    w = np.asarray(w, F64)[:, None]
    return d / sd * w + np.asarray(b, F64)[:, None], dict(d=d, v=v, sd=sd, A=np.abs(x).mean(-2, keepdims=True))


def ref_dwconv(x, dw, db, ctx=None):
    """causal depthwise 7-tap: a[b][c][t] = db[c] + sum_k dw[c][k] * x[b][c][t + k - 6], 6 zeros (or the context's last 6 columns,
    ctx [B][C][>= 6]) in front -> (a, S = sum |dw x| + |db|)"""
    x = np.asarray(x, F64)
    B, C, T = x.shape
    left = np.zeros((B, C, 6)) if ctx is None else np.asarray(ctx, F64)[:, :, -6:]
    xp = np.concatenate([left, x], axis=2)
    dw = np.asarray(dw, F64)
    a = np.zeros((B, C, T))
    S = np.zeros((B, C, T))
    for k in range(7):
        term = dw[None, :, k, None] * xp[:, :, k: k + T]
        a += term
        S += np.abs(term)
    db = np.asarray(db, F64)[None, :, None]
    return a + db, S + np.abs(db)


def ref_dwconv_ln(x, dw, db, lnw, lnb, ctx=None):
    a, S = ref_dwconv(x, dw, db, ctx)
    y, parts = ref_layernorm_cf(a, lnw, lnb)
    parts["S"] = S
    return y, parts


def fsq_bound64(z, lv):
    """FSQ bound of one coordinate with lv levels, float64"""
    half_l = (lv - 1.0) * 1.001 / 2.0
    offset = 0.5 if lv % 2 == 0 else 0.0
    return np.tanh(z + np.arctanh(offset / half_l)) * half_l - offset


def ref_fsq_encode(z, pin_w, pin_b, G):
    """z [C][T], pin_w [G][4][dg], pin_b [G][4] -> (indices uint32 [G][T], margin float64 [G][T] = the smallest distance of a pre-round
    value from a rounding boundary x.5).  bound is applied twice (project_in -> bound -> the layer's own quantize), as the reference does."""
    z = np.asarray(z, F64)
    C, T = z.shape
    dg = C // G
    pre = np.einsum("gkc,gct->gkt", np.asarray(pin_w, F64).reshape(G, 4, dg), z.reshape(G, dg, T)) + np.asarray(pin_b, F64).reshape(G, 4, 1)
    idx = np.zeros((G, T), np.int64)
    margin = np.full((G, T), 1.0)
    for k, lv in enumerate(LEVELS):
        p = fsq_bound64(fsq_bound64(pre[:, k], lv), lv)
        margin = np.minimum(margin, np.abs(np.abs(p - np.floor(p)) - 0.5))
        idx += (np.rint(p).astype(np.int64) + lv // 2) * BASIS[k]
    return idx.astype(np.uint32), margin


def fsq_codes64(idx):
    """indices [...] -> the four code coordinates float64 [4][...] in [-1, 1]"""
    idx = np.asarray(idx, np.int64)
    return np.stack([((idx // BASIS[k]) % lv - lv // 2) / float(lv // 2) for k, lv in enumerate(LEVELS)])


def ref_fsq_project(codes, B, G, pw, pb, dg, item_rows=False):
    """codes [B * G][T], pw [G][dg][4], pb [G][dg] -> (z [B][G * dg][T], S = sum |code w| + |b|); item (b, g) reads row g * B + b, or with
    item_rows row b * G + g"""
    codes = np.asarray(codes)
    T = codes.shape[1]
    pw, pb = np.asarray(pw, F64).reshape(G, dg, 4), np.asarray(pb, F64).reshape(G, dg)
    z, S = np.zeros((B, G * dg, T)), np.zeros((B, G * dg, T))
    for b in range(B):
        for g in range(G):
            code = fsq_codes64(codes[b * G + g if item_rows else g * B + b])  # [4][T]
            z[b, g * dg:(g + 1) * dg] = pw[g] @ code + pb[g][:, None]
            S[b, g * dg:(g + 1) * dg] = np.abs(pw[g]) @ np.abs(code) + np.abs(pb[g])[:, None]
    return z, S


# ------------------------------------------------------------------------------------------------------------------------- bounds
def layernorm_tol(parts, y, w, C, fn_bound, exact_mean=False, conv_S=None):
    """per-element bound of an f32 LayerNorm over C channels against ref_layernorm_cf (derivation: header of test_codec_encoder_ops_gpu.py).
    exact_mean: the planted rows whose channel sum is exact in f32 in any order.  conv_S: the depthwise conv in front (k_dwconv_ln)."""
    d, v, sd, A = parts["d"], parts["v"], parts["sd"], parts["A"]
    w = np.abs(np.asarray(w, F64))[:, None]
    dm = 0.0 if exact_mean else (C + 1) * U * A
    eps_sd = 0.5 * ((C + 5) * U * v + dm * dm) / (sd * sd) + 2 * U
    nd = np.abs(d) / sd
    tol = w * (dm / sd + nd * (4 * U + eps_sd + fn_bound)) + U * np.abs(y)
    if conv_S is not None:
        e = 8 * U * conv_S
        tol = tol + w / sd * (e + e.mean(-2, keepdims=True) + nd * np.sqrt((e * e).mean(-2, keepdims=True)))
    return tol


# ------------------------------------------------------------------------------------------------------------------------- inputs
def clip(n, seed):
    """the encode suite's test clip (tests/test_codec_encode.py: _clip): two sinusoids and noise"""
    rng = np.random.RandomState(seed)
    t = np.arange(n) / 44100.0
    return (0.25 * np.sin(2 * np.pi * 330.0 * t) + 0.1 * np.sin(2 * np.pi * 2500.0 * t + 0.5) + 0.05 * rng.randn(n)).astype(F32)


def fsq_safe_targets(lv, min_margin=0.05):
    """pre-projection values (multiples of 1/16 in [-4, 4], and the saturating +-50) whose twice-bounded value stays min_margin away from
    every rounding boundary"""
    cand = np.concatenate([[-50.0], np.arange(-64, 65) / 16.0, [50.0]])
    p = fsq_bound64(fsq_bound64(cand, lv), lv)
    return cand[np.abs(np.abs(p - np.floor(p)) - 0.5) >= min_margin]


def fsq_exact_case(C, G, T, seed):
    """z, pin_w, pin_b (all dyadic: the f32 projection chain is exact in any order) whose four projections per (g, t) walk through every
    safe target of their level; (g, t) = (0, 0) is all -50 (index 0), (G - 1, T - 1) all +50 (index 999) when T > 1"""
    rng = np.random.RandomState(seed)
    dg = C // G
    w = np.zeros((G, 4, dg))
    for k in range(4):
        w[:, k, k] = 1.0
    if dg > 4:
        w[:, :, 4:] = rng.randint(-2, 3, (G, 4, dg - 4)) / 2.0
    b = rng.randint(-8, 9, (G, 4)) / 16.0
    z = np.zeros((G, dg, T))
    if dg > 4:
        z[:, 4:] = rng.randint(-8, 9, (G, dg - 4, T)) / 4.0
    for k, lv in enumerate(LEVELS):
        safe = fsq_safe_targets(lv)
        tgt = safe[(np.arange(G * T).reshape(G, T) * (2 * k + 7) + k) % safe.size]  # steps 7, 9, 11, 13: coprime to the list lengths
        tgt[0, 0] = -50.0
        tgt[G - 1, T - 1] = 50.0 if T > 1 or G > 1 else -50.0
        z[:, k] = tgt - b[:, k, None] - np.einsum("gc,gct->gt", w[:, k, 4:], z[:, 4:])
    z, w, b = z.reshape(C, T).astype(F32), w.astype(F32), b.astype(F32)
    return z, w, b


def fsq_random_case(C, G, T, seed):
    rng = np.random.RandomState(seed)
    dg = C // G
    z = rng.randn(C, T).astype(F32)
    w = (rng.randn(G, 4, dg) / np.sqrt(dg)).astype(F32)
    b = (0.02 * rng.randn(G, 4)).astype(F32)
    return z, w, b


# seeds found by a CPU search (test_codec_encoder_ref_cpu.py re-checks them): fsq_random_case(C, G = 8, T, seed) has a float64 reference
# margin >= 1e-4 at EVERY index, so the f32 kernel (projection error <= (dg + 2) 2^-24 sum |z w| ~ 1e-6, tanhf / logf ~ 1e-7 on values
# <= 4) must produce the reference's index everywhere
FSQ_RANDOM_SEEDS = {(64, 1): 1, (64, 63): 2, (64, 64): 1, (64, 65): 1,      # (C, T) -> seed; margins found: 1.3e-2, 1.3e-4, 1.7e-4, 1.2e-3
                    (512, 1): 1, (512, 63): 3, (512, 64): 2, (512, 65): 1}  # 2.3e-2, 2.9e-4, 1.1e-3, 2.9e-4
FSQ_RANDOM_MARGIN = 1e-4

# _clip seeds found by a CPU search (re-checked by test_codec_encoder_ref_cpu.py): the tiny oracle's rounding margin (encode_mel stage 7)
# is >= 1e-3 at every index of clip(9000, seed) AND of its prefix of the listed length
STRICT_CLIPS = ((101, 9000), (102, 2304), (103, 5000), (104, 7777), (106, 3333), (107, 6000))  # (seed, prefix length)
# margins found (whole clip / prefix): 1.8e-3 / 1.8e-3, 1.7e-3 / 3.1e-3, 3.5e-3 / 4.4e-2, 6.5e-3 / 6.5e-3, 4.1e-3 / 5.4e-2, 1.1e-2 / 1.1e-2
STRICT_MARGIN = 1e-3

# d_i of test_codec_encoder_stages_gpu.py: max |f32 oracle - the golden file's restatement| at encoder stage i on the golden mel, computed on
# the CPU (test_codec_encoder_ref_cpu.py recomputes it)
STAGE_D = (3.34e-06, 2.57e-06, 2.61e-06, 3.19e-06, 3.22e-06, 2.21e-06, 2.75e-06)


# ------------------------------------------------------------------------------------------------------------------------- the entry point
def _fp(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def run_op(op, n_out, x=None, w=(), ctx=None, ctx_off=None, codes=None, ctx_elems=0, out_dtype=F32, **dims):
    """one fs_selftest_codec_op call -> (out [n_out] f32 or uint32, guard_ok).  dims: the int fields of fs_codec_op_case"""
    from fishrt import _ffi
    keep = [None if a is None else np.ascontiguousarray(a, F32) for a in [x, *w, *([None] * (4 - len(w))), ctx]]
    off = None if ctx_off is None else np.ascontiguousarray(ctx_off, np.int64)
    cd = None if codes is None else np.ascontiguousarray(codes, np.uint32)
    c = _ffi.CodecOpCase(op=op, ctx_elems=int(ctx_elems), **{k: int(v) for k, v in dims.items()})
    c.x, c.w0, c.w1, c.w2, c.w3, c.ctx = [_fp(a) for a in keep]
    if off is not None:
        c.ctx_off = off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    if cd is not None:
        c.codes = cd.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    out = np.zeros(max(int(n_out), 1), out_dtype)
    n, ok = ctypes.c_size_t(0), ctypes.c_int(0)
    _ffi.check(_ffi.lib().fs_selftest_codec_op(0, ctypes.byref(c), out.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(int(n_out)),
                                               ctypes.byref(n), ctypes.byref(ok)))
    assert n.value == n_out, (n.value, n_out)
    return out[: n.value], bool(ok.value)
