"""Every launch variant of the vocoder's conv kernels (csrc/codec_kernels.hip, csrc/codec_conv_bf3.hip) against a per-sample float64 oracle.

One entry point, fs_selftest_conv1d (include/fishrt.h), runs ONE conv on host data through the engine's own load-time functions (re-layout,
pack), plane producers and launchers, and reports the name of the kernel instantiation the launcher chose.  The tables below name, for every
case, the variant it must reach; VARIANTS is the dispatch of conv1d_launch, conv1d_bf3_impl and codec_respair_f16 written out branch for
branch, and test_every_listed_variant_is_reached holds the two together: a retuned threshold breaks a test instead of losing a kernel.

Variant names: "f32/..." = conv1d_launch's own kernels (k_conv1d_one, k_conv1d_mfma, k_conv1d); "bf3/..." and "f16/..." = conv1d_bf3_impl in
bf16x3 / f16 mode -- "bf3x" the f32-input kernel k_conv1d_bf3 (seven branches over six instantiations), "bf3p/pw8" the pointwise plane path,
"bf3t" the thin plane path, "bf3p/TT*/nibs*" the wide plane path; "f16/pair" = k_respair_f16t.  psN = polyphase rows of a transposed conv.
Not reachable without the FISHRT_BF3P_* knobs, hence not listed: f16 wide TT256 with nibs4 (TT256 needs >= 1024 blocks, nibs4 <= 512), bf16x3
with nibs > 1, and the ragged instantiations of the pair (streaming contexts are held bit for bit by the stream / ragged suites).

Tier A (exact): x, w, res, mean_* in {q/8, |q| <= 8}, bias in multiples of 1/64, gamma in +-{1/4, 1/2, 1, 2}.  The operands are exact in f16
and bf16 (lo plane = 0), every product is a multiple of 1/64 of magnitude <= 1 and |sum| * 64 <= 13 * 2048 * 64 < 2^24, so every partial sum
is exact in f32 in any order and inside an MFMA: the output must EQUAL the float64 reference rounded to f32 (to the plane format for a plane
output) at every sample, in all three modes.  The mean fold is one f32 add chain and one f32 multiply, mirrored in numpy f32.

Tier B (derived bound, normal data, w ~ N(0, 1/(Cin K))): the reference rounds the operands as the mode does (f16: RNE, saturating; f32 and
bf16x3: not at all) and sums in float64; per sample, with S = sum |w_i x_i| and n = Cin K,
    |conv - ref| <= (c_mode + n 2^-23 [+ delta_mode if a SiLU feeds the conv]) S + 2^-23 |ref|,   c_f32 = c_f16 = 2^-23, c_bf16x3 = 3 * 2^-16
(the dropped lo*lo term and the two split residuals: header of codec_conv_bf3.hip); delta_f16 = 2^-10, delta_bf16x3 = 2^-15 cover a device SiLU
that lands on the other side of a rounding boundary, delta_f32 = SILU_F32_BOUND is the device SiLU's own error.  An epilogue adds 2^-23 times
the magnitudes of its operands per f32 operation; a plane output adds the format's rounding (f16: 2^-11 relative and 2^-25 absolute;
bf16x3: 2^-16 relative -- bf16 RNE has unit roundoff 2^-8, applied to v and again to v - hi); a post_silu plane output is taken through the
1.1-Lipschitz SiLU.

Measured allowances (MI355X, over this module's own inputs; asserted = 4 x measured, the ulp error of __expf varies with the argument):
    device SiLU, f32 mode (dsilu, the expression of c3_silu), relative, x ~ N(0, 16):  measured 8.442e-07 (14.2 x 2^-24), asserted 3.4e-06
    c3_silu / c3_silu_fast read through the bf16x3 split (residual <= 2^-16), relative:  measured 7.4e-06 / 7.1e-06, inside delta_bf16x3 = 3.05e-05
    c3_silu / c3_silu_fast read through the f16 format (2^-11), relative:                measured 4.85e-04 / 4.88e-04, inside delta_f16 = 9.77e-04
    GELU, |y - gelu64(v)| / max(|v|, 1), every family:                                   measured 9.236e-08 (1.55 x 2^-24), asserted 3.7e-07
    tanh, |y - tanh64(v)| (and |y| <= 1 always), every family:                           measured 5.537e-08 (0.93 x 2^-24), asserted 2.3e-07
GELU and tanh run on Tier A inputs, so the pre-activation v is exact and what remains is the device function's own error.

Tier C (bit identity the code promises): same case at another (T, B) -- another instantiation -- gives the same common samples; the fused
pair equals the two-launch sequence; the folded mean equals k_mean3 / k_mean3_planes; the range-checked twin equals the plain kernels with
both counters at what the data holds (0), and counts exactly the operands planted above 65504 / below 2^-24."""
import ctypes
import os
import zlib
from collections import namedtuple

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import fishrt
from fishrt import _ffi

F32 = np.float32
PAD = 64  # CODEC_PLANE_PAD
CONV, TCONV, CONV_P, TCONV_P, PAIR = range(5)
IN_F32, IN_SPLIT, IN_SPLIT_SILU, IN_MEAN3, IN_MEAN3_SILU = range(5)
NONE, GELU, GAMMA_RES, RES, TANH = range(5)
OUT_Y, OUT_P, OUT_BOTH = 1, 2, 3
MODE = {0: "f32", 1: "bf3", 2: "f16"}

# measured on an MI355X by test_device_silu_error / test_gelu_tanh_function_error (printed there); asserted = 4 x measured
SILU_F32_MEASURED = 8.442e-07
SILU_F32_BOUND = 3.4e-06
GELU_MEASURED = 9.236e-08
GELU_BOUND = 3.7e-07
TANH_MEASURED = 5.537e-08
TANH_BOUND = 2.3e-07

KNOBS = ("FISHRT_BF3P_TT", "FISHRT_BF3P_NIBS", "FISHRT_BF3P_NIBS4_BLOCKS", "FISHRT_PAIR_NW1", "FISHRT_PAIR_NW2", "FISHRT_VOC_NO_PAIR_FUSION")


# ---------------------------------------------------------------------------------------------------------------- the dispatch, written out
def _variants():
    v = ["f32/one/CIN16"]
    v += [f"f32/mfma/OT{ot}/TT{tt}" for ot in (64, 32) for tt in (256, 128)]
    v += ["f32/valu/OT64/TT128", "f32/valu/OT32/TT128", "f32/valu/OT16/TT256", "f32/valu/OT8/TT256"]
    forms = ("RES", "NONE/ps1", "NONE/psN")
    for m in ("bf3", "f16"):
        v += [f"{m}/bf3x/pw8", f"{m}/bf3x/resident/nib1", f"{m}/bf3x/resident/nib2"]
        v += [f"{m}/bf3x/OT{ot}/TT{tt}" for ot in (64, 32) for tt in (256, 128)]
        v += [f"{m}/bf3p/pw8/{e}" for e in ("GELU", "GAMMA_RES", "NONE/ps1", "NONE/psN")]
        v += [f"{m}/bf3t/K{k}/nib{nib}/{f}" for k in (2, 3, 7, 11) for nib in (1, 2) for f in forms]
        shapes = [(128, 1), (256, 1)] if m == "bf3" else [(128, 1), (128, 2), (128, 4), (256, 1), (256, 2)]
        v += [f"{m}/bf3p/TT{tt}/nibs{nb}/{f}" for tt, nb in shapes for f in forms]
    v += [f"f16/pair/K{k}/nib{nib}/NW{4 if nib == 1 else 8}/NH{nh}" for k in (3, 7, 11) for nib in (1, 2) for nh in (1, 2)]
    return v


VARIANTS = _variants()
assert len(VARIANTS) == len(set(VARIANTS)) == 9 + 41 + 50 + 12

Case = namedtuple("Case", "name variant flow prec B Cin Cout T K dil stride epi inp out mean post_silu pre_silu")


def C(name, variant, flow, prec, B, Cin, Cout, T, K, dil=1, stride=1, epi=NONE, inp=IN_F32, out=OUT_Y, mean=False, post_silu=0, pre_silu=0):
    return Case(name, variant, flow, prec, B, Cin, Cout, T, K, dil, stride, epi, inp, out, mean, post_silu, pre_silu)


def _table_a():
    """Tier A / Tier B cases: the smallest shapes that reach each branch (T from the grid threshold, never a multiple of 32; B = 3 on every
    family; dilations 1, 3, 5; K = 13 at the staging limits; T = 1 and T = halo on the small branches)"""
    t = [
        # ---- conv1d_launch (f32 mode)
        C("one_k13", "f32/one/CIN16", CONV, 0, 3, 16, 1, 1037, 13),
        C("one_T1", "f32/one/CIN16", CONV, 0, 1, 16, 1, 1, 13),
        C("one_Thalo", "f32/one/CIN16", CONV, 0, 2, 16, 1, 12, 13),
        C("one_k7", "f32/one/CIN16", CONV, 0, 2, 16, 1, 600, 7),
        C("mfma32_128", "f32/mfma/OT32/TT128", CONV, 0, 3, 32, 48, 300, 3, 3, epi=RES),
        C("mfma32_128_cin24_T1", "f32/mfma/OT32/TT128", CONV, 0, 1, 24, 32, 1, 7),
        C("mfma32_128_Thalo", "f32/mfma/OT32/TT128", CONV, 0, 2, 16, 16, 12, 7, 2, epi=GAMMA_RES),
        C("mfma32_128_k13", "f32/mfma/OT32/TT128", CONV, 0, 1, 16, 20, 200, 13, 10),       # halo 120: 128 + halo <= 256
        C("mfma64_128", "f32/mfma/OT64/TT128", CONV, 0, 2, 32, 250, 4059, 3, 5, epi=GAMMA_RES),  # tall: 32 x 4 x 2 = 256 blocks
        C("mfma64_256_k13", "f32/mfma/OT64/TT256", CONV, 0, 2, 16, 256, 16347, 13, 21),    # wide: 64 x 4 x 2 = 512; halo 252: 256 + halo <= 512
        C("mfma32_256", "f32/mfma/OT32/TT256", CONV, 0, 3, 16, 48, 21779, 3, 1, epi=RES),   # wide, not tall: 86 x 2 x 3 = 516
        C("valu64", "f32/valu/OT64/TT128", CONV, 0, 3, 8, 72, 200, 5, 2, epi=RES),
        C("valu64_k15", "f32/valu/OT64/TT128", CONV, 0, 1, 32, 64, 150, 15),
        C("valu32", "f32/valu/OT32/TT128", CONV, 0, 2, 8, 40, 130, 3, 3, epi=GAMMA_RES),
        C("valu16", "f32/valu/OT16/TT256", CONV, 0, 3, 8, 20, 300, 7),
        C("valu8", "f32/valu/OT8/TT256", CONV, 0, 3, 20, 5, 300, 7, 5, epi=RES),
        C("valu8_T1", "f32/valu/OT8/TT256", CONV, 0, 1, 4, 8, 1, 3),
        C("tconv_mfma", "f32/mfma/OT32/TT128", TCONV, 0, 3, 32, 16, 100, 16, stride=8),
        C("tconv_valu", "f32/valu/OT8/TT256", TCONV, 0, 2, 8, 4, 70, 4, stride=2),
    ]
    for prec in (1, 2):
        m = MODE[prec]
        # ---- conv1d_bf3_impl, f32 input
        t += [
            C(f"{m}_x_pw8", f"{m}/bf3x/pw8", CONV, prec, 3, 136, 40, 200, 1, epi=GAMMA_RES),
            C(f"{m}_x_res1", f"{m}/bf3x/resident/nib1", CONV_P, prec, 3, 16, 24, 600, 7, 3, out=OUT_BOTH),
            C(f"{m}_x_res1_T1", f"{m}/bf3x/resident/nib1", CONV_P, prec, 1, 16, 16, 1, 3, 5, out=OUT_BOTH),
            C(f"{m}_x_res1_loop", f"{m}/bf3x/resident/nib1", CONV, prec, 3, 16, 512, 5500, 3, 1, epi=RES),  # 22 tiles on 21 blocks
            C(f"{m}_x_res2", f"{m}/bf3x/resident/nib2", CONV, prec, 3, 24, 40, 300, 11, 5, epi=RES),
            C(f"{m}_x_res2_Thalo", f"{m}/bf3x/resident/nib2", CONV_P, prec, 2, 32, 32, 50, 11, 5, out=OUT_P),
            C(f"{m}_x_res2_loop", f"{m}/bf3x/resident/nib2", CONV, prec, 2, 32, 512, 4200, 3, 1),            # 33 tiles on 32 blocks
            C(f"{m}_x_32_128", f"{m}/bf3x/OT32/TT128", CONV, prec, 3, 48, 40, 300, 3, 5, epi=GAMMA_RES),
            C(f"{m}_x_32_128_k13", f"{m}/bf3x/OT32/TT128", CONV, prec, 1, 40, 16, 100, 13, 21),               # halo 252
            C(f"{m}_x_64_128", f"{m}/bf3x/OT64/TT128", CONV, prec, 2, 48, 250, 4059, 3, 1, epi=RES),
            C(f"{m}_x_64_256_k13", f"{m}/bf3x/OT64/TT256", CONV, prec, 2, 48, 256, 16347, 13, 21),           # 256 + 252 <= 512
            C(f"{m}_x_32_256", f"{m}/bf3x/OT32/TT256", CONV, prec, 3, 48, 48, 21779, 3, 3),
            C(f"{m}_x_tconv", f"{m}/bf3x/resident/nib2", TCONV, prec, 2, 32, 16, 100, 16, stride=8),
        ]
        # ---- plane input: pointwise
        t += [
            C(f"{m}_pw8_gamma", f"{m}/bf3p/pw8/GAMMA_RES", CONV_P, prec, 3, 128, 40, 200, 1, epi=GAMMA_RES, inp=IN_SPLIT, out=OUT_BOTH),
            C(f"{m}_pw8_none", f"{m}/bf3p/pw8/NONE/ps1", CONV_P, prec, 2, 256, 64, 130, 1, inp=IN_SPLIT, out=OUT_P),
            C(f"{m}_pw8_tconv", f"{m}/bf3p/pw8/NONE/psN", TCONV_P, prec, 3, 128, 24, 100, 2, stride=2, inp=IN_SPLIT),
        ]
        # ---- plane input: thin
        for K, dil, st in ((2, 5, 8), (3, 3, 2), (7, 5, 2), (11, 5, 2)):
            for nib in (1, 2):
                Cin, v = 16 * nib, f"{m}/bf3t/K{K}/nib{nib}"
                t += [
                    C(f"{m}_t_K{K}n{nib}_res", v + "/RES", CONV_P, prec, 3, Cin, Cin if K != 7 else 40, 301, K, dil, epi=RES, inp=IN_SPLIT, out=OUT_BOTH,
                      mean=nib == 2),
                    C(f"{m}_t_K{K}n{nib}_none", v + "/NONE/ps1", CONV_P, prec, 2 if nib == 1 else 1, Cin, 24, (K - 1) * dil if nib == 1 else 1, K, dil,
                      inp=IN_SPLIT, out=OUT_BOTH),
                    C(f"{m}_t_K{K}n{nib}_tconv", v + "/NONE/psN", TCONV_P, prec, 3, Cin, 8, 100, K * st, stride=st, inp=IN_SPLIT),
                ]
        t.append(C(f"{m}_t_loop", f"{m}/bf3t/K3/nib1/RES", CONV_P, prec, 3, 16, 16, 33000, 3, 1, epi=RES, inp=IN_SPLIT))  # 1032 wave tiles on 4 x 256 waves
        # ---- plane input: wide.  TT256: b256 = 32 x 16 x 2 = 1024 blocks; nibs: bf16x3 always 1; f16: 4 where <= 512 blocks and nib % 4 == 0, else 2 where nib is even
        wide = [(128, 1, 48)] + ([(128, 2, 96), (128, 4, 64)] if prec == 2 else [])
        for tt, nb, Cin in wide:
            v = f"{m}/bf3p/TT{tt}/nibs{nb}"
            t += [
                C(f"{m}_w{tt}n{nb}_res", v + "/RES", CONV_P, prec, 3, Cin, 40, 300, 3, 5, epi=RES, inp=IN_SPLIT, out=OUT_BOTH, mean=nb == 1),
                C(f"{m}_w{tt}n{nb}_none_k13", v + "/NONE/ps1", CONV_P, prec, 1, Cin, 32, 200, 13, 5, inp=IN_SPLIT, out=OUT_BOTH),  # halo 60 <= 64
                C(f"{m}_w{tt}n{nb}_tconv", v + "/NONE/psN", TCONV_P, prec, 2, Cin, 16, 100, 4, stride=2, inp=IN_SPLIT),
            ]
        t.append(C(f"{m}_w128n1_thinK13", f"{m}/bf3p/TT128/nibs1/NONE/ps1", CONV_P, prec, 3, 16, 16, 70, 13, 3, inp=IN_SPLIT, out=OUT_BOTH))
        for tt, nb, Cin in [(256, 1, 48)] + ([(256, 2, 64)] if prec == 2 else []):
            v = f"{m}/bf3p/TT{tt}/nibs{nb}"
            t += [
                C(f"{m}_w{tt}n{nb}_res", v + "/RES", CONV_P, prec, 2, Cin, 512, 8192 - 37, 3, 3, epi=RES, inp=IN_SPLIT),
                C(f"{m}_w{tt}n{nb}_none", v + "/NONE/ps1", CONV_P, prec, 2, Cin, 512, 8192 - 37, 2, 1, inp=IN_SPLIT, out=OUT_P),
                C(f"{m}_w{tt}n{nb}_tconv", v + "/NONE/psN", TCONV_P, prec, 2, Cin, 256, 8192 - 37, 4, stride=2, inp=IN_SPLIT),
            ]
    return t


def _table_fn():
    """GELU / tanh on Tier A inputs: every kernel family that carries the two functions"""
    t = [
        C("fn_mfma_gelu", "f32/mfma/OT32/TT128", CONV, 0, 2, 32, 48, 300, 3, epi=GELU),
        C("fn_mfma_tanh", "f32/mfma/OT32/TT128", CONV, 0, 2, 32, 48, 300, 3, epi=TANH),
        C("fn_valu_gelu", "f32/valu/OT8/TT256", CONV, 0, 2, 8, 5, 300, 7, epi=GELU),
        C("fn_valu_tanh", "f32/valu/OT8/TT256", CONV, 0, 2, 8, 5, 300, 7, epi=TANH),
        C("fn_one_tanh", "f32/one/CIN16", CONV, 0, 2, 16, 1, 1037, 13, epi=TANH),
        C("fn_one_gelu", "f32/one/CIN16", CONV, 0, 2, 16, 1, 1037, 13, epi=GELU),
    ]
    for prec in (1, 2):
        m = MODE[prec]
        t += [
            C(f"fn_{m}_x_gelu", f"{m}/bf3x/OT32/TT128", CONV, prec, 2, 48, 40, 300, 3, epi=GELU),
            C(f"fn_{m}_x_tanh", f"{m}/bf3x/OT32/TT128", CONV, prec, 2, 48, 40, 300, 3, epi=TANH),
            C(f"fn_{m}_pw8_gelu", f"{m}/bf3p/pw8/GELU", CONV_P, prec, 3, 128, 40, 200, 1, epi=GELU, inp=IN_SPLIT),
        ]
    return t


PAIR_DILS = {3: (5, 20), 7: (3, 9), 11: (3, 5)}  # a dilation on each side of halo = 32


def _table_pair():
    t = []
    for K, dils in PAIR_DILS.items():
        for nib in (1, 2):
            for nh, dil in enumerate(dils, 1):
                t.append(C(f"pair_K{K}n{nib}h{nh}", f"f16/pair/K{K}/nib{nib}/NW{4 if nib == 1 else 8}/NH{nh}", PAIR, 2, 3, 16 * nib, 16 * nib, 701, K, dil,
                           epi=RES, inp=IN_SPLIT_SILU, out=OUT_BOTH))
    t.append(C("pair_T1", "f16/pair/K3/nib1/NW4/NH1", PAIR, 2, 2, 16, 16, 1, 3, 5, epi=RES, inp=IN_SPLIT_SILU, out=OUT_BOTH))
    t.append(C("pair_Thalo", "f16/pair/K11/nib2/NW8/NH2", PAIR, 2, 2, 32, 32, 50, 11, 5, epi=RES, inp=IN_SPLIT_SILU, out=OUT_BOTH))
    return t


TABLE_A, TABLE_FN, TABLE_PAIR = _table_a(), _table_fn(), _table_pair()
ALL_CASES = TABLE_A + TABLE_FN + TABLE_PAIR
assert len({c.name for c in ALL_CASES}) == len(ALL_CASES)
_ids = lambda t: [c.name for c in t]


# ---------------------------------------------------------------------------------------------------------------- the reference (float64)
def silu64(v):
    return v / (1.0 + np.exp(-v))


def gelu64(v):  # candle Tensor::gelu: the tanh approximation (convnext.rs:115)
    return 0.5 * v * (1.0 + np.tanh(0.7978845608028654 * v * (1.0 + 0.044715 * v * v)))


def ref_conv(x, w, dil):
    """causal conv, stride 1, left zero pad (K-1)*dil (utils/mod.rs:53-62): x [B][Cin][T], w [Cout][Cin][K] float64 -> (y, S) [B][Cout][T],
    y without bias, S = sum |w_i x_i| per output sample.  One (Cout x Cin K) @ (Cin K x T) product per item."""
    B, Cin, T = x.shape
    Cout, _, K = w.shape
    halo = (K - 1) * dil
    W = np.ascontiguousarray(w.reshape(Cout, Cin * K))
    y, S = np.empty((B, Cout, T)), np.empty((B, Cout, T))
    for b in range(B):
        xp = np.zeros((Cin, halo + T))
        xp[:, halo:] = x[b]
        cols = np.stack([xp[:, k * dil:k * dil + T] for k in range(K)], axis=1).reshape(Cin * K, T)
        y[b], S[b] = W @ cols, np.abs(W) @ np.abs(cols)
    return y, S


def ref_tconv(x, w, stride):
    """ConvTranspose1d with right trim K - stride (utils/mod.rs:110-122): x [B][Cin][T], w [Cin][Cout][K] float64 -> (y, S) [B][Cout][T * stride]:
    sample t of the input adds w[:, :, k] x[:, t] to output sample t * stride + k; the last K - stride samples are dropped"""
    B, Cin, T = x.shape
    _, Cout, K = w.shape
    L = (T - 1) * stride + K
    y, S = np.zeros((B, Cout, L)), np.zeros((B, Cout, L))
    for k in range(K):
        wk = np.ascontiguousarray(w[:, :, k].T)
        sl = slice(k, k + (T - 1) * stride + 1, stride)
        y[:, :, sl] += np.matmul(wk, x)
        S[:, :, sl] += np.matmul(np.abs(wk), np.abs(x))
    return y[:, :, :T * stride], S[:, :, :T * stride]


def bf16_rne(v):
    u = np.ascontiguousarray(v, F32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(F32)


def f16_rne(v):  # RNE, saturating at 65504
    return np.clip(np.asarray(v, np.float64), -65504.0, 65504.0).astype(np.float16).astype(np.float64)


def plane_round(v32, prec):
    """the f32 value an activation plane encodes: f16, or bf16 hi + bf16 lo (lo = bf16(v - hi))"""
    v32 = np.ascontiguousarray(v32, F32)
    if prec == 2:
        return np.clip(v32, -65504.0, 65504.0).astype(np.float16).astype(F32)
    hi = bf16_rne(v32)
    return hi + bf16_rne(v32 - hi)


THIRD = F32(1.0 / 3.0)


def mean3_f32(a, b, c):  # k_mean3: ((a + b) + c) * (float)(1/3), all f32
    return ((a.astype(F32) + b.astype(F32)) + c.astype(F32)) * THIRD


# ---------------------------------------------------------------------------------------------------------------- data and the device call
def make_data(c, kind):
    """kind "exact": Tier A lattice; "normal": seeded normal data, w ~ N(0, 1 / (Cin K))"""
    rng = np.random.RandomState(zlib.crc32((c.name + kind).encode()) & 0x7FFFFFFF)
    tr = c.flow in (TCONV, TCONV_P)
    wshape = (c.Cin, c.Cout, c.K) if tr else (c.Cout, c.Cin, c.K)
    yshape = (c.B, c.Cout, c.T * c.stride)
    if kind == "exact":
        lat = lambda shape: (rng.randint(-8, 9, shape) / 8.0).astype(F32)
        d = dict(x=lat((c.B, c.Cin, c.T)), w=lat(wshape), bias=(rng.randint(-64, 65, c.Cout) / 64.0).astype(F32))
        vec = lambda: (rng.choice([0.25, 0.5, 1.0, 2.0], c.Cout) * rng.choice([-1.0, 1.0], c.Cout)).astype(F32)
    else:
        nrm = lambda shape, s=1.0: (rng.standard_normal(shape) * s).astype(F32)
        lat = nrm
        d = dict(x=nrm((c.B, c.Cin, c.T)), w=nrm(wshape, 1.0 / np.sqrt(c.Cin * c.K)), bias=nrm(c.Cout, 0.1))
        vec = lambda: nrm(c.Cout)
    if c.inp >= IN_MEAN3:
        d["x_b"], d["x_c"] = lat((c.B, c.Cin, c.T)), lat((c.B, c.Cin, c.T))
    if c.flow == PAIR:
        d["w2"] = lat(wshape) if kind == "exact" else (rng.standard_normal(wshape) / np.sqrt(c.Cin * c.K)).astype(F32)
        d["bias2"] = d["bias"][::-1].copy()
    if c.epi in (RES, GAMMA_RES) or c.flow == PAIR:
        d["res"] = lat(yshape)
    if c.epi == GAMMA_RES:
        d["gamma"] = vec()
    if c.mean:
        d["mean_a"], d["mean_b"] = lat(yshape), lat(yshape)
    return d


Got = namedtuple("Got", "y planes variant range")
REACHED = {}  # case name -> variant name the entry point reported


def run(c, d, range_check=False):
    cc = _ffi.ConvCase()
    for f in ("flow", "prec", "B", "Cin", "Cout", "T", "K", "dil", "stride", "pre_silu", "epi", "post_silu"):
        setattr(cc, "precision" if f == "prec" else f, int(getattr(c, f)))
    cc.input, cc.outputs, cc.range_check = c.inp, c.out, int(range_check)
    keep = []
    for f in ("x", "x_b", "x_c", "w", "bias", "w2", "bias2", "res", "gamma", "mean_a", "mean_b"):
        if d.get(f) is not None:
            a = np.ascontiguousarray(d[f], F32)
            keep.append(a)
            setattr(cc, f, a.ctypes.data_as(_ffi._F32P))
    y = np.empty((c.B, c.Cout, c.T * c.stride), F32) if c.out & OUT_Y else None
    pl = np.empty((c.B, c.Cout, PAD + c.T), F32) if c.out & OUT_P else None
    name = ctypes.create_string_buffer(96)
    rng = (ctypes.c_uint64 * 2)(0, 0)
    p = lambda a: a.ctypes.data_as(_ffi._F32P) if a is not None else None
    _ffi.check(fishrt.lib().fs_selftest_conv1d(0, ctypes.byref(cc), p(y), p(pl), name, 96, rng))
    variant = name.value.decode()
    if not range_check:
        REACHED[c.name] = variant
    if pl is not None:  # the causal left padding of a plane tensor at the start of a signal
        assert not pl[:, :, :PAD].any(), f"{c.name}: non-zero pad slots in front of the output planes"
        pl = np.ascontiguousarray(pl[:, :, PAD:])
    return Got(y, pl, variant, (int(rng[0]), int(rng[1])))


def producer_values(c, d, kind):
    """float64 values the conv multiplies: (v = the f32 value in front of an optional SiLU, silu?)"""
    if c.inp >= IN_MEAN3:
        v = mean3_f32(d["x"], d["x_b"], d["x_c"])
    else:
        v = d["x"]
    silu = c.inp in (IN_SPLIT_SILU, IN_MEAN3_SILU) or (c.inp == IN_F32 and c.pre_silu)
    return v.astype(np.float64), silu


C_MODE = {0: 2.0 ** -23, 1: 3 * 2.0 ** -16, 2: 2.0 ** -23}
PLANE_REL = {1: 2.0 ** -16, 2: 2.0 ** -11}


def delta_silu(prec):
    return {0: SILU_F32_BOUND, 1: 2.0 ** -15, 2: 2.0 ** -10}[prec]


def reference(c, d, kind):
    """-> dict(y=f32 expectation of the f32 output, p=of the plane output, E=per-sample bound on y (Tier B), Ep=on the planes, v=pre-activation)"""
    xv, silu = producer_values(c, d, kind)
    if silu:
        xv = silu64(xv)
    w = d["w"].astype(np.float64)
    if c.prec == 2 and kind != "exact":  # the f16 mode rounds every matrix operand once
        xv, w = f16_rne(xv), f16_rne(w)
    conv, S = ref_tconv(xv, w, c.stride) if c.flow in (TCONV, TCONV_P) else ref_conv(xv, w, c.dil)
    n = c.Cin * c.K
    v = conv + d["bias"].astype(np.float64)[None, :, None]
    E = (C_MODE[c.prec] + n * 2.0 ** -23 + (delta_silu(c.prec) if silu and kind != "exact" else 0.0)) * S + 2.0 ** -23 * np.abs(v)
    u = 2.0 ** -23
    if c.epi == GELU:
        out = gelu64(v)
    elif c.epi == TANH:
        out = np.tanh(v)
    elif c.epi == GAMMA_RES:
        g, r = d["gamma"].astype(np.float64)[None, :, None], d["res"].astype(np.float64)
        out, E = r + g * v, np.abs(g) * E + u * (np.abs(r) + np.abs(g * v))
    elif c.epi == RES:
        r = d["res"].astype(np.float64)
        out, E = r + v, E + u * (np.abs(r) + np.abs(v))
        if c.mean:
            a, b = d["mean_a"].astype(np.float64), d["mean_b"].astype(np.float64)
            if kind == "exact":  # one f32 add chain and one f32 multiply, mirrored
                out = mean3_f32(d["mean_a"], d["mean_b"], out.astype(F32)).astype(np.float64)
            else:
                E = E / 3 + 4 * u * (np.abs(a) + np.abs(b) + np.abs(r) + np.abs(v))
                out = ((a + b) + out) / 3.0
    else:
        out = v
    r = dict(v=v, y=out.astype(F32), E=E)
    if c.out & OUT_P:
        po, Ep = out, E
        if c.post_silu:  # |silu'| <= 1.1; the device SiLU's own error is below the f32-mode bound
            po, Ep = silu64(out), 1.1 * E + SILU_F32_BOUND * np.abs(silu64(out)) if kind != "exact" else E
        # Tier A: the exact value in the plane format.  Tier B: the UNROUNDED reference -- the format's rounding of the device value is in Ep (a
        # rounded reference would add a second half ulp: the two may sit on either side of a rounding boundary)
        r["p"] = plane_round(po.astype(F32), c.prec) if kind == "exact" else po
        r["Ep"] = Ep + PLANE_REL[c.prec] * (np.abs(po) + Ep) + 2.0 ** -25
    return r


def first_bad(bad):
    i = np.argwhere(bad)
    return f"{int(bad.sum())} of {bad.size} samples, first at [b, o, t] = {i[0].tolist()}, last at {i[-1].tolist()}"


def check_variant(c, got):
    assert got.variant == c.variant, f"{c.name}: the launcher chose {got.variant}, the table says {c.variant}"


@pytest.fixture(scope="module", autouse=True)
def _no_dispatch_knobs():
    set_ = [k for k in KNOBS if k in os.environ]
    assert not set_, f"{set_} change the conv dispatch (read once per process): unset them, this module pins the default dispatch"
    assert fishrt.lib().fs_device_count() >= 1


# ---------------------------------------------------------------------------------------------------------------- Tier A
@pytest.mark.parametrize("c", TABLE_A, ids=_ids(TABLE_A))
def test_tier_a_exact(c):
    d = make_data(c, "exact")
    got = run(c, d)
    check_variant(c, got)
    ref = reference(c, d, "exact")
    assert np.abs(ref["v"]).max() * 64 < 2 ** 24
    if got.y is not None:
        bad = ~(got.y == ref["y"])
        assert not bad.any(), f"{c.name} [{got.variant}] f32 output != reference: {first_bad(bad)}"
    if got.planes is not None:
        bad = ~(got.planes == ref["p"])
        assert not bad.any(), f"{c.name} [{got.variant}] plane output != reference: {first_bad(bad)}"


# ---------------------------------------------------------------------------------------------------------------- Tier B
def _tier_b_cases():
    t = list(TABLE_A)
    # SiLU in front of the conv: pre_silu of the f32-input kernels, SiLU plane producers, SiLU plane outputs
    t += [
        C("b_mfma_silu", "f32/mfma/OT32/TT128", CONV, 0, 3, 32, 48, 300, 3, 3, epi=RES, pre_silu=1),
        C("b_valu_silu", "f32/valu/OT8/TT256", CONV, 0, 3, 20, 5, 300, 7, 5, pre_silu=1),
        C("b_one_silu", "f32/one/CIN16", CONV, 0, 3, 16, 1, 1037, 13, pre_silu=1),
        C("b_tconv_silu", "f32/mfma/OT32/TT128", TCONV, 0, 3, 32, 16, 100, 16, stride=8, pre_silu=1),
    ]
    for prec in (1, 2):
        m = MODE[prec]
        t += [
            C(f"b_{m}_x_silu", f"{m}/bf3x/OT32/TT128", CONV, prec, 3, 48, 40, 300, 3, 5, pre_silu=1),
            C(f"b_{m}_x_res1_silu_out", f"{m}/bf3x/resident/nib1", CONV_P, prec, 3, 16, 24, 600, 7, 3, out=OUT_BOTH, pre_silu=1, post_silu=1),
            C(f"b_{m}_t_silu", f"{m}/bf3t/K7/nib2/RES", CONV_P, prec, 3, 32, 32, 301, 7, 5, epi=RES, inp=IN_SPLIT_SILU, out=OUT_BOTH, post_silu=1),
            C(f"b_{m}_t_mean3", f"{m}/bf3t/K3/nib1/NONE/ps1", CONV_P, prec, 3, 16, 24, 301, 3, 3, inp=IN_MEAN3, out=OUT_BOTH),
            C(f"b_{m}_w_mean3_silu", f"{m}/bf3p/TT128/nibs1/RES", CONV_P, prec, 3, 48, 40, 300, 3, 5, epi=RES, inp=IN_MEAN3_SILU, out=OUT_BOTH, mean=True,
              post_silu=1),
            C(f"b_{m}_tconv_silu", f"{m}/bf3t/K2/nib2/NONE/psN", TCONV_P, prec, 3, 32, 8, 100, 16, stride=8, inp=IN_SPLIT_SILU),
        ]
    return t


TABLE_B = _tier_b_cases()


@pytest.mark.parametrize("c", TABLE_B, ids=_ids(TABLE_B))
def test_tier_b_bound(c):
    assert SILU_F32_BOUND is not None, "SILU_F32_BOUND is not filled in: run test_device_silu_error on the GPU first"
    d = make_data(c, "normal")
    got = run(c, d)
    check_variant(c, got)
    ref = reference(c, d, "normal")
    for what, g, r, E in (("f32", got.y, ref["y"], ref["E"]), ("plane", got.planes, ref.get("p"), ref.get("Ep"))):
        if g is None:
            continue
        err = np.abs(g.astype(np.float64) - r.astype(np.float64))
        E = E + 2.0 ** -24 * np.abs(r)  # the reference's own rounding to f32
        print(f"{c.name} [{got.variant}] {what}: max err {err.max():.3e}, max err / bound {np.max(err / E):.3f}")
        bad = ~(err <= E)
        assert not bad.any(), f"{c.name} [{got.variant}] {what} output outside the derived bound: {first_bad(bad)}"


# ---------------------------------------------------------------------------------------------------------------- measured allowances
def _identity_case(name, variant, flow, prec, C_, **kw):
    return C(name, variant, flow, prec, 2, C_, C_, 2000, 1, **kw)


def _identity(c):
    d = make_data(c, "normal")
    d["x"] = (d["x"] * 4).astype(F32)  # N(0, 16): the SiLU's whole active range
    d["w"] = np.eye(c.Cin, dtype=F32)[:, :, None].copy()
    d["bias"] = np.zeros(c.Cout, F32)
    return d


def test_device_silu_error():
    """the device SiLU against float64 SiLU, read through an identity conv (w = I, bias 0: y = silu(x) exactly in f32 mode).  f32 mode:
    dsilu == the expression of c3_silu; the two matrix modes: c3_silu / c3_silu_fast seen through the bf16x3 split (2^-16) and the f16 format"""
    worst = 0.0
    for c in (_identity_case("silu_mfma", "f32/mfma/OT32/TT128", CONV, 0, 16, pre_silu=1),
              _identity_case("silu_valu", "f32/valu/OT8/TT256", CONV, 0, 8, pre_silu=1)):
        d = _identity(c)
        got = run(c, d)
        check_variant(c, got)
        s = silu64(d["x"].astype(np.float64))
        rel = float(np.max(np.abs(got.y - s) / np.maximum(np.abs(s), 2.0 ** -100)))
        print(f"{c.name}: device SiLU (f32 mode) max relative error {rel:.3e} = {rel * 2 ** 24:.2f} x 2^-24")
        worst = max(worst, rel)
    for prec, lim in ((1, 2.0 ** -15), (2, 2.0 ** -10)):
        m = MODE[prec]
        c = _identity_case(f"silu_{m}_in", f"{m}/bf3x/resident/nib1", CONV_P, prec, 16, pre_silu=1, post_silu=1, out=OUT_BOTH)
        d = _identity(c)
        if prec == 2:
            d["x"] = d["x"].astype(np.float16).astype(F32)
        else:
            d["x"] = bf16_rne(d["x"])
        got = run(c, d)
        check_variant(c, got)
        floor = 2.0 ** -14  # the smallest normal f16: below it the f16 format's error is absolute
        s = silu64(d["x"].astype(np.float64))
        rel_in = float(np.max(np.abs(got.y - s) / np.maximum(np.abs(s), floor)))          # c3_silu, then the operand split
        ss = silu64(got.y.astype(np.float64))
        rel_out = float(np.max(np.abs(got.planes - ss) / np.maximum(np.abs(ss), floor)))  # c3_silu_fast, then the plane format
        print(f"{c.name}: c3_silu through the operand format {rel_in:.3e}, c3_silu_fast through the plane format {rel_out:.3e} (delta_{m} = {lim:.3e})")
        assert rel_in <= lim and rel_out <= lim
    print(f"SILU_F32_MEASURED = {worst:.3e}; asserted SILU_F32_BOUND = {SILU_F32_BOUND}")
    assert SILU_F32_BOUND is not None and worst <= SILU_F32_BOUND


@pytest.mark.parametrize("c", TABLE_FN, ids=_ids(TABLE_FN))
def test_gelu_tanh_function_error(c):
    """Tier A inputs: the pre-activation v is exact, what remains is the device GELU / tanh against the float64 function"""
    d = make_data(c, "exact")
    got = run(c, d)
    check_variant(c, got)
    ref = reference(c, d, "exact")
    v = ref["v"]
    assert np.isfinite(got.y).all()
    if c.epi == TANH:
        assert np.abs(got.y).max() <= 1.0, "|tanh| above 1"
        err = float(np.max(np.abs(got.y - np.tanh(v))))
        print(f"{c.name} [{got.variant}]: tanh max |error| {err:.3e} = {err * 2 ** 24:.2f} x 2^-24 (asserted {TANH_BOUND})")
        assert TANH_BOUND is not None and err <= TANH_BOUND
    else:
        err = float(np.max(np.abs(got.y - gelu64(v)) / np.maximum(np.abs(v), 1.0)))
        print(f"{c.name} [{got.variant}]: GELU max |error| / max(|v|, 1) {err:.3e} = {err * 2 ** 24:.2f} x 2^-24 (asserted {GELU_BOUND})")
        assert GELU_BOUND is not None and err <= GELU_BOUND


# ---------------------------------------------------------------------------------------------------------------- Tier C
def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


SHAPE_PAIRS = [  # (small case, the same conv at another (B, T), the other instantiation)
    ("mfma", C("c_mfma_s", "f32/mfma/OT32/TT128", CONV, 0, 1, 32, 250, 700, 3, 5), C("c_mfma_l", "f32/mfma/OT64/TT128", CONV, 0, 2, 32, 250, 4059, 3, 5)),
    ("bf3_x", C("c_bf3_x_s", "bf3/bf3x/OT32/TT128", CONV, 1, 1, 48, 250, 700, 3, 5), C("c_bf3_x_l", "bf3/bf3x/OT64/TT128", CONV, 1, 2, 48, 250, 4059, 3, 5)),
    ("f16_x", C("c_f16_x_s", "f16/bf3x/OT32/TT128", CONV, 2, 1, 48, 250, 700, 3, 5), C("c_f16_x_l", "f16/bf3x/OT64/TT128", CONV, 2, 2, 48, 250, 4059, 3, 5)),
    ("bf3_w", C("c_bf3_w_s", "bf3/bf3p/TT128/nibs1/RES", CONV_P, 1, 1, 48, 512, 700, 3, 3, epi=RES, inp=IN_SPLIT_SILU, out=OUT_BOTH, post_silu=1),
     C("c_bf3_w_l", "bf3/bf3p/TT256/nibs1/RES", CONV_P, 1, 2, 48, 512, 8192 - 37, 3, 3, epi=RES, inp=IN_SPLIT_SILU, out=OUT_BOTH, post_silu=1)),
    ("f16_w", C("c_f16_w_s", "f16/bf3p/TT128/nibs4/RES", CONV_P, 2, 1, 64, 512, 700, 3, 3, epi=RES, inp=IN_SPLIT_SILU, out=OUT_BOTH, post_silu=1),
     C("c_f16_w_l", "f16/bf3p/TT256/nibs2/RES", CONV_P, 2, 2, 64, 512, 8192 - 37, 3, 3, epi=RES, inp=IN_SPLIT_SILU, out=OUT_BOTH, post_silu=1)),
]


@pytest.mark.parametrize("small,large", [p[1:] for p in SHAPE_PAIRS], ids=[p[0] for p in SHAPE_PAIRS])
def test_tier_c_tile_shape_independent(small, large):
    """the summation order of one output does not depend on the tile shape: item 0's first samples are bit-identical whatever T, B"""
    dl = make_data(large, "normal")
    ds = dict(dl)
    for k in ("x", "res"):
        if k in dl:
            ds[k] = np.ascontiguousarray(dl[k][:small.B, :, :small.T])
    gl, gs = run(large, dl), run(small, ds)
    check_variant(large, gl)
    check_variant(small, gs)
    assert gl.variant != gs.variant
    for a, b in ((gs.y, gl.y), (gs.planes, gl.planes)):
        if a is not None:
            assert np.array_equal(_bits(a), _bits(b[:small.B, :, :small.T]))


@pytest.mark.parametrize("c", TABLE_PAIR, ids=_ids(TABLE_PAIR))
def test_tier_c_fused_pair_equals_two_launches(c):
    """codec_respair_f16 == plane conv with a post_silu plane output, then a RES plane conv (both thin-path kernels held by Tiers A and B)"""
    d = make_data(c, "normal")
    got = run(c, d)
    check_variant(c, got)
    c1 = c._replace(name=c.name + "_c1", flow=CONV_P, epi=NONE, out=OUT_P, post_silu=1)
    g1 = run(c1, dict(x=d["x"], w=d["w"], bias=d["bias"]))
    assert g1.variant == f"f16/bf3t/K{c.K}/nib{c.Cin // 16}/NONE/ps1"
    # the intermediate's planes hold f16 values: splitting them again (no SiLU) reproduces them bit for bit
    c2 = c._replace(name=c.name + "_c2", flow=CONV_P, epi=RES, inp=IN_SPLIT, out=OUT_BOTH, post_silu=1)
    g2 = run(c2, dict(x=g1.planes, w=d["w2"], bias=d["bias2"], res=d["res"]))
    assert g2.variant == f"f16/bf3t/K{c.K}/nib{c.Cin // 16}/RES"
    assert np.array_equal(_bits(got.y), _bits(g2.y)) and np.array_equal(_bits(got.planes), _bits(g2.planes))
    assert np.isfinite(got.y).all()


@pytest.mark.parametrize("prec,wide", [(1, False), (2, False), (1, True), (2, True)], ids=["bf3_thin", "f16_thin", "bf3_wide", "f16_wide"])
def test_tier_c_mean_fold_equals_mean3(prec, wide):
    """((mean_a + mean_b) + (res + conv)) / 3 folded into the RES epilogue == k_mean3 (numpy f32: IEEE adds and one multiply) and ==
    k_mean3_planes (read out through an identity conv) on the un-folded output"""
    m = MODE[prec]
    Cin, v = (48, f"{m}/bf3p/TT128/nibs1/RES") if wide else (32, f"{m}/bf3t/K3/nib2/RES")
    for post_silu in (0, 1):
        base = C(f"c_fold_{m}_{int(wide)}_{post_silu}", v, CONV_P, prec, 3, Cin, 32, 301, 3, 5, epi=RES, inp=IN_SPLIT_SILU, out=OUT_BOTH, mean=True,
                 post_silu=post_silu)
        d = make_data(base, "normal")
        fold = run(base, d)
        check_variant(base, fold)
        plain = run(base._replace(name=base.name + "_plain", mean=False), {k: a for k, a in d.items() if not k.startswith("mean_")})
        assert np.array_equal(_bits(fold.y), _bits(mean3_f32(d["mean_a"], d["mean_b"], plain.y)))
        # k_mean3_planes on (mean_a, mean_b, plain.y), SiLU as the fold's, read back by y = I * planes
        ident = C(base.name + "_ident", f"{m}/bf3p/TT128/nibs{prec}/NONE/ps1", CONV_P, prec, 3, 32, 32, 301, 1, inp=IN_MEAN3_SILU if post_silu else IN_MEAN3)
        gi = run(ident, dict(x=d["mean_a"], x_b=d["mean_b"], x_c=plain.y, w=np.eye(32, dtype=F32)[:, :, None].copy(), bias=np.zeros(32, F32)))
        check_variant(ident, gi)
        assert np.array_equal(_bits(fold.planes), _bits(gi.y))


TWIN_A = [c for c in TABLE_A if c.prec == 2 and c.B * c.Cout * c.T <= 100_000]
# (the pair on normal data only: on the Tier A lattice its second conv reaches v < -17.4, where silu(v) is below 2^-24 and is counted, rightly)
TWIN_CASES = [(c, k) for c in TWIN_A for k in ("exact", "normal")] + [(c, "normal") for c in TABLE_PAIR[:4]]


def _operand_counts(*arrays):
    a = np.concatenate([np.abs(np.asarray(v, np.float64)).ravel() for v in arrays])
    return int((a > 65504.0).sum()), int(((a != 0) & (a < 2.0 ** -24)).sum())


@pytest.mark.parametrize("c,kind", TWIN_CASES, ids=[f"{c.name}-{k}" for c, k in TWIN_CASES])
def test_tier_c_range_checked_twin(c, kind):
    """f16 mode: the range-checked twin == the plain kernels bit for bit, both counters at 0 (nothing in the data is out of range: the one
    normal draw in ~10^7 that falls below 2^-24 is lifted to 2^-20 first)"""
    d = make_data(c, kind)
    for k in ("x", "w", "w2"):
        if k in d:
            tiny = (d[k] != 0) & (np.abs(d[k]) < 2.0 ** -20)
            d[k][tiny] = np.copysign(F32(2.0 ** -20), d[k][tiny])
    plain, twin = run(c, d), run(c, d, range_check=True)
    assert twin.variant == "chk/" + plain.variant == "chk/" + c.variant
    for a, b in ((plain.y, twin.y), (plain.planes, twin.planes)):
        if a is not None:
            assert np.array_equal(_bits(a), _bits(b))
    assert _operand_counts(d["x"], d["w"], d.get("w2", 0.0)) == (0, 0)
    assert twin.range == (0, 0), twin.range


@pytest.mark.parametrize("which", ["saturated", "flushed"])
def test_tier_c_range_counters_count_planted_operands(which):
    """operands above 65504 (activations, converted once by codec_act_split) / below 2^-24 (weights, converted once by codec_pack_bf3) are counted
    exactly; the f32 output keeps the conversions of the epilogue out of the count"""
    c = C("c_range_" + which, "f16/bf3t/K3/nib2/NONE/ps1", CONV_P, 2, 3, 32, 24, 301, 3, 3, inp=IN_SPLIT)
    d = make_data(c, "normal")
    rng = np.random.RandomState(7)
    if which == "saturated":
        idx = rng.choice(d["x"].size, 37, replace=False)
        d["x"].reshape(-1)[idx] = rng.choice([-1.0, 1.0], 37) * rng.uniform(65505.0, 3e5, 37)
        want = (37, 0)
    else:
        idx = rng.choice(d["w"].size, 23, replace=False)
        d["w"].reshape(-1)[idx] = rng.choice([-1.0, 1.0], 23) * rng.uniform(1e-12, 5.9e-8, 23)
        want = (0, 23)
    assert _operand_counts(d["x"], d["w"]) == want
    got = run(c, d, range_check=True)
    assert got.variant == "chk/" + c.variant and got.range == want, (got.variant, got.range)
    assert np.isfinite(got.y).all()


# ---------------------------------------------------------------------------------------------------------------- coverage
def test_every_listed_variant_is_reached():
    """runs last: the names the entry point reported for the tables' cases are exactly VARIANTS (cases not run yet in this process -- a
    filtered run -- are launched here, without their reference)"""
    for c in ALL_CASES:
        if c.name not in REACHED:
            run(c, make_data(c, "exact"))
    wrong = {c.name: (REACHED[c.name], c.variant) for c in ALL_CASES if REACHED[c.name] != c.variant}
    assert not wrong, wrong
    reached = {REACHED[c.name] for c in ALL_CASES}
    assert reached == set(VARIANTS), (sorted(set(VARIANTS) - reached), sorted(reached - set(VARIANTS)))
