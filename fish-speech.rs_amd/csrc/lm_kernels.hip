// Dual-AR transformer kernels for gfx950 (MI355X): the batch-1 token path (one GEMV kernel per node), the embedding and weight
// fill / convert kernels and a few engine utilities.  The MFMA row path (skinny GEMMs over activation rows) is in lm_gemm.hip, the
// attention kernels of both paths in lm_attn.hip, the on-device samplers in lm_sample.hip; the device helpers the four files use are
// in lm_dev.h.
//
// Every kernel here is HBM/latency-bound weight streaming (a 1024x1024 bf16 matrix is 2 MB; one CU can keep
// ~32 KB in flight), so the design rules are (MI355X guide, "GEMV / M <= 16 decode weights"):
//   * weights go global -> VGPR directly as 16-B/lane non-temporal loads, all of a wave's loads issued before
//     the first use (no LDS round trip: nothing is shared between waves);
//   * one wave = 64 lanes owns whole rows; the activation slice a lane needs (K/64 floats) is loaded once into
//     registers and reused for every row of the wave;
//   * RMSNorm, RoPE, SwiGLU, residual adds, KV append and the attention combine are fused into the GEMV that
//     produces / consumes them, so a transformer block is 5 launches (4 for the fast decoder);
//   * reductions are wave64 shuffles; no atomics, fixed summation order => run-to-run deterministic tokens.
// Reference semantics implemented: fish_speech_core/lib/lm/dual_ar.rs:118-165 (FFN), :239-249 (rope_i),
// :252-279 (SDPA), :281-384 (Attention::forward), :429-440 (block), :532-567 (embed), :629-631 (head).
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/fishrt.h"
#include "fs_common.h"
#include "fs_synth.h"
#include "lm_kernels.h"
#include "lm_dev.h"

namespace fs {

// ------------------------------------------------------------------------------------------------ device helpers
// per-row dequantisation scale (fp8 only; other weight types carry none)
template <typename WT>
__device__ __forceinline__ float row_scale(const float* __restrict__ ws, int row) {
    if constexpr (std::is_same<WT, fp8_t>::value) return ws[row];
    else return 1.0f;
}

// A wave's view of a length-K vector / weight row: chunk c covers elements [c*64*EPL, (c+1)*64*EPL), lane l owns
// EPL consecutive elements starting at c*64*EPL + l*EPL.
template <typename WT, int K, bool NT = true>
struct Row {
    static constexpr int EPL = WTr<WT>::EPL;
    static constexpr int CH = 64 * EPL;
    static constexpr int NCH = (K + CH - 1) / CH;
    static constexpr int NX = NCH * EPL;
    using vec = typename WTr<WT>::vec;

    __device__ static __forceinline__ void load_x(const float* __restrict__ x, int lane, float (&xr)[NX]) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int base = c * CH + lane * EPL;
            if (base < K) {
#pragma unroll
                for (int i = 0; i < EPL; i += 4) {
                    const float4 t = *reinterpret_cast<const float4*>(x + base + i);
                    xr[c * EPL + i] = t.x; xr[c * EPL + i + 1] = t.y; xr[c * EPL + i + 2] = t.z; xr[c * EPL + i + 3] = t.w;
                }
            } else {
#pragma unroll
                for (int i = 0; i < EPL; ++i) xr[c * EPL + i] = 0.f;
            }
        }
    }
    __device__ static __forceinline__ void load_w(const WT* __restrict__ row, int lane, vec (&wv)[NCH]) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int base = c * CH + lane * EPL;
            if (base < K) wv[c] = NT ? ld_stream(reinterpret_cast<const vec*>(row + base)) : *reinterpret_cast<const vec*>(row + base);
            else wv[c] = vec(0);
        }
    }
    __device__ static __forceinline__ float dot(const vec (&wv)[NCH], const float (&xr)[NX]) {
        float acc = 0.f;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            float f[EPL];
            WTr<WT>::unpack(wv[c], f);
#pragma unroll
            for (int i = 0; i < EPL; ++i) acc = fmaf(f[i], xr[c * EPL + i], acc);
        }
        return acc;
    }
    // in-register RMSNorm of the wave's x slice: x / sqrt(mean(x^2) + eps) * w   (candle_nn::RmsNorm); `nr` = the
    // lane's slice of the norm weight, loaded by the caller together with x so that no load sits behind the reduction
    __device__ static __forceinline__ void rmsnorm(float (&xr)[NX], const float (&nr)[NX], float eps) {
        float ss = 0.f;
#pragma unroll
        for (int i = 0; i < NX; ++i) ss = fmaf(xr[i], xr[i], ss);
        const float d = sqrtf(wave_sum(ss) / (float)K + eps);
#pragma unroll
        for (int i = 0; i < NX; ++i) xr[i] = (xr[i] / d) * nr[i];
    }
};

// ------------------------------------------------------------------------------------------------ qkv + rope + kv append
// One wave per ROW of Wqkv (measured: a 2 MB GEMV node costs 2.4 us at one row per wave, 3.1 us at two -- the wave count, not
// the byte count, sets the latency of these small nodes); the two rows of an interleaved-RoPE pair (2p, 2p+1) sit in adjacent
// waves of one block and meet through 8 bytes of LDS.  Position, page and cos/sin are requested while the weights are in
// flight, so the epilogue has no dependent load left.
template <typename WT, int K, int WAVES, bool NT>
__global__ __launch_bounds__(WAVES * 64) void k_qkv(const float* __restrict__ x, const float* __restrict__ norm_w, float eps,
                                                    const WT* __restrict__ W, const float* __restrict__ cos_t,
                                                    const float* __restrict__ sin_t, const SeqState* __restrict__ state,
                                                    int pos_static, int rope_static, float* __restrict__ q_out, KVView kv,
                                                    int H, int Hk, int Dh, const float* __restrict__ wscale) {
    using R = Row<WT, K, NT>;
    using KT = KVT<WT>;
    static_assert(WAVES % 2 == 0, "row pairs live in one block");
    __shared__ float dots[WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n_rows = (H + 2 * Hk) * Dh;
    const int row = min(blockIdx.x * WAVES + wave, n_rows - 1);  // clamped (the grid covers whole pairs; n_rows is even)
    // small L2-resident vectors FIRST (vmcnt retires in order: a load issued after the weight stream would wait for it),
    // then the weight stream, then the position-dependent scalar chain (pos -> page / cos / sin, only needed by the
    // epilogue); the RMSNorm math and that chain overlap the weights' HBM flight
    float xr[R::NX], nr[R::NX];
    R::load_x(x, lane, xr);
    R::load_x(norm_w, lane, nr);
    const float sc = row_scale<WT>(wscale, row);  // fp8: requested in front of the weight stream (an L2 round trip at the tail otherwise)
    typename R::vec wv[R::NCH];
    R::load_w(W + (size_t)row * K, lane, wv);
    FS_ISSUE_FENCE();
    const int r0 = row & ~1, qdim = H * Dh, kdim = Hk * Dh, half = Dh / 2;
    const int pos = state ? state->pos : pos_static;
    const int rpos = state ? pos + state->rope_off : rope_static;
    float c = 1.f, s = 0.f;
    KT* dst = nullptr;
    if (r0 < qdim + kdim) {
        const int j = (r0 % Dh) / 2;
        c = cos_t[(size_t)rpos * half + j];
        s = sin_t[(size_t)rpos * half + j];
    }
    if (r0 >= qdim) {
        const int rk = (r0 - qdim) % kdim, g = rk / Dh, dd = rk % Dh;
        dst = kv_addr<KT>(r0 < qdim + kdim ? kv.k : kv.v, kv.page_table, pos, g, Hk, Dh) + dd;
    }
    R::rmsnorm(xr, nr, eps);
    const float d = wave_sum(R::dot(wv, xr)) * sc;
    if (lane == 0) dots[wave] = d;
    __syncthreads();
    if (lane != 0 || (wave & 1) || blockIdx.x * WAVES + wave >= n_rows) return;
    const float a = dots[wave], b = dots[wave + 1];
    if (r0 < qdim + kdim) {  // rope_i on the pair (2j, 2j+1) of its head (dual_ar.rs:246-247)
        const float o0 = a * c - b * s, o1 = a * s + b * c;
        if (r0 < qdim) { q_out[r0] = o0; q_out[r0 + 1] = o1; }
        else { dst[0] = WTr<KT>::from_f32(o0); dst[1] = WTr<KT>::from_f32(o1); }
    } else {
        dst[0] = WTr<KT>::from_f32(a); dst[1] = WTr<KT>::from_f32(b);
    }
}

// ------------------------------------------------------------------------------------------------ wo + residual
// Prologue (whole block, result in LDS): either combine the per-chunk partials of k_attn_decode, or -- FUSED, used by
// the fast decoder whose KV length is <= 8 -- run the whole attention for all heads redundantly per block.
// Body: one wave per output row: x[r] += Wo[r,:] . attn   (dual_ar.rs:383,437)
template <typename WT, int K, int WAVES, bool FUSED, int DH, bool NT>
__global__ __launch_bounds__(WAVES * 64) void k_wo(const float* __restrict__ part, int n_chunks_max, int chunk,
                                                   const SeqState* __restrict__ state, const float* __restrict__ q, KVView kv,
                                                   int fused_T, const WT* __restrict__ W, float* __restrict__ x, int H, int Hk,
                                                   int n_rows, const float* __restrict__ wscale, int nc_launch) {
    using R = Row<WT, K, NT>;
    using KT = KVT<WT>;
    constexpr int NTH = WAVES * 64;
    constexpr int EPL = WTr<KT>::EPL;   // the prologue reads the KV cache (KT), the body streams W (WT)
    using vec = typename WTr<KT>::vec;
    static_assert(K % 4 == 0 && DH % 16 == 0, "geometry");
    __shared__ __attribute__((aligned(16))) float attn[K];
    __shared__ float wl[FUSED ? 32 * 8 : 32 * 128];
    __shared__ float ml[FUSED ? 2 : 2 * 32 * 128];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blockIdx.x * WAVES + wave;
    const int n_rep = H / Hk;
    typename R::vec wv[R::NCH];
    const float xres = (row < n_rows && lane == 0) ? x[row] : 0.f;
    const float sc = row_scale<WT>(wscale, min(row, n_rows - 1));  // fp8: in front of the weight stream
    // Few, wide prologue loads (the texture-address unit retires one wave-instruction per ~16 cycles whatever its width),
    // all issued before the weight stream (vmcnt retires in issue order).
    if (!FUSED && nc_launch <= 8) {
        // short sequences (<= 8 chunks): every thread merges the chunks of its own head in registers -- its {m, l} pairs and its
        // four output dims of every chunk are 16 independent loads issued before the weight stream; no LDS hop, no barrier
        // until the result vector is complete (same arithmetic, in the same order, as the general path below)
        const int e4 = threadIdx.x * 4;
        const bool has_o = e4 < K;
        const int ho = (has_o ? e4 : 0) / DH, ddo = e4 % DH;
        const float* pb = part + (size_t)ho * n_chunks_max * (DH + 2);
        float2 mlv[8];
        float4 ov[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int cc = min(c, nc_launch - 1);
            mlv[c] = *reinterpret_cast<const float2*>(pb + (size_t)cc * (DH + 2) + DH);
            ov[c] = *reinterpret_cast<const float4*>(pb + (size_t)cc * (DH + 2) + ddo);
        }
        R::load_w(W + (size_t)min(row, n_rows - 1) * K, lane, wv);
        FS_ISSUE_FENCE();
        const int T = state->pos + 1;
        const int nc = (T + chunk - 1) / chunk;  // chunks k_attn_decode produced (<= nc_launch)
        float mn = -1e30f;
#pragma unroll
        for (int c = 0; c < 8; ++c) if (c < nc) mn = fmaxf(mn, mlv[c].x);
        float L = 0.f;
#pragma unroll
        for (int c = 0; c < 8; ++c) if (c < nc) L += mlv[c].y * __expf(mlv[c].x - mn);
        const float inv = 1.f / L;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int c = 0; c < 8; ++c)
            if (c < nc) {
                const float wj = __expf(mlv[c].x - mn) * inv;
                acc.x = fmaf(wj, ov[c].x, acc.x); acc.y = fmaf(wj, ov[c].y, acc.y);
                acc.z = fmaf(wj, ov[c].z, acc.z); acc.w = fmaf(wj, ov[c].w, acc.w);
            }
        if (has_o) *reinterpret_cast<float4*>(&attn[e4]) = acc;
    } else if (!FUSED) {
        // every prologue load is addressed from launch-time constants only (nc_launch = chunks this graph bucket launches),
        // so nothing waits for state->pos before the weight stream is requested; chunks >= nc hold stale (finite) partials of
        // earlier frames and are masked below
        // (a) {m, l} of every (head, chunk) + the first four chunks' o values (float4 per thread per chunk)
        const int e0 = threadIdx.x;
        const int eh = e0 / nc_launch, ec = e0 % nc_launch;
        const bool in_ml = e0 < H * nc_launch;
        const float2 mv = *reinterpret_cast<const float2*>(part + ((size_t)(in_ml ? eh : 0) * n_chunks_max + ec) * (DH + 2) + DH);
        const int e4 = threadIdx.x * 4;  // this thread's 4 consecutive attn elements (K <= 4 * NTH for every supported K here)
        const bool has_o = e4 < K;
        const int ho = (has_o ? e4 : 0) / DH, ddo = e4 % DH;
        const float* po = part + (size_t)ho * n_chunks_max * (DH + 2) + ddo;
        float4 v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = *reinterpret_cast<const float4*>(po + (size_t)min(j, nc_launch - 1) * (DH + 2));
        R::load_w(W + (size_t)min(row, n_rows - 1) * K, lane, wv);  // clamped, not predicated: a predicated load costs a wait
        FS_ISSUE_FENCE();
        const int T = state->pos + 1;
        const int nc = (T + chunk - 1) / chunk;  // chunks k_attn_decode produced (<= nc_launch)
        if (in_ml && ec < nc) { ml[2 * (eh * 128 + ec)] = mv.x; ml[2 * (eh * 128 + ec) + 1] = mv.y; }
        for (int e = threadIdx.x + NTH; e < H * nc_launch; e += NTH) {  // only when H * nc_launch > NTH (very long sequences)
            const int h = e / nc_launch, c = e % nc_launch;
            if (c >= nc) continue;
            const float2 t2 = *reinterpret_cast<const float2*>(part + ((size_t)h * n_chunks_max + c) * (DH + 2) + DH);
            ml[2 * (h * 128 + c)] = t2.x;
            ml[2 * (h * 128 + c) + 1] = t2.y;
        }
        __syncthreads();
        // (b) per head: softmax-merge weights wl[h][c] = exp(m_c - M) / sum_c l_c exp(m_c - M)
        for (int h = threadIdx.x; h < H; h += NTH) {
            float mn = -1e30f;
            for (int c = 0; c < nc; ++c) mn = fmaxf(mn, ml[2 * (h * 128 + c)]);
            float L = 0.f;
            for (int c = 0; c < nc; ++c) L += ml[2 * (h * 128 + c) + 1] * __expf(ml[2 * (h * 128 + c)] - mn);
            const float inv = 1.f / L;
            for (int c = 0; c < nc; ++c) wl[h * 128 + c] = __expf(ml[2 * (h * 128 + c)] - mn) * inv;
        }
        __syncthreads();
        // (c) attn[e] = sum_c wl[h][c] * o[h][c][dd]
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int c0 = 0; c0 < nc; c0 += 4) {
            if (c0 > 0) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    v[j] = (has_o && c0 + j < nc) ? *reinterpret_cast<const float4*>(po + (size_t)(c0 + j) * (DH + 2))
                                                  : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (c0 + j < nc) {
                    const float wj = wl[ho * 128 + c0 + j];
                    acc.x = fmaf(wj, v[j].x, acc.x); acc.y = fmaf(wj, v[j].y, acc.y);
                    acc.z = fmaf(wj, v[j].z, acc.z); acc.w = fmaf(wj, v[j].w, acc.w);
                }
        }
        if (has_o) *reinterpret_cast<float4*>(&attn[e4]) = acc;
    } else if (DH == 64 && K == 4 * NTH && H * 16 == NTH) {
        // Fast decoder, Fish geometry (16 heads x 64 dims, 256 threads): head h is produced AND consumed by the 16 lanes
        // tid = 16h .. 16h+15 (one DPP row of one wave): scores[h][t] by lane pair (2t, 2t+1) (32 dims each), then every lane of
        // the row does softmax . V for 4 of the head's 64 dims.  The score exchange stays inside the wave (8 floats per head in
        // LDS, no block barrier: a wave's LDS operations execute in order) -- one __syncthreads() less than the general path.
        const float scale = 1.0f / sqrtf((float)DH);
        const KT* kbase = reinterpret_cast<const KT*>(kv.k);
        const KT* vbase = reinterpret_cast<const KT*>(kv.v);
        constexpr int QD = DH / 2;
        const int hh = threadIdx.x >> 4, t1 = (threadIdx.x >> 1) & 7, sl = threadIdx.x & 1;
        const int g = hh / n_rep;
        vec kvv[QD / EPL];
        float4 qv[QD / 4];
        {
            const KT* kp = kbase + ((size_t)g * KV_PAGE + t1) * DH + sl * QD;  // rows t >= fused_T are stale but in bounds; masked below
#pragma unroll
            for (int i = 0; i < QD / EPL; ++i) kvv[i] = *reinterpret_cast<const vec*>(kp + i * EPL);
#pragma unroll
            for (int i = 0; i < QD / 4; ++i) qv[i] = *reinterpret_cast<const float4*>(q + hh * DH + sl * QD + i * 4);
        }
        const int ddv = (threadIdx.x & 15) * 4;  // this lane's 4 output dims of head hh
        float vf4[8][4];
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const KT* vp = vbase + ((size_t)g * KV_PAGE + t) * DH + ddv;
#pragma unroll
            for (int i = 0; i < 4; ++i) vf4[t][i] = WTr<KT>::to_f32(vp[i]);
        }
        R::load_w(W + (size_t)min(row, n_rows - 1) * K, lane, wv);
        FS_ISSUE_FENCE();
        {
            float acc = 0.f;
#pragma unroll
            for (int i = 0; i < QD / EPL; ++i) {
                float kf[EPL];
                WTr<KT>::unpack(kvv[i], kf);
#pragma unroll
                for (int j = 0; j < EPL; j += 4) {
                    const float4 qq = qv[(i * EPL + j) / 4];
                    acc = fmaf(qq.x, kf[j] * scale, acc); acc = fmaf(qq.y, kf[j + 1] * scale, acc);
                    acc = fmaf(qq.z, kf[j + 2] * scale, acc); acc = fmaf(qq.w, kf[j + 3] * scale, acc);
                }
            }
            acc = group_sum<2>(acc);
            if (sl == 0) wl[hh * 8 + t1] = acc;
        }
        // (same wave: no block barrier)
        float mn = -1e30f;
#pragma unroll
        for (int t = 0; t < 8; ++t) if (t < fused_T) mn = fmaxf(mn, wl[hh * 8 + t]);
        float L = 0.f, O[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 8; ++t)
            if (t < fused_T) {
                const float p = __expf(wl[hh * 8 + t] - mn);
                L += p;
#pragma unroll
                for (int i = 0; i < 4; ++i) O[i] = fmaf(p, vf4[t][i], O[i]);
            }
        const float inv = 1.f / L;
        *reinterpret_cast<float4*>(&attn[threadIdx.x * 4]) = make_float4(O[0] * inv, O[1] * inv, O[2] * inv, O[3] * inv);
    } else {
        // Fast decoder: <= 8 cached tokens, all in page 0 of this layer's private KV page (no page-table lookup).
        // step 1: scores[h][t], TWO threads per (h, t) (DH/2 dims each, DPP pair-sum); step 2: softmax . V with one
        // thread per EPL consecutive dims (one 16-B V load per token).
        const float scale = 1.0f / sqrtf((float)DH);
        const KT* kbase = reinterpret_cast<const KT*>(kv.k);
        const KT* vbase = reinterpret_cast<const KT*>(kv.v);
        constexpr int QD = DH / 2;  // dims per step-1 thread
        const int e1 = threadIdx.x >> 1, sl = threadIdx.x & 1;
        const bool has_s = e1 < H * fused_T;
        const int h1 = has_s ? e1 / fused_T : 0, t1 = has_s ? e1 % fused_T : 0;
        vec kvv[QD / EPL];
        float4 qv[QD / 4];
        {
            const KT* kp = kbase + ((size_t)(h1 / n_rep) * KV_PAGE + t1) * DH + sl * QD;
#pragma unroll
            for (int i = 0; i < QD / EPL; ++i) kvv[i] = *reinterpret_cast<const vec*>(kp + i * EPL);
#pragma unroll
            for (int i = 0; i < QD / 4; ++i) qv[i] = *reinterpret_cast<const float4*>(q + h1 * DH + sl * QD + i * 4);
        }
        const int ev = threadIdx.x * EPL;  // this thread's EPL consecutive attn elements
        const bool has_v = ev < K;
        const int hv = (has_v ? ev : 0) / DH, ddv = ev % DH;
        vec vvv[8];
#pragma unroll
        for (int t = 0; t < 8; ++t)  // unconditional (rows t >= fused_T of the page are stale but in bounds; masked at use)
            vvv[t] = *reinterpret_cast<const vec*>(vbase + ((size_t)(hv / n_rep) * KV_PAGE + t) * DH + ddv);
        R::load_w(W + (size_t)min(row, n_rows - 1) * K, lane, wv);
        FS_ISSUE_FENCE();
        {
            float acc = 0.f;
#pragma unroll
            for (int i = 0; i < QD / EPL; ++i) {
                float kf[EPL];
                WTr<KT>::unpack(kvv[i], kf);
#pragma unroll
                for (int j = 0; j < EPL; j += 4) {
                    const float4 qq = qv[(i * EPL + j) / 4];
                    acc = fmaf(qq.x, kf[j] * scale, acc); acc = fmaf(qq.y, kf[j + 1] * scale, acc);
                    acc = fmaf(qq.z, kf[j + 2] * scale, acc); acc = fmaf(qq.w, kf[j + 3] * scale, acc);
                }
            }
            acc = group_sum<2>(acc);
            if (has_s && sl == 0) wl[h1 * 8 + t1] = acc;
        }
        __syncthreads();
        if (has_v) {
            float mn = -1e30f;
#pragma unroll
            for (int t = 0; t < 8; ++t) if (t < fused_T) mn = fmaxf(mn, wl[hv * 8 + t]);
            float L = 0.f, O[EPL];
#pragma unroll
            for (int i = 0; i < EPL; ++i) O[i] = 0.f;
#pragma unroll
            for (int t = 0; t < 8; ++t)
                if (t < fused_T) {
                    const float p = __expf(wl[hv * 8 + t] - mn);
                    L += p;
                    float vf[EPL];
                    WTr<KT>::unpack(vvv[t], vf);
#pragma unroll
                    for (int i = 0; i < EPL; ++i) O[i] = fmaf(p, vf[i], O[i]);
                }
            const float inv = 1.f / L;
#pragma unroll
            for (int i = 0; i < EPL; ++i) attn[ev + i] = O[i] * inv;
        }
    }
    __syncthreads();
    if (row >= n_rows) return;
    float xr[R::NX];
    R::load_x(attn, lane, xr);
    const float d = wave_sum(R::dot(wv, xr)) * sc;
    if (lane == 0) x[row] = xres + d;
}

// ------------------------------------------------------------------------------------------------ SwiGLU up
// One wave per (w1[r], w3[r]) pair of the row-interleaved W13: act[r] = silu(w1[r].xn) * (w3[r].xn)
template <typename WT, int K, int WAVES, bool NT>
__global__ __launch_bounds__(WAVES * 64) void k_ffn_up(const float* __restrict__ x, const float* __restrict__ norm_w,
                                                       float eps, const WT* __restrict__ W13, float* __restrict__ act,
                                                       int inter, const float* __restrict__ wscale) {
    using R = Row<WT, K, NT>;
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (r >= inter) return;
    float xr[R::NX], nr[R::NX];
    R::load_x(x, lane, xr);
    R::load_x(norm_w, lane, nr);
    const float s1 = row_scale<WT>(wscale, 2 * r), s3 = row_scale<WT>(wscale, 2 * r + 1);  // fp8: in front of the weight stream
    typename R::vec w1[R::NCH], w3[R::NCH];
    R::load_w(W13 + (size_t)(2 * r) * K, lane, w1);
    R::load_w(W13 + (size_t)(2 * r + 1) * K, lane, w3);
    FS_ISSUE_FENCE();
    R::rmsnorm(xr, nr, eps);
    const float a = wave_sum(R::dot(w1, xr)) * s1;
    const float b = wave_sum(R::dot(w3, xr)) * s3;
    if (lane == 0) act[r] = (a / (1.f + __expf(-a))) * b;  // candle silu = x / (1 + exp(-x))
}

// ------------------------------------------------------------------------------------------------ down + residual
// x[r] += W2[r,:] . act with K = inter split over the KS waves of a block (one row per block): every wave streams
// K/KS contiguous weights against its own slice of `act` (registers, straight from L2), the KS partial sums meet in LDS
// and are added in a fixed order.
template <typename WT, int K, int KS, bool NT>
__global__ __launch_bounds__(KS * 64) void k_ffn_down(const float* __restrict__ act, const WT* __restrict__ W2,
                                                      float* __restrict__ x, int n_rows, const float* __restrict__ wscale) {
    using R = Row<WT, K / KS, NT>;
    __shared__ float red[KS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blockIdx.x;
    const float xres = (threadIdx.x == 0) ? x[row] : 0.f;
    const float sc = row_scale<WT>(wscale, row);  // fp8: in front of the weight stream
    float xr[R::NX];
    R::load_x(act + wave * (K / KS), lane, xr);
    typename R::vec wv[R::NCH];
    R::load_w(W2 + (size_t)row * K + wave * (K / KS), lane, wv);
    FS_ISSUE_FENCE();
    const float d = wave_sum(R::dot(wv, xr));
    if (lane == 0) red[wave] = d;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = red[0];
#pragma unroll
        for (int i = 1; i < KS; ++i) t += red[i];
        x[row] = xres + t * sc;
    }
}

// ------------------------------------------------------------------------------------------------ norm + head GEMV
template <typename WT, int K, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void k_head(const float* __restrict__ x, const float* __restrict__ norm_w, float eps,
                                                     const WT* __restrict__ W, int n_rows, float* __restrict__ logits,
                                                     const float* __restrict__ wscale) {
    using R = Row<WT, K>;
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (r >= n_rows) return;
    float xr[R::NX], nr[R::NX];
    R::load_x(x, lane, xr);
    R::load_x(norm_w, lane, nr);
    const float sc = row_scale<WT>(wscale, r);  // fp8: in front of the weight stream
    typename R::vec wv[R::NCH];
    R::load_w(W + (size_t)r * K, lane, wv);
    FS_ISSUE_FENCE();
    R::rmsnorm(xr, nr, eps);
    const float d = wave_sum(R::dot(wv, xr)) * sc;
    if (lane == 0) logits[r] = d;
}

// ------------------------------------------------------------------------------------------------ embedding (embed_tokens: lm_dev.h)
template <typename WT>
__global__ void k_embed(const WT* __restrict__ tok_emb, const WT* __restrict__ cb_emb, int dim, int n_cb, int cb_size,
                        const SampleCfg* __restrict__ cfg, const uint32_t* __restrict__ prompt, SeqState* __restrict__ state,
                        float* __restrict__ x) {
    const uint32_t sem_lo = cfg->sem_lo, sem_hi = cfg->sem_hi;
    if (prompt) embed_tokens<WT>(tok_emb, cb_emb, dim, n_cb, cb_size, sem_lo, sem_hi, prompt + state->step, state->prompt_L, x,
                                 threadIdx.x, blockDim.x);
    else embed_tokens<WT>(tok_emb, cb_emb, dim, n_cb, cb_size, sem_lo, sem_hi, state->cur, 1, x, threadIdx.x, blockDim.x);
}

template <typename WT>
__global__ void k_fast_embed(const WT* __restrict__ fast_emb, int dim, const uint32_t* __restrict__ ids, float* __restrict__ out) {
    const uint32_t id = ids[blockIdx.x];
    for (int d = threadIdx.x; d < dim; d += blockDim.x) out[(size_t)blockIdx.x * dim + d] = WTr<WT>::to_f32(fast_emb[(size_t)id * dim + d]);
}

template <typename WT>
__global__ void k_gather_rows(const WT* __restrict__ src, int dim, uint32_t r0, uint32_t r1, WT* __restrict__ dst) {
    for (int d = threadIdx.x; d < dim; d += blockDim.x) {
        dst[d] = src[(size_t)r0 * dim + d];
        dst[dim + d] = src[(size_t)r1 * dim + d];
    }
}

__global__ void k_advance(SeqState* state) {
    state->pos += 1;
    state->step += 1;
}

__global__ void k_advance_n(SeqState* state, int n) {
    state->pos += n;
    state->step += n;
}

// ------------------------------------------------------------------------------------------------ weight fill / convert
template <typename WT>
__global__ void k_synth_fill(WT* __restrict__ dst, uint64_t key, long long n_rows, long long n_cols, int row_mul, int row_off,
                             float mean, float scale, int round_bf16) {
    const long long n = n_rows * n_cols;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        float v = synth_elem(key, (uint64_t)i, mean, scale);
        if (round_bf16) v = bf16_bits_to_f32(WTr<bf16_t>::from_f32(v));
        const long long r = i / n_cols, cidx = i % n_cols;
        dst[(r * row_mul + row_off) * n_cols + cidx] = WTr<WT>::from_f32(v);
    }
}
template <typename WT>
__global__ void k_convert_rows(WT* __restrict__ dst, const float* __restrict__ src, long long n_rows, long long n_cols,
                               int row_mul, int row_off) {
    const long long n = n_rows * n_cols;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / n_cols, cidx = i % n_cols;
        dst[(r * row_mul + row_off) * n_cols + cidx] = WTr<WT>::from_f32(src[i]);
    }
}

// fp8 quantiser: one block per source row.  scale = amax / 448 (1 for an all-zero row); byte = e4m3fn_rne(v / scale) with an
// IEEE-exact f32 division: pure integer / correctly-rounded f32 arithmetic, so any IEEE-754 host reproduces the stored
// bytes and scales bit-for-bit (tests/test_fp8_gpu.py checks that against the CPU restatement).
template <bool SYNTH>
__global__ __launch_bounds__(256) void k_quant_fp8(uint8_t* __restrict__ dst, float* __restrict__ scales, const float* __restrict__ src,
                                                   uint64_t key, long long n_cols, int row_mul, int row_off, float mean, float gscale) {
    __shared__ float red[256];
    const long long r = blockIdx.x;
    auto elem = [&](long long c) -> float {
        if (SYNTH) return synth_elem(key, (uint64_t)(r * n_cols + c), mean, gscale);
        return src[r * n_cols + c];
    };
    float amax = 0.f;
    for (long long c = threadIdx.x; c < n_cols; c += 256) amax = fmaxf(amax, fabsf(elem(c)));
    red[threadIdx.x] = amax;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + o]);
        __syncthreads();
    }
    amax = red[0];
    const float sc = amax > 0.f ? __fdiv_rn(amax, 448.0f) : 1.0f;
    const long long orow = r * row_mul + row_off;
    if (threadIdx.x == 0) scales[orow] = sc;
    for (long long c = threadIdx.x; c < n_cols; c += 256) dst[orow * n_cols + c] = f32_to_e4m3(__fdiv_rn(elem(c), sc));
}

// out[b] = the value the GEMV kernels' unpack path (v_cvt_pk_f32_fp8) assigns to byte b, in each of the 16 lane slots
__global__ void k_fp8_decode_table(float* __restrict__ out) {
    const unsigned b = threadIdx.x & 255u, slot = blockIdx.x;  // slot 0..15: position of the byte inside the 16-byte lane load
    unsigned w[4] = {0u, 0u, 0u, 0u};
    w[slot >> 2] = b << (8 * (slot & 3));
    u32x4 v; v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
    float f[16];
    WTr<fp8_t>::unpack(v, f);
    float r = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) if (i == (int)slot) r = f[i];
    out[slot * 256 + b] = r;
}

// ================================================================================================ launchers
#define FS_LAUNCH_CHECK() FS_HIP(hipGetLastError())

template <typename F>
static void dispatch_k(int K, F&& f) {
    switch (K) {
        case 128: f(std::integral_constant<int, 128>()); break;
        case 256: f(std::integral_constant<int, 256>()); break;
        case 1024: f(std::integral_constant<int, 1024>()); break;
        case 4096: f(std::integral_constant<int, 4096>()); break;
        default: throw Error("unsupported GEMV width K=" + std::to_string(K) + " (supported: 128, 256, 1024, 4096)");
    }
}

// ---- the one place that decides which instantiation and grid a batch-1 GEMV launcher runs (GemvPlan: lm_kernels.h)
constexpr int GEMV_QKV_WAVES = 2;  // one row per wave, one RoPE pair per block
constexpr int GEMV_ROW_WAVES = 4;  // k_wo, k_ffn_up, k_head
constexpr int GEMV_DOWN_KS = 4;    // k_ffn_down: waves that share one row
template <typename WT> constexpr int gemv_wt() { return std::is_same<WT, float>::value ? 0 : (std::is_same<WT, bf16_t>::value ? 1 : 2); }

std::string GemvPlan::name() const {
    static const char* const ops[] = {"qkv", "wo", "up", "down", "head"};
    static const char* const wts[] = {"f32", "bf16", "fp8"};
    std::string n = std::string(ops[op]) + "/" + wts[wt] + "/K" + std::to_string(K) + (op == FFN_DOWN ? "/ks" : "/w") + std::to_string(waves);
    if (op == WO) n += (fused ? "/fused" : "") + std::string("/dh") + std::to_string(DH);
    if (op != HEAD) n += nt ? "/nt" : "/res";
    return n;
}

GemvPlan gemv_plan(int op, int wt, const ModelDims& d, int n_rows, bool cache_resident, int fused_T) {
    FS_REQUIRE(op >= GemvPlan::QKV && op <= GemvPlan::HEAD && wt >= 0 && wt <= 2, "unknown GEMV op or weight type");
    GemvPlan p;
    p.op = (GemvPlan::Op)op; p.wt = wt; p.nt = !cache_resident;
    p.K = op == GemvPlan::FFN_DOWN ? d.inter : d.dim;
    if (op == GemvPlan::WO) {
        FS_REQUIRE(fused_T <= 8 && d.H <= 32 && d.H * 8 * 2 <= GEMV_ROW_WAVES * 64 && d.dim <= 4 * GEMV_ROW_WAVES * 64, "fused attention supports at most 8 cached tokens and 16 heads");
        FS_REQUIRE(d.Dh == 64 || d.Dh == 32, "unsupported head_dim");
        p.fused = fused_T > 0; p.DH = d.Dh;
    }
    dispatch_k(p.K, [](auto) {});  // (throws for a width without an instantiation)
    if (op == GemvPlan::FFN_DOWN) { p.waves = GEMV_DOWN_KS; p.gx = (unsigned)n_rows; }  // one row per block
    else {
        p.waves = op == GemvPlan::QKV ? GEMV_QKV_WAVES : GEMV_ROW_WAVES;
        p.gx = (unsigned)((n_rows + p.waves - 1) / p.waves);
    }
    p.block = (unsigned)p.waves * 64;
    if (op == GemvPlan::HEAD) p.nt = true;
    return p;
}

template <typename WT>
void LmKernels<WT>::qkv(const ModelDims& d, const float* x, const LayerW& w, const float* cos_t, const float* sin_t,
                        const SeqState* state, int pos_static, int rope_static, float* q_out, KVView kv, hipStream_t st) {
    constexpr int WAVES = GEMV_QKV_WAVES;
    const GemvPlan p = gemv_plan(GemvPlan::QKV, gemv_wt<WT>(), d, (d.H + 2 * d.Hk) * d.Dh, w.cache_resident);
    dispatch_k(p.K, [&](auto Kc) {
        constexpr int K = decltype(Kc)::value;
        if (!p.nt)
            hipLaunchKernelGGL((k_qkv<WT, K, WAVES, false>), dim3(p.gx), dim3(p.block), 0, st, x, w.attn_norm, d.eps,
                               (const WT*)w.wqkv, cos_t, sin_t, state, pos_static, rope_static, q_out, kv, d.H, d.Hk, d.Dh, w.s_qkv);
        else
            hipLaunchKernelGGL((k_qkv<WT, K, WAVES, true>), dim3(p.gx), dim3(p.block), 0, st, x, w.attn_norm, d.eps,
                               (const WT*)w.wqkv, cos_t, sin_t, state, pos_static, rope_static, q_out, kv, d.H, d.Hk, d.Dh, w.s_qkv);
    });
    FS_LAUNCH_CHECK();
}

template <typename WT>
void LmKernels<WT>::wo(const ModelDims& d, const float* part, int n_chunks_max, int nc_launch, const SeqState* state, const float* q,
                       KVView kv, int fused_T, const LayerW& w, float* x, hipStream_t st) {
    int chunk = AttnKernels<WT>::chunk();
    if (fused_T <= 0) {
        FS_REQUIRE(nc_launch >= 1 && nc_launch <= n_chunks_max, "bad attention chunk count");
        const int tpb = AttnKernels<WT>::tiles_per_block(d, nc_launch);  // AttnKernels::decode left one partial per super-chunk
        chunk *= tpb;
        nc_launch = (nc_launch + tpb - 1) / tpb;
    } else nc_launch = 1;
    constexpr int WAVES = GEMV_ROW_WAVES;
    const GemvPlan p = gemv_plan(GemvPlan::WO, gemv_wt<WT>(), d, d.dim, w.cache_resident, fused_T);
    dispatch_k(p.K, [&](auto Kc) {
        constexpr int K = decltype(Kc)::value;
        auto go = [&](auto fused, auto dh) {
            if (!p.nt)
                hipLaunchKernelGGL((k_wo<WT, K, WAVES, decltype(fused)::value, decltype(dh)::value, false>), dim3(p.gx), dim3(p.block), 0,
                                   st, part, n_chunks_max, chunk, state, q, kv, fused_T, (const WT*)w.wo, x, d.H, d.Hk, d.dim, w.s_o, nc_launch);
            else
                hipLaunchKernelGGL((k_wo<WT, K, WAVES, decltype(fused)::value, decltype(dh)::value, true>), dim3(p.gx), dim3(p.block), 0,
                                   st, part, n_chunks_max, chunk, state, q, kv, fused_T, (const WT*)w.wo, x, d.H, d.Hk, d.dim, w.s_o, nc_launch);
        };
        using T = std::true_type; using F = std::false_type;
        using D64 = std::integral_constant<int, 64>; using D32 = std::integral_constant<int, 32>;
        if (p.fused) { if (p.DH == 64) go(T(), D64()); else go(T(), D32()); }
        else { if (p.DH == 64) go(F(), D64()); else go(F(), D32()); }
    });
    FS_LAUNCH_CHECK();
}

template <typename WT>
void LmKernels<WT>::ffn_up(const ModelDims& d, const float* x, const LayerW& w, float* act, hipStream_t st) {
    constexpr int WAVES = GEMV_ROW_WAVES;
    const GemvPlan p = gemv_plan(GemvPlan::FFN_UP, gemv_wt<WT>(), d, d.inter, w.cache_resident);
    dispatch_k(p.K, [&](auto Kc) {
        constexpr int K = decltype(Kc)::value;
        if (!p.nt)
            hipLaunchKernelGGL((k_ffn_up<WT, K, WAVES, false>), dim3(p.gx), dim3(p.block), 0, st, x, w.ffn_norm, d.eps,
                               (const WT*)w.w13, act, d.inter, w.s_13);
        else
            hipLaunchKernelGGL((k_ffn_up<WT, K, WAVES, true>), dim3(p.gx), dim3(p.block), 0, st, x, w.ffn_norm, d.eps,
                               (const WT*)w.w13, act, d.inter, w.s_13);
    });
    FS_LAUNCH_CHECK();
}

template <typename WT>
void LmKernels<WT>::ffn_down(const ModelDims& d, const float* act, const LayerW& w, float* x, hipStream_t st) {
    constexpr int KS = GEMV_DOWN_KS;
    const GemvPlan p = gemv_plan(GemvPlan::FFN_DOWN, gemv_wt<WT>(), d, d.dim, w.cache_resident);
    dispatch_k(p.K, [&](auto Kc) {
        constexpr int K = decltype(Kc)::value;
        if (!p.nt)
            hipLaunchKernelGGL((k_ffn_down<WT, K, KS, false>), dim3(p.gx), dim3(p.block), 0, st, act, (const WT*)w.w2, x, d.dim, w.s_2);
        else
            hipLaunchKernelGGL((k_ffn_down<WT, K, KS, true>), dim3(p.gx), dim3(p.block), 0, st, act, (const WT*)w.w2, x, d.dim, w.s_2);
    });
    FS_LAUNCH_CHECK();
}

template <typename WT>
void LmKernels<WT>::head(const ModelDims& d, const float* x, const float* norm_w, const void* W, const float* wscale, int n_rows,
                         float* logits, hipStream_t st) {
    constexpr int WAVES = GEMV_ROW_WAVES;
    const GemvPlan p = gemv_plan(GemvPlan::HEAD, gemv_wt<WT>(), d, n_rows, false);
    dispatch_k(p.K, [&](auto Kc) {
        constexpr int K = decltype(Kc)::value;
        hipLaunchKernelGGL((k_head<WT, K, WAVES>), dim3(p.gx), dim3(p.block), 0, st, x, norm_w, d.eps, (const WT*)W,
                           n_rows, logits, wscale);
    });
    FS_LAUNCH_CHECK();
}

template <typename WT>
void LmKernels<WT>::embed(const ModelDims& d, const void* tok_emb, const void* cb_emb, int n_cb, int cb_size,
                          const SampleCfg* cfg, const uint32_t* prompt, SeqState* state, float* x, hipStream_t st) {
    hipLaunchKernelGGL((k_embed<KVT<WT>>), dim3(1), dim3(256), 0, st, (const KVT<WT>*)tok_emb, (const KVT<WT>*)cb_emb, d.dim, n_cb, cb_size,
                       cfg, prompt, state, x);
    FS_LAUNCH_CHECK();
}

template <typename WT>
void LmKernels<WT>::fast_embed(const ModelDims& d, const void* fast_emb, const uint32_t* ids, int n, float* out,
                               hipStream_t st) {
    hipLaunchKernelGGL((k_fast_embed<KVT<WT>>), dim3(n), dim3(256), 0, st, (const KVT<WT>*)fast_emb, d.dim, ids, out);
    FS_LAUNCH_CHECK();
}

template <typename WT>
void launch_gather_rows(const void* src, int dim, uint32_t r0, uint32_t r1, void* dst, hipStream_t st) {
    hipLaunchKernelGGL((k_gather_rows<WT>), dim3(1), dim3(256), 0, st, (const WT*)src, dim, r0, r1, (WT*)dst);
    FS_LAUNCH_CHECK();
}
template void launch_gather_rows<bf16_t>(const void*, int, uint32_t, uint32_t, void*, hipStream_t);
template void launch_gather_rows<float>(const void*, int, uint32_t, uint32_t, void*, hipStream_t);
template void launch_gather_rows<fp8_t>(const void*, int, uint32_t, uint32_t, void*, hipStream_t);

void launch_advance(SeqState* state, hipStream_t st) {
    hipLaunchKernelGGL(k_advance, dim3(1), dim3(1), 0, st, state);
    FS_LAUNCH_CHECK();
}

template <typename WT>
void launch_synth_fill(WT* dst, uint64_t key, int64_t n_rows, int64_t n_cols, int row_mul, int row_off, float mean, float scale,
                       int round_bf16, hipStream_t st) {
    const long long n = n_rows * n_cols;
    const int grid = (int)std::min<long long>((n + 255) / 256, 4096);
    hipLaunchKernelGGL((k_synth_fill<WT>), dim3(grid), dim3(256), 0, st, dst, key, (long long)n_rows, (long long)n_cols, row_mul,
                       row_off, mean, scale, round_bf16);
    FS_LAUNCH_CHECK();
}
template <typename WT>
void launch_convert_rows(WT* dst, const float* src, int64_t n_rows, int64_t n_cols, int row_mul, int row_off, hipStream_t st) {
    const long long n = n_rows * n_cols;
    const int grid = (int)std::min<long long>((n + 255) / 256, 4096);
    hipLaunchKernelGGL((k_convert_rows<WT>), dim3(grid), dim3(256), 0, st, dst, src, (long long)n_rows, (long long)n_cols,
                       row_mul, row_off);
    FS_LAUNCH_CHECK();
}

void launch_synth_quant_fp8(uint8_t* dst, float* scales, uint64_t key, int64_t n_rows, int64_t n_cols, int row_mul, int row_off,
                            float mean, float scale, hipStream_t st) {
    hipLaunchKernelGGL((k_quant_fp8<true>), dim3((unsigned)n_rows), dim3(256), 0, st, dst, scales, (const float*)nullptr, key,
                       (long long)n_cols, row_mul, row_off, mean, scale);
    FS_LAUNCH_CHECK();
}
void launch_fp8_decode_table(float* out, hipStream_t st) {
    hipLaunchKernelGGL(k_fp8_decode_table, dim3(16), dim3(256), 0, st, out);
    FS_LAUNCH_CHECK();
}
void launch_quant_rows_fp8(uint8_t* dst, float* scales, const float* src, int64_t n_rows, int64_t n_cols, int row_mul, int row_off,
                           hipStream_t st) {
    hipLaunchKernelGGL((k_quant_fp8<false>), dim3((unsigned)n_rows), dim3(256), 0, st, dst, scales, src, (uint64_t)0,
                       (long long)n_cols, row_mul, row_off, 0.f, 0.f);
    FS_LAUNCH_CHECK();
}

void launch_advance_n(SeqState* state, int n, hipStream_t st) {
    hipLaunchKernelGGL(k_advance_n, dim3(1), dim3(1), 0, st, state, n);
    FS_LAUNCH_CHECK();
}

// Copy-on-write of shared KV pages: page pairs[2i] -> page pairs[2i + 1] in every one of the n_regions regions of the pool (the K and
// the V pages of every slow layer: region r starts r * region_bytes in).  Block = (pair, region); 16-byte vector loads and stores.
__global__ __launch_bounds__(256) void k_kv_page_copy(uint8_t* __restrict__ pool, size_t region_bytes, size_t page_bytes,
                                                      const int* __restrict__ pairs) {
    const int src = pairs[2 * blockIdx.x], dst = pairs[2 * blockIdx.x + 1];
    uint8_t* const base = pool + (size_t)blockIdx.y * region_bytes;
    const uint4* s = reinterpret_cast<const uint4*>(base + (size_t)src * page_bytes);
    uint4* d = reinterpret_cast<uint4*>(base + (size_t)dst * page_bytes);
    const size_t n16 = page_bytes / 16;
    for (size_t i = threadIdx.x; i < n16; i += blockDim.x) d[i] = s[i];
}
void launch_kv_page_copy(void* pool, int n_regions, size_t region_bytes, size_t page_bytes, const int* pairs, int n_pairs, hipStream_t st) {
    if (n_pairs <= 0) return;
    FS_REQUIRE(page_bytes % 16 == 0 && region_bytes % 16 == 0, "KV pages must be whole 16-byte units");
    hipLaunchKernelGGL(k_kv_page_copy, dim3(n_pairs, n_regions), dim3(256), 0, st, reinterpret_cast<uint8_t*>(pool), region_bytes, page_bytes, pairs);
    FS_LAUNCH_CHECK();
}

// Prefix KV blobs (fishrt.h: fs_lm_session_prefix_export / _import).  Block = (page j of the prefix, region); the regions are those of
// k_kv_page_copy.  A page holds [Hk][64][Dh]; the packed payload of a region holds the prefix's P rows as [t][Hk][Dh].  The block moves
// only the min(64, P - 64 j) valid rows of its page, in 16-byte units along Dh (`upr` units per [Dh] row): unit i of the block's packed
// span is (t, g, u) = (i / (Hk upr), i / upr % Hk, i % upr), its place in the page is ((g 64 + t) upr + u).
template <bool kScatter>
__device__ __forceinline__ void kv_rows_move(uint8_t* pool, size_t region_bytes, size_t page_bytes, const int* __restrict__ pages, int P, int Hk,
                                             int upr, uint8_t* packed) {
    const int j = blockIdx.x;
    const int rows = min(KV_PAGE, P - KV_PAGE * j);
    if (rows <= 0) return;
    uint4* const page = reinterpret_cast<uint4*>(pool + (size_t)blockIdx.y * region_bytes + (size_t)pages[j] * page_bytes);
    const int row_units = Hk * upr;  // 16-byte units of one packed row
    uint4* const pk = reinterpret_cast<uint4*>(packed) + ((size_t)blockIdx.y * P + (size_t)KV_PAGE * j) * row_units;
    const int n = rows * row_units;
    for (int i = threadIdx.x; i < n; i += 256) {
        const int t = i / row_units, rem = i - t * row_units, g = rem / upr, u = rem - g * upr;
        const int at = (g * KV_PAGE + t) * upr + u;
        if (kScatter) page[at] = pk[i];
        else pk[i] = page[at];
    }
}
__global__ __launch_bounds__(256) void k_kv_rows_gather(const uint8_t* __restrict__ pool, size_t region_bytes, size_t page_bytes,
                                                        const int* __restrict__ pages, int P, int Hk, int upr, uint8_t* __restrict__ packed) {
    kv_rows_move<false>(const_cast<uint8_t*>(pool), region_bytes, page_bytes, pages, P, Hk, upr, packed);
}
__global__ __launch_bounds__(256) void k_kv_rows_scatter(uint8_t* __restrict__ pool, size_t region_bytes, size_t page_bytes,
                                                         const int* __restrict__ pages, int P, int Hk, int upr, const uint8_t* __restrict__ packed) {
    kv_rows_move<true>(pool, region_bytes, page_bytes, pages, P, Hk, upr, const_cast<uint8_t*>(packed));
}
static void check_kv_rows(size_t region_bytes, size_t page_bytes, int P, int Hk, int Dh, size_t elem_bytes) {
    FS_REQUIRE(Dh % 8 == 0, "prefix KV blobs need head_dim % 8 == 0 (the rows move in 16-byte units along head_dim)");
    FS_REQUIRE(P >= 1 && Hk >= 1 && (Dh * elem_bytes) % 16 == 0 && page_bytes == (size_t)Hk * KV_PAGE * Dh * elem_bytes && region_bytes % page_bytes == 0,
               "prefix KV blob: page geometry does not match the pool");
}
void launch_kv_rows_gather(const void* pool, int n_regions, size_t region_bytes, size_t page_bytes, const int* pages, int P, int Hk, int Dh,
                           size_t elem_bytes, void* packed, hipStream_t st) {
    check_kv_rows(region_bytes, page_bytes, P, Hk, Dh, elem_bytes);
    hipLaunchKernelGGL(k_kv_rows_gather, dim3((P + KV_PAGE - 1) / KV_PAGE, n_regions), dim3(256), 0, st, reinterpret_cast<const uint8_t*>(pool),
                       region_bytes, page_bytes, pages, P, Hk, (int)(Dh * elem_bytes / 16), reinterpret_cast<uint8_t*>(packed));
    FS_LAUNCH_CHECK();
}
void launch_kv_rows_scatter(void* pool, int n_regions, size_t region_bytes, size_t page_bytes, const int* pages, int P, int Hk, int Dh,
                            size_t elem_bytes, const void* packed, hipStream_t st) {
    check_kv_rows(region_bytes, page_bytes, P, Hk, Dh, elem_bytes);
    hipLaunchKernelGGL(k_kv_rows_scatter, dim3((P + KV_PAGE - 1) / KV_PAGE, n_regions), dim3(256), 0, st, reinterpret_cast<uint8_t*>(pool),
                       region_bytes, page_bytes, pages, P, Hk, (int)(Dh * elem_bytes / 16), reinterpret_cast<const uint8_t*>(packed));
    FS_LAUNCH_CHECK();
}

// Fingerprint of the weight arena (fishrt.h: fs_lm_weights_fingerprint): *acc += sum over the arena's 32-bit words w[i] of
// w[i] * (2 i + 1), in wrapping 64-bit integer arithmetic -- a sum of integers, so the grid size and the order of the atomics do not
// change a bit of it.  Lanes read 16 bytes (4 words) per step; the n % 4 last words are taken by the first lanes of block 0.
__global__ __launch_bounds__(256) void k_arena_fingerprint(const uint32_t* __restrict__ w, uint64_t n, unsigned long long* __restrict__ acc) {
    __shared__ unsigned long long part[4];
    const uint64_t n4 = n / 4;
    const uint4* w4 = reinterpret_cast<const uint4*>(w);
    unsigned long long s = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (uint64_t)gridDim.x * 256) {
        const uint4 v = w4[i];
        const uint64_t k = 8 * i + 1;  // 2 * (4 i) + 1
        s += (uint64_t)v.x * k + (uint64_t)v.y * (k + 2) + (uint64_t)v.z * (k + 4) + (uint64_t)v.w * (k + 6);
    }
    if (blockIdx.x == 0 && 4 * n4 + threadIdx.x < n) s += (uint64_t)w[4 * n4 + threadIdx.x] * (2 * (4 * n4 + threadIdx.x) + 1);
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(acc, part[0] + part[1] + part[2] + part[3]);
}
void launch_arena_fingerprint(const void* arena, size_t bytes, uint64_t* acc, hipStream_t st) {
    FS_REQUIRE(bytes % 4 == 0 && ((uintptr_t)arena & 15) == 0, "the weight arena must be whole 32-bit words, 16-byte aligned");
    const uint64_t n = bytes / 4;
    const int grid = (int)std::max<uint64_t>(1, std::min<uint64_t>((n / 4 + 255) / 256, 2048));
    hipLaunchKernelGGL(k_arena_fingerprint, dim3(grid), dim3(256), 0, st, reinterpret_cast<const uint32_t*>(arena), n,
                       reinterpret_cast<unsigned long long*>(acc));
    FS_LAUNCH_CHECK();
}

// Hidden-state collection of session slots: one block per slot.  The row index is the slot's own counter in the table (== its iteration
// index: a slot runs one iteration per step from its activation until done != 0), so a parked, frozen, finished or not yet joined slot
// (done != 0) stores nothing and a full buffer is never overrun.  256 lanes x 16 bytes = one 1024-float row per pass.
__global__ __launch_bounds__(256) void k_hidden_rows(HidSlot* __restrict__ tab, const SeqState* __restrict__ states, const float* __restrict__ X,
                                                     int dim) {
    const int b = blockIdx.x;
    HidSlot* h = tab + b;
    float* rows = h->rows;
    if (!rows) return;
    if (states[b].done != 0) return;
    const int it = h->count;
    if (it >= h->cap) return;
    const float4* s = reinterpret_cast<const float4*>(X + (size_t)b * dim);
    float4* d = reinterpret_cast<float4*>(rows + (size_t)it * dim);
    for (int i = threadIdx.x; i < dim / 4; i += 256) d[i] = s[i];
    __syncthreads();  // (every wave has read count)
    if (threadIdx.x == 0) h->count = it + 1;
}
void launch_hidden_rows(HidSlot* tab, const SeqState* states, const float* X, int dim, int B, hipStream_t st) {
    if (B <= 0) return;
    FS_REQUIRE(dim % 4 == 0, "hidden rows are copied in 16-byte units");
    hipLaunchKernelGGL(k_hidden_rows, dim3(B), dim3(256), 0, st, tab, states, X, dim);
    FS_LAUNCH_CHECK();
}

template struct LmKernels<bf16_t>;
template struct LmKernels<float>;
template struct LmKernels<fp8_t>;
template void launch_synth_fill<bf16_t>(bf16_t*, uint64_t, int64_t, int64_t, int, int, float, float, int, hipStream_t);
template void launch_synth_fill<float>(float*, uint64_t, int64_t, int64_t, int, int, float, float, int, hipStream_t);
template void launch_convert_rows<bf16_t>(bf16_t*, const float*, int64_t, int64_t, int, int, hipStream_t);
template void launch_convert_rows<float>(float*, const float*, int64_t, int64_t, int, int, hipStream_t);

// ================================================================================================ fs_selftest_gemv (include/fishrt.h)
// ONE launcher call of LmKernels on caller data and nothing else.  Everything a launch writes (the output vector, both KV pools) lies between
// 256-element guards of 0xFF bytes and is poisoned with 0xFF bytes (NaN) where the caller provides nothing; the whole case is validated before
// the first device call.
namespace {
constexpr size_t kGemvGuard = 256;
struct GemvDev {  // device buffer of n elements of es bytes between two guards, all 0xFF bytes at first
    void* p = nullptr;
    size_t n = 0, es = 4;
    void alloc(size_t n_, size_t es_, hipStream_t st) {
        n = n_; es = es_;
        FS_HIP(hipMalloc(&p, (n + 2 * kGemvGuard) * es));
        FS_HIP(hipMemsetAsync(p, 0xFF, (n + 2 * kGemvGuard) * es, st));
    }
    char* data() const { return (char*)p + kGemvGuard * es; }
    void up(const void* src, size_t count, hipStream_t st) {  // synchronous: the source may be a temporary
        FS_HIP(hipMemcpyAsync(data(), src, count * es, hipMemcpyHostToDevice, st));
        FS_HIP(hipStreamSynchronize(st));
    }
    void put(const void* src, size_t count, size_t es_, hipStream_t st) { alloc(count, es_, st); up(src, count, st); }
    bool intact(hipStream_t st) const {
        if (!p) return true;
        std::vector<uint8_t> g(2 * kGemvGuard * es);
        FS_HIP(hipMemcpyAsync(g.data(), p, kGemvGuard * es, hipMemcpyDeviceToHost, st));
        FS_HIP(hipMemcpyAsync(g.data() + kGemvGuard * es, data() + n * es, kGemvGuard * es, hipMemcpyDeviceToHost, st));
        FS_HIP(hipStreamSynchronize(st));
        for (uint8_t b : g) if (b != 0xFF) return false;
        return true;
    }
    ~GemvDev() { if (p) (void)hipFree(p); }
};

void gemv_req(bool ok, const char* msg) { if (!ok) throw Error(std::string("GEMV self-test: ") + msg); }

// f32 values -> the storage type T (exact: validation has checked that every value is on T's grid)
template <typename T> T gemv_cast(float f) {
    if constexpr (std::is_same<T, float>::value) return f;
    else if constexpr (std::is_same<T, bf16_t>::value) return f32_to_bf16_host(f);
    else return fp8_t{f32_to_e4m3(f)};
}
template <typename T> float gemv_f32(T v) {
    if constexpr (std::is_same<T, float>::value) return v;
    else if constexpr (std::is_same<T, bf16_t>::value) return bf16_to_f32_host(v);
    else return e4m3_to_f32(v.v);
}
template <typename T> void gemv_put_as(GemvDev& b, const float* src, size_t n, hipStream_t st) {
    std::vector<T> h(n);
    for (size_t i = 0; i < n; ++i) h[i] = gemv_cast<T>(src[i]);
    b.put(h.data(), n, sizeof(T), st);
}
void gemv_on_grid(const float* a, size_t n, int wt, const char* msg) {  // wt: 0 f32 (anything), 1 bf16, 2 e4m3fn
    if (wt == FS_GEMV_WT_F32) return;
    for (size_t i = 0; i < n; ++i) {
        const float w = a[i];
        gemv_req(wt == FS_GEMV_WT_FP8 ? e4m3_to_f32(f32_to_e4m3(w)) == w : bf16_to_f32_host(f32_to_bf16_host(w)) == w, msg);
    }
}

// everything validation derives from a case: the dims, the plan's name and grid, the extents
struct GemvCaseInfo {
    ModelDims d{};
    std::string name;
    unsigned gx = 1;
    size_t w_rows = 0, w_cols = 0, n_x = 0, n_y = 0, n_pool = 0;
};

void gemv_validate(const fs_gemv_case& c, GemvCaseInfo& I) {
    const auto req = gemv_req;
    static const char* const wts[] = {"f32", "bf16", "fp8"};
    req(c.op >= FS_GEMV_QKV && c.op <= FS_GEMV_FAST_EMBED, "unknown op");
    req(c.wt >= FS_GEMV_WT_F32 && c.wt <= FS_GEMV_WT_FP8, "unknown weight type");
    req(std::isfinite(c.eps) && c.eps >= 0.f, "eps must be finite and >= 0");
    const int kvt = c.wt == FS_GEMV_WT_F32 ? FS_GEMV_WT_F32 : FS_GEMV_WT_BF16;  // KVT<WT>: pools and embedding tables
    ModelDims& d = I.d;
    d.dim = c.dim; d.inter = c.inter; d.H = c.H; d.Hk = c.Hk; d.Dh = c.Dh; d.n_rep = c.Hk > 0 ? c.H / c.Hk : 0; d.eps = c.eps;
    req(c.dim >= 1 && c.dim <= 16384, "1 <= dim <= 16384");
    if (c.op == FS_GEMV_EMBED || c.op == FS_GEMV_FAST_EMBED) {
        req(c.tok_emb && c.tok_rows >= 1 && (size_t)c.tok_rows * c.dim <= ((size_t)1 << 24), "tok_emb [tok_rows][dim] is required, at most 2^24 elements");
        gemv_on_grid(c.tok_emb, (size_t)c.tok_rows * c.dim, kvt, "an embedding value is not a value of the table type");
        if (c.op == FS_GEMV_FAST_EMBED) {
            req(c.ids && c.n_ids >= 1 && c.n_ids <= 4096, "fast embed: ids [n_ids] is required, 1 <= n_ids <= 4096");
            for (int i = 0; i < c.n_ids; ++i) req(c.ids[i] < (uint32_t)c.tok_rows, "fast embed: an id is outside the table");
            I.name = std::string("fast_embed/") + wts[kvt]; I.gx = (unsigned)c.n_ids; I.n_y = (size_t)c.n_ids * c.dim;
            return;
        }
        req(c.n_cb >= 0 && c.n_cb <= 15 && c.cb_size >= 1 && (c.n_cb == 0 || c.cb_emb) && (size_t)std::max(c.n_cb, 1) * c.cb_size * c.dim <= ((size_t)1 << 24),
            "embed: 0 <= n_cb <= 15 (SeqState::cur holds 16 tokens), cb_size >= 1, cb_emb [n_cb cb_size][dim] of at most 2^24 elements");
        gemv_on_grid(c.cb_emb, (size_t)c.n_cb * c.cb_size * c.dim, kvt, "an embedding value is not a value of the table type");
        req(c.tokens != nullptr, "embed: tokens is required");
        int stride = 1;
        if (c.use_prompt) {
            req(c.prompt_L >= 1 && c.step >= 0 && c.step < c.prompt_L, "embed: prompt source needs prompt_L >= 1 and 0 <= step < prompt_L");
            req((long long)c.n_tokens >= (long long)c.n_cb * c.prompt_L + c.step + 1, "embed: the staged prompt does not hold every token the column reads");
            stride = c.prompt_L;
        } else req(c.n_tokens >= c.n_cb + 1, "embed: cur source needs n_cb + 1 tokens");
        const uint32_t* t = c.tokens + (c.use_prompt ? c.step : 0);
        req(t[0] < (uint32_t)c.tok_rows, "embed: the semantic token is outside tok_emb");
        for (int k = 0; k < c.n_cb; ++k) req(t[(size_t)(k + 1) * stride] < (uint32_t)c.cb_size, "embed: a code is outside its codebook");
        I.name = std::string("embed/") + wts[kvt]; I.gx = 1; I.n_y = (size_t)c.dim;
        return;
    }
    req(c.x && c.w, "x and w are required");
    req(c.wt != FS_GEMV_WT_FP8 || c.wscale, "fp8 weights need their row scales (wscale)");
    const bool resident = c.cache_resident != 0;
    GemvPlan p;
    switch (c.op) {
    case FS_GEMV_QKV:
        req(c.H >= 1 && c.H <= 64 && c.Hk >= 1 && c.Hk <= c.H && c.H % c.Hk == 0, "1 <= Hk <= H <= 64, H a multiple of Hk");
        req(c.Dh >= 2 && c.Dh <= 256 && c.Dh % 2 == 0, "head_dim must be even (RoPE rotates pairs), 2 <= Dh <= 256");
        req(c.dim == c.H * c.Dh, "dim must equal H * Dh");
        p = gemv_plan(GemvPlan::QKV, c.wt, d, (c.H + 2 * c.Hk) * c.Dh, resident);
        req(c.norm_w && c.cos_t && c.sin_t && c.k && c.v && c.page_table, "qkv: norm_w, cos_t, sin_t, k, v and page_table are required");
        req(c.n_pages >= 1 && c.n_pages <= 4096 && c.pt_len >= 1 && c.pt_len <= (1 << 16), "qkv: 1 <= n_pages <= 4096, 1 <= pt_len <= 2^16");
        req(c.pos >= 0 && c.pos < (1 << 20) && c.rope_off >= 0 && c.rope_off < (1 << 20) && c.rope_rows >= 1 && c.pos + c.rope_off < c.rope_rows,
            "qkv: the position or the RoPE row is outside [0, 2^20) / the cos / sin tables");
        req(c.pos / KV_PAGE < c.pt_len, "qkv: the page table does not cover pos");
        for (int i = 0; i < c.pt_len; ++i) req(c.page_table[i] >= 0 && c.page_table[i] < c.n_pages, "qkv: a page id is outside the pool");
        I.w_rows = (size_t)(c.H + 2 * c.Hk) * c.Dh; I.w_cols = (size_t)c.dim; I.n_x = (size_t)c.dim; I.n_y = (size_t)c.H * c.Dh;
        I.n_pool = (size_t)c.n_pages * c.Hk * KV_PAGE * c.Dh;
        gemv_on_grid(c.k, I.n_pool, kvt, "a pool value is not a value of the KV type");
        gemv_on_grid(c.v, I.n_pool, kvt, "a pool value is not a value of the KV type");
        break;
    case FS_GEMV_FFN_UP:
        req(c.inter >= 1 && c.inter <= 16384 && c.norm_w, "up: 1 <= inter <= 16384, norm_w is required");
        p = gemv_plan(GemvPlan::FFN_UP, c.wt, d, c.inter, resident);
        I.w_rows = (size_t)2 * c.inter; I.w_cols = (size_t)c.dim; I.n_x = (size_t)c.dim; I.n_y = (size_t)c.inter;
        break;
    case FS_GEMV_FFN_DOWN:
        req(c.inter >= 1 && c.y, "down: inter >= 1, y (the residual stream) is required");
        p = gemv_plan(GemvPlan::FFN_DOWN, c.wt, d, c.dim, resident);
        I.w_rows = (size_t)c.dim; I.w_cols = (size_t)c.inter; I.n_x = (size_t)c.inter; I.n_y = (size_t)c.dim;
        break;
    case FS_GEMV_HEAD:
        req(c.n_rows >= 1 && c.n_rows <= (1 << 18) && c.norm_w, "head: 1 <= n_rows <= 2^18, norm_w is required");
        p = gemv_plan(GemvPlan::HEAD, c.wt, d, c.n_rows, false);
        I.w_rows = (size_t)c.n_rows; I.w_cols = (size_t)c.dim; I.n_x = (size_t)c.dim; I.n_y = (size_t)c.n_rows;
        break;
    default:  // FS_GEMV_WO_BODY
        req(c.H >= 1 && c.H <= 16 && c.Hk >= 1 && c.Hk <= c.H && c.H % c.Hk == 0, "wo: 1 <= Hk <= H <= 16, H a multiple of Hk");
        req(c.Dh >= 2 && c.Dh % 2 == 0, "head_dim must be even (RoPE rotates pairs), 2 <= Dh <= 256");
        req(c.dim == c.H * c.Dh, "dim must equal H * Dh");
        req(c.y != nullptr, "wo: y (the residual stream) is required");
        p = gemv_plan(GemvPlan::WO, c.wt, d, c.dim, resident, 0);
        I.w_rows = (size_t)c.dim; I.w_cols = (size_t)c.dim; I.n_x = (size_t)c.dim; I.n_y = (size_t)c.dim;
        break;
    }
    req(I.w_rows * I.w_cols <= ((size_t)1 << 26), "the weight matrix has more than 2^26 elements");
    I.name = p.name(); I.gx = p.gx;
    gemv_on_grid(c.w, I.w_rows * I.w_cols, c.wt, c.wt == FS_GEMV_WT_FP8 ? "a weight is not an e4m3fn value" : "a weight is not a bf16 value");
}

template <typename WT>
void gemv_run(const fs_gemv_case& c, const GemvCaseInfo& I, fs_gemv_out& o, hipStream_t st) {
    using KT = KVT<WT>;
    const ModelDims& d = I.d;
    GemvDev dX, dG, dW, dS, dY, dCos, dSin, dK, dV, dTab, dState, dPart, dCfg, dTok, dCb, dIds, dPrompt;
    SeqState hs;
    std::memset(&hs, 0, sizeof(SeqState));
    if (c.op == FS_GEMV_EMBED || c.op == FS_GEMV_FAST_EMBED) {
        gemv_put_as<KT>(dTok, c.tok_emb, (size_t)c.tok_rows * c.dim, st);
        dY.alloc(I.n_y, 4, st);
        if (c.op == FS_GEMV_FAST_EMBED) {
            dIds.put(c.ids, (size_t)c.n_ids, 4, st);
            LmKernels<WT>::fast_embed(d, dTok.data(), (const uint32_t*)dIds.data(), c.n_ids, (float*)dY.data(), st);
        } else {
            if (c.n_cb > 0) gemv_put_as<KT>(dCb, c.cb_emb, (size_t)c.n_cb * c.cb_size * c.dim, st);
            SampleCfg hc = {};
            hc.sem_lo = c.sem_lo; hc.sem_hi = c.sem_hi;
            dCfg.put(&hc, sizeof(SampleCfg), 1, st);
            hs.step = c.step; hs.prompt_L = c.prompt_L;
            if (c.use_prompt) dPrompt.put(c.tokens, (size_t)c.n_tokens, 4, st);
            else for (int i = 0; i <= c.n_cb; ++i) hs.cur[i] = c.tokens[i];
            dState.put(&hs, sizeof(SeqState), 1, st);
            LmKernels<WT>::embed(d, dTok.data(), c.n_cb > 0 ? dCb.data() : nullptr, c.n_cb, c.cb_size, (const SampleCfg*)dCfg.data(),
                                 c.use_prompt ? (const uint32_t*)dPrompt.data() : nullptr, (SeqState*)dState.data(), (float*)dY.data(), st);
        }
    } else {
        dX.put(c.x, I.n_x, 4, st);
        if (c.norm_w) dG.put(c.norm_w, I.n_x, 4, st);
        gemv_put_as<WT>(dW, c.w, I.w_rows * I.w_cols, st);
        const float* scale = nullptr;
        if (std::is_same<WT, fp8_t>::value) { dS.put(c.wscale, I.w_rows, 4, st); scale = (const float*)dS.data(); }
        LayerW w{};
        w.cache_resident = c.cache_resident != 0;
        dY.alloc(I.n_y, 4, st);
        if (c.op == FS_GEMV_FFN_DOWN || c.op == FS_GEMV_WO_BODY) dY.up(c.y, I.n_y, st);
        switch (c.op) {
        case FS_GEMV_QKV: {
            w.wqkv = dW.data(); w.attn_norm = (const float*)dG.data(); w.s_qkv = scale;
            const size_t nr = (size_t)c.rope_rows * (c.Dh / 2);
            dCos.put(c.cos_t, nr, 4, st); dSin.put(c.sin_t, nr, 4, st);
            gemv_put_as<KT>(dK, c.k, I.n_pool, st); gemv_put_as<KT>(dV, c.v, I.n_pool, st);
            dTab.put(c.page_table, (size_t)c.pt_len, 4, st);
            hs.pos = c.pos; hs.rope_off = c.rope_off;
            if (c.use_state) dState.put(&hs, sizeof(SeqState), 1, st);
            const KVView kv{dK.data(), dV.data(), (const int*)dTab.data()};
            LmKernels<WT>::qkv(d, (const float*)dX.data(), w, (const float*)dCos.data(), (const float*)dSin.data(),
                               c.use_state ? (const SeqState*)dState.data() : nullptr, c.use_state ? 0 : c.pos, c.use_state ? 0 : c.pos + c.rope_off,
                               (float*)dY.data(), kv, st);
            break;
        }
        case FS_GEMV_FFN_UP:
            w.w13 = dW.data(); w.ffn_norm = (const float*)dG.data(); w.s_13 = scale;
            LmKernels<WT>::ffn_up(d, (const float*)dX.data(), w, (float*)dY.data(), st);
            break;
        case FS_GEMV_FFN_DOWN:
            w.w2 = dW.data(); w.s_2 = scale;
            LmKernels<WT>::ffn_down(d, (const float*)dX.data(), w, (float*)dY.data(), st);
            break;
        case FS_GEMV_HEAD:
            LmKernels<WT>::head(d, (const float*)dX.data(), (const float*)dG.data(), dW.data(), scale, c.n_rows, (float*)dY.data(), st);
            break;
        default: {  // FS_GEMV_WO_BODY: one chunk per head, {o = x, m = 0, l = 1}, position 0 -> merge weight __expf(0) / (1 * __expf(0))
            w.wo = dW.data(); w.s_o = scale;
            std::vector<float> part((size_t)c.H * (c.Dh + 2));
            for (int h = 0; h < c.H; ++h) {
                for (int e = 0; e < c.Dh; ++e) part[(size_t)h * (c.Dh + 2) + e] = c.x[h * c.Dh + e];
                part[(size_t)h * (c.Dh + 2) + c.Dh] = 0.f; part[(size_t)h * (c.Dh + 2) + c.Dh + 1] = 1.f;
            }
            dPart.put(part.data(), part.size(), 4, st);
            dState.put(&hs, sizeof(SeqState), 1, st);  // pos = 0: T = 1, one chunk
            LmKernels<WT>::wo(d, (const float*)dPart.data(), 1, 1, (const SeqState*)dState.data(), nullptr, KVView{nullptr, nullptr, nullptr}, 0, w,
                              (float*)dY.data(), st);
            break;
        }
        }
    }
    if (o.y) FS_HIP(hipMemcpyAsync(o.y, dY.data(), I.n_y * 4, hipMemcpyDeviceToHost, st));
    std::vector<KT> hk(I.n_pool), hv(I.n_pool);
    if (I.n_pool) {
        FS_HIP(hipMemcpyAsync(hk.data(), dK.data(), I.n_pool * sizeof(KT), hipMemcpyDeviceToHost, st));
        FS_HIP(hipMemcpyAsync(hv.data(), dV.data(), I.n_pool * sizeof(KT), hipMemcpyDeviceToHost, st));
    }
    FS_HIP(hipStreamSynchronize(st));
    for (size_t i = 0; i < I.n_pool; ++i) { if (o.k) o.k[i] = gemv_f32<KT>(hk[i]); if (o.v) o.v[i] = gemv_f32<KT>(hv[i]); }
    bool ok = true;
    for (const GemvDev* b : {&dY, &dK, &dV}) ok = b->intact(st) && ok;
    o.guard_ok = ok ? 1 : 0;
}
}  // namespace

void gemv_selftest(int device, const fs_gemv_case& c, fs_gemv_out& o) {
    GemvCaseInfo I;
    gemv_validate(c, I);
    std::snprintf(o.variant, o.variant_cap, "%s", I.name.c_str());
    o.grid[0] = (int32_t)I.gx; o.grid[1] = 1; o.grid[2] = 1;
    o.n_y = I.n_y; o.n_pool = I.n_pool;
    if (c.plan_only) return;
    gemv_req((!o.y || o.y_cap >= I.n_y) && ((!o.k && !o.v) || o.pool_cap >= I.n_pool), "an output capacity is too small");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) throw Error("no HIP device visible: libfishrt has no CPU fallback (MI355X / gfx950 required)");
    FS_REQUIRE(device >= 0 && device < ndev, "device_id out of range");
    FS_HIP(hipSetDevice(device));
    hipStream_t st = nullptr;
    FS_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    struct StreamGuard { hipStream_t s; ~StreamGuard() { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } } sg{st};
    if (c.wt == FS_GEMV_WT_F32) gemv_run<float>(c, I, o, st);
    else if (c.wt == FS_GEMV_WT_BF16) gemv_run<bf16_t>(c, I, o, st);
    else gemv_run<fp8_t>(c, I, o, st);
}

}  // namespace fs
