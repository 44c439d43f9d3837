// Dual-AR transformer kernels for gfx950 (MI355X): the batch-1 token path (GEMV kernels) first, then the MFMA row path (skinny
// GEMMs over activation rows) used by the prefill and by the static-batch generator.  The attention kernels of both paths are in
// lm_attn.hip, the on-device samplers in lm_sample.hip; the device helpers the three files use are in lm_dev.h.
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
#include <string>
#include <vector>

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

template <typename V>
__device__ __forceinline__ V ld_stream(const V* p) {  // streamed-once weights: non-temporal (guide: nt-weights)
    return __builtin_nontemporal_load(p);
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

template <typename WT>
__device__ __forceinline__ WT* kv_addr(void* pool, const int* __restrict__ page_table, int t, int g, int Hk, int Dh) {
    const int page = page_table[t / KV_PAGE];
    return reinterpret_cast<WT*>(pool) + ((size_t)(page * Hk + g) * KV_PAGE + (t % KV_PAGE)) * Dh;
}

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

// ------------------------------------------------------------------------------------------------ skinny GEMMs (MFMA)
// Activation ROWS against bf16 weights: the prefill (rows = up to 512 consecutive prompt tokens of one sequence per pass) and the
// batched decode step (rows = sequences).  Y[M, N] = f(A[M, K]) . W[N, K]^T, 32 rows (one MFMA column-tile pair) at a time.
// Numerics: activations stay f32-grade end to end -- every GEMM input is split once into bf16 hi + bf16 lo parts
// (a = hi + lo up to 2^-17 relative; k_prep / producer epilogues) and both parts go through v_mfma_f32_16x16x32_bf16 with
// f32 accumulation, so the MFMA path agrees with the f32-activation GEMV path far below bf16 resolution (the reference's
// own CUDA path rounds activations to bf16).  Kernel: k_gemm3 below (A operand = weights straight from global, non-temporal;
// B operand = fragment-major activations straight from L2; no LDS staging).
constexpr int PF_M = 32;    // activation rows per pass

// EPI_QKV_SEQ: EPI_QKV for a group prefill pass whose sequences start at different positions -- sequence s of the pass sits at
// state[s].pos (+ state[s].rope_off); its own instantiation, so that the other QKV GEMMs compile exactly as without it
enum { EPI_STORE = 0, EPI_RESIDUAL = 1, EPI_SWIGLU = 2, EPI_QKV = 3, EPI_RESIDUAL_NORM = 4, EPI_SWIGLU_RMS = 5, EPI_QKV_RMS = 6, EPI_STORE_RMS = 7,
       EPI_QKV_SEQ = 8 };
// epilogues that divide the K-summed accumulators by the row's rms (the producer left split(x * g) and sum-of-squares partials: NormAux)
__host__ __device__ constexpr bool epi_rms(int e) { return e == EPI_SWIGLU_RMS || e == EPI_QKV_RMS || e == EPI_STORE_RMS; }
// RMSNorm folded into the GEMMs around it (saves the k_prep node between Wo and W13): the Wo GEMM's epilogue writes the new
// residual stream, the UN-normalised GEMM input split(x * g) and one sum-of-squares partial per (block, row); the W13 GEMM's
// epilogue divides its accumulators by rms[m] = sqrt(sum_b partial[m][b] / D + eps) (a per-row scalar commutes with the GEMM).
struct NormAux {
    const float* g;   // norm weight [D]                       (EPI_RESIDUAL_NORM)
    float* ss;        // partials [Mcap][nblk], row-major       (written by RESIDUAL_NORM, read by SWIGLU_RMS)
    bf16_t* A2;       // fragment-major output of RESIDUAL_NORM
    int nblk;         // blocks of the producing GEMM (multiple of 8)
    int D;
    float eps;
};

struct RowMap {       // how activation row m maps onto sequences / positions
    int pos_step;     // prefill: 1 (row m = token at pos + m of ONE sequence); batched decode: 0 (every row at pos)
    int pt_stride;    // prefill: 0 (one page table); batched decode: page-table stride between sequences
    int seq_rows;     // > 0: group prefill -- row m = token (m % seq_rows) of sequence (m / seq_rows), page tables pt_stride apart
};

// X[m] (+= sum_s P[s][m], fixed order) ; optional RMSNorm ; emit bf16 hi/lo (fragment-major).  One block per row.
__global__ __launch_bounds__(256) void k_prep(float* __restrict__ X, int D, const float* __restrict__ P, int S, size_t slab_stride,
                                              const float* __restrict__ norm_w, float eps, bf16_t* __restrict__ Ohi) {
    __shared__ float red[4];
    const int m = blockIdx.x;
    float* xm = X + (size_t)m * D;
    float ss = 0.f;
    // D <= 1024 (every row-path model here): a thread's one float4 stays in registers between the two phases -- the second phase used to
    // read the row back from memory behind the block barrier, one more dependent L2 round trip in a node that is nothing but latency
    const bool one = D <= 1024;
    float4 keep = make_float4(0.f, 0.f, 0.f, 0.f), wkeep = make_float4(1.f, 1.f, 1.f, 1.f);
    if (one && norm_w && threadIdx.x * 4 < D) wkeep = *reinterpret_cast<const float4*>(norm_w + threadIdx.x * 4);  // (requested with the row, not behind the barrier)
    for (int e = threadIdx.x * 4; e < D; e += 1024) {
        float4 v = *reinterpret_cast<const float4*>(xm + e);
        for (int sI = 0; sI < S; ++sI) {
            const float4 p = *reinterpret_cast<const float4*>(P + (size_t)sI * slab_stride + (size_t)m * D + e);
            v.x += p.x; v.y += p.y; v.z += p.z; v.w += p.w;
        }
        if (S > 0) *reinterpret_cast<float4*>(xm + e) = v;
        ss = fmaf(v.x, v.x, ss); ss = fmaf(v.y, v.y, ss); ss = fmaf(v.z, v.z, ss); ss = fmaf(v.w, v.w, ss);
        keep = v;
    }
    if (!Ohi) return;
    float d = 1.f;
    if (norm_w) {
        ss = wave_sum(ss);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
        __syncthreads();
        d = sqrtf(((red[0] + red[1]) + (red[2] + red[3])) / (float)D + eps);
    }
    for (int e = threadIdx.x * 4; e < D; e += 1024) {
        const float4 v = one ? keep : *reinterpret_cast<const float4*>(xm + e);  // (else: own earlier write, same thread)
        float a[4] = {v.x, v.y, v.z, v.w};
        if (norm_w) {
            const float4 w = one ? wkeep : *reinterpret_cast<const float4*>(norm_w + e);
            a[0] = (a[0] / d) * w.x; a[1] = (a[1] / d) * w.y; a[2] = (a[2] / d) * w.z; a[3] = (a[3] / d) * w.w;
        }
        store_frag4(Ohi, m, e, D, a);
    }
}

// Epilogue of the row-path GEMMs for one (row pair r/r+1, activation row m): a, b are the K-summed (and fp8-scaled) dot products.
// Thread mapping contract: the ROWS / 2 threads of one m are adjacent lanes (RESIDUAL_NORM's sum of squares meets by shuffles).
struct GemmEpi {
    float* Y; int ldy; size_t slab_stride; bf16_t* Of; int ldo;
    const float *cos_t, *sin_t;
    KVView kv; int H, Hk, Dh; RowMap rm; NormAux na;
    int pos0, rope_off, N;
    const SeqState* states = nullptr;  // pos_step < 0: row m reads its own position (session slots)
    bf16_t* o1 = nullptr;              // EPI_QKV*: every row sits at position 0 of an empty cache (the fast decoder's first pass): attention over one
                                       // token is the identity on V, so the V rows also leave the attention output (hi = the cached bf16 value, lo = 0:
                                       // exactly what the attention node computes for T = 1) in fragment-major order and that node is not launched
};
// values the epilogue needs from memory that do not depend on the GEMM: requested at kernel entry by k_gemm3 (one slot per thread, first
// panel) so that they arrive under the weight stream instead of starting a dependent L2 round trip behind the K loop
struct EpiPre { float2 o; float2 g; float cs, sn; };
template <int EPI, int ROWS>
__device__ __forceinline__ void gemm_epilogue(float a, float b, int r, int m, int ml, int pr, const GemmEpi& g, const float* s_rms,
                                              const EpiPre* pre = nullptr) {
    float* const Y = g.Y; const int ldy = g.ldy, ldo = g.ldo, N = g.N, H = g.H, Hk = g.Hk, Dh = g.Dh, pos0 = g.pos0, rope_off = g.rope_off;
    const size_t slab_stride = g.slab_stride;
    bf16_t* const Of = g.Of;
    const float *cos_t = g.cos_t, *sin_t = g.sin_t;
    const KVView& kv = g.kv; const RowMap& rm = g.rm; const NormAux& na = g.na;
    if (EPI == EPI_QKV_RMS || EPI == EPI_STORE_RMS) { const float dn = s_rms[ml]; a /= dn; b /= dn; }  // (a per-row scalar commutes with the GEMM)
    if (EPI == EPI_STORE || EPI == EPI_STORE_RMS) {  // split-K slab blockIdx.y
        float* yp = Y + (size_t)blockIdx.y * slab_stride + (size_t)m * ldy + r;
        yp[0] = a;
        if (r + 1 < N) yp[1] = b;
    } else if (EPI == EPI_RESIDUAL) {
        float2* yp = reinterpret_cast<float2*>(Y + (size_t)m * ldy + r);
        const float2 o = pre ? pre->o : *yp;
        *yp = make_float2(o.x + a, o.y + b);
    } else if (EPI == EPI_RESIDUAL_NORM) {  // the ROWS/2 threads of one m are adjacent lanes (8, 16 or 32 of them)
        float2* yp = reinterpret_cast<float2*>(Y + (size_t)m * ldy + r);
        const float2 o = pre ? pre->o : *yp;
        const float v0 = o.x + a, v1 = o.y + b;
        *yp = make_float2(v0, v1);
        bf16_t h0, l0, h1, l1;
        const float2 gw = pre ? pre->g : make_float2(na.g[r], na.g[r + 1]);
        split_bf16(v0 * gw.x, h0, l0); split_bf16(v1 * gw.y, h1, l1);
        *reinterpret_cast<uint32_t*>(na.A2 + frag_off(m, r, 0, na.D)) = h0 | ((uint32_t)h1 << 16);
        *reinterpret_cast<uint32_t*>(na.A2 + frag_off(m, r, 1, na.D)) = l0 | ((uint32_t)l1 << 16);
        float ssq = group_sum<(ROWS / 2 >= 16 ? 16 : ROWS / 2)>(fmaf(v0, v0, v1 * v1));
        if (ROWS / 2 == 32) ssq += __shfl_xor(ssq, 16, 64);
        if (pr == 0) na.ss[(size_t)m * na.nblk + blockIdx.x] = ssq;
    } else if (EPI == EPI_SWIGLU_RMS) {
        const float dn = s_rms[ml];
        const float an = a / dn, bn = b / dn;
        const float v = (an / (1.f + __expf(-an))) * bn;
        bf16_t hh, ll;
        split_bf16(v, hh, ll);
        Of[frag_off(m, r / 2, 0, ldo)] = hh;
        Of[frag_off(m, r / 2, 1, ldo)] = ll;
    } else if (EPI == EPI_SWIGLU) {  // interleaved rows (2r, 2r+1) = (w1[r], w3[r]) -> act hi/lo for the down GEMM
        const float v = (a / (1.f + __expf(-a))) * b;
        bf16_t h, l;
        split_bf16(v, h, l);
        Of[frag_off(m, r / 2, 0, ldo)] = h;
        Of[frag_off(m, r / 2, 1, ldo)] = l;
    } else {  // EPI_QKV: rope_i + scatter (q -> Y[m][r], k/v -> paged cache of row m's sequence)
        const int sq = rm.seq_rows > 0 ? m / rm.seq_rows : m;  // sequence of row m / its token index within the pass
        int pos = pos0 + (rm.seq_rows > 0 ? m - sq * rm.seq_rows : m * rm.pos_step), rpos = pos + rope_off;
        if (rm.pos_step < 0) { pos = g.states[m].pos; rpos = pos + g.states[m].rope_off; }
        if (EPI == EPI_QKV_SEQ) { pos = g.states[sq].pos + (m - sq * rm.seq_rows); rpos = pos + g.states[sq].rope_off; }
        const int* ptab = kv.page_table + (size_t)sq * rm.pt_stride;
        const int qdim = H * Dh, kdim = Hk * Dh, half = Dh / 2;
        if (r < qdim + kdim) {
            const int j = (r % Dh) / 2;
            const float cs = pre ? pre->cs : cos_t[(size_t)rpos * half + j], sn = pre ? pre->sn : sin_t[(size_t)rpos * half + j];
            const float o0 = a * cs - b * sn, o1 = a * sn + b * cs;
            if (r < qdim) { *reinterpret_cast<float2*>(Y + (size_t)m * ldy + r) = make_float2(o0, o1); }
            else {
                const int rk = r - qdim;
                bf16_t* dst = kv_addr<bf16_t>(kv.k, ptab, pos, rk / Dh, Hk, Dh) + rk % Dh;
                *reinterpret_cast<uint32_t*>(dst) = WTr<bf16_t>::from_f32(o0) | ((uint32_t)WTr<bf16_t>::from_f32(o1) << 16);
            }
        } else {
            const int rv = r - qdim - kdim;
            bf16_t* dst = kv_addr<bf16_t>(kv.v, ptab, pos, rv / Dh, Hk, Dh) + rv % Dh;
            const uint32_t vb2 = WTr<bf16_t>::from_f32(a) | ((uint32_t)WTr<bf16_t>::from_f32(b) << 16);
            *reinterpret_cast<uint32_t*>(dst) = vb2;
            if (g.o1) {
                const int n_rep = H / Hk, gk = rv / Dh, dd = rv % Dh;
                for (int hh = 0; hh < n_rep; ++hh) {
                    const int e = (gk * n_rep + hh) * Dh + dd;
                    *reinterpret_cast<uint32_t*>(g.o1 + frag_off(m, e, 0, qdim)) = vb2;
                    *reinterpret_cast<uint32_t*>(g.o1 + frag_off(m, e, 1, qdim)) = 0u;
                }
            }
        }
    }
}

// Block = 16*RT weight rows x one K range of 128*NKS (the 4 waves take a quarter each, NKS k-steps of 32) x ALL activation
// rows, 32 at a time.  No LDS staging and no barrier in front of the MFMAs: a wave puts its whole weight panel in flight at
// kernel entry (A operand, non-temporal, kept in VGPRs for every row panel), then per 32-row panel loads its B operands
// (hi + lo slices of the activations, 16 B per lane per slice, L2-resident) straight into VGPRs and runs NKS * RT * 4 MFMAs.
// The four K-quarter accumulators meet in 8 KB of LDS and are summed in a fixed order; the epilogue gives every thread
// one (row pair, m) so RoPE pairs and SwiGLU (w1[r], w3[r]) pairs stay in one lane.  Small grids were the problem of the
// first version of this kernel (64-row blocks: 20 blocks for Wqkv); 16-row blocks give 80 / 64 / 512 (256 with RT = 2) / 256.
// FP8: the weights are e4m3fn bytes + one f32 scale per row (FS_FP8 handles): a lane's 8 bytes per k-step are widened to bf16 in
// registers (exact: e4m3 has 3 mantissa bits) and the row scale is applied to the K-summed accumulator in the epilogue.
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ u32x4 fp8x8_to_bf16x8(u32x2 v) {
    u32x4 o;
    const uint32_t w[2] = {v.x, v.y};
    uint32_t r[4];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(w[i], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8(w[i], true);
        r[2 * i] = (__float_as_uint(lo.x) >> 16) | (__float_as_uint(lo.y) & 0xFFFF0000u);
        r[2 * i + 1] = (__float_as_uint(hi.x) >> 16) | (__float_as_uint(hi.y) & 0xFFFF0000u);
    }
    o.x = r[0]; o.y = r[1]; o.z = r[2]; o.w = r[3];
    return o;
}
// HALF: M <= 16 (small static batches) -- rows 16..31 of the only panel do not exist: their operand loads and MFMAs are skipped.
template <int EPI, int NKS, int RT, bool FP8, bool HALF = false>
__global__ __launch_bounds__(256) void k_gemm3(const bf16_t* __restrict__ Xf, int M, int K,
                                               const void* __restrict__ Wv, const float* __restrict__ wscale, int N, float* __restrict__ Y, int ldy, size_t slab_stride,
                                               bf16_t* __restrict__ Of, int ldo,
                                               const float* __restrict__ cos_t, const float* __restrict__ sin_t,
                                               const SeqState* __restrict__ state, KVView kv, int H, int Hk, int Dh, RowMap rm, NormAux na) {
    constexpr int ROWS = 16 * RT;
    __shared__ float red[4][ROWS][33];
    __shared__ float s_rms[PF_M];
    const int lane = threadIdx.x & 63, kq = threadIdx.x >> 6;
    const int n0 = blockIdx.x * ROWS;
    const int kbeg = ((int)blockIdx.y * 4 + kq) * NKS * 32 + (lane >> 4) * 8;  // this lane's first k of every 32-wide step (weights)
    int pos0 = 0, rope_off = 0;
    if (EPI == EPI_QKV || EPI == EPI_QKV_RMS) { pos0 = state->pos; rope_off = state->rope_off; }  // requested up front: the epilogue must not start a dependent chain
    const GemmEpi ge{Y, ldy, slab_stride, Of, ldo, cos_t, sin_t, kv, H, Hk, Dh, rm, na, pos0, rope_off, N, state,
                     (EPI == EPI_QKV || EPI == EPI_QKV_RMS || EPI == EPI_QKV_SEQ) ? Of : nullptr};  // (Of of a QKV launch: GemmEpi::o1)
    u32x4 wf[RT][NKS];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const size_t woff = (size_t)min(n0 + rt * 16 + (lane & 15), N - 1) * K + kbeg;
        if (FP8) {
            const uint8_t* wp = reinterpret_cast<const uint8_t*>(Wv) + woff;
            u32x2 raw[NKS];
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) raw[ks] = ld_stream(reinterpret_cast<const u32x2*>(wp + ks * 32));
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) wf[rt][ks] = fp8x8_to_bf16x8(raw[ks]);
        } else {
            const bf16_t* wp = reinterpret_cast<const bf16_t*>(Wv) + woff;
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) wf[rt][ks] = ld_stream(reinterpret_cast<const u32x4*>(wp + ks * 32));
        }
    }
    // one epilogue slot per thread (RT == 1): what that slot reads from memory is requested now, behind the weight stream (first panel)
    constexpr bool PRE_RES = RT == 1 && (EPI == EPI_RESIDUAL || EPI == EPI_RESIDUAL_NORM), PRE_QKV = RT == 1 && (EPI == EPI_QKV || EPI == EPI_QKV_RMS);
    EpiPre pre{make_float2(0.f, 0.f), make_float2(1.f, 1.f), 1.f, 0.f};
    const int pre_r = n0 + 2 * ((int)threadIdx.x % (ROWS / 2)), pre_m = (int)blockIdx.z * PF_M + (int)threadIdx.x / (ROWS / 2);
    bool use_pre = PRE_RES;
    if (PRE_RES && pre_r < N && pre_m < M) {
        pre.o = *reinterpret_cast<const float2*>(Y + (size_t)pre_m * ldy + pre_r);
        if (EPI == EPI_RESIDUAL_NORM) pre.g = *reinterpret_cast<const float2*>(na.g + pre_r);
    }
    if (PRE_QKV) use_pre = rm.pos_step == 0 && rm.seq_rows == 0;  // lock-step decode rows: every row at state->pos (block-uniform)
    // row panels are spread over blockIdx.z (prefill: many panels -> more blocks; the weight tile is then re-read from L2)
    bool first_panel = true;
    for (int mp = (int)blockIdx.z * PF_M; mp < M; mp += (int)gridDim.z * PF_M) {
        float ss8 = 0.f;
        if (epi_rms(EPI)) {  // this panel's 32 row norms: thread (m = tid/8, j = tid%8) sums every 8th block's partial, then 8 lanes meet
            const float* sp = na.ss + (size_t)(mp + (threadIdx.x >> 3)) * na.nblk + (threadIdx.x & 7);
            for (int q8 = 0; q8 < na.nblk; q8 += 8) ss8 += sp[q8];
        }
        // B operands of this panel (fragment-major: [k-step][hi, lo][16-row tile] blocks of one KiB each, lane-major)
        const bf16_t* xp = Xf + ((size_t)(mp >> 5) * (K >> 5) + ((int)blockIdx.y * 4 + kq) * NKS) * 2048 + lane * 8;
        u32x4 xf[NKS][4];
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            xf[ks][0] = *reinterpret_cast<const u32x4*>(xp + ks * 2048);          // hi, rows 0..15
            xf[ks][1] = *reinterpret_cast<const u32x4*>(xp + ks * 2048 + 1024);   // lo, rows 0..15
            if (!HALF) {
                xf[ks][2] = *reinterpret_cast<const u32x4*>(xp + ks * 2048 + 512);    // hi, rows 16..31
                xf[ks][3] = *reinterpret_cast<const u32x4*>(xp + ks * 2048 + 1536);   // lo, rows 16..31
            }
        }
        if (PRE_QKV && first_panel && use_pre && pre_r < (H + Hk) * Dh) {  // (waits for the scalar position load; the operand loads are already out)
            const int j = (pre_r % Dh) / 2;
            pre.cs = cos_t[(size_t)(pos0 + rope_off) * (Dh / 2) + j]; pre.sn = sin_t[(size_t)(pos0 + rope_off) * (Dh / 2) + j];
        }
        FS_ISSUE_FENCE();  // every operand load of the panel is in flight before the first MFMA waits (the scheduler would
                           // otherwise meter them out a dozen at a time, one memory round trip per batch)
        f32x4v acc[RT][2];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) { acc[rt][0] = f32x4v{0.f, 0.f, 0.f, 0.f}; acc[rt][1] = f32x4v{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                const bf16x8 af = __builtin_bit_cast(bf16x8, wf[rt][ks]);
#pragma unroll
                for (int j = 0; j < (HALF ? 2 : 4); ++j)
                    acc[rt][j >> 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, __builtin_bit_cast(bf16x8, xf[ks][j]), acc[rt][j >> 1], 0, 0, 0);
            }
        if (!first_panel) __syncthreads();  // the previous panel's epilogue has read `red` (and s_rms)
        first_panel = false;
        if (epi_rms(EPI)) {
            const float tot = group_sum<8>(ss8);
            if ((threadIdx.x & 7) == 0) s_rms[threadIdx.x >> 3] = sqrtf(tot / (float)na.D + na.eps);
        }
        // lane holds C[row = rt*16 + (lane>>4)*4 + i][m = mt*16 + (lane&15)]
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                const f32x4v c = acc[rt][mt];
                float* rp = &red[kq][rt * 16 + (lane >> 4) * 4][mt * 16 + (lane & 15)];
                rp[0] = c.x; rp[33] = c.y; rp[66] = c.z; rp[99] = c.w;
            }
        __syncthreads();
        // epilogue: slot = (row pair, m); K-quarters summed in a fixed order
#pragma unroll
        for (int sI = 0; sI < RT; ++sI) {
            const int slot = sI * 256 + (int)threadIdx.x;
            const int pr = slot % (ROWS / 2), ml = slot / (ROWS / 2);
            const int r = n0 + 2 * pr, m = mp + ml;
            float a = (red[0][2 * pr][ml] + red[1][2 * pr][ml]) + (red[2][2 * pr][ml] + red[3][2 * pr][ml]);
            float b = (red[0][2 * pr + 1][ml] + red[1][2 * pr + 1][ml]) + (red[2][2 * pr + 1][ml] + red[3][2 * pr + 1][ml]);
            if (r >= N || m >= M) continue;
            if (FP8) { a *= wscale[r]; b *= wscale[min(r + 1, N - 1)]; }
            gemm_epilogue<EPI, ROWS>(a, b, r, m, ml, pr, ge, s_rms, (PRE_RES || PRE_QKV) && use_pre && mp == (int)blockIdx.z * PF_M ? &pre : nullptr);
        }
    }
}

constexpr unsigned DOWN_SPIN_MAX = 1u << 17;  // polls of an in-launch exchange unit before a thread gives up (~0.1 s; reported through epoch[1])
// ---- down projection of a decode step (M <= 32 rows) that closes the layer itself: split-K over gridDim.y blocks per 16-row weight tile
// as before (every CU streams a 32 KB weight tile: the K depth of 4096 needs all of them), but the K partials meet INSIDE the launch
// instead of in slabs + a k_prep node: thread (row pair pr, activation row ml) of block y publishes its two partial sums as one 16-byte
// unit {a, tag, b, tag} (relaxed agent-scope write-through store, each 8-byte half self-validating -- the edge protocol of the persistent
// decode kernels, lm_persist_dev.h) unless block y owns row ml; wave y of block y owns rows [y * 32 / ksplit, (y + 1) * 32 / ksplit):
// it sweeps the other blocks' units of its slots (sc1 loads, retried until both tags match), adds the partials in block order and runs the
// epilogue -- x += sum (residual stream), split(x * g_next) in fragment-major order for the next GEMM and one sum-of-squares partial per
// (tile, row); the next GEMM divides its accumulators by the row's rms (EPI_QKV_RMS / EPI_STORE_RMS).  One of six graph nodes per layer
// (~5 us each at 32 rows whatever they do) becomes a ~1 us in-launch hand-off among the <= 4 blocks of a tile, which share an XCD
// (linear block id = tile + gridDim.x * y, gridDim.x % 8 == 0).  tag = step epoch * 4096 + node id: a unit is rewritten by every node
// that uses the buffer, so a stale unit always carries the tag of the previous node or step.
// Measured and rejected first (round 5): the same layer-closing epilogue on an UN-split block (16 weight rows x 16 activation rows x the
// whole depth, 128 blocks): 9.0 us per node against 5.0 + 5.1 for the split GEMM + k_prep -- 384 KB of operands through ONE CU's vector
// memory path at one wave per SIMD is ~55 GB/s per CU.
template <int NKS, bool FP8>
__global__ __launch_bounds__(256) void k_gemm_down(const bf16_t* __restrict__ Xf, int M, int K, const void* __restrict__ Wv,
                                                   const float* __restrict__ wscale, int N, float* __restrict__ Y, int ldy, NormAux na,
                                                   u32x4* __restrict__ xchg, uint32_t* __restrict__ epoch, uint32_t node_id, int nap) {
    __shared__ float red[4][16][33];
    const int lane = threadIdx.x & 63, kq = threadIdx.x >> 6;
    const int n0 = blockIdx.x * 16, y = blockIdx.y, ksplit = gridDim.y, rows_per = PF_M / ksplit;
    const unsigned tag = epoch[0] * 4096u + node_id;
    const int pr = threadIdx.x & 7, ml = threadIdx.x >> 3;   // epilogue slot: rows (r, r + 1) of activation row ml
    const int r = n0 + 2 * pr;
    const bool owner = ml / rows_per == y;                  // == (kq == y) for ksplit == 4; wave-uniform for every ksplit
    float2 xo = make_float2(0.f, 0.f), gw = make_float2(1.f, 1.f), sc = make_float2(1.f, 1.f);
    const int kbeg = (y * 4 + kq) * NKS * 32 + (lane >> 4) * 8;
    u32x4 wf[NKS];
    {
        const size_t woff = (size_t)(n0 + (lane & 15)) * K + kbeg;
        if (FP8) {
            const uint8_t* wp = reinterpret_cast<const uint8_t*>(Wv) + woff;
            u32x2 raw[NKS];
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) raw[ks] = ld_stream(reinterpret_cast<const u32x2*>(wp + ks * 32));
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) wf[ks] = fp8x8_to_bf16x8(raw[ks]);
        } else {
            const bf16_t* wp = reinterpret_cast<const bf16_t*>(Wv) + woff;
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) wf[ks] = ld_stream(reinterpret_cast<const u32x4*>(wp + ks * 32));
        }
    }
    const bf16_t* xp = Xf + (size_t)((y * 4 + kq) * NKS) * 2048 + lane * 8;
    u32x4 xf[NKS][4];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
        xf[ks][0] = *reinterpret_cast<const u32x4*>(xp + ks * 2048);          // hi, rows 0..15
        xf[ks][1] = *reinterpret_cast<const u32x4*>(xp + ks * 2048 + 1024);   // lo, rows 0..15
        xf[ks][2] = *reinterpret_cast<const u32x4*>(xp + ks * 2048 + 512);    // hi, rows 16..31
        xf[ks][3] = *reinterpret_cast<const u32x4*>(xp + ks * 2048 + 1536);   // lo, rows 16..31
    }
    if (owner) {  // what the epilogue reads from memory does not depend on the GEMM: requested behind the operands
        if (ml < M) xo = *reinterpret_cast<const float2*>(Y + (size_t)ml * ldy + r);
        gw = *reinterpret_cast<const float2*>(na.g + r);
    }
    if (FP8) sc = *reinterpret_cast<const float2*>(wscale + r);
    FS_ISSUE_FENCE();
    f32x4v acc[2] = {f32x4v{0.f, 0.f, 0.f, 0.f}, f32x4v{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
        const bf16x8 af = __builtin_bit_cast(bf16x8, wf[ks]);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j >> 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, __builtin_bit_cast(bf16x8, xf[ks][j]), acc[j >> 1], 0, 0, 0);
    }
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {  // lane holds C[row = (lane>>4)*4 + i][m = mt*16 + (lane&15)]
        const f32x4v c = acc[mt];
        float* rp = &red[kq][(lane >> 4) * 4][mt * 16 + (lane & 15)];
        rp[0] = c.x; rp[33] = c.y; rp[66] = c.z; rp[99] = c.w;
    }
    __syncthreads();
    float a = (red[0][2 * pr][ml] + red[1][2 * pr][ml]) + (red[2][2 * pr][ml] + red[3][2 * pr][ml]);
    float b = (red[0][2 * pr + 1][ml] + red[1][2 * pr + 1][ml]) + (red[2][2 * pr + 1][ml] + red[3][2 * pr + 1][ml]);
    if (FP8) { a *= sc.x; b *= sc.y; }
    // unit of (tile, source block, row, pair)
    u32x4* const units = xchg + ((size_t)blockIdx.x * ksplit * PF_M + ml) * 8 + pr;
    if (!owner) {
        const u32x4 u = {__float_as_uint(a), tag, __float_as_uint(b), tag};
        asm volatile("global_store_dwordx4 %0, %1, off sc1" : : "v"(units + (size_t)y * PF_M * 8), "v"(u) : "memory");
        return;
    }
    // the other blocks' units of this slot: all requests in flight together, retried (only the missing ones) until both tags of each match.
    // The partners finish their K quarter when this block does and their stores take ~1 us to become visible: polling from the first instant
    // only re-reads units that cannot be there yet (memory-side traffic in front of the stores everybody waits for), so the sweep starts
    // `nap` x 64 clocks later (as the persistent kernels' pre-sweep naps)
    for (int i = 0; i < nap; ++i) __builtin_amdgcn_s_sleep(1);
    u32x4 pv[4];
    {
        bool ok[4];
#pragma unroll
        for (int ys = 0; ys < 4; ++ys) { ok[ys] = ys >= ksplit || ys == y; pv[ys] = u32x4{0u, 0u, 0u, 0u}; }
        for (unsigned spins = 0;; ++spins) {
#pragma unroll
            for (int ys = 0; ys < 4; ++ys)
                if (!ok[ys]) asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=v"(pv[ys]) : "v"(units + (size_t)ys * PF_M * 8) : "memory");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            bool all = true;
#pragma unroll
            for (int ys = 0; ys < 4; ++ys) {
                // (the asm outputs above are only written when the load was issued; keep the compiler from assuming otherwise)
                asm volatile("" : "+v"(pv[ys]));
                if (!ok[ys]) ok[ys] = pv[ys].y == tag && pv[ys].w == tag;
                all = all && ok[ys];
            }
            if (all) break;
            if (spins > DOWN_SPIN_MAX) { atomicAdd(epoch + 1, 1u); break; }  // (reported: check_rows_xchg)
        }
    }
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int ys = 0; ys < 4; ++ys)  // partials in block order (the own one from registers)
        if (ys < ksplit) {
            s0 += ys == y ? a : __uint_as_float(pv[ys].x);
            s1 += ys == y ? b : __uint_as_float(pv[ys].z);
        }
    const float v0 = xo.x + s0, v1 = xo.y + s1;
    const bool live = ml < M;
    const float ssq = group_sum<8>(live ? fmaf(v0, v0, v1 * v1) : 0.f);
    if (!live) return;
    *reinterpret_cast<float2*>(Y + (size_t)ml * ldy + r) = make_float2(v0, v1);
    bf16_t h0, l0, h1, l1;
    split_bf16(v0 * gw.x, h0, l0); split_bf16(v1 * gw.y, h1, l1);
    *reinterpret_cast<uint32_t*>(na.A2 + frag_off(ml, r, 0, na.D)) = h0 | ((uint32_t)h1 << 16);
    *reinterpret_cast<uint32_t*>(na.A2 + frag_off(ml, r, 1, na.D)) = l0 | ((uint32_t)l1 << 16);
    if (pr == 0) na.ss[(size_t)ml * na.nblk + blockIdx.x] = ssq;
}

// ---- large-M variant (M >= GB_MIN_M rows: prefill passes, group prefill, big static batches) ---------------------------------
// k_gemm3 re-reads a panel's activation fragments once per 16 (or 32) weight rows through the CU's vector L1, which bounds it at
// 64 B/clk; with many panels that traffic, not the weight stream, is the cost.  Here a block owns 64 weight rows x one 1024-deep
// K range (wave = (K half, 32-row group): 2 A tiles x 16 k-steps stay in VGPRs for every panel) and the panel's fragments go
// through LDS once per block: 4-k-step chunks (32 KB: both K halves), double-buffered, global loads for chunk i+1 in flight
// during the 32 MFMAs per wave of chunk i; every fragment read from LDS feeds two A tiles.  Per chunk and block: 32 KB through
// L1, 64 KB of LDS reads, 128 MFMAs -- the three pipes are balanced.  The two K halves meet in LDS (aliased onto the stage
// buffer that was just consumed) and the epilogue is the one of k_gemm3 (ROWS = 64).
constexpr int GB_ROWS = 64, GB_CH = 4, GB_MIN_M = 128;
static int gemm_big_min_m() {  // FISHRT_GEMM_BIG_MIN_M: tuning / test hook (rows from which the LDS-staged variant is taken)
    static const int v = [] { const char* e = std::getenv("FISHRT_GEMM_BIG_MIN_M"); return e ? std::atoi(e) : GB_MIN_M; }();
    return v;
}
// measured (tools/ubench_gemm, Fish-1.5 shapes): a block's fixed cost (128 KB weight tile + 4 latency-exposed chunk rounds) is
// ~8 us, so the variant wins from 128 rows for the wide GEMMs (W13: 128 tiles, W2: 16 tiles x 4 K ranges) and only from
// ~512 rows for Wqkv / Wo (20 / 16 tiles)
static bool gemm_big_ok(int M, int N, int K, int ksplit) {
    if (K % ksplit != 0 || K / ksplit != 1024) return false;
    const int m0 = gemm_big_min_m();
    return M >= 4 * m0 || (M >= m0 && (N + GB_ROWS - 1) / GB_ROWS * ksplit >= 64);
}
template <int EPI, bool FP8>
__global__ __launch_bounds__(256, 2) void k_gemm_big(const bf16_t* __restrict__ Xf, int M, int K,
                                                     const void* __restrict__ Wv, const float* __restrict__ wscale, int N, float* __restrict__ Y, int ldy,
                                                     size_t slab_stride, bf16_t* __restrict__ Of, int ldo,
                                                     const float* __restrict__ cos_t, const float* __restrict__ sin_t,
                                                     const SeqState* __restrict__ state, KVView kv, int H, int Hk, int Dh, RowMap rm, NormAux na) {
    constexpr int ROWS = GB_ROWS, NKS = 16, STAGE = 2 * GB_CH * 4096;  // bytes per stage: 2 K halves x 4 k-steps x 4 KB
    __shared__ __attribute__((aligned(16))) uint8_t lds[2 * STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kh = wave >> 1, rg = wave & 1;
    const int n0 = blockIdx.x * ROWS;
    int mp = (int)blockIdx.z * PF_M;
    if (mp >= M) return;
    int pos0 = 0, rope_off = 0;
    if (EPI == EPI_QKV || EPI == EPI_QKV_RMS) { pos0 = state->pos; rope_off = state->rope_off; }
    const GemmEpi ge{Y, ldy, slab_stride, Of, ldo, cos_t, sin_t, kv, H, Hk, Dh, rm, na, pos0, rope_off, N, state};
    const int ksw = (int)blockIdx.y * 32 + kh * NKS;  // this wave's first 32-deep k-step
    u32x4 wf[2][NKS];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const size_t woff = (size_t)min(n0 + rg * 32 + t * 16 + (lane & 15), N - 1) * K + (size_t)ksw * 32 + (lane >> 4) * 8;
        if (FP8) {
            const uint8_t* wp = reinterpret_cast<const uint8_t*>(Wv) + woff;
            u32x2 raw[NKS];
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) raw[ks] = ld_stream(reinterpret_cast<const u32x2*>(wp + ks * 32));
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) wf[t][ks] = fp8x8_to_bf16x8(raw[ks]);
        } else {
            const bf16_t* wp = reinterpret_cast<const bf16_t*>(Wv) + woff;
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) wf[t][ks] = ld_stream(reinterpret_cast<const u32x4*>(wp + ks * 32));
        }
    }
    // chunk c of panel p: thread unit i -> K half i >> 2, k-step i & 3 of the chunk, 16-B slot tid of that k-step's 4 KB block
    u32x4 g[8];
    auto load_chunk = [&](int p, int c) {
        const bf16_t* base = Xf + ((size_t)(p >> 5) * (K >> 5) + (size_t)blockIdx.y * 32 + c * GB_CH) * 2048 + tid * 8;
#pragma unroll
        for (int i = 0; i < 8; ++i) g[i] = *reinterpret_cast<const u32x4*>(base + (size_t)((i >> 2) * NKS + (i & 3)) * 2048);
    };
    auto store_chunk = [&](int sb) {
        uint8_t* dst = lds + sb * STAGE + tid * 16;
#pragma unroll
        for (int i = 0; i < 8; ++i) *reinterpret_cast<u32x4*>(dst + i * 4096) = g[i];
    };
    load_chunk(mp, 0);
    store_chunk(0);
    __syncthreads();
    int sb = 0;
    const int mstep = (int)gridDim.z * PF_M;
    for (; mp < M; mp += mstep) {
        const int mp_next = mp + mstep;
        float ss8 = 0.f;
        if (epi_rms(EPI)) {
            const float* sp = na.ss + (size_t)(mp + (tid >> 3)) * na.nblk + (tid & 7);
            for (int q8 = 0; q8 < na.nblk; q8 += 8) ss8 += sp[q8];
        }
        f32x4v acc[2][2];
#pragma unroll
        for (int t = 0; t < 2; ++t) { acc[t][0] = f32x4v{0.f, 0.f, 0.f, 0.f}; acc[t][1] = f32x4v{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
        for (int c = 0; c < NKS / GB_CH; ++c) {
            const bool has_next = c + 1 < NKS / GB_CH || mp_next < M;
            if (has_next) load_chunk(c + 1 < NKS / GB_CH ? mp : mp_next, (c + 1) % (NKS / GB_CH));
            const uint8_t* src = lds + sb * STAGE + kh * (GB_CH * 4096) + lane * 16;
#pragma unroll
            for (int ks = 0; ks < GB_CH; ++ks) {
                bf16x8 xf[4];  // hi rows 0..15, lo rows 0..15, hi rows 16..31, lo rows 16..31 (order of k_gemm3)
                xf[0] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(src + ks * 4096));
                xf[1] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(src + ks * 4096 + 2048));
                xf[2] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(src + ks * 4096 + 1024));
                xf[3] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(src + ks * 4096 + 3072));
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const bf16x8 af = __builtin_bit_cast(bf16x8, wf[t][c * GB_CH + ks]);
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[t][j >> 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, xf[j], acc[t][j >> 1], 0, 0, 0);
                }
            }
            if (c == NKS / GB_CH - 1) {  // panel complete: the K halves meet in the stage buffer that was just consumed
                float (*red)[ROWS][33] = reinterpret_cast<float (*)[ROWS][33]>(lds + sb * STAGE);
                float* s_rms = reinterpret_cast<float*>(lds + sb * STAGE + 2 * ROWS * 33 * sizeof(float));
                __syncthreads();
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt) {
                        const f32x4v cc = acc[t][mt];
                        float* rp = &red[kh][rg * 32 + t * 16 + (lane >> 4) * 4][mt * 16 + (lane & 15)];
                        rp[0] = cc.x; rp[33] = cc.y; rp[66] = cc.z; rp[99] = cc.w;
                    }
                if (epi_rms(EPI)) {
                    const float tot = group_sum<8>(ss8);
                    if ((tid & 7) == 0) s_rms[tid >> 3] = sqrtf(tot / (float)na.D + na.eps);
                }
                __syncthreads();
#pragma unroll
                for (int sI = 0; sI < ROWS / 16; ++sI) {
                    const int slot = sI * 256 + tid;
                    const int pr = slot % (ROWS / 2), ml = slot / (ROWS / 2);
                    const int r = n0 + 2 * pr, m = mp + ml;
                    float a = red[0][2 * pr][ml] + red[1][2 * pr][ml];
                    float b = red[0][2 * pr + 1][ml] + red[1][2 * pr + 1][ml];
                    if (r >= N || m >= M) continue;
                    if (FP8) { a *= wscale[r]; b *= wscale[min(r + 1, N - 1)]; }
                    gemm_epilogue<EPI, ROWS>(a, b, r, m, ml, pr, ge, s_rms);
                }
            }
            if (has_next) store_chunk(sb ^ 1);
            __syncthreads();
            sb ^= 1;
        }
    }
}

template <typename WT>
__global__ void k_embed_rows(const WT* __restrict__ tok_emb, const WT* __restrict__ cb_emb, int dim, int n_cb, int cb_size,
                             const SampleCfg* __restrict__ cfg, const uint32_t* __restrict__ prompt,
                             const SeqState* __restrict__ state, float* __restrict__ X, int seq_rows, size_t prompt_stride) {
    // seq_rows > 0: group pass -- row m = prompt column step + (m % seq_rows) of the (m / seq_rows)-th staged prompt
    const int m = blockIdx.x, sq = seq_rows > 0 ? m / seq_rows : 0, j = seq_rows > 0 ? m - sq * seq_rows : m;
    embed_tokens<WT>(tok_emb, cb_emb, dim, n_cb, cb_size, cfg->sem_lo, cfg->sem_hi, prompt + (size_t)sq * prompt_stride + state->step + j,
                     state->prompt_L, X + (size_t)m * dim, threadIdx.x, blockDim.x);
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

template <typename WT>
void LmKernels<WT>::qkv(const ModelDims& d, const float* x, const LayerW& w, const float* cos_t, const float* sin_t,
                        const SeqState* state, int pos_static, int rope_static, float* q_out, KVView kv, hipStream_t st) {
    constexpr int WAVES = 2;  // one row per wave, one RoPE pair per block
    const int n_rows = (d.H + 2 * d.Hk) * d.Dh;
    const int grid = (n_rows + WAVES - 1) / WAVES;
    dispatch_k(d.dim, [&](auto Kc) {
        constexpr int K = decltype(Kc)::value;
        if (w.cache_resident)
            hipLaunchKernelGGL((k_qkv<WT, K, WAVES, false>), dim3(grid), dim3(WAVES * 64), 0, st, x, w.attn_norm, d.eps,
                               (const WT*)w.wqkv, cos_t, sin_t, state, pos_static, rope_static, q_out, kv, d.H, d.Hk, d.Dh, w.s_qkv);
        else
            hipLaunchKernelGGL((k_qkv<WT, K, WAVES, true>), dim3(grid), dim3(WAVES * 64), 0, st, x, w.attn_norm, d.eps,
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
    constexpr int WAVES = 4;
    const int grid = (d.dim + WAVES - 1) / WAVES;
    FS_REQUIRE(fused_T <= 8 && d.H <= 32 && d.H * 8 * 2 <= WAVES * 64 && d.dim <= 4 * WAVES * 64, "fused attention supports at most 8 cached tokens and 16 heads");
    FS_REQUIRE(d.Dh == 64 || d.Dh == 32, "unsupported head_dim");
    dispatch_k(d.dim, [&](auto Kc) {
        constexpr int K = decltype(Kc)::value;
        auto go = [&](auto fused, auto dh) {
            if (w.cache_resident)
                hipLaunchKernelGGL((k_wo<WT, K, WAVES, decltype(fused)::value, decltype(dh)::value, false>), dim3(grid), dim3(WAVES * 64), 0,
                                   st, part, n_chunks_max, chunk, state, q, kv, fused_T, (const WT*)w.wo, x, d.H, d.Hk, d.dim, w.s_o, nc_launch);
            else
                hipLaunchKernelGGL((k_wo<WT, K, WAVES, decltype(fused)::value, decltype(dh)::value, true>), dim3(grid), dim3(WAVES * 64), 0,
                                   st, part, n_chunks_max, chunk, state, q, kv, fused_T, (const WT*)w.wo, x, d.H, d.Hk, d.dim, w.s_o, nc_launch);
        };
        using T = std::true_type; using F = std::false_type;
        using D64 = std::integral_constant<int, 64>; using D32 = std::integral_constant<int, 32>;
        if (fused_T > 0) { if (d.Dh == 64) go(T(), D64()); else go(T(), D32()); }
        else { if (d.Dh == 64) go(F(), D64()); else go(F(), D32()); }
    });
    FS_LAUNCH_CHECK();
}

template <typename WT>
void LmKernels<WT>::ffn_up(const ModelDims& d, const float* x, const LayerW& w, float* act, hipStream_t st) {
    constexpr int WAVES = 4;
    const int grid = (d.inter + WAVES - 1) / WAVES;
    dispatch_k(d.dim, [&](auto Kc) {
        constexpr int K = decltype(Kc)::value;
        if (w.cache_resident)
            hipLaunchKernelGGL((k_ffn_up<WT, K, WAVES, false>), dim3(grid), dim3(WAVES * 64), 0, st, x, w.ffn_norm, d.eps,
                               (const WT*)w.w13, act, d.inter, w.s_13);
        else
            hipLaunchKernelGGL((k_ffn_up<WT, K, WAVES, true>), dim3(grid), dim3(WAVES * 64), 0, st, x, w.ffn_norm, d.eps,
                               (const WT*)w.w13, act, d.inter, w.s_13);
    });
    FS_LAUNCH_CHECK();
}

template <typename WT>
void LmKernels<WT>::ffn_down(const ModelDims& d, const float* act, const LayerW& w, float* x, hipStream_t st) {
    constexpr int KS = 4;
    dispatch_k(d.inter, [&](auto Kc) {
        constexpr int K = decltype(Kc)::value;
        if (w.cache_resident)
            hipLaunchKernelGGL((k_ffn_down<WT, K, KS, false>), dim3(d.dim), dim3(KS * 64), 0, st, act, (const WT*)w.w2, x, d.dim, w.s_2);
        else
            hipLaunchKernelGGL((k_ffn_down<WT, K, KS, true>), dim3(d.dim), dim3(KS * 64), 0, st, act, (const WT*)w.w2, x, d.dim, w.s_2);
    });
    FS_LAUNCH_CHECK();
}

template <typename WT>
void LmKernels<WT>::head(const ModelDims& d, const float* x, const float* norm_w, const void* W, const float* wscale, int n_rows,
                         float* logits, hipStream_t st) {
    constexpr int WAVES = 4;
    const int grid = (n_rows + WAVES - 1) / WAVES;
    dispatch_k(d.dim, [&](auto Kc) {
        constexpr int K = decltype(Kc)::value;
        hipLaunchKernelGGL((k_head<WT, K, WAVES>), dim3(grid), dim3(WAVES * 64), 0, st, x, norm_w, d.eps, (const WT*)W,
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

// ---- MFMA row-path launchers (bf16 and fp8 weights; f32 handles take the sequential decode-kernel path)
template <typename WT>
bool LmKernels<WT>::has_mfma_prefill() { return std::is_same<WT, bf16_t>::value || std::is_same<WT, fp8_t>::value; }

template <typename WT>
void LmKernels<WT>::prefill_embed(const ModelDims& d, const void* tok_emb, const void* cb_emb, int n_cb, int cb_size,
                                  const SampleCfg* cfg, const uint32_t* prompt, const SeqState* state, int M, float* X,
                                  hipStream_t st, int seq_rows, size_t prompt_stride) {
    hipLaunchKernelGGL((k_embed_rows<KVT<WT>>), dim3(M), dim3(256), 0, st, (const KVT<WT>*)tok_emb, (const KVT<WT>*)cb_emb, d.dim, n_cb, cb_size,
                       cfg, prompt, state, X, seq_rows, prompt_stride);
    FS_LAUNCH_CHECK();
}

// Y[M, N] (+)= f(X[M, K]) . W[N, K]^T over `ksplit` K ranges (slabs Y + s * slab_stride for EPI_STORE); rt = 16-row tiles
// per wave (2 halves the L2 re-reads of the activations for the wide W13 GEMM)
template <int EPI>
static void launch_gemm3(int N, int ksplit, int rt, hipStream_t st, const bf16_t* Xf, int M, int K, const void* W, const float* wscale,
                         float* Y, int ldy, size_t slab_stride, bf16_t* Of, int ldo, const float* cos_t, const float* sin_t,
                         const SeqState* state, KVView kv, int H, int Hk, int Dh, RowMap rm, NormAux na = NormAux{}) {
    FS_REQUIRE(K % (ksplit * 128) == 0, "GEMM depth must be a multiple of 128 per K range");
    if (gemm_big_ok(M, N, K, ksplit)) {
        const int tiles = (N + GB_ROWS - 1) / GB_ROWS, panels_b = (M + PF_M - 1) / PF_M;
        const int gzb = std::max(1, std::min(panels_b, 512 / std::max(1, tiles * ksplit)));
        const dim3 gridb(tiles, ksplit, gzb);
        if (wscale)
            hipLaunchKernelGGL((k_gemm_big<EPI, true>), gridb, dim3(256), 0, st, Xf, M, K, W, wscale, N, Y, ldy, slab_stride, Of, ldo, cos_t, sin_t,
                               state, kv, H, Hk, Dh, rm, na);
        else
            hipLaunchKernelGGL((k_gemm_big<EPI, false>), gridb, dim3(256), 0, st, Xf, M, K, W, wscale, N, Y, ldy, slab_stride, Of, ldo, cos_t, sin_t,
                               state, kv, H, Hk, Dh, rm, na);
        return;
    }
    const int nks = K / ksplit / 128;
    // enough blocks to fill 256 CUs a few times over: spread the row panels over blockIdx.z until ~1024 blocks
    const int nb = (N + 16 * rt - 1) / (16 * rt) * ksplit, panels = (M + PF_M - 1) / PF_M;
    const int gz = std::max(1, std::min(panels, 1024 / std::max(1, nb)));
    const dim3 grid((N + 16 * rt - 1) / (16 * rt), ksplit, gz);
#define FS_GEMM_CASE(nk, r)                                                                                                          \
    do {                                                                                                                             \
        if (wscale && M <= 16)                                                                                                       \
            hipLaunchKernelGGL((k_gemm3<EPI, nk, r, true, true>), grid, dim3(256), 0, st, Xf, M, K, W, wscale, N, Y, ldy, slab_stride, Of, \
                               ldo, cos_t, sin_t, state, kv, H, Hk, Dh, rm, na);                                                 \
        else if (wscale)                                                                                                             \
            hipLaunchKernelGGL((k_gemm3<EPI, nk, r, true>), grid, dim3(256), 0, st, Xf, M, K, W, wscale, N, Y, ldy, slab_stride, Of, ldo,  \
                               cos_t, sin_t, state, kv, H, Hk, Dh, rm, na);                                                      \
        else if (M <= 16)                                                                                                            \
            hipLaunchKernelGGL((k_gemm3<EPI, nk, r, false, true>), grid, dim3(256), 0, st, Xf, M, K, W, wscale, N, Y, ldy, slab_stride, Of, \
                               ldo, cos_t, sin_t, state, kv, H, Hk, Dh, rm, na);                                                 \
        else                                                                                                                         \
            hipLaunchKernelGGL((k_gemm3<EPI, nk, r, false>), grid, dim3(256), 0, st, Xf, M, K, W, wscale, N, Y, ldy, slab_stride, Of, ldo, \
                               cos_t, sin_t, state, kv, H, Hk, Dh, rm, na);                                                      \
    } while (0)
    if (rt == 4) {
        switch (nks) {
            case 8: FS_GEMM_CASE(8, 4); break;
            case 2: FS_GEMM_CASE(2, 4); break;
            case 1: FS_GEMM_CASE(1, 4); break;
            default: throw Error("unsupported GEMM depth per K range " + std::to_string(K / ksplit) + " (supported: 1024, 256, 128)");
        }
    } else if (rt == 2) {
        switch (nks) {
            case 8: FS_GEMM_CASE(8, 2); break;
            case 2: FS_GEMM_CASE(2, 2); break;
            case 1: FS_GEMM_CASE(1, 2); break;
            default: throw Error("unsupported GEMM depth per K range " + std::to_string(K / ksplit) + " (supported: 1024, 256, 128)");
        }
    } else {
        switch (nks) {
            case 8: FS_GEMM_CASE(8, 1); break;
            case 2: FS_GEMM_CASE(2, 1); break;
            case 1: FS_GEMM_CASE(1, 1); break;
            default: throw Error("unsupported GEMM depth per K range " + std::to_string(K / ksplit) + " (supported: 1024, 256, 128)");
        }
    }
#undef FS_GEMM_CASE
}

// layer-closing down projection of a decode step (k_gemm_down): M <= 32 rows, depth = NKS * 128 * ksplit
static bool gemm_down_ok(int M, int N, int K) { return M <= PF_M && N % 128 == 0 && (K == 4096 || K == 1024 || K == 256); }
size_t rows_xchg_bytes(int dim) { return (size_t)(dim / 16) * 4 * PF_M * 8 * 16; }
static void launch_gemm_down(hipStream_t st, const bf16_t* Xf, int M, int K, const void* W, const float* wscale, int N, float* Y, int ldy, NormAux na,
                             void* xchg, uint32_t* epoch, uint32_t node_id) {
    FS_REQUIRE(xchg && epoch, "folded decode step without an exchange buffer");
    const int nks = K == 4096 ? 8 : (K == 1024 ? 2 : 1), ksplit = K / (nks * 128);   // 4, 4 (mid-size tests), 2 (tiny tests)
    static const int nap = [] { const char* e = std::getenv("FISHRT_DOWN_NAP"); return e ? std::atoi(e) : 8; }();  // 64-clock units before the first sweep (0 / 8 / 16 / 24 / 40: 1820 / 1813 / 1820 / 1853 / 1890 us per B = 32 step)
    const dim3 grid(N / 16, ksplit);
#define FS_DOWN_CASE(nk)                                                                                                              \
    do {                                                                                                                              \
        if (wscale) hipLaunchKernelGGL((k_gemm_down<nk, true>), grid, dim3(256), 0, st, Xf, M, K, W, wscale, N, Y, ldy, na, (u32x4*)xchg, epoch, node_id, nap);  \
        else hipLaunchKernelGGL((k_gemm_down<nk, false>), grid, dim3(256), 0, st, Xf, M, K, W, wscale, N, Y, ldy, na, (u32x4*)xchg, epoch, node_id, nap);        \
    } while (0)
    switch (nks) {
        case 8: FS_DOWN_CASE(8); break;
        case 2: FS_DOWN_CASE(2); break;
        default: FS_DOWN_CASE(1); break;
    }
#undef FS_DOWN_CASE
}
// FISHRT_ROWS_NO_FOLD=1: A/B hook -- decode steps keep the split-K slabs + k_prep nodes
static bool rows_fold_enabled() {
    static const bool v = [] { const char* e = std::getenv("FISHRT_ROWS_NO_FOLD"); return !(e && std::atoi(e) != 0); }();
    return v;
}
// k_gemm_down's owner waves spin on units published by the other K-quarter blocks of the SAME launch: every block of the grid must be
// resident at once.  The grid is dispatched y = 0 first; on a device (or partition: CPX, a masked-off part) where
// occupancy x CUs < N / 16 x ksplit the owners of resident tiles would wait for blocks that cannot be scheduled.  Checked once per
// (device, instantiation) with the runtime's occupancy query; such devices keep the slab + k_prep step.
template <int NKS, bool FP8>
static bool gemm_down_resident_inst(int blocks) {
    static int cached_dev = -1, cached_cap = 0;
    int dev = 0;
    FS_HIP(hipGetDevice(&dev));
    if (dev != cached_dev) {
        int per_cu = 0;
        hipDeviceProp_t prop;
        FS_HIP(hipGetDeviceProperties(&prop, dev));
        FS_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(k_gemm_down<NKS, FP8>), 256, 0));
        cached_cap = per_cu * prop.multiProcessorCount;
        cached_dev = dev;
    }
    if (const char* e = std::getenv("FISHRT_DOWN_FAKE_CAPACITY")) return std::atoi(e) >= blocks;  // (test hook: pretend a smaller device)
    return cached_cap >= blocks;
}
static bool gemm_down_resident(int N, int K, bool fp8) {
    const int nks = K == 4096 ? 8 : (K == 1024 ? 2 : 1), ksplit = K / (nks * 128), blocks = (N / 16) * ksplit;
    switch (nks) {
        case 8: return fp8 ? gemm_down_resident_inst<8, true>(blocks) : gemm_down_resident_inst<8, false>(blocks);
        case 2: return fp8 ? gemm_down_resident_inst<2, true>(blocks) : gemm_down_resident_inst<2, false>(blocks);
        default: return fp8 ? gemm_down_resident_inst<1, true>(blocks) : gemm_down_resident_inst<1, false>(blocks);
    }
}
template <typename WT>
bool LmKernels<WT>::rows_fold_ok(const ModelDims& d, int M, const RowsCtx& c) {
    if constexpr (std::is_same<WT, float>::value) return false;
    else
        return rows_fold_enabled() && c.A2 != nullptr && c.ss != nullptr && c.xchg != nullptr && c.epoch != nullptr && gemm_down_ok(M, d.dim, d.inter) &&
               !gemm_big_ok(M, d.dim, d.dim, 1) && c.stage_mask == 0xFFu && gemm_down_resident(d.dim, d.inter, std::is_same<WT, fp8_t>::value);
}

template <typename WT>
void LmKernels<WT>::rows_layer(const ModelDims& d, int M, const RowsCtx& c, const LayerW& w, KVView kv, bool first, hipStream_t st, const float* next_norm) {
    if constexpr (std::is_same<WT, float>::value) {
        throw Error("the MFMA row path needs bf16 or fp8 weights");
    } else {
        FS_REQUIRE(M >= 1 && M <= c.Mcap, "more activation rows than the row buffers hold");
        FS_REQUIRE(d.dim % 128 == 0 && d.inter % 128 == 0, "row path needs dim % 128 == 0 and intermediate_size % 128 == 0");
        const int qkv_rows = (d.H + 2 * d.Hk) * d.Dh;
        // 16-row-tiles per wave: 1 everywhere, 2 for the wide W13 (halves the L2 re-reads of the activation fragments).  64-row
        // blocks (rt = 4) were measured for prefill-sized passes and are SLOWER (W13 at 384 rows: 33 -> 41 us): the lost
        // occupancy costs more than the saved fragment traffic.
        static const int rt13_env = [] { const char* e = std::getenv("FISHRT_RT13"); return e ? std::atoi(e) : 0; }();  // experiment hook (1, 2 or 4)
        const int rt_qkv = 1, rt_o = 1, rt_13 = (rt13_env == 1 || rt13_env == 2 || rt13_env == 4) ? rt13_env : 2, rt_2 = 1;
        const int nblk_o = gemm_big_ok(M, d.dim, d.dim, 1) ? d.dim / GB_ROWS : d.dim / (16 * rt_o);  // blocks of the Wo GEMM (sum-of-squares partials)
        const RowMap rm{c.pos_step, c.pt_stride, c.seq_rows};
        const RowMap none{0, 0, 0};
        KVView nokv = {};
        const size_t slab = (size_t)c.Mcap * d.dim;
        const int DOWN_SPLIT = c.down_split;
        // decode steps (c.fold): the previous layer's un-split down projection (k_gemm_down) closed the residual stream and left
        // split(x * attention_norm) + sum-of-squares partials in c.A / c.ss: no k_prep node, Wqkv divides by the row's rms instead
        const bool fold = c.fold && next_norm != nullptr;
        if (fold) FS_REQUIRE(rows_fold_ok(d, M, c), "folded decode step on a shape the un-split down projection does not take");
        const int nblk_d = d.dim / 16;
        // (1) x += previous layer's down-proj slabs ; RMSNorm(attention_norm) -> hi/lo
        // c.qkv0_tbl (fold, small_attn, first layer of a codebook pass >= 1): q / k / v of the new token are a row of the qkv table -- no k_prep, no Wqkv
        // GEMM; the attention node reads the table itself (k_attn_small_rows_tbl)
        const bool tbl0 = fold && first && c.qkv0_tbl != nullptr && AttnKernels<WT>::rows_qkv0_ok(d, c);
        if (tbl0) {}
        else if (fold && (!first || c.first_prepped)) {}   // (first_prepped: the sampler that wrote the input row left its normalised fragments in c.A)
        else if (c.stage_mask & 1u) hipLaunchKernelGGL(k_prep, dim3(M), dim3(256), 0, st, c.X, d.dim, c.P, first ? 0 : DOWN_SPLIT, slab, w.attn_norm, d.eps, c.A);
        // (2) Wqkv + rope + KV scatter
        // c.attn_t1 (fold, small_attn; every row at position 0 of an empty cache): the Wqkv epilogue leaves the attention output itself
        // (GemmEpi::o1) in c.C -- free until this layer's W13 -- and the attention node is not launched
        const bool t1 = fold && c.attn_t1 && c.small_attn && !gemm_big_ok(M, qkv_rows, d.dim, 1);
        bf16_t* const o1 = t1 ? c.C : nullptr;
        // (Measured and rejected, round 5: Wqkv + the row attention of the later passes in ONE launch -- the GEMM blocks publish q / k / v as
        // tagged units, block m then attends for row m, bit-identical results: 10.1-10.4 us per node against 5.7 + 5.6 for the two nodes under
        // rocprofv3, 1856-1877 vs 1825-1833 us per step -- a consumer that waits for units from all 80 blocks on all 8 XCDs pays the slowest
        // block's finish + cross-XCD visibility, unlike k_gemm_down's four same-XCD partners; profiles/r05_rows_fold.txt)
        if (tbl0) {}
        else if (fold && !first)
            launch_gemm3<EPI_QKV_RMS>(qkv_rows, 1, rt_qkv, st, c.A, M, d.dim, w.wqkv, w.s_qkv, c.Q, d.dim, 0, o1, 0,
                                      c.cos_t, c.sin_t, c.state, kv, d.H, d.Hk, d.Dh, rm, NormAux{nullptr, c.ss, nullptr, nblk_d, d.dim, d.eps});
        else if ((c.stage_mask & 2u) && c.seq_rows > 0 && c.seq_states)
            launch_gemm3<EPI_QKV_SEQ>(qkv_rows, 1, rt_qkv, st, c.A, M, d.dim, w.wqkv, w.s_qkv, c.Q, d.dim, 0, o1, 0,
                                      c.cos_t, c.sin_t, c.seq_states, kv, d.H, d.Hk, d.Dh, rm);
        else if (c.stage_mask & 2u) launch_gemm3<EPI_QKV>(qkv_rows, 1, rt_qkv, st, c.A, M, d.dim, w.wqkv, w.s_qkv, c.Q, d.dim, 0, o1, 0,
                              c.cos_t, c.sin_t, c.state, kv, d.H, d.Hk, d.Dh, rm);
        // (3) attention over each row's KV prefix (+ chunk combine) -> hi/lo in c.A
        if (!t1) AttnKernels<WT>::rows(d, M, c, kv, tbl0, st);
        // (4) Wo + residual (each output element owned by one lane: deterministic)
        const bool fuse_norm = c.A2 != nullptr && c.ss != nullptr && nblk_o % 8 == 0 && d.dim % (16 * rt_o) == 0;
        NormAux na{w.ffn_norm, c.ss, c.A2, nblk_o, d.dim, d.eps};
        if (!(c.stage_mask & 16u)) {}
        else if (fuse_norm)
            launch_gemm3<EPI_RESIDUAL_NORM>(d.dim, 1, rt_o, st, t1 ? c.C : c.A, M, d.dim, w.wo, w.s_o, c.X, d.dim, 0, nullptr, 0, nullptr, nullptr,
                                            nullptr, nokv, 0, 0, 0, none, na);
        else launch_gemm3<EPI_RESIDUAL>(d.dim, 1, rt_o, st, c.A, M, d.dim, w.wo, w.s_o, c.X, d.dim, 0, nullptr, 0,
                                   nullptr, nullptr, nullptr, nokv, 0, 0, 0, none);
        // (5) RMSNorm(ffn_norm) -> hi/lo ; W1||W3 + SwiGLU -> act hi/lo ; W2 split-K slabs (summed by the next k_prep)
        if (fuse_norm) {
            if (c.stage_mask & 64u) launch_gemm3<EPI_SWIGLU_RMS>(2 * d.inter, 1, rt_13, st, c.A2, M, d.dim, w.w13, w.s_13, nullptr, 0, 0, c.C, d.inter,
                                     nullptr, nullptr, nullptr, nokv, 0, 0, 0, none, na);
        } else {
            if (c.stage_mask & 32u) hipLaunchKernelGGL(k_prep, dim3(M), dim3(256), 0, st, c.X, d.dim, (const float*)nullptr, 0, slab, w.ffn_norm, d.eps, c.A);
            if (c.stage_mask & 64u) launch_gemm3<EPI_SWIGLU>(2 * d.inter, 1, rt_13, st, c.A, M, d.dim, w.w13, w.s_13, nullptr, 0, 0, c.C, d.inter,
                                     nullptr, nullptr, nullptr, nokv, 0, 0, 0, none);
        }
        if (fold)  // x += W2 . act ; split(x * next_norm) -> c.A ; sum-of-squares partials -> c.ss  (the attention output in c.A and Wo's partials are consumed)
            launch_gemm_down(st, c.C, M, d.inter, w.w2, w.s_2, d.dim, c.X, d.dim, NormAux{next_norm, c.ss, c.A, nblk_d, d.dim, d.eps}, c.xchg, c.epoch, c.node_id);
        else if (c.stage_mask & 128u) launch_gemm3<EPI_STORE>(d.dim, DOWN_SPLIT, rt_2, st, c.C, M, d.inter, w.w2, w.s_2, c.P, d.dim, slab, nullptr, 0, nullptr, nullptr,
                                nullptr, nokv, 0, 0, 0, none);
        FS_LAUNCH_CHECK();
    }
}

template <typename WT>
void LmKernels<WT>::rows_finish(const ModelDims& d, int M, const RowsCtx& c, const float* norm_w, hipStream_t st) {
    hipLaunchKernelGGL(k_prep, dim3(M), dim3(256), 0, st, c.X, d.dim, c.P, c.down_split, (size_t)c.Mcap * d.dim, norm_w, d.eps,
                       norm_w ? c.A : (bf16_t*)nullptr);
    FS_LAUNCH_CHECK();
}

// head GEMM of the MFMA row path: logits[m][0..n_rows) = W[n_rows, dim] . (hi + lo)[m]  (input = rows_finish(norm_w) output)
template <typename WT>
void LmKernels<WT>::rows_head(const ModelDims& d, int M, const RowsCtx& c, const void* W, const float* wscale, int n_rows, float* logits, int ld,
                              hipStream_t st, bool rms) {
    if constexpr (std::is_same<WT, float>::value) {
        throw Error("the MFMA row path needs bf16 or fp8 weights");
    } else {
        FS_REQUIRE(ld >= n_rows, "logits row stride must cover n_rows");
        KVView nokv = {};
        // EPI_STORE with one K range writes slab 0 == the logits matrix itself (row stride ld)
        if (rms)  // folded decode step: c.A holds split(x * norm_w), c.ss the sum-of-squares partials of the last down projection
            launch_gemm3<EPI_STORE_RMS>(n_rows, 1, 1, st, c.A, M, d.dim, W, wscale, logits, ld, 0, nullptr, 0, nullptr, nullptr, nullptr, nokv, 0, 0,
                                        0, RowMap{0, 0}, NormAux{nullptr, c.ss, nullptr, d.dim / 16, d.dim, d.eps});
        else
        launch_gemm3<EPI_STORE>(n_rows, 1, 1, st, c.A, M, d.dim, W, wscale, logits, ld, 0, nullptr, 0, nullptr, nullptr, nullptr, nokv, 0, 0,
                                0, RowMap{0, 0});
        FS_LAUNCH_CHECK();
    }
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

}  // namespace fs
