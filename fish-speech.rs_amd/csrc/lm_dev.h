// Device helpers shared by the transformer kernels (lm_kernels.hip), the row-path GEMMs (lm_gemm.hip), the attention kernels (lm_attn.hip)
// and the on-device samplers (lm_sample.hip): weight-type traits, the streamed weight load, the paged KV address, cross-lane reductions,
// the token embedding, row positions, and the fragment-major GEMM-input layout with the one-row RMSNorm + hi/lo split.
// Device code only -- except frag_off, which the host side of fs_selftest_attn uses to de-fragment; the host-side launch interface is lm_kernels.h.
#pragma once
#include <hip/hip_runtime.h>

#include "fs_common.h"
#include "lm_kernels.h"

namespace fs {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));   // MFMA operands / accumulators
typedef float f32x4v __attribute__((ext_vector_type(4)));

// Everything above this point is ISSUED before anything below it: keeps the machine scheduler from sinking the weight-stream
// loads under the wait for the small L2-resident vectors (it otherwise serialises x-load -> RMSNorm -> weight request, which
// costs a full L2 round trip + the norm per kernel node before the first HBM byte is even asked for).
#define FS_ISSUE_FENCE() __builtin_amdgcn_sched_barrier(0)

__device__ __forceinline__ float bf16_bits_to_f32(uint32_t hi16) { return __uint_as_float(hi16 << 16); }

template <typename V>
__device__ __forceinline__ V ld_stream(const V* p) {  // streamed-once weights: non-temporal (guide: nt-weights)
    return __builtin_nontemporal_load(p);
}

// element (token t, kv head g, dim 0) of a paged KV pool (layout: lm_kernels.h)
template <typename WT>
__device__ __forceinline__ WT* kv_addr(void* pool, const int* __restrict__ page_table, int t, int g, int Hk, int Dh) {
    const int page = page_table[t / KV_PAGE];
    return reinterpret_cast<WT*>(pool) + ((size_t)(page * Hk + g) * KV_PAGE + (t % KV_PAGE)) * Dh;
}

// position of activation row m: pos_step 1 = consecutive tokens of one sequence (prefill), 0 = every row at state->pos (lock-step static
// batch), -1 = row m is its own sequence with its own state (session slots, fs_lm_session_*)
__device__ __forceinline__ int row_pos(const SeqState* __restrict__ state, int m, int pos_step) {
    return pos_step < 0 ? state[m].pos : state->pos + m * pos_step;
}

template <typename WT>
struct WTr;
template <>
struct WTr<bf16_t> {
    static constexpr int EPL = 8;  // elements per 16-byte lane load
    using vec = u32x4;
    __device__ static __forceinline__ void unpack(const u32x4& v, float* f) {
        f[0] = __uint_as_float(v.x << 16); f[1] = __uint_as_float(v.x & 0xFFFF0000u);
        f[2] = __uint_as_float(v.y << 16); f[3] = __uint_as_float(v.y & 0xFFFF0000u);
        f[4] = __uint_as_float(v.z << 16); f[5] = __uint_as_float(v.z & 0xFFFF0000u);
        f[6] = __uint_as_float(v.w << 16); f[7] = __uint_as_float(v.w & 0xFFFF0000u);
    }
    __device__ static __forceinline__ float to_f32(bf16_t h) { return __uint_as_float((uint32_t)h << 16); }
    __device__ static __forceinline__ bf16_t from_f32(float f) {  // RNE
        uint32_t u = __float_as_uint(f);
        u += 0x7FFFu + ((u >> 16) & 1u);
        return (bf16_t)(u >> 16);
    }
};
template <>
struct WTr<float> {
    static constexpr int EPL = 4;
    using vec = f32x4;
    __device__ static __forceinline__ void unpack(const f32x4& v, float* f) { f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w; }
    __device__ static __forceinline__ float to_f32(float h) { return h; }
    __device__ static __forceinline__ float from_f32(float f) { return f; }
};

typedef float f32x2 __attribute__((ext_vector_type(2)));
template <>
struct WTr<fp8_t> {
    static constexpr int EPL = 16;  // OCP e4m3fn weights: 16 per 16-byte lane load
    using vec = u32x4;
    __device__ static __forceinline__ void unpack(const u32x4& v, float* f) {
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(w[i], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8(w[i], true);
            f[4 * i] = lo.x; f[4 * i + 1] = lo.y; f[4 * i + 2] = hi.x; f[4 * i + 3] = hi.y;
        }
    }
    __device__ static __forceinline__ float to_f32(fp8_t h) { return e4m3_to_f32(h.v); }
    __device__ static __forceinline__ fp8_t from_f32(float f) { return fp8_t{f32_to_e4m3(f)}; }
};

// ---- cross-lane reductions: DPP inside a 16-lane row (no LDS crossbar), v_readlane across the four rows.
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
constexpr int DPP_XOR1 = 0xB1;         // quad_perm [1,0,3,2]
constexpr int DPP_XOR2 = 0x4E;         // quad_perm [2,3,0,1]
constexpr int DPP_HALF_MIRROR = 0x141; // lane i <-> 7-i inside each 8
constexpr int DPP_MIRROR = 0x140;      // lane i <-> 15-i inside each 16
__device__ __forceinline__ float readlane(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

// sum over the whole wave; the result is wave-uniform (scalar registers)
__device__ __forceinline__ float wave_sum(float v) {
    v += dpp_mov<DPP_XOR1>(v);
    v += dpp_mov<DPP_XOR2>(v);
    v += dpp_mov<DPP_HALF_MIRROR>(v);
    v += dpp_mov<DPP_MIRROR>(v);
    return (readlane(v, 15) + readlane(v, 31)) + (readlane(v, 47) + readlane(v, 63));
}
// sum / max over aligned groups of N consecutive lanes (N in {1,2,4,8,16}); every lane of the group gets the result
template <int N>
__device__ __forceinline__ float group_sum(float v) {
    if (N >= 2) v += dpp_mov<DPP_XOR1>(v);
    if (N >= 4) v += dpp_mov<DPP_XOR2>(v);
    if (N >= 8) v += dpp_mov<DPP_HALF_MIRROR>(v);
    if (N >= 16) v += dpp_mov<DPP_MIRROR>(v);
    return v;
}

// dual_ar.rs:532-567: x = tok_emb[t0] + sum_c (sem_lo <= t0 <= sem_hi) * cb_emb[c*cb_size + t_{c+1}], summed in order.
template <typename WT>
__device__ __forceinline__ void embed_tokens(const WT* __restrict__ tok_emb, const WT* __restrict__ cb_emb, int dim, int n_cb,
                                             int cb_size, uint32_t sem_lo, uint32_t sem_hi, const uint32_t* toks, int stride,
                                             float* __restrict__ x, int tid, int nthreads) {
    const uint32_t sem = toks[0];
    const float m = (sem >= sem_lo && sem <= sem_hi) ? 1.f : 0.f;
    for (int d = tid; d < dim; d += nthreads) {
        float acc = 0.f + WTr<WT>::to_f32(tok_emb[(size_t)sem * dim + d]);
        for (int c = 0; c < n_cb; ++c) {
            const uint32_t code = toks[(size_t)(c + 1) * stride];
            acc += WTr<WT>::to_f32(cb_emb[((size_t)c * cb_size + code) * dim + d]) * m;
        }
        x[d] = acc;
    }
}

__device__ __forceinline__ void split_bf16(float a, bf16_t& hi, bf16_t& lo) {
    hi = WTr<bf16_t>::from_f32(a);
    lo = WTr<bf16_t>::from_f32(a - WTr<bf16_t>::to_f32(hi));
}

// GEMM-input layout ("fragment-major"): the bf16 hi/lo activations are stored exactly as the MFMA B operand wants them, so
// that every wave-wide operand load of k_gemm3 is ONE contiguous KiB (8 full cache lines) instead of 16 half lines strided
// by a row (measured: the strided form cost 3.3 us of a 7 us GEMM node).  Element (row m, depth k, part hi=0 / lo=1) of a
// [rows][K] activation matrix lives at (in bf16 elements)
//     (((((m / 32) * (K / 32) + k / 32) * 2 + part) * 2 + (m / 16) % 2) * 64 + ((k / 8) % 4) * 16 + m % 16) * 8 + k % 8
// i.e. [32-row panel][32-deep k-step][part][16-row tile][lane = kq*16 + row][8 consecutive k].
__host__ __device__ __forceinline__ size_t frag_off(int m, int k, int part, int K) {
    const int p = m >> 5, mt = (m >> 4) & 1, lr = m & 15, kk = k >> 5, lq = (k >> 3) & 3, e = k & 7;
    return (((((size_t)p * (K >> 5) + kk) * 2 + part) * 2 + mt) * 64 + (lq * 16 + lr)) * 8 + e;
}

// elements (m, e .. e + 3), e % 4 == 0, of a fragment-major [rows][K] matrix: hi/lo split of a[0..3], one 8-byte store per part
__device__ __forceinline__ void store_frag4(bf16_t* A, int m, int e, int K, const float (&a)[4]) {
    bf16_t hi[4], lo[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) split_bf16(a[i], hi[i], lo[i]);
    uint2 ph, pl;
    ph.x = hi[0] | ((uint32_t)hi[1] << 16); ph.y = hi[2] | ((uint32_t)hi[3] << 16);
    pl.x = lo[0] | ((uint32_t)lo[1] << 16); pl.y = lo[2] | ((uint32_t)lo[3] << 16);
    *reinterpret_cast<uint2*>(A + frag_off(m, e, 0, K)) = ph;
    *reinterpret_cast<uint2*>(A + frag_off(m, e, 1, K)) = pl;
}

// k_prep's RMSNorm + hi/lo split of ONE row by the block that has just written it (the batched samplers: the row is the fast decoder's
// next input, so its first layer needs no k_prep node in a folded decode step).  Threads 0..255 take one float4 each (D <= 1024) and the sums
// meet in k_prep's order: the fragments are bit-identical to what the node would have produced.
struct PrepOut { const float* g; float eps; bf16_t* A; uint32_t* epoch; };   // g == nullptr: disabled; epoch != nullptr (slow-token sampler): the step epoch of k_gemm_down's tags is bumped here, once per step
__device__ __forceinline__ void block_prep_row(const float* __restrict__ xm, int D, const PrepOut& po, int m, float* red4) {
    __syncthreads();  // the row's stores by the other threads of this block
    const int e = threadIdx.x * 4;
    const bool act = threadIdx.x < 256 && e < D;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f), w = make_float4(1.f, 1.f, 1.f, 1.f);
    if (act) { v = *reinterpret_cast<const float4*>(xm + e); w = *reinterpret_cast<const float4*>(po.g + e); }
    float ss = 0.f;
    ss = fmaf(v.x, v.x, ss); ss = fmaf(v.y, v.y, ss); ss = fmaf(v.z, v.z, ss); ss = fmaf(v.w, v.w, ss);
    ss = wave_sum(ss);
    if (threadIdx.x < 256 && (threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = ss;
    __syncthreads();
    if (!act) return;
    const float d = sqrtf(((red4[0] + red4[1]) + (red4[2] + red4[3])) / (float)D + po.eps);
    const float a[4] = {(v.x / d) * w.x, (v.y / d) * w.y, (v.z / d) * w.z, (v.w / d) * w.w};
    store_frag4(po.A, m, e, D, a);
}

}  // namespace fs
