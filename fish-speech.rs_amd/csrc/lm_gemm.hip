// MFMA row path of the dual-AR transformer for gfx950 (MI355X): skinny GEMMs over activation rows -- the prefill passes and the
// static-batch / session decode steps.  Kernels: k_prep (slab sum + RMSNorm + hi/lo split), k_gemm3 (<= 32-row blocks, operands straight
// from global / L2), k_gemm_down (layer-closing down projection of a decode step), k_gemm_big (LDS-staged, from 128 rows) and the row
// embedding; RowKernels<WT>::rows_layer decides which of them a layer runs.  The attention nodes of the row path are in lm_attn.hip.
// Launch interface: RowKernels<WT> in lm_kernels.h; device helpers: lm_dev.h.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <set>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/fishrt.h"
#include "fs_common.h"
#include "lm_kernels.h"
#include "lm_dev.h"

namespace fs {

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
// A lane's weight panel: NKS k-steps of one weight row from element offset `woff` (its 8 k of every 32-wide step), all requested before
// the first is used; fp8 bytes are widened to bf16 once they are all in flight.
template <int NKS, bool FP8>
__device__ __forceinline__ void load_wpanel(const void* __restrict__ Wv, size_t woff, u32x4 (&wf)[NKS]) {
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
// the four K-quarter partials of (weight row, activation row), summed in a fixed order
template <int ROWS>
__device__ __forceinline__ float ksum4(const float (&red)[4][ROWS][33], int row, int ml) {
    return (red[0][row][ml] + red[1][row][ml]) + (red[2][row][ml] + red[3][row][ml]);
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
    for (int rt = 0; rt < RT; ++rt) load_wpanel<NKS, FP8>(Wv, (size_t)min(n0 + rt * 16 + (lane & 15), N - 1) * K + kbeg, wf[rt]);
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
            float a = ksum4(red, 2 * pr, ml), b = ksum4(red, 2 * pr + 1, ml);
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
    load_wpanel<NKS, FP8>(Wv, (size_t)(n0 + (lane & 15)) * K + kbeg, wf);
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
    float a = ksum4(red, 2 * pr, ml), b = ksum4(red, 2 * pr + 1, ml);
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
static bool gemm_big_ok(int M, int N, int K, int ksplit, int big_min_m = 0) {  // big_min_m > 0: this call's own threshold (fs_selftest_gemm)
    if (K % ksplit != 0 || K / ksplit != 1024) return false;
    const int m0 = big_min_m > 0 ? big_min_m : gemm_big_min_m();
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
    for (int t = 0; t < 2; ++t)
        load_wpanel<NKS, FP8>(Wv, (size_t)min(n0 + rg * 32 + t * 16 + (lane & 15), N - 1) * K + (size_t)ksw * 32 + (lane >> 4) * 8, wf[t]);
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

// ================================================================================================ launchers
#define FS_LAUNCH_CHECK() FS_HIP(hipGetLastError())

// run-time choices that select an instantiation: f(std::true_type / std::false_type), f(std::integral_constant<int, NKS>)
template <typename F>
static void with_bool(bool v, F&& f) {
    if (v) f(std::true_type()); else f(std::false_type());
}
template <typename F>
static void with_nks(int nks, F&& f) {  // k-steps of 32 per wave: depth per K range / 128
    switch (nks) {
        case 8: f(std::integral_constant<int, 8>()); break;
        case 2: f(std::integral_constant<int, 2>()); break;
        case 1: f(std::integral_constant<int, 1>()); break;
        default: throw Error("unsupported GEMM depth per K range " + std::to_string(nks * 128) + " (supported: 1024, 256, 128)");
    }
}

// ---- MFMA row-path launchers (bf16 and fp8 weights; f32 handles take the sequential decode-kernel path)
template <typename WT>
bool RowKernels<WT>::has_mfma_prefill() { return std::is_same<WT, bf16_t>::value || std::is_same<WT, fp8_t>::value; }

template <typename WT>
void RowKernels<WT>::prefill_embed(const ModelDims& d, const void* tok_emb, const void* cb_emb, int n_cb, int cb_size,
                                   const SampleCfg* cfg, const uint32_t* prompt, const SeqState* state, int M, float* X,
                                   hipStream_t st, int seq_rows, size_t prompt_stride) {
    hipLaunchKernelGGL((k_embed_rows<KVT<WT>>), dim3(M), dim3(256), 0, st, (const KVT<WT>*)tok_emb, (const KVT<WT>*)cb_emb, d.dim, n_cb, cb_size,
                       cfg, prompt, state, X, seq_rows, prompt_stride);
    FS_LAUNCH_CHECK();
}

// Host-side arguments of one row-path GEMM: Y[M, N] (+)= f(X[M, K]) . W[N, K]^T over `ksplit` K ranges (slabs Y + s * slab_stride for
// EPI_STORE).  A call site states the parts its epilogue uses; launch_gemm3 unpacks them into the kernels' parameter list.
struct GemmIn { const bf16_t* Xf; int M, K; const void* W; const float* wscale; int N; int ksplit = 1; int big_min_m = 0; };  // big_min_m: gemm_plan's
struct GemmOut { float* Y = nullptr; int ldy = 0; size_t slab_stride = 0; bf16_t* Of = nullptr; int ldo = 0; };
struct GemmQkv {   // EPI_QKV*: RoPE tables, position source, KV cache and head geometry, row -> sequence mapping
    const float *cos_t = nullptr, *sin_t = nullptr; const SeqState* state = nullptr;
    KVView kv = {}; int H = 0, Hk = 0, Dh = 0; RowMap rm = {0, 0, 0};
};
struct GemmArgs { GemmIn in; GemmOut out; GemmQkv qkv = {}; NormAux na = {}; };

// RT = 16-row tiles per wave (2 halves the L2 re-reads of the activations for the wide W13 GEMM)
template <int EPI, int RT = 1>
static void launch_gemm3(hipStream_t st, const GemmArgs& g) {
    const GemmIn& in = g.in; const GemmOut& out = g.out; const GemmQkv& q = g.qkv;
    const int M = in.M, N = in.N, K = in.K;
    const GemmPlan p = gemm_plan(EPI, RT, M, N, K, in.ksplit, in.wscale != nullptr, in.big_min_m);
    const dim3 grid(p.gx, p.gy, p.gz);
    if (p.kind == GemmPlan::BIG) {
        with_bool(p.fp8, [&](auto fp8) {
            hipLaunchKernelGGL((k_gemm_big<EPI, decltype(fp8)::value>), grid, dim3(256), 0, st, in.Xf, M, K, in.W, in.wscale, N, out.Y, out.ldy,
                               out.slab_stride, out.Of, out.ldo, q.cos_t, q.sin_t, q.state, q.kv, q.H, q.Hk, q.Dh, q.rm, g.na);
        });
        return;
    }
    with_nks(p.nks, [&](auto nks) {
        with_bool(p.fp8, [&](auto fp8) {
            with_bool(p.half, [&](auto half) {
                hipLaunchKernelGGL((k_gemm3<EPI, decltype(nks)::value, RT, decltype(fp8)::value, decltype(half)::value>), grid, dim3(256), 0, st,
                                   in.Xf, M, K, in.W, in.wscale, N, out.Y, out.ldy, out.slab_stride, out.Of, out.ldo, q.cos_t, q.sin_t, q.state,
                                   q.kv, q.H, q.Hk, q.Dh, q.rm, g.na);
            });
        });
    });
}

// layer-closing down projection of a decode step (k_gemm_down): M <= 32 rows, depth = nks * 128 * ksplit
struct DownShape { int nks, ksplit; };
static DownShape down_shape(int K) {  // {0, 0}: not a depth k_gemm_down takes
    switch (K) {
        case 4096: return {8, 4};
        case 1024: return {2, 4};  // (mid-size tests)
        case 256: return {1, 2};   // (tiny tests)
        default: return {0, 0};
    }
}
static bool gemm_down_ok(int M, int N, int K) { return M <= PF_M && N % 128 == 0 && down_shape(K).nks != 0; }
size_t rows_xchg_bytes(int dim) { return (size_t)(dim / 16) * 4 * PF_M * 8 * 16; }

// ---- the one place that decides which instantiation and grid a row-path GEMM runs (GemmPlan: lm_kernels.h)
static const char* const kEpiNames[] = {"STORE", "RESIDUAL", "SWIGLU", "QKV", "RESIDUAL_NORM", "SWIGLU_RMS", "QKV_RMS", "STORE_RMS", "QKV_SEQ"};
std::string GemmPlan::name() const {
    const std::string wt = fp8 ? "fp8" : "bf16";
    switch (kind) {
    case BIG: return std::string("big/") + kEpiNames[epi] + "/" + wt;
    case DOWN: return "down/nks" + std::to_string(nks) + "/ks" + std::to_string(ksplit) + "/" + wt;
    default: return std::string("gemm3/") + kEpiNames[epi] + "/nks" + std::to_string(nks) + "/rt" + std::to_string(rt) + "/" + wt + (half ? "/half" : "");
    }
}
GemmPlan gemm_plan(int epi, int rt, int M, int N, int K, int ksplit, bool fp8, int big_min_m) {
    GemmPlan p;
    p.epi = epi; p.fp8 = fp8;
    FS_REQUIRE(M >= 1 && N >= 1 && K >= 1, "GEMM needs M, N, K >= 1");
    if (epi == GEMM_EPI_DOWN) {
        FS_REQUIRE(gemm_down_ok(M, N, K), "down projection on a shape k_gemm_down does not take (M <= 32, N % 128 == 0, K in {4096, 1024, 256})");
        const DownShape s = down_shape(K);
        p.kind = GemmPlan::DOWN; p.nks = s.nks; p.ksplit = s.ksplit; p.gx = N / 16; p.gy = s.ksplit;
        return p;
    }
    FS_REQUIRE(epi >= EPI_STORE && epi <= EPI_QKV_SEQ && (rt == 1 || rt == 2), "unknown GEMM epilogue or tile count");
    FS_REQUIRE(ksplit >= 1 && K % (ksplit * 128) == 0, "GEMM depth must be a multiple of 128 per K range");
    p.ksplit = ksplit; p.gy = ksplit;
    const int panels = (M + PF_M - 1) / PF_M;
    if (gemm_big_ok(M, N, K, ksplit, big_min_m)) {
        const int tiles = (N + GB_ROWS - 1) / GB_ROWS;
        p.kind = GemmPlan::BIG; p.nks = 16; p.rt = GB_ROWS / 16;
        p.gx = tiles; p.gz = std::max(1, std::min(panels, 512 / std::max(1, tiles * ksplit)));
        return p;
    }
    // enough blocks to fill 256 CUs a few times over: spread the row panels over blockIdx.z until ~1024 blocks
    const int tiles = (N + 16 * rt - 1) / (16 * rt);
    p.kind = GemmPlan::GEMM3; p.rt = rt; p.half = M <= 16;
    p.nks = K / ksplit / 128;  // k-steps of 32 per wave: depth per K range / 128
    if (p.nks != 8 && p.nks != 2 && p.nks != 1)
        throw Error("unsupported GEMM depth per K range " + std::to_string(p.nks * 128) + " (supported: 1024, 256, 128)");
    p.gx = tiles; p.gz = std::max(1, std::min(panels, 1024 / std::max(1, tiles * ksplit)));
    return p;
}
// what rows_layer / rows_fold_ok need to know about a launch before they make it (the Wo GEMM's block count, the o1 and fold decisions):
// asked of the plan itself, with the arguments of that launch (one K range, RT 1)
static bool plan_is_big(int epi, int M, int N, int K) { return gemm_plan(epi, 1, M, N, K, 1, false).kind == GemmPlan::BIG; }

static void launch_gemm_down(hipStream_t st, const bf16_t* Xf, int M, int K, const void* W, const float* wscale, int N, float* Y, int ldy, NormAux na,
                             void* xchg, uint32_t* epoch, uint32_t node_id) {
    FS_REQUIRE(xchg && epoch, "folded decode step without an exchange buffer");
    const GemmPlan p = gemm_plan(GEMM_EPI_DOWN, 1, M, N, K, 0, wscale != nullptr);
    static const int nap = [] { const char* e = std::getenv("FISHRT_DOWN_NAP"); return e ? std::atoi(e) : 8; }();  // 64-clock units before the first sweep (0 / 8 / 16 / 24 / 40: 1820 / 1813 / 1820 / 1853 / 1890 us per B = 32 step)
    with_nks(p.nks, [&](auto nks) {
        with_bool(p.fp8, [&](auto fp8) {
            hipLaunchKernelGGL((k_gemm_down<decltype(nks)::value, decltype(fp8)::value>), dim3(p.gx, p.gy), dim3(256), 0, st, Xf, M, K, W, wscale,
                               N, Y, ldy, na, (u32x4*)xchg, epoch, node_id, nap);
        });
    });
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
    const DownShape s = down_shape(K);
    bool ok = false;
    with_nks(s.nks, [&](auto nks) {
        with_bool(fp8, [&](auto f8) { ok = gemm_down_resident_inst<decltype(nks)::value, decltype(f8)::value>((N / 16) * s.ksplit); });
    });
    return ok;
}
template <typename WT>
bool RowKernels<WT>::rows_fold_ok(const ModelDims& d, int M, const RowsCtx& c) {
    if constexpr (std::is_same<WT, float>::value) return false;
    else
        return rows_fold_enabled() && c.A2 != nullptr && c.ss != nullptr && c.xchg != nullptr && c.epoch != nullptr && gemm_down_ok(M, d.dim, d.inter) &&
               !plan_is_big(EPI_RESIDUAL_NORM, M, d.dim, d.dim) && c.stage_mask == 0xFFu && gemm_down_resident(d.dim, d.inter, std::is_same<WT, fp8_t>::value);
}

template <typename WT>
void RowKernels<WT>::rows_layer(const ModelDims& d, int M, const RowsCtx& c, const LayerW& w, KVView kv, bool first, hipStream_t st, const float* next_norm) {
    if constexpr (std::is_same<WT, float>::value) {
        throw Error("the MFMA row path needs bf16 or fp8 weights");
    } else {
        FS_REQUIRE(M >= 1 && M <= c.Mcap, "more activation rows than the row buffers hold");
        FS_REQUIRE(d.dim % 128 == 0 && d.inter % 128 == 0, "row path needs dim % 128 == 0 and intermediate_size % 128 == 0");
        const int qkv_rows = (d.H + 2 * d.Hk) * d.Dh;
        // 16-row tiles per wave (launch_gemm3's RT): 1 everywhere, 2 for the wide W13 (halves the L2 re-reads of the activation fragments).
        // 64-row blocks (RT = 4) were measured for prefill-sized passes and are SLOWER (W13 at 384 rows: 33 -> 41 us): the lost
        // occupancy costs more than the saved fragment traffic.
        const int nblk_o = plan_is_big(EPI_RESIDUAL_NORM, M, d.dim, d.dim) ? d.dim / GB_ROWS : d.dim / 16;  // blocks of the Wo GEMM (sum-of-squares partials)
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
        const bool t1 = fold && c.attn_t1 && c.small_attn && !plan_is_big(EPI_QKV_RMS, M, qkv_rows, d.dim);
        const GemmIn in_qkv{c.A, M, d.dim, w.wqkv, w.s_qkv, qkv_rows};
        const GemmOut out_qkv{c.Q, d.dim, 0, t1 ? c.C : nullptr, 0};
        const GemmQkv rope{c.cos_t, c.sin_t, c.state, kv, d.H, d.Hk, d.Dh, RowMap{c.pos_step, c.pt_stride, c.seq_rows}};
        // (Measured and rejected, round 5: Wqkv + the row attention of the later passes in ONE launch -- the GEMM blocks publish q / k / v as
        // tagged units, block m then attends for row m, bit-identical results: 10.1-10.4 us per node against 5.7 + 5.6 for the two nodes under
        // rocprofv3, 1856-1877 vs 1825-1833 us per step -- a consumer that waits for units from all 80 blocks on all 8 XCDs pays the slowest
        // block's finish + cross-XCD visibility, unlike k_gemm_down's four same-XCD partners; profiles/r05_rows_fold.txt)
        if (tbl0) {}
        else if (fold && !first) launch_gemm3<EPI_QKV_RMS>(st, {in_qkv, out_qkv, rope, NormAux{nullptr, c.ss, nullptr, nblk_d, d.dim, d.eps}});
        else if ((c.stage_mask & 2u) && c.seq_rows > 0 && c.seq_states) {
            GemmQkv seq = rope;
            seq.state = c.seq_states;
            launch_gemm3<EPI_QKV_SEQ>(st, {in_qkv, out_qkv, seq});
        } else if (c.stage_mask & 2u) launch_gemm3<EPI_QKV>(st, {in_qkv, out_qkv, rope});
        // (3) attention over each row's KV prefix (+ chunk combine) -> hi/lo in c.A
        if (!t1) AttnKernels<WT>::rows(d, M, c, kv, tbl0, st);
        // (4) Wo + residual (each output element owned by one lane: deterministic)
        const bool fuse_norm = c.A2 != nullptr && c.ss != nullptr && nblk_o % 8 == 0 && d.dim % 16 == 0;
        const NormAux na{w.ffn_norm, c.ss, c.A2, nblk_o, d.dim, d.eps};
        if (!(c.stage_mask & 16u)) {}
        else if (fuse_norm) launch_gemm3<EPI_RESIDUAL_NORM>(st, {{t1 ? c.C : c.A, M, d.dim, w.wo, w.s_o, d.dim}, {c.X, d.dim}, {}, na});
        else launch_gemm3<EPI_RESIDUAL>(st, {{c.A, M, d.dim, w.wo, w.s_o, d.dim}, {c.X, d.dim}});
        // (5) RMSNorm(ffn_norm) -> hi/lo ; W1||W3 + SwiGLU -> act hi/lo ; W2 split-K slabs (summed by the next k_prep)
        const GemmOut out_13{nullptr, 0, 0, c.C, d.inter};
        if (fuse_norm) {
            if (c.stage_mask & 64u) launch_gemm3<EPI_SWIGLU_RMS, 2>(st, {{c.A2, M, d.dim, w.w13, w.s_13, 2 * d.inter}, out_13, {}, na});
        } else {
            if (c.stage_mask & 32u) hipLaunchKernelGGL(k_prep, dim3(M), dim3(256), 0, st, c.X, d.dim, (const float*)nullptr, 0, slab, w.ffn_norm, d.eps, c.A);
            if (c.stage_mask & 64u) launch_gemm3<EPI_SWIGLU, 2>(st, {{c.A, M, d.dim, w.w13, w.s_13, 2 * d.inter}, out_13});
        }
        if (fold)  // x += W2 . act ; split(x * next_norm) -> c.A ; sum-of-squares partials -> c.ss  (the attention output in c.A and Wo's partials are consumed)
            launch_gemm_down(st, c.C, M, d.inter, w.w2, w.s_2, d.dim, c.X, d.dim, NormAux{next_norm, c.ss, c.A, nblk_d, d.dim, d.eps}, c.xchg, c.epoch, c.node_id);
        else if (c.stage_mask & 128u) launch_gemm3<EPI_STORE>(st, {{c.C, M, d.inter, w.w2, w.s_2, d.dim, DOWN_SPLIT}, {c.P, d.dim, slab}});
        FS_LAUNCH_CHECK();
    }
}

template <typename WT>
void RowKernels<WT>::rows_finish(const ModelDims& d, int M, const RowsCtx& c, const float* norm_w, hipStream_t st) {
    hipLaunchKernelGGL(k_prep, dim3(M), dim3(256), 0, st, c.X, d.dim, c.P, c.down_split, (size_t)c.Mcap * d.dim, norm_w, d.eps,
                       norm_w ? c.A : (bf16_t*)nullptr);
    FS_LAUNCH_CHECK();
}

// head GEMM of the MFMA row path: logits[m][0..n_rows) = W[n_rows, dim] . (hi + lo)[m]  (input = rows_finish(norm_w) output)
template <typename WT>
void RowKernels<WT>::rows_head(const ModelDims& d, int M, const RowsCtx& c, const void* W, const float* wscale, int n_rows, float* logits, int ld,
                               hipStream_t st, bool rms) {
    if constexpr (std::is_same<WT, float>::value) {
        throw Error("the MFMA row path needs bf16 or fp8 weights");
    } else {
        FS_REQUIRE(ld >= n_rows, "logits row stride must cover n_rows");
        // EPI_STORE with one K range writes slab 0 == the logits matrix itself (row stride ld)
        const GemmIn in{c.A, M, d.dim, W, wscale, n_rows};
        if (rms)  // folded decode step: c.A holds split(x * norm_w), c.ss the sum-of-squares partials of the last down projection
            launch_gemm3<EPI_STORE_RMS>(st, {in, {logits, ld}, {}, NormAux{nullptr, c.ss, nullptr, d.dim / 16, d.dim, d.eps}});
        else
            launch_gemm3<EPI_STORE>(st, {in, {logits, ld}});
        FS_LAUNCH_CHECK();
    }
}

template struct RowKernels<bf16_t>;
template struct RowKernels<float>;
template struct RowKernels<fp8_t>;

// ================================================================================================ fs_selftest_gemm (include/fishrt.h)
// ONE launcher call of this file on caller data and nothing else.  Everything a launch writes lies between 256-element guards of 0xFF bytes
// and is poisoned with 0xFF bytes (f32 / bf16 NaN) where the caller provides nothing; the fragment rows [M, Mcap) of a GEMM input are bf16
// NaN, so a live output that depends on a row that does not exist comes back NaN; the whole case is validated before the first device call.
namespace {
constexpr size_t kGemmGuard = 256;
struct GemmDev {  // device buffer of n elements of es bytes between two guards, all 0xFF bytes at first
    void* p = nullptr;
    size_t n = 0, es = 4;
    void alloc(size_t n_, size_t es_, hipStream_t st) {
        n = n_; es = es_;
        FS_HIP(hipMalloc(&p, (n + 2 * kGemmGuard) * es));
        FS_HIP(hipMemsetAsync(p, 0xFF, (n + 2 * kGemmGuard) * es, st));
    }
    char* data() const { return (char*)p + kGemmGuard * es; }
    void up(const void* src, size_t count, hipStream_t st) { FS_HIP(hipMemcpyAsync(data(), src, count * es, hipMemcpyHostToDevice, st)); }
    void down(void* dst, hipStream_t st) const { FS_HIP(hipMemcpyAsync(dst, data(), n * es, hipMemcpyDeviceToHost, st)); }
    void poison(hipStream_t st) { FS_HIP(hipMemsetAsync(data(), 0xFF, n * es, st)); }
    bool intact(hipStream_t st) const {
        if (!p) return true;
        std::vector<uint8_t> g(2 * kGemmGuard * es);
        FS_HIP(hipMemcpyAsync(g.data(), p, kGemmGuard * es, hipMemcpyDeviceToHost, st));
        FS_HIP(hipMemcpyAsync(g.data() + kGemmGuard * es, data() + n * es, kGemmGuard * es, hipMemcpyDeviceToHost, st));
        FS_HIP(hipStreamSynchronize(st));
        for (uint8_t b : g) if (b != 0xFF) return false;
        return true;
    }
    ~GemmDev() { if (p) (void)hipFree(p); }
};

struct GemmRowPos { int pos, rpos, sq; };
// everything validation derives from a case: the launch plan, its name, the output extents
struct GemmCaseInfo {
    GemmPlan plan;
    std::string name;
    int Mcap = 0, nblk = 0, C = 0, ldo = 0, n_seq = 0, n_state = 1;
    bool qkv = false, rms = false, store = false, residual = false, swiglu = false;
    size_t n_y = 0, n_planes = 0, n_ss = 0, n_pool = 0;
    std::vector<GemmRowPos> rows;
};
void gemm_req(bool ok, const char* msg) { if (!ok) throw Error(std::string("GEMM self-test: ") + msg); }

// position, RoPE row and sequence of activation row m, as gemm_epilogue's QKV branch derives them
GemmRowPos gemm_row_pos(const fs_gemm_case& c, int m) {
    const int sq = c.seq_rows > 0 ? m / c.seq_rows : m, j = c.seq_rows > 0 ? m - sq * c.seq_rows : 0;
    long long pos = (long long)c.pos + (c.seq_rows > 0 ? j : (long long)m * c.pos_step), rpos = pos + c.rope_off;
    if (c.pos_step < 0) { pos = c.row_pos[m]; rpos = pos + (c.row_rope_off ? c.row_rope_off[m] : c.rope_off); }
    if (c.epi == EPI_QKV_SEQ) { pos = (long long)c.seq_pos[sq] + j; rpos = pos + (c.seq_rope_off ? c.seq_rope_off[sq] : c.rope_off); }
    gemm_req(pos >= 0 && pos < (1 << 20) && rpos >= 0 && rpos < c.rope_rows, "a row's position or RoPE row is outside [0, 2^20) / the cos / sin tables");
    return {(int)pos, (int)rpos, sq};
}

void gemm_validate(const fs_gemm_case& c, GemmCaseInfo& I) {
    const auto req = gemm_req;
    req(c.op >= FS_GEMM_PREP && c.op <= FS_GEMM_DOWN, "unknown op");
    req(c.M >= 1 && c.M <= 1024, "1 <= M <= 1024");
    req(std::isfinite(c.eps) && c.eps >= 0.f, "eps must be finite and >= 0");
    I.Mcap = (c.M + PF_M - 1) / PF_M * PF_M;
    if (c.op == FS_GEMM_PREP) {
        req(c.D >= 32 && c.D <= 8192 && c.D % 32 == 0, "prep: 32 <= D <= 8192, D a multiple of 32 (fragment layout)");
        req(c.S >= 0 && c.S <= 8 && c.x && (c.S == 0 || c.p), "prep: 0 <= S <= 8, x is required, p with S > 0");
        I.name = c.D <= 1024 ? "prep/one" : "prep/reread";
        I.plan.gx = (unsigned)c.M;
        I.n_y = (size_t)c.M * c.D;
        I.n_planes = c.want_frag ? (size_t)2 * I.Mcap * c.D : 0;
        return;
    }
    req(c.N >= 1 && c.N <= 16384 && c.K >= 128 && c.K <= 8192 && c.K % 128 == 0, "1 <= N <= 16384, 128 <= K <= 8192, K a multiple of 128");
    req(c.x && c.w && (!c.fp8 || c.wscale), "x and w are required, wscale with fp8");
    if (c.op == FS_GEMM_DOWN) {
        I.plan = gemm_plan(GEMM_EPI_DOWN, 1, c.M, c.N, c.K, 0, c.fp8 != 0);
        req(c.y && c.g, "down: y and g are required");
        req((c.n_launches == 1 || c.n_launches == 2) && (c.n_launches == 1 || c.x2), "down: n_launches is 1 or 2, x2 with 2");
        req(c.epoch >= 1 && c.epoch < (1 << 19) && c.node_id >= 0 && c.node_id + c.n_launches <= 4096, "down: 1 <= epoch < 2^19, node ids < 4096");
        for (int l = 0; l < c.n_launches; ++l)
            req((uint32_t)c.stale_tag != (uint32_t)c.epoch * 4096u + (uint32_t)(c.node_id + l), "down: stale_tag equals a launch's own tag");
        I.nblk = c.N / 16; I.C = c.N;
        I.n_y = (size_t)c.n_launches * PF_M * c.N;
        I.n_planes = (size_t)c.n_launches * 2 * PF_M * c.N;
        I.n_ss = (size_t)c.n_launches * PF_M * I.nblk;
    } else {
        static const int pair_rt[9] = {1, 1, 2, 1, 1, 2, 1, 1, 1};  // the (EPI, RT) pairs rows_layer / rows_head launch
        req(c.epi >= EPI_STORE && c.epi <= EPI_QKV_SEQ && c.rt == pair_rt[c.epi], "rows: (epi, rt) is not a pair rows_layer / rows_head launch");
        req(c.ksplit >= 1 && c.ksplit <= 4, "rows: 1 <= ksplit <= 4");
        I.plan = gemm_plan(c.epi, c.rt, c.M, c.N, c.K, c.ksplit, c.fp8 != 0, c.big_min_m);
        I.store = c.epi == EPI_STORE || c.epi == EPI_STORE_RMS;
        I.residual = c.epi == EPI_RESIDUAL || c.epi == EPI_RESIDUAL_NORM;
        I.swiglu = c.epi == EPI_SWIGLU || c.epi == EPI_SWIGLU_RMS;
        I.qkv = c.epi == EPI_QKV || c.epi == EPI_QKV_RMS || c.epi == EPI_QKV_SEQ;
        I.rms = epi_rms(c.epi);
        req(I.store || c.ksplit == 1, "rows: only the STORE epilogues take split-K slabs");
        if (I.rms) {
            req(c.ss && c.nblk >= 8 && c.nblk <= 1024 && c.nblk % 8 == 0, "rows: *_RMS needs ss [M][nblk], nblk a multiple of 8 in [8, 1024]");
            I.nblk = c.nblk;
        }
        if (I.store) {
            req(c.ldy >= c.N, "rows: ldy must cover N");
            I.n_y = (size_t)c.ksplit * I.Mcap * c.ldy;
        } else if (I.residual) {
            req(c.y && c.N % 2 == 0 && c.ldy >= c.N && c.ldy % 2 == 0, "rows: RESIDUAL* needs y, even N, even ldy >= N");
            I.n_y = (size_t)I.Mcap * c.ldy;
            if (c.epi == EPI_RESIDUAL_NORM) {
                const int rows = I.plan.kind == GemmPlan::BIG ? GB_ROWS : 16;
                I.nblk = (int)I.plan.gx;
                req(c.g && c.N % rows == 0 && c.N % 32 == 0 && I.nblk % 8 == 0, "rows: RESIDUAL_NORM needs g, whole blocks and a block count that is a multiple of 8");
                I.C = c.N; I.n_planes = (size_t)2 * I.Mcap * c.N; I.n_ss = (size_t)I.Mcap * I.nblk;
            }
        } else if (I.swiglu) {
            I.ldo = c.ldo ? c.ldo : c.N / 2;
            req(c.N % 64 == 0 && I.ldo >= c.N / 2 && I.ldo % 32 == 0, "rows: SWIGLU* needs N a multiple of 64 and ldo >= N / 2, a multiple of 32");
            I.C = I.ldo; I.n_planes = (size_t)2 * I.Mcap * I.ldo;
        } else {
            req((c.Dh == 64 || c.Dh == 32) && c.Hk >= 1 && c.H >= c.Hk && c.H <= 32 && c.H % c.Hk == 0, "rows: QKV* needs Dh in {32, 64}, 1 <= Hk <= H <= 32, H a multiple of Hk");
            const int qdim = c.H * c.Dh;
            req(c.N == (c.H + 2 * c.Hk) * c.Dh && c.ldy >= qdim && c.ldy % 2 == 0, "rows: QKV* needs N == (H + 2 Hk) Dh and an even ldy >= H Dh");
            req(c.cos_t && c.sin_t && c.rope_rows >= 1 && c.rope_rows <= (1 << 16), "rows: QKV* needs cos_t, sin_t, 1 <= rope_rows <= 2^16");
            req(c.k && c.v && c.n_pages >= 1 && c.n_pages <= 4096, "rows: QKV* needs k, v, 1 <= n_pages <= 4096");
            req(c.page_table && c.pt_rows >= 1 && c.pt_len >= 1 && (long long)c.pt_rows * c.pt_len <= (1 << 20) && c.pt_stride >= 0, "rows: page_table [pt_rows][pt_len] is required");
            const long long n_tab = (long long)c.pt_rows * c.pt_len;
            for (long long i = 0; i < n_tab; ++i) req(c.page_table[i] >= 0 && c.page_table[i] < c.n_pages, "a page id is outside the pool");
            req(c.pos_step == 1 || c.pos_step == 0 || c.pos_step == -1, "pos_step is 1, 0 or -1");
            req(c.pos_step >= 0 || c.row_pos, "pos_step < 0 needs row_pos");
            req(c.seq_rows >= 0 && (c.seq_rows == 0 || (c.pos_step == 1 && c.M % c.seq_rows == 0)), "group rows: pos_step 1, M a multiple of seq_rows");
            req(c.epi != EPI_QKV_SEQ || (c.seq_rows > 0 && c.seq_pos), "QKV_SEQ needs seq_rows > 0 and seq_pos");
            I.n_seq = c.seq_rows > 0 ? c.M / c.seq_rows : 0;
            I.n_state = std::max(std::max(c.M, I.n_seq), 1);
            std::set<std::pair<int, int>> cells;
            for (int m = 0; m < c.M; ++m) {
                const GemmRowPos rp = gemm_row_pos(c, m);
                const long long slot = (long long)rp.sq * c.pt_stride + rp.pos / KV_PAGE;
                req(rp.pos / KV_PAGE < c.pt_len && slot < n_tab, "a row's page-table slot is outside the table");
                req(cells.insert({c.page_table[slot], rp.pos % KV_PAGE}).second, "two rows write the same cache row");
                I.rows.push_back(rp);
            }
            if (c.o1) {
                req(I.plan.kind == GemmPlan::GEMM3 && qdim % 32 == 0, "rows: o1 needs the k_gemm3 path and H Dh a multiple of 32");
                I.C = qdim; I.n_planes = (size_t)2 * I.Mcap * qdim;
            }
            I.n_y = (size_t)I.Mcap * c.ldy;
            I.n_pool = (size_t)c.n_pages * c.Hk * KV_PAGE * c.Dh;
        }
    }
    I.name = I.plan.name();
    // the weights: exactly representable in the weight type, so that the caller's f32 matrix IS what the kernel multiplies
    const size_t nw = (size_t)c.N * c.K;
    for (size_t i = 0; i < nw; ++i) {
        const float w = c.w[i];
        const bool exact = c.fp8 ? e4m3_to_f32(f32_to_e4m3(w)) == w : bf16_to_f32_host(f32_to_bf16_host(w)) == w;
        req(exact, c.fp8 ? "a weight is not an e4m3fn value" : "a weight is not a bf16 value");
    }
}

struct GemmStream {
    hipStream_t st = nullptr;
    explicit GemmStream(int device) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) throw Error("no HIP device visible: libfishrt has no CPU fallback (MI355X / gfx950 required)");
        FS_REQUIRE(device >= 0 && device < ndev, "device_id out of range");
        FS_HIP(hipSetDevice(device));
        FS_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    }
    ~GemmStream() { if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); } }
};

// fragment-major bf16 [Mcap][C] (hi and lo parts) -> two f32 planes [Mcap][C]
void gemm_defrag(const std::vector<uint16_t>& A, int Mcap, int C, float* out) {
    const size_t plane = (size_t)Mcap * C;
    for (int m = 0; m < Mcap; ++m)
        for (int k = 0; k < C; ++k) {
            out[(size_t)m * C + k] = bf16_to_f32_host(A[frag_off(m, k, 0, C)]);
            out[plane + (size_t)m * C + k] = bf16_to_f32_host(A[frag_off(m, k, 1, C)]);
        }
}
// the GEMM input of x [M][K]: a plain split by k_prep (no norm), rows [M, Mcap) left as bf16 NaN
void gemm_make_frags(const float* x, int M, int Mcap, int K, GemmDev& dX, GemmDev& dXf, hipStream_t st) {
    dX.alloc((size_t)M * K, 4, st); dX.up(x, (size_t)M * K, st);
    dXf.alloc((size_t)2 * Mcap * K, 2, st);
    hipLaunchKernelGGL(k_prep, dim3(M), dim3(256), 0, st, (float*)dX.data(), K, (const float*)nullptr, 0, (size_t)0, (const float*)nullptr, 0.f, (bf16_t*)dXf.data());
    FS_LAUNCH_CHECK();
}
void gemm_upload_w(const fs_gemm_case& c, GemmDev& dW, GemmDev& dS, hipStream_t st) {
    const size_t nw = (size_t)c.N * c.K;
    if (c.fp8) {
        std::vector<uint8_t> h(nw);
        for (size_t i = 0; i < nw; ++i) h[i] = f32_to_e4m3(c.w[i]);
        dW.alloc(nw, 1, st); dW.up(h.data(), nw, st);
        dS.alloc((size_t)c.N, 4, st); dS.up(c.wscale, (size_t)c.N, st);
        FS_HIP(hipStreamSynchronize(st));
    } else {
        std::vector<uint16_t> h(nw);
        for (size_t i = 0; i < nw; ++i) h[i] = f32_to_bf16_host(c.w[i]);
        dW.alloc(nw, 2, st); dW.up(h.data(), nw, st);
        FS_HIP(hipStreamSynchronize(st));
    }
}

void gemm_run_prep(const fs_gemm_case& c, const GemmCaseInfo& I, fs_gemm_out& o, hipStream_t st) {
    GemmDev dX, dP, dW, dA;
    dX.alloc((size_t)c.M * c.D, 4, st); dX.up(c.x, (size_t)c.M * c.D, st);
    if (c.S > 0) { dP.alloc((size_t)c.S * c.M * c.D, 4, st); dP.up(c.p, (size_t)c.S * c.M * c.D, st); }
    if (c.norm_w) { dW.alloc((size_t)c.D, 4, st); dW.up(c.norm_w, (size_t)c.D, st); }
    if (c.want_frag) dA.alloc((size_t)2 * I.Mcap * c.D, 2, st);
    hipLaunchKernelGGL(k_prep, dim3(c.M), dim3(256), 0, st, (float*)dX.data(), c.D, c.S > 0 ? (const float*)dP.data() : nullptr, c.S, (size_t)c.M * c.D,
                       c.norm_w ? (const float*)dW.data() : nullptr, c.eps, c.want_frag ? (bf16_t*)dA.data() : nullptr);
    FS_LAUNCH_CHECK();
    std::vector<uint16_t> hA(dA.n);
    if (o.y) dX.down(o.y, st);
    if (c.want_frag) dA.down(hA.data(), st);
    FS_HIP(hipStreamSynchronize(st));
    if (c.want_frag && o.planes) gemm_defrag(hA, I.Mcap, c.D, o.planes);
    o.guard_ok = (dX.intact(st) && dA.intact(st)) ? 1 : 0;
}

template <int EPI, int RT>
void gemm_launch_pair(hipStream_t st, const GemmArgs& g) { launch_gemm3<EPI, RT>(st, g); }

void gemm_run_rows(const fs_gemm_case& c, const GemmCaseInfo& I, fs_gemm_out& o, hipStream_t st) {
    GemmDev dX, dXf, dW, dS, dY, dOf, dSS, dG, dCos, dSin, dK, dV, dTab, dState;
    gemm_make_frags(c.x, c.M, I.Mcap, c.K, dX, dXf, st);
    gemm_upload_w(c, dW, dS, st);
    GemmArgs g;
    g.in = GemmIn{(const bf16_t*)dXf.data(), c.M, c.K, dW.data(), c.fp8 ? (const float*)dS.data() : nullptr, c.N, c.ksplit, c.big_min_m};
    if (I.n_y) {
        dY.alloc(I.n_y, 4, st);
        if (I.residual)
            FS_HIP(hipMemcpyAsync(dY.data(), c.y, (size_t)c.M * c.ldy * 4, hipMemcpyHostToDevice, st));
    }
    if (I.n_planes) dOf.alloc(I.n_planes, 2, st);
    g.out = GemmOut{I.n_y ? (float*)dY.data() : nullptr, c.ldy, (size_t)I.Mcap * c.ldy, nullptr, 0};
    if (I.swiglu) { g.out.Of = (bf16_t*)dOf.data(); g.out.ldo = I.ldo; }
    if (I.qkv && c.o1) g.out.Of = (bf16_t*)dOf.data();
    if (I.rms) {
        dSS.alloc((size_t)I.Mcap * I.nblk, 4, st); dSS.up(c.ss, (size_t)c.M * I.nblk, st);
        g.na = NormAux{nullptr, (float*)dSS.data(), nullptr, I.nblk, c.K, c.eps};
    }
    if (c.epi == EPI_RESIDUAL_NORM) {
        dSS.alloc(I.n_ss, 4, st);
        dG.alloc((size_t)c.N, 4, st); dG.up(c.g, (size_t)c.N, st);
        g.na = NormAux{(const float*)dG.data(), (float*)dSS.data(), (bf16_t*)dOf.data(), I.nblk, c.N, c.eps};
    }
    std::vector<SeqState> hs((size_t)I.n_state);
    std::vector<uint16_t> hk, hv;
    if (I.qkv) {
        for (auto& s : hs) { std::memset(&s, 0, sizeof(SeqState)); s.pos = c.pos; s.rope_off = c.rope_off; }
        if (c.pos_step < 0)
            for (int m = 0; m < c.M; ++m) { hs[(size_t)m].pos = c.row_pos[m]; if (c.row_rope_off) hs[(size_t)m].rope_off = c.row_rope_off[m]; }
        if (c.epi == EPI_QKV_SEQ)
            for (int s = 0; s < I.n_seq; ++s) { hs[(size_t)s].pos = c.seq_pos[s]; if (c.seq_rope_off) hs[(size_t)s].rope_off = c.seq_rope_off[s]; }
        dState.alloc(hs.size() * sizeof(SeqState), 1, st); dState.up(hs.data(), hs.size() * sizeof(SeqState), st);
        const size_t nr = (size_t)c.rope_rows * (c.Dh / 2);
        dCos.alloc(nr, 4, st); dCos.up(c.cos_t, nr, st);
        dSin.alloc(nr, 4, st); dSin.up(c.sin_t, nr, st);
        hk.resize(I.n_pool); hv.resize(I.n_pool);
        for (size_t i = 0; i < I.n_pool; ++i) { hk[i] = f32_to_bf16_host(c.k[i]); hv[i] = f32_to_bf16_host(c.v[i]); }
        dK.alloc(I.n_pool, 2, st); dK.up(hk.data(), I.n_pool, st);
        dV.alloc(I.n_pool, 2, st); dV.up(hv.data(), I.n_pool, st);
        const size_t nt = (size_t)c.pt_rows * c.pt_len;
        dTab.alloc(nt, 4, st); dTab.up(c.page_table, nt, st);
        g.qkv = GemmQkv{(const float*)dCos.data(), (const float*)dSin.data(), (const SeqState*)dState.data(),
                        KVView{dK.data(), dV.data(), (const int*)dTab.data()}, c.H, c.Hk, c.Dh, RowMap{c.pos_step, c.pt_stride, c.seq_rows}};
    }
    switch (c.epi) {
    case EPI_STORE: gemm_launch_pair<EPI_STORE, 1>(st, g); break;
    case EPI_RESIDUAL: gemm_launch_pair<EPI_RESIDUAL, 1>(st, g); break;
    case EPI_SWIGLU: gemm_launch_pair<EPI_SWIGLU, 2>(st, g); break;
    case EPI_QKV: gemm_launch_pair<EPI_QKV, 1>(st, g); break;
    case EPI_RESIDUAL_NORM: gemm_launch_pair<EPI_RESIDUAL_NORM, 1>(st, g); break;
    case EPI_SWIGLU_RMS: gemm_launch_pair<EPI_SWIGLU_RMS, 2>(st, g); break;
    case EPI_QKV_RMS: gemm_launch_pair<EPI_QKV_RMS, 1>(st, g); break;
    case EPI_STORE_RMS: gemm_launch_pair<EPI_STORE_RMS, 1>(st, g); break;
    default: gemm_launch_pair<EPI_QKV_SEQ, 1>(st, g); break;
    }
    FS_LAUNCH_CHECK();
    std::vector<uint16_t> hA(dOf.n);
    if (o.y && I.n_y) dY.down(o.y, st);
    if (I.n_planes) dOf.down(hA.data(), st);
    if (o.ss && I.n_ss) dSS.down(o.ss, st);
    if (I.qkv) { dK.down(hk.data(), st); dV.down(hv.data(), st); }
    FS_HIP(hipStreamSynchronize(st));
    if (I.n_planes && o.planes) gemm_defrag(hA, I.Mcap, I.C, o.planes);
    if (I.qkv)
        for (size_t i = 0; i < I.n_pool; ++i) { if (o.k) o.k[i] = bf16_to_f32_host(hk[i]); if (o.v) o.v[i] = bf16_to_f32_host(hv[i]); }
    bool ok = true;
    for (const GemmDev* b : {&dXf, &dY, &dOf, &dSS, &dK, &dV}) ok = b->intact(st) && ok;
    o.guard_ok = ok ? 1 : 0;
}

void gemm_run_down(const fs_gemm_case& c, const GemmCaseInfo& I, fs_gemm_out& o, hipStream_t st) {
    // the owner waves wait for blocks of the same launch: never launched where the engine would not launch it
    gemm_req(gemm_down_resident(c.N, c.K, c.fp8 != 0), "down: this device does not hold the whole grid at once (gemm_down_resident)");
    GemmDev dX[2], dXf[2], dW, dS, dY, dA, dSS, dG, dXchg, dEpoch;
    gemm_make_frags(c.x, c.M, PF_M, c.K, dX[0], dXf[0], st);
    if (c.n_launches == 2) gemm_make_frags(c.x2, c.M, PF_M, c.K, dX[1], dXf[1], st);
    gemm_upload_w(c, dW, dS, st);
    dY.alloc((size_t)PF_M * c.N, 4, st); dY.up(c.y, (size_t)c.M * c.N, st);
    dA.alloc((size_t)2 * PF_M * c.N, 2, st);
    dSS.alloc((size_t)PF_M * I.nblk, 4, st);
    dG.alloc((size_t)c.N, 4, st); dG.up(c.g, (size_t)c.N, st);
    const size_t units = rows_xchg_bytes(c.N) / 16;
    std::vector<uint32_t> hx(units * 4);
    for (size_t u = 0; u < units; ++u) { hx[4 * u] = 0x7FC00000u; hx[4 * u + 1] = (uint32_t)c.stale_tag; hx[4 * u + 2] = 0x7FC00000u; hx[4 * u + 3] = (uint32_t)c.stale_tag; }
    dXchg.alloc(units * 4, 4, st); dXchg.up(hx.data(), units * 4, st);
    const uint32_t he[2] = {(uint32_t)c.epoch, 0u};
    dEpoch.alloc(2, 4, st); dEpoch.up(he, 2, st);
    FS_HIP(hipStreamSynchronize(st));
    const NormAux na{(const float*)dG.data(), (float*)dSS.data(), (bf16_t*)dA.data(), I.nblk, c.N, c.eps};
    std::vector<uint16_t> hA(dA.n);
    for (int l = 0; l < c.n_launches; ++l) {
        if (l > 0) { dA.poison(st); dSS.poison(st); }
        launch_gemm_down(st, (const bf16_t*)dXf[l].data(), c.M, c.K, dW.data(), c.fp8 ? (const float*)dS.data() : nullptr, c.N, (float*)dY.data(), c.N, na,
                         dXchg.data(), (uint32_t*)dEpoch.data(), (uint32_t)(c.node_id + l));
        FS_LAUNCH_CHECK();
        uint32_t e[2] = {0u, 0u};
        if (o.y) dY.down(o.y + (size_t)l * PF_M * c.N, st);
        dA.down(hA.data(), st);
        if (o.ss) dSS.down(o.ss + (size_t)l * PF_M * I.nblk, st);
        FS_HIP(hipMemcpyAsync(e, dEpoch.data(), 8, hipMemcpyDeviceToHost, st));
        FS_HIP(hipStreamSynchronize(st));
        if (o.planes) gemm_defrag(hA, PF_M, c.N, o.planes + (size_t)l * 2 * PF_M * c.N);
        if (o.epoch1) o.epoch1[l] = e[1];
    }
    bool ok = true;
    for (const GemmDev* b : {&dXf[0], &dXf[1], &dY, &dA, &dSS, &dXchg, &dEpoch}) ok = b->intact(st) && ok;
    o.guard_ok = ok ? 1 : 0;
}
}  // namespace

void gemm_selftest(int device, const fs_gemm_case& c, fs_gemm_out& o) {
    GemmCaseInfo I;
    gemm_validate(c, I);
    std::snprintf(o.variant, o.variant_cap, "%s", I.name.c_str());
    o.grid[0] = (int32_t)I.plan.gx; o.grid[1] = (int32_t)I.plan.gy; o.grid[2] = (int32_t)I.plan.gz;
    o.n_y = I.n_y; o.n_planes = I.n_planes; o.n_ss = I.n_ss;
    if (c.plan_only) return;
    gemm_req((!o.y || o.y_cap >= I.n_y) && (!o.planes || o.planes_cap >= I.n_planes) && (!o.ss || o.ss_cap >= I.n_ss) &&
             ((!o.k && !o.v) || o.pool_cap >= I.n_pool), "an output capacity is too small");
    GemmStream gs(device);
    if (c.op == FS_GEMM_PREP) gemm_run_prep(c, I, o, gs.st);
    else if (c.op == FS_GEMM_ROWS) gemm_run_rows(c, I, o, gs.st);
    else gemm_run_down(c, I, o, gs.st);
}

}  // namespace fs
