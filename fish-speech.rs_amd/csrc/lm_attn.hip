// Attention kernels of the dual-AR transformer for gfx950 (MI355X): flash-decoding over the paged KV cache for the batch-1 token
// path (k_attn_decode, merged by k_wo in lm_kernels.hip), and the row path's attention nodes -- one-node static-batch decode
// (k_attn_rows), the fast decoder's <= 8-token rows (k_attn_small_rows, _tbl), the chunk combine, and the causal MFMA prefill.
// Launch interface: AttnKernels<WT> in lm_kernels.h; RowKernels<WT>::rows_layer (lm_gemm.hip) decides which rows get an attention node.
// Reference semantics implemented: fish_speech_core/lib/lm/dual_ar.rs:252-279 (SDPA), :239-249 (rope_i, k_attn_small_rows_tbl).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/fishrt.h"
#include "fs_common.h"
#include "lm_kernels.h"
#include "lm_dev.h"

namespace fs {

// ------------------------------------------------------------------------------------------------ decode attention
// Flash-decoding over the paged cache.  grid = Hk * n_chunks_max blocks of 4 waves; block (g, c) owns the n_rep query
// heads of kv head g and the ATTN_CHUNK tokens [c*CH, (c+1)*CH); blocks past the current length exit at once, so the
// captured graph serves every sequence length.  Each wave stages its TW tokens of K and V (one coalesced 16-B/lane
// load per KiB, all in flight together) into its private LDS tile, then lane GROUPS of LPT lanes (LPT*16 B = one head
// row) each own one (query head, token subset): scores by DPP group-sums, a two-pass softmax in registers (no rescale
// chain), P.V accumulated on the group's own dims -- no cross-group reduction of the output.  The block merges its
// waves in LDS and writes one un-normalised partial {o[Dh], m, l} per (head, chunk); k_wo combines the chunks.
// chunk = NW waves x TW tokens (16 waves x 8 tokens was measured too: 4.49 vs 4.36 us, the wider block merge eats the shorter loop)
template <typename WT, int DH> struct AttnGeom { static constexpr int TW = 16, NW = 8; };                          // bf16: 8 waves x 16 tokens = 128-token chunks
template <int DH> struct AttnGeom<float, DH> { static constexpr int TW = 16, NW = 4; };                           // f32 :  64-token chunks

// Wave-tile geometry of k_attn_decode and k_attn_rows, and their block merge.  Lane l of a wave belongs to lane group l / LPT: query head
// rl(l) of the current head pass, token subset ts(l) (tokens ts, ts + NTS, ... of the wave's tile), 16-B slice sub(l) of the head row.
// The tile request, the stash, the score loop and the p.V loop are written out in both kernels: each of them as a shared __forceinline__
// helper moves the VGPR count of some instantiation (profiles/attn_split_resource_usage.md), the merge does not.
template <typename WT, int DH, int NREP>
struct AttnTile {
    static constexpr int EPL = WTr<WT>::EPL;
    static constexpr int LPT = DH / EPL;             // lanes per head row
    static constexpr int G = 64 / LPT;               // lane groups per wave
    static constexpr int NRP = NREP < G ? NREP : G;  // heads served per pass
    static constexpr int NTS = G / NRP;              // token subsets per head
    static constexpr int NHP = NREP / NRP;           // head passes
    static constexpr int TW = AttnGeom<WT, DH>::TW;  // tokens per wave
    static constexpr int NW = AttnGeom<WT, DH>::NW;  // waves per block
    static constexpr int CH = NW * TW;               // tokens per block
    static constexpr int TPG = TW / NTS;             // tokens per group
    static constexpr int NLD = TW * LPT / 64;        // 16-B loads per lane per tile
    static_assert(TW % NTS == 0 && NLD >= 1, "attention geometry");
    static_assert(KV_PAGE % TW == 0, "a wave's tokens must not straddle a KV page");
    // q . (k^T * scale)  (dual_ar.rs:260).  For head_dim 64 the scale is 2^-3: scaling by a power of two commutes with every
    // f32 rounding, so folding it into q once is bit-identical to scaling each k element (8 multiplies per token saved).
    static constexpr bool POW2 = (DH == 64 || DH == 16 || DH == 256);
    using vec = typename WTr<WT>::vec;
    using Tile = WT[NW][TW * DH];                    // LDS: one private K (or V) tile per wave
    using Merge = float[NW][NREP][NTS][DH + 2];      // LDS: {o[DH], m, l} per (wave, head, token subset)

    __device__ static __forceinline__ int sub(int lane) { return lane % LPT; }
    __device__ static __forceinline__ int rl(int lane) { return (lane / LPT) % NRP; }
    __device__ static __forceinline__ int ts(int lane) { return (lane / LPT) / NRP; }

    // (behind a block barrier) dim dd of head r merged over the waves and token subsets: max, sum and un-normalised output
    __device__ static __forceinline__ void merge(const Merge& sp, int r, int dd, float& mn, float& L, float& O) {
        mn = -1e30f;
#pragma unroll
        for (int w = 0; w < NW; ++w)
#pragma unroll
            for (int k = 0; k < NTS; ++k) mn = fmaxf(mn, sp[w][r][k][DH]);
        L = 0.f; O = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w)
#pragma unroll
            for (int k = 0; k < NTS; ++k) {
                const float cf = __expf(sp[w][r][k][DH] - mn);
                L += sp[w][r][k][DH + 1] * cf;
                O += sp[w][r][k][dd] * cf;
            }
    }
};

template <typename WT, int DH, int NREP>
__global__ __launch_bounds__((AttnGeom<WT, DH>::NW * 64)) void k_attn_decode(const float* __restrict__ q_all, KVView kv,
                                                     const SeqState* __restrict__ state, float* __restrict__ part_all,
                                                     int Hk, int n_chunks_max, int nc_launch, int pos_step, int pt_stride, int hsplit) {
    using AT = AttnTile<WT, DH, NREP>;
    using vec = typename AT::vec;
    // hsplit > 1: the query heads of a kv group are spread over hsplit blocks of NREP heads each (the score / P.V work of a wave is
    // VALU-bound: 16 tokens x 8 heads ~ 900 instructions; the K/V tiles are then read hsplit times, from L2)
    const int GH = NREP * hsplit;
    // blockIdx.y = activation row m (0 for the batch-1 decode step): prefill -> token pos + m of one sequence (pos_step 1,
    // pt_stride 0); batched decode -> sequence m at pos (pos_step 0, pt_stride = page-table stride)
    kv.page_table += (size_t)blockIdx.y * pt_stride;
    const float* q = q_all + (size_t)blockIdx.y * Hk * GH * DH;
    float* part = part_all + (size_t)blockIdx.y * Hk * GH * n_chunks_max * (DH + 2);
    // block id = head part * (Hk * nc_launch) + (kv head * nc_launch + chunk): with Hk * nc_launch a multiple of 8 the blocks that share
    // a K/V tile get ids congruent mod 8, i.e. the same XCD and L2 (workgroups go round-robin over the 8 XCDs)
    const int tile = blockIdx.x % (Hk * nc_launch), hb = (int)(blockIdx.x / (Hk * nc_launch)) * NREP;
    const int g = tile / nc_launch, c = tile % nc_launch;  // nc_launch <= n_chunks_max chunks are launched
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __shared__ __attribute__((aligned(16))) typename AT::Tile sk, sv;
    __shared__ typename AT::Merge sp;
    const int t_base = c * AT::CH + wave * AT::TW;
    // stage K/V tiles: lane l of load i covers token (i*64 + l) / LPT, 16-B slice l % LPT (1 KiB contiguous per load)
    // all TW tokens of a wave live in ONE page (TW divides KV_PAGE, t_base is TW-aligned): a single wave-uniform
    // (scalar) page-table read, then 1 KiB-contiguous tile loads.  Neither depends on the current length: the page-table
    // slot exists for every launched chunk (unassigned slots hold a valid page id) and rows past the length are stale but
    // in bounds (the pools are zero-initialised, so always finite) -- they are masked below.  The length itself is read
    // in parallel instead of in front of the chain.
    const int t_base_u = __builtin_amdgcn_readfirstlane(t_base);
    const int page = kv.page_table[t_base_u / KV_PAGE];
    const WT* kpage = reinterpret_cast<const WT*>(kv.k) + (size_t)(page * Hk + g) * KV_PAGE * DH;
    const WT* vpage = reinterpret_cast<const WT*>(kv.v) + (size_t)(page * Hk + g) * KV_PAGE * DH;
    vec kreg[AT::NLD], vreg[AT::NLD];
#pragma unroll
    for (int i = 0; i < AT::NLD; ++i) {
        const int tl = (i * 64 + lane) / AT::LPT, sl = lane % AT::LPT;
        const int t = t_base + tl;
        kreg[i] = *reinterpret_cast<const vec*>(kpage + (size_t)(t % KV_PAGE) * DH + sl * AT::EPL);
        vreg[i] = *reinterpret_cast<const vec*>(vpage + (size_t)(t % KV_PAGE) * DH + sl * AT::EPL);
    }
    const int sub = AT::sub(lane), rl = AT::rl(lane), ts = AT::ts(lane);
    float qr[AT::NHP][AT::EPL];
#pragma unroll
    for (int hp = 0; hp < AT::NHP; ++hp) {
        const float* qp = q + (size_t)(g * GH + hb + hp * AT::NRP + rl) * DH + sub * AT::EPL;
#pragma unroll
        for (int i = 0; i < AT::EPL; ++i) qr[hp][i] = qp[i];
    }
    if (AT::POW2) {
        const float s0 = 1.0f / sqrtf((float)DH);
#pragma unroll
        for (int hp = 0; hp < AT::NHP; ++hp)
#pragma unroll
            for (int i = 0; i < AT::EPL; ++i) qr[hp][i] *= s0;
    }
    FS_ISSUE_FENCE();
    const int T = row_pos(state, (int)blockIdx.y, pos_step) + 1;  // the row's own K/V were appended by the qkv stage
    if (c * AT::CH >= T) return;
#pragma unroll
    for (int i = 0; i < AT::NLD; ++i) {
        *reinterpret_cast<vec*>(&sk[wave][(size_t)(i * 64 + lane) * AT::EPL]) = kreg[i];
        *reinterpret_cast<vec*>(&sv[wave][(size_t)(i * 64 + lane) * AT::EPL]) = vreg[i];
    }
    // (each wave reads only the tile it wrote: no block barrier needed, the compiler orders the LDS accesses)
    const float scale = 1.0f / sqrtf((float)DH);
#pragma unroll
    for (int hp = 0; hp < AT::NHP; ++hp) {  // one chunk: two-pass softmax in registers, no rescale chain
        float sc[AT::TPG];
        float m = -1e30f;
#pragma unroll
        for (int j = 0; j < AT::TPG; ++j) {
            const int tl = ts + j * AT::NTS;
            float kf[AT::EPL];
            WTr<WT>::unpack(*reinterpret_cast<const vec*>(&sk[wave][(size_t)tl * DH + sub * AT::EPL]), kf);
            float a = 0.f;
#pragma unroll
            for (int i = 0; i < AT::EPL; ++i) a = AT::POW2 ? fmaf(qr[hp][i], kf[i], a) : fmaf(qr[hp][i], kf[i] * scale, a);
            a = group_sum<AT::LPT>(a);
            sc[j] = (t_base + tl < T) ? a : -1e30f;
            m = fmaxf(m, sc[j]);
        }
        float l = 0.f, o[AT::EPL];
#pragma unroll
        for (int i = 0; i < AT::EPL; ++i) o[i] = 0.f;
#pragma unroll
        for (int j = 0; j < AT::TPG; ++j) {
            const int tl = ts + j * AT::NTS;
            const float p = (t_base + tl < T) ? __expf(sc[j] - m) : 0.f;
            l += p;
            float vf[AT::EPL];
            WTr<WT>::unpack(*reinterpret_cast<const vec*>(&sv[wave][(size_t)tl * DH + sub * AT::EPL]), vf);
#pragma unroll
            for (int i = 0; i < AT::EPL; ++i) o[i] = fmaf(p, vf[i], o[i]);
        }
        float* dst = sp[wave][hp * AT::NRP + rl][ts];
#pragma unroll
        for (int i = 0; i < AT::EPL; ++i) dst[sub * AT::EPL + i] = o[i];
        if (sub == 0) { dst[DH] = m; dst[DH + 1] = l; }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < NREP * DH; e += AT::NW * 64) {
        const int r = e / DH, dd = e % DH;
        float mn, L, O;
        AT::merge(sp, r, dd, mn, L, O);
        float* dst = part + ((size_t)(g * GH + hb + r) * n_chunks_max + c) * (DH + 2);
        dst[dd] = O;
        if (dd == 0) { dst[DH] = mn; dst[DH + 1] = L; }
    }
}

// Static-batch decode attention in ONE node: block = (kv head g, activation row m) walks the row's whole KV prefix chunk by
// chunk (k_attn_decode's geometry; the next chunk's K/V tiles are in flight while the current one is
// scored), every lane group keeps a running (max, sum, o) (online softmax), the waves meet once in LDS and the normalised result
// goes straight into the fragment-major hi/lo input of the Wo GEMM -- replaces k_attn_decode over (chunks x rows) blocks +
// k_attn_combine (two graph nodes and the partials round trip) for the rows-are-sequences passes.
// PART (batch-1 decode over a LONG prefix, > 8 chunks of 128 tokens): blockIdx.z = super-chunk of `tpb` consecutive chunks; instead
// of the normalised hi/lo row the block leaves {o, m, l} in slot blockIdx.z of k_attn_decode's partials layout, so that k_wo always
// merges <= 8 partials in registers (its general LDS merge over 32..64 chunks costs 9..16 us per layer at 4..8 k tokens).
template <typename WT, int DH, int NREP, bool PART = false>
__global__ __launch_bounds__((AttnGeom<WT, DH>::NW * 64)) void k_attn_rows(const float* __restrict__ q_all, KVView kv,
                                                   const SeqState* __restrict__ state, int Hk, int pos_step, int pt_stride,
                                                   bf16_t* __restrict__ Ohi, int hsplit, float* __restrict__ part_all = nullptr,
                                                   int n_chunks_max = 0, int tpb = 1 << 30) {
    using AT = AttnTile<WT, DH, NREP>;
    using vec = typename AT::vec;
    // hsplit > 1: the query heads of a kv group are spread over hsplit blocks of NREP heads each (small batches: more blocks,
    // less VALU work per wave; the K/V tiles are then read hsplit times, from L2)
    int g = blockIdx.x / hsplit, hb = (blockIdx.x % hsplit) * NREP, mrow = blockIdx.y;
    if (!PART && hsplit > 1) {
        // XCD-aware placement: workgroups go round-robin over the 8 XCDs by linear id, and each XCD has its own L2 -- the hsplit blocks
        // that share one (kv head, row) K/V stream must land on ONE XCD or the stream crosses the fabric hsplit times (PMC at B = 32:
        // 711 MB per step for 162 MB of K/V with the plain mapping)
        const int total = gridDim.x * gridDim.y, per_xcd = total / (8 * hsplit);
        if (per_xcd * 8 * hsplit == total) {
            const int lin = blockIdx.x + gridDim.x * blockIdx.y, k = lin >> 3, grp = (lin & 7) * per_xcd + k / hsplit;
            g = grp % Hk; mrow = grp / Hk; hb = (k % hsplit) * NREP;
        }
    }
    const int GH = NREP * hsplit;  // query heads per kv head
    kv.page_table += (size_t)mrow * pt_stride;
    const float* q = q_all + (size_t)mrow * Hk * GH * DH;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __shared__ __attribute__((aligned(16))) typename AT::Tile sk, sv;
    __shared__ typename AT::Merge sp;
    const int T = row_pos(state, mrow, pos_step) + 1;  // the row's own K/V were appended by the qkv stage
    const int nc_all = (T + AT::CH - 1) / AT::CH;
    const int c0 = PART ? (int)blockIdx.z * tpb : 0, nc = PART ? min(nc_all, c0 + tpb) : nc_all;  // this block's chunks [c0, nc)
    if (c0 >= nc) return;  // super-chunk past the current length (the graph bucket launches a power of two of them)
    vec kreg[AT::NLD], vreg[AT::NLD];
    auto load_tiles = [&](int c) {  // chunk c: this wave's TW tokens live in one page
        const int t_base = __builtin_amdgcn_readfirstlane(c * AT::CH + wave * AT::TW);
        const int page = kv.page_table[t_base / KV_PAGE];
        const WT* kpage = reinterpret_cast<const WT*>(kv.k) + (size_t)(page * Hk + g) * KV_PAGE * DH;
        const WT* vpage = reinterpret_cast<const WT*>(kv.v) + (size_t)(page * Hk + g) * KV_PAGE * DH;
#pragma unroll
        for (int i = 0; i < AT::NLD; ++i) {
            const int tl = (i * 64 + lane) / AT::LPT, sl = lane % AT::LPT;
            const int t = t_base + tl;
            kreg[i] = *reinterpret_cast<const vec*>(kpage + (size_t)(t % KV_PAGE) * DH + sl * AT::EPL);
            vreg[i] = *reinterpret_cast<const vec*>(vpage + (size_t)(t % KV_PAGE) * DH + sl * AT::EPL);
        }
    };
    load_tiles(c0);
    const int sub = AT::sub(lane), rl = AT::rl(lane), ts = AT::ts(lane);
    const float scale = 1.0f / sqrtf((float)DH);
    float qr[AT::NHP][AT::EPL];
#pragma unroll
    for (int hp = 0; hp < AT::NHP; ++hp) {
        const float* qp = q + (size_t)(g * GH + hb + hp * AT::NRP + rl) * DH + sub * AT::EPL;
#pragma unroll
        for (int i = 0; i < AT::EPL; ++i) qr[hp][i] = AT::POW2 ? qp[i] * scale : qp[i];  // 2^-k scale folded into q (exact)
    }
    float mr[AT::NHP], lr[AT::NHP], orun[AT::NHP][AT::EPL];
#pragma unroll
    for (int hp = 0; hp < AT::NHP; ++hp) {
        mr[hp] = -1e30f; lr[hp] = 0.f;
#pragma unroll
        for (int i = 0; i < AT::EPL; ++i) orun[hp][i] = 0.f;
    }
    for (int c = c0; c < nc; ++c) {
        const int t_base = c * AT::CH + wave * AT::TW;
#pragma unroll
        for (int i = 0; i < AT::NLD; ++i) {
            *reinterpret_cast<vec*>(&sk[wave][(size_t)(i * 64 + lane) * AT::EPL]) = kreg[i];
            *reinterpret_cast<vec*>(&sv[wave][(size_t)(i * 64 + lane) * AT::EPL]) = vreg[i];
        }
        if (c + 1 < nc) load_tiles(c + 1);
#pragma unroll
        for (int hp = 0; hp < AT::NHP; ++hp) {
            float sc[AT::TPG];
            float mc = -1e30f;
#pragma unroll
            for (int j = 0; j < AT::TPG; ++j) {
                const int tl = ts + j * AT::NTS;
                float kf[AT::EPL];
                WTr<WT>::unpack(*reinterpret_cast<const vec*>(&sk[wave][(size_t)tl * DH + sub * AT::EPL]), kf);
                float a = 0.f;
#pragma unroll
                for (int i = 0; i < AT::EPL; ++i) a = AT::POW2 ? fmaf(qr[hp][i], kf[i], a) : fmaf(qr[hp][i], kf[i] * scale, a);
                a = group_sum<AT::LPT>(a);
                sc[j] = (t_base + tl < T) ? a : -1e30f;
                mc = fmaxf(mc, sc[j]);
            }
            const float mn = fmaxf(mr[hp], mc), f = __expf(mr[hp] - mn);  // online softmax: the running (l, o) go to the new maximum first
            float l = lr[hp] * f, o[AT::EPL];
#pragma unroll
            for (int i = 0; i < AT::EPL; ++i) o[i] = orun[hp][i] * f;
#pragma unroll
            for (int j = 0; j < AT::TPG; ++j) {
                const int tl = ts + j * AT::NTS;
                const float p = (t_base + tl < T) ? __expf(sc[j] - mn) : 0.f;
                l += p;
                float vf[AT::EPL];
                WTr<WT>::unpack(*reinterpret_cast<const vec*>(&sv[wave][(size_t)tl * DH + sub * AT::EPL]), vf);
#pragma unroll
                for (int i = 0; i < AT::EPL; ++i) o[i] = fmaf(p, vf[i], o[i]);
            }
            mr[hp] = mn; lr[hp] = l;
#pragma unroll
            for (int i = 0; i < AT::EPL; ++i) orun[hp][i] = o[i];
        }
    }
#pragma unroll
    for (int hp = 0; hp < AT::NHP; ++hp) {
        float* dst = sp[wave][hp * AT::NRP + rl][ts];
#pragma unroll
        for (int i = 0; i < AT::EPL; ++i) dst[sub * AT::EPL + i] = orun[hp][i];
        if (sub == 0) { dst[DH] = mr[hp]; dst[DH + 1] = lr[hp]; }
    }
    __syncthreads();
    const int H = Hk * GH;
    for (int e = threadIdx.x; e < NREP * DH; e += AT::NW * 64) {
        const int r = e / DH, dd = e % DH;
        float mn, L, O;
        AT::merge(sp, r, dd, mn, L, O);
        if (PART) {
            float* dst = part_all + (((size_t)mrow * H + g * GH + hb + r) * n_chunks_max + blockIdx.z) * (DH + 2);
            dst[dd] = O;
            if (dd == 0) { dst[DH] = mn; dst[DH + 1] = L; }
        } else {
            bf16_t hi, lo;
            split_bf16(O / L, hi, lo);
            const int col = (g * GH + hb + r) * DH + dd;
            Ohi[frag_off(mrow, col, 0, H * DH)] = hi;
            Ohi[frag_off(mrow, col, 1, H * DH)] = lo;
        }
    }
}

// combine the per-chunk attention partials of M rows -> attn hi/lo bf16 [PF_M][H*DH] (input of the Wo GEMM)
template <int DH>
__global__ __launch_bounds__(256) void k_attn_combine(const float* __restrict__ part_all, int n_chunks_max, int chunk,
                                                      const SeqState* __restrict__ state, int pos_step, bf16_t* __restrict__ Ohi, int H) {
    const int m = blockIdx.x;
    const int T = row_pos(state, m, pos_step) + 1, nc = (T + chunk - 1) / chunk;
    const float* part = part_all + (size_t)m * H * n_chunks_max * (DH + 2);
    __shared__ float wl[32 * 128];
    for (int h = threadIdx.x; h < H; h += 256) {
        const float* p = part + (size_t)h * n_chunks_max * (DH + 2);
        float mn = -1e30f;
        for (int c = 0; c < nc; ++c) mn = fmaxf(mn, p[c * (DH + 2) + DH]);
        float L = 0.f;
        for (int c = 0; c < nc; ++c) L += p[c * (DH + 2) + DH + 1] * __expf(p[c * (DH + 2) + DH] - mn);
        const float inv = 1.f / L;
        for (int c = 0; c < nc; ++c) wl[h * 128 + c] = __expf(p[c * (DH + 2) + DH] - mn) * inv;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < H * DH; e += 256) {
        const int h = e / DH, dd = e % DH;
        const float* p = part + (size_t)h * n_chunks_max * (DH + 2) + dd;
        float O = 0.f;
        for (int c = 0; c < nc; ++c) O = fmaf(wl[h * 128 + c], p[c * (DH + 2)], O);
        bf16_t hi, lo;
        split_bf16(O, hi, lo);
        Ohi[frag_off(m, e, 0, H * DH)] = hi;
        Ohi[frag_off(m, e, 1, H * DH)] = lo;
    }
}

// ---- the fast decoder's rows: <= 8 cached tokens in ONE page, all H heads in one 256-thread block.  Steps shared by k_attn_small_rows and
// k_attn_small_rows_tbl; NEW_LDS (the _tbl kernel): position `pos` is the token the block has just appended -- its K / V come from the
// block's LDS copy (kn / vn: [Hk][DH] f32, the cached bf16-rounded values) instead of from the page.
// the V values of the thread's first (head, 4 dims) output item: requested with the K rows, not behind the score barrier (all 8 token
// slots of the page exist; slots >= T hold stale finite bf16 and are masked by t < T at use)
template <int DH>
__device__ __forceinline__ void small_rows_v_prefetch(const bf16_t* vb, int H, int n_rep, int tid, uint2 (&vpre)[8]) {
    const int e4 = tid * 4;
    if (e4 < H * DH) {
        const int h = e4 / DH, dd = e4 % DH;
#pragma unroll
        for (int t = 0; t < 8; ++t) vpre[t] = *reinterpret_cast<const uint2*>(vb + ((size_t)(h / n_rep) * KV_PAGE + t) * DH + dd);
    }
}
// sc[h * 8 + t] = q[h] . (k[t]^T * scale)  (dual_ar.rs:260): two threads per (head, token), DH / 2 dims each
template <int DH, bool NEW_LDS>
__device__ __forceinline__ void small_rows_scores(const float* q, const bf16_t* kb, int H, int n_rep, int tid, float* sc, const float* kn = nullptr,
                                                  int pos = 0) {
    const float scale = 1.0f / sqrtf((float)DH);
    constexpr int QD = DH / 2;
    for (int e1 = tid >> 1; e1 < H * 8; e1 += 128) {
        const int h = e1 >> 3, t = e1 & 7, sl = tid & 1;
        const bf16_t* kp = kb + ((size_t)(h / n_rep) * KV_PAGE + t) * DH + sl * QD;
        const float* qp = q + h * DH + sl * QD;
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < QD; i += 8) {
            float kf[8];
            WTr<bf16_t>::unpack(*reinterpret_cast<const u32x4*>(kp + i), kf);
            if (NEW_LDS && t == pos) {
#pragma unroll
                for (int j = 0; j < 8; ++j) kf[j] = kn[(h / n_rep) * DH + sl * QD + i + j];
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) acc = fmaf(qp[i + j], kf[j] * scale, acc);
        }
        acc += dpp_mov<DPP_XOR1>(acc);
        if (sl == 0) sc[e1] = acc;
    }
}
// (behind the score barrier) softmax over the row's T tokens . V, four output dims per thread, straight into the fragment-major hi/lo GEMM input
template <int DH, bool NEW_LDS>
__device__ __forceinline__ void small_rows_pv_store(const float* sc, const bf16_t* vb, const uint2 (&vpre)[8], int T, int H, int n_rep, int tid, int m,
                                                    bf16_t* Ohi, const float* vnS = nullptr, int pos = 0) {
    for (int e4 = tid * 4; e4 < H * DH; e4 += 1024) {
        const int h = e4 / DH, dd = e4 % DH;
        const bool firstit = e4 == tid * 4;
        float mx = -1e30f;
#pragma unroll
        for (int t = 0; t < 8; ++t) if (t < T) mx = fmaxf(mx, sc[h * 8 + t]);
        float L = 0.f, O[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 8; ++t)
            if (t < T) {
                const float p = __expf(sc[h * 8 + t] - mx);
                L += p;
                if (NEW_LDS && t == pos) {
                    const float* vn = vnS + (h / n_rep) * DH + dd;
                    O[0] = fmaf(p, vn[0], O[0]); O[1] = fmaf(p, vn[1], O[1]); O[2] = fmaf(p, vn[2], O[2]); O[3] = fmaf(p, vn[3], O[3]);
                } else {
                    const uint2 vv = firstit ? vpre[t] : *reinterpret_cast<const uint2*>(vb + ((size_t)(h / n_rep) * KV_PAGE + t) * DH + dd);
                    O[0] = fmaf(p, bf16_bits_to_f32((bf16_t)(vv.x & 0xFFFFu)), O[0]); O[1] = fmaf(p, bf16_bits_to_f32((bf16_t)(vv.x >> 16)), O[1]);
                    O[2] = fmaf(p, bf16_bits_to_f32((bf16_t)(vv.y & 0xFFFFu)), O[2]); O[3] = fmaf(p, bf16_bits_to_f32((bf16_t)(vv.y >> 16)), O[3]);
                }
            }
        const float inv = 1.f / L;
        const float a[4] = {O[0] * inv, O[1] * inv, O[2] * inv, O[3] * inv};
        store_frag4(Ohi, m, e4, H * DH, a);
    }
}

// Whole attention of one activation row over <= 8 cached tokens (the fast decoder in the batched row path): replaces k_attn_decode +
// k_attn_combine (two graph nodes) where one 8-token page is all there is.  The row's page is page_table[m * pt_stride] (single page),
// its length state->pos + 1 + m * pos_step <= 8.
template <int DH>
__global__ __launch_bounds__(256) void k_attn_small_rows(const float* __restrict__ q_all, KVView kv, const SeqState* __restrict__ state,
                                                         int H, int Hk, int pos_step, int pt_stride, bf16_t* __restrict__ Ohi, int identity_pages) {
    __shared__ float sc[32 * 8];
    const int m = blockIdx.x, tid = threadIdx.x;
    // identity_pages: row m's only page IS page m (the batched fast decoder's table) -- one dependent L2 round trip less in a node that is
    // nothing but a chain of them
    const int page = identity_pages ? m : kv.page_table[(size_t)m * pt_stride];
    const int n_rep = H / Hk;
    const float* q = q_all + (size_t)m * H * DH;
    const bf16_t* kb = reinterpret_cast<const bf16_t*>(kv.k) + (size_t)page * Hk * KV_PAGE * DH;
    const bf16_t* vb = reinterpret_cast<const bf16_t*>(kv.v) + (size_t)page * Hk * KV_PAGE * DH;
    uint2 vpre[8];
    small_rows_v_prefetch<DH>(vb, H, n_rep, tid, vpre);
    const int T = row_pos(state, m, pos_step) + 1;
    small_rows_scores<DH, false>(q, kb, H, n_rep, tid, sc);
    __syncthreads();
    small_rows_pv_store<DH, false>(sc, vb, vpre, T, H, n_rep, tid, m, Ohi);
}

// k_attn_small_rows for the FIRST fast layer of the codebook passes 1.. (round 6): that layer's input row is fast_embeddings[code] of the code the
// previous pass's sampler picked (static_batch.rs:236-241 / single_batch.rs:181-183), so attention_norm + Wqkv of it is row `code` of the qkv
// table the persistent fast decoder builds at load time (lm_persist.hip k_pf_qkv0_table: 1024 x 1280 f32, pre-RoPE).  The node takes q / k / v of
// the new token from that row instead of from a Wqkv GEMM node in front of it (7 nodes of a step disappear): RoPE at the pass's position, K / V
// appended to the row's page exactly as the GEMM epilogue would (bf16, EPI_QKV), and the new position's K / V used from LDS in their cached
// (bf16-rounded) form.  code = row_states[m].cur[code_slot] (written by the sampler node in front of this one).
template <int DH>
__global__ __launch_bounds__(256) void k_attn_small_rows_tbl(const float* __restrict__ tbl, const SeqState* __restrict__ row_states, int code_slot, KVView kv,
                                                             const SeqState* __restrict__ state, int H, int Hk, int pos_step, int pt_stride,
                                                             const float* __restrict__ cos_t, const float* __restrict__ sin_t, bf16_t* __restrict__ Ohi,
                                                             int identity_pages) {
    __shared__ float sc[32 * 8];
    __shared__ __attribute__((aligned(16))) float qS[32 * DH];
    __shared__ __attribute__((aligned(16))) float knS[4 * DH], vnS[4 * DH];
    const int m = blockIdx.x, tid = threadIdx.x;
    const int page = identity_pages ? m : kv.page_table[(size_t)m * pt_stride];
    const int n_rep = H / Hk;
    bf16_t* kb = reinterpret_cast<bf16_t*>(kv.k) + (size_t)page * Hk * KV_PAGE * DH;
    bf16_t* vb = reinterpret_cast<bf16_t*>(kv.v) + (size_t)page * Hk * KV_PAGE * DH;
    constexpr int QD = DH / 2;
    uint2 vpre[8];  // (the slot of the new position is stale here and replaced from vnS)
    small_rows_v_prefetch<DH>(vb, H, n_rep, tid, vpre);
    const int pos = row_pos(state, m, pos_step), T = pos + 1;
    const int rpos = pos + (pos_step < 0 ? state[m].rope_off : state->rope_off);
    const uint32_t code = row_states[m].cur[code_slot];
    const int qdim = H * DH, kdim = Hk * DH;
    const float* row = tbl + (size_t)code * (qdim + 2 * kdim);
    for (int i = tid; i < (qdim + 2 * kdim) / 2; i += 256) {
        const int r = 2 * i;
        const float2 ab = *reinterpret_cast<const float2*>(row + r);
        if (r < qdim + kdim) {  // rope_i (dual_ar.rs:246-247)
            const int j = (r % DH) / 2;
            const float cs = cos_t[(size_t)rpos * QD + j], sn = sin_t[(size_t)rpos * QD + j];
            const float o0 = ab.x * cs - ab.y * sn, o1 = ab.x * sn + ab.y * cs;
            if (r < qdim) { qS[r] = o0; qS[r + 1] = o1; }
            else {
                const int rk = r - qdim;
                const bf16_t b0 = WTr<bf16_t>::from_f32(o0), b1 = WTr<bf16_t>::from_f32(o1);
                *reinterpret_cast<uint32_t*>(kb + ((size_t)(rk / DH) * KV_PAGE + pos) * DH + rk % DH) = b0 | ((uint32_t)b1 << 16);
                knS[rk] = bf16_bits_to_f32(b0); knS[rk + 1] = bf16_bits_to_f32(b1);
            }
        } else {
            const int rv = r - qdim - kdim;
            const bf16_t b0 = WTr<bf16_t>::from_f32(ab.x), b1 = WTr<bf16_t>::from_f32(ab.y);
            *reinterpret_cast<uint32_t*>(vb + ((size_t)(rv / DH) * KV_PAGE + pos) * DH + rv % DH) = b0 | ((uint32_t)b1 << 16);
            vnS[rv] = bf16_bits_to_f32(b0); vnS[rv + 1] = bf16_bits_to_f32(b1);
        }
    }
    __syncthreads();
    small_rows_scores<DH, true>(qS, kb, H, n_rep, tid, sc, knS, pos);
    __syncthreads();
    small_rows_pv_store<DH, true>(sc, vb, vpre, T, H, n_rep, tid, m, Ohi, vnS, pos);
}

// ------------------------------------------------------------------------------------------------ prefill attention (MFMA)
// Causal flash attention for the rows of a prefill pass (consecutive tokens of ONE sequence, bf16 KV, head_dim 64): block =
// (query head, 16-row tile); its 4 waves split the sequence page-wise (wave w takes KV pages w, w+4, ...), each producing a
// local (max, sum, O) with a two-pass softmax over its own pages; one LDS merge, and the normalised result goes straight into
// the fragment-major hi/lo GEMM input (replaces k_attn_decode over (chunks x rows) blocks + k_attn_combine: 57 + 7 us per
// layer at 384 rows).  Per page (64 tokens = 4 MFMA token tiles) every operand load is in flight before the first MFMA.
//   S^T[token][row] = K_tile[16 x 64] . Q^T[64 x 16]   v_mfma_f32_16x16x32_bf16, A = K straight from the paged cache (one 16-B load
//                                                      per lane per 32 dims), B = the rows' q split bf16 hi + lo (held in VGPRs)
//   two-pass softmax: pass 1 only takes the column maxima; pass 2 recomputes S, p = exp(s - max) -- the S^T accumulator layout
//   (lane: row l&15, tokens (l>>4)*4..+3) IS the A-operand layout of the 16x16x16 MFMA, so
//   O[row][dim] += P[row][16 tokens] . V[16 tokens][dim]   v_mfma_f32_16x16x16_bf16, p split hi + lo, B = V gathered from the
//                                                      wave's private LDS copy of the tile (token-major -> 4 strided bf16)
// The softmax scale 2^-3 is folded into q (exact).  Rows >= M and tokens past a row's position are masked.
typedef short short4v __attribute__((ext_vector_type(4)));
// blockIdx.y = sequence of a group pass (rows [y * M, (y + 1) * M), page table y * pt_stride further on, first position state->pos +
// seq_states[y].pos when seq_states is set: members that join on a shared prefix start past it); one sequence: gridDim.y = 1.
__global__ __launch_bounds__(256) void k_attn_prefill_mfma(const float* __restrict__ q_all, KVView kv, const SeqState* __restrict__ state,
                                                           int M, int H, int Hk, bf16_t* __restrict__ Ohi, int pt_stride,
                                                           const SeqState* __restrict__ seq_states) {
    constexpr int DH = 64, VLD = DH + 8;
    __shared__ __attribute__((aligned(16))) bf16_t vt[4][KV_PAGE * VLD];
    __shared__ __attribute__((aligned(16))) float sm_o[4][16][DH + 4];
    __shared__ float sm_m[4][16], sm_l[4][16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = blockIdx.x % H, rt = blockIdx.x / H;  // query head, row tile
    const int g = h / (H / Hk);
    const int row0 = rt * 16, pos0 = seq_states ? seq_states[blockIdx.y].pos : state->pos;  // row m of this sequence sits at position pos0 + m
    const int mbase = (int)blockIdx.y * M;              // first activation row of this sequence
    const int* ptab = kv.page_table + (size_t)blockIdx.y * pt_stride;
    const int c16 = lane & 15, q4 = lane >> 4;
    // B operand of QK^T: q[row0 + c16][h][ks*32 + q4*8 ..+8], scaled, split hi/lo
    bf16x8 qh[2], ql[2];
    {
        const int m = min(row0 + c16, M - 1);
        const float* qp = q_all + ((size_t)(mbase + m) * H + h) * DH + q4 * 8;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const float4 a = *reinterpret_cast<const float4*>(qp + ks * 32), b = *reinterpret_cast<const float4*>(qp + ks * 32 + 4);
            const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
            uint32_t hw[4], lw[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                bf16_t h0, l0, h1, l1;
                split_bf16(v[2 * i] * 0.125f, h0, l0); split_bf16(v[2 * i + 1] * 0.125f, h1, l1);
                hw[i] = h0 | ((uint32_t)h1 << 16); lw[i] = l0 | ((uint32_t)l1 << 16);
            }
            u32x4 hv, lv; hv.x = hw[0]; hv.y = hw[1]; hv.z = hw[2]; hv.w = hw[3]; lv.x = lw[0]; lv.y = lw[1]; lv.z = lw[2]; lv.w = lw[3];
            qh[ks] = __builtin_bit_cast(bf16x8, hv); ql[ks] = __builtin_bit_cast(bf16x8, lv);
        }
    }
    const int my_pos = pos0 + row0 + c16;                       // last token this lane's row may see
    const int n_tok = pos0 + min(row0 + 15, M - 1) + 1;           // tokens the tile's LAST row needs
    const int n_groups = (n_tok + KV_PAGE - 1) / KV_PAGE;         // one group = one KV page = 4 token tiles of 16
    const bf16_t* kpool = reinterpret_cast<const bf16_t*>(kv.k);
    const bf16_t* vpool = reinterpret_cast<const bf16_t*>(kv.v);
    // S^T of the 4 token tiles of page `grp`: all 8 K loads (A operands, straight from the cache) are in flight together
    auto scores = [&](int grp, f32x4v (&sacc)[4]) {
        const int page = ptab[grp];
        const bf16_t* kp = kpool + ((size_t)(page * Hk + g) * KV_PAGE + c16) * DH + q4 * 8;
        u32x4 k0[4], k1[4];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            k0[tt] = *reinterpret_cast<const u32x4*>(kp + (size_t)tt * 16 * DH);
            k1[tt] = *reinterpret_cast<const u32x4*>(kp + (size_t)tt * 16 * DH + 32);
        }
        FS_ISSUE_FENCE();
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            f32x4v a = f32x4v{0.f, 0.f, 0.f, 0.f};
            a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, k0[tt]), qh[0], a, 0, 0, 0);
            a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, k0[tt]), ql[0], a, 0, 0, 0);
            a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, k1[tt]), qh[1], a, 0, 0, 0);
            a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, k1[tt]), ql[1], a, 0, 0, 0);
            const int t0 = grp * KV_PAGE + tt * 16;
#pragma unroll
            for (int i = 0; i < 4; ++i) if (t0 + q4 * 4 + i > my_pos) a[i] = -1e30f;  // causal mask (also hides stale rows of the page)
            sacc[tt] = a;
        }
    };
    // pass 1: column maxima
    float mx = -1e30f;
    for (int grp = wave; grp < n_groups; grp += 4) {
        f32x4v s4[4];
        scores(grp, s4);
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) mx = fmaxf(fmaxf(mx, fmaxf(s4[tt][0], s4[tt][1])), fmaxf(s4[tt][2], s4[tt][3]));
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    // pass 2: P . V
    f32x4v o[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) o[nt] = f32x4v{0.f, 0.f, 0.f, 0.f};
    float lsum = 0.f;
    bf16_t* myv = vt[wave];
    for (int grp = wave; grp < n_groups; grp += 4) {
        {   // stage the page's V (64 tokens x 64 dims) token-major into the wave's private LDS region: 8 x 16-B loads per lane
            const int page = ptab[grp];
            const bf16_t* vp = vpool + (size_t)(page * Hk + g) * KV_PAGE * DH;
            u32x4 vr[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) vr[j] = *reinterpret_cast<const u32x4*>(vp + (size_t)(j * 64 + lane) * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int e = j * 64 + lane, tk = e >> 3, d8 = (e & 7) * 8;
                *reinterpret_cast<u32x4*>(myv + tk * VLD + d8) = vr[j];
            }
        }
        f32x4v s4[4];
        scores(grp, s4);
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            uint32_t ph[2], pl[2];
            {
                bf16_t hb[4], lb[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float p = s4[tt][i] > -1e29f ? __expf(s4[tt][i] - mx) : 0.f;
                    lsum += p;
                    split_bf16(p, hb[i], lb[i]);
                }
                ph[0] = hb[0] | ((uint32_t)hb[1] << 16); ph[1] = hb[2] | ((uint32_t)hb[3] << 16);
                pl[0] = lb[0] | ((uint32_t)lb[1] << 16); pl[1] = lb[2] | ((uint32_t)lb[3] << 16);
            }
            uint2 phv, plv; phv.x = ph[0]; phv.y = ph[1]; plv.x = pl[0]; plv.y = pl[1];
            const short4v pa_h = __builtin_bit_cast(short4v, phv), pa_l = __builtin_bit_cast(short4v, plv);
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const bf16_t* vq = myv + (tt * 16 + q4 * 4) * VLD + nt * 16 + c16;  // V[token tt*16 + q4*4 + j][dim nt*16 + c16]
                uint2 bv;
                bv.x = vq[0] | ((uint32_t)vq[VLD] << 16);
                bv.y = vq[2 * VLD] | ((uint32_t)vq[3 * VLD] << 16);
                const short4v vb = __builtin_bit_cast(short4v, bv);
                o[nt] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(pa_h, vb, o[nt], 0, 0, 0);
                o[nt] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(pa_l, vb, o[nt], 0, 0, 0);
            }
        }
    }
    lsum += __shfl_xor(lsum, 16, 64);
    lsum += __shfl_xor(lsum, 32, 64);
    // merge the 4 page-splits: o[nt][i] = O_w[row q4*4 + i][dim nt*16 + c16]; max / sum live in column layout (row = c16)
    if (q4 == 0) { sm_m[wave][c16] = mx; sm_l[wave][c16] = lsum; }
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int i = 0; i < 4; ++i) sm_o[wave][q4 * 4 + i][nt * 16 + c16] = o[nt][i];
    __syncthreads();
    {
        const int r = threadIdx.x >> 4, d4 = (threadIdx.x & 15) * 4, m = row0 + r;
        if (m < M) {
            const float mg = fmaxf(fmaxf(sm_m[0][r], sm_m[1][r]), fmaxf(sm_m[2][r], sm_m[3][r]));
            float L = 0.f, O[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int w2 = 0; w2 < 4; ++w2) {
                const float cf = __expf(sm_m[w2][r] - mg);  // a split without pages has max -1e30, sum 0, O 0
                L = fmaf(sm_l[w2][r], cf, L);
                const float4 ov = *reinterpret_cast<const float4*>(&sm_o[w2][r][d4]);
                O[0] = fmaf(ov.x, cf, O[0]); O[1] = fmaf(ov.y, cf, O[1]); O[2] = fmaf(ov.z, cf, O[2]); O[3] = fmaf(ov.w, cf, O[3]);
            }
            const float inv = 1.f / L;
            const float a[4] = {O[0] * inv, O[1] * inv, O[2] * inv, O[3] * inv};
            store_frag4(Ohi, mbase + m, h * DH + d4, H * DH, a);
        }
    }
}

// ================================================================================================ launchers
#define FS_LAUNCH_CHECK() FS_HIP(hipGetLastError())

// model geometries (head_dim, query heads per kv head) the wave-tile kernels serve
static bool attn_geom_ok(const ModelDims& d) { return (d.Dh == 64 && (d.n_rep == 8 || d.n_rep == 2)) || (d.Dh == 32 && d.n_rep == 2); }
// (head_dim, query heads per block) -> f(integral constants DH, NREP); false: no such instantiation
template <typename F>
static bool dispatch_attn(int Dh, int nrep, F&& f) {
    using D64 = std::integral_constant<int, 64>;
    using D32 = std::integral_constant<int, 32>;
    if (Dh == 64 && nrep == 8) f(D64(), std::integral_constant<int, 8>());
    else if (Dh == 64 && nrep == 4) f(D64(), std::integral_constant<int, 4>());
    else if (Dh == 64 && nrep == 2) f(D64(), std::integral_constant<int, 2>());
    else if (Dh == 32 && nrep == 2) f(D32(), std::integral_constant<int, 2>());
    else return false;
    return true;
}

template <typename WT>
int AttnKernels<WT>::chunk() { return AttnGeom<KVT<WT>, 64>::NW * AttnGeom<KVT<WT>, 64>::TW; }  // same for every head_dim

template <typename WT>
int AttnKernels<WT>::tiles_per_block(const ModelDims& d, int nc_launch) {
    static const bool on = [] { const char* e = std::getenv("FISHRT_ATTN_SUPERCHUNK"); return !e || std::atoi(e) != 0; }();
    if (!on || std::is_same<WT, float>::value || d.Dh != 64 || d.n_rep != 8 || nc_launch <= 8) return 1;
    return (nc_launch + 7) / 8;
}

// ---- one place that decides the path: the launchers below dispatch through these plans and fs_selftest_attn reports their names
std::string AttnPlan::name() const {
    const std::string dh = std::to_string(DH), hs = hsplit > 1 ? "/hs" + std::to_string(hsplit) : std::string();
    switch (kind) {
    case DECODE: return std::string("decode/") + (f32_kv ? "f32/" : "bf16/") + dh + "/" + std::to_string(nrep) + hs;
    case DECODE_PART: return "decode/part/tpb" + std::to_string(tpb);
    case ROWS: return "rows/bf16/" + dh + "/" + std::to_string(nrep) + hs + (remap ? "/remap" : "");
    case ROWS_CHUNKED: return "rows/chunked/" + dh;
    case SMALL: return "small/" + dh + (ident ? "/ident" : "");
    case SMALL_TBL: return "small_tbl/" + dh;
    default: return group ? "prefill_mfma/group" : "prefill_mfma/seq";
    }
}

template <typename WT>
AttnPlan AttnKernels<WT>::decode_plan(const ModelDims& d, int nc_launch) {
    static const int hs8 = [] { const char* e = std::getenv("FISHRT_ATTN_HSPLIT"); return e ? std::atoi(e) : 4; }();  // tuning hook: 1, 2 or 4
    AttnPlan p;
    p.f32_kv = std::is_same<KVT<WT>, float>::value;
    p.DH = d.Dh;
    if (const int tpb = tiles_per_block(d, nc_launch); tpb > 1) {
        p.kind = AttnPlan::DECODE_PART; p.DH = 64; p.nrep = 2; p.hsplit = 4; p.tpb = tpb;
        p.gx = d.Hk * 4; p.gz = (nc_launch + tpb - 1) / tpb;
        return p;
    }
    // the 8 query heads of a Fish kv group go over hs blocks (bf16 KV only)
    const bool split = d.Dh == 64 && d.n_rep == 8 && !std::is_same<WT, float>::value;
    const int hs = split && (hs8 == 8 || hs8 == 4 || hs8 == 2) ? hs8 : 1;
    p.kind = AttnPlan::DECODE; p.hsplit = hs; p.nrep = d.n_rep / hs; p.gx = d.Hk * nc_launch * hs;
    if (hs != 8 && !(attn_geom_ok(d) && dispatch_attn(d.Dh, p.nrep, [](auto, auto) {})))
        throw Error("unsupported attention geometry (head_dim, n_rep) = (" + std::to_string(d.Dh) + ", " +
                    std::to_string(d.n_rep) + ")");
    return p;
}

template <typename WT>
void AttnKernels<WT>::decode(const ModelDims& d, const float* q, KVView kv, const SeqState* state, float* part,
                             int n_chunks_max, int nc_launch, hipStream_t st) {
    using KT = KVT<WT>;
    FS_REQUIRE(nc_launch >= 1 && nc_launch <= n_chunks_max, "bad attention chunk count");
    FS_REQUIRE(n_chunks_max <= 128, "attention supports at most 128 chunks per sequence");
    const AttnPlan p = decode_plan(d, nc_launch);
    if (p.kind == AttnPlan::DECODE_PART) {
        if constexpr (!std::is_same<WT, float>::value)
            hipLaunchKernelGGL((k_attn_rows<KT, 64, 2, true>), dim3(p.gx, 1, p.gz), dim3(AttnGeom<KT, 64>::NW * 64), 0,
                               st, q, kv, state, d.Hk, 0, 0, (bf16_t*)nullptr, p.hsplit, part, n_chunks_max, p.tpb);
        FS_LAUNCH_CHECK();
        return;
    }
    auto go = [&](auto dh, auto nr) {
        constexpr int DH = decltype(dh)::value, NREP = decltype(nr)::value;
        hipLaunchKernelGGL((k_attn_decode<KT, DH, NREP>), dim3(p.gx), dim3(AttnGeom<KT, DH>::NW * 64), 0, st, q, kv, state, part, d.Hk, n_chunks_max,
                           nc_launch, 0, 0, p.hsplit);
    };
    if (p.nrep == 1) go(std::integral_constant<int, 64>(), std::integral_constant<int, 1>());
    else dispatch_attn(p.DH, p.nrep, go);
    FS_LAUNCH_CHECK();
}

template <typename WT>
bool AttnKernels<WT>::rows_qkv0_ok(const ModelDims& d, const RowsCtx& c) {
    return c.small_attn && !c.attn_t1 && d.Dh == 64 && d.H <= 32 && d.Hk <= 4 && (c.stage_mask & 4u);
}

template <typename WT>
AttnPlan AttnKernels<WT>::rows_plan(const ModelDims& d, int M, const RowsCtx& c, bool tbl0) {
    if (std::is_same<WT, float>::value) throw Error("the MFMA row path needs bf16 or fp8 weights");
    AttnPlan p;
    p.DH = d.Dh; p.nrep = d.n_rep;
    if (tbl0) {
        p.kind = AttnPlan::SMALL_TBL; p.DH = 64; p.ident = c.identity_pages; p.gx = M;
    } else if (c.seq_rows > 0) {
        // group prefill: M = n_seq * seq_rows rows, sequence s starts at state->pos (or c.seq_states[s].pos); flash attention per sequence
        FS_REQUIRE(d.Dh == 64 && M % c.seq_rows == 0 && !c.no_flash, "group prefill needs head_dim 64 and whole sequences");
        p.kind = AttnPlan::PREFILL_MFMA; p.group = true; p.gx = d.H * ((c.seq_rows + 15) / 16); p.gy = M / c.seq_rows;
    } else if (c.pos_step == 1 && c.pt_stride == 0 && (c.stage_mask & 4u) && d.Dh == 64 && M > 1 && !c.no_flash) {
        // prefill: causal flash attention on the matrix cores, result straight into the Wo GEMM's input
        p.kind = AttnPlan::PREFILL_MFMA; p.gx = d.H * ((M + 15) / 16);
    } else if (c.small_attn && (c.stage_mask & 4u) && d.H <= 32 && (d.Dh == 64 || d.Dh == 32)) {
        // fast decoder: <= 8 tokens in one page -> one node instead of two
        p.kind = AttnPlan::SMALL; p.ident = c.identity_pages; p.gx = M;
    } else if (c.pos_step <= 0 && !c.chunked_attn && attn_geom_ok(d)) {
        // static-batch decode: one fused node per layer (whole KV prefix per (kv head, row) block)
        // few rows: split the 8 query heads of a kv group over two blocks (64 -> 128 blocks at 32 rows)
        const int hs = (d.Dh == 64 && d.n_rep == 8) ? (d.Hk * M <= 64 ? 4 : (d.Hk * M < 256 ? 2 : 1)) : 1;
        p.kind = AttnPlan::ROWS; p.hsplit = hs; p.nrep = d.n_rep / hs; p.gx = d.Hk * hs; p.gy = M;
        const int total = (int)(p.gx * p.gy), per_xcd = total / (8 * hs);  // k_attn_rows' own condition
        p.remap = hs > 1 && per_xcd * 8 * hs == total;
    } else {
        FS_REQUIRE(M <= c.part_rows, "more rows than the attention-partials buffer holds");
        p.kind = AttnPlan::ROWS_CHUNKED; p.gx = d.Hk * c.nc_launch; p.gy = M;
    }
    return p;
}

template <typename WT>
void AttnKernels<WT>::rows(const ModelDims& d, int M, const RowsCtx& c, KVView kv, bool tbl0, hipStream_t st) {
    const AttnPlan p = rows_plan(d, M, c, tbl0);
    if constexpr (!std::is_same<WT, float>::value) {
        using KT = KVT<WT>;  // bf16 KV cache for both weight types
        switch (p.kind) {
        case AttnPlan::SMALL_TBL:
            hipLaunchKernelGGL((k_attn_small_rows_tbl<64>), dim3(p.gx), dim3(256), 0, st, c.qkv0_tbl, c.row_states, c.code_slot, kv, c.state, d.H, d.Hk, c.pos_step,
                               c.pt_stride, c.cos_t, c.sin_t, c.A, (int)c.identity_pages);
            break;
        case AttnPlan::PREFILL_MFMA:
            if (!p.group)
                hipLaunchKernelGGL(k_attn_prefill_mfma, dim3(p.gx), dim3(256), 0, st, c.Q, kv, c.state, M, d.H, d.Hk, c.A, 0,
                                   (const SeqState*)nullptr);
            else if (c.stage_mask & 4u)
                hipLaunchKernelGGL(k_attn_prefill_mfma, dim3(p.gx, p.gy), dim3(256), 0, st, c.Q, kv, c.state,
                                   c.seq_rows, d.H, d.Hk, c.A, c.pt_stride, c.seq_states);
            break;
        case AttnPlan::SMALL:
            if (p.DH == 64)
                hipLaunchKernelGGL((k_attn_small_rows<64>), dim3(p.gx), dim3(256), 0, st, c.Q, kv, c.state, d.H, d.Hk, c.pos_step, c.pt_stride, c.A, (int)c.identity_pages);
            else
                hipLaunchKernelGGL((k_attn_small_rows<32>), dim3(p.gx), dim3(256), 0, st, c.Q, kv, c.state, d.H, d.Hk, c.pos_step, c.pt_stride, c.A, (int)c.identity_pages);
            break;
        case AttnPlan::ROWS:
            if (c.stage_mask & 4u)
                dispatch_attn(p.DH, p.nrep, [&](auto dh, auto nr) {
                    constexpr int DH = decltype(dh)::value, NREP = decltype(nr)::value;
                    hipLaunchKernelGGL((k_attn_rows<KT, DH, NREP>), dim3(p.gx, p.gy), dim3(AttnGeom<KT, DH>::NW * 64), 0, st, c.Q, kv, c.state, d.Hk, c.pos_step,
                                       c.pt_stride, c.A, p.hsplit);
                });
            break;
        default:
            if (c.stage_mask & 4u) {
                const bool ok = attn_geom_ok(d) && dispatch_attn(p.DH, p.nrep, [&](auto dh, auto nr) {
                    constexpr int DH = decltype(dh)::value, NREP = decltype(nr)::value;
                    hipLaunchKernelGGL((k_attn_decode<KT, DH, NREP>), dim3(p.gx, p.gy), dim3(AttnGeom<KT, DH>::NW * 64), 0, st, c.Q, kv, c.state, c.part,
                                       d.Hk, c.n_chunks_max, c.nc_launch, c.pos_step, c.pt_stride, 1);
                });
                if (!ok) throw Error("unsupported attention geometry");
            }
            if (!(c.stage_mask & 8u)) {}
            else if (d.Dh == 64)
                hipLaunchKernelGGL((k_attn_combine<64>), dim3(M), dim3(256), 0, st, c.part, c.n_chunks_max, chunk(), c.state, c.pos_step, c.A, d.H);
            else
                hipLaunchKernelGGL((k_attn_combine<32>), dim3(M), dim3(256), 0, st, c.part, c.n_chunks_max, chunk(), c.state, c.pos_step, c.A, d.H);
        }
        FS_LAUNCH_CHECK();
    }
}

template struct AttnKernels<bf16_t>;
template struct AttnKernels<float>;
template struct AttnKernels<fp8_t>;

// ================================================================================================ fs_selftest_attn (include/fishrt.h)
// ONE launcher call on caller data through AttnKernels / LmKernels::wo and nothing else.  Everything the launch writes lies between
// 256-element guards of 0xFF bytes, outputs are NaN-poisoned, and the whole case is validated on the host before the first device call.
__global__ void k_attn_expf_probe(const float* __restrict__ x, float* __restrict__ y, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = __expf(x[i]);
}

namespace {
constexpr size_t kAttnGuard = 256;
struct AttnDev {  // device buffer of n elements of es bytes between two guards, all 0xFF bytes at first
    void* p = nullptr;
    size_t n = 0, es = 4;
    void alloc(size_t n_, size_t es_, hipStream_t st) {
        n = n_; es = es_;
        FS_HIP(hipMalloc(&p, (n + 2 * kAttnGuard) * es));
        FS_HIP(hipMemsetAsync(p, 0xFF, (n + 2 * kAttnGuard) * es, st));
    }
    char* data() const { return (char*)p + kAttnGuard * es; }
    void up(const void* src, hipStream_t st) { FS_HIP(hipMemcpyAsync(data(), src, n * es, hipMemcpyHostToDevice, st)); }
    bool intact(hipStream_t st) const {
        if (!p) return true;
        std::vector<uint8_t> g(2 * kAttnGuard * es);
        FS_HIP(hipMemcpyAsync(g.data(), p, kAttnGuard * es, hipMemcpyDeviceToHost, st));
        FS_HIP(hipMemcpyAsync(g.data() + kAttnGuard * es, data() + n * es, kAttnGuard * es, hipMemcpyDeviceToHost, st));
        FS_HIP(hipStreamSynchronize(st));
        for (uint8_t b : g) if (b != 0xFF) return false;
        return true;
    }
    ~AttnDev() { if (p) (void)hipFree(p); }
};

// everything validate() derives from a case: the launch plan, its name, the output extent
struct AttnCaseInfo {
    ModelDims d{};
    AttnPlan plan;
    std::string name;
    int K = 0, CH = 0, Mcap = 0, n_seq = 0;
    bool f32_kv = false, use_part = false;
    size_t n_out = 0, n_pool = 0, n_part = 0;
    RowsCtx rc{};
};

template <typename WT>
void attn_validate(const fs_attn_case& c, AttnCaseInfo& I) {
    auto req = [](bool ok, const char* msg) { if (!ok) throw Error(std::string("attention self-test: ") + msg); };
    req(c.H >= 1 && c.H <= 32 && c.Hk >= 1 && c.Hk <= c.H && c.H % c.Hk == 0, "1 <= Hk <= H <= 32, H a multiple of Hk");
    ModelDims& d = I.d;
    d.H = c.H; d.Hk = c.Hk; d.Dh = c.Dh; d.n_rep = c.H / c.Hk; d.dim = c.dim; d.inter = 0; d.eps = 1e-6f;
    req(attn_geom_ok(d), "(head_dim, n_rep) must be (64, 8), (64, 2) or (32, 2)");
    req(c.dim == c.H * c.Dh, "dim must equal H * Dh");
    I.K = c.H * c.Dh;
    I.f32_kv = std::is_same<KVT<WT>, float>::value;
    I.CH = AttnKernels<WT>::chunk();
    req(c.n_pages >= 1 && c.n_pages <= 4096 && c.k && c.v, "1 <= n_pages <= 4096, k and v are required");
    I.n_pool = (size_t)c.n_pages * c.Hk * KV_PAGE * c.Dh;
    const bool wo_op = c.op == FS_ATTN_DECODE_WO || c.op == FS_ATTN_WO_FUSED;
    if (wo_op) req(c.wo && c.x && (c.dim == 128 || c.dim == 256 || c.dim == 1024) && c.H <= 16, "wo and x are required, dim in {128, 256, 1024}, H <= 16");
    if (c.op == FS_ATTN_WO_FUSED) {
        req(c.M == 1 && c.fused_T >= 1 && c.fused_T <= 8 && c.q, "fused wo: M == 1, 1 <= fused_T <= 8, q is required");
        I.name = "wo/fused/" + std::to_string(c.Dh);
        I.n_out = (size_t)c.dim;
        return;
    }
    // the page table: every entry a page of the pool, whichever slot a block may read
    req(c.page_table && c.pt_rows >= 1 && c.pt_len >= 1 && (long long)c.pt_rows * c.pt_len <= (1 << 20) && c.pt_stride >= 0, "page_table [pt_rows][pt_len] is required");
    const long long n_tab = (long long)c.pt_rows * c.pt_len;
    for (long long i = 0; i < n_tab; ++i) req(c.page_table[i] >= 0 && c.page_table[i] < c.n_pages, "a page id is outside the pool");
    // table row r (at r * pt_stride) is read at slots [0, n): inside the table, and inside its own pt_len
    auto need = [&](int r, long long n) {
        req(n <= c.pt_len && (long long)r * c.pt_stride + n <= n_tab, "a launched block would read a page-table slot outside the table (T <= pt_len * 64)");
    };
    auto pos_ok = [&](long long p) { req(p >= 0 && p < (1 << 20), "a row position is outside [0, 2^20)"); };
    req(c.q, "q is required");
    if (c.op == FS_ATTN_DECODE || c.op == FS_ATTN_DECODE_WO) {
        req(c.M == 1 && c.pos_step == 0, "decode: M == 1, pos_step 0");
        pos_ok(c.pos);
        req(c.nc_launch >= 1 && c.nc_launch <= c.n_chunks_max && c.n_chunks_max <= 128, "1 <= nc_launch <= n_chunks_max <= 128");
        const long long T = (long long)c.pos + 1;
        req(T <= (long long)c.nc_launch * I.CH, "the launched chunks do not cover the length");
        I.plan = AttnKernels<WT>::decode_plan(d, c.nc_launch);
        // k_attn_decode reads the slot of every launched chunk, whatever the length; the super-chunk kernel those below the length
        need(0, I.plan.kind == AttnPlan::DECODE ? (long long)c.nc_launch * I.CH / KV_PAGE : (T + I.CH - 1) / I.CH * I.CH / KV_PAGE);
        I.name = I.plan.name();
        I.n_part = (size_t)c.H * c.n_chunks_max * (c.Dh + 2);
        I.use_part = true;
        if (c.op == FS_ATTN_DECODE_WO) {
            const int tpb = AttnKernels<WT>::tiles_per_block(d, c.nc_launch);
            I.name += (c.nc_launch + tpb - 1) / tpb <= 8 ? "+wo/reg" : "+wo/lds";
            I.n_out = (size_t)c.dim;
        } else I.n_out = I.n_part;
        return;
    }
    req(c.op == FS_ATTN_ROWS, "unknown op");
    req(c.M >= 1 && c.M <= 512, "rows: 1 <= M <= 512");
    req(c.pos_step == 1 || c.pos_step == 0 || c.pos_step == -1, "pos_step is 1, 0 or -1");
    req(c.pos_step >= 0 || c.row_pos, "pos_step < 0 needs row_pos");
    req(c.seq_rows >= 0 && (c.seq_rows == 0 || (c.pos_step == 1 && c.M % c.seq_rows == 0)), "group prefill: pos_step 1, M a multiple of seq_rows");
    I.Mcap = (c.M + 31) / 32 * 32;
    I.n_seq = c.seq_rows > 0 ? c.M / c.seq_rows : 0;
    RowsCtx& rc = I.rc;
    rc.Mcap = I.Mcap; rc.part_rows = c.part_rows; rc.n_chunks_max = c.n_chunks_max; rc.nc_launch = c.nc_launch;
    rc.pos_step = c.pos_step; rc.pt_stride = c.pt_stride; rc.seq_rows = c.seq_rows;
    rc.no_flash = c.no_flash != 0; rc.chunked_attn = c.chunked_attn != 0; rc.small_attn = c.small_attn != 0; rc.identity_pages = c.identity_pages != 0;
    rc.code_slot = c.code_slot;
    if (c.tbl0) req(AttnKernels<WT>::rows_qkv0_ok(d, rc), "tbl0 needs small_attn, head_dim 64, H <= 32, Hk <= 4");
    I.plan = AttnKernels<WT>::rows_plan(d, c.M, rc, c.tbl0 != 0);
    I.name = I.plan.name();
    auto T_of = [&](int m) -> long long {
        if (c.seq_rows > 0) return (long long)(c.seq_pos ? c.seq_pos[m / c.seq_rows] : c.pos) + m % c.seq_rows + 1;
        return (c.pos_step < 0 ? (long long)c.row_pos[m] : (long long)c.pos + (long long)m * c.pos_step) + 1;
    };
    for (int m = 0; m < c.M; ++m) pos_ok(T_of(m) - 1);
    if (c.small_attn) for (int m = 0; m < c.M; ++m) req(T_of(m) <= 8, "small_attn: every row attends over <= 8 tokens");
    switch (I.plan.kind) {
    case AttnPlan::SMALL_TBL:
    case AttnPlan::SMALL:
        req(c.small_attn, "the one-page kernels need small_attn");
        for (int m = 0; m < c.M; ++m) {
            if (c.identity_pages) req(m < c.n_pages, "identity pages: row m uses page m");
            else need(m, 1);
        }
        if (I.plan.kind == AttnPlan::SMALL_TBL) {
            req(c.tbl && c.codes && c.cos_t && c.sin_t && c.tbl_rows >= 1 && c.tbl_rows <= 4096 && c.rope_rows >= 1 && c.rope_rows <= (1 << 16),
                "tbl0 needs tbl, codes, cos_t, sin_t, 1 <= tbl_rows <= 4096, 1 <= rope_rows <= 2^16");
            req(c.code_slot >= 0 && c.code_slot < 16, "code_slot is one of the 16 cur[] cells");
            std::vector<char> used((size_t)c.n_pages, 0);
            for (int m = 0; m < c.M; ++m) {
                req(c.codes[m] < (uint32_t)c.tbl_rows, "a code is outside the qkv table");
                const long long rp = T_of(m) - 1 + c.rope_off;
                req(rp >= 0 && rp < c.rope_rows, "a RoPE row is outside the cos / sin tables");
                const int page = c.identity_pages ? m : c.page_table[(size_t)m * c.pt_stride];
                req(!used[(size_t)page], "tbl0: two rows append to the same page");
                used[(size_t)page] = 1;
            }
        }
        break;
    case AttnPlan::PREFILL_MFMA:
        if (I.plan.group) for (int s = 0; s < I.n_seq; ++s) need(s, (T_of(s * c.seq_rows + c.seq_rows - 1) + KV_PAGE - 1) / KV_PAGE);
        else need(0, (T_of(c.M - 1) + KV_PAGE - 1) / KV_PAGE);
        break;
    case AttnPlan::ROWS:
        for (int m = 0; m < c.M; ++m) need(m, (T_of(m) + I.CH - 1) / I.CH * I.CH / KV_PAGE);
        break;
    default:  // k_attn_decode over (chunks x rows) + k_attn_combine
        req(c.nc_launch >= 1 && c.nc_launch <= c.n_chunks_max && c.n_chunks_max <= 128 && c.part_rows >= c.M && c.part_rows <= 512,
            "chunked rows: 1 <= nc_launch <= n_chunks_max <= 128, M <= part_rows <= 512");
        for (int m = 0; m < c.M; ++m) {
            req(T_of(m) <= (long long)c.nc_launch * I.CH, "the launched chunks do not cover a row's length");
            need(m, (long long)c.nc_launch * I.CH / KV_PAGE);
        }
        I.use_part = true;
        I.n_part = (size_t)c.part_rows * c.H * c.n_chunks_max * (c.Dh + 2);
    }
    I.n_out = (size_t)2 * I.Mcap * I.K;
}

template <typename WT>
void attn_selftest_run(int device, const fs_attn_case& c, const AttnCaseInfo& I, float* out, float* k_out, float* v_out, int* guard_ok) {
    using KT = KVT<WT>;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) throw Error("no HIP device visible: libfishrt has no CPU fallback (MI355X / gfx950 required)");
    FS_REQUIRE(device >= 0 && device < ndev, "device_id out of range");
    FS_HIP(hipSetDevice(device));
    hipStream_t st = nullptr;
    FS_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    struct StreamGuard { hipStream_t s; ~StreamGuard() { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } } sg{st};
    const ModelDims& d = I.d;
    // pools in the KV type
    AttnDev dk, dv, dtab, dq, dpart, dx, dA, dwo, dso, dstate, drstate, dsstate, dtbl, dcos, dsin;
    std::vector<KT> hk(I.n_pool), hv(I.n_pool);
    for (size_t i = 0; i < I.n_pool; ++i) {
        if constexpr (std::is_same<KT, float>::value) { hk[i] = c.k[i]; hv[i] = c.v[i]; }
        else { hk[i] = f32_to_bf16_host(c.k[i]); hv[i] = f32_to_bf16_host(c.v[i]); }
    }
    dk.alloc(I.n_pool, sizeof(KT), st); dk.up(hk.data(), st);
    dv.alloc(I.n_pool, sizeof(KT), st); dv.up(hv.data(), st);
    if (c.page_table) { dtab.alloc((size_t)c.pt_rows * c.pt_len, 4, st); dtab.up(c.page_table, st); }
    dq.alloc((size_t)c.M * I.K, 4, st); dq.up(c.q, st);
    KVView kv{dk.data(), dv.data(), c.page_table ? (const int*)dtab.data() : nullptr};
    // generator states: positions, RoPE offset, the rows' codes
    const int n_state = std::max(c.M, 1);
    std::vector<SeqState> hs((size_t)n_state), hseq((size_t)std::max(I.n_seq, 1));
    for (auto& s : hs) std::memset(&s, 0, sizeof(SeqState));
    for (auto& s : hseq) std::memset(&s, 0, sizeof(SeqState));
    for (int m = 0; m < n_state; ++m) {
        hs[(size_t)m].pos = (c.op == FS_ATTN_ROWS && c.pos_step < 0) ? c.row_pos[m] : c.pos;
        hs[(size_t)m].rope_off = c.rope_off;
        if (c.op == FS_ATTN_ROWS && c.tbl0) hs[(size_t)m].cur[c.code_slot] = c.codes[m];
    }
    for (int s = 0; s < I.n_seq; ++s) hseq[(size_t)s].pos = c.seq_pos ? c.seq_pos[s] : c.pos;
    dstate.alloc(hs.size() * sizeof(SeqState), 1, st); dstate.up(hs.data(), st);
    const SeqState* state = (const SeqState*)dstate.data();
    std::vector<float> host_out;
    std::vector<uint16_t> host_A;
    if (I.use_part) {
        dpart.alloc(I.n_part, 4, st);
        if (c.op == FS_ATTN_DECODE_WO) {  // stale partials instead of poison: the merge has to mask them
            std::vector<float> fill(I.n_part, c.stale_part);
            dpart.up(fill.data(), st);
            FS_HIP(hipStreamSynchronize(st));
        }
    }
    LayerW w{};
    if (c.op == FS_ATTN_DECODE_WO || c.op == FS_ATTN_WO_FUSED) {
        const size_t nw = (size_t)c.dim * c.dim;
        std::vector<WT> hw(nw);
        for (size_t i = 0; i < nw; ++i) {
            if constexpr (std::is_same<WT, float>::value) hw[i] = c.wo[i];
            else if constexpr (std::is_same<WT, bf16_t>::value) hw[i] = f32_to_bf16_host(c.wo[i]);
            else hw[i] = fp8_t{f32_to_e4m3(c.wo[i])};
        }
        dwo.alloc(nw, sizeof(WT), st); dwo.up(hw.data(), st);
        w.wo = dwo.data();
        if constexpr (std::is_same<WT, fp8_t>::value) {
            std::vector<float> ones((size_t)c.dim, 1.0f);
            dso.alloc((size_t)c.dim, 4, st); dso.up(ones.data(), st);
            FS_HIP(hipStreamSynchronize(st));
            w.s_o = (const float*)dso.data();
        }
        dx.alloc((size_t)c.dim, 4, st); dx.up(c.x, st);
        FS_HIP(hipStreamSynchronize(st));  // hw goes out of scope below
    }
    switch (c.op) {
    case FS_ATTN_DECODE:
        AttnKernels<WT>::decode(d, (const float*)dq.data(), kv, state, (float*)dpart.data(), c.n_chunks_max, c.nc_launch, st);
        break;
    case FS_ATTN_DECODE_WO:
        AttnKernels<WT>::decode(d, (const float*)dq.data(), kv, state, (float*)dpart.data(), c.n_chunks_max, c.nc_launch, st);
        LmKernels<WT>::wo(d, (const float*)dpart.data(), c.n_chunks_max, c.nc_launch, state, (const float*)dq.data(), kv, 0, w, (float*)dx.data(), st);
        break;
    case FS_ATTN_WO_FUSED:
        LmKernels<WT>::wo(d, nullptr, 1, 1, state, (const float*)dq.data(), kv, c.fused_T, w, (float*)dx.data(), st);
        break;
    default: {
        RowsCtx rc = I.rc;
        dA.alloc((size_t)2 * I.Mcap * I.K, 2, st);
        rc.Q = (float*)dq.data(); rc.A = (uint16_t*)dA.data(); rc.part = I.use_part ? (float*)dpart.data() : nullptr;
        rc.state = state;
        if (I.n_seq > 0 && c.seq_pos) {
            dsstate.alloc(hseq.size() * sizeof(SeqState), 1, st); dsstate.up(hseq.data(), st);
            rc.seq_states = (const SeqState*)dsstate.data();
        }
        if (c.tbl0) {
            const size_t row = (size_t)(c.H + 2 * c.Hk) * c.Dh;
            dtbl.alloc((size_t)c.tbl_rows * row, 4, st); dtbl.up(c.tbl, st);
            dcos.alloc((size_t)c.rope_rows * (c.Dh / 2), 4, st); dcos.up(c.cos_t, st);
            dsin.alloc((size_t)c.rope_rows * (c.Dh / 2), 4, st); dsin.up(c.sin_t, st);
            rc.qkv0_tbl = (const float*)dtbl.data(); rc.cos_t = (const float*)dcos.data(); rc.sin_t = (const float*)dsin.data();
            rc.row_states = state;
        }
        AttnKernels<WT>::rows(d, c.M, rc, kv, c.tbl0 != 0, st);
    }
    }
    // results
    if (c.op == FS_ATTN_ROWS) {
        host_A.resize((size_t)2 * I.Mcap * I.K);
        FS_HIP(hipMemcpyAsync(host_A.data(), dA.data(), host_A.size() * 2, hipMemcpyDeviceToHost, st));
    } else {
        host_out.resize(I.n_out);
        FS_HIP(hipMemcpyAsync(host_out.data(), c.op == FS_ATTN_DECODE ? dpart.data() : dx.data(), I.n_out * 4, hipMemcpyDeviceToHost, st));
    }
    FS_HIP(hipMemcpyAsync(hk.data(), dk.data(), I.n_pool * sizeof(KT), hipMemcpyDeviceToHost, st));
    FS_HIP(hipMemcpyAsync(hv.data(), dv.data(), I.n_pool * sizeof(KT), hipMemcpyDeviceToHost, st));
    FS_HIP(hipStreamSynchronize(st));
    bool ok = true;
    for (const AttnDev* b : {&dk, &dv, &dpart, &dx, &dA}) ok = b->intact(st) && ok;
    *guard_ok = ok ? 1 : 0;
    if (c.op == FS_ATTN_ROWS) {
        const size_t plane = (size_t)I.Mcap * I.K;
        for (int m = 0; m < I.Mcap; ++m)
            for (int k = 0; k < I.K; ++k) {
                out[(size_t)m * I.K + k] = bf16_to_f32_host(host_A[frag_off(m, k, 0, I.K)]);
                out[plane + (size_t)m * I.K + k] = bf16_to_f32_host(host_A[frag_off(m, k, 1, I.K)]);
            }
    } else std::memcpy(out, host_out.data(), I.n_out * 4);
    for (size_t i = 0; i < I.n_pool; ++i) {
        if constexpr (std::is_same<KT, float>::value) { if (k_out) k_out[i] = hk[i]; if (v_out) v_out[i] = hv[i]; }
        else { if (k_out) k_out[i] = bf16_to_f32_host(hk[i]); if (v_out) v_out[i] = bf16_to_f32_host(hv[i]); }
    }
}

void attn_expf_probe(int device, const fs_attn_case& c, float* out) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) throw Error("no HIP device visible: libfishrt has no CPU fallback (MI355X / gfx950 required)");
    FS_REQUIRE(device >= 0 && device < ndev, "device_id out of range");
    FS_HIP(hipSetDevice(device));
    hipStream_t st = nullptr;
    FS_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    struct StreamGuard { hipStream_t s; ~StreamGuard() { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } } sg{st};
    AttnDev dx, dy;
    dx.alloc((size_t)c.n_expf, 4, st); dx.up(c.expf_x, st);
    dy.alloc((size_t)c.n_expf, 4, st);
    hipLaunchKernelGGL(k_attn_expf_probe, dim3((c.n_expf + 255) / 256), dim3(256), 0, st, (const float*)dx.data(), (float*)dy.data(), c.n_expf);
    FS_LAUNCH_CHECK();
    FS_HIP(hipMemcpyAsync(out, dy.data(), (size_t)c.n_expf * 4, hipMemcpyDeviceToHost, st));
    FS_HIP(hipStreamSynchronize(st));
}
}  // namespace

void attn_selftest(int device, const fs_attn_case& c, float* out, size_t out_cap, size_t* n_out, float* k_out, float* v_out, char* variant_out,
                   size_t variant_cap, int* guard_ok) {
    FS_REQUIRE(c.op >= FS_ATTN_DECODE && c.op <= FS_ATTN_EXPF, "attention self-test: unknown op");
    if (c.op == FS_ATTN_EXPF) {
        FS_REQUIRE(c.n_expf >= 1 && c.n_expf <= (1 << 22) && c.expf_x, "attention self-test: 1 <= n_expf <= 2^22, expf_x is required");
        std::snprintf(variant_out, variant_cap, "expf");
        if (c.plan_only) return;
        FS_REQUIRE(out && out_cap >= (size_t)c.n_expf, "attention self-test: out capacity too small");
        attn_expf_probe(device, c, out);
        *n_out = (size_t)c.n_expf; *guard_ok = 1;
        return;
    }
    FS_REQUIRE(c.wt >= FS_ATTN_WT_F32 && c.wt <= FS_ATTN_WT_FP8, "attention self-test: unknown weight type");
    AttnCaseInfo I;
    if (c.wt == FS_ATTN_WT_F32) attn_validate<float>(c, I);
    else if (c.wt == FS_ATTN_WT_BF16) attn_validate<bf16_t>(c, I);
    else attn_validate<fp8_t>(c, I);
    std::snprintf(variant_out, variant_cap, "%s", I.name.c_str());
    if (c.plan_only) return;
    FS_REQUIRE(out && out_cap >= I.n_out, "attention self-test: out capacity too small");
    if (c.wt == FS_ATTN_WT_F32) attn_selftest_run<float>(device, c, I, out, k_out, v_out, guard_ok);
    else if (c.wt == FS_ATTN_WT_BF16) attn_selftest_run<bf16_t>(device, c, I, out, k_out, v_out, guard_ok);
    else attn_selftest_run<fp8_t>(device, c, I, out, k_out, v_out, guard_ok);
    *n_out = I.n_out;
}

}  // namespace fs
