// On-device samplers of the Dual-AR transformer for gfx950 (MI355X): the single-sequence samplers (k_sample_slow / k_sample_fast), the
// static-batch row samplers (k_sample_*_rows, and _rows_par on the block-parallel sampler of lm_bsample_dev.h), the per-slot session
// samplers (k_sample_*_slots), the decision capture of the row path and the sampler test hook.  Launch interface: lm_kernels.h.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/fishrt.h"
#include "fs_common.h"
#include "lm_kernels.h"
#include "lm_dev.h"

namespace fs {

// ------------------------------------------------------------------------------------------------ sampling
#if defined(FS_SAMPLE_DBG) && FS_SAMPLE_DBG == 9
__device__ unsigned long long g_dbg_ts[64];
#define FS_TS(i) do { if (threadIdx.x == 0) g_dbg_ts[i] = clock64(); } while (0)
void fs_dbg_read_ts(unsigned long long* out) { (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_dbg_ts), sizeof(unsigned long long) * 64); }
#else
#define FS_TS(i) do {} while (0)
#endif
#include "lm_bsample_dev.h"  // chacha12_word + the block-parallel sampler

// ---- single-thread sequential f32 chains over an LDS array (the sampler's sums must not depend on a reduction order, so
// they are evaluated exactly as the scalar reference does: one running f32 sum in ascending order).  A naive loop pays the
// LDS latency (~100 cycles) per element; these helpers fetch 32 values per step with eight independent 16-byte reads and
// then run the dependent adds out of registers (~10 cycles per element).  `a` must be 16-byte aligned and readable up to
// the next multiple of 32; entries >= n count as +0.0 (x + 0.0f == x exactly for the non-negative sums used here).
__device__ __forceinline__ void lds_fetch32(const float* a, int j, int n, float (&v)[32]) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const float4 t = *reinterpret_cast<const float4*>(a + j + 4 * q);
        v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
    }
    if (j + 32 > n) {  // tail chunk only: the full chunks run without per-element masking
#pragma unroll
        for (int e = 0; e < 32; ++e) if (j + e >= n) v[e] = 0.f;
    }
}
__device__ float seq_sum(const float* a, int n) {
    float sum = 0.f;
    for (int j = 0; j < n; j += 32) {
        float v[32];
        lds_fetch32(a, j, n, v);
#pragma unroll
        for (int e = 0; e < 32; ++e) sum += v[e];
    }
    return sum;
}
// same chain, also leaving the running sums in cum[0..n) (cum may be written up to the next multiple of 32)
__device__ float seq_sum_prefix(const float* a, int n, float* cum) {
    float sum = 0.f;
    for (int j = 0; j < n; j += 32) {
        float v[32];
        lds_fetch32(a, j, n, v);
#pragma unroll
        for (int e = 0; e < 32; ++e) { sum += v[e]; v[e] = sum; }
#pragma unroll
        for (int q = 0; q < 8; ++q) *reinterpret_cast<float4*>(cum + j + 4 * q) = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
    }
    return sum;
}
// top-p cut over probabilities sorted in descending order: the first rank r at which the running sum of sp[0..r) has
// reached top_p (sampling/mod.rs:117-126); n when it never does
__device__ int seq_topp_cut(const float* sp, int n, float top_p) {
    float cumsum = 0.f;
    for (int j = 0; j < n; j += 32) {
        float v[32];
        lds_fetch32(sp, j, n, v);
#pragma unroll
        for (int e = 0; e < 32; ++e) {
            if (j + e >= n) return n;
            if (cumsum >= top_p) return j + e;
            cumsum += v[e];
        }
    }
    return n;
}

constexpr int SAMPLE_THREADS = 1024;
constexpr int SAMPLE_MAXN = 4096;  // candidates handled by the sampler (audio range 2037, codebook 1024)

// WeightedIndex::new + sample over the contiguous weights w[0..cnt) (ascending token index; zero weights do not move the
// cumulative sum): rand 0.8.5 UniformFloat<f32>::sample_single over [0, total) + partition_point on the cumulative weights.
// Block-wide: thread 0 runs the one sequential f32 chain (leaving the running sums in `cum`), then every thread tests its
// own entries -- the pick is the FIRST non-zero entry whose inclusive running sum exceeds the draw, else the last non-zero
// entry.  `word` = the StdRng word for this draw (computed off the critical path by a side wave).  All threads must call.
// NT = threads of the calling block; *drew (every thread) = 1 iff the draw consumed `word` (WeightedIndex needs a positive total).
template <int NT>
__device__ int block_weighted_pick_nt(const float* w, int cnt, float* cum, uint32_t word, int* drew) {
    __shared__ float s_chosen;
    __shared__ int s_first, s_last, s_any;
    const int tid = threadIdx.x;
    if (tid == 0) {
        const float total = seq_sum_prefix(w, cnt, cum);
        s_any = total > 0.f ? 1 : 0;
        if (total > 0.f) {
            const float max_rand = __uint_as_float((0xFFFFFFFFu >> 9) | (127u << 23)) - 1.0f;
            float scale = total;
            while (scale * max_rand + 0.f >= total) scale = __uint_as_float(__float_as_uint(scale) - 1u);
            s_chosen = (__uint_as_float((word >> 9) | (127u << 23)) - 1.0f) * scale + 0.f;
        }
        s_first = 0x7FFFFFFF; s_last = -1;
    }
    __syncthreads();
    if (s_any) {
        const float chosen = s_chosen;
        int first = 0x7FFFFFFF, last = -1;
        for (int j = tid; j < cnt; j += NT) {
            if (w[j] == 0.f) continue;
            last = j;
            if (cum[j] > chosen && first == 0x7FFFFFFF) first = j;
        }
        if (first != 0x7FFFFFFF) atomicMin(&s_first, first);
        if (last >= 0) atomicMax(&s_last, last);
    }
    __syncthreads();
    const int res = !s_any ? 0 : (s_first != 0x7FFFFFFF ? s_first : s_last);
    *drew = s_any;
    __syncthreads();
    return res;
}
__device__ int block_weighted_pick(const float* w, int cnt, float* cum, RngState* rng, uint32_t word) {
    int drew = 0;
    const int res = block_weighted_pick_nt<SAMPLE_THREADS>(w, cnt, cum, word, &drew);
    if (threadIdx.x == 0 && drew) rng->consumed += 1;
    return res;
}

// ---- top-k (k <= 256) sampling of n <= 64 * EPL candidates by ONE wave, no block barrier inside (a barrier phase of a
// 16-wave block costs ~0.4 us on this chip and the sort-based version needed ~40 of them; measured 36 us per call).  Lane l
// owns the EPL consecutive candidates l*EPL .. l*EPL+EPL-1 in registers (ascending index == lane-major order):
//   1. softmax in registers (DPP max, f64 sum);
//   2. the k-th largest probability T by radix select on its bit pattern (8 + 8 + 8 + 6 bits, LDS histogram per pass);
//   3. keep p > T and the first k - #{p > T} ties in index order (v_mbcnt prefix counts), compact the kept set into the
//      contiguous index-ordered arrays kp / ki and 64-bit keys (p bits : 255 - position);
//   4. sort the <= 256 keys descending in registers (4 per lane: in-lane swaps, DPP for lane^1 / lane^2, ds_bpermute above);
//   5. lane 0 runs the ascending-index sum of the kept probabilities while lane 1 runs the descending-order top-p cumsum --
//      two sequential f32 chains in one instruction stream; entries ranked at or after the cut are zeroed.
// wave_topk_select leaves kp / ki in LDS; wave_pick then draws from them.  Decisions are identical to the sorted version
// (top-k ties: lower index first; sequential f32 sums in the reference's order).
// (implementation note, measured with tools/ubench_valu.hip: a lone wave retires a dependent VALU op every ~6 cycles, but a
// VALU result consumed by the SCALAR unit -- v_cmp -> s_bcnt1, ballot -> s_and -- costs ~32 cycles per hop, and a dependent
// ds_bpermute ~70.  Hence: counts and prefix sums stay in vector registers (v_addc, DPP scans), compare-exchanges are
// written as max / min selects, and the sequential sums are pure add chains whose comparisons happen afterwards in parallel.)
// inclusive prefix sum over the 64 lanes (DPP row shifts + row broadcasts, no LDS, no scalar hop)
__device__ __forceinline__ int wave_incl_scan(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, false);  // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, false);  // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, false);  // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, false);  // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false);  // row_bcast:15 -> rows 1, 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false);  // row_bcast:31 -> rows 2, 3
    return v;
}
__device__ __forceinline__ unsigned long long dpp_xor_lane_u64(unsigned long long v, int which /*1: lane^1, 2: lane^2*/) {
    uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
    if (which == 1) { lo = __builtin_amdgcn_mov_dpp(lo, DPP_XOR1, 0xF, 0xF, false); hi = __builtin_amdgcn_mov_dpp(hi, DPP_XOR1, 0xF, 0xF, false); }
    else { lo = __builtin_amdgcn_mov_dpp(lo, DPP_XOR2, 0xF, 0xF, false); hi = __builtin_amdgcn_mov_dpp(hi, DPP_XOR2, 0xF, 0xF, false); }
    return ((unsigned long long)hi << 32) | lo;
}

template <int EPL>
__device__ void wave_topk_select(const float* lg, int n, int kk, float inv_t, float top_p, float* kp, int* ki, float* sp,
                                 unsigned long long* keyb, float* cumsp, bool batch, double top_p64) {
    const int lane = threadIdx.x & 63;
    const int base = lane * EPL;
    uint32_t u[EPL];
    {
        float v[EPL];
        float mx = -INFINITY;
#pragma unroll
        for (int q = 0; q < EPL / 4; ++q) {
            const float4 t = *reinterpret_cast<const float4*>(lg + base + 4 * q);
            v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
        }
#pragma unroll
        for (int s = 0; s < EPL; ++s) {
            v[s] = (base + s < n) ? v[s] * inv_t : -INFINITY;
            mx = fmaxf(mx, v[s]);
        }
        mx = fmaxf(mx, dpp_mov<DPP_XOR1>(mx)); mx = fmaxf(mx, dpp_mov<DPP_XOR2>(mx));
        mx = fmaxf(mx, dpp_mov<DPP_HALF_MIRROR>(mx)); mx = fmaxf(mx, dpp_mov<DPP_MIRROR>(mx));
        mx = fmaxf(fmaxf(readlane(mx, 15), readlane(mx, 31)), fmaxf(readlane(mx, 47), readlane(mx, 63)));
        double part = 0.0;
#pragma unroll
        for (int s = 0; s < EPL; ++s) {
            v[s] = (base + s < n) ? expf(v[s] - mx) : 0.f;
            part += (double)v[s];
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) part += __shfl_xor(part, m, 64);
        const float denom = (float)part;
#pragma unroll
        for (int s = 0; s < EPL; ++s) u[s] = __float_as_uint(v[s] / denom);  // 0 for slots past n
    }
    FS_TS(1);
    // k-th largest value T (#{u > T} < k <= #{u >= T}) by radix select over the 30-bit patterns, 8 + 8 + 8 + 6 bits from the top:
    // per pass the candidates whose higher bits match the prefix are counted into a 256-bin LDS histogram (ds_add, no return),
    // every lane takes 4 bins, a DPP scan gives the counts above each lane, and the bin holding the rank-th candidate extends
    // the prefix -- 4 passes of ~1000 cycles instead of 30 bisection steps of ~380 (each a count over all candidates + a scalar hop)
    uint32_t* hist = reinterpret_cast<uint32_t*>(keyb);  // 256 bins; keyb is only written after T is known
    uint32_t prefix = 0u;
    int krem = kk;
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = pass == 0 ? 22 : (pass == 1 ? 14 : (pass == 2 ? 6 : 0)), bits = pass == 3 ? 6 : 8;
        *reinterpret_cast<uint4*>(hist + lane * 4) = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
        for (int s2 = 0; s2 < EPL; ++s2)
            if (pass == 0 || (u[s2] >> (shift + bits)) == prefix) atomicAdd(&hist[(u[s2] >> shift) & ((1u << bits) - 1u)], 1u);
        const uint4 hv = *reinterpret_cast<const uint4*>(hist + lane * 4);  // bins 4 * lane .. 4 * lane + 3 (one wave: LDS ops stay in order)
        const int h4[4] = {(int)hv.x, (int)hv.y, (int)hv.z, (int)hv.w};
        const int mine = (h4[0] + h4[1]) + (h4[2] + h4[3]);
        const int incl = wave_incl_scan(mine);
        int above = __builtin_amdgcn_readlane(incl, 63) - incl;  // candidates in bins of higher lanes
        int found_bin = -1, found_above = 0;
#pragma unroll
        for (int j = 3; j >= 0; --j) {  // from this lane's top bin down: the bin with above < rank <= above + count
            if (found_bin < 0 && above < krem && krem <= above + h4[j]) { found_bin = lane * 4 + j; found_above = above; }
            above += h4[j];
        }
        const unsigned long long m = __ballot(found_bin >= 0);  // exactly one lane (rank <= number of candidates)
        const int src = __builtin_ctzll(m);
        prefix = (prefix << bits) | (uint32_t)__builtin_amdgcn_readlane(found_bin, src);
        krem -= __builtin_amdgcn_readlane(found_above, src);
    }
    const uint32_t lo = prefix;
    const uint32_t T = lo;
    FS_TS(2);
    // keep p > T and the first k - #{p > T} ties in index order (lane-major, then slot)
    const int nvalid = min(max(n - base, 0), EPL);  // only matters for ties at T == 0 (slots past n hold 0 as well)
    int my_gt = 0, my_eq = 0;
#pragma unroll
    for (int s = 0; s < EPL; ++s) { my_gt += u[s] > T ? 1 : 0; my_eq += (u[s] == T && s < nvalid) ? 1 : 0; }
    const int sc_gt = wave_incl_scan(my_gt), sc_eq = wave_incl_scan(my_eq);
    const int r_ties = kk - __builtin_amdgcn_readlane(sc_gt, 63);  // ties to keep (>= 1)
    int run_eq = sc_eq - my_eq;                                    // ties in lower lanes
    uint32_t keepbits = 0u;
    int my_keep = 0;
#pragma unroll
    for (int s = 0; s < EPL; ++s) {
        const bool eq = u[s] == T && s < nvalid;
        const bool keep = u[s] > T || (eq && run_eq < r_ties);
        run_eq += eq ? 1 : 0;
        keepbits |= keep ? (1u << s) : 0u;
        my_keep += keep ? 1 : 0;
    }
    int pos = wave_incl_scan(my_keep) - my_keep;
#pragma unroll
    for (int s = 0; s < EPL; ++s)
        if (keepbits & (1u << s)) {
            kp[pos] = __uint_as_float(u[s]);
            ki[pos] = base + s;
            keyb[pos] = ((unsigned long long)u[s] << 32) | (unsigned long long)(255 - pos);
            ++pos;
        }
    FS_TS(3);
    // sort the kept keys (descending): position i = lane * 4 + s.  Bitonic network with the direction folded into the keys
    // (keys of "ascending" regions are complemented for the duration of a merge phase), so every compare-exchange is the
    // same max / min select.
    unsigned long long k[4];
    {
        const ulonglong2 a = *reinterpret_cast<const ulonglong2*>(keyb + lane * 4), b = *reinterpret_cast<const ulonglong2*>(keyb + lane * 4 + 2);
        k[0] = lane * 4 + 0 < kk ? a.x : 0ull; k[1] = lane * 4 + 1 < kk ? a.y : 0ull;
        k[2] = lane * 4 + 2 < kk ? b.x : 0ull; k[3] = lane * 4 + 3 < kk ? b.y : 0ull;
    }
#pragma unroll
    for (int lk = 1; lk <= 8; ++lk) {       // merge phase K = 1 << lk
        const int K = 1 << lk;
#pragma unroll
        for (int s = 0; s < 4; ++s) {       // complement the regions that this phase sorts ascending
            const uint32_t f = 0u - (uint32_t)(((lane * 4 + s) >> lk) & 1);
            k[s] ^= ((unsigned long long)f << 32) | f;
        }
#pragma unroll
        for (int j = K >> 1; j > 0; j >>= 1) {
            if (j >= 4) {
                const int lm = j >> 2;
                const bool lower = (lane & lm) == 0;
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const unsigned long long o = lm == 1 ? dpp_xor_lane_u64(k[s], 1) : (lm == 2 ? dpp_xor_lane_u64(k[s], 2) : __shfl_xor(k[s], lm, 64));
                    const bool g = k[s] > o;
                    const unsigned long long mxk = g ? k[s] : o, mnk = g ? o : k[s];
                    k[s] = lower ? mxk : mnk;
                }
            } else {
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    if (s & j) continue;
                    const unsigned long long a = k[s], b = k[s ^ j];
                    const bool g = a > b;
                    k[s] = g ? a : b;
                    k[s ^ j] = g ? b : a;
                }
            }
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const uint32_t f = 0u - (uint32_t)(((lane * 4 + s) >> lk) & 1);
            k[s] ^= ((unsigned long long)f << 32) | f;
        }
    }
    *reinterpret_cast<float4*>(sp + lane * 4) = make_float4(__uint_as_float((uint32_t)(k[0] >> 32)), __uint_as_float((uint32_t)(k[1] >> 32)),
                                                            __uint_as_float((uint32_t)(k[2] >> 32)), __uint_as_float((uint32_t)(k[3] >> 32)));
    FS_TS(4);
    // two sequential f32 chains in one instruction stream, pure adds: lane 0 sums kp (ascending index), lane 1 walks sp
    // (descending order) and leaves its running sums in cumsp; the top-p cut is then found in parallel:
    // cut = first rank r whose EXCLUSIVE running sum is >= top_p  ==  1 + first q with inclusive sum[q] >= top_p
    const float* arr = lane == 1 ? sp : kp;
    float cum = 0.f;
    for (int j = 0; j < kk; j += 32) {
        float v[32];
        lds_fetch32(arr, j, kk, v);
#pragma unroll
        for (int e = 0; e < 32; ++e) { cum += v[e]; v[e] = cum; }
        if (lane == 1) {
#pragma unroll
            for (int q = 0; q < 8; ++q) *reinterpret_cast<float4*>(cumsp + j + 4 * q) = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
        }
    }
    const float sum_p = readlane(cum, 0);
    const bool do_topp = batch ? !(top_p64 <= 0.0 || top_p64 >= (double)sum_p) : !(top_p <= 0.f || top_p >= sum_p);  // sampling/mod.rs:68
    FS_TS(5);
    if (do_topp) {  // zero every prob once the running cumsum (descending order) reached top_p
        const float4 cq = *reinterpret_cast<const float4*>(cumsp + lane * 4);
        const float cs[4] = {cq.x, cq.y, cq.z, cq.w};
        int first = 0x7FFFFFFF;
#pragma unroll
        for (int s = 3; s >= 0; --s) if (lane * 4 + s < kk && cs[s] >= top_p) first = lane * 4 + s;
        const unsigned long long mh = __ballot(first != 0x7FFFFFFF);
        const int cutv = mh ? __builtin_amdgcn_readlane(first, __builtin_ctzll(mh)) + 1 : kk;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int i = lane * 4 + s;
            if (i < kk && i >= cutv) kp[255 - (int)(k[s] & 0xFFull)] = 0.f;
        }
    }
}

// WeightedIndex::new + sample over the contiguous weights w[0..cnt), cnt <= 256, by one wave.  Zero weights (entries cut by top-p)
// do not move the cumulative f32 sum (x + 0 == x exactly) and are never picked, so the sequential chain only walks the NON-ZERO
// weights, compacted in ascending index order first (DPP prefix scan; `cval` / `cpos` = LDS scratch for <= 256 floats / ints):
// after a top-p cut that is typically a few dozen of the 256 entries.  Every lane runs the same chain (lane 0 leaves the running
// sums in `cum`), then each lane tests its four compacted entries.
__device__ int wave_pick(const float* w, int cnt, float* cum, RngState* rng, uint32_t word, float* cval, int* cpos) {
    const int lane = threadIdx.x & 63;
    const float4 wv = *reinterpret_cast<const float4*>(w + lane * 4);
    const float ws[4] = {wv.x, wv.y, wv.z, wv.w};
    int mine = 0;
#pragma unroll
    for (int s = 0; s < 4; ++s) mine += (lane * 4 + s < cnt && ws[s] != 0.f) ? 1 : 0;
    const int incl = wave_incl_scan(mine);
    const int m = __builtin_amdgcn_readlane(incl, 63);  // non-zero weights
    if (m == 0) return 0;
    int pos = incl - mine;
#pragma unroll
    for (int s = 0; s < 4; ++s)
        if (lane * 4 + s < cnt && ws[s] != 0.f) { cval[pos] = ws[s]; cpos[pos] = lane * 4 + s; ++pos; }
    float total = 0.f;
    for (int j = 0; j < m; j += 32) {
        float v[32];
        lds_fetch32(cval, j, m, v);
#pragma unroll
        for (int e = 0; e < 32; ++e) { total += v[e]; v[e] = total; }
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < 8; ++q) *reinterpret_cast<float4*>(cum + j + 4 * q) = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
        }
    }
    if (!(total > 0.f)) return 0;
    const float max_rand = __uint_as_float((0xFFFFFFFFu >> 9) | (127u << 23)) - 1.0f;
    float scale = total;
    while (scale * max_rand + 0.f >= total) scale = __uint_as_float(__float_as_uint(scale) - 1u);
    if (lane == 0) rng->consumed += 1;
    const float chosen = (__uint_as_float((word >> 9) | (127u << 23)) - 1.0f) * scale + 0.f;
    const float4 cv = *reinterpret_cast<const float4*>(cum + lane * 4);
    const float cs[4] = {cv.x, cv.y, cv.z, cv.w};
    int first = 0x7FFFFFFF;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int j = lane * 4 + s;
        if (j < m && cs[s] > chosen && first == 0x7FFFFFFF) first = j;  // first kept item whose inclusive cumulative weight is > chosen
    }
    const unsigned long long mh = __ballot(first != 0x7FFFFFFF);
    const int jsel = mh ? __builtin_amdgcn_readlane(first, __builtin_ctzll(mh)) : m - 1;  // else the last non-zero item
    return cpos[jsel];
}

// Block-wide selection of one index from `n` logits held in LDS (already penalised / masked).
//  temp == 0: the argmax by IEEE comparison, FIRST (first_max: the batch rule, the only one production reaches here) or LAST index;
//             the host-ArgMax rule of the single-sequence and slot paths (totalOrder) is greedy_pick's / slot_greedy_pick's.
//  temp  > 0: softmax(logits / temp) -> top-k (ties: lower index first) -> top-p -> WeightedIndex draw, evaluated in
//             ascending-index order with the StdRng stream (sampling/mod.rs:51-132).  Identical decision procedure to
//             oracle::LogitsProcessor::sample; the softmax denominator is accumulated in f64 on both sides so that
//             the result does not depend on reduction order.
__device__ int block_sample(float* lg /*LDS [n]*/, int n, const SampleCfg& c, RngState* rng, float* sp /*LDS [SAMPLE_MAXN]*/,
                            int* si /*LDS [SAMPLE_MAXN]*/, double* red /*LDS [SAMPLE_THREADS]*/, bool first_max = false) {
    const int tid = threadIdx.x;
    __shared__ int s_result;
    if (c.temp == 0.f) {
        // argmax with the host rule (LAST maximal index) or the device rule (FIRST): per-thread scan, DPP/readlane wave
        // reduction of the value, ballot-free index pick, then one LDS hop across the waves
        float bv = -INFINITY;
        int bi = -1;
        for (int i = tid; i < n; i += SAMPLE_THREADS) {
            const float v = lg[i];
            if (bi < 0 || (first_max ? (v > bv) : !(v < bv))) { bv = v; bi = i; }  // ascending i per thread
        }
        float wm = bv;
        wm = fmaxf(wm, dpp_mov<DPP_XOR1>(wm)); wm = fmaxf(wm, dpp_mov<DPP_XOR2>(wm));
        wm = fmaxf(wm, dpp_mov<DPP_HALF_MIRROR>(wm)); wm = fmaxf(wm, dpp_mov<DPP_MIRROR>(wm));
        wm = fmaxf(fmaxf(readlane(wm, 15), readlane(wm, 31)), fmaxf(readlane(wm, 47), readlane(wm, 63)));
        int cand = (bi >= 0 && bv == wm) ? bi : (first_max ? 0x7FFFFFFF : -1);
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const int o = __shfl_xor(cand, m, 64);
            cand = first_max ? min(cand, o) : max(cand, o);
        }
        float* rv = reinterpret_cast<float*>(red);
        int* ri = reinterpret_cast<int*>(red) + 64;
        const int wv = tid >> 6;
        if ((tid & 63) == 0) { rv[wv] = wm; ri[wv] = cand; }
        __syncthreads();
        if (tid == 0) {
            float gv = rv[0];
            int gi = ri[0];
            for (int w2 = 1; w2 < SAMPLE_THREADS / 64; ++w2) {
                const float v2 = rv[w2];
                const int i2 = ri[w2];
                if (v2 > gv || (v2 == gv && (first_max ? i2 < gi : i2 > gi))) { gv = v2; gi = i2; }
            }
            s_result = gi;
        }
        __syncthreads();
        const int res = s_result;
        __syncthreads();
        return res;
    }
    {
        const bool use_k0 = c.top_k > 0 && c.top_k < n;
        if (use_k0 && c.top_k <= 256 && n <= 2048) {
            // one-wave path (see wave_topk_select): wave 0 selects, the last wave computes this draw's StdRng word meanwhile
            const float inv_t0 = (float)(1.0 / (double)c.temp);
            __shared__ uint32_t s_word0;
            __shared__ __attribute__((aligned(16))) float w_kp[256 + 32];
            __shared__ __attribute__((aligned(16))) float w_cum[256 + 32];
            __shared__ __attribute__((aligned(16))) unsigned long long w_key[256];
            __shared__ int w_ki[256];
            const int kk0 = c.top_k;
            FS_TS(0);
            if (tid < 64) {
                if (n <= 1024) wave_topk_select<16>(lg, n, kk0, inv_t0, c.top_p, w_kp, w_ki, sp, w_key, w_cum, first_max, c.top_p64);
                else wave_topk_select<32>(lg, n, kk0, inv_t0, c.top_p, w_kp, w_ki, sp, w_key, w_cum, first_max, c.top_p64);
            } else if (tid == SAMPLE_THREADS - 1) {
                s_word0 = chacha12_word(rng->key, rng->consumed);
            }
            FS_TS(6);
            __syncthreads();
            FS_TS(7);
            if (tid < 64) {
                const int pick = wave_pick(w_kp, kk0, w_cum, rng, s_word0, sp, si);  // sp / si: free after the sort
                if (tid == 0) s_result = w_ki[pick];
            }
            FS_TS(8);
            __syncthreads();
            const int res = s_result;
            __syncthreads();
            return res;
        }
    }
    // softmax(logits * (1/temp)).  Blocked ownership: thread t owns the `ept` consecutive candidates t*ept .. t*ept+ept-1
    // (ascending index order == thread-major order, which the index-order prefix scans below rely on).
    FS_TS(0);
    const float inv_t = (float)(1.0 / (double)c.temp);
    const int ept = (n + SAMPLE_THREADS - 1) / SAMPLE_THREADS;  // 1..4
    const int lane = tid & 63, wv = tid >> 6;
    // the StdRng word of this call's draw: ~800 dependent integer ops, computed by the last wave while the others select
    __shared__ uint32_t s_word;
    if (tid == SAMPLE_THREADS - 1) s_word = chacha12_word(rng->key, rng->consumed);
    float pv[4];
    bool valid[4];
    float mx = -INFINITY;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int i = tid * ept + s;
        valid[s] = s < ept && i < n;
        pv[s] = valid[s] ? lg[i] * inv_t : -INFINITY;
        mx = fmaxf(mx, pv[s]);
    }
    float* rv = reinterpret_cast<float*>(red);
    mx = fmaxf(mx, dpp_mov<DPP_XOR1>(mx)); mx = fmaxf(mx, dpp_mov<DPP_XOR2>(mx));
    mx = fmaxf(mx, dpp_mov<DPP_HALF_MIRROR>(mx)); mx = fmaxf(mx, dpp_mov<DPP_MIRROR>(mx));
    mx = fmaxf(fmaxf(readlane(mx, 15), readlane(mx, 31)), fmaxf(readlane(mx, 47), readlane(mx, 63)));
    if (lane == 0) rv[wv] = mx;
    __syncthreads();
#pragma unroll
    for (int w2 = 0; w2 < SAMPLE_THREADS / 64; ++w2) mx = fmaxf(mx, rv[w2]);
    __syncthreads();
    double part = 0.0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        pv[s] = valid[s] ? expf(pv[s] - mx) : 0.f;
        part += (double)pv[s];
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) part += __shfl_xor(part, m, 64);
    if (lane == 0) red[wv] = part;
    __syncthreads();
    double dsum = 0.0;
#pragma unroll
    for (int w2 = 0; w2 < SAMPLE_THREADS / 64; ++w2) dsum += red[w2];
    const float denom = (float)dsum;
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 4; ++s) pv[s] = pv[s] / denom;  // probabilities (by index, in registers)
    FS_TS(1);
    const bool use_k = c.top_k > 0 && c.top_k < n;
    const int kk = use_k ? c.top_k : n;
    __shared__ int s_cut;       // number of leading sorted entries that survive top-p
    __shared__ int s_do_topp;
    // ---- general path (no top-k, k > 256, or more than 2048 candidates): full bitonic sort by (prob desc, index asc) over the next power of two
#pragma unroll
    for (int s = 0; s < 4; ++s) if (valid[s]) lg[tid * ept + s] = pv[s];
    int np2 = 1;
    while (np2 < n) np2 <<= 1;
    __syncthreads();
    for (int i = tid; i < np2; i += SAMPLE_THREADS) {
        if (i < n) { sp[i] = lg[i]; si[i] = i; } else { sp[i] = -1.f; si[i] = 0x7FFFFFFF; }
    }
    __syncthreads();
    for (int k = 2; k <= np2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < np2; i += SAMPLE_THREADS) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const bool up = (i & k) == 0;
                    const float p1 = sp[i], p2 = sp[ixj];
                    const int i1 = si[i], i2 = si[ixj];
                    const bool before = (p1 > p2) || (p1 == p2 && i1 < i2);  // element i sorts before element ixj
                    if (before != up) { sp[i] = p2; sp[ixj] = p1; si[i] = i2; si[ixj] = i1; }
                }
            }
            __syncthreads();
        }
    }
    // ---- tail.  Decision procedure and f32 rounding identical to the oracle restatement: sums and the WeightedIndex scan
    // run in ascending token-index order, the top-p cut in descending probability order, every sum is a sequential f32
    // chain.  To keep those chains short and free of dependent LDS indirections, the kept set (top_k entries, or all n)
    // is materialised as CONTIGUOUS arrays: kp[j] = probability of the j-th kept token in index order, ki[j] = its index.
    int* ki = reinterpret_cast<int*>(red);  // 8 KB scratch: up to 2048 ints
    float* kp = lg;                          // the by-index array is no longer needed once (sp, si) are sorted
    const bool small = use_k && kk <= 2 * SAMPLE_THREADS;
    int cnt;                                 // entries of (ki, kp)
    if (small) {
        int kp2 = 1;
        while (kp2 < kk) kp2 <<= 1;
        __syncthreads();
        for (int r = tid; r < kp2; r += SAMPLE_THREADS) { ki[r] = r < kk ? si[r] : 0x7FFFFFFF; kp[r] = r < kk ? sp[r] : 0.f; }
        __syncthreads();
        for (int k2 = 2; k2 <= kp2; k2 <<= 1)
            for (int j = k2 >> 1; j > 0; j >>= 1) {
                for (int i = tid; i < kp2; i += SAMPLE_THREADS) {
                    const int ixj = i ^ j;
                    if (ixj > i) {
                        const int a0 = ki[i], a1 = ki[ixj];
                        const bool up = (i & k2) == 0;
                        if ((a0 > a1) == up) {
                            ki[i] = a1; ki[ixj] = a0;
                            const float t0 = kp[i]; kp[i] = kp[ixj]; kp[ixj] = t0;
                        }
                    }
                }
                __syncthreads();
            }
        cnt = kk;
    } else {  // all n tokens (or a top-k too large for the scratch): index order is the identity
        __syncthreads();
        for (int i = tid; i < n; i += SAMPLE_THREADS) kp[i] = 0.f;
        __syncthreads();
        for (int r = tid; r < kk; r += SAMPLE_THREADS) kp[si[r]] = sp[r];
        __syncthreads();
        cnt = n;
    }
    if (tid == 0) {
        bool do_topp = true;
        if (use_k) {
            const float sum_p = seq_sum(kp, cnt);  // ascending index; entries outside the top-k are 0 (or absent)
            do_topp = first_max ? !(c.top_p64 <= 0.0 || c.top_p64 >= (double)sum_p) : !(c.top_p <= 0.f || c.top_p >= sum_p);  // (first_max == batch semantics)
        }
        // zero every prob once the running cumsum (descending order) reached top_p
        s_cut = do_topp ? seq_topp_cut(sp, kk, c.top_p) : kk;
        s_do_topp = do_topp ? 1 : 0;
    }
    __syncthreads();
    if (s_do_topp && s_cut < kk) {  // entries sorting at or after rank `cut` are zeroed (parallel predicate on (prob, index))
        const float pc = sp[s_cut];
        const int ic = si[s_cut];
        for (int j = tid; j < cnt; j += SAMPLE_THREADS) {
            const float pj = kp[j];
            const int ij = small ? ki[j] : j;
            if (pj < pc || (pj == pc && ij >= ic)) kp[j] = 0.f;
        }
    }
    __syncthreads();
    {
        const int r = block_weighted_pick(kp, cnt, sp, rng, s_word);
        const int res = small ? ki[r] : r;
        __syncthreads();
        return res;
    }
}

// Greedy pick (temp == 0, host ArgMax rule, fishrt.h: the maximum under IEEE totalOrder -- -0.0 < +0.0 -- and the LAST index among
// identical bit patterns) without the three block barriers of block_sample: a thread's candidates (indices tid + j * SAMPLE_THREADS)
// stay in registers as total-order keys, a wave reduces (key, then index) by DPP, lane 0 of every wave does one 64-bit LDS atomicMax on
// {key : index}, ONE barrier, everybody reads the winner.  The same order at every level: thread, wave, block.  *s_key must have been
// zeroed before the previous barrier.  (A 16-wave barrier phase costs ~0.4 us on this chip.)
__device__ __forceinline__ int dpp_wave_max_int(int v) {
    v = max(v, __builtin_amdgcn_mov_dpp(v, DPP_XOR1, 0xF, 0xF, false)); v = max(v, __builtin_amdgcn_mov_dpp(v, DPP_XOR2, 0xF, 0xF, false));
    v = max(v, __builtin_amdgcn_mov_dpp(v, DPP_HALF_MIRROR, 0xF, 0xF, false)); v = max(v, __builtin_amdgcn_mov_dpp(v, DPP_MIRROR, 0xF, 0xF, false));
    return max(max(__builtin_amdgcn_readlane(v, 15), __builtin_amdgcn_readlane(v, 31)), max(__builtin_amdgcn_readlane(v, 47), __builtin_amdgcn_readlane(v, 63)));
}
// IEEE-754 totalOrder as a signed integer key: key(a) < key(b) iff a.total_cmp(b) is Less (-0.0 < +0.0; identical bit patterns are equal)
__device__ __forceinline__ int total_key(float v) {
    const int s = __float_as_int(v);
    return s ^ ((s >> 31) & 0x7FFFFFFF);
}
__device__ __forceinline__ int greedy_pick(const float (&val)[SAMPLE_MAXN / SAMPLE_THREADS], int n, unsigned long long* s_key) {
    const int tid = threadIdx.x;
    int bk = (int)0x80000000;
    int bi = -1;
#pragma unroll
    for (int j = 0; j < SAMPLE_MAXN / SAMPLE_THREADS; ++j) {
        const int i = tid + j * SAMPLE_THREADS;
        const int k = total_key(val[j]);
        if (i < n && (bi < 0 || k >= bk)) { bk = k; bi = i; }  // ascending i per thread: the later identical value wins
    }
    const int wk = dpp_wave_max_int(bk);
    const int ci = dpp_wave_max_int((bi >= 0 && bk == wk) ? bi : -1);
    if ((tid & 63) == 0 && ci >= 0)  // (key with the sign bit flipped: unsigned order == total order)
        atomicMax(s_key, ((unsigned long long)((uint32_t)wk ^ 0x80000000u) << 32) | (unsigned long long)(uint32_t)ci);
    __syncthreads();
    return (int)(*s_key & 0xFFFFFFFFull);
}

// legacy_softmax_sample (sampling/mod.rs:8-26), the Fish <= 1.4 slow token: P(pad) = softmax([pad, eos])[0] in f32; u ~ U[0,1) =
// (next_u32 >> 8) * 2^-24 (rand Standard<f32>).  The reference draws from an unseeded thread_rng; here `w` is a word of the request's
// seeded StdRng stream so that runs are reproducible.  What `done` and the capture record make of the draw is the caller's.
struct LegacyDraw { float u; bool is_pad; };
__device__ __forceinline__ LegacyDraw legacy_draw(float pad, float eos, uint32_t w, int ignore_eos) {
    const float m = fmaxf(pad, eos);
    const float e_pad = expf(pad - m), e_eos = expf(eos - m);
    const float p_pad = e_pad / (e_pad + e_eos);
    const float u = (float)(w >> 8) * (1.0f / 16777216.0f);
    return {u, u < p_pad || ignore_eos};
}

// SingleBatchedRepPenProcessor::apply (rep_pen.rs:37-65): the 16-deep window of one codebook's previous picks as a 17-slot ring.  The plan
// is this call's push_front of the previous pick and the pop_back past 16 entries, read from (ring, meta) before either is written;
// "token in tokens_seen" == "mask[token] == penalty" (set on insert, reset to 1 on removal; with penalty == 1 the mask never changes).
// The kernel stores ring[head] = last, meta = {head, drop ? 16 : len} where its barriers allow, and mask[i] = apply(i, mask[i], ..) where
// the two differ; the logit is divided by the new mask value whatever its sign (rep_pen.rs:62).
struct RepPenPlan {
    int last = -1, dropped = -1, head = 0, len = 0;
    bool drop = false;
    __device__ __forceinline__ float apply(int i, float m0, float rep_pen) const {
        float m = m0;
        if (i == last) m = rep_pen;
        if (i == dropped && m == rep_pen) m = 1.0f;
        return m;
    }
};
__device__ __forceinline__ RepPenPlan reppen_plan(bool have_prev, const uint32_t& prev_code, const int* ring, const int* meta) {
    RepPenPlan p;
    if (have_prev) {
        p.last = (int)prev_code;
        p.head = (meta[0] + 16) % 17; p.len = meta[1] + 1;               // push_front
        p.drop = p.len > 16;
        if (p.drop) p.dropped = ring[(p.head + p.len - 1) % 17];         // pop_back (never the slot that takes `last`)
    }
    return p;
}

__device__ inline void child_rng(const RngState* master, unsigned long long n64, RngState* out);

template <typename WT>
__global__ __launch_bounds__(SAMPLE_THREADS) void k_sample_slow(const float* __restrict__ logits, int n,
                                                                const SampleCfg* __restrict__ cp, RngState* rng, SeqState* __restrict__ state,
                                                                const float* __restrict__ x, float* __restrict__ xf, int dim,
                                                                float* const* __restrict__ hid_slot) {
    __shared__ __attribute__((aligned(16))) float lg[SAMPLE_MAXN];
    __shared__ __attribute__((aligned(16))) float sp[SAMPLE_MAXN];
    __shared__ __attribute__((aligned(16))) int si[SAMPLE_MAXN];
    __shared__ double red[SAMPLE_THREADS];
    const int tid = threadIdx.x;
    const SampleCfg c = *cp;
    // generate_blocking_with_hidden (single_batch.rs:250,264-266): the hidden state of every generator iteration, the terminating one
    // included, row = iteration index; replays after termination (done != 0 on entry) write nothing
    float* hid = hid_slot ? *hid_slot : nullptr;
    if (hid && state->done != 0) hid = nullptr;
    if (hid) hid += (size_t)state->frame * dim;
    __shared__ unsigned long long s_key;
    if (c.batch_rows > 0 && !c.legacy) {  // row `batch_row` of a static batch on the single-sequence path: sampling/mod.rs:77-109
        __shared__ RngState lrng;
        SampleCfg cb = c;
        if (cb.temp <= 1e-7f) cb.temp = 0.f;
        for (int i = tid; i < n; i += SAMPLE_THREADS) lg[i] = logits[i];
        for (int i = tid; i < dim; i += SAMPLE_THREADS) { const float h = x[i]; xf[i] = h; if (hid) hid[i] = h; }
        if (tid == 0 && cb.temp != 0.f)
            child_rng(rng, (unsigned long long)state->frame * (unsigned long long)c.batch_calls * c.batch_rows + c.batch_row, &lrng);
        __syncthreads();
        if (cb.ignore_eos && tid == 0) lg[0] = -INFINITY;
        __syncthreads();
        const int idx = block_sample(lg, n, cb, &lrng, sp, si, red, /*first_max=*/true);
        if (tid == 0) {
            uint32_t tok = audio_tok(c, idx);
            if (state->done) tok = c.im_end_id;
            state->cur[0] = tok;
            if (tok == c.im_end_id && state->done == 0) state->done = 1;
        }
        return;
    }
    if (c.temp == 0.f && !c.legacy) {  // greedy: two barriers instead of five (see greedy_pick)
        if (tid == 0) s_key = 0ull;
        float val[SAMPLE_MAXN / SAMPLE_THREADS];
#pragma unroll
        for (int j = 0; j < SAMPLE_MAXN / SAMPLE_THREADS; ++j) {
            const int i = tid + j * SAMPLE_THREADS;
            val[j] = i < n ? logits[i] : -INFINITY;
            if (i == 0 && c.ignore_eos) val[j] = -INFINITY;
        }
        for (int i = tid; i < dim; i += SAMPLE_THREADS) { const float h = x[i]; xf[i] = h; if (hid) hid[i] = h; }  // hidden_states -> fast decoder input (:149)
        __syncthreads();
        const int idx = greedy_pick(val, n, &s_key);
        if (tid == 0) {
            uint32_t tok = audio_tok(c, idx);  // rescale_semantic_tokens (utils.rs:45-46)
            if (state->done) tok = c.im_end_id;
            state->cur[0] = tok;
            if (tok == c.im_end_id && state->done == 0) state->done = 1;
        }
        return;
    }
    for (int i = tid; i < n; i += SAMPLE_THREADS) lg[i] = logits[i];
    for (int i = tid; i < dim; i += SAMPLE_THREADS) { const float h = x[i]; xf[i] = h; if (hid) hid[i] = h; }  // hidden_states -> fast decoder input (:149)
    __syncthreads();
    if (c.legacy) {
        if (tid == 0) {
            const uint32_t w = chacha12_word(rng->key, rng->consumed);
            rng->consumed += 1;
            uint32_t tok = legacy_draw(lg[0], lg[1], w, c.ignore_eos).is_pad ? c.pad_id : c.im_end_id;
            if (state->done) tok = c.im_end_id;
            state->cur[0] = tok;
            if (tok == c.im_end_id && state->done == 0) state->done = 1;
        }
        return;
    }
    if (c.ignore_eos && tid == 0) lg[0] = -INFINITY;
    __syncthreads();
    const int idx = block_sample(lg, n, c, rng, sp, si, red);
    if (tid == 0) {
        uint32_t tok = audio_tok(c, idx);  // rescale_semantic_tokens (utils.rs:45-46)
        if (state->done) tok = c.im_end_id;  // generator already terminated (single_batch.rs:86-88): stay terminated
        state->cur[0] = tok;
        if (tok == c.im_end_id && state->done == 0) state->done = 1;  // 1 = terminated by THIS frame, 2 = earlier
    }
}

template <typename WT>
__global__ __launch_bounds__(SAMPLE_THREADS) void k_sample_fast(const float* __restrict__ logits, int cb, int n_cb, int cb_size,
                                                                const SampleCfg* __restrict__ cp, RngState* rng, RepPenState rp,
                                                                SeqState* __restrict__ state, const WT* __restrict__ fast_emb,
                                                                float* __restrict__ xf, const WT* __restrict__ tok_emb,
                                                                const WT* __restrict__ cb_emb, float* __restrict__ x, int dim,
                                                                uint32_t* __restrict__ out_codes, int out_cap) {
    __shared__ __attribute__((aligned(16))) float lg[SAMPLE_MAXN];
    __shared__ __attribute__((aligned(16))) float sp[SAMPLE_MAXN];
    __shared__ __attribute__((aligned(16))) int si[SAMPLE_MAXN];
    __shared__ double red[SAMPLE_THREADS];
    const int tid = threadIdx.x;
    const int n = cb_size;
    const SampleCfg c = *cp;
    // one round trip for everything the decision needs: state words, the repetition-penalty ring, logits and mask
    __shared__ int s_ring[17], s_meta[2];
    __shared__ uint32_t s_prev, s_cur0, s_have_prev;
    __shared__ unsigned long long s_key;
    // batch_rows > 0: BatchedLogitsProcessor semantics (see k_sample_slow): first-max argmax at temp <= 1e-7, else the child StdRng of
    // (frame, codebook call, row)
    const bool bm = c.batch_rows > 0;
    SampleCfg cc = c;
    if (bm && cc.temp <= 1e-7f) cc.temp = 0.f;
    const bool greedy = cc.temp == 0.f && !bm;
    __shared__ RngState lrng;
    if (bm && tid == 23 && cc.temp != 0.f)
        child_rng(rng, ((unsigned long long)state->frame * (unsigned long long)(n_cb + 1) + 1ull + (unsigned long long)cb) * c.batch_rows + c.batch_row, &lrng);
    if (tid == 22) s_key = 0ull;
    if (tid < 17) s_ring[tid] = rp.ring[cb * 17 + tid];
    else if (tid < 19) s_meta[tid - 17] = rp.ring_meta[cb * 2 + tid - 17];
    else if (tid == 19) s_prev = state->prev[cb + 1];
    else if (tid == 20) s_cur0 = state->cur[0];
    else if (tid == 21) s_have_prev = (uint32_t)state->have_prev;
    float* mask = rp.mask + (size_t)cb * cb_size;
    float lv[SAMPLE_MAXN / SAMPLE_THREADS], mv[SAMPLE_MAXN / SAMPLE_THREADS];
#pragma unroll
    for (int j = 0; j < SAMPLE_MAXN / SAMPLE_THREADS; ++j) {
        const int i = tid + j * SAMPLE_THREADS;
        lv[j] = i < n ? logits[i] : 0.f;
        mv[j] = i < n ? mask[i] : 1.f;
    }
    __syncthreads();
    const bool eos = s_cur0 == c.im_end_id;  // single_batch.rs:153-156: push 0, skip the fast step
    if (!eos) {
        const bool pen = s_have_prev != 0;
        // the repetition-penalty window (RepPenPlan) from the LDS copy of the ring, applied to the register copy of the mask
        const RepPenPlan win = reppen_plan(pen, s_prev, s_ring, s_meta);
        if (pen && tid == 0) { rp.ring[cb * 17 + win.head] = win.last; rp.ring_meta[cb * 2] = win.head; rp.ring_meta[cb * 2 + 1] = win.drop ? 16 : win.len; }
#pragma unroll
        for (int j = 0; j < SAMPLE_MAXN / SAMPLE_THREADS; ++j) {
            const int i = tid + j * SAMPLE_THREADS;
            if (i < n) {
                float m = mv[j];
                if (pen) {
                    m = win.apply(i, mv[j], c.rep_pen);
                    if (m != mv[j]) mask[i] = m;
                }
                lv[j] = pen ? lv[j] / m : lv[j];
                if (!greedy) lg[i] = lv[j];
            }
        }
        if (!greedy) __syncthreads();
    }
    int code = 0;
    if (!eos) code = greedy ? greedy_pick(lv, n, &s_key) : block_sample(lg, n, cc, bm ? &lrng : rng, sp, si, red, /*first_max=*/bm);
    if (tid == 0) state->cur[cb + 1] = (uint32_t)code;
    if (cb != n_cb - 1) {
        if (!eos)
            for (int d = tid; d < dim; d += SAMPLE_THREADS) xf[d] = WTr<WT>::to_f32(fast_emb[(size_t)code * dim + d]);
        return;
    }
    // ---- end of frame (single_batch.rs:185-210 + generate_blocking :250,264-266).  Not rows_frame_commit: the single sequence has its own
    // state machine -- `done` goes 1 -> 2 here, the emit rule is `frame == 0 ||` this frame's slow token, and nothing freezes.
    __syncthreads();
    __shared__ uint32_t cur[16];
    if (tid <= n_cb) cur[tid] = (tid == n_cb) ? (uint32_t)code : state->cur[tid];
    __syncthreads();
    if (tid == 0 && state->done != 2) {
        const int frame = state->frame;
        if (state->done == 1) state->done = 2;  // replays after termination leave pos / outputs untouched
        if (frame == 0 || cur[0] != c.im_end_id) {
            const int o = state->n_out;
            if (o < out_cap)
                for (int cc = 0; cc < n_cb; ++cc) out_codes[(size_t)cc * out_cap + o] = cur[cc + 1];
            state->n_out = o + 1;
        }
        for (int i = 0; i <= n_cb; ++i) state->prev[i] = cur[i];
        state->have_prev = 1;
        state->pos += 1;
        state->frame = frame + 1;
    }
    // next slow input: embed([slow, c0..c7]) (dual_ar.rs:532-567)
    embed_tokens<WT>(tok_emb, cb_emb, dim, n_cb, cb_size, c.sem_lo, c.sem_hi, cur, 1, x, tid, SAMPLE_THREADS);
}

// ------------------------------------------------------------------------------------------------ batched (static-batch) sampling
// generate/static_batch.rs:117-274 + sampling/mod.rs:77-109: one block per batch row.  temp <= 1e-7 -> device argmax
// (FIRST maximal index); else softmax(logits / temp) and, per sample() call, every row draws from its OWN child StdRng
// seeded with the next u64 of the master StdRng (sampling/mod.rs:93-95): call c of the request, row b uses master u64
// number c * B + b, and the single WeightedIndex draw consumes word 0 of the child stream.
__device__ inline void child_rng(const RngState* master, unsigned long long n64, RngState* out) {
    const unsigned long long lo = chacha12_word(master->key, 2 * n64), hi = chacha12_word(master->key, 2 * n64 + 1);
    seed_from_u64((hi << 32) | lo, out->key);
    out->consumed = 0;
}

// ---- end of frame of the row families (k_sample_fast_rows, _rows_par, _slots; static_batch.rs:224-267 + generate_static_batch :305-338):
// the last codebook's block of row `b` assembles the frame in `cur`, emits it, advances the row and embeds the next slow input into X[b].
// take_code: the last code is this launch's `code` (else the row keeps st->cur[n_cb]).  freeze: session slots (SampleCfg::session; always
// for per-slot sessions, whose emit rule is then that of single_batch.rs:185-210: first frame unconditionally, the terminating
// iteration's codes are not) -- a dead slot is frozen: it neither emits nor advances from the frame after its last one.  All `nthreads`
// threads of the block must call.
template <typename WT>
__device__ __forceinline__ void rows_frame_commit(SeqState* st, const SampleCfg& c, int code, bool take_code, bool freeze, int b, int n_cb,
                                                  int cb_size, const WT* __restrict__ tok_emb, const WT* __restrict__ cb_emb,
                                                  float* __restrict__ X, int dim, uint32_t* __restrict__ out_codes, int out_cap, int nthreads) {
    const int tid = threadIdx.x;
    __syncthreads();
    __shared__ uint32_t cur[16];
    if (tid <= n_cb) {
        const uint32_t slow = st->cur[0];
        const bool is_audio = slow >= c.sem_lo;  // :229 (non-audio rows carry zero codes)
        uint32_t v = tid == 0 ? slow : (tid == n_cb && take_code ? (uint32_t)code : st->cur[tid]);
        if (tid > 0 && !is_audio) v = 0;
        cur[tid] = v;
    }
    __syncthreads();
    if (tid == 0) {
        const int frame = st->frame;
        const bool frozen = freeze && st->done != 0 && frame > 0;
        if (!frozen) {
            if (frame == 0 || !st->done) {  // first position unconditionally, then only while the row is active
                if (frame == 0 && cur[0] < c.sem_lo) st->step = -1;  // BatchPosition::is_audio of the first position (static_batch.rs:229): `step` is free during decode
                const int o = st->n_out;
                uint32_t* oc = out_codes + (size_t)b * n_cb * out_cap;
                if (o < out_cap)
                    for (int cc = 0; cc < n_cb; ++cc) oc[(size_t)cc * out_cap + o] = cur[cc + 1];
                st->n_out = o + 1;
            }
            for (int i = 0; i <= n_cb; ++i) { st->prev[i] = cur[i]; st->cur[i] = cur[i]; }
            st->have_prev = 1;
            st->pos += 1;  // dead rows keep stepping in lock-step (:255-261)
            st->frame = frame + 1;
        }
    }
    embed_tokens<WT>(tok_emb, cb_emb, dim, n_cb, cb_size, c.sem_lo, c.sem_hi, cur, 1, X + (size_t)b * dim, tid, nthreads);
}

template <typename WT>
__global__ __launch_bounds__(SAMPLE_THREADS) void k_sample_slow_rows(const float* __restrict__ logits, int ld, int n,
                                                                     const SampleCfg* __restrict__ cp, const RngState* __restrict__ master,
                                                                     int B, int calls_per_frame, SeqState* __restrict__ states,
                                                                     const float* __restrict__ X, float* __restrict__ XF, int dim, PrepOut po) {
    __shared__ float red4[4];
    __shared__ __attribute__((aligned(16))) float lg[SAMPLE_MAXN];
    __shared__ __attribute__((aligned(16))) float sp[SAMPLE_MAXN];
    __shared__ __attribute__((aligned(16))) int si[SAMPLE_MAXN];
    __shared__ double red[SAMPLE_THREADS];
    __shared__ RngState lrng;
    const int tid = threadIdx.x, b = blockIdx.x;
    SeqState* st = states + b;
    SampleCfg c = *cp;
    if (c.temp <= 1e-7f) c.temp = 0.f;  // sampling/mod.rs:80
    for (int i = tid; i < n; i += SAMPLE_THREADS) lg[i] = logits[(size_t)b * ld + i];
    for (int i = tid; i < dim; i += SAMPLE_THREADS) XF[(size_t)b * dim + i] = X[(size_t)b * dim + i];  // hidden_states (:175)
    __syncthreads();
    if (c.ignore_eos && tid == 0) lg[0] = -INFINITY;
    __syncthreads();
    // the child StdRng (two ChaCha12 blocks + the PCG expansion: ~3 us of dependent integer work) is derived by the thread that also
    // computes the draw's word inside block_sample -- the last one -- while wave 0 already selects; nobody else reads lrng before the
    // barrier in front of the pick
    if (tid == SAMPLE_THREADS - 1 && c.temp != 0.f) child_rng(master, (unsigned long long)st->frame * calls_per_frame * B + b, &lrng);
    const int idx = block_sample(lg, n, c, &lrng, sp, si, red, /*first_max=*/true);
    if (tid == 0) {
        const uint32_t tok = audio_tok(c, idx);  // rescale_semantic_tokens (utils.rs:45-46)
        st->cur[0] = tok;
        if (tok == c.im_end_id) st->done = 1;  // batch_item_is_dead |= newly dead (:160-173)
    }
    if (po.epoch && b == 0 && tid == 0) po.epoch[0] += 1;
    if (po.g) block_prep_row(XF + (size_t)b * dim, dim, po, b, red4);
}

template <typename WT>
__global__ __launch_bounds__(SAMPLE_THREADS) void k_sample_fast_rows(const float* __restrict__ logits, int cb, int n_cb, int cb_size,
                                                                     const SampleCfg* __restrict__ cp, const RngState* __restrict__ master,
                                                                     int B, SeqState* __restrict__ states, const WT* __restrict__ fast_emb,
                                                                     float* __restrict__ XF, const WT* __restrict__ tok_emb,
                                                                     const WT* __restrict__ cb_emb, float* __restrict__ X, int dim,
                                                                     uint32_t* __restrict__ out_codes, int out_cap, PrepOut po) {
    __shared__ float red4[4];
    __shared__ __attribute__((aligned(16))) float lg[SAMPLE_MAXN];
    __shared__ __attribute__((aligned(16))) float sp[SAMPLE_MAXN];
    __shared__ __attribute__((aligned(16))) int si[SAMPLE_MAXN];
    __shared__ double red[SAMPLE_THREADS];
    __shared__ RngState lrng;
    const int tid = threadIdx.x, b = blockIdx.x, n = cb_size;
    SeqState* st = states + b;
    SampleCfg c = *cp;
    if (c.temp <= 1e-7f) c.temp = 0.f;
    // the batch repetition-penalty mask is never updated for Fish models (static_batch.rs:204-206): logits / 1.0
    for (int i = tid; i < n; i += SAMPLE_THREADS) lg[i] = logits[(size_t)b * n + i];
    __syncthreads();
    if (tid == SAMPLE_THREADS - 1 && c.temp != 0.f)  // (see k_sample_slow_rows: off wave 0's critical path)
        child_rng(master, ((unsigned long long)st->frame * (n_cb + 1) + 1 + cb) * B + b, &lrng);
    const int code = block_sample(lg, n, c, &lrng, sp, si, red, /*first_max=*/true);
    if (tid == 0) st->cur[cb + 1] = (uint32_t)code;
    if (cb != n_cb - 1) {
        for (int d = tid; d < dim; d += SAMPLE_THREADS) XF[(size_t)b * dim + d] = WTr<WT>::to_f32(fast_emb[(size_t)code * dim + d]);
        if (po.g) block_prep_row(XF + (size_t)b * dim, dim, po, b, red4);
        return;
    }
    rows_frame_commit<WT>(st, c, code, /*take_code=*/true, /*freeze=*/c.session != 0, b, n_cb, cb_size, tok_emb, cb_emb, X, dim, out_codes, out_cap,
                          SAMPLE_THREADS);
}

// ---- the batched samplers on the block-parallel sampler (lm_bsample_dev.h): 512 threads per row, for temp > 1e-7 with 0 < top_k <= 256
// (BASELINE configs[2]: top-k 256 / top-p 0.8).  The per-(call, row) child StdRng derivation -- two ChaCha12 blocks, the PCG expansion
// and the word of the draw: ~5 us of dependent integer work -- no longer hides behind a 13 us one-wave selection, so it runs once per
// step for all the step's calls: k_rows_rng_words, thread c of block b = call c of row b (the same master u64 numbers as above).
constexpr int ROWS_WORDS_LD = 16;
__global__ __launch_bounds__(64) void k_rows_rng_words(const RngState* __restrict__ master, int B, int calls_per_frame,
                                                       const SeqState* __restrict__ states, uint32_t* __restrict__ words) {
    const int b = blockIdx.x, c = threadIdx.x;
    if (c >= calls_per_frame) return;
    RngState child;
    child_rng(master, ((unsigned long long)states[b].frame * calls_per_frame + c) * B + b, &child);
    words[b * ROWS_WORDS_LD + c] = chacha12_word(child.key, 0);
}
constexpr int PAR_THREADS = 512;
template <typename WT>
__global__ __launch_bounds__(PAR_THREADS) void k_sample_slow_rows_par(const float* __restrict__ logits, int ld, int n, const SampleCfg* __restrict__ cp,
                                                                       const uint32_t* __restrict__ words, SeqState* __restrict__ states,
                                                                       const float* __restrict__ X, float* __restrict__ XF, int dim, PrepOut po) {
    __shared__ float red4[4];
    __shared__ BSampLds S;
    const int tid = threadIdx.x, b = blockIdx.x;
    SeqState* st = states + b;
    const SampleCfg c = *cp;
    float lv[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int i = tid * 4 + s;
        lv[s] = i < n ? logits[(size_t)b * ld + i] : 0.f;
        if (i == 0 && c.ignore_eos) lv[s] = -INFINITY;
    }
    for (int i = tid; i < dim; i += PAR_THREADS) XF[(size_t)b * dim + i] = X[(size_t)b * dim + i];  // hidden_states (:175)
    int used = 0;
    const int idx = bsample<PAR_THREADS, 4>(lv, n, c.top_k, (float)(1.0 / (double)c.temp), c.top_p, words[b * ROWS_WORDS_LD], &used, S, true, c.top_p64);
    if (tid == 0) {
        const uint32_t tok = audio_tok(c, idx);  // rescale_semantic_tokens (utils.rs:45-46)
        st->cur[0] = tok;
        if (tok == c.im_end_id) st->done = 1;  // batch_item_is_dead |= newly dead (:160-173)
    }
    if (po.epoch && b == 0 && tid == 0) po.epoch[0] += 1;
    if (po.g) block_prep_row(XF + (size_t)b * dim, dim, po, b, red4);
}
template <typename WT>
__global__ __launch_bounds__(PAR_THREADS) void k_sample_fast_rows_par(const float* __restrict__ logits, int cb, int n_cb, int cb_size,
                                                                       const SampleCfg* __restrict__ cp, const uint32_t* __restrict__ words, SeqState* __restrict__ states,
                                                                       const WT* __restrict__ fast_emb, float* __restrict__ XF, const WT* __restrict__ tok_emb,
                                                                       const WT* __restrict__ cb_emb, float* __restrict__ X, int dim,
                                                                       uint32_t* __restrict__ out_codes, int out_cap, PrepOut po) {
    __shared__ float red4[4];
    __shared__ BSampLds S;
    const int tid = threadIdx.x, b = blockIdx.x, n = cb_size;
    SeqState* st = states + b;
    const SampleCfg c = *cp;
    // the batch repetition-penalty mask is never updated for Fish models (static_batch.rs:204-206): logits / 1.0
    float lv[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) { const int i = tid * 2 + s; lv[s] = i < n ? logits[(size_t)b * n + i] : 0.f; }
    int used = 0;
    const int code = bsample<PAR_THREADS, 2>(lv, n, c.top_k, (float)(1.0 / (double)c.temp), c.top_p, words[b * ROWS_WORDS_LD + 1 + cb], &used, S, true, c.top_p64);
    if (tid == 0) st->cur[cb + 1] = (uint32_t)code;
    if (cb != n_cb - 1) {
        for (int d = tid; d < dim; d += PAR_THREADS) XF[(size_t)b * dim + d] = WTr<WT>::to_f32(fast_emb[(size_t)code * dim + d]);
        if (po.g) block_prep_row(XF + (size_t)b * dim, dim, po, b, red4);
        return;
    }
    rows_frame_commit<WT>(st, c, code, /*take_code=*/true, /*freeze=*/c.session != 0, b, n_cb, cb_size, tok_emb, cb_emb, X, dim, out_codes, out_cap,
                          PAR_THREADS);
}

// ---- per-slot samplers (fs_lm_session_begin with FS_SESSION_PER_SLOT): one block per session slot on the static-batch step, every decision
// that of the slot's OWN generate_blocking call (k_sample_slow / k_sample_fast above; single_batch.rs:102-210, sampling/mod.rs:51-75,
// rep_pen.rs:4-72): the slot's SampleCfg, one StdRng stream per slot whose consumed count lives on the device, the 16-deep repetition
// penalty window per codebook from the slot's second frame on, greedy iff temp == 0 with the LAST-max tie rule, top-p compared in f32, and
// no codebook decision (codes 0, nothing drawn, window untouched) once the slow token is <|im_end|>.  Everything is read through per-slot
// pointers, so one captured graph serves every mix of settings; greedy / sampled is a block-uniform branch.  A parked, frozen or
// finished slot (done != 0) decides nothing, draws nothing and leaves its generator state alone; it still writes finite fast-decoder
// input rows, because the step's GEMMs run over all rows.
// The block has one wave more than the sampler needs.  The StdRng word of a draw is one ChaCha12 block of dependent integer work; all
// PAR_THREADS threads take part in bsample's barriers, so none of them can compute it while the selection runs.  The extra wave does:
// while decision d selects, it derives the word decision d + 1 will most likely need (stream position consumed + 1) into the slot's
// look-ahead cell, tagged with that position, and ends (a terminated wave does not count at the block's barriers).  Decision d + 1 takes
// the cell when its tag equals the stream position and derives the word itself otherwise (first decision after activation, a draw that
// consumed nothing) -- the tag makes the look-ahead a pure latency matter, never one of correctness.
constexpr int SLOT_THREADS = PAR_THREADS + 64;
__device__ __forceinline__ void slot_word_ahead(SlotRng* rg, int next_decision, unsigned long long used = 1ull) {
    const unsigned long long at = rg->rng.consumed + used;
    rg->ahead_word[next_decision] = chacha12_word(rg->rng.key, at);
    rg->ahead_at[next_decision] = at;
}
__device__ __forceinline__ uint32_t slot_word(const SlotRng* rg, int decision, unsigned long long at) {
    if (rg->ahead_at[decision] == at) return rg->ahead_word[decision];
    return chacha12_word(rg->rng.key, at);  // (block-uniform: every thread derives the same word)
}
// greedy_pick's rule (host ArgMax: totalOrder, the LAST index among identical bit patterns) for bsample's blocked ownership (thread t owns candidates t * EPT ..): the
// block maximum of {order-preserving value bits : index}.  *s_key must have been zeroed before the previous barrier; one barrier.
template <int EPT>
__device__ __forceinline__ int slot_greedy_pick(const float (&lv)[EPT], int n, unsigned long long* s_key) {
    const int tid = threadIdx.x;
    unsigned long long key = 0ull;
#pragma unroll
    for (int s = 0; s < EPT; ++s) {
        const int i = tid * EPT + s;
        if (i < n) {
            uint32_t u = __float_as_uint(lv[s]);          // (the bit pattern as it is: -0 sorts below +0)
            u ^= (u >> 31) ? 0xFFFFFFFFu : 0x80000000u;  // unsigned order == total order
            const unsigned long long k = ((unsigned long long)u << 32) | (unsigned long long)(uint32_t)i;
            key = k > key ? k : key;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { const unsigned long long o = __shfl_xor(key, m, 64); key = o > key ? o : key; }
    if ((tid & 63) == 0) atomicMax(s_key, key);
    __syncthreads();
    return (int)(*s_key & 0xFFFFFFFFull);
}
// ---- the wide decision of a slot block (FS_SESSION_WIDE_SAMPLER): no top-k (top_k == 0 or >= n: nucleus-only) or 256 < top_k < n, over
// n <= NT * EPT <= 2048 candidates, by the NT threads of the block in bsample's blocked ownership (thread t owns candidates t * EPT ..) and with
// bsample's contract: `word` = the StdRng word the draw would consume, *consumed = 1 iff it did, the pick on every thread.  The arithmetic is
// block_sample's general path, operation for operation: lg * inv_t, block max, expf, the f64 denominator narrowed to f32, the division; the
// order (probability descending, index ascending); seq_sum over the kept probabilities in index order (top-k only; entries outside the
// top-k weigh +0.0, which moves no f32 sum); seq_topp_cut along the descending order; block_weighted_pick's cumulative chain over all n
// weights in index order.  Only the sort is organised differently: one 64-bit key {probability bits : ~index} per candidate (probabilities
// are >= +0, so the bit patterns order like the values, and a larger key sorts FIRST: higher probability, then lower index), every thread
// taking np2 / (2 NT) compare-exchanges per bitonic stage.  The two chains that do not depend on each other (the index-order sum, the
// descending top-p walk) run at the same time on lanes of two different waves.
struct alignas(16) WideLds {  // 32.2 KB
    unsigned long long key[2048];  // sort keys; [r] = rank r of the descending order once sorted
    float p[2048];                 // probabilities by index; zeroed outside the top-k and behind the top-p cut: the draw's weights
    float sp[2048];                // probabilities in descending order; then the draw's cumulative weights
    double wsum[16];
    float wmax[16];
    float sum_p;
    int cut;
};
template <int NT, int EPT>
__device__ int wide_sample(const float (&lv)[EPT], int n, int top_k, float inv_t, float top_p, uint32_t word, int* consumed, WideLds& W) {
    static_assert(NT % 64 == 0 && NT >= 128 && NT * EPT <= 2048, "block shape");
    constexpr int NW = NT / 64;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int base = tid * EPT;
    // softmax(logits * (1 / temp)), as bsample phase A
    float v[EPT];
    float mx = -INFINITY;
#pragma unroll
    for (int s = 0; s < EPT; ++s) {
        v[s] = (base + s < n) ? lv[s] * inv_t : -INFINITY;
        mx = fmaxf(mx, v[s]);
    }
    mx = bs_wave_max(mx);
    if (lane == 0) W.wmax[wv] = mx;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < NW; ++w) mx = fmaxf(mx, W.wmax[w]);
    double part = 0.0;
#pragma unroll
    for (int s = 0; s < EPT; ++s) {
        v[s] = (base + s < n) ? expf(v[s] - mx) : 0.f;
        part += (double)v[s];
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) part += __shfl_xor(part, m, 64);
    if (lane == 0) W.wsum[wv] = part;
    __syncthreads();
    double dsum = 0.0;
#pragma unroll
    for (int w = 0; w < NW; ++w) dsum += W.wsum[w];
    const float denom = (float)dsum;
    int np2 = 1;
    while (np2 < n) np2 <<= 1;  // <= NT * EPT (a power of two)
#pragma unroll
    for (int s = 0; s < EPT; ++s) {
        const int i = base + s;
        if (i < n) {
            const float pr = v[s] / denom;
            W.p[i] = pr;
            W.key[i] = ((unsigned long long)__float_as_uint(pr) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)i);
        } else if (i < np2) {
            W.key[i] = 0ull;  // behind every candidate (a candidate's low word is never 0)
        }
    }
    __syncthreads();
    // bitonic sort, descending: np2 / 2 compare-exchanges per stage, pair q = (i, i | j) with bit j of i clear
    for (int k = 2; k <= np2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int q = tid; q < (np2 >> 1); q += NT) {
                const int i = ((q & ~(j - 1)) << 1) | (q & (j - 1)), ixj = i | j;
                const unsigned long long a = W.key[i], b = W.key[ixj];
                const bool up = (i & k) == 0;
                if ((a > b) != up) { W.key[i] = b; W.key[ixj] = a; }
            }
            __syncthreads();
        }
    }
    const bool use_k = top_k > 0 && top_k < n;
    const int kk = use_k ? top_k : n;
    for (int r = tid; r < n; r += NT) {
        const unsigned long long kr = W.key[r];
        W.sp[r] = __uint_as_float((uint32_t)(kr >> 32));
        if (r >= kk) W.p[0xFFFFFFFFu - (uint32_t)kr] = 0.f;  // outside the top-k (ties at the boundary: the lower index was kept)
    }
    __syncthreads();
    // the index-order sum of the kept probabilities (top-k only: it decides whether top-p applies at all) and the descending top-p walk
    if (tid == 0) W.sum_p = use_k ? seq_sum(W.p, n) : 0.f;
    if (tid == 64) W.cut = seq_topp_cut(W.sp, kk, top_p);
    __syncthreads();
    const bool do_topp = !use_k || !(top_p <= 0.f || top_p >= W.sum_p);
    const int cut = do_topp ? W.cut : kk;
    if (cut < kk) {  // entries sorting at or after rank `cut` are zeroed: a parallel predicate on the keys
        const unsigned long long kc = W.key[cut];
        for (int j = tid; j < n; j += NT) {
            const unsigned long long kj = ((unsigned long long)__float_as_uint(W.p[j]) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)j);
            if (kj <= kc) W.p[j] = 0.f;
        }
    }
    __syncthreads();
    int drew = 0;
    const int res = block_weighted_pick_nt<NT>(W.p, n, W.sp, word, &drew);
    *consumed = drew;
    return res;
}
// one sampled (temp > 0) decision of a slot in a wide session: the block-uniform choice between the two samplers
template <int EPT>
__device__ __forceinline__ int slot_sample_wide(const float (&lv)[EPT], int n, const SampleCfg& c, uint32_t word, int* used, BSampLds& S, WideLds& W) {
    const float inv_t = (float)(1.0 / (double)c.temp);
    if (c.top_k == 0 || c.top_k > BS_MAXK || c.top_k >= n) return wide_sample<PAR_THREADS, EPT>(lv, n, c.top_k, inv_t, c.top_p, word, used, W);
    return bsample<PAR_THREADS, EPT>(lv, n, c.top_k, inv_t, c.top_p, word, used, S);
}
template <typename WT, bool WIDE>
__global__ __launch_bounds__(SLOT_THREADS) void k_sample_slow_slots(const float* __restrict__ logits, int ld, int n, const SampleCfg* __restrict__ cfgs,
                                                                     SlotRng* __restrict__ rngs, SeqState* __restrict__ states,
                                                                     const float* __restrict__ X, float* __restrict__ XF, int dim, PrepOut po,
                                                                     float* __restrict__ cap, int cap_frames) {
    __shared__ float red4[4];
    __shared__ BSampLds S;
    __shared__ unsigned long long s_key;
    const int tid = threadIdx.x, b = blockIdx.x;
    SeqState* st = states + b;
    SlotRng* rg = rngs + b;
    const bool live = st->done == 0;
    const float temp = cfgs[b].temp;
    if (tid >= PAR_THREADS) {  // the look-ahead wave (see above); a legacy slow draw takes exactly one word, like a sampled one
        if (tid == PAR_THREADS && live && temp != 0.f) slot_word_ahead(rg, 1);
        return;
    }
    const SampleCfg c = cfgs[b];
    if (tid == 0) s_key = 0ull;
    for (int i = tid; i < dim; i += PAR_THREADS) XF[(size_t)b * dim + i] = X[(size_t)b * dim + i];  // hidden_states -> fast decoder input
    if (live && c.legacy) {
        // Fish <= 1.4 (legacy_draw; single_batch.rs:104-124): the head rows are [pad, im_end]; the draw takes ONE word of the slot's stream
        // per live frame at every temperature, greedy included.  Block-uniform branch (every slot of a handle shares the token layout).
        if (tid == 0) {
            const float pad = logits[(size_t)b * ld], eos = logits[(size_t)b * ld + 1];
            const unsigned long long at = rg->rng.consumed;
            const uint32_t w = slot_word(rg, 0, at);
            rg->rng.consumed = at + 1ull;
            const LegacyDraw dr = legacy_draw(pad, eos, w, c.ignore_eos);
            const uint32_t tok = dr.is_pad ? c.pad_id : c.im_end_id;
            st->cur[0] = tok;
            if (tok == c.im_end_id) st->done = 1;  // the frame's codebook decisions are skipped; the slot freezes at the end of the frame
            if (cap && st->frame < cap_frames) {  // (fs_lm_debug_capture: the two logits, the uniform draw, the pick -- k_fast_persist's record)
                float* rec = cap + ((size_t)b * cap_frames + st->frame) * 9 * 2048;
                rec[0] = pad; rec[1] = eos; rec[2] = dr.u; rec[2047] = dr.is_pad ? 0.f : 1.f;
            }
        }
    } else if (live) {
        float lv[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int i = tid * 4 + s;
            lv[s] = i < n ? logits[(size_t)b * ld + i] : 0.f;
            if (i == 0 && c.ignore_eos) lv[s] = -INFINITY;
        }
        int idx;
        if (temp == 0.f) {
            __syncthreads();  // s_key
            idx = slot_greedy_pick<4>(lv, n, &s_key);
        } else {
            const unsigned long long at = rg->rng.consumed;
            const uint32_t word = slot_word(rg, 0, at);
            int used = 0;
            if constexpr (WIDE) {
                __shared__ WideLds Wd;
                idx = slot_sample_wide<4>(lv, n, c, word, &used, S, Wd);
            } else {
                idx = bsample<PAR_THREADS, 4>(lv, n, c.top_k, (float)(1.0 / (double)c.temp), c.top_p, word, &used, S);
            }
            if (tid == 0) rg->rng.consumed = at + (unsigned long long)used;
        }
        if (tid == 0) {
            const uint32_t tok = audio_tok(c, idx);  // rescale_semantic_tokens (utils.rs:45-46)
            st->cur[0] = tok;
            if (tok == c.im_end_id) st->done = 1;  // the frame's codebook decisions are skipped; the slot freezes at the end of the frame
        }
    }
    if (po.epoch && b == 0 && tid == 0) po.epoch[0] += 1;
    if (po.g) block_prep_row(XF + (size_t)b * dim, dim, po, b, red4);
}
template <typename WT, bool WIDE>
__global__ __launch_bounds__(SLOT_THREADS) void k_sample_fast_slots(const float* __restrict__ logits, int cb, int n_cb, int cb_size,
                                                                     const SampleCfg* __restrict__ cfgs, SlotRng* __restrict__ rngs, RepPenState rp,
                                                                     SeqState* __restrict__ states, const WT* __restrict__ fast_emb, float* __restrict__ XF,
                                                                     const WT* __restrict__ tok_emb, const WT* __restrict__ cb_emb, float* __restrict__ X,
                                                                     int dim, uint32_t* __restrict__ out_codes, int out_cap, PrepOut po) {
    __shared__ float red4[4];
    __shared__ BSampLds S;
    __shared__ unsigned long long s_key;
    const int tid = threadIdx.x, b = blockIdx.x, n = cb_size;
    SeqState* st = states + b;
    SlotRng* rg = rngs + b;
    // done != 0: parked / frozen / finished, or this frame's slow token was <|im_end|> (single_batch.rs:153-156: push 0, skip the fast step)
    const bool live = st->done == 0;
    const float temp = cfgs[b].temp;
    if (tid >= PAR_THREADS) {  // the look-ahead wave: the next decision is codebook cb + 1, or the next frame's slow token
        if (tid == PAR_THREADS && live && temp != 0.f) slot_word_ahead(rg, cb == n_cb - 1 ? 0 : cb + 2);
        // (a greedy Fish <= 1.4 slot still draws its slow word: this greedy decision consumes none, so the word sits at `consumed` itself)
        else if (tid == PAR_THREADS && live && cb == n_cb - 1 && cfgs[b].legacy) slot_word_ahead(rg, 0, 0ull);
        return;
    }
    const SampleCfg c = cfgs[b];
    if (tid == 0) s_key = 0ull;
    int code = 0;
    if (live) {
        // the slot's RepPenState of this codebook: mask [slot][n_cb][cb_size], ring [slot][n_cb][17], meta [slot][n_cb][2]
        const size_t sc = (size_t)b * n_cb + cb;
        float* mask = rp.mask + sc * cb_size;
        int* ring = rp.ring + sc * 17;
        int* meta = rp.ring_meta + sc * 2;
        const bool pen = st->have_prev != 0;
        // the repetition-penalty window (RepPenPlan) of the slot's ring, read here and written behind the decision's barriers
        const RepPenPlan win = reppen_plan(pen, st->prev[cb + 1], ring, meta);
        float lv[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int i = tid * 2 + s;
            lv[s] = 0.f;
            if (i < n) {
                lv[s] = logits[(size_t)b * n + i];
                if (pen) {
                    const float m0 = mask[i], m = win.apply(i, m0, c.rep_pen);
                    if (m != m0) mask[i] = m;
                    lv[s] = lv[s] / m;
                }
            }
        }
        if (temp == 0.f) {
            __syncthreads();  // s_key
            code = slot_greedy_pick<2>(lv, n, &s_key);
        } else {
            const unsigned long long at = rg->rng.consumed;
            const uint32_t word = slot_word(rg, 1 + cb, at);
            int used = 0;
            if constexpr (WIDE) {
                __shared__ WideLds Wd;
                code = slot_sample_wide<2>(lv, n, c, word, &used, S, Wd);
            } else {
                code = bsample<PAR_THREADS, 2>(lv, n, c.top_k, (float)(1.0 / (double)c.temp), c.top_p, word, &used, S);
            }
            if (tid == 0) rg->rng.consumed = at + (unsigned long long)used;
        }
        if (tid == 0) {
            if (pen) { ring[win.head] = win.last; meta[0] = win.head; meta[1] = win.drop ? 16 : win.len; }
            st->cur[cb + 1] = (uint32_t)code;  // (also the next pass's qkv-table row)
        }
    }
    if (cb != n_cb - 1) {
        for (int d = tid; d < dim; d += PAR_THREADS) XF[(size_t)b * dim + d] = WTr<WT>::to_f32(fast_emb[(size_t)code * dim + d]);
        if (po.g) block_prep_row(XF + (size_t)b * dim, dim, po, b, red4);
        return;
    }
    // a slot that decided nothing in this launch (done != 0) keeps its last code; the frozen-slot rule always applies
    rows_frame_commit<WT>(st, c, code, /*take_code=*/live, /*freeze=*/true, b, n_cb, cb_size, tok_emb, cb_emb, X, dim, out_codes, out_cap, PAR_THREADS);
}

// test hook of the block-parallel sampler (lm_bsample_dev.h) with the static-batch RNG derivation of k_sample_slow_rows
template <int NT, int EPT>
__global__ __launch_bounds__(NT) void k_bsample_rows_test(const float* __restrict__ logits, int n, const SampleCfg* __restrict__ cp,
                                                          const RngState* __restrict__ master, int B, int call, uint32_t* __restrict__ out) {
    __shared__ BSampLds S;
    __shared__ RngState lrng;
    __shared__ uint32_t s_word;
    const int tid = threadIdx.x, b = blockIdx.x;
    const SampleCfg c = *cp;
    float lv[EPT];
#pragma unroll
    for (int s = 0; s < EPT; ++s) { const int i = tid * EPT + s; lv[s] = i < n ? logits[(size_t)b * n + i] : 0.f; }
    if (tid == NT - 1) { child_rng(master, (unsigned long long)call * B + b, &lrng); s_word = chacha12_word(lrng.key, 0); }
    __syncthreads();
    int consumed = 0;
    const int idx = bsample<NT, EPT>(lv, n, c.top_k, (float)(1.0 / (double)c.temp), c.top_p, s_word, &consumed, S, /*batch=*/true, c.top_p64);
    if (tid == 0) out[b] = (uint32_t)idx;
}

// test hook of the per-slot decision of a wide session (fs_selftest_sample_slots): block b is one slot -- its own StdRng stream, its own
// settings -- making R decisions in order on caller-provided rows; greedy, bsample or wide_sample exactly as k_sample_*_slots<.., true> choose
template <int EPT>
__global__ __launch_bounds__(PAR_THREADS) void k_sample_slots_test(const float* __restrict__ logits, int R, int n, const SampleCfg* __restrict__ cfgs,
                                                                   const unsigned long long* __restrict__ seeds, uint32_t* __restrict__ out,
                                                                   unsigned long long* __restrict__ words_used) {
    __shared__ BSampLds S;
    __shared__ WideLds Wd;
    __shared__ unsigned long long s_key;
    __shared__ uint32_t s_rkey[8];
    const int tid = threadIdx.x, b = blockIdx.x;
    const SampleCfg c = cfgs[b];
    if (tid == 0) seed_from_u64(seeds[b], s_rkey);
    __syncthreads();
    uint32_t key[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) key[i] = s_rkey[i];
    unsigned long long at = 0ull;
    for (int r = 0; r < R; ++r) {
        const float* row = logits + ((size_t)b * R + r) * n;
        float lv[EPT];
#pragma unroll
        for (int s = 0; s < EPT; ++s) { const int i = tid * EPT + s; lv[s] = i < n ? row[i] : 0.f; }
        int idx;
        if (c.temp == 0.f) {
            if (tid == 0) s_key = 0ull;
            __syncthreads();
            idx = slot_greedy_pick<EPT>(lv, n, &s_key);
            __syncthreads();  // (the next decision zeroes s_key)
        } else {
            const uint32_t word = chacha12_word(key, at);  // (block-uniform)
            int used = 0;
            idx = slot_sample_wide<EPT>(lv, n, c, word, &used, S, Wd);
            at += (unsigned long long)used;
        }
        if (tid == 0) out[(size_t)b * R + r] = (uint32_t)idx;
    }
    if (tid == 0) words_used[b] = at;
}

__global__ void k_reppen_reset(RepPenState rp, int n_cb, int cb_size) {
    const int n = n_cb * cb_size;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) { rp.mask[i] = 1.0f; rp.seen[i] = 0; }
    if (blockIdx.x == 0 && threadIdx.x < n_cb) { rp.ring_meta[threadIdx.x * 2] = 0; rp.ring_meta[threadIdx.x * 2 + 1] = 0; }
}

// ================================================================================================ launchers
#define FS_LAUNCH_CHECK() FS_HIP(hipGetLastError())

template <typename WT>
void SampleKernels<WT>::sample_slow(const ModelDims& d, const float* logits, int n, const SampleCfg* c, RngState* rng,
                                    SeqState* state, const float* x, float* xf, hipStream_t st, float* const* hid_slot) {
    FS_REQUIRE(n <= SAMPLE_MAXN, "audio-range vocabulary larger than the sampler capacity");
    hipLaunchKernelGGL((k_sample_slow<KVT<WT>>), dim3(1), dim3(SAMPLE_THREADS), 0, st, logits, n, c, rng, state, x, xf, d.dim, hid_slot);
    FS_LAUNCH_CHECK();
}

template <typename WT>
void SampleKernels<WT>::sample_fast(const ModelDims& d, const float* logits, int cb, int n_cb, int cb_size, const SampleCfg* c,
                                    RngState* rng, RepPenState rp, SeqState* state, const void* fast_emb, float* xf,
                                    const void* tok_emb, const void* cb_emb, float* x, uint32_t* out_codes, int out_cap,
                                    hipStream_t st) {
    FS_REQUIRE(cb_size <= SAMPLE_MAXN, "codebook larger than the sampler capacity");
    hipLaunchKernelGGL((k_sample_fast<KVT<WT>>), dim3(1), dim3(SAMPLE_THREADS), 0, st, logits, cb, n_cb, cb_size, c, rng, rp, state,
                       (const KVT<WT>*)fast_emb, xf, (const KVT<WT>*)tok_emb, (const KVT<WT>*)cb_emb, x, d.dim, out_codes, out_cap);
    FS_LAUNCH_CHECK();
}

template <typename WT>
void SampleKernels<WT>::rows_rng_words(const RngState* master, int B, int calls_per_frame, const SeqState* states, uint32_t* words, hipStream_t st) {
    FS_REQUIRE(calls_per_frame <= ROWS_WORDS_LD, "too many sample() calls per frame");
    hipLaunchKernelGGL(k_rows_rng_words, dim3(B), dim3(64), 0, st, master, B, calls_per_frame, states, words);
    FS_LAUNCH_CHECK();
}
// the row / slot samplers' optional RMSNorm + hi/lo split of the row they leave for the fast decoder (block_prep_row: one float4 per thread)
static PrepOut prep_out(const ModelDims& d, const float* prep_g, uint16_t* prep_A, uint32_t* epoch) {
    FS_REQUIRE(!prep_g || (d.dim <= 1024 && d.dim % 4 == 0), "sampler-side RMSNorm of the next input row: dim <= 1024");
    return PrepOut{prep_g, d.eps, prep_A, epoch};
}
bool rows_par_sampler_ok(double temp, uint64_t top_k, int n_slow, int cb_size) {
    return temp > 1e-7 && top_k > 0 && top_k <= (uint64_t)BS_MAXK && (int)top_k < cb_size && (int)top_k < n_slow && n_slow <= 2048 && cb_size <= 1024;
}
template <typename WT>
void SampleKernels<WT>::sample_slow_rows(const ModelDims& d, const float* logits, int ld, int n, const SampleCfg* c, const RngState* master,
                                         int B, int calls_per_frame, SeqState* states, const float* X, float* XF, hipStream_t st, const uint32_t* words,
                                         const float* prep_g, uint16_t* prep_A, uint32_t* epoch) {
    FS_REQUIRE(n <= SAMPLE_MAXN, "audio-range vocabulary larger than the sampler capacity");
    const PrepOut po = prep_out(d, prep_g, prep_A, epoch);
    if (words) {
        hipLaunchKernelGGL((k_sample_slow_rows_par<KVT<WT>>), dim3(B), dim3(PAR_THREADS), 0, st, logits, ld, n, c, words, states, X, XF, d.dim, po);
        FS_LAUNCH_CHECK();
        return;
    }
    hipLaunchKernelGGL((k_sample_slow_rows<KVT<WT>>), dim3(B), dim3(SAMPLE_THREADS), 0, st, logits, ld, n, c, master, B, calls_per_frame, states,
                       X, XF, d.dim, po);
    FS_LAUNCH_CHECK();
}
template <typename WT>
void SampleKernels<WT>::sample_fast_rows(const ModelDims& d, const float* logits, int cb, int n_cb, int cb_size, const SampleCfg* c,
                                         const RngState* master, int B, SeqState* states, const void* fast_emb, float* XF,
                                         const void* tok_emb, const void* cb_emb, float* X, uint32_t* out_codes, int out_cap,
                                         hipStream_t st, const uint32_t* words, const float* prep_g, uint16_t* prep_A) {
    FS_REQUIRE(cb_size <= SAMPLE_MAXN, "codebook larger than the sampler capacity");
    const PrepOut po = prep_out(d, prep_g, prep_A, nullptr);
    if (words) {
        hipLaunchKernelGGL((k_sample_fast_rows_par<KVT<WT>>), dim3(B), dim3(PAR_THREADS), 0, st, logits, cb, n_cb, cb_size, c, words, states,
                           reinterpret_cast<const KVT<WT>*>(fast_emb), XF, reinterpret_cast<const KVT<WT>*>(tok_emb), reinterpret_cast<const KVT<WT>*>(cb_emb), X, d.dim,
                           out_codes, out_cap, po);
        FS_LAUNCH_CHECK();
        return;
    }
    hipLaunchKernelGGL((k_sample_fast_rows<KVT<WT>>), dim3(B), dim3(SAMPLE_THREADS), 0, st, logits, cb, n_cb, cb_size, c, master, B, states,
                       (const KVT<WT>*)fast_emb, XF, (const KVT<WT>*)tok_emb, (const KVT<WT>*)cb_emb, X, d.dim, out_codes, out_cap, po);
    FS_LAUNCH_CHECK();
}

template <typename WT>
void SampleKernels<WT>::sample_slow_slots(const ModelDims& d, const float* logits, int ld, int n, const SampleCfg* cfgs, SlotRng* rngs, int B,
                                          SeqState* states, const float* X, float* XF, hipStream_t st, const float* prep_g, uint16_t* prep_A,
                                          uint32_t* epoch, float* cap, int cap_frames, bool wide) {
    FS_REQUIRE(n <= PAR_THREADS * 4 && n <= ld && n >= 2, "audio-range vocabulary outside the per-slot sampler capacity (2 .. 2048)");
    const PrepOut po = prep_out(d, prep_g, prep_A, epoch);
    if (wide)
        hipLaunchKernelGGL((k_sample_slow_slots<KVT<WT>, true>), dim3(B), dim3(SLOT_THREADS), 0, st, logits, ld, n, cfgs, rngs, states, X, XF, d.dim, po,
                           cap, cap_frames);
    else
        hipLaunchKernelGGL((k_sample_slow_slots<KVT<WT>, false>), dim3(B), dim3(SLOT_THREADS), 0, st, logits, ld, n, cfgs, rngs, states, X, XF, d.dim, po,
                           cap, cap_frames);
    FS_LAUNCH_CHECK();
}
template <typename WT>
void SampleKernels<WT>::sample_fast_slots(const ModelDims& d, const float* logits, int cb, int n_cb, int cb_size, const SampleCfg* cfgs,
                                          SlotRng* rngs, RepPenState rp, int B, SeqState* states, const void* fast_emb, float* XF,
                                          const void* tok_emb, const void* cb_emb, float* X, uint32_t* out_codes, int out_cap, hipStream_t st,
                                          const float* prep_g, uint16_t* prep_A, bool wide) {
    FS_REQUIRE(cb_size <= PAR_THREADS * 2 && n_cb + 1 <= 16, "codebook larger than the per-slot sampler capacity (1024)");
    const PrepOut po = prep_out(d, prep_g, prep_A, nullptr);
    if (wide)
        hipLaunchKernelGGL((k_sample_fast_slots<KVT<WT>, true>), dim3(B), dim3(SLOT_THREADS), 0, st, logits, cb, n_cb, cb_size, cfgs, rngs, rp, states,
                           reinterpret_cast<const KVT<WT>*>(fast_emb), XF, reinterpret_cast<const KVT<WT>*>(tok_emb),
                           reinterpret_cast<const KVT<WT>*>(cb_emb), X, d.dim, out_codes, out_cap, po);
    else
        hipLaunchKernelGGL((k_sample_fast_slots<KVT<WT>, false>), dim3(B), dim3(SLOT_THREADS), 0, st, logits, cb, n_cb, cb_size, cfgs, rngs, rp, states,
                           reinterpret_cast<const KVT<WT>*>(fast_emb), XF, reinterpret_cast<const KVT<WT>*>(tok_emb),
                           reinterpret_cast<const KVT<WT>*>(cb_emb), X, d.dim, out_codes, out_cap, po);
    FS_LAUNCH_CHECK();
}

void launch_reppen_reset(RepPenState rp, int n_cb, int cb_size, hipStream_t st) {
    hipLaunchKernelGGL(k_reppen_reset, dim3(8), dim3(256), 0, st, rp, n_cb, cb_size);
    FS_LAUNCH_CHECK();
}

// ---- decision capture on the row path (fs_lm_debug_capture for generate_static_batch / sessions): what every row's decision saw and picked,
// in the layout of the request-row kernels' record: cap[row][cap_frames][9][2048], logits at [0, n), the pick at [2047] (slow) / [1024] (fast)
__global__ __launch_bounds__(256) void k_cap_rows_logits(const float* __restrict__ logits, int ld, int n, const SeqState* __restrict__ states,
                                                         const SampleCfg* __restrict__ cp, float* __restrict__ cap, int cap_frames, int decision) {
    const int b = blockIdx.x, frame = states[b].frame;
    if (frame >= cap_frames) return;
    // Fish <= 1.4 slots (per-slot sessions): the slow sampler records its own 2-way decision; a slot that is done (this frame's slow token
    // was <|im_end|>, or frozen since) decides nothing, and its frame counter no longer moves: leave the terminating frame's record alone
    if (cp->legacy && (decision == 0 || states[b].done != 0)) return;
    float* dst = cap + (((size_t)b * cap_frames + frame) * 9 + decision) * 2048;
    for (int i = threadIdx.x; i < n; i += 256) {
        float v = logits[(size_t)b * ld + i];
        if (decision == 0 && i == 0 && cp->ignore_eos) v = -INFINITY;  // (what the slow samplers do to <|im_end|> before they select)
        dst[i] = v;
    }
}
__global__ __launch_bounds__(64) void k_cap_rows_picks(const SeqState* __restrict__ states, const SampleCfg* __restrict__ cp, float* __restrict__ cap,
                                                       int cap_frames, int n_cb) {
    const int b = blockIdx.x, frame = states[b].frame - 1, t = threadIdx.x;  // (the last sampler of the frame advanced the counter)
    if (frame < 0 || frame >= cap_frames || t > n_cb) return;
    float* dst = cap + (((size_t)b * cap_frames + frame) * 9 + t) * 2048;
    const uint32_t v = states[b].cur[t];
    if (t == 0 && cp->legacy) return;  // (recorded by the slow sampler itself: index 0 pad, 1 im_end)
    if (t == 0) dst[2047] = v == cp->im_end_id ? 0.f : (float)(v - cp->audio_base);
    else dst[1024] = (float)v;
}
void launch_cap_rows_logits(const float* logits, int ld, int n, const SeqState* states, const SampleCfg* cfg, int B, float* cap, int cap_frames, int decision,
                            hipStream_t st) {
    hipLaunchKernelGGL(k_cap_rows_logits, dim3(B), dim3(256), 0, st, logits, ld, n, states, cfg, cap, cap_frames, decision);
}
void launch_cap_rows_picks(const SeqState* states, const SampleCfg* cfg, int B, float* cap, int cap_frames, int n_cb, hipStream_t st) {
    hipLaunchKernelGGL(k_cap_rows_picks, dim3(B), dim3(64), 0, st, states, cfg, cap, cap_frames, n_cb);
}

// ---- scoring slots of a FS_SESSION_SCORE session (fishrt.h: fs_lm_session_add_scored): one node in front of each of the step's 9 per-slot
// sampler nodes.  Block b scores the row its slot's sampler is about to read against the slot's forced target -- f32 log-softmax entry of
// the target, of the maximum, the LAST maximal index (slot_greedy_pick's rule and key) -- and then stores +INFINITY over the target's
// logit, so the (unchanged, greedy) sampler node behind it picks the target and does the frame bookkeeping as for any slot.
// 256 threads, thread t owns the float4 groups at 4 t and 1024 + 4 t (n <= 2048); a group is one 16-byte load where the row start is
// 16-byte aligned and the group lies inside [0, n), guarded scalar loads otherwise.  Two barriers (max key, sum), each behind one
// __shfl_xor wave reduction and a 4-entry LDS array every thread folds itself.  All 256 threads take the same path.
constexpr int SCORE_THREADS = 256;
struct ScoreOut { float logprob, top_logprob, eos_logprob; uint32_t top; };
// What a scoring and a traced decision share: the row in the thread's registers (lv: the blocked ownership above; entries at or beyond n
// hold -inf, candidate 0 too when it is left out), its maximum m by the LAST-max key, log(sum exp(x - m)), the maximal index.  m, ls and
// top are the row's on every thread; x0 (candidate 0 as scored) is thread 0's.
// ALTS (the FS_SESSION_ALTS instantiation of the node): the exp pass also sums exp(x - m) (x - m) over the finite entries, and
// ent = log(s) - that sum / s is the row's entropy on every thread.  Without ALTS the function is what it was, instruction for instruction.
struct RowStats { float m, ls, x0; uint32_t top; float ent; };
template <bool ALTS = false>
__device__ __forceinline__ RowStats score_row_stats(const float* __restrict__ row, int n, bool exclude0, float (&lv)[8]) {
    __shared__ unsigned long long s_k[SCORE_THREADS / 64];
    __shared__ float s_s[SCORE_THREADS / 64];
    __shared__ float s_e[ALTS ? SCORE_THREADS / 64 : 1];
    const int tid = threadIdx.x;
    const bool vec = (reinterpret_cast<uintptr_t>(row) & 15u) == 0;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        const int i0 = g * (SCORE_THREADS * 4) + tid * 4;
        if (vec && i0 + 3 < n) {
            const float4 v = *reinterpret_cast<const float4*>(row + i0);
            lv[g * 4 + 0] = v.x; lv[g * 4 + 1] = v.y; lv[g * 4 + 2] = v.z; lv[g * 4 + 3] = v.w;
        } else {
#pragma unroll
            for (int s = 0; s < 4; ++s) lv[g * 4 + s] = i0 + s < n ? row[i0 + s] : -INFINITY;
        }
    }
    if (tid == 0 && exclude0) lv[0] = -INFINITY;
    unsigned long long key = 0ull;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const int i = (s >> 2) * (SCORE_THREADS * 4) + tid * 4 + (s & 3);
        if (i < n) {
            uint32_t u = __float_as_uint(lv[s] + 0.f);  // (-0 -> +0: equal values, the later index wins)
            u ^= (u >> 31) ? 0xFFFFFFFFu : 0x80000000u;  // unsigned order == float order
            const unsigned long long k = ((unsigned long long)u << 32) | (unsigned long long)(uint32_t)i;
            key = k > key ? k : key;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { const unsigned long long o = __shfl_xor(key, m, 64); key = o > key ? o : key; }
    if ((tid & 63) == 0) s_k[tid >> 6] = key;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < SCORE_THREADS / 64; ++w) { const unsigned long long o = s_k[w]; key = o > key ? o : key; }
    uint32_t mu = (uint32_t)(key >> 32);
    mu ^= (mu >> 31) ? 0x80000000u : 0xFFFFFFFFu;
    RowStats r;
    r.m = __uint_as_float(mu);
    float sum = 0.f, esum = 0.f;
    if constexpr (ALTS) {
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const float dx = lv[s] - r.m, e = expf(dx);
            sum += e;
            esum += lv[s] == -INFINITY ? 0.f : e * dx;  // (a -inf entry contributes exactly 0, not 0 * -inf)
        }
    } else {
#pragma unroll
        for (int s = 0; s < 8; ++s) sum += expf(lv[s] - r.m);  // (owned entries at or beyond n hold -inf: +0)
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if constexpr (ALTS) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) esum += __shfl_xor(esum, o, 64);
    }
    if ((tid & 63) == 0) { s_s[tid >> 6] = sum; if constexpr (ALTS) s_e[tid >> 6] = esum; }
    __syncthreads();
    sum = (s_s[0] + s_s[1]) + (s_s[2] + s_s[3]);
    r.ls = logf(sum);
    r.ent = 0.f;
    if constexpr (ALTS) r.ent = r.ls - ((s_e[0] + s_e[1]) + (s_e[2] + s_e[3])) / sum;
    r.x0 = lv[0];
    r.top = (uint32_t)(key & 0xFFFFFFFFull);
    return r;
}
// ---- the alternatives of a FS_SESSION_ALTS session (fishrt.h: fs_lm_session_poll_alts): the N <= ALTS_MAX largest candidates of the row
// in lv (score_row_stats' ownership), by the node's own key -- value descending, -0 == +0, the HIGHER index first among equals -- with the
// node's log-prob expression (x - m) - log s.  ONE barrier on top of score_row_stats' two: each of the 4 waves extracts its own top N
// with wave-only key reductions, the owner lane dropping the winner from its registers each round, and parks N {key, x} pairs in LDS
// arrays of its own; then wave 0 holds the 4 N <= 64 pairs one per lane, and a lane whose key has fewer than N larger ones among them
// stores its pair as the alternative of that rank.  A key of 0 is "no candidate" (entries at or beyond n, candidate 0 when it is left
// out; no finite or infinite value has the key 0); the ranks behind the last candidate get the padding, 0xFFFFFFFF / NaN.  All 256
// threads take the same path; n_alts is block-uniform; once per launch.
constexpr int ALTS_MAX = 16;
// the maximum of a 64-bit key over the wave, on every lane: an all-VALU butterfly (the DPP controls and lane swaps of
// lm_persist_rows.hip's pr_wave_max_*: xor 1, xor 2, half mirror, row mirror, then the 16- and 32-lane swaps), both words moved with the
// same control.  A round of the selection is this reduction and little else, and the LDS crossbar form (__shfl_xor: 12 ds_bpermute
// round trips per key) measured 1.1 us per round and node.
template <int CTRL>
__device__ __forceinline__ unsigned long long key_max_dpp(unsigned long long k) {
    const uint32_t hi = (uint32_t)__builtin_amdgcn_mov_dpp((int)(uint32_t)(k >> 32), CTRL, 0xF, 0xF, false);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_mov_dpp((int)(uint32_t)k, CTRL, 0xF, 0xF, false);
    const unsigned long long o = ((unsigned long long)hi << 32) | lo;
    return o > k ? o : k;
}
__device__ __forceinline__ unsigned long long wave_max_key(unsigned long long k) {
    constexpr int XOR1 = 0xB1, XOR2 = 0x4E, HALF_MIRROR = 0x141, MIRROR = 0x140;
    k = key_max_dpp<XOR1>(k); k = key_max_dpp<XOR2>(k); k = key_max_dpp<HALF_MIRROR>(k); k = key_max_dpp<MIRROR>(k);
    {
        const uint32_t hi = (uint32_t)(k >> 32), lo = (uint32_t)k;
        const auto rh = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
        const auto rl = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
        const unsigned long long a = ((unsigned long long)rh[0] << 32) | rl[0], b = ((unsigned long long)rh[1] << 32) | rl[1];
        k = a > b ? a : b;
    }
    {
        const uint32_t hi = (uint32_t)(k >> 32), lo = (uint32_t)k;
        const auto rh = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
        const auto rl = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
        const unsigned long long a = ((unsigned long long)rh[0] << 32) | rl[0], b = ((unsigned long long)rh[1] << 32) | rl[1];
        k = a > b ? a : b;
    }
    return k;
}
__device__ __forceinline__ void row_alts(const float (&lv)[8], int n, bool exclude0, const RowStats& st, int n_alts, uint32_t* __restrict__ alt_index,
                                         float* __restrict__ alt_logprob) {
    __shared__ unsigned long long s_ak[SCORE_THREADS / 64][ALTS_MAX];
    __shared__ float s_ax[SCORE_THREADS / 64][ALTS_MAX];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long k[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const int i = (s >> 2) * (SCORE_THREADS * 4) + tid * 4 + (s & 3);
        uint32_t u = __float_as_uint(lv[s] + 0.f);
        u ^= (u >> 31) ? 0xFFFFFFFFu : 0x80000000u;
        k[s] = (i < n && !(exclude0 && i == 0)) ? (((unsigned long long)u << 32) | (unsigned long long)(uint32_t)i) : 0ull;
    }
    unsigned long long best = 0ull;
#pragma unroll
    for (int s = 0; s < 8; ++s) best = k[s] > best ? k[s] : best;
    for (int r = 0; r < n_alts; ++r) {
        const unsigned long long win = wave_max_key(best);
        if (win != 0ull && best == win) {  // the owner lane (keys are distinct: the index is part of them)
            float x = 0.f;
            best = 0ull;
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                if (k[s] == win) { k[s] = 0ull; x = lv[s]; }
                best = k[s] > best ? k[s] : best;
            }
            s_ak[wave][r] = win; s_ax[wave][r] = x;
        } else if (win == 0ull && lane == 0) {
            s_ak[wave][r] = 0ull; s_ax[wave][r] = 0.f;
        }
    }
    __syncthreads();
    if (wave == 0) {
        const int w = lane >> 4, j = lane & (ALTS_MAX - 1);
        const unsigned long long key = j < n_alts ? s_ak[w][j] : 0ull;
        const float x = j < n_alts ? s_ax[w][j] : 0.f;
        // the rank of the lane's key among the 4 N parked ones = how many are larger (they are distinct): 4 N independent broadcast
        // reads instead of N more dependent reductions; cnt = the candidates there are (wave-uniform)
        int rank = 0, cnt = 0;
        for (int w2 = 0; w2 < SCORE_THREADS / 64; ++w2) {
#pragma unroll 4
            for (int j2 = 0; j2 < n_alts; ++j2) {
                const unsigned long long o = s_ak[w2][j2];
                rank += o > key ? 1 : 0;
                cnt += o != 0ull ? 1 : 0;
            }
        }
        if (key != 0ull && rank < n_alts) {
            alt_index[rank] = (uint32_t)(key & 0xFFFFFFFFull);
            alt_logprob[rank] = (x - st.m) - st.ls;
        }
        if (lane < n_alts && lane >= cnt) {
            alt_index[lane] = 0xFFFFFFFFu;
            alt_logprob[lane] = __uint_as_float(0x7FC00000u);
        }
    }
}
// where the alternatives of a slot's buffer lie: behind the records [cap][32] and the targets / token rows [cap][n_cb + 1] --
// alt_index u32 [cap][n_cb + 1][N], alt_logprob f32 [cap][n_cb + 1][N], entropy f32 [cap][n_cb + 1] (fs_slot_book.h)
struct AltsOut { uint32_t* index; float* logprob; float* entropy; };
__device__ __forceinline__ AltsOut alts_out(float* rec, int cap, int count, int d, int n_cb, int n_alts) {
    const size_t C1 = (size_t)n_cb + 1, per = (size_t)cap * C1 * (size_t)n_alts, at = (size_t)count * C1 + (size_t)d;
    uint32_t* base = reinterpret_cast<uint32_t*>(rec + (size_t)cap * 32) + (size_t)cap * C1;
    AltsOut o;
    o.index = base + at * n_alts;
    o.logprob = reinterpret_cast<float*>(base + per) + at * n_alts;
    o.entropy = reinterpret_cast<float*>(base + 2 * per) + at;
    return o;
}
template <bool ALTS = false>
__device__ __forceinline__ ScoreOut score_row(float* __restrict__ row, int n, int t, bool exclude0, int n_alts = 0, uint32_t* alt_index = nullptr,
                                              float* alt_logprob = nullptr, float* entropy = nullptr) {
    const int tid = threadIdx.x;
    // the target's logit, read by thread 0 ahead of the barriers (the store at the end comes behind them); candidate 0's comes out of lv
    const bool t_ok = (unsigned)t < (unsigned)n;
    float xr = 0.f;
    if (tid == 0 && t_ok && t != 0) xr = row[t];
    float lv[8];
    const RowStats st = score_row_stats<ALTS>(row, n, exclude0, lv);
    if constexpr (ALTS) {  // (from the registers: the row as it was, before +inf goes over the target)
        row_alts(lv, n, exclude0, st, n_alts, alt_index, alt_logprob);
        if (tid == 0) *entropy = st.ent;
    }
    const float xt = !t_ok ? __uint_as_float(0x7FC00000u) : (t == 0 ? st.x0 : xr);
    ScoreOut r;
    r.logprob = (xt - st.m) - st.ls;
    r.top_logprob = -st.ls;
    r.eos_logprob = (st.x0 - st.m) - st.ls;
    r.top = st.top;
    if (tid == 0 && t_ok) row[t] = INFINITY;  // the forcing: the unique maximum of a finite row
    return r;  // (logprob / eos_logprob: thread 0's are the row's)
}
// ---- traced slots of a FS_SESSION_TRACE session (fishrt.h: fs_lm_session_add_traced): slots that SAMPLE and leave the scoring slots'
// record of their own picks.  Their table entry is a ScoreSlot without targets (targets == null, rec != null).  The pick is not known in
// front of the sampler, and the next pass's head overwrites the codebook row, so the record is made in two parts: the score node of
// decision d writes what does not depend on the pick (top_logprob, top, eos_logprob), keeps m and log s, and copies the raw row into the
// slot's stash; ONE node behind the frame's last sampler (k_trace_commit) reads the picks out of SeqState::cur and closes the row.
// The stash of slot b, TRACE_STASH_WORDS f32: a 32-word head -- [0..8] m of decision d, [9..17] log s, [18] the open-row mark (u32: set
// by decision 0 of an iteration the slot runs, cleared by the tail node, so the iteration whose slow pick was <|im_end|> -- the slot is
// `done` from there on and its codebook nodes exit -- is still closed, exactly once, and a parked, frozen, finished or not yet joined
// slot adds no row) -- then the 9 raw rows [9][2048].  The row is NOT modified: the slot's sampler decides on what it always decided on.
constexpr int TRACE_HEAD_WORDS = 32, TRACE_ROW_WORDS = 2048, TRACE_OPEN = 18;
static_assert(TRACE_STASH_WORDS == TRACE_HEAD_WORDS + 9 * TRACE_ROW_WORDS, "stash layout");
template <bool ALTS = false>
__device__ __forceinline__ void trace_row(float* __restrict__ rec, float* __restrict__ stash, const float* __restrict__ row, int n, int d,
                                          bool exclude0, int n_alts = 0, uint32_t* alt_index = nullptr, float* alt_logprob = nullptr,
                                          float* entropy = nullptr) {
    const int tid = threadIdx.x;
    float lv[8];
    const RowStats st = score_row_stats<ALTS>(row, n, exclude0, lv);
    if constexpr (ALTS) {  // (neither depends on the pick)
        row_alts(lv, n, exclude0, st, n_alts, alt_index, alt_logprob);
        if (tid == 0) *entropy = st.ent;
    }
    float* dst = stash + TRACE_HEAD_WORDS + (size_t)d * TRACE_ROW_WORDS;  // (16-byte aligned: the stash is, and every offset is a multiple of 4 words)
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        const int i0 = g * (SCORE_THREADS * 4) + tid * 4;
        if (i0 + 3 < n) {
            *reinterpret_cast<float4*>(dst + i0) = make_float4(lv[g * 4 + 0], lv[g * 4 + 1], lv[g * 4 + 2], lv[g * 4 + 3]);
        } else {
#pragma unroll
            for (int s = 0; s < 4; ++s) if (i0 + s < n) dst[i0 + s] = lv[g * 4 + s];
        }
    }
    if (tid == 0) {
        stash[d] = st.m;
        stash[9 + d] = st.ls;
        rec[9 + d] = -st.ls;
        rec[18 + d] = __uint_as_float(st.top);
        if (d == 0) {
            rec[27] = (st.x0 - st.m) - st.ls;
            rec[28] = 0.f; rec[29] = 0.f; rec[30] = 0.f; rec[31] = 0.f;
            reinterpret_cast<uint32_t*>(stash)[TRACE_OPEN] = 1u;
        }
    }
}
// ALTS: the node of FS_SESSION_ALTS sessions -- every scoring and traced slot also leaves the n_alts most likely candidates and the
// entropy of the decision behind its records (alts_out).  The other instantiation does not read n_alts and is the node it always was.
template <bool ALTS>
__global__ __launch_bounds__(SCORE_THREADS) void k_score_slots(ScoreSlot* __restrict__ tab, const SeqState* __restrict__ states,
                                                               const SampleCfg* __restrict__ cfgs, float* __restrict__ logits, int ld, int n,
                                                               int d, int n_cb, float* __restrict__ stash, int n_alts) {
    const int b = blockIdx.x;
    ScoreSlot* sc = tab + b;
    float* rec = sc->rec;
    const int count = sc->count;
    if (!rec || states[b].done != 0 || count >= sc->cap) return;  // (block-uniform)
    const uint32_t* targets = sc->targets;
    AltsOut ao = {nullptr, nullptr, nullptr};
    if constexpr (ALTS) ao = alts_out(rec, sc->cap, count, d, n_cb, n_alts);
    if (!targets) {  // a traced slot (block-uniform; only the tables of FS_SESSION_TRACE sessions hold such entries, and those have a stash)
        if (stash) trace_row<ALTS>(rec + (size_t)count * 32, stash + (size_t)b * TRACE_STASH_WORDS, logits + (size_t)b * ld, n, d, d == 0 && cfgs[b].ignore_eos != 0,
                                   n_alts, ao.index, ao.logprob, ao.entropy);
        return;
    }
    const uint32_t tok = targets[(size_t)count * (n_cb + 1) + d];
    const int t = d == 0 ? (int)(tok - cfgs[b].audio_base) : (int)tok;
    const ScoreOut r = score_row<ALTS>(logits + (size_t)b * ld, n, t, d == 0 && cfgs[b].ignore_eos != 0, n_alts, ao.index, ao.logprob, ao.entropy);
    if (threadIdx.x == 0) {
        rec += (size_t)count * 32;
        rec[d] = r.logprob;
        rec[9 + d] = r.top_logprob;
        rec[18 + d] = __uint_as_float(r.top);
        if (d == 0) { rec[27] = r.eos_logprob; rec[28] = 0.f; rec[29] = 0.f; rec[30] = 0.f; rec[31] = 0.f; }
        if (d == n_cb) sc->count = count + 1;
    }
}
void launch_score_slots(ScoreSlot* tab, const SeqState* states, const SampleCfg* cfgs, float* logits, int ld, int n, int decision, int n_cb, int B,
                        hipStream_t st, float* trace_stash, int n_alts) {
    FS_REQUIRE(n >= 2 && n <= SCORE_THREADS * 8 && n <= ld && n_cb == 8 && decision >= 0 && decision <= n_cb,
               "score node: 2 .. 2048 candidates, 8 codebooks (the 32-word record holds 9 decisions)");
    FS_REQUIRE(n_alts >= 0 && n_alts <= ALTS_MAX, "score node: at most 16 alternatives");
    if (n_alts > 0)
        hipLaunchKernelGGL(k_score_slots<true>, dim3(B), dim3(SCORE_THREADS), 0, st, tab, states, cfgs, logits, ld, n, decision, n_cb, trace_stash, n_alts);
    else
        hipLaunchKernelGGL(k_score_slots<false>, dim3(B), dim3(SCORE_THREADS), 0, st, tab, states, cfgs, logits, ld, n, decision, n_cb, trace_stash, 0);
    FS_LAUNCH_CHECK();
}
// The tail node of a traced iteration: block b closes the row its slot's decision-0 node opened in this step.  Thread d <= n_cb takes
// decision d: the pick out of cur[] (the frame commit has run: cur[0] the slow token as it goes into the next input column, cur[1 + c] the
// codes; slow index = tok - audio_base, <|im_end|> = candidate 0), its log-prob from the stashed row, m and log s -- the score node's
// expression -- or, for the codebook decisions an <|im_end|> iteration skipped, NaN / NaN / 0xFFFFFFFF / token 0.  The picks go to the
// slot's token rows u32 [cap][n_cb + 1] behind the records (where a scoring slot keeps its targets).  Then the mark is cleared and the
// count bumped.  Everything else -- null and scoring entries, no open row -- exits at once.
// ALTS (FS_SESSION_ALTS sessions): a skipped decision's alternatives and entropy get the same fill -- 0xFFFFFFFF / NaN / NaN.
template <bool ALTS>
__global__ __launch_bounds__(64) void k_trace_commit(ScoreSlot* __restrict__ tab, const SeqState* __restrict__ states, const SampleCfg* __restrict__ cfgs,
                                                    float* __restrict__ stash_all, int n_slow, int cb_size, int n_cb, int n_alts) {
    const int b = blockIdx.x, d = threadIdx.x;
    ScoreSlot* sc = tab + b;
    float* rec = sc->rec;
    if (!rec || sc->targets) return;  // (block-uniform)
    float* stash = stash_all + (size_t)b * TRACE_STASH_WORDS;
    uint32_t* open = reinterpret_cast<uint32_t*>(stash) + TRACE_OPEN;
    const int count = sc->count, cap = sc->cap;
    if (*open == 0u || count >= cap) return;  // (block-uniform)
    if (d <= n_cb) {
        const uint32_t slow = states[b].cur[0], tok = states[b].cur[d];
        const bool eos = slow == cfgs[b].im_end_id;
        const uint32_t idx = d == 0 ? (eos ? 0u : tok - cfgs[b].audio_base) : tok;
        const bool made = (d == 0 || !eos) && idx < (uint32_t)(d == 0 ? n_slow : cb_size);
        float* r = rec + (size_t)count * 32;
        uint32_t* toks = reinterpret_cast<uint32_t*>(rec + (size_t)cap * 32) + (size_t)count * (n_cb + 1);
        const float nan = __uint_as_float(0x7FC00000u);
        if (made) {
            r[d] = (stash[TRACE_HEAD_WORDS + (size_t)d * TRACE_ROW_WORDS + idx] - stash[d]) - stash[9 + d];
            toks[d] = tok;
        } else {
            r[d] = nan;
            if (d > 0 && eos) { r[9 + d] = nan; r[18 + d] = __uint_as_float(0xFFFFFFFFu); }
            toks[d] = 0u;
            if constexpr (ALTS) {
                if (d > 0 && eos) {
                    const AltsOut ao = alts_out(rec, cap, count, d, n_cb, n_alts);
                    for (int j = 0; j < n_alts; ++j) { ao.index[j] = 0xFFFFFFFFu; ao.logprob[j] = nan; }
                    *ao.entropy = nan;
                }
            }
        }
    }
    __syncthreads();  // (every thread has read the count and the mark)
    if (d == 0) { *open = 0u; sc->count = count + 1; }
}
void launch_trace_commit(ScoreSlot* tab, const SeqState* states, const SampleCfg* cfgs, float* trace_stash, int n_slow, int cb_size, int n_cb, int B,
                         hipStream_t st, int n_alts) {
    FS_REQUIRE(trace_stash && n_cb == 8 && n_slow >= 2 && n_slow <= TRACE_ROW_WORDS && cb_size >= 2 && cb_size <= TRACE_ROW_WORDS,
               "trace node: 8 codebooks, rows of 2 .. 2048 candidates");
    FS_REQUIRE(n_alts >= 0 && n_alts <= ALTS_MAX, "trace node: at most 16 alternatives");
    if (n_alts > 0) hipLaunchKernelGGL(k_trace_commit<true>, dim3(B), dim3(64), 0, st, tab, states, cfgs, trace_stash, n_slow, cb_size, n_cb, n_alts);
    else hipLaunchKernelGGL(k_trace_commit<false>, dim3(B), dim3(64), 0, st, tab, states, cfgs, trace_stash, n_slow, cb_size, n_cb, 0);
    FS_LAUNCH_CHECK();
}
// test hook (fs_selftest_score_rows): score_row on caller rows, one block per row
__global__ __launch_bounds__(SCORE_THREADS) void k_score_rows_test(float* __restrict__ rows, int n, const uint32_t* __restrict__ targets, int exclude0,
                                                                   float* __restrict__ logprob, float* __restrict__ top_logprob,
                                                                   uint32_t* __restrict__ top) {
    const int b = blockIdx.x;
    const ScoreOut r = score_row(rows + (size_t)b * n, n, (int)targets[b], exclude0 != 0);
    if (threadIdx.x == 0) { logprob[b] = r.logprob; top_logprob[b] = r.top_logprob; top[b] = r.top; }
}
void debug_score_rows(int device, const float* logits, int S, int n, const uint32_t* targets, int exclude0, float* logprob_out,
                      float* top_logprob_out, uint32_t* top_out, float* row_out) {
    FS_REQUIRE(S >= 1 && S <= (1 << 16) && n >= 2 && n <= SCORE_THREADS * 8, "bad score test shape (1 <= S <= 65536 rows of 2 <= n <= 2048)");
    for (int s = 0; s < S; ++s) FS_REQUIRE(targets[s] < (uint32_t)n, "score test: a target is outside [0, n)");
    FS_HIP(hipSetDevice(device));
    const size_t nl = (size_t)S * n;
    float *d_rows = nullptr, *d_lp = nullptr, *d_tlp = nullptr; uint32_t *d_t = nullptr, *d_top = nullptr;
    FS_HIP(hipMalloc(&d_rows, sizeof(float) * nl));
    FS_HIP(hipMalloc(&d_lp, sizeof(float) * S)); FS_HIP(hipMalloc(&d_tlp, sizeof(float) * S));
    FS_HIP(hipMalloc(&d_t, sizeof(uint32_t) * S)); FS_HIP(hipMalloc(&d_top, sizeof(uint32_t) * S));
    FS_HIP(hipMemcpy(d_rows, logits, sizeof(float) * nl, hipMemcpyHostToDevice));
    FS_HIP(hipMemcpy(d_t, targets, sizeof(uint32_t) * S, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_score_rows_test, dim3(S), dim3(SCORE_THREADS), 0, nullptr, d_rows, n, d_t, exclude0, d_lp, d_tlp, d_top);
    FS_LAUNCH_CHECK();
    FS_HIP(hipDeviceSynchronize());
    if (logprob_out) FS_HIP(hipMemcpy(logprob_out, d_lp, sizeof(float) * S, hipMemcpyDeviceToHost));
    if (top_logprob_out) FS_HIP(hipMemcpy(top_logprob_out, d_tlp, sizeof(float) * S, hipMemcpyDeviceToHost));
    if (top_out) FS_HIP(hipMemcpy(top_out, d_top, sizeof(uint32_t) * S, hipMemcpyDeviceToHost));
    if (row_out) FS_HIP(hipMemcpy(row_out, d_rows, sizeof(float) * nl, hipMemcpyDeviceToHost));
    (void)hipFree(d_rows); (void)hipFree(d_lp); (void)hipFree(d_tlp); (void)hipFree(d_t); (void)hipFree(d_top);
}
// test hook (fs_selftest_alt_rows): the ALTS node's device functions on caller rows, one block per row
__global__ __launch_bounds__(SCORE_THREADS) void k_alt_rows_test(const float* __restrict__ rows, int n, int exclude0, int n_alts,
                                                                 uint32_t* __restrict__ alt_index, float* __restrict__ alt_logprob,
                                                                 float* __restrict__ entropy) {
    const int b = blockIdx.x;
    float lv[8];
    const RowStats st = score_row_stats<true>(rows + (size_t)b * n, n, exclude0 != 0, lv);
    row_alts(lv, n, exclude0 != 0, st, n_alts, alt_index + (size_t)b * n_alts, alt_logprob + (size_t)b * n_alts);
    if (threadIdx.x == 0) entropy[b] = st.ent;
}
void debug_alt_rows(int device, const float* logits, int S, int n, int exclude0, int n_alts, uint32_t* alt_index_out, float* alt_logprob_out,
                    float* entropy_out) {
    FS_REQUIRE(S >= 1 && S <= (1 << 16) && n >= 2 && n <= SCORE_THREADS * 8, "bad alternatives test shape (1 <= S <= 65536 rows of 2 <= n <= 2048)");
    FS_REQUIRE(n_alts >= 1 && n_alts <= ALTS_MAX, "alternatives test: 1 <= n_alts <= 16");
    FS_HIP(hipSetDevice(device));
    const size_t nl = (size_t)S * n, na = (size_t)S * n_alts;
    float *d_rows = nullptr, *d_lp = nullptr, *d_ent = nullptr; uint32_t* d_idx = nullptr;
    FS_HIP(hipMalloc(&d_rows, sizeof(float) * nl));
    FS_HIP(hipMalloc(&d_lp, sizeof(float) * na)); FS_HIP(hipMalloc(&d_idx, sizeof(uint32_t) * na)); FS_HIP(hipMalloc(&d_ent, sizeof(float) * S));
    FS_HIP(hipMemcpy(d_rows, logits, sizeof(float) * nl, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_alt_rows_test, dim3(S), dim3(SCORE_THREADS), 0, nullptr, d_rows, n, exclude0, n_alts, d_idx, d_lp, d_ent);
    FS_LAUNCH_CHECK();
    FS_HIP(hipDeviceSynchronize());
    if (alt_index_out) FS_HIP(hipMemcpy(alt_index_out, d_idx, sizeof(uint32_t) * na, hipMemcpyDeviceToHost));
    if (alt_logprob_out) FS_HIP(hipMemcpy(alt_logprob_out, d_lp, sizeof(float) * na, hipMemcpyDeviceToHost));
    if (entropy_out) FS_HIP(hipMemcpy(entropy_out, d_ent, sizeof(float) * S, hipMemcpyDeviceToHost));
    (void)hipFree(d_rows); (void)hipFree(d_lp); (void)hipFree(d_idx); (void)hipFree(d_ent);
}

// ---- sampler test hook (fs_selftest_sample_rows): the static-batch slow sampler on caller-provided logits, B rows of n candidates,
// as sample() call number `call_index` of a request (child StdRng of row b = master u64 number call_index * B + b)
void debug_sample_rows(int device, const float* logits, int B, int n, double temp, double top_p, uint64_t top_k, uint64_t seed,
                       int call_index, uint32_t* out) {
    FS_REQUIRE(B >= 1 && n >= 1 && n <= SAMPLE_MAXN, "bad sampler test shape");
    FS_HIP(hipSetDevice(device));
    float* d_logits = nullptr; SampleCfg* d_cfg = nullptr; RngState* d_rng = nullptr; SeqState* d_st = nullptr;
    FS_HIP(hipMalloc(&d_logits, sizeof(float) * (size_t)B * n));
    FS_HIP(hipMalloc(&d_cfg, sizeof(SampleCfg))); FS_HIP(hipMalloc(&d_rng, sizeof(RngState))); FS_HIP(hipMalloc(&d_st, sizeof(SeqState) * B));
    FS_HIP(hipMemcpy(d_logits, logits, sizeof(float) * (size_t)B * n, hipMemcpyHostToDevice));
    SampleCfg c = {};
    c.temp = (float)temp; c.top_p = (float)top_p; c.top_k = (int)std::min<uint64_t>(top_k, 1u << 30); c.rep_pen = 1.f; c.top_p64 = top_p;
    FS_HIP(hipMemcpy(d_cfg, &c, sizeof(c), hipMemcpyHostToDevice));
    RngState r = {};
    seed_from_u64(seed, r.key);
    FS_HIP(hipMemcpy(d_rng, &r, sizeof(r), hipMemcpyHostToDevice));
    std::vector<SeqState> hs(B);
    for (auto& s : hs) { s = SeqState{}; s.frame = call_index; }
    FS_HIP(hipMemcpy(d_st, hs.data(), sizeof(SeqState) * B, hipMemcpyHostToDevice));
    // FISHRT_SAMPLER_IMPL=par512: the block-parallel sampler the persistent fast decoder uses (lm_bsample_dev.h), 512 threads per row
    const char* impl = getenv("FISHRT_SAMPLER_IMPL");
    const bool par = impl && std::string(impl) == "par512" && temp > 1e-7 && top_k > 0 && top_k <= 256 && (int)top_k < n && n <= 2048;
    if (par) {
        uint32_t* d_out = nullptr;
        FS_HIP(hipMalloc(&d_out, sizeof(uint32_t) * B));
        if (n <= 1024) hipLaunchKernelGGL((k_bsample_rows_test<512, 2>), dim3(B), dim3(512), 0, nullptr, d_logits, n, d_cfg, d_rng, B, call_index, d_out);
        else hipLaunchKernelGGL((k_bsample_rows_test<512, 4>), dim3(B), dim3(512), 0, nullptr, d_logits, n, d_cfg, d_rng, B, call_index, d_out);
        FS_LAUNCH_CHECK();
        FS_HIP(hipDeviceSynchronize());
        FS_HIP(hipMemcpy(out, d_out, sizeof(uint32_t) * B, hipMemcpyDeviceToHost));
        (void)hipFree(d_out);
    } else {
        hipLaunchKernelGGL((k_sample_slow_rows<bf16_t>), dim3(B), dim3(SAMPLE_THREADS), 0, nullptr, d_logits, n, n, d_cfg, d_rng, B, 1, d_st,
                           (const float*)nullptr, (float*)nullptr, 0, PrepOut{nullptr, 0.f, nullptr, nullptr});
        FS_LAUNCH_CHECK();
        FS_HIP(hipDeviceSynchronize());
        FS_HIP(hipMemcpy(hs.data(), d_st, sizeof(SeqState) * B, hipMemcpyDeviceToHost));
        for (int b = 0; b < B; ++b) out[b] = hs[b].cur[0];
    }
    (void)hipFree(d_logits); (void)hipFree(d_cfg); (void)hipFree(d_rng); (void)hipFree(d_st);
}

// ---- per-slot sampler test hook (fs_selftest_sample_slots): S independent slot streams of R decisions each on caller-provided logits
// f32 [S][R][n]; cfgs[s] / seeds[s] = the slot's settings and StdRng seed; out [S][R] the picks, words_used [S] the stream positions afterwards
void debug_sample_slots(int device, const float* logits, int S, int R, int n, const SampleCfg* cfgs, const uint64_t* seeds, uint32_t* out,
                        uint64_t* words_used) {
    FS_REQUIRE(S >= 1 && R >= 1 && n >= 1 && n <= PAR_THREADS * 4 && (size_t)S * R <= (1u << 20), "bad sampler test shape (n <= 2048)");
    FS_HIP(hipSetDevice(device));
    const size_t nl = (size_t)S * R * n;
    float* d_logits = nullptr; SampleCfg* d_cfg = nullptr; unsigned long long* d_seeds = nullptr; uint32_t* d_out = nullptr; unsigned long long* d_used = nullptr;
    FS_HIP(hipMalloc(&d_logits, sizeof(float) * nl));
    FS_HIP(hipMalloc(&d_cfg, sizeof(SampleCfg) * S)); FS_HIP(hipMalloc(&d_seeds, sizeof(unsigned long long) * S));
    FS_HIP(hipMalloc(&d_out, sizeof(uint32_t) * (size_t)S * R)); FS_HIP(hipMalloc(&d_used, sizeof(unsigned long long) * S));
    FS_HIP(hipMemcpy(d_logits, logits, sizeof(float) * nl, hipMemcpyHostToDevice));
    FS_HIP(hipMemcpy(d_cfg, cfgs, sizeof(SampleCfg) * S, hipMemcpyHostToDevice));
    FS_HIP(hipMemcpy(d_seeds, seeds, sizeof(unsigned long long) * S, hipMemcpyHostToDevice));
    if (n <= PAR_THREADS * 2) hipLaunchKernelGGL((k_sample_slots_test<2>), dim3(S), dim3(PAR_THREADS), 0, nullptr, d_logits, R, n, d_cfg, d_seeds, d_out, d_used);
    else hipLaunchKernelGGL((k_sample_slots_test<4>), dim3(S), dim3(PAR_THREADS), 0, nullptr, d_logits, R, n, d_cfg, d_seeds, d_out, d_used);
    FS_LAUNCH_CHECK();
    FS_HIP(hipDeviceSynchronize());
    FS_HIP(hipMemcpy(out, d_out, sizeof(uint32_t) * (size_t)S * R, hipMemcpyDeviceToHost));
    FS_HIP(hipMemcpy(words_used, d_used, sizeof(unsigned long long) * S, hipMemcpyDeviceToHost));
    (void)hipFree(d_logits); (void)hipFree(d_cfg); (void)hipFree(d_seeds); (void)hipFree(d_out); (void)hipFree(d_used);
}


// ---- sampler-node test hook (fs_selftest_sample_frames, include/fishrt.h): F frames of the production launchers above on caller logits,
// in the engine's order, the complete sampler state copied out after every launch.  The SampleCfg, the request stream and a slot's
// activation come from the setup the engine uses (lm_kernels.h: sample_cfg_make, rng_fresh, slot_rng_fresh, slot_sampling_error).
namespace {
constexpr size_t kSampGuard = 1024;  // bytes: 256 f32 elements
struct SampDev {  // device buffer of n bytes between two guards, all 0xFF bytes at first
    void* p = nullptr;
    size_t n = 0;
    void alloc(size_t bytes, hipStream_t st) {
        n = (bytes + 15) & ~(size_t)15;
        FS_HIP(hipMalloc(&p, n + 2 * kSampGuard));
        FS_HIP(hipMemsetAsync(p, 0xFF, n + 2 * kSampGuard, st));
    }
    char* data() const { return (char*)p + kSampGuard; }
    template <typename T> T* as() const { return reinterpret_cast<T*>(data()); }
    void up(const void* src, size_t bytes, hipStream_t st, size_t off = 0) {  // synchronous: the source may be a temporary
        FS_HIP(hipMemcpyAsync(data() + off, src, bytes, hipMemcpyHostToDevice, st));
        FS_HIP(hipStreamSynchronize(st));
    }
    void put(const void* src, size_t bytes, hipStream_t st) { alloc(bytes, st); up(src, bytes, st); }
    bool intact(hipStream_t st) const {
        if (!p) return true;
        std::vector<uint8_t> g(2 * kSampGuard);
        FS_HIP(hipMemcpyAsync(g.data(), p, kSampGuard, hipMemcpyDeviceToHost, st));
        FS_HIP(hipMemcpyAsync(g.data() + kSampGuard, data() + n, kSampGuard, hipMemcpyDeviceToHost, st));
        FS_HIP(hipStreamSynchronize(st));
        for (uint8_t b : g) if (b != 0xFF) return false;
        return true;
    }
    ~SampDev() { if (p) (void)hipFree(p); }
};
void samp_req(bool ok, const char* msg) { if (!ok) throw Error(std::string("sampler self-test: ") + msg); }
static_assert(sizeof(SeqState) == 40 * 4, "fs_sample_case::state0 is the SeqState as 40 words");
static_assert(sizeof(RngState) == 10 * 4 && sizeof(SlotRng) == 58 * 4, "FS_SAMPLE_OUT_RNG word counts");

struct SampInfo {
    bool single = false, rows = false, slots = false, wide = false, par = false, legacy = false;
    int L = 0, Lf = 0, R = 0, hid_rows = 0;
    size_t per[FS_SAMPLE_OUT_COUNT] = {};  // bytes per launch of every output
    std::vector<SampleCfg> cfgs;
};
void sample_validate(const fs_sample_case& c, SampInfo& I) {
    samp_req(c.family >= FS_SAMPLE_SINGLE && c.family <= FS_SAMPLE_SLOTS_WIDE, "unknown family");
    samp_req(c.wt == FS_GEMV_WT_F32 || c.wt == FS_GEMV_WT_BF16, "wt must be f32 or bf16 (the table types)");
    I.single = c.family == FS_SAMPLE_SINGLE || c.family == FS_SAMPLE_SINGLE_BATCHROW;
    I.rows = c.family == FS_SAMPLE_ROWS || c.family == FS_SAMPLE_ROWS_PAR;
    I.slots = c.family == FS_SAMPLE_SLOTS || c.family == FS_SAMPLE_SLOTS_WIDE;
    I.wide = c.family == FS_SAMPLE_SLOTS_WIDE;
    I.par = c.family == FS_SAMPLE_ROWS_PAR;
    I.legacy = c.tokens.has_semantic_end == 0;
    samp_req(c.B >= 1 && c.B <= 256 && c.F >= 1 && c.F <= 4096, "1 <= B <= 256, 1 <= F <= 4096");
    samp_req(c.n_cb >= 1 && c.n_cb + 1 <= 16, "n_cb + 1 <= 16 (SeqState::cur, the words table)");
    samp_req(c.cb_size >= 2 && c.n_slow >= 2 && c.ld >= c.n_slow, "cb_size >= 2, 2 <= n_slow <= ld");
    samp_req(c.dim >= 1 && c.out_cap >= 1 && c.tok_rows >= 1, "dim, out_cap, tok_rows >= 1");
    samp_req(c.samplings && c.seeds && c.ignore_eos && c.state0 && c.tok_emb && c.cb_emb && c.fast_emb && c.x && c.logits, "null argument");
    samp_req(c.n_cfg == (I.slots ? c.B : 1), "n_cfg: B for the slot families, 1 otherwise");
    if (I.single) {
        samp_req(c.B == 1, "the single-sequence kernels take one row");
        samp_req(c.n_slow <= SAMPLE_MAXN, "audio-range vocabulary larger than the sampler capacity");
        samp_req(c.cb_size <= SAMPLE_MAXN, "codebook larger than the sampler capacity");
        samp_req(!c.prep && !c.session && !c.cap_frames, "the single-sequence kernels have no prep epilogue, session mode or capture record");
        if (c.family == FS_SAMPLE_SINGLE_BATCHROW)
            samp_req(!I.legacy && c.batch_rows >= 1 && c.batch_row >= 0 && c.batch_row < c.batch_rows, "batch row: 0 <= batch_row < batch_rows, Fish 1.5 / generic layout");
        else samp_req(c.batch_rows == 0 && c.batch_row == 0, "batch_rows / batch_row belong to SINGLE_BATCHROW");
    } else {
        samp_req(!c.hid && c.batch_rows == 0 && c.batch_row == 0, "hid / batch_rows belong to the single-sequence families");
    }
    if (I.rows) {
        samp_req(!I.legacy, "the static-batch samplers need the Fish 1.5 / generic token layout");
        samp_req(c.n_slow <= SAMPLE_MAXN, "audio-range vocabulary larger than the sampler capacity");
        samp_req(c.cb_size <= SAMPLE_MAXN, "codebook larger than the sampler capacity");
        samp_req(c.n_cb + 1 <= ROWS_WORDS_LD, "too many sample() calls per frame");
        samp_req(!c.cap_frames, "the capture record belongs to the slot families");
    }
    if (I.slots) {
        samp_req(c.n_slow <= PAR_THREADS * 4, "audio-range vocabulary outside the per-slot sampler capacity (2 .. 2048)");
        samp_req(c.cb_size <= PAR_THREADS * 2, "codebook larger than the per-slot sampler capacity (1024)");
        samp_req(!c.session, "session belongs to the row families (slots always freeze)");
        samp_req(c.cap_frames >= 0 && (size_t)c.B * (size_t)c.cap_frames <= 64, "capture record: B x cap_frames <= 64");
    }
    if (I.legacy) samp_req(c.n_slow == 2, "Fish <= 1.4 layout: the slow logits are [pad, im_end]");
    if (c.prep) samp_req(c.prep_g && c.dim <= 1024 && c.dim % 32 == 0 && c.B <= 32, "sampler-side RMSNorm of the next input row: dim <= 1024, dim % 32 == 0 (whole fragments), B <= 32");
    // the SampleCfg of every row / slot, as the engine makes it
    const TokenLayout lay{c.tokens.im_end_id, c.tokens.pad_id, c.tokens.semantic_start_id, c.tokens.semantic_end_id, c.tokens.has_semantic_end != 0};
    if (!I.legacy) samp_req(lay.semantic_start_id >= 1, "semantic_start_id >= 1");
    for (int i = 0; i < c.n_cfg; ++i) {
        const fs_sampling& s = c.samplings[i];
        samp_req(std::isfinite(s.temp) && s.temp >= 0.0 && std::isfinite(s.top_p) && std::isfinite(s.repetition_penalty) && s.repetition_penalty > 0.f,
                 "temp finite and >= 0, top_p finite, repetition_penalty finite and > 0");
        SampleCfg cfg = sample_cfg_make(lay, s.temp, s.top_p, s.top_k, s.repetition_penalty, c.ignore_eos[i] != 0);
        if (c.family == FS_SAMPLE_SINGLE_BATCHROW) { cfg.batch_rows = c.batch_rows; cfg.batch_row = c.batch_row; cfg.batch_calls = c.n_cb + 1; }
        if (I.rows) { cfg.rep_pen = 1.0f; cfg.session = c.session ? 1 : 0; }
        if (I.slots) {
            cfg.session = 1;
            if (const char* e = slot_sampling_error(s.temp, s.top_p, s.top_k, I.wide)) throw Error(std::string("sampler self-test: ") + e);
            if (!I.wide && s.temp > 0.0)
                samp_req((int)s.top_k < c.cb_size && (I.legacy || (int)s.top_k < c.n_slow), "a narrow slot's top_k must be below its candidate counts (0 < top_k <= 256 < n)");
        }
        if (I.par) samp_req(rows_par_sampler_ok(s.temp, s.top_k, c.n_slow, c.cb_size), "settings outside the block-parallel row sampler (rows_par_sampler_ok)");
        I.cfgs.push_back(cfg);
    }
    // every token id the tables can be indexed with: the slow picks, <|im_end|>, pad, and the initial states' rows
    const SampleCfg& c0 = I.cfgs[0];
    samp_req(c0.im_end_id < (uint32_t)c.tok_rows, "im_end_id outside tok_emb");
    if (I.legacy) samp_req(c0.pad_id < (uint32_t)c.tok_rows, "pad_id outside tok_emb");
    else samp_req((uint64_t)c0.audio_base + (uint64_t)c.n_slow <= (uint64_t)c.tok_rows, "a slow candidate lies outside tok_emb");
    int frame0 = 0;
    for (int b = 0; b < c.B; ++b) {
        const int32_t* s = c.state0 + (size_t)b * 40;
        samp_req(s[0] >= 0 && s[2] >= 0 && s[3] >= 0 && s[3] <= 2 && s[4] >= 0 && (s[5] == 0 || s[5] == 1), "state0: pos, frame, n_out >= 0; done 0..2; have_prev 0 / 1");
        samp_req((uint32_t)s[8] < (uint32_t)c.tok_rows && (uint32_t)s[24] < (uint32_t)c.tok_rows, "state0: a slow token outside tok_emb");
        for (int i = 1; i <= c.n_cb; ++i)
            samp_req((uint32_t)s[8 + i] < (uint32_t)c.cb_size && (uint32_t)s[24 + i] < (uint32_t)c.cb_size, "state0: a code outside the codebook");
        frame0 = std::max(frame0, s[2]);
    }
    I.Lf = (I.par ? 1 : 0) + 1 + c.n_cb;
    I.L = c.F * I.Lf;
    I.R = I.slots ? c.B : (I.single ? 1 : 0);
    I.hid_rows = c.hid ? frame0 + c.F : 0;
    const size_t B = (size_t)c.B, C = (size_t)c.n_cb;
    I.per[FS_SAMPLE_OUT_STATES] = B * sizeof(SeqState);
    I.per[FS_SAMPLE_OUT_RING] = (size_t)I.R * C * 17 * 4;
    I.per[FS_SAMPLE_OUT_META] = (size_t)I.R * C * 2 * 4;
    I.per[FS_SAMPLE_OUT_MASK] = (size_t)I.R * C * c.cb_size * 4;
    I.per[FS_SAMPLE_OUT_RNG] = I.slots ? B * sizeof(SlotRng) : sizeof(RngState);
    I.per[FS_SAMPLE_OUT_WORDS] = I.par ? B * ROWS_WORDS_LD * 4 : 0;
    I.per[FS_SAMPLE_OUT_XF] = I.per[FS_SAMPLE_OUT_X] = B * c.dim * 4;
    I.per[FS_SAMPLE_OUT_PREP] = c.prep ? (size_t)2 * 32 * c.dim * 2 : 0;
    I.per[FS_SAMPLE_OUT_EPOCH] = c.prep ? 8 : 0;
    I.per[FS_SAMPLE_OUT_CODES] = B * C * c.out_cap * 4;
    I.per[FS_SAMPLE_OUT_HID] = (size_t)I.hid_rows * c.dim * 4;
    I.per[FS_SAMPLE_OUT_CAP] = B * (size_t)c.cap_frames * 4 * 4;
}

template <typename T> void samp_put_as(SampDev& b, const float* src, size_t n, hipStream_t st) {
    std::vector<T> h(n);
    for (size_t i = 0; i < n; ++i) {
        if constexpr (std::is_same<T, float>::value) h[i] = src[i];
        else h[i] = f32_to_bf16_host(src[i]);
    }
    b.put(h.data(), n * sizeof(T), st);
}

template <typename WT>
void sample_frames_run(const fs_sample_case& c, const SampInfo& I, fs_sample_out& o, hipStream_t st) {
    using SK = SampleKernels<WT>;
    const int B = c.B, C = c.n_cb, dim = c.dim;
    ModelDims d{};
    d.dim = dim; d.eps = c.eps;
    SampDev dTok, dCb, dFast, dG, dCfg, dRng, dState, dMask, dSeen, dRing, dMeta, dLs, dLf, dX, dXF, dA, dEp, dCodes, dHid, dHidCell, dCap, dWords;
    samp_put_as<WT>(dTok, c.tok_emb, (size_t)c.tok_rows * dim, st);
    samp_put_as<WT>(dCb, c.cb_emb, (size_t)C * c.cb_size * dim, st);
    samp_put_as<WT>(dFast, c.fast_emb, (size_t)c.cb_size * dim, st);
    if (c.prep) dG.put(c.prep_g, (size_t)dim * 4, st);
    dCfg.put(I.cfgs.data(), I.cfgs.size() * sizeof(SampleCfg), st);
    if (I.slots) {
        std::vector<SlotRng> r;
        for (int b = 0; b < B; ++b) r.push_back(slot_rng_fresh(c.seeds[b]));
        dRng.put(r.data(), r.size() * sizeof(SlotRng), st);
    } else {
        const RngState r = rng_fresh(c.seeds[0]);
        dRng.put(&r, sizeof(r), st);
    }
    dState.put(c.state0, (size_t)B * sizeof(SeqState), st);
    RepPenState rp{nullptr, nullptr, nullptr, nullptr};
    if (I.R) {  // RepPenBufs' layout, row after row; reset per row as at a request's start / a slot's activation
        const size_t per = (size_t)C * c.cb_size;
        dMask.alloc((size_t)I.R * per * 4, st); dSeen.alloc((size_t)I.R * per, st);
        dRing.alloc((size_t)I.R * C * 17 * 4, st); dMeta.alloc((size_t)I.R * C * 2 * 4, st);
        FS_HIP(hipMemsetAsync(dRing.data(), 0, (size_t)I.R * C * 17 * 4, st));
        rp = RepPenState{dMask.as<float>(), dSeen.as<uint8_t>(), dRing.as<int>(), dMeta.as<int>()};
        for (int r = 0; r < I.R; ++r)
            launch_reppen_reset(RepPenState{rp.mask + r * per, rp.seen + r * per, rp.ring + (size_t)r * C * 17, rp.ring_meta + (size_t)r * C * 2}, C, c.cb_size, st);
    }
    dLs.alloc((size_t)B * c.ld * 4, st); dLf.alloc((size_t)B * c.cb_size * 4, st);
    dX.alloc((size_t)B * dim * 4, st); dXF.alloc((size_t)B * dim * 4, st);
    if (c.prep) {
        dA.alloc((size_t)2 * 32 * dim * 2, st);
        const uint32_t z[2] = {0u, 0u};
        dEp.put(z, 8, st);
    }
    dCodes.alloc((size_t)B * C * c.out_cap * 4, st);
    if (c.hid) {
        dHid.alloc((size_t)I.hid_rows * dim * 4, st);
        float* hp = dHid.as<float>();
        dHidCell.put(&hp, sizeof(hp), st);
    }
    if (c.cap_frames) dCap.alloc((size_t)B * c.cap_frames * 9 * 2048 * 4, st);
    if (I.par) dWords.alloc((size_t)B * ROWS_WORDS_LD * 4, st);
    const float* prep_g = c.prep ? dG.as<float>() : nullptr;
    uint16_t* prep_A = c.prep ? dA.as<uint16_t>() : nullptr;
    uint32_t* epoch = c.prep ? dEp.as<uint32_t>() : nullptr;
    const uint32_t* words = I.par ? dWords.as<uint32_t>() : nullptr;

    int l = 0;
    auto record = [&]() {  // the complete state after launch l
        FS_HIP(hipStreamSynchronize(st));
        auto down = [&](int which, const SampDev& b) {
            if (o.buf[which] && I.per[which]) FS_HIP(hipMemcpyAsync((char*)o.buf[which] + (size_t)l * I.per[which], b.data(), I.per[which], hipMemcpyDeviceToHost, st));
        };
        down(FS_SAMPLE_OUT_STATES, dState);
        if (I.R) { down(FS_SAMPLE_OUT_RING, dRing); down(FS_SAMPLE_OUT_META, dMeta); down(FS_SAMPLE_OUT_MASK, dMask); }
        down(FS_SAMPLE_OUT_RNG, dRng);
        if (I.par) down(FS_SAMPLE_OUT_WORDS, dWords);
        down(FS_SAMPLE_OUT_XF, dXF); down(FS_SAMPLE_OUT_X, dX);
        if (c.prep) { down(FS_SAMPLE_OUT_PREP, dA); down(FS_SAMPLE_OUT_EPOCH, dEp); }
        down(FS_SAMPLE_OUT_CODES, dCodes);
        if (c.hid) down(FS_SAMPLE_OUT_HID, dHid);
        if (c.cap_frames && o.buf[FS_SAMPLE_OUT_CAP]) {
            float* dst = (float*)((char*)o.buf[FS_SAMPLE_OUT_CAP] + (size_t)l * I.per[FS_SAMPLE_OUT_CAP]);
            for (int r = 0; r < B * c.cap_frames; ++r) {
                const float* rec = dCap.as<float>() + (size_t)r * 9 * 2048;
                FS_HIP(hipMemcpyAsync(dst + (size_t)r * 4, rec, 12, hipMemcpyDeviceToHost, st));
                FS_HIP(hipMemcpyAsync(dst + (size_t)r * 4 + 3, rec + 2047, 4, hipMemcpyDeviceToHost, st));
            }
        }
        FS_HIP(hipStreamSynchronize(st));
        ++l;
    };
    const size_t frame_logits = (size_t)B * c.n_slow + (size_t)C * B * c.cb_size;
    for (int f = 0; f < c.F; ++f) {
        const float* lg = c.logits + (size_t)f * frame_logits;
        dX.up(c.x + (size_t)f * B * dim, (size_t)B * dim * 4, st);
        for (int b = 0; b < B; ++b) dLs.up(lg + (size_t)b * c.n_slow, (size_t)c.n_slow * 4, st, (size_t)b * c.ld * 4);
        if (I.par) { SK::rows_rng_words(dRng.as<RngState>(), B, C + 1, dState.as<SeqState>(), dWords.as<uint32_t>(), st); record(); }
        if (I.single)
            SK::sample_slow(d, dLs.as<float>(), c.n_slow, dCfg.as<SampleCfg>(), dRng.as<RngState>(), dState.as<SeqState>(), dX.as<float>(), dXF.as<float>(), st,
                            c.hid ? dHidCell.as<float*>() : nullptr);
        else if (I.rows)
            SK::sample_slow_rows(d, dLs.as<float>(), c.ld, c.n_slow, dCfg.as<SampleCfg>(), dRng.as<RngState>(), B, C + 1, dState.as<SeqState>(), dX.as<float>(),
                                 dXF.as<float>(), st, words, prep_g, prep_A, epoch);
        else
            SK::sample_slow_slots(d, dLs.as<float>(), c.ld, c.n_slow, dCfg.as<SampleCfg>(), dRng.as<SlotRng>(), B, dState.as<SeqState>(), dX.as<float>(),
                                  dXF.as<float>(), st, prep_g, prep_A, epoch, c.cap_frames ? dCap.as<float>() : nullptr, c.cap_frames, I.wide);
        record();
        for (int cb = 0; cb < C; ++cb) {
            dLf.up(lg + (size_t)B * c.n_slow + (size_t)cb * B * c.cb_size, (size_t)B * c.cb_size * 4, st);
            if (I.single)
                SK::sample_fast(d, dLf.as<float>(), cb, C, c.cb_size, dCfg.as<SampleCfg>(), dRng.as<RngState>(), rp, dState.as<SeqState>(), dFast.data(),
                                dXF.as<float>(), dTok.data(), dCb.data(), dX.as<float>(), dCodes.as<uint32_t>(), c.out_cap, st);
            else if (I.rows)
                SK::sample_fast_rows(d, dLf.as<float>(), cb, C, c.cb_size, dCfg.as<SampleCfg>(), dRng.as<RngState>(), B, dState.as<SeqState>(), dFast.data(),
                                     dXF.as<float>(), dTok.data(), dCb.data(), dX.as<float>(), dCodes.as<uint32_t>(), c.out_cap, st, words, prep_g, prep_A);
            else
                SK::sample_fast_slots(d, dLf.as<float>(), cb, C, c.cb_size, dCfg.as<SampleCfg>(), dRng.as<SlotRng>(), rp, B, dState.as<SeqState>(), dFast.data(),
                                      dXF.as<float>(), dTok.data(), dCb.data(), dX.as<float>(), dCodes.as<uint32_t>(), c.out_cap, st, prep_g, prep_A, I.wide);
            record();
        }
    }
    bool ok = true;
    for (const SampDev* b : {&dTok, &dCb, &dFast, &dG, &dCfg, &dRng, &dState, &dMask, &dSeen, &dRing, &dMeta, &dLs, &dLf, &dX, &dXF, &dA, &dEp, &dCodes, &dHid,
                             &dHidCell, &dCap, &dWords})
        ok = b->intact(st) && ok;
    o.guard_ok = ok ? 1 : 0;
}
}  // namespace

void sample_frames_selftest(int device, const fs_sample_case& c, fs_sample_out& o) {
    SampInfo I;
    sample_validate(c, I);
    o.n_launches = I.L;
    for (int i = 0; i < FS_SAMPLE_OUT_COUNT; ++i) o.need[i] = I.per[i] * (size_t)I.L;
    if (c.plan_only) return;
    for (int i = 0; i < FS_SAMPLE_OUT_COUNT; ++i) samp_req(!o.buf[i] || o.cap[i] >= o.need[i], "an output capacity is too small");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) throw Error("no HIP device visible: libfishrt has no CPU fallback (MI355X / gfx950 required)");
    FS_REQUIRE(device >= 0 && device < ndev, "device_id out of range");
    FS_HIP(hipSetDevice(device));
    hipStream_t st = nullptr;
    FS_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    struct StreamGuard { hipStream_t s; ~StreamGuard() { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } } sg{st};
    if (c.wt == FS_GEMV_WT_F32) sample_frames_run<float>(c, I, o, st);
    else sample_frames_run<bf16_t>(c, I, o, st);
}

template struct SampleKernels<bf16_t>;
template struct SampleKernels<float>;
template struct SampleKernels<fp8_t>;

}  // namespace fs
