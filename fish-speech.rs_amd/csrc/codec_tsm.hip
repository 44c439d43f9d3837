// Device time-scale modification of the vocoder's PCM: WSOLA with a squared-difference measure (no reference kernel: the reference has no
// speed control).  The definition, the order of the error sums and the tie rule are in fs_tsm_plan.h, whose host evaluator computes the same
// bits.  Two launches:
//   * k_tsm_chain: one workgroup per row walks the row's frames in order (frame k's template starts where frame k-1 was placed).  Per frame
//     it stages the template (N floats) and the candidate region (N + 2D floats, rounded up to whole lag blocks) in LDS, gives every thread one
//     (block of 13 adjacent lags) x (one of the 6 segments of i) -- each LDS read of the template and of the region then feeds 13 sums; at the
//     defaults 79 blocks x 6 = 474 of the 512 threads, two waves per SIMD -- combines the 6 partial sums of every lag in the fixed order, and
//     reduces to d* with the tie rule.  No atomics, nothing between workgroups.
//   * k_tsm_ola: one thread per output sample reads the positions and overlap-adds, ragged over the rows like k_resample.
// A row is a window of a stream (codec_tsm.h TsmItem): frames [k0, k1) of absolute indices, the input found in a carry row or in the new chunk
// by its absolute index (never by where a chunk began), p_{k0-1} read from the stream's position word and p_{k1-1} written back, and -- the
// chain kernel's last step -- the stream's new carry written to its other carry row, which nothing in either launch reads.  A one-shot row is
// the window k0 = 0, k1 = K with no carry; every frame runs the same instructions in the same order either way.
// __fsub_rn / __fmul_rn / __fadd_rn and an explicit fmaf: the build contracts a * b + c into an FMA otherwise, which changes the last bit.
#include "codec_tsm.h"

#include <algorithm>

#include "fs_common.h"

namespace fs {

#define FS_LAUNCH_CHECK() FS_HIP(hipGetLastError())

namespace {

constexpr int kRoundBlocks = kTsmChainWg / kTsmSegs;  // 85 lag blocks (510 threads) per round; the defaults need 79

// x[a]: the new chunk from in0 on, the carry row for the carry_len samples in front of it, zero elsewhere (the overlap-add and the carry
// step; the chain's staging loops use tsm_span below).  One guarded load whose row and offset are selected per lane
__device__ __forceinline__ float tsm_fetch(const TsmItem& it, long long a) {
    const long long c0 = it.in0 - (long long)it.carry_len;  // (>= 0: the carry holds samples the stream has seen)
    const bool fresh = a >= it.in0;
    const float* row = fresh ? it.src : it.carry;
    const long long at = a - (fresh ? it.in0 : c0);
    return a >= c0 && a >= 0 && a < it.n ? row[at] : 0.f;
}

// The same lookup for a run of indices base + u, u a small non-negative int (the staging loops of the chain kernel): the three boundaries and
// the two row pointers are made relative to `base` once, on the scalar unit, so a lane compares and adds 32-bit offsets only.  A boundary more
// than 2^30 away from base is clamped there; u stays below 2^13, so the comparisons come out the same.  The pointers are formed as integers:
// either may point outside its row, and is only dereferenced at an offset inside it.
struct TsmSpan {
    const float *src, *car;  // x[base + u] = src[u] for mid <= u < hi, car[u] for lo <= u < mid, zero elsewhere
    int lo, mid, hi;
};
__device__ __forceinline__ TsmSpan tsm_span(const TsmItem& it, long long base) {
    const long long c0 = it.in0 - (long long)it.carry_len, far = 1ll << 30;
    TsmSpan s;
    s.lo = (int)min(max(max(c0, 0ll) - base, -far), far);
    s.mid = (int)min(max(it.in0 - base, -far), far);
    s.hi = (int)min(max(it.n - base, -far), far);
    s.src = reinterpret_cast<const float*>(reinterpret_cast<intptr_t>(it.src) + (base - it.in0) * (long long)sizeof(float));
    s.car = reinterpret_cast<const float*>(reinterpret_cast<intptr_t>(it.carry) + (base - c0) * (long long)sizeof(float));
    return s;
}
__device__ __forceinline__ float tsm_at_span(const TsmSpan& s, int u) {
    const float* row = u >= s.mid ? s.src : s.car;
    return u >= s.lo && u < s.hi ? row[u] : 0.f;
}

// (e1, d1) better than (e0, d0): fs_tsm_plan.h tsm_better
__device__ __forceinline__ bool tsm_better_d(float e1, int d1, float e0, int d0) {
    if (e1 < e0) return true;
    if (!(e1 == e0)) return false;
    const int a1 = abs(d1), a0 = abs(d0);
    return a1 < a0 || (a1 == a0 && d1 < d0);
}

// acc[j] += sum_{i < cnt} (t[i] - r[i + j])^2 in ascending i: the candidate samples slide through a register window, one LDS read per i
__device__ __forceinline__ void tsm_accumulate(const float* __restrict__ t, const float* __restrict__ r, int cnt, float (&acc)[kTsmLags]) {
    float w[kTsmLags];
#pragma unroll
    for (int j = 0; j < kTsmLags - 1; ++j) w[j] = r[j];
#pragma unroll 13
    for (int i = 0; i < cnt; ++i) {  // (unrolled by the window's length, the window's rotation is a renaming)
        w[kTsmLags - 1] = r[i + kTsmLags - 1];
        const float tv = t[i];
#pragma unroll
        for (int j = 0; j < kTsmLags; ++j) {
            const float df = __fsub_rn(tv, w[j]);
            acc[j] = fmaf(df, df, acc[j]);
        }
#pragma unroll
        for (int j = 0; j < kTsmLags - 1; ++j) w[j] = w[j + 1];
    }
}

__global__ __launch_bounds__(kTsmChainWg) void k_tsm_chain(const TsmItem* __restrict__ items, int N, int D) {
    extern __shared__ float lds[];
    const TsmItem it = items[blockIdx.x];
    if (it.k1 <= it.k0 && !it.carry_out) return;  // (uniform)
    const int tid = (int)threadIdx.x, Hs = N / 2, seg = (N + kTsmSegs - 1) / kTsmSegs;
    const int nlags = 2 * D + 1, nLB = (nlags + kTsmLags - 1) / kTsmLags, Rlen = nLB * kTsmLags + N - 1;
    float* tmpl = lds;                               // [N]
    float* reg = lds + N;                            // [Rlen]: x[q_k - D ...]
    float* part = reg + ((Rlen + 3) & ~3);           // [13][512]: the partial sums of a round, part[j][thread]
    float* wbe = part + kTsmLags * kTsmChainWg;      // [8] + [8]: the waves' winners
    int* wbd = reinterpret_cast<int*>(wbe + kTsmChainWg / 64);
    long long pprev = 0;
    if (it.k1 > it.k0) {  // (uniform)
        if (it.k0 >= 1) {
            pprev = *it.state;  // (tid 0 writes the word after the frames' barriers)
            if (tid == 0) it.pos[it.k0 - 1 - it.pos0] = pprev;
        } else if (tid == 0) {
            it.pos[0 - it.pos0] = 0;
        }
    }
    const int lbl = tid / kTsmSegs, s = tid - lbl * kTsmSegs;
    const int i0 = s * seg, cnt = min(seg, N - i0);  // (N >= 64: cnt >= 1)
    for (long long k = max(it.k0, 1ll); k < it.k1; ++k) {
        const long long q = (long long)floor((double)(k * Hs) * it.speed + 0.5);
        const long long tpos = pprev + Hs, r0 = q - D;
        const TsmSpan ts = tsm_span(it, tpos), rs = tsm_span(it, r0);
        for (int u = tid; u < N; u += kTsmChainWg) tmpl[u] = tsm_at_span(ts, u);
        for (int u = tid; u < Rlen; u += kTsmChainWg) reg[u] = tsm_at_span(rs, u);
        __syncthreads();
        float be = __builtin_inff();
        int bd = 0;
        for (int rb0 = 0; rb0 < nLB; rb0 += kRoundBlocks) {
            const int lb = rb0 + lbl;
            if (tid < kRoundBlocks * kTsmSegs && lb < nLB) {
                float acc[kTsmLags];
#pragma unroll
                for (int j = 0; j < kTsmLags; ++j) acc[j] = 0.f;
                tsm_accumulate(tmpl + i0, reg + lb * kTsmLags + i0, cnt, acc);
#pragma unroll
                for (int j = 0; j < kTsmLags; ++j) part[j * kTsmChainWg + tid] = acc[j];
            }
            __syncthreads();
            for (int li = tid; li < kRoundBlocks * kTsmLags; li += kTsmChainWg) {
                const int bl = li / kTsmLags, j = li - bl * kTsmLags, lag = (rb0 + bl) * kTsmLags + j;
                if (rb0 + bl < nLB && lag < nlags) {
                    const float* pp = part + j * kTsmChainWg + bl * kTsmSegs;
                    float e = pp[0];
#pragma unroll
                    for (int t = 1; t < kTsmSegs; ++t) e = __fadd_rn(e, pp[t]);
                    const int d = lag - D;
                    if (tsm_better_d(e, d, be, bd)) { be = e; bd = d; }
                }
            }
            __syncthreads();  // (the next round, or the next frame, writes `part` again)
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const float oe = __shfl_xor(be, off);
            const int od = __shfl_xor(bd, off);
            if (tsm_better_d(oe, od, be, bd)) { be = oe; bd = od; }
        }
        if ((tid & 63) == 0) { wbe[tid >> 6] = be; wbd[tid >> 6] = bd; }
        __syncthreads();
        be = wbe[0]; bd = wbd[0];
#pragma unroll
        for (int v = 1; v < kTsmChainWg / 64; ++v)
            if (tsm_better_d(wbe[v], wbd[v], be, bd)) { be = wbe[v]; bd = wbd[v]; }
        pprev = q + __builtin_amdgcn_readfirstlane(bd);  // (every lane holds the same winner: keep the position, and the spans made from it, scalar)
        if (tid == 0) it.pos[k - it.pos0] = pprev;
    }
    if (it.state && it.k1 > it.k0 && tid == 0) *it.state = pprev;
    // the stream's new carry: the last new_carry_len samples it has seen, to its other row
    if (it.carry_out) {
        const long long a0 = it.n - (long long)it.new_carry_len;
        for (int t = tid; t < it.new_carry_len; t += kTsmChainWg) it.carry_out[t] = tsm_fetch(it, a0 + t);
    }
}

__global__ __launch_bounds__(kTsmWg) void k_tsm_ola(const TsmItem* __restrict__ items, int n_items, const float* __restrict__ w, int N) {
    const int bid = (int)blockIdx.x, tid = (int)threadIdx.x;
    int ii = 0;
    while (ii + 1 < n_items && items[ii + 1].wg0 <= bid) ++ii;
    const TsmItem it = items[ii];
    const long long l = (long long)(bid - it.wg0) * kTsmWg + tid;  // relative to the item's first output sample, k0 * Hs
    if (l >= it.out_len) return;
    const int Hs = N / 2;
    const long long m = it.k0 * Hs + l, k = m / Hs;
    const int i = (int)(m - k * Hs);
    float v;
    if (k == 0) {
        v = tsm_fetch(it, m);
    } else {
        const long long pa = it.pos[k - 1 - it.pos0] + Hs + i, pb = it.pos[k - it.pos0] + i;
        v = __fadd_rn(__fmul_rn(w[i + Hs], tsm_fetch(it, pa)), __fmul_rn(w[i], tsm_fetch(it, pb)));
    }
    it.out[l] = v;
}

}  // namespace

TimeStretcher::~TimeStretcher() {
    for (auto& w : windows_) (void)hipFree(w.second);
    if (d_items_) (void)hipFree(d_items_);
}

const float* TimeStretcher::window(int N) {
    auto f = windows_.find(N);
    if (f == windows_.end()) {
        const std::vector<float> w = tsm_window(N);
        float* d = nullptr;
        FS_HIP(hipMalloc(&d, w.size() * sizeof(float)));
        f = windows_.emplace(N, d).first;
        FS_HIP(hipMemcpyAsync(d, w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice, st_));
        FS_HIP(hipStreamSynchronize(st_));  // w goes out of scope
    }
    return f->second;
}

void TimeStretcher::run(const std::vector<TsmItem>& items, double speed, const TsmParams& p) {
    if (items.empty()) return;
    tsm_require_speed(speed);
    tsm_require_params(p);
    h_items_ = items;
    long long wg = 0;
    bool frames = false;
    for (auto& it : h_items_) {
        FS_REQUIRE(it.n >= 0 && it.n < (1ll << 40), "time stretch item: the row's length");
        FS_REQUIRE(it.n == 0 || it.src, "time stretch item: no source row");
        it.out_len = tsm_out_len(it.n, speed);
        it.K = tsm_frames(it.out_len, p);
        FS_REQUIRE(it.out_len == 0 || (it.out && it.pos), "time stretch item: no output or position row");
        FS_REQUIRE(wg < (1ll << 30), "time stretch: too many output samples in one call");
        it.wg0 = (int)wg;
        wg += (it.out_len + kTsmWg - 1) / kTsmWg;
        frames |= it.K > 0;
        // the whole row as one window: frames [0, K), nothing carried in or out
        it.in0 = 0; it.k0 = 0; it.k1 = it.K; it.pos0 = 0; it.speed = speed;
        it.carry = nullptr; it.carry_out = nullptr; it.state = nullptr; it.carry_len = it.new_carry_len = 0;
    }
    FS_REQUIRE(wg < (1ll << 30), "time stretch: too many output samples in one call");
    if (!frames) return;
    launch(p);
}

void TimeStretcher::run_items(const std::vector<TsmItem>& items, const TsmParams& p) {
    if (items.empty()) return;
    tsm_require_params(p);
    h_items_ = items;
    long long wg = 0;
    bool work = false;
    for (auto& it : h_items_) {
        tsm_require_speed(it.speed);
        const long long nf = it.k1 - it.k0;
        FS_REQUIRE(it.in0 >= 0 && it.n >= it.in0 && it.n < (1ll << 40), "time stretch item: the window's place in the stream");
        FS_REQUIRE(it.n == it.in0 || it.src, "time stretch item: no source row");
        FS_REQUIRE(it.carry_len >= 0 && it.new_carry_len >= 0 && (it.carry_len == 0 || it.carry), "time stretch item: no carry row");
        FS_REQUIRE(!it.carry_out || (it.carry_out != it.carry && (long long)it.new_carry_len <= (long long)it.carry_len + it.n - it.in0),
                   "time stretch item: the new carry");
        FS_REQUIRE(it.k0 >= 0 && nf >= 0 && it.pos0 == std::max(it.k0 - 1, 0ll), "time stretch item: the frame range");
        FS_REQUIRE(nf == 0 ? it.out_len == 0 : (it.out_len > (nf - 1) * p.Hs() && it.out_len <= nf * p.Hs()), "time stretch item: the output length");
        FS_REQUIRE(nf == 0 || (it.out && it.pos && (it.k0 == 0 || it.state)), "time stretch item: no output, position row or position word");
        FS_REQUIRE(wg < (1ll << 30), "time stretch: too many output samples in one call");
        it.wg0 = (int)wg;
        wg += (it.out_len + kTsmWg - 1) / kTsmWg;
        work |= nf > 0 || it.carry_out;
    }
    FS_REQUIRE(wg < (1ll << 30), "time stretch: too many output samples in one call");
    if (!work) return;
    launch(p);
}

void TimeStretcher::launch(const TsmParams& p) {
    long long wg = 0;
    for (const auto& it : h_items_) wg += (it.out_len + kTsmWg - 1) / kTsmWg;
    const float* w = window(p.N);
    const size_t bytes = h_items_.size() * sizeof(TsmItem);
    if (bytes > d_items_cap_) {
        if (d_items_) (void)hipFree(d_items_);
        d_items_ = nullptr; d_items_cap_ = 0;
        FS_HIP(hipMalloc(&d_items_, bytes));
        d_items_cap_ = bytes;
    }
    FS_HIP(hipMemcpyAsync(d_items_, h_items_.data(), bytes, hipMemcpyHostToDevice, st_));
    const int n = (int)h_items_.size();
    const int nLB = (2 * p.D + 1 + kTsmLags - 1) / kTsmLags, Rlen = nLB * kTsmLags + p.N - 1;
    const size_t lds = ((size_t)p.N + (size_t)((Rlen + 3) & ~3) + (size_t)kTsmLags * kTsmChainWg + 2 * (kTsmChainWg / 64)) * sizeof(float);  // <= 51 296 B
    hipLaunchKernelGGL(k_tsm_chain, dim3((unsigned)n), dim3(kTsmChainWg), lds, st_, (const TsmItem*)d_items_, p.N, p.D);
    FS_LAUNCH_CHECK();
    if (wg > 0) {
        hipLaunchKernelGGL(k_tsm_ola, dim3((unsigned)wg), dim3(kTsmWg), 0, st_, (const TsmItem*)d_items_, n, w, p.N);
        FS_LAUNCH_CHECK();
    }
}

}  // namespace fs
