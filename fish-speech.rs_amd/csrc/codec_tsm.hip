// Device time-scale modification of the vocoder's PCM: WSOLA with a squared-difference measure (no reference kernel: the reference has no
// speed control).  The definition, the order of the error sums and the tie rule are in fs_tsm_plan.h, whose host evaluator computes the same
// bits.  Two launches:
//   * k_tsm_chain: one workgroup per row walks the row's frames in order (frame k's template starts where frame k-1 was placed).  Per frame
//     it stages the template (N floats) and the candidate region (N + 2D floats, rounded up to whole lag blocks) in LDS, gives every thread one
//     (block of 13 adjacent lags) x (one of the 6 segments of i) -- each LDS read of the template and of the region then feeds 13 sums; at the
//     defaults 79 blocks x 6 = 474 of the 512 threads, two waves per SIMD -- combines the 6 partial sums of every lag in the fixed order, and
//     reduces to d* with the tie rule.  No atomics, nothing between workgroups.
//   * k_tsm_ola: one thread per output sample reads the positions and overlap-adds, ragged over the rows like k_resample.
// __fsub_rn / __fmul_rn / __fadd_rn and an explicit fmaf: the build contracts a * b + c into an FMA otherwise, which changes the last bit.
#include "codec_tsm.h"

#include <algorithm>

#include "fs_common.h"

namespace fs {

#define FS_LAUNCH_CHECK() FS_HIP(hipGetLastError())

namespace {

constexpr int kRoundBlocks = kTsmChainWg / kTsmSegs;  // 85 lag blocks (510 threads) per round; the defaults need 79

__device__ __forceinline__ float tsm_fetch(const TsmItem& it, long long a) { return a >= 0 && a < it.n ? it.src[a] : 0.f; }

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

__global__ __launch_bounds__(kTsmChainWg) void k_tsm_chain(const TsmItem* __restrict__ items, double speed, int N, int D) {
    extern __shared__ float lds[];
    const TsmItem it = items[blockIdx.x];
    if (it.K <= 0) return;  // (uniform)
    const int tid = (int)threadIdx.x, Hs = N / 2, seg = (N + kTsmSegs - 1) / kTsmSegs;
    const int nlags = 2 * D + 1, nLB = (nlags + kTsmLags - 1) / kTsmLags, Rlen = nLB * kTsmLags + N - 1;
    float* tmpl = lds;                               // [N]
    float* reg = lds + N;                            // [Rlen]: x[q_k - D ...]
    float* part = reg + ((Rlen + 3) & ~3);           // [13][512]: the partial sums of a round, part[j][thread]
    float* wbe = part + kTsmLags * kTsmChainWg;      // [8] + [8]: the waves' winners
    int* wbd = reinterpret_cast<int*>(wbe + kTsmChainWg / 64);
    if (tid == 0) it.pos[0] = 0;
    const int lbl = tid / kTsmSegs, s = tid - lbl * kTsmSegs;
    const int i0 = s * seg, cnt = min(seg, N - i0);  // (N >= 64: cnt >= 1)
    long long pprev = 0;
    for (long long k = 1; k < it.K; ++k) {
        const long long q = (long long)floor((double)(k * Hs) * speed + 0.5);
        const long long tpos = pprev + Hs, r0 = q - D;
        for (int u = tid; u < N; u += kTsmChainWg) tmpl[u] = tsm_fetch(it, tpos + u);
        for (int u = tid; u < Rlen; u += kTsmChainWg) reg[u] = tsm_fetch(it, r0 + u);
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
        pprev = q + bd;
        if (tid == 0) it.pos[k] = pprev;
    }
}

__global__ __launch_bounds__(kTsmWg) void k_tsm_ola(const TsmItem* __restrict__ items, int n_items, const float* __restrict__ w, int N) {
    const int bid = (int)blockIdx.x, tid = (int)threadIdx.x;
    int ii = 0;
    while (ii + 1 < n_items && items[ii + 1].wg0 <= bid) ++ii;
    const TsmItem it = items[ii];
    const long long m = (long long)(bid - it.wg0) * kTsmWg + tid;
    if (m >= it.out_len) return;
    const int Hs = N / 2;
    const long long k = m / Hs;
    const int i = (int)(m - k * Hs);
    float v;
    if (k == 0) {
        v = tsm_fetch(it, m);
    } else {
        const long long pa = it.pos[k - 1] + Hs + i, pb = it.pos[k] + i;
        v = __fadd_rn(__fmul_rn(w[i + Hs], tsm_fetch(it, pa)), __fmul_rn(w[i], tsm_fetch(it, pb)));
    }
    it.out[m] = v;
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
    }
    FS_REQUIRE(wg < (1ll << 30), "time stretch: too many output samples in one call");
    if (!frames) return;
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
    hipLaunchKernelGGL(k_tsm_chain, dim3((unsigned)n), dim3(kTsmChainWg), lds, st_, (const TsmItem*)d_items_, speed, p.N, p.D);
    FS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_tsm_ola, dim3((unsigned)wg), dim3(kTsmWg), 0, st_, (const TsmItem*)d_items_, n, w, p.N);
    FS_LAUNCH_CHECK();
}

}  // namespace fs
