// Device loudness normalisation of the vocoder's PCM: BS.1770-4 integrated loudness, one channel, in f64 (no reference kernel: the reference
// has no level control).  The definition is in fs_loud_plan.h, whose host evaluator walks it serially.  Nothing here walks a row: the
// K-weighting cascade is a linear recurrence with a 4 x 4 transition matrix A, so the state after a chunk is M s_in + (the state the chunk
// leaves from zero state), M = A^kLoudChunk.  Four launches, ragged over the rows of a call (a workgroup finds its row by its index):
//   * k_loud_scan: a workgroup stages kLoudSpan = 8192 samples in LDS (rows of 33 floats: lane l reads its 32 samples without a bank
//     conflict), every lane filters its chunk of 32 from zero state, and a Hillis-Steele scan over the 256 lanes with the precomputed powers
//     M^(2^k) turns the chunk states into every lane's entry state as if the workgroup had been entered with zero state.  Written: those
//     entry states and the workgroup's own end state.
//   * k_loud_energy: lane 0 carries the row's state up to this workgroup, s <- M^256 s + (end state of workgroup j), one 4 x 4 product per
//     workgroup in front of it; each lane adds M^l times that to its entry state, filters its chunk again, now with the true state, and sums z^2 in
//     f64 into the (at most two) hops its chunk touches, and takes max |x| in the same sweep.  Written: two partial sums and a peak per chunk.
//   * k_loud_tail: one workgroup per row.  A wave per hop sums the chunk partials of that hop (lane-strided, then a butterfly: one fixed
//     order whatever else the call holds), all lanes compute m_j and l_j, lane 0 applies both gates (additions only) and writes L, the peak,
//     the gain and the counts.
//   * k_loud_gain: y = x * g, fully parallel (not launched when the call only measures).
// Longest dependent chain of one thread: 32 samples of the cascade (about four dependent f64 fmas each) plus 8 scan steps in k_loud_scan; 32
// samples plus one 4 x 4 product per workgroup in front of this one in k_loud_energy (8192 samples each: 162 products for 30 s at 44.1 kHz);
// two f64 additions per 100 ms block in k_loud_tail.  No atomics: a row's result does not depend on what else the call holds.
#include "codec_loud.h"

#include <algorithm>

#include "fs_common.h"

namespace fs {

#define FS_LAUNCH_CHECK() FS_HIP(hipGetLastError())

namespace {

constexpr int kXsRow = kLoudChunk + 1;  // floats of one lane's row in LDS

// the last row whose first workgroup is <= wg (rows without samples have no workgroup and share wg0 with the row behind them)
__device__ __forceinline__ int loud_row_of(const LoudItem* items, int n, int wg) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (items[mid].wg0 <= wg) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// the workgroup's kLoudSpan samples from `base` on, zero behind the row's end (zeros drive the filter on; their z is never counted)
__device__ __forceinline__ void loud_stage(const LoudItem& it, long long base, float* xs) {
    for (int i = threadIdx.x; i < kLoudSpan; i += kLoudWg) {
        const long long a = base + i;
        xs[(i >> 5) * kXsRow + (i & 31)] = a < it.n ? it.src[a] : 0.f;
    }
}

struct LoudC {
    double b0, b1, b2, a1, a2, d1, d2;
};
__device__ __forceinline__ LoudC loud_c(const double* tab) {
    return LoudC{tab[kLoudTabCoef + 0], tab[kLoudTabCoef + 1], tab[kLoudTabCoef + 2], tab[kLoudTabCoef + 3],
                 tab[kLoudTabCoef + 4], tab[kLoudTabCoef + 5], tab[kLoudTabCoef + 6]};
}
// loud_step of fs_loud_plan.h
__device__ __forceinline__ double loud_dstep(const LoudC& c, double x, double (&s)[4]) {
    const double y = c.b0 * x + s[0];
    s[0] = c.b1 * x - c.a1 * y + s[1];
    s[1] = c.b2 * x - c.a2 * y;
    const double z = y + s[2];
    s[2] = -2.0 * y - c.d1 * z + s[3];
    s[3] = y - c.d2 * z;
    return z;
}
// r += m (4 x 4, row-major) * v
__device__ __forceinline__ void loud_mac(const double* m, const double (&v)[4], double (&r)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] += m[i * 4 + 0] * v[0] + m[i * 4 + 1] * v[1] + m[i * 4 + 2] * v[2] + m[i * 4 + 3] * v[3];
}

__global__ __launch_bounds__(kLoudWg) void k_loud_scan(const LoudItem* __restrict__ items, int n_items, const double* __restrict__ tab,
                                                       double* __restrict__ pre, double* __restrict__ agg) {
    __shared__ float xs[kLoudWg * kXsRow];
    __shared__ double sc[4 * kLoudWg];
    const int wg = blockIdx.x, l = threadIdx.x;
    const LoudItem& it = items[loud_row_of(items, n_items, wg)];
    const int wl = wg - it.wg0;
    loud_stage(it, (long long)wl * kLoudSpan, xs);
    __syncthreads();
    const LoudC c = loud_c(tab);
    double s[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 8
    for (int k = 0; k < kLoudChunk; ++k) (void)loud_dstep(c, (double)xs[l * kXsRow + k], s);
#pragma unroll
    for (int j = 0; j < 4; ++j) sc[j * kLoudWg + l] = s[j];
    __syncthreads();
    // inclusive scan: after step k lane l holds the state its own chunk and the 2^(k+1) - 1 chunks in front of it leave from zero state
    for (int k = 0; k < kLoudScanSteps; ++k) {
        const int off = 1 << k;
        const bool on = l >= off;
        double t[4] = {0.0, 0.0, 0.0, 0.0};
        if (on) {
#pragma unroll
            for (int j = 0; j < 4; ++j) t[j] = sc[j * kLoudWg + l - off];
        }
        __syncthreads();
        if (on) {
            loud_mac(tab + kLoudTabP + 16 * k, t, s);
#pragma unroll
            for (int j = 0; j < 4; ++j) sc[j * kLoudWg + l] = s[j];
        }
        __syncthreads();
    }
    const long long chunk = it.chunk0 + (long long)wl * kLoudWg + l;
#pragma unroll
    for (int j = 0; j < 4; ++j) pre[4 * chunk + j] = l ? sc[j * kLoudWg + l - 1] : 0.0;
    if (l == kLoudWg - 1) {
#pragma unroll
        for (int j = 0; j < 4; ++j) agg[4 * (long long)wg + j] = s[j];
    }
}

__global__ __launch_bounds__(kLoudWg) void k_loud_energy(const LoudItem* __restrict__ items, int n_items, const double* __restrict__ tab,
                                                         const double* __restrict__ pre, const double* __restrict__ agg,
                                                         double* __restrict__ pe, float* __restrict__ pk) {
    __shared__ float xs[kLoudWg * kXsRow];
    __shared__ double sw[4];
    const int wg = blockIdx.x, l = threadIdx.x;
    const LoudItem& it = items[loud_row_of(items, n_items, wg)];
    const int wl = wg - it.wg0;
    loud_stage(it, (long long)wl * kLoudSpan, xs);
    if (l == 0) {  // the row's state at this workgroup's first sample
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        for (int j = 0; j < wl; ++j) {
            const double* e = agg + 4 * (long long)(it.wg0 + j);
            double r[4] = {e[0], e[1], e[2], e[3]};
            loud_mac(tab + kLoudTabP + 16 * kLoudScanSteps, s, r);
#pragma unroll
            for (int i = 0; i < 4; ++i) s[i] = r[i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) sw[i] = s[i];
    }
    __syncthreads();
    const long long chunk = it.chunk0 + (long long)wl * kLoudWg + l;
    const LoudC c = loud_c(tab);
    const double in[4] = {sw[0], sw[1], sw[2], sw[3]};
    double s[4] = {pre[4 * chunk + 0], pre[4 * chunk + 1], pre[4 * chunk + 2], pre[4 * chunk + 3]};
    loud_mac(tab + kLoudTabLane + 16 * l, in, s);
    // the chunk's first sample, its hop, and how many of its samples that hop still takes (n <= 2^30: the row's indices fit 32 bits)
    const unsigned a0 = (unsigned)wl * (unsigned)kLoudSpan + (unsigned)l * (unsigned)kLoudChunk, h = (unsigned)it.h;
    const unsigned bnd = (a0 / h + 1u) * h - a0, left = (long long)a0 < it.n ? (unsigned)min((long long)kLoudChunk, it.n - (long long)a0) : 0u;
    double e0 = 0.0, e1 = 0.0;
    float peak = 0.f;
#pragma unroll 8
    for (int k = 0; k < kLoudChunk; ++k) {
        const float xf = xs[l * kXsRow + k];
        const double z = loud_dstep(c, (double)xf, s);
        const double z2 = (unsigned)k < left ? z * z : 0.0;
        if ((unsigned)k < bnd) e0 += z2; else e1 += z2;
        peak = fmaxf(peak, fabsf(xf));  // (fmaxf returns the other operand for a NaN)
    }
    pe[2 * chunk] = e0;
    pe[2 * chunk + 1] = e1;
    pk[chunk] = peak;
}

struct LoudGainArgs {
    double target, g_max, peak_lin;  // target_lufs, 10^(max_gain_db / 20), 10^(peak_db / 20)
    int apply;                       // 0: measure only, gain 1
};

__global__ __launch_bounds__(kLoudWg) void k_loud_tail(const LoudItem* __restrict__ items, const double* __restrict__ pe,
                                                       const float* __restrict__ pk, double* __restrict__ ws, LoudResult* __restrict__ res,
                                                       LoudGainArgs ga) {
    __shared__ float pks[kLoudWg];
    const LoudItem& it = items[blockIdx.x];
    const int l = threadIdx.x, wave = l >> 6, lane = l & 63, nb = it.nb, nblk = nb >= 4 ? nb - 3 : 0;
    const unsigned h = (unsigned)it.h;
    double* sh = ws + it.hop0;                       // s_i
    double *mj = sh + nb, *lj = sh + 2 * (long long)nb;  // m_j, l_j
    for (int i = wave; i < nb; i += kLoudWg / 64) {
        const unsigned lo = (unsigned)i * h, c_lo = lo >> 5, c_hi = (lo + h - 1u) >> 5;
        double acc = 0.0;
        for (unsigned cc = c_lo + (unsigned)lane; cc <= c_hi; cc += 64u) {
            const bool first = (cc << 5) / h == (unsigned)i;  // the chunk begins in hop i: its front part; else it began in hop i - 1
            acc += pe[2 * (it.chunk0 + (long long)cc) + (first ? 0 : 1)];
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
        if (lane == 0) sh[i] = acc;
    }
    float peak = 0.f;
    for (long long cc = l; cc < (long long)it.nwg * kLoudWg; cc += kLoudWg) peak = fmaxf(peak, pk[it.chunk0 + cc]);
    pks[l] = peak;
    __syncthreads();
    for (int off = kLoudWg / 2; off >= 1; off >>= 1) {
        if (l < off) pks[l] = fmaxf(pks[l], pks[l + off]);
        __syncthreads();
    }
    for (int j = l; j < nblk; j += kLoudWg) {
        const double m = (sh[j] + sh[j + 1] + sh[j + 2] + sh[j + 3]) / (4.0 * (double)h);
        mj[j] = m;
        lj[j] = -0.691 + 10.0 * log10(m);
    }
    __syncthreads();
    if (l != 0) return;
    LoudResult r;
    r.lufs = -INFINITY; r.peak = pks[0]; r.gain = 1.f; r.blocks_total = nblk; r.blocks_kept = 0;
    double sum = 0.0;
    int kept = 0;
    for (int j = 0; j < nblk; ++j)
        if (lj[j] > -70.0) { sum += mj[j]; ++kept; }
    if (kept) {
        const double gamma = -0.691 + 10.0 * log10(sum / (double)kept) - 10.0;
        sum = 0.0; kept = 0;
        for (int j = 0; j < nblk; ++j)
            if (lj[j] > -70.0 && lj[j] > gamma) { sum += mj[j]; ++kept; }
        if (kept) {
            r.blocks_kept = kept;
            r.lufs = -0.691 + 10.0 * log10(sum / (double)kept);
            if (ga.apply) {
                double g = pow(10.0, (ga.target - r.lufs) / 20.0);
                g = fmin(g, ga.g_max);
                if (r.peak > 0.f) g = fmin(g, ga.peak_lin / (double)r.peak);
                r.gain = (float)g;
            }
        }
    }
    res[blockIdx.x] = r;
}

__global__ __launch_bounds__(kLoudWg) void k_loud_gain(const LoudItem* __restrict__ items, int n_items, const LoudResult* __restrict__ res) {
    const int wg = blockIdx.x, row = loud_row_of(items, n_items, wg);
    const LoudItem& it = items[row];
    if (!it.out) return;
    const float g = res[row].gain;
    const long long base = (long long)(wg - it.wg0) * kLoudSpan;
#pragma unroll 4
    for (int k = 0; k < kLoudChunk; ++k) {
        const long long a = base + k * kLoudWg + threadIdx.x;
        if (a < it.n) it.out[a] = __fmul_rn(it.src[a], g);
    }
}

}  // namespace

void Loudness::Buf::ensure(size_t bytes) {
    if (bytes <= cap) return;
    if (p) (void)hipFree(p);
    p = nullptr; cap = 0;
    FS_HIP(hipMalloc(&p, bytes));
    cap = bytes;
}
Loudness::Buf::~Buf() { if (p) (void)hipFree(p); }

Loudness::~Loudness() {
    for (auto& t : tables_) (void)hipFree(t.second);
}

const double* Loudness::tables(int rate) {
    auto f = tables_.find(rate);
    if (f != tables_.end()) return f->second;
    const std::vector<double> t = loud_tables(rate);
    double* d = nullptr;
    FS_HIP(hipMalloc(&d, t.size() * sizeof(double)));
    tables_[rate] = d;
    FS_HIP(hipMemcpyAsync(d, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice, st_));
    FS_HIP(hipStreamSynchronize(st_));  // (t leaves scope)
    return d;
}

void Loudness::run(const std::vector<LoudItem>& items, int rate, const LoudParams* p) {
    if (items.empty()) return;
    loud_require_rate(rate);
    if (p) loud_require_params(*p);
    h_items_ = items;
    const int h = loud_hop(rate);
    long long wg = 0, words = 0;
    bool apply = false;
    for (auto& it : h_items_) {
        FS_REQUIRE(it.n >= 0 && it.n <= kLoudMaxSamples, "loudness item: the row's length");
        FS_REQUIRE(it.n == 0 || it.src, "loudness item: no source row");
        FS_REQUIRE(wg < (1ll << 30), "loudness: too many samples in one call");
        it.wg0 = (int)wg;
        it.nwg = (int)((it.n + kLoudSpan - 1) / kLoudSpan);
        it.chunk0 = wg * kLoudWg;
        it.h = h;
        it.nb = (int)loud_hops(it.n, rate);
        it.hop0 = words;
        words += 3 * (long long)it.nb;
        wg += it.nwg;
        apply |= p && it.out && it.n;
    }
    FS_REQUIRE(wg < (1ll << 30), "loudness: too many samples in one call");
    static_assert(sizeof(LoudResult) == 24, "fs_loud_result is copied out as it is");
    const size_t n = h_items_.size(), chunks = (size_t)wg * kLoudWg;
    const double* tab = tables(rate);
    d_items_.ensure(n * sizeof(LoudItem));
    d_res_.ensure(n * sizeof(LoudResult));
    d_pre_.ensure(std::max<size_t>(chunks, 1) * 4 * sizeof(double));
    d_agg_.ensure(std::max<size_t>((size_t)wg, 1) * 4 * sizeof(double));
    d_pe_.ensure(std::max<size_t>(chunks, 1) * 2 * sizeof(double));
    d_pk_.ensure(std::max<size_t>(chunks, 1) * sizeof(float));
    d_ws_.ensure(std::max<size_t>((size_t)words, 1) * sizeof(double));
    FS_HIP(hipMemcpyAsync(d_items_.p, h_items_.data(), n * sizeof(LoudItem), hipMemcpyHostToDevice, st_));
    const LoudItem* di = (const LoudItem*)d_items_.p;
    if (wg > 0) {
        hipLaunchKernelGGL(k_loud_scan, dim3((unsigned)wg), dim3(kLoudWg), 0, st_, di, (int)n, tab, (double*)d_pre_.p, (double*)d_agg_.p);
        FS_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_loud_energy, dim3((unsigned)wg), dim3(kLoudWg), 0, st_, di, (int)n, tab, (const double*)d_pre_.p,
                           (const double*)d_agg_.p, (double*)d_pe_.p, (float*)d_pk_.p);
        FS_LAUNCH_CHECK();
    }
    LoudGainArgs ga{};
    ga.apply = p ? 1 : 0;
    if (p) { ga.target = p->target_lufs; ga.g_max = std::pow(10.0, p->max_gain_db / 20.0); ga.peak_lin = std::pow(10.0, p->peak_db / 20.0); }
    hipLaunchKernelGGL(k_loud_tail, dim3((unsigned)n), dim3(kLoudWg), 0, st_, di, (const double*)d_pe_.p, (const float*)d_pk_.p,
                       (double*)d_ws_.p, (LoudResult*)d_res_.p, ga);
    FS_LAUNCH_CHECK();
    if (apply && wg > 0) {
        hipLaunchKernelGGL(k_loud_gain, dim3((unsigned)wg), dim3(kLoudWg), 0, st_, di, (int)n, (const LoudResult*)d_res_.p);
        FS_LAUNCH_CHECK();
    }
}

}  // namespace fs
