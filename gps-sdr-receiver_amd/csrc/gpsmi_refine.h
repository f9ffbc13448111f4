// Refinement of weak / deep acquisition hits (gpsmi_acq_refine, include/gpsmi.h; DESIGN.md 4.2f;
// numpy restatement: tests/refine_ref.py).  Kernels and their host-side plan; the entry points sit
// beside the acquisition handle in gpsmi_acq.hip.
//
//   refine_prompt_kernel  one workgroup per (hit, run of kRefMsPerWg consecutive milliseconds): the
//                         replica staged in LDS once, every sample of a window loaded, decoded and
//                         mixed once (integer carrier phase) and multiplied into the early, prompt
//                         and late sums; wave shuffles, then LDS in wave order.
//   refine_grid_kernel    one workgroup per (hit, four df): the prompt row in LDS, a wave per df, a
//                         lane per 20-ms block; the 20 edges of a block are one sliding sum.
//   refine_final_kernel   one workgroup per hit: first-index argmax, the lower median by bisection
//                         on the float bits (integer counts), the bit sums of the three taps at the
//                         peak, and the record.  No float atomics anywhere; every sum has one order.
#pragma once
#include <cmath>
#include <vector>

#include "gpsmi_common.h"
#include "gpsmi_windows.h"

namespace gpsmi {

constexpr int kRefMsPerWg = 8;
constexpr int kRefMaxDf = 1024;
constexpr int kRefMaxHits = 64;
constexpr int kRefEdges = 20;                     // milliseconds per data bit
static_assert(GPSMI_REFINE_MAX_MS * sizeof(float2) <= 64 * 1024, "the prompt row must fit 64 KiB of LDS");

struct RefHit {                                   // one hit as the kernels see it
    unsigned long long inc;                       // freq_hz / fs in 0.64 fixed point
    double freq_hz;
    int prn, delay;
};

// x exp(-j 2 pi (idx * inc mod 2^64) / 2^64): the top 24 bits of the phase as a signed fraction of pi
__device__ __forceinline__ float2 ref_rotate(float2 x, unsigned long long idx, unsigned long long inc) {
    const unsigned long long ph = idx * inc;
    const float a = (float)((long long)ph >> 40) * 0x1p-23f;          // [-1, 1), exact
    float sn, cs;
    sincospif(a, &sn, &cs);
    return make_float2(x.x * cs + x.y * sn, x.y * cs - x.x * sn);
}

__device__ __forceinline__ float ref_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// P[hit][tap][k], taps early / prompt / late.  start[hit][k] = n_k, the first sample of the prompt
// window of millisecond k (the host has checked n_k - tap >= 0 and n_k + cs + tap <= n).
// LDS: the replica [cs], then the waves' partial sums [kRefMsPerWg][4][6].
template <int FMT>
__global__ __launch_bounds__(256) void refine_prompt_kernel(
    const void* __restrict__ iq, const float* __restrict__ rep_time, const RefHit* __restrict__ hits,
    const long long* __restrict__ start, int cs, int tap, int n_ms, float2* __restrict__ P) {
    extern __shared__ __attribute__((aligned(16))) float ref_lds[];
    float* rep = ref_lds;
    float* red = ref_lds + cs;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int hit = blockIdx.y, k0 = blockIdx.x * kRefMsPerWg;
    const RefHit hh = hits[hit];
    const float* R = rep_time + (size_t)hh.prn * cs;
    for (int i = t; i < cs; i += 256) rep[i] = R[i];
    __syncthreads();
    const int span = cs + 2 * tap;
    const int nk = n_ms - k0 < kRefMsPerWg ? n_ms - k0 : kRefMsPerWg;
    for (int q = 0; q < nk; ++q) {
        const long long j0 = start[(size_t)hit * n_ms + k0 + q] - tap;
        float acc[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) acc[c] = 0.f;
        // sample u of the span is replica point u of the early window, u - tap of the prompt
        // window and u - 2 tap of the late one
        for (int u = t; u < span; u += 256) {
            const long long j = j0 + u;
            const float2 y = ref_rotate(load_iq<FMT>(iq, (size_t)j), (unsigned long long)j, hh.inc);
            const int up = u - tap, ul = u - 2 * tap;
            if (u < cs) { const float r = rep[u]; acc[0] += y.x * r; acc[1] += y.y * r; }
            if (up >= 0 && up < cs) { const float r = rep[up]; acc[2] += y.x * r; acc[3] += y.y * r; }
            if (ul >= 0) { const float r = rep[ul]; acc[4] += y.x * r; acc[5] += y.y * r; }
        }
#pragma unroll
        for (int c = 0; c < 6; ++c) acc[c] = ref_wave_sum(acc[c]);
        if (lane == 0) {
#pragma unroll
            for (int c = 0; c < 6; ++c) red[(q * 4 + wave) * 6 + c] = acc[c];
        }
    }
    __syncthreads();
    if (t < nk * 6) {
        const int q = t / 6, c = t % 6;
        float s = red[(q * 4 + 0) * 6 + c];
        s += red[(q * 4 + 1) * 6 + c];
        s += red[(q * 4 + 2) * 6 + c];
        s += red[(q * 4 + 3) * 6 + c];
        float* o = reinterpret_cast<float*>(P + ((size_t)hit * 3 + (c >> 1)) * n_ms + k0 + q);
        o[c & 1] = s;
    }
}

// M[hit][d][e] = sum_b |sum_{k = e + 20 b}^{e + 20 b + 19} P[hit][1][k] exp(-j 2 pi df_d k / 1000)|^2,
// b < B = n_ms / 20 - 1.  Lane l of the wave of df d takes blocks l, l + 64, ...: the sum of edge 0
// from 20 derotated prompts, then edge e from edge e - 1 by dropping one prompt and taking the next.
__global__ __launch_bounds__(256) void refine_grid_kernel(
    const float2* __restrict__ P, const unsigned long long* __restrict__ dfinc, int n_df, int n_ms,
    float* __restrict__ M) {
    extern __shared__ __attribute__((aligned(16))) float ref_lds[];
    float2* row = reinterpret_cast<float2*>(ref_lds);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, hit = blockIdx.y;
    const float2* P0 = P + ((size_t)hit * 3 + 1) * n_ms;
    for (int i = t; i < n_ms; i += 256) row[i] = P0[i];
    __syncthreads();
    const int d = blockIdx.x * 4 + wave;
    if (d >= n_df) return;
    const unsigned long long inc = dfinc[d];
    const int B = n_ms / kRefEdges - 1;
    float acc[kRefEdges];
#pragma unroll
    for (int e = 0; e < kRefEdges; ++e) acc[e] = 0.f;
    for (int b = lane; b < B; b += 64) {
        const int kb = b * kRefEdges;
        float2 z[kRefEdges];
        float sr = 0.f, si = 0.f;
#pragma unroll
        for (int i = 0; i < kRefEdges; ++i) {
            z[i] = ref_rotate(row[kb + i], (unsigned long long)(kb + i), inc);
            sr += z[i].x; si += z[i].y;
        }
        acc[0] += sr * sr + si * si;
#pragma unroll
        for (int e = 1; e < kRefEdges; ++e) {
            const int k = kb + kRefEdges - 1 + e;
            const float2 zn = ref_rotate(row[k], (unsigned long long)k, inc);
            sr += zn.x - z[e - 1].x; si += zn.y - z[e - 1].y;
            acc[e] += sr * sr + si * si;
        }
    }
#pragma unroll
    for (int e = 0; e < kRefEdges; ++e) acc[e] = ref_wave_sum(acc[e]);
    if (lane == 0) {
        float* o = M + ((size_t)hit * n_df + d) * kRefEdges;
#pragma unroll
        for (int e = 0; e < kRefEdges; ++e) o[e] = acc[e];
    }
}

// sum over the workgroup: wave shuffles, then the four waves in order (s4: 4 floats of LDS)
__device__ __forceinline__ float ref_block_sum(float v, float* s4, int t) {
    v = ref_wave_sum(v);
    __syncthreads();
    if ((t & 63) == 0) s4[t >> 6] = v;
    __syncthreads();
    return ((s4[0] + s4[1]) + s4[2]) + s4[3];
}

__global__ __launch_bounds__(256) void refine_final_kernel(
    const float2* __restrict__ P, const float* __restrict__ M, const unsigned long long* __restrict__ dfinc,
    const double* __restrict__ dfs, const RefHit* __restrict__ hits, int n_df, int n_ms, int tap,
    double step_hz, float min_ratio, gpsmi_refine_out* __restrict__ out) {
    __shared__ float s_v[256];
    __shared__ int s_i[256];
    __shared__ int s_c[4];
    __shared__ float s_f[4];
    const int t = threadIdx.x, hit = blockIdx.x, N = n_df * kRefEdges;
    const float* Mh = M + (size_t)hit * N;
    // first-index argmax (M >= 0; a NaN never wins)
    float bv = -1.f;
    int bi = 0x7fffffff;
    for (int i = t; i < N; i += 256) {
        const float v = Mh[i];
        if (v > bv) { bv = v; bi = i; }
    }
    s_v[t] = bv; s_i[t] = bi;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) {
            const float v = s_v[t + o];
            const int i = s_i[t + o];
            if (v > s_v[t] || (v == s_v[t] && i < s_i[t])) { s_v[t] = v; s_i[t] = i; }
        }
        __syncthreads();
    }
    const float peak = s_v[0];
    const int best = s_i[0] < N ? s_i[0] : 0;
    // lower median, rank (N - 1) / 2 from 0: the largest bit pattern v with #{M < v} <= rank (the
    // patterns of non-negative floats order as unsigned integers)
    const int rank = (N - 1) / 2;
    unsigned med = 0;
    for (int bit = 31; bit >= 0; --bit) {
        const unsigned cand = med | (1u << bit);
        int cnt = 0;
        for (int i = t; i < N; i += 256) cnt += __float_as_uint(Mh[i]) < cand ? 1 : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
        __syncthreads();
        if ((t & 63) == 0) s_c[t >> 6] = cnt;
        __syncthreads();
        if (s_c[0] + s_c[1] + s_c[2] + s_c[3] <= rank) med = cand;
    }
    const float median = __uint_as_float(med);
    // the bit sums of the three taps at the peak, and mu of the prompt tap
    const int d = best / kRefEdges, e = best % kRefEdges, B = n_ms / kRefEdges - 1;
    const unsigned long long inc = dfinc[d];
    float tm[3] = {0.f, 0.f, 0.f}, mu = 0.f;
    for (int b = t; b < B; b += 256) {
#pragma unroll
        for (int tp = 0; tp < 3; ++tp) {
            const float2* row = P + ((size_t)hit * 3 + tp) * n_ms;
            float sr = 0.f, si = 0.f, w = 0.f;
            for (int i = 0; i < kRefEdges; ++i) {
                const int k = e + b * kRefEdges + i;
                const float2 x = row[k];
                const float2 z = ref_rotate(x, (unsigned long long)k, inc);
                sr += z.x; si += z.y;
                w += x.x * x.x + x.y * x.y;
            }
            const float nb = sr * sr + si * si;
            tm[tp] += nb;
            if (tp == 1 && w > 0.f) mu += nb / w;        // (a bit of 20 zero prompts counts 0)
        }
    }
    tm[0] = ref_block_sum(tm[0], s_f, t);
    tm[1] = ref_block_sum(tm[1], s_f, t);
    tm[2] = ref_block_sum(tm[2], s_f, t);
    mu = ref_block_sum(mu, s_f, t) / (float)B;
    if (t != 0) return;
    const RefHit hh = hits[hit];
    gpsmi_refine_out r;
    r.prn = hh.prn; r.edge_ms = e; r.n_bits = B;
    r.peak = peak; r.median = median; r.ratio = peak / median;
    r.confirmed = r.ratio > min_ratio ? 1 : 0;
    double f = hh.freq_hz + dfs[d];
    if (d > 0 && d < n_df - 1) {
        const double l = Mh[(d - 1) * kRefEdges + e], c = peak, rr = Mh[(d + 1) * kRefEdges + e];
        const double den = l - 2.0 * c + rr;
        if (den != 0.0) f += 0.5 * (l - rr) / den * step_hz;
    }
    r.f_hz = f;
    r.tap_metric[0] = tm[0]; r.tap_metric[1] = tm[1]; r.tap_metric[2] = tm[2];
    if (tm[0] > tm[1] || tm[2] > tm[1]) {
        r.code_phase = -1.0;
    } else {
        const double E = tm[0], Pp = tm[1], L = tm[2], den = E - 2.0 * Pp + L;
        r.code_phase = (double)hh.delay + (den != 0.0 ? 0.5 * (E - L) / den * (double)tap : 0.0);
    }
    r.mu = mu;
    r.cn0_dbhz = mu > 1.0f ? (float)(10.0 * log10(1000.0 * ((double)mu - 1.0) / (20.0 - (double)mu)))
                           : __builtin_nanf("");
    out[hit] = r;
}

// ---- the plan: everything a call derives from its arguments, on the host, no GPU --------------
struct RefPlan {
    int cs = 0, n_ms = 0, tap = 0, n_df = 0;
    double step = 0.0, half = 0.0;
    float min_ratio = 0.f;
    size_t hi = 0;                                // one past the last sample any window reads
    std::vector<RefHit> hits;
    std::vector<long long> start;                 // [nhits][n_ms]
    std::vector<unsigned long long> dfinc;        // [n_df]
    std::vector<double> dfs;                      // [n_df]
};

// Validates the arguments of gpsmi_acq_refine (the handle aside) and fills the plan (pl may be null).
inline int ref_plan(int cs, size_t n, const gpsmi_refine_hit* hits, int nhits, const gpsmi_refine_cfg* c,
                    RefPlan* pl) {
    static const char* const fn = "gpsmi_acq_refine";
    GPSMI_REQUIRE_IN(fn, hits && c, "null argument");
    GPSMI_REQUIRE_IN(fn, nhits >= 1 && nhits <= kRefMaxHits, "nhits out of range 1..64");
    GPSMI_REQUIRE_IN(fn, c->n_ms >= 40 && c->n_ms % 20 == 0, "n_ms must be a multiple of 20, >= 40");
    GPSMI_REQUIRE_IN(fn, std::isfinite(c->carrier_hz) && c->carrier_hz > 0.0, "carrier_hz must be positive");
    GPSMI_REQUIRE_IN(fn, std::isfinite(c->f_offset_hz), "f_offset_hz must be finite");
    GPSMI_REQUIRE_IN(fn, c->df_step_hz >= 0.0 && std::isfinite(c->df_step_hz), "df_step_hz must be >= 0 (0: 2 Hz)");
    GPSMI_REQUIRE_IN(fn, c->df_half_hz >= 0.0 && std::isfinite(c->df_half_hz), "df_half_hz must be >= 0 (0: 120 Hz)");
    GPSMI_REQUIRE_IN(fn, c->tap_samples >= 0, "tap_samples must be >= 1 (0: the default)");
    GPSMI_REQUIRE_IN(fn, c->min_ratio >= 0.f, "min_ratio must be >= 0 (0: 2.5), not NaN");
    const double step = c->df_step_hz > 0.0 ? c->df_step_hz : 2.0;
    const double half = c->df_half_hz > 0.0 ? c->df_half_hz : 120.0;
    const double pts = std::floor(2.0 * half / step + 1e-9) + 1.0;
    GPSMI_REQUIRE_IN(fn, pts <= (double)kRefMaxDf, "more than 1024 grid points");
    GPSMI_REQUIRE_IN(fn, half < 500.0, "df_half_hz must stay below 500 Hz (the prompts are 1 ms apart)");
    if (cs != 2048 && cs != 16368)
        return fail(GPSMI_E_UNSUPPORTED, "gpsmi_acq_refine: code_samples 2048 and 16368 only (%d)", cs);
    if (c->n_ms > GPSMI_REFINE_MAX_MS)
        return fail(GPSMI_E_UNSUPPORTED, "gpsmi_acq_refine: n_ms %d beyond the %d the grid kernel's LDS holds",
                    c->n_ms, GPSMI_REFINE_MAX_MS);
    const int tap = c->tap_samples > 0 ? c->tap_samples : (cs == 2048 ? 1 : 8);
    GPSMI_REQUIRE_IN(fn, tap <= cs / 4, "tap_samples beyond a quarter of the code");
    GPSMI_REQUIRE_IN(fn, n >= ((size_t)c->n_ms + 2) * cs + tap,
                     "iq shorter than (n_ms + 2) code periods + tap_samples");
    const double fs = 1000.0 * cs;
    RefPlan tmp;
    RefPlan& p = pl ? *pl : tmp;
    p.cs = cs; p.n_ms = c->n_ms; p.tap = tap; p.n_df = (int)pts; p.step = step; p.half = half;
    p.min_ratio = c->min_ratio > 0.f ? c->min_ratio : 2.5f;
    p.hi = 0;
    try {
        p.hits.resize(nhits);
        p.start.resize((size_t)nhits * c->n_ms);
        p.dfinc.resize(p.n_df);
        p.dfs.resize(p.n_df);
    } catch (const std::bad_alloc&) {
        return fail(GPSMI_E_NOMEM, "gpsmi_acq_refine: out of host memory");
    }
    for (int i = 0; i < p.n_df; ++i) {
        p.dfs[i] = -half + (double)i * step;
        p.dfinc[i] = ref_phase_inc(p.dfs[i], 1000.0);
    }
    for (int hdx = 0; hdx < nhits; ++hdx) {
        const gpsmi_refine_hit& g = hits[hdx];
        GPSMI_REQUIRE_IN(fn, g.prn >= 1 && g.prn <= GPSMI_MAX_PRN, "prn out of range 1..37");
        GPSMI_REQUIRE_IN(fn, g.delay >= 0 && g.delay < cs, "delay out of range 0..code_samples - 1");
        GPSMI_REQUIRE_IN(fn, std::isfinite(g.freq_hz) && std::fabs(g.freq_hz) < 0.5 * fs, "freq_hz out of range");
        const long long d0 = g.delay < tap ? (long long)g.delay + cs : g.delay;
        p.hits[hdx] = RefHit{ref_phase_inc(g.freq_hz, fs), g.freq_hz, g.prn, g.delay};
        for (int k = 0; k < c->n_ms; ++k) {
            // m[k] of gpsmi.h: float64 left to right, ties to even
            const double m = std::nearbyint(-(g.freq_hz - c->f_offset_hz) / c->carrier_hz * (double)k * (double)cs);
            GPSMI_REQUIRE_IN(fn, std::fabs(m) < 1e15, "code slide out of range");
            const long long nk = (long long)k * cs + d0 + (long long)m;
            GPSMI_REQUIRE_IN(fn, nk - tap >= 0 && (unsigned long long)(nk + cs + tap) <= (unsigned long long)n,
                        "a window of the code slide leaves iq");
            p.start[(size_t)hdx * c->n_ms + k] = nk;
            if ((size_t)(nk + cs + tap) > p.hi) p.hi = (size_t)(nk + cs + tap);
        }
    }
    return GPSMI_OK;
}

}  // namespace gpsmi
