// Cancellation of strong satellites ahead of the weak searches (gpsmi_acq_cancel, include/gpsmi.h;
// DESIGN.md 4.2j; numpy restatement: tests/cancel_ref.py).  Kernels and their host-side plan; the
// entry points sit beside the acquisition handle in gpsmi_acq.hip.
//
//   cancel_decode_kernel  step 0 of raw input: uint16 -> complex64, gpsmi_dev_unpack_u8iq's arithmetic.
//   cancel_kernel         one launch per satellite, one 256-thread workgroup per code period
//                         (window) of it, in place on the complex64 output.  Pass 1 reads the window
//                         from global memory and accumulates the three projections, the six Gram sums
//                         and the energy (13 float64 sums per thread of float32 factors; DPP within
//                         a row of 16 lanes, LDS across the 16 rows, one order); thread 0 solves the
//                         3 x 3 normal equations in double; pass 2 reads the window again (from L2),
//                         subtracts and stores.  Nothing of a window is staged in LDS: a window is
//                         16 KiB at 2048 and 131 KiB at 16368.
//
// Races: the windows of one satellite are disjoint sample ranges, so the workgroups of a launch
// touch disjoint memory; the launches of the satellites follow one another on the handle's stream.
// No atomics, no communication between workgroups.  Every workgroup writes its result into the
// record of its own window; the host adds the records in index order, in double: the same
// arguments give the same bytes.
#pragma once
#include <cmath>
#include <vector>

#include "gpsmi_common.h"
#include "gpsmi_refine.h"
#include "gpsmi_stats.h"
#include "gpsmi_windows.h"

namespace gpsmi {

constexpr int kCancelMaxSats = 32;
constexpr int kCancelSums = 13;                   // 3 complex projections, 6 Gram sums, the energy
constexpr double kCancelPivotMin = 1.0e-6;        // of trace(G)

struct CancelWin {                                // one window as the kernel sees it
    long long lo;                                 // its first sample
    int len;                                      // its samples, >= 1
    int r0;                                       // (lo - j) mod cs: the replica point of sample lo, tap d = 0
};
struct CancelRes {                                // what a window leaves; all zero: skipped
    float2 c[3];                                  // taps d = -1, 0, +1
    double e_in, e_rem;
    int done, pad;
};

__global__ __launch_bounds__(256) void cancel_decode_kernel(const uint16_t* __restrict__ raw, size_t n,
                                                            float2* __restrict__ out) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = load_iq<1>(raw, i);
}

// exp(+j 2 pi ((idx + 1) * inc mod 2^64) / 2^64), the carrier of sample idx (SEC_TIME counts from 1):
// the phase is an integer, exact at any index; its top 24 bits give sine and cosine (ref_rotate)
__device__ __forceinline__ float2 cancel_carrier(unsigned long long idx, unsigned long long inc) {
    const unsigned long long ph = (idx + 1ull) * inc;
    float sn, cs;
    sincospif((float)((long long)ph >> 40) * 0x1p-23f, &sn, &cs);
    return make_float2(cs, sn);
}

// the replica at taps d = -1, 0, +1 of sample u of a window: points i + 1, i, i - 1 (mod cs), i = r0 + u
__device__ __forceinline__ void cancel_taps(const float* __restrict__ R, int r0, int u, int cs, float& rm,
                                            float& r0v, float& rp) {
    int i = r0 + u;                               // < 2.02 cs + 1: a window is at most 1.011 cs + 1 samples
    i -= i >= cs ? cs : 0;
    i -= i >= cs ? cs : 0;
    rm = R[i + 1 == cs ? 0 : i + 1];
    r0v = R[i];
    rp = R[i == 0 ? cs - 1 : i - 1];
}

__global__ __launch_bounds__(256) void cancel_kernel(float2* __restrict__ y, const float* __restrict__ rep,
                                                     const CancelWin* __restrict__ wins, unsigned long long inc,
                                                     int cs, int min_window, CancelRes* __restrict__ res) {
    __shared__ double red[16][kCancelSums];        // the 16 DPP rows of the workgroup, in thread order
    __shared__ float2 s_c[3];
    __shared__ int s_done;
    const int t = threadIdx.x;
    const CancelWin w = wins[blockIdx.x];
    if (w.len < min_window) return;               // (its record stays zero: skipped)
    float2* yw = y + w.lo;
    // float64 products and sums of the float32 factors: at 16368 the three replicas are nearly
    // parallel (neighbouring shifts correlate to 15 / 16) and G nearly singular; float32 sums left the
    // output 2.6e-5 of rms(x) from the float64 restatement there, 100 times what they leave at 2048
    double acc[kCancelSums];
#pragma unroll
    for (int q = 0; q < kCancelSums; ++q) acc[q] = 0.0;
    for (int u = t; u < w.len; u += 256) {
        const float2 x = yw[u];
        const float2 e = cancel_carrier((unsigned long long)(w.lo + u), inc);
        const float zr = x.x * e.x + x.y * e.y, zi = x.y * e.x - x.x * e.y;      // x conj(e)
        float ra, rb, rc;
        cancel_taps(rep, w.r0, u, cs, ra, rb, rc);
        const double a = ra, b = rb, c = rc;
        acc[0] += a * zr; acc[1] += a * zi;
        acc[2] += b * zr; acc[3] += b * zi;
        acc[4] += c * zr; acc[5] += c * zi;
        acc[6] += a * a; acc[7] += b * b; acc[8] += c * c;
        acc[9] += a * b; acc[10] += b * c; acc[11] += a * c;
        acc[12] += (double)x.x * x.x + (double)x.y * x.y;
    }
#pragma unroll
    for (int q = 0; q < kCancelSums; ++q) acc[q] = row_sum_f64_dpp(acc[q]);
    if ((t & 15) == 0) {
#pragma unroll
        for (int q = 0; q < kCancelSums; ++q) red[t >> 4][q] = acc[q];
    }
    __syncthreads();
    if (t == 0) {
        double s[kCancelSums];
#pragma unroll
        for (int q = 0; q < kCancelSums; ++q) {
            double v = red[0][q];
            for (int r = 1; r < 16; ++r) v += red[r][q];
            s[q] = v;
        }
        // G = [[s6, s9, s11], [s9, s7, s10], [s11, s10, s8]] = L D L^T, no permutation
        const double thr = kCancelPivotMin * (s[6] + s[7] + s[8]);
        const double d0 = s[6];
        bool ok = d0 > 0.0 && d0 >= thr;
        double l10 = 0.0, l20 = 0.0, l21 = 0.0, d1 = 0.0, d2 = 0.0;
        if (ok) {
            l10 = s[9] / d0; l20 = s[11] / d0;
            d1 = s[7] - l10 * s[9];
            ok = d1 > 0.0 && d1 >= thr;
        }
        if (ok) {
            l21 = (s[10] - l20 * s[9]) / d1;
            d2 = s[8] - l20 * s[11] - l21 * l21 * d1;
            ok = d2 >= thr;
        }
        CancelRes r;
        r.c[0] = r.c[1] = r.c[2] = make_float2(0.f, 0.f);
        r.e_in = r.e_rem = 0.0; r.done = 0; r.pad = 0;
        if (ok) {
            double cr[3], ci[3];
#pragma unroll
            for (int part = 0; part < 2; ++part) {            // real and imaginary right-hand sides
                const double p0 = s[part], p1 = s[2 + part], p2 = s[4 + part];
                const double z0 = p0, z1 = p1 - l10 * z0, z2 = p2 - l20 * z0 - l21 * z1;
                const double x2 = z2 / d2, x1 = z1 / d1 - l21 * x2, x0 = z0 / d0 - l10 * x1 - l20 * x2;
                double* o = part ? ci : cr;
                o[0] = x0; o[1] = x1; o[2] = x2;
            }
            const double G[3][3] = {{s[6], s[9], s[11]}, {s[9], s[7], s[10]}, {s[11], s[10], s[8]}};
            double q = 0.0;
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int k = 0; k < 3; ++k) q += G[i][k] * (cr[i] * cr[k] + ci[i] * ci[k]);
#pragma unroll
            for (int i = 0; i < 3; ++i) r.c[i] = make_float2((float)cr[i], (float)ci[i]);
            r.e_in = s[12]; r.e_rem = q; r.done = 1;
        }
        res[blockIdx.x] = r;
        s_c[0] = r.c[0]; s_c[1] = r.c[1]; s_c[2] = r.c[2];
        s_done = r.done;
    }
    __syncthreads();
    if (!s_done) return;                          // (the window passes through bit for bit)
    const float2 c0 = s_c[0], c1 = s_c[1], c2 = s_c[2];
    for (int u = t; u < w.len; u += 256) {
        const float2 x = yw[u];
        const float2 e = cancel_carrier((unsigned long long)(w.lo + u), inc);
        float a, b, c;
        cancel_taps(rep, w.r0, u, cs, a, b, c);
        const float vr = c0.x * a + c1.x * b + c2.x * c, vi = c0.y * a + c1.y * b + c2.y * c;
        yw[u] = make_float2(x.x - (vr * e.x - vi * e.y), x.y - (vr * e.y + vi * e.x));
    }
}

// ---- the plan: everything a call derives from its arguments, on the host, no GPU --------------
struct CancelPlan {
    int cs = 0, min_window = 0, max_windows = 0;
    std::vector<int> first;                       // [nsat + 1]: where a satellite's windows start in `wins`
    std::vector<CancelWin> wins;
    std::vector<unsigned long long> inc;          // [nsat]
};

// Validates the arguments of gpsmi_acq_cancel (the handle and the buffers aside) and fills the plan
// (pl may be null).  The records and the common cfg fields are checked by the window rule
// (gpsmi_windows.h); the windows themselves are cancellation's own: they tile iq without a gap, so
// their edges are ceil(e_k), the first and the last are cut at iq's ends, and the replica is laid
// from the rounded start j_k.
inline int cancel_plan(int cs, size_t n, const gpsmi_cancel_sat* sats, int nsat, const gpsmi_cancel_cfg* c,
                       CancelPlan* pl) {
    WinCall w{"gpsmi_acq_cancel"};
    return win_guarded(w.fn, [&]() -> int {
        GPSMI_REQUIRE_IN(w.fn, nsat >= 0 && nsat <= kCancelMaxSats, "nsat out of range 0..32");
        GPSMI_REQUIRE_IN(w.fn, sats || nsat == 0, "null argument");
        GPSMI_REQUIRE_IN(w.fn, n >= 1 && n <= ((size_t)1 << 40), "n out of range 1..2^40");
        int rc, min_window = 16;
        if (c) {
            if ((rc = win_cfg(w, c->carrier_hz, c->f_offset_hz))) return rc;
            GPSMI_REQUIRE_IN(w.fn, c->min_window >= 0, "min_window must be >= 1 (0: 16)");
            if (c->min_window > 0) min_window = c->min_window;
        }
        if ((rc = win_code(w, cs))) return rc;
        CancelPlan tmp;
        CancelPlan& p = pl ? *pl : tmp;
        p.cs = cs; p.min_window = min_window; p.max_windows = 0;
        p.first.assign(1, 0);
        p.wins.clear();
        p.inc.clear();
        for (int s = 0; s < nsat; ++s) {
            const gpsmi_cancel_sat& g = sats[s];
            bool twice = false;
            for (int q = 0; q < s; ++q) twice |= sats[q].prn == g.prn;
            double Tc;
            unsigned long long inc;
            if ((rc = win_record(w, g.prn, twice ? "a PRN appears twice" : nullptr, g.f_hz, g.tau, &Tc, &inc)))
                return rc;
            p.inc.push_back(inc);
            // the window that holds sample 0: ceil(edge k) <= 0 < ceil(edge k + 1)
            long long k = (long long)std::floor(-g.tau / Tc);
            while (std::ceil(win_edge(g.tau, Tc, k)) > 0.0) --k;
            while (std::ceil(win_edge(g.tau, Tc, k + 1)) <= 0.0) ++k;
            for (;; ++k) {
                const double e0 = win_edge(g.tau, Tc, k);
                long long lo = (long long)std::ceil(e0), hi = (long long)std::ceil(win_edge(g.tau, Tc, k + 1));
                if (lo >= (long long)n) break;
                const long long j = (long long)std::nearbyint(e0);
                lo = lo < 0 ? 0 : lo;
                hi = hi > (long long)n ? (long long)n : hi;
                long long r0 = (lo - j) % cs;
                if (r0 < 0) r0 += cs;
                p.wins.push_back(CancelWin{lo, (int)(hi - lo), (int)r0});
            }
            p.first.push_back((int)p.wins.size());
            p.max_windows = std::max(p.max_windows, p.first[s + 1] - p.first[s]);
        }
        return GPSMI_OK;
    });
}

}  // namespace gpsmi
