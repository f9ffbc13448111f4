// Multi-tap correlation profiles of refined records on one antenna (gpsmi_acq_profile, include/gpsmi.h;
// DESIGN.md 4.2r; numpy restatement: tests/profile_ref.py).  Kernels and their host-side plan; the entry
// points sit beside the signature's in gpsmi_acq.hip.
//
//   prof_sum_kernel  one workgroup per (record, run of coh_ms windows), wave v takes the windows v, v + 4,
//                    ... of the run.  A window goes by in chunks of kProfChunk samples: the wave wipes the
//                    chunk and Lh samples on either side ONCE (carrier at the absolute index, so a wiped
//                    sample is one value for all taps) into its own part of LDS, then every lane takes
//                    four consecutive replica points per step -- one 16-byte read of the replica -- and
//                    feeds all 2 LH + 1 tap sums from 2 LH + 4 wiped samples.  LDS is laid out in four
//                    planes by the sample index mod 4, so that the lanes of one read are 8 bytes apart.
//                    2 (2 LH + 1) float32 sums per lane, a butterfly over the wave per window, the windows
//                    of the run through LDS and added in ascending order by one thread per tap and
//                    component.  LH = 8 or 32 is compiled in: the smallest that holds the call's Lh (a
//                    tap's sum is the same instructions in the same order in either).
//   prof_cov_kernel  one workgroup per record: thread t takes the pairs t, t + 256, ... of the upper
//                    triangle and adds S_l conj(S_l') over the runs in ascending order in float64; it
//                    stores the entry and its conjugate.  No atomics; every sum has one order.
#pragma once
#include <cmath>
#include <vector>

#include "gpsmi_common.h"
#include "gpsmi_cancel.h"
#include "gpsmi_refine.h"
#include "gpsmi_windows.h"

namespace gpsmi {

constexpr int kProfMaxSats = 64;
constexpr int kProfMaxHalf = 32;                  // Lh
constexpr int kProfMaxCoh = 20;                   // windows of a run
constexpr int kProfChunk = 1024;                  // samples of a window wiped at a time: 4 steps of 256

// the wiped samples of one wave: kProfChunk + 2 LH of them in four planes (index mod 4), one item of
// padding per plane so that the planes start in different banks
template <int LH>
struct ProfLds {
    static constexpr int kItems = kProfChunk + 2 * LH;            // a multiple of 4
    static constexpr int kPlane = kItems / 4 + 1;
    static constexpr int kTaps = 2 * LH + 1;
    float2 w[4][4 * kPlane];                                      // [wave][plane][position]
    float d[kProfMaxCoh][kTaps][2];                               // the windows of the run
};

// S[rec][l][run].  start[rec][run coh + q] = j_k of window q of the run (the host has checked
// j_k - Lh >= 0 and j_k + Lh + cs <= n); S is [nsat][2 Lh + 1][max_runs], zeroed by the caller.
template <int FMT, int LH>
__global__ __launch_bounds__(256) void prof_sum_kernel(
    const void* __restrict__ iq, const float* __restrict__ rep_time, const WinRec* __restrict__ recs,
    const long long* __restrict__ start, int cs, int Lh, int coh, int max_runs, float2* __restrict__ S) {
    using L = ProfLds<LH>;
    __shared__ __attribute__((aligned(16))) L lds;
    constexpr int KT = L::kTaps;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int rec = blockIdx.y, run = blockIdx.x;
    const WinRec rr = recs[rec];
    if (run >= rr.count) return;                 // (the whole workgroup: nothing of it is waited for)
    const float* R = rep_time + (size_t)rr.prn * cs;
    const long long* st = start + ((size_t)rec * max_runs + run) * coh;
    float2* wv = lds.w[wave];
    for (int q0 = 0; q0 < coh; q0 += 4) {         // (every wave makes every trip: the barriers are uniform)
        const int q = q0 + wave;
        const bool live = q < coh;
        const long long j0 = live ? st[q] : 0;
        float ar[KT], ai[KT];
#pragma unroll
        for (int l = 0; l < KT; ++l) ar[l] = ai[l] = 0.f;
        for (int c0 = 0; c0 < cs; c0 += kProfChunk) {
            const int len = cs - c0 < kProfChunk ? cs - c0 : kProfChunk;
            if (live) {
                // item s holds w[j0 + c0 + s - LH]; outside the Lh samples on either side: 0, nothing read
                for (int s = lane; s < L::kItems; s += 64) {
                    const int u = c0 + s - LH;                    // from the window's first sample
                    float2 w = make_float2(0.f, 0.f);
                    if (u >= c0 - Lh && u < c0 + len + Lh) {
                        const size_t j = (size_t)(j0 + u);
                        const float2 e = cancel_carrier((unsigned long long)j, rr.inc);
                        const float2 x = load_iq<FMT>(iq, j);
                        w.x = __fmaf_rn(x.x, e.x, x.y * e.y);
                        w.y = __fmaf_rn(x.y, e.x, -(x.x * e.y));
                    }
                    wv[(s & 3) * L::kPlane + (s >> 2)] = w;
                }
            }
            __syncthreads();
            if (live) {
#pragma unroll 1
                for (int v = 4 * lane; v < len; v += 256) {       // (len is a multiple of 4)
                    const float4 r4 = *reinterpret_cast<const float4*>(R + c0 + v);
                    const float rb[4] = {r4.x, r4.y, r4.z, r4.w};
                    const float2* p = wv + (v >> 2);
#pragma unroll
                    for (int m = 0; m < KT + 3; ++m) {            // wiped sample v + m - LH of the chunk
                        // (LH = 32: at most 8 reads ahead of their use, or the 68 of them spill 130 sums:
                        // 193 VGPRs and two waves per SIMD with this hint, 256 + 72 AGPRs and one wave without;
                        // a hint only -- tests/test_profile.py holds the registers the build reports)
                        if (LH > 8 && m % 8 == 0) __asm__ volatile("" ::: "memory");
                        const float2 w = p[(m & 3) * L::kPlane + (m >> 2)];
#pragma unroll
                        for (int b = 0; b < 4; ++b) {             // ... meets point v + b at tap m - b
                            const int l = m - b;
                            if (l >= 0 && l < KT) {
                                ar[l] = __fmaf_rn(w.x, rb[b], ar[l]);
                                ai[l] = __fmaf_rn(w.y, rb[b], ai[l]);
                            }
                        }
                    }
                }
            }
            __syncthreads();
        }
        if (live) {
#pragma unroll
            for (int l = 0; l < KT; ++l) {
                const float sr = ref_wave_sum(ar[l]), si = ref_wave_sum(ai[l]);
                if (lane == 0) { lds.d[q][l][0] = sr; lds.d[q][l][1] = si; }
            }
        }
    }
    __syncthreads();
    const int K = 2 * Lh + 1;
    if (t < 2 * K) {
        const int l = t >> 1, c = t & 1, lt = l - Lh + LH;
        float s = lds.d[0][lt][c];
        for (int q = 1; q < coh; ++q) s += lds.d[q][lt][c];
        reinterpret_cast<float*>(S + ((size_t)rec * K + l) * max_runs + run)[c] = s;
    }
}

// Q[rec][l][l'] = sum_m S[rec][l][m] conj(S[rec][l'][m]), float64 [nsat][K][K][2]
__global__ __launch_bounds__(256) void prof_cov_kernel(const float2* __restrict__ S, const WinRec* __restrict__ recs,
                                                       int K, int max_runs, double* __restrict__ cov) {
    const int rec = blockIdx.x, n_runs = recs[rec].count;
    const float2* Sr = S + (size_t)rec * K * max_runs;
    double* c = cov + (size_t)rec * K * K * 2;
    for (int p = threadIdx.x; p < K * (K + 1) / 2; p += 256) {
        int a = 0, q = p;                          // pair p of the upper triangle, row by row
        while (q >= K - a) { q -= K - a; ++a; }
        const int b = a + q;
        const float2 *Sa = Sr + (size_t)a * max_runs, *Sb = Sr + (size_t)b * max_runs;
        double sr = 0.0, si = 0.0;
        for (int m = 0; m < n_runs; ++m) {
            const float2 x = Sa[m], y = Sb[m];
            const double xr = x.x, xi = x.y, yr = y.x, yi = y.y;
            sr += xr * yr + xi * yi;
            si += xi * yr - xr * yi;
        }
        if (a == b) {
            c[((size_t)a * K + a) * 2] = sr;
            c[((size_t)a * K + a) * 2 + 1] = 0.0;
        } else {
            c[((size_t)a * K + b) * 2] = sr;
            c[((size_t)a * K + b) * 2 + 1] = si;
            c[((size_t)b * K + a) * 2] = sr;
            c[((size_t)b * K + a) * 2 + 1] = -si;
        }
    }
}

// ---- the plan: everything a call derives from its arguments, on the host, no GPU --------------
struct ProfPlan : WinTable {                      // recs[].count: a record's runs; start [nsat][max_runs][coh]
    int cs = 0, Lh = 0, coh = 0, max_runs = 0;
};

// Validates the arguments of gpsmi_acq_profile (the handle and the buffers aside) and fills the plan
// (pl may be null).  The windows are the window rule's (gpsmi_windows.h) with half_taps samples of
// guard, skip_ms of them dropped; what is the profiles' own is the run: coh_ms windows in a row, the
// windows behind the last whole run left out.
inline int prof_plan(int cs, size_t n, const gpsmi_prof_sat* sats, int nsat, const gpsmi_prof_cfg* c, ProfPlan* pl) {
    WinCall w{"gpsmi_acq_profile"};
    return win_guarded(w.fn, [&]() -> int {
        GPSMI_REQUIRE_IN(w.fn, nsat >= 1 && nsat <= kProfMaxSats, "nsat out of range 1..64");
        GPSMI_REQUIRE_IN(w.fn, sats, "null argument");
        int rc, Lh = 0, coh = kProfMaxCoh, want_runs = 0;
        if (c) {
            GPSMI_REQUIRE_IN(w.fn, c->half_taps >= 0 && c->half_taps <= kProfMaxHalf,
                             "half_taps out of range 1..32 (0: the default)");
            GPSMI_REQUIRE_IN(w.fn, c->coh_ms >= 0 && c->coh_ms <= kProfMaxCoh, "coh_ms out of range 1..20 (0: 20)");
            GPSMI_REQUIRE_IN(w.fn, c->n_runs >= 0, "n_runs must be >= 1 (0: every run that fits)");
            GPSMI_REQUIRE_IN(w.fn, c->reserved == 0, "a reserved field is not 0");
            if ((rc = win_cfg(w, c->carrier_hz, c->f_offset_hz))) return rc;
            Lh = c->half_taps;
            if (c->coh_ms > 0) coh = c->coh_ms;
            want_runs = c->n_runs;
        }
        GPSMI_REQUIRE_IN(w.fn, n >= 1 && n <= ((size_t)1 << 40), "n out of range 1..2^40");
        if ((rc = win_code(w, cs))) return rc;
        if (Lh == 0) Lh = cs == 2048 ? 8 : 32;    // +- 4 chips, +- 2 chips
        ProfPlan tmp;
        ProfPlan& p = pl ? *pl : tmp;
        p.cs = cs; p.Lh = Lh; p.coh = coh;
        p.recs.assign(nsat, WinRec{0ull, 0, 0});
        std::vector<std::vector<long long>> wins(nsat);
        for (int s = 0; s < nsat; ++s) {
            const gpsmi_prof_sat& g = sats[s];
            const bool skip_ok = g.skip_ms >= 0 && g.skip_ms < kProfMaxCoh;
            double Tc;
            if ((rc = win_record(w, g.prn, skip_ok ? nullptr : "skip_ms out of range 0..19", g.f_hz, g.tau, &Tc,
                                 &p.recs[s].inc)))
                return rc;
            win_starts(g.tau, Tc, cs, n, Lh, g.skip_ms, (long long)want_runs * coh, wins[s]);
            const int runs = (int)(wins[s].size() / (size_t)coh);
            GPSMI_REQUIRE_IN(w.fn, runs >= 1, "a record has no run inside iq");
            p.recs[s].prn = g.prn;
            p.recs[s].count = runs;
        }
        p.max_runs = win_pad(wins, coh, p);
        return GPSMI_OK;
    });
}

}  // namespace gpsmi
