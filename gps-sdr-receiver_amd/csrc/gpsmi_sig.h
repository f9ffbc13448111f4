// Spatial signatures of refined records over several coherent antennas (gpsmi_acq_signature,
// include/gpsmi.h; numpy restatement: tests/sig_ref.py).  Kernels and their host-side
// plan; the entry points sit beside the acquisition handle in gpsmi_acq.hip.
//
//   sig_prompt_kernel  one workgroup per (record, run of kSigWinPerWg consecutive windows): the replica
//                      staged in LDS once; per sample the carrier (integer phase) is made once,
//                      multiplied into the replica point and applied to the sample of every antenna;
//                      2 A float32 sums per lane; wave shuffles, then the four waves in order through
//                      LDS.  Antenna a's sum is the same instructions in the same order whatever A is:
//                      the antennas are a bounded loop of eight with the ones past A switched off.
//   sig_cov_kernel     one workgroup per record: thread t takes the windows t, t + 256, ... in order
//                      and adds P_a conj(P_b) in float64 for one pair of the upper triangle after the
//                      other; wave shuffles, the four waves in order, and the entry and its conjugate
//                      stored by one thread.  No atomics; every sum has one order.
#pragma once
#include <cmath>
#include <vector>

#include "gpsmi_common.h"
#include "gpsmi_cancel.h"
#include "gpsmi_refine.h"
#include "gpsmi_windows.h"

namespace gpsmi {

constexpr int kSigMaxAnt = 8;
constexpr int kSigMaxSats = 64;
constexpr int kSigWinPerWg = 8;
constexpr int kSigPairs = kSigMaxAnt * (kSigMaxAnt + 1) / 2;

// LDS of sig_prompt_kernel: the replica [cs], then the waves' partial sums [kSigWinPerWg][4][2 kSigMaxAnt]
inline size_t sig_lds_bytes(int cs) {
    return ((size_t)cs + (size_t)kSigWinPerWg * 4 * 2 * kSigMaxAnt) * sizeof(float);
}

// P[rec][a][k], a < A.  iq: A rows of n samples; start[rec][k] = j_k, the first sample of window k (the
// host has checked 0 <= j_k and j_k + cs <= n); P is [nsat][A][max_w], zero where a record has no window.
template <int FMT>
__global__ __launch_bounds__(256) void sig_prompt_kernel(
    const void* __restrict__ iq, size_t n, int A, const float* __restrict__ rep_time,
    const WinRec* __restrict__ recs, const long long* __restrict__ start, int cs, int max_w,
    float2* __restrict__ P) {
    extern __shared__ __attribute__((aligned(16))) float sig_lds[];
    float* rep = sig_lds;
    float* red = sig_lds + cs;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int rec = blockIdx.y, k0 = blockIdx.x * kSigWinPerWg;
    const WinRec rr = recs[rec];
    if (k0 >= rr.count) return;                   // (the whole workgroup: nothing of it is waited for)
    const float* R = rep_time + (size_t)rr.prn * cs;
    for (int i = t; i < cs; i += 256) rep[i] = R[i];
    __syncthreads();
    const int nk = rr.count - k0 < kSigWinPerWg ? rr.count - k0 : kSigWinPerWg;
    for (int q = 0; q < nk; ++q) {
        const long long j0 = start[(size_t)rec * max_w + k0 + q];
        float acc[2 * kSigMaxAnt];
#pragma unroll
        for (int c = 0; c < 2 * kSigMaxAnt; ++c) acc[c] = 0.f;
        for (int u = t; u < cs; u += 256) {
            const size_t j = (size_t)(j0 + u);
            const float2 e = cancel_carrier((unsigned long long)j, rr.inc);
            const float r = rep[u];
            const float wr = e.x * r, wi = e.y * r;               // R[u] exp(+j phase); x conj(.) below
#pragma unroll
            for (int a = 0; a < kSigMaxAnt; ++a) {
                if (a < A) {
                    const float2 x = load_iq<FMT>(iq, (size_t)a * n + j);
                    acc[2 * a] = __fmaf_rn(x.x, wr, __fmaf_rn(x.y, wi, acc[2 * a]));
                    acc[2 * a + 1] = __fmaf_rn(x.y, wr, __fmaf_rn(-x.x, wi, acc[2 * a + 1]));
                }
            }
        }
#pragma unroll
        for (int a = 0; a < kSigMaxAnt; ++a) {
            if (a < A) {
                const float sr = ref_wave_sum(acc[2 * a]), si = ref_wave_sum(acc[2 * a + 1]);
                if (lane == 0) {
                    red[(q * 4 + wave) * 2 * kSigMaxAnt + 2 * a] = sr;
                    red[(q * 4 + wave) * 2 * kSigMaxAnt + 2 * a + 1] = si;
                }
            }
        }
    }
    __syncthreads();
    if (t < nk * 2 * kSigMaxAnt) {
        const int q = t / (2 * kSigMaxAnt), c = t % (2 * kSigMaxAnt), a = c >> 1;
        if (a < A) {
            float s = red[(q * 4 + 0) * 2 * kSigMaxAnt + c];
            s += red[(q * 4 + 1) * 2 * kSigMaxAnt + c];
            s += red[(q * 4 + 2) * 2 * kSigMaxAnt + c];
            s += red[(q * 4 + 3) * 2 * kSigMaxAnt + c];
            float* o = reinterpret_cast<float*>(P + ((size_t)rec * A + a) * max_w + k0 + q);
            o[c & 1] = s;
        }
    }
}

__device__ __forceinline__ double sig_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// C[rec][a][b] = sum_k P[rec][a][k] conj(P[rec][b][k]), float64 [nsat][A][A][2]
__global__ __launch_bounds__(256) void sig_cov_kernel(const float2* __restrict__ P, const WinRec* __restrict__ recs,
                                                      int A, int max_w, double* __restrict__ cov) {
    __shared__ double red[4][2 * kSigPairs];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, rec = blockIdx.x;
    const int n_win = recs[rec].count;
    const float2* Pr = P + (size_t)rec * A * max_w;
    int p = 0;
    for (int a = 0; a < A; ++a) {
        for (int b = a; b < A; ++b, ++p) {
            const float2 *Pa = Pr + (size_t)a * max_w, *Pb = Pr + (size_t)b * max_w;
            double sr = 0.0, si = 0.0;
            for (int k = t; k < n_win; k += 256) {
                const float2 x = Pa[k], y = Pb[k];
                const double xr = x.x, xi = x.y, yr = y.x, yi = y.y;
                sr += xr * yr + xi * yi;
                si += xi * yr - xr * yi;
            }
            sr = sig_wave_sum(sr);
            si = sig_wave_sum(si);
            if (lane == 0) { red[wave][2 * p] = sr; red[wave][2 * p + 1] = si; }
        }
    }
    __syncthreads();
    if (t < p) {
        int a = 0, q = t;                          // pair t of the upper triangle, row by row
        while (q >= A - a) { q -= A - a; ++a; }
        const int b = a + q;
        const double sr = ((red[0][2 * t] + red[1][2 * t]) + red[2][2 * t]) + red[3][2 * t];
        const double si = ((red[0][2 * t + 1] + red[1][2 * t + 1]) + red[2][2 * t + 1]) + red[3][2 * t + 1];
        double* c = cov + (size_t)rec * A * A * 2;
        if (a == b) {
            c[((size_t)a * A + a) * 2] = sr;
            c[((size_t)a * A + a) * 2 + 1] = 0.0;
        } else {
            c[((size_t)a * A + b) * 2] = sr;
            c[((size_t)a * A + b) * 2 + 1] = si;
            c[((size_t)b * A + a) * 2] = sr;
            c[((size_t)b * A + a) * 2 + 1] = -si;
        }
    }
}

// ---- the plan: everything a call derives from its arguments, on the host, no GPU --------------
struct SigPlan : WinTable {                       // recs[].count: a record's windows; start [nsat][max_windows]
    int cs = 0, A = 0, max_windows = 0;
};

// Validates the arguments of gpsmi_acq_signature (the handle and the buffers aside) and fills the plan
// (pl may be null).  The windows are the window rule's (gpsmi_windows.h) with no guard: whole periods
// at their rounded starts, n_ms of them at the most.
inline int sig_plan(int cs, size_t n, const gpsmi_sig_sat* sats, int nsat, const gpsmi_sig_cfg* c, SigPlan* pl) {
    WinCall w{"gpsmi_acq_signature"};
    return win_guarded(w.fn, [&]() -> int {
        GPSMI_REQUIRE_IN(w.fn, nsat >= 1 && nsat <= kSigMaxSats, "nsat out of range 1..64");
        GPSMI_REQUIRE_IN(w.fn, sats, "null argument");
        int rc, A = 2, n_ms = 0;
        if (c) {
            GPSMI_REQUIRE_IN(w.fn, c->antennas == 0 || (c->antennas >= 2 && c->antennas <= kSigMaxAnt),
                             "antennas out of range 2..8 (0: 2)");
            GPSMI_REQUIRE_IN(w.fn, c->n_ms >= 0, "n_ms must be >= 1 (0: every window that fits)");
            if ((rc = win_cfg(w, c->carrier_hz, c->f_offset_hz))) return rc;
            if (c->antennas > 0) A = c->antennas;
            n_ms = c->n_ms;
        }
        GPSMI_REQUIRE_IN(w.fn, n >= 1 && n <= ((size_t)1 << 40) / (size_t)A, "n out of range 1..2^40 / antennas");
        if ((rc = win_code(w, cs))) return rc;
        SigPlan tmp;
        SigPlan& p = pl ? *pl : tmp;
        p.cs = cs; p.A = A;
        p.recs.assign(nsat, WinRec{0ull, 0, 0});
        std::vector<std::vector<long long>> wins(nsat);
        for (int s = 0; s < nsat; ++s) {
            const gpsmi_sig_sat& g = sats[s];
            double Tc;
            if ((rc = win_record(w, g.prn, g.reserved != 0 ? "a reserved field is not 0" : nullptr, g.f_hz, g.tau, &Tc,
                                 &p.recs[s].inc)))
                return rc;
            win_starts(g.tau, Tc, cs, n, 0, 0, n_ms, wins[s]);
            GPSMI_REQUIRE_IN(w.fn, !wins[s].empty(), "a record has no window inside iq");
            p.recs[s].prn = g.prn;
            p.recs[s].count = (int)wins[s].size();
        }
        p.max_windows = win_pad(wins, 1, p);
        return GPSMI_OK;
    });
}

}  // namespace gpsmi
