// Bit-synchronous tracking of refined hits (gpsmi_acq_track, include/gpsmi.h; numpy
// restatement: tests/wtrk_ref.py).  The kernel and its host-side plan; the entry points sit beside
// the acquisition handle in gpsmi_acq.hip.
//
//   wtrk_kernel   one persistent workgroup per channel, four waves.  The replica is staged in LDS
//                 once; the workgroup then loops over the bits of the call.  Within a bit wave w
//                 takes milliseconds w, w + 4, ...: every sample of a millisecond's span is loaded,
//                 decoded and rotated once (integer carrier phase) and multiplied into the twelve
//                 whole-sample sums (early / prompt / late x replica shift 0 / 1 x re / im); wave
//                 shuffles, lane 0 to LDS.  Thread 0 then runs the float64 update in written-out
//                 order, writes the bit's record and lays the next bit's windows, phase increment
//                 and phase into LDS.  No workgroup reads another channel's data; no atomics.
#pragma once
#include <cmath>

#include "gpsmi_refine.h"

namespace gpsmi {

constexpr int kWtrkMaxHits = 64;
constexpr int kWtrkMaxBits = 1 << 20;
constexpr int kWtrkMs = 20;                       // milliseconds per data bit
constexpr int kWtrkSums = 12;                     // [tap 3][shift 2][re, im]
constexpr double kWtrkT = 0.020;                  // s per loop update
constexpr double kWtrkLockAlpha = 0.05;
constexpr double kWtrkDefPll = 4.0, kWtrkDefFll = 1.0, kWtrkDefDll = 0.5;
constexpr int kWtrkDefPullIn = 10;

struct WtrkPar {                                  // a call as the kernel sees it
    double first, n;                              // stream index of iq[0] and the sample count (exact: < 2^53)
    double carrier, f_off, fs, cs_d;
    double k_p1, k_p2, k_f, k_d;                  // w_p^2 T, 1.414 w_p, w_f T, 4 B_d T
    double cmt;                                   // cs / 1023 - tap
    int cs, tap, n_bits, pull_in;
};

struct WtrkBitPlan {                              // what thread 0 lays out for the next bit (LDS)
    long long nloc[kWtrkMs];                      // n_k - first_sample
    double a[kWtrkMs];
    unsigned long long inc, theta;
    double Tc;
    int go, pad;
};

inline size_t wtrk_lds_bytes(int cs) {
    return (size_t)cs * sizeof(float) + sizeof(WtrkBitPlan) + sizeof(gpsmi_wtrk_state) +
           kWtrkMs * kWtrkSums * sizeof(float);
}

// ---- the float64 steps: one operation per rounding, as gpsmi.h writes them ----------------------
#pragma clang fp contract(off)

// f / fs mod 1 in 0.64 fixed point (ref_phase_inc's value)
__device__ inline unsigned long long wtrk_inc(double f, double fs) {
    double x = f / fs;
    x -= floor(x);
    if (!(x < 1.0)) x = 0.0;
    return (unsigned long long)(x * 0x1p64);
}

// The windows of the bit that starts at (tau, f): false when one leaves [first, first + n) (or the
// state is not finite), and then nothing is written.
__device__ inline bool wtrk_windows(const WtrkPar& p, double tau, double f, WtrkBitPlan* pl) {
    const double Tc = p.cs_d / (1.0 + (f - p.f_off) / p.carrier);
    const double f0 = floor(tau + 0.0 * Tc), f19 = floor(tau + 19.0 * Tc);
    const double tap = (double)p.tap, end = p.first + p.n, len = p.cs_d + tap;
    if (!(f0 - tap >= p.first) || !(f19 - tap >= p.first) || !(f0 + len <= end) || !(f19 + len <= end))
        return false;
    for (int k = 0; k < kWtrkMs; ++k) {
        const double s = tau + (double)k * Tc, fl = floor(s);
        pl->a[k] = s - fl;
        pl->nloc[k] = (long long)(fl - p.first);
    }
    pl->Tc = Tc;
    return true;
}

// One bit: the blend, the discriminators, the record and the loop filters.  D: [20][12] whole-sample sums.
__device__ inline void wtrk_update(const WtrkPar& p, const WtrkBitPlan* pl, const float* D,
                                   gpsmi_wtrk_state& st, gpsmi_wtrk_bit* out) {
    const double two_pi = 6.283185307179586;
    double z[3][2] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};        // E, H1 (second half of P), L
    double h0[2] = {0.0, 0.0}, w = 0.0;
    for (int k = 0; k < kWtrkMs; ++k) {
        const double a = pl->a[k], a1 = 1.0 - a;
        const float* d = D + k * kWtrkSums;
        for (int tp = 0; tp < 3; ++tp) {
            const double re = a * (double)d[tp * 4 + 2] + a1 * (double)d[tp * 4 + 0];
            const double im = a * (double)d[tp * 4 + 3] + a1 * (double)d[tp * 4 + 1];
            if (tp == 1) {
                w += re * re + im * im;
                if (k < kWtrkMs / 2) { h0[0] += re; h0[1] += im; continue; }
            }
            z[tp][0] += re; z[tp][1] += im;
        }
    }
    const double h1r = z[1][0], h1i = z[1][1];
    const double pr = h0[0] + h1r, pi = h0[1] + h1i;
    const double ae = sqrt(z[0][0] * z[0][0] + z[0][1] * z[0][1]);
    const double al = sqrt(z[2][0] * z[2][0] + z[2][1] * z[2][1]);
    const double pp = pr * pr + pi * pi;
    const double e_f = atan2(h0[0] * h1i - h0[1] * h1r, h0[0] * h1r + h0[1] * h1i) / (two_pi * 0.010);
    const double e_p = pr == 0.0 ? (pi > 0.0 ? 0.25 : (pi < 0.0 ? -0.25 : 0.0)) : atan(pi / pr) / two_pi;
    const double e_d = ae + al > 0.0 ? p.cmt * (al - ae) / (ae + al) : 0.0;
    const int b = st.bit_no;
    st.mu_ring[b % GPSMI_WTRK_RING] = (float)(w > 0.0 ? pp / w : 0.0);
    const int cnt = b + 1 < GPSMI_WTRK_RING ? b + 1 : GPSMI_WTRK_RING;
    double mu = 0.0;
    for (int i = 0; i < cnt; ++i) mu += (double)st.mu_ring[i];
    mu /= (double)cnt;
    st.lock += kWtrkLockAlpha * ((pp > 0.0 ? (pr * pr - pi * pi) / pp : 0.0) - st.lock);
    gpsmi_wtrk_bit r;
    r.p_i = (float)pr; r.p_q = (float)pi; r.abs_e = (float)ae; r.abs_l = (float)al;
    r.h0_i = (float)h0[0]; r.h0_q = (float)h0[1]; r.h1_i = (float)h1r; r.h1_q = (float)h1i;
    r.f_hz = st.f_hz; r.tau = st.tau;
    r.cn0_dbhz = mu > 1.0 ? (float)(10.0 * log10(1000.0 * (mu - 1.0) / (20.0 - mu))) : __builtin_nanf("");
    r.lock = (float)st.lock; r.dll_err = (float)e_d; r.bit_no = b;
    *out = r;
    const double ep = (p.k_p2 > 0.0 && b >= p.pull_in) ? e_p : 0.0;
    const double ef = p.k_f > 0.0 ? e_f : 0.0;
    st.f_acc += p.k_p1 * ep + p.k_f * ef;
    st.f_hz = st.f_acc + p.k_p2 * ep;
    const double tau1 = (st.tau + 20.0 * pl->Tc) + p.k_d * e_d;
    const long long dn = (long long)(floor(tau1) - floor(st.tau));
    st.theta += (unsigned long long)dn * pl->inc;
    st.tau = tau1;
    st.bit_no = b + 1;
}
#pragma clang fp contract(fast)

// states[ch] in and out; bits[ch][n_bits] (zeroed by the host).  LDS: the replica [cs], the bit
// plan, the channel's state, the sums [20][12].  The host has checked that every state's first bit starts inside iq;
// wtrk_windows checks every bit's windows before a sample of it is read.
template <int FMT>
__global__ __launch_bounds__(256) void wtrk_kernel(
    const void* __restrict__ iq, const float* __restrict__ rep_time, const WtrkPar par,
    gpsmi_wtrk_state* __restrict__ states, gpsmi_wtrk_bit* __restrict__ bits) {
    extern __shared__ __attribute__((aligned(16))) float wtrk_lds[];
    float* rep = wtrk_lds;
    WtrkBitPlan* pl = reinterpret_cast<WtrkBitPlan*>(wtrk_lds + par.cs);
    gpsmi_wtrk_state& st = *reinterpret_cast<gpsmi_wtrk_state*>(pl + 1);     // thread 0's alone
    float* red = reinterpret_cast<float*>(&st + 1);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, ch = blockIdx.x;
    const int cs = par.cs, tap = par.tap, span = cs + 2 * tap;
    if (t == 0) {
        st = states[ch];
        st.flags &= ~GPSMI_WTRK_DATA_END;
        pl->go = wtrk_windows(par, st.tau, st.f_hz, pl) ? 1 : 0;
        pl->inc = wtrk_inc(st.f_hz, par.fs);
        pl->theta = st.theta;
        if (!pl->go) st.flags |= GPSMI_WTRK_DATA_END;
    }
    const float* R = rep_time + (size_t)states[ch].prn * cs;
    for (int i = t; i < cs; i += 256) rep[i] = R[i];
    __syncthreads();
    gpsmi_wtrk_bit* out = bits + (size_t)ch * par.n_bits;
    for (int b = 0; b < par.n_bits; ++b) {
        if (!pl->go) break;                              // (the same LDS word for every thread)
        const unsigned long long inc = pl->inc, theta = pl->theta;
        const long long n0 = pl->nloc[0];
        for (int k = wave; k < kWtrkMs; k += 4) {
            const long long j0 = pl->nloc[k] - tap;      // first sample of the early window
            float acc[kWtrkSums];
#pragma unroll
            for (int c = 0; c < kWtrkSums; ++c) acc[c] = 0.f;
            // sample u of the span is replica point u of the early window, u - tap of the prompt
            // window and u - 2 tap of the late one; shift 1 takes the replica point before it
            for (int u = lane; u < span; u += 64) {
                const long long j = j0 + u;
                const float2 x = load_iq<FMT>(iq, (size_t)j);
                const unsigned long long ph = theta + (unsigned long long)(j - n0) * inc;
                const float a = (float)((long long)ph >> 40) * 0x1p-23f;          // [-1, 1), exact
                float sn, co;
                sincospif(a, &sn, &co);
                const float yr = x.x * co + x.y * sn, yi = x.y * co - x.x * sn;
#pragma unroll
                for (int tp = 0; tp < 3; ++tp) {
                    const int i = u - tp * tap;
                    if (i >= 0 && i < cs) {
                        const float r0 = rep[i], r1 = rep[i == 0 ? cs - 1 : i - 1];
                        acc[tp * 4 + 0] += yr * r0; acc[tp * 4 + 1] += yi * r0;
                        acc[tp * 4 + 2] += yr * r1; acc[tp * 4 + 3] += yi * r1;
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < kWtrkSums; ++c) acc[c] = ref_wave_sum(acc[c]);
            if (lane == 0) {
#pragma unroll
                for (int c = 0; c < kWtrkSums; ++c) red[k * kWtrkSums + c] = acc[c];
            }
        }
        __syncthreads();
        if (t == 0) {
            wtrk_update(par, pl, red, st, out + b);
            if (b + 1 < par.n_bits) {
                pl->go = wtrk_windows(par, st.tau, st.f_hz, pl) ? 1 : 0;
                pl->inc = wtrk_inc(st.f_hz, par.fs);
                pl->theta = st.theta;
                if (!pl->go) st.flags |= GPSMI_WTRK_DATA_END;
            }
        }
        __syncthreads();
    }
    if (t == 0) states[ch] = st;
}

// ---- the plan: the argument checks and the gains, on the host, no GPU ---------------------------
inline int wtrk_default_tap(int cs) { return cs == 2048 ? 1 : 8; }

// Validates the arguments of gpsmi_acq_track (the handle aside) and fills the kernel's parameters.
inline int wtrk_plan(int cs, size_t n, const gpsmi_wtrk_state* st, int nhits, const gpsmi_wtrk_cfg* c,
                     WtrkPar* par) {
    static const char* const fn = "gpsmi_acq_track";
    GPSMI_REQUIRE_IN(fn, st && c, "null argument");
    GPSMI_REQUIRE_IN(fn, nhits >= 1 && nhits <= kWtrkMaxHits, "nhits out of range 1..64");
    GPSMI_REQUIRE_IN(fn, c->n_bits >= 1 && c->n_bits <= kWtrkMaxBits, "n_bits out of range 1..2^20");
    GPSMI_REQUIRE_IN(fn, std::isfinite(c->carrier_hz) && c->carrier_hz > 0.0, "carrier_hz must be positive");
    GPSMI_REQUIRE_IN(fn, std::isfinite(c->f_offset_hz), "f_offset_hz must be finite");
    GPSMI_REQUIRE_IN(fn, std::isfinite(c->pll_bw_hz) && std::isfinite(c->fll_bw_hz),
                     "pll_bw_hz / fll_bw_hz must be finite");
    GPSMI_REQUIRE_IN(fn, std::isfinite(c->dll_bw_hz) && c->dll_bw_hz >= 0.0, "dll_bw_hz must be >= 0 (0: the default)");
    GPSMI_REQUIRE_IN(fn, c->tap_samples >= 0, "tap_samples must be >= 1 (0: the default)");
    GPSMI_REQUIRE_IN(fn, n >= 1 && n < (size_t(1) << 52), "n out of range");
    GPSMI_REQUIRE_IN(fn, c->first_sample > -(int64_t(1) << 52) && c->first_sample < (int64_t(1) << 52),
                 "first_sample out of range");
    if (cs != 2048 && cs != 16368)
        return fail(GPSMI_E_UNSUPPORTED, "gpsmi_acq_track: code_samples 2048 and 16368 only (%d)", cs);
    const int tap = c->tap_samples > 0 ? c->tap_samples : wtrk_default_tap(cs);
    GPSMI_REQUIRE_IN(fn, (double)tap < (double)cs / 1023.0, "tap_samples must stay below one chip");
    const double fs = 1000.0 * cs;
    for (int i = 0; i < nhits; ++i) {
        const gpsmi_wtrk_state& s = st[i];
        GPSMI_REQUIRE_IN(fn, s.prn >= 1 && s.prn <= GPSMI_MAX_PRN, "prn out of range 1..37");
        GPSMI_REQUIRE_IN(fn, s.bit_no >= 0, "bit_no must be >= 0");
        GPSMI_REQUIRE_IN(fn, std::isfinite(s.f_hz) && std::fabs(s.f_hz) < 0.5 * fs, "f_hz out of range");
        GPSMI_REQUIRE_IN(fn, std::isfinite(s.f_acc), "f_acc must be finite");
        GPSMI_REQUIRE_IN(fn, std::isfinite(s.tau) && std::fabs(s.tau) < 0x1p52, "tau out of range");
        GPSMI_REQUIRE_IN(fn, std::floor(s.tau) - (double)tap >= (double)c->first_sample,
                     "a state's next bit starts before first_sample");
    }
    if (!par) return GPSMI_OK;
    const double pll = c->pll_bw_hz == 0.0 ? kWtrkDefPll : c->pll_bw_hz;
    const double fll = c->fll_bw_hz == 0.0 ? kWtrkDefFll : c->fll_bw_hz;
    const double dll = c->dll_bw_hz == 0.0 ? kWtrkDefDll : c->dll_bw_hz;
    const double wp = pll > 0.0 ? pll / 0.53 : 0.0, wf = fll > 0.0 ? fll / 0.25 : 0.0;
    par->first = (double)c->first_sample; par->n = (double)n;
    par->carrier = c->carrier_hz; par->f_off = c->f_offset_hz; par->fs = fs; par->cs_d = (double)cs;
    par->k_p1 = wp * wp * kWtrkT; par->k_p2 = 1.414 * wp; par->k_f = wf * kWtrkT;
    par->k_d = 4.0 * dll * kWtrkT;
    par->cmt = (double)cs / 1023.0 - (double)tap;
    par->cs = cs; par->tap = tap; par->n_bits = c->n_bits;
    par->pull_in = c->pull_in_bits == 0 ? kWtrkDefPullIn : (c->pull_in_bits < 0 ? 0 : c->pull_in_bits);
    return GPSMI_OK;
}

// gpsmi_wtrk_open of gpsmi.h
inline int wtrk_open(const gpsmi_refine_out* r, int cs, int rtap, int64_t start, double carrier, double f_off,
                     gpsmi_wtrk_state* st) {
    if (!r || !st) return fail(GPSMI_E_ARG, "gpsmi_wtrk_open: null argument");
    if (cs != 2048 && cs != 16368)
        return fail(GPSMI_E_UNSUPPORTED, "gpsmi_wtrk_open: code_samples 2048 and 16368 only (%d)", cs);
    if (!std::isfinite(carrier) || !(carrier > 0.0) || !std::isfinite(f_off))
        return fail(GPSMI_E_ARG, "gpsmi_wtrk_open: carrier_hz must be positive, f_offset_hz finite");
    if (rtap < 0 || rtap > cs / 4) return fail(GPSMI_E_ARG, "gpsmi_wtrk_open: refine_tap_samples out of range");
    if (r->prn < 1 || r->prn > GPSMI_MAX_PRN || r->edge_ms < 0 || r->edge_ms >= kWtrkMs)
        return fail(GPSMI_E_ARG, "gpsmi_wtrk_open: not a record of gpsmi_acq_refine");
    if (!std::isfinite(r->f_hz) || !std::isfinite(r->code_phase) || r->code_phase < 0.0 ||
        r->tap_metric[0] > r->tap_metric[1] || r->tap_metric[2] > r->tap_metric[1])
        return fail(GPSMI_E_ARG, "gpsmi_wtrk_open: the record has no code phase");
    const int tap = rtap > 0 ? rtap : wtrk_default_tap(cs);
    const double E = r->tap_metric[0], P = r->tap_metric[1], L = r->tap_metric[2], den = E - 2.0 * P + L;
    const double v = den != 0.0 ? 0.5 * (E - L) / den * (double)tap : 0.0;
    const double delay = std::nearbyint(r->code_phase - v);
    gpsmi_wtrk_state s = {};
    s.prn = r->prn;
    const double Tc = (double)cs / (1.0 + (r->f_hz - f_off) / carrier);
    s.tau = (double)start + r->code_phase + (double)(r->edge_ms + (delay < (double)tap ? 1 : 0)) * Tc;
    s.f_hz = s.f_acc = r->f_hz;
    *st = s;
    return GPSMI_OK;
}

}  // namespace gpsmi
