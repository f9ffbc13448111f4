// The window rule of the stages that work on refined records (prn, f_hz, tau) -- cancellation
// (gpsmi_cancel.h), signatures (gpsmi_sig.h), profiles (gpsmi_profile.h) --, described in DESIGN.md
// 4.2j: the code periods' edges e_k = tau + k Tc, their rounded starts j_k = rint(e_k), the windows
// with `guard` samples of iq on either side.  One wrong rounding here moves every window by a sample,
// so the rule, the checks of a record and the tables made from it are written once.  Host only and
// free of HIP: tests/host/windows_check.cpp builds it with the host compiler alone.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <new>
#include <vector>

#include "../../include/gpsmi.h"

namespace gpsmi {

int fail(int code, const char* fmt, ...);         // gpsmi_core.hip (a host test brings its own)

// A refused argument of the entry point `fn`: GPSMI_E_ARG, "<fn>: <msg>".
#define GPSMI_REQUIRE_IN(fn, cond, msg)                                          \
    do {                                                                         \
        if (!(cond)) return ::gpsmi::fail(GPSMI_E_ARG, "%s: %s", fn, msg);       \
    } while (0)

// body() with the one out-of-memory path of a plan: nothing is thrown across the C ABI
template <typename F>
inline int win_guarded(const char* fn, F&& body) {
    try {
        return body();
    } catch (const std::bad_alloc&) {
        return fail(GPSMI_E_NOMEM, "%s: out of host memory", fn);
    }
}

// f / rate mod 1 in 0.64 fixed point (two's complement), as the front end's mixer increment
inline unsigned long long ref_phase_inc(double f, double rate) {
    double x = f / rate;
    x -= std::floor(x);
    long double scaled = std::ldexp((long double)x, 64);
    if (scaled >= std::ldexp((long double)1.0, 64)) scaled = 0.0L;
    return (unsigned long long)scaled;
}

struct WinRec {                                   // one record as the kernels see it
    unsigned long long inc;                       // f_hz / fs in 0.64 fixed point
    int prn, count;                               // its windows (signatures) or runs (profiles)
};

struct WinCall {                                  // what the stages share of a call's arguments
    const char* fn;                               // the entry point, for the refusals
    int cs = 0;
    double fs = 0.0, carrier = 1575.42e6, f_offset = 0.0;
};

// the two fields every stage's cfg has
inline int win_cfg(WinCall& w, double carrier_hz, double f_offset_hz) {
    GPSMI_REQUIRE_IN(w.fn, std::isfinite(carrier_hz) && carrier_hz >= 0.0, "carrier_hz must be positive (0: L1)");
    GPSMI_REQUIRE_IN(w.fn, std::isfinite(f_offset_hz), "f_offset_hz must be finite");
    if (carrier_hz > 0.0) w.carrier = carrier_hz;
    w.f_offset = f_offset_hz;
    return GPSMI_OK;
}

inline int win_code(WinCall& w, int cs) {
    if (cs != 2048 && cs != 16368)
        return fail(GPSMI_E_UNSUPPORTED, "%s: code_samples 2048 and 16368 only (%d)", w.fn, cs);
    w.cs = cs;
    w.fs = 1000.0 * cs;
    return GPSMI_OK;
}

// One record -> its code period Tc in samples and its carrier's phase increment.  `own`: what the
// stage itself objects to in the record (null: nothing), refused where the stages have always
// refused it, behind the PRN.
inline int win_record(const WinCall& w, int prn, const char* own, double f_hz, double tau, double* Tc,
                      unsigned long long* inc) {
    GPSMI_REQUIRE_IN(w.fn, prn >= 1 && prn <= GPSMI_MAX_PRN, "prn out of range 1..37");
    GPSMI_REQUIRE_IN(w.fn, !own, own);
    GPSMI_REQUIRE_IN(w.fn, std::isfinite(f_hz) && std::fabs(f_hz) < 0.5 * w.fs, "f_hz out of range");
    GPSMI_REQUIRE_IN(w.fn, std::isfinite(tau) && std::fabs(tau) < 1e15, "tau out of range");
    const double scale = 1.0 + (f_hz - w.f_offset) / w.carrier;
    GPSMI_REQUIRE_IN(w.fn, scale > 0.99 && scale < 1.01, "f_hz - f_offset_hz beyond 1 % of carrier_hz");
    *Tc = (double)w.cs / scale;
    *inc = ref_phase_inc(f_hz, w.fs);
    return GPSMI_OK;
}

#pragma clang fp contract(off)
// edge k of a record's code periods, float64, unfused: tau + k Tc
inline double win_edge(double tau, double Tc, long long k) { return tau + (double)k * Tc; }
#pragma clang fp contract(fast)

// the first k with guard <= j_k = rint(tau + k Tc)
inline long long win_first(double tau, double Tc, int guard) {
    long long k = (long long)std::floor(((double)guard - tau) / Tc);
    while (std::nearbyint(win_edge(tau, Tc, k)) >= (double)guard) --k;
    while (std::nearbyint(win_edge(tau, Tc, k)) < (double)guard) ++k;
    return k;
}

// the starts j_k of a record's windows, guard <= j_k and j_k + cs + guard <= n, appended to `out` in
// order: from window `skip` on, `cap` of them at the most (0: every one that fits)
inline void win_starts(double tau, double Tc, int cs, size_t n, int guard, int skip, long long cap,
                       std::vector<long long>& out) {
    for (long long k = win_first(tau, Tc, guard) + skip;; ++k) {
        const long long j = (long long)std::nearbyint(win_edge(tau, Tc, k));
        if ((unsigned long long)(j + cs + guard) > (unsigned long long)n) break;
        if (cap > 0 && (long long)out.size() >= cap) break;
        out.push_back(j);
    }
}

struct WinTable {                                 // the tables of a call, as they go to the device
    std::vector<WinRec> recs;                     // [nsat]
    std::vector<long long> start;                 // [nsat][width], 0 behind a record's last window
};

// t.start from the records' own lists: the first recs[rec].count * per starts of every record, width =
// the largest count * per.  -> the largest count.
inline int win_pad(const std::vector<std::vector<long long>>& wins, int per, WinTable& t) {
    int most = 0;
    for (const WinRec& r : t.recs) most = std::max(most, r.count);
    const size_t width = (size_t)most * per;
    t.start.assign(t.recs.size() * width, 0ll);
    for (size_t s = 0; s < t.recs.size(); ++s)
        std::copy(wins[s].begin(), wins[s].begin() + (size_t)t.recs[s].count * per, t.start.begin() + s * width);
    return most;
}

}  // namespace gpsmi
