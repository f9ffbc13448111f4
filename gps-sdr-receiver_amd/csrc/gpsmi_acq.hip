// Acquisition: batched per-SV x Doppler parallel code-phase search on gfx950: the handle and the
// entry points.  The kernels live beside it, one header per feature:
//
//   gpsmi_acq_search.h    the coherent, the non-coherent and the deep search (gpsmi_acq_search*,
//                         DESIGN.md 4.2, 4.2a, 4.2e): one wipe-off fold per code length, one
//                         correlation kernel in three modes
//   gpsmi_longcorr.h      the correlations of the other code lengths (gpsmi_pfa.h, gpsmi_bigfft.h,
//                         gpsmi_direct.h), shared with the tracking handle
//   gpsmi_acq_array.h     the array search (gpsmi_acq_search_array*): the deep search
//                         over 2 .. 4 antennas, their complex correlations combined per lag
//   gpsmi_refine.h        refinement of weak / deep hits (gpsmi_acq_refine): fine
//                         Doppler, bit edge, sub-sample code phase, C/N0
//   gpsmi_wtrk.h          bit-synchronous tracking of refined hits (gpsmi_acq_track)
//   gpsmi_cancel.h        cancellation of strong satellites ahead of the weak searches
//                         (gpsmi_acq_cancel): per-period projection, in place
//   gpsmi_collective.h    collective detection over the surfaces of a deep search
//                         (gpsmi_acq_collective)
//   gpsmi_peaks.h         the k largest peaks of every satellite over those surfaces, for the
//                         spoofing check (gpsmi_acq_peaks)
//   gpsmi_sig.h           spatial signatures of refined records over several antennas
//                         (gpsmi_acq_signature): prompts per antenna, their covariance
//   gpsmi_profile.h       multi-tap correlation profiles of refined records on one antenna
//                         (gpsmi_acq_profile): bit-coherent sums per tap, their covariance
//   gpsmi_windows.h       host only: the window rule, the record checks and the tables that
//                         cancellation, the signatures and the profiles share
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "gpsmi_common.h"
#include "gpsmi_devmem.h"
#include "gpsmi_longcorr.h"
#include "gpsmi_fft.h"
#include "gpsmi_stats.h"
#include "gpsmi_refine.h"
#include "gpsmi_wtrk.h"
#include "gpsmi_cancel.h"
#include "gpsmi_collective.h"
#include "gpsmi_peaks.h"
#include "gpsmi_sig.h"
#include "gpsmi_profile.h"
#include "gpsmi_acq_search.h"
#include "gpsmi_acq_array.h"

using namespace gpsmi;

struct gpsmi_acq;
namespace gpsmi { HandleSync trk_sync(gpsmi_trk* h); }

struct gpsmi_acq {
    gpsmi_cfg cfg;
    // device memory: every buffer is a DevBuf (gpsmi_devmem.h) with a capacity of its own, in elements
    DevBuf<float2> d_tw;
    DevBuf<float> d_t32;
    DevBuf<float2> d_rep;             // [GPSMI_MAX_PRN + 1][cs]
    bool have_rep[GPSMI_MAX_PRN + 1] = {};
    DevBuf<float2> d_iq;              // host input of any entry point, sized as complex64 (acq_input)
    DevBuf<float2> d_spec;            // [bins][2048]
    DevBuf<float> d_omega;            // [bins]
    DevBuf<int> d_slot;
    DevBuf<gpsmi_peak> d_peaks;       // [bins][nsv]
    DevBuf<float2> d_nbr;
    // page-locked staging of the per-call parameters (two sets: a search can be enqueued
    // while the previous one still runs; no blocking copy, no use of the null stream)
    float* h_om[2] = {nullptr, nullptr};
    int32_t* h_slot[2] = {nullptr, nullptr};
    bool staged_used[2] = {false, false};
    int stage = 0;
    // code_samples != 2048: the bins folded in the time domain, then the long-code correlation
    bool direct = false;
    DevBuf<float> d_rep_time;               // [GPSMI_MAX_PRN + 1][cs]
    bool have_time[GPSMI_MAX_PRN + 1] = {};
    DevBuf<float2> d_fold;                  // [bins][cs]
    LongCorr lc;                            // its method, replica spectra, cell tables and statistics
    // non-coherent search: the per-(bin, segment) spectra (CS = 2048) or folded samples (16368) of
    // one chunk of bins, sized per call (gpsmi_acq_search_nc)
    DevBuf<float2> d_nc;
    // deep search: the lag rotation of every (bin, segment) of a call (gpsmi_acq_search_deep)
    DevBuf<int> d_shift;
    // refinement (gpsmi_acq_refine): prompts [nhits][3][n_ms], grid [nhits][n_df][20], the per-call
    // tables (hits, window starts, df increments, df) in one block, the records
    DevBuf<float2> d_rp;
    DevBuf<float> d_rm;
    DevBuf<char> d_rt;
    DevBuf<gpsmi_refine_out> d_ro;          // [kRefMaxHits]
    // bit-synchronous tracking (gpsmi_acq_track): the states of a call, its bit records
    DevBuf<gpsmi_wtrk_state> d_ws;          // [kWtrkMaxHits]
    DevBuf<gpsmi_wtrk_bit> d_wb;
    // cancellation (gpsmi_acq_cancel): the complex64 output of a host call whose input is raw, the
    // window tables of a call, the windows' results [nsat][max_windows]
    DevBuf<float2> d_cx;
    DevBuf<CancelWin> d_cw;
    DevBuf<CancelRes> d_cr;
    // collective detection (gpsmi_acq_collective): the normalised rows and the pooled ones, the
    // satellites of a call, its cell map
    DevBuf<float> d_cz;
    DevBuf<gpsmi_collective_sat> d_csat;          // [kColMaxSats]
    DevBuf<gpsmi_collective_cell> d_cc;
    // auxiliary peaks (gpsmi_acq_peaks): the statistics [nsv][nbins], zmax and its bins [nsv][cs], the
    // picks [nsv][k] and their columns [nsv][k][2][nbins]
    DevBuf<float2> d_pst;
    DevBuf<float> d_pz;
    DevBuf<int> d_pb;
    DevBuf<gpsmi_peaks_pick> d_pk;
    DevBuf<float> d_pcol;
    // signatures and profiles (gpsmi_acq_signature, gpsmi_acq_profile; either call has left the stream
    // when it returns, so one set serves both): the sums -- prompts [nsat][A][max_windows] or tap sums
    // [nsat][K][max_runs] --, the records and the window starts of a call in one block, the covariances
    // [nsat][A][A][2] or [nsat][K][K][2]
    DevBuf<float2> d_vs;
    DevBuf<char> d_vt;
    DevBuf<double> d_vc;
    int iq_fmt = GPSMI_IQ_C64;              // what the iq pointers of the search calls point to
    // bytes of `n` samples in the handle's input format
    size_t iq_bytes(size_t n) const { return n * (iq_fmt == GPSMI_IQ_U8 ? 2 : sizeof(float2)); }
    float last_ms = 0.f;
    bool pending = false;
    // released bottom up: the events, then the stream, then (above) the device buffers
    DevStream stream;
    DevEvent ev0, ev1;
    DevEvent order;                         // orders other handles' streams behind this one
    DevEvent staged[2];
};

extern "C" int gpsmi_acq_wait(gpsmi_acq* h);

namespace gpsmi {
HandleSync acq_sync(gpsmi_acq* h) { return HandleSync{h->stream, h->order, h->cfg.device, nullptr}; }
}  // namespace gpsmi

// the buffers every search needs: per bin, per cell
static int acq_reserve(gpsmi_acq* h, int nbins, int nsv) {
    const size_t cells = (size_t)nbins * nsv;
    int rc = h->d_spec.reserve((size_t)nbins * kFftN, "gpsmi_acq spectra");
    if (!rc) rc = h->d_omega.reserve(nbins, "gpsmi_acq bin table");
    if (!rc) rc = h->d_peaks.reserve(cells, "gpsmi_acq peak table");
    if (!rc) rc = h->d_nbr.reserve(cells, "gpsmi_acq neighbour table");
    return rc;
}

// ---- one call on the handle: every entry point is its own checks and plan, then
// acq_enter, acq_input, its reserves (and acq_tables / acq_lds_optin where it has tables or a large
// LDS), acq_begin, its launches, acq_end, its read-backs, gpsmi_acq_wait ----------------------------

// behind the argument checks: a refused call leaves last_ms and the device alone
static int acq_enter(gpsmi_acq* h) {
    h->last_ms = 0.f;
    GPSMI_HIP(hipSetDevice(h->cfg.device));
    return GPSMI_OK;
}

// -> *d_iq, what the kernels read: the caller's device pointer, or d_iq with the `count` samples a host
// call reads, in the handle's input format, on their way up on the handle's stream (d_iq is sized for
// complex64; raw input fills a quarter)
static int acq_input(gpsmi_acq* h, const void* iq, bool on_host, size_t count, const void** d_iq) {
    *d_iq = iq;
    if (!on_host) return GPSMI_OK;
    const int rc = h->d_iq.reserve(count, "gpsmi_acq input block");
    if (rc) return rc;
    GPSMI_HIP(hipMemcpyAsync(h->d_iq.p, iq, h->iq_bytes(count), hipMemcpyHostToDevice, h->stream));
    *d_iq = h->d_iq.p;
    return GPSMI_OK;
}

// the refinement, tracking and cancellation kernels read GPSCacode itself; prn_of(i): the PRN of item i
template <typename PrnOf>
static int acq_need_time(const gpsmi_acq* h, const char* fn, int n, PrnOf&& prn_of) {
    for (int i = 0; i < n; ++i)
        if (!h->have_time[prn_of(i)])
            return fail(GPSMI_E_STATE, "%s: no time-domain replica set for PRN %d (gpsmi_acq_set_replica_time)", fn,
                        (int)prn_of(i));
    return GPSMI_OK;
}

// per-call tables from pageable host memory into reserved device memory: the copies, then the stream
// synchronised, since the tables may leave scope (or be rewritten by the caller) once this returns
struct HostTable { void* dst; const void* src; size_t bytes; };
static int acq_tables(gpsmi_acq* h, std::initializer_list<HostTable> tables) {
    for (const HostTable& t : tables)
        GPSMI_HIP(hipMemcpyAsync(t.dst, t.src, t.bytes, hipMemcpyHostToDevice, h->stream));
    GPSMI_HIP(hipStreamSynchronize(h->stream));
    return GPSMI_OK;
}

// more than 64 KiB of dynamic LDS for the kernel of the handle's input format
template <typename K>
static int acq_lds_optin(const gpsmi_acq* h, K* u8, K* c64, size_t lds) {
    if (lds > 64 * 1024)
        GPSMI_HIP(hipFuncSetAttribute((const void*)(h->iq_fmt == GPSMI_IQ_U8 ? u8 : c64),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return GPSMI_OK;
}

static int acq_begin(gpsmi_acq* h) {         // ahead of a call's first launch
    GPSMI_HIP(hipEventRecord(h->ev0, h->stream));
    return GPSMI_OK;
}

static int acq_end(gpsmi_acq* h) {           // behind its last one; gpsmi_acq_wait completes the call
    GPSMI_HIP(hipGetLastError());
    GPSMI_HIP(hipEventRecord(h->ev1, h->stream));
    h->pending = true;
    return GPSMI_OK;
}

// ---- the call of the two covariance stages on refined records, signatures and profiles ---------
struct CovCall {
    const char* fn;                         // the entry point
    const char* sums;                       // what its sums are called: "prompts", "sums"
    size_t n_in, n_sums, n_cov;             // samples read; complex64 sums and float64 values made
};

static void acq_counts(const WinTable& t, int32_t* counts) {
    if (counts)
        for (size_t s = 0; s < t.recs.size(); ++s) counts[s] = t.recs[s].count;
}

// One call of either stage behind its plan: the tables of the call go up in one block, the sums are
// zeroed, launch(d_iq, d_rec, d_start) -- acq_begin, the stage's kernels from d_vs into d_vc, acq_end --
// runs, and the covariances, the sums where asked for and the records' counts come back.
template <typename Launch>
static int acq_cov_call(gpsmi_acq* h, const void* iq, bool on_host, const CovCall& c, const WinTable& t, double* cov,
                        int32_t* counts, float* sums, Launch&& launch) {
    int rc;
    const void* d_iq;
    if ((rc = acq_need_time(h, c.fn, (int)t.recs.size(), [&](int i) { return t.recs[i].prn; })) ||
        (rc = acq_enter(h)) || (rc = acq_input(h, iq, on_host, c.n_in, &d_iq)))
        return rc;
    const char* part[3] = {"tables", c.sums, "covariances"};
    char what[3][64];                       // the buffers' names, for a refused allocation
    for (int i = 0; i < 3; ++i) snprintf(what[i], sizeof(what[i]), "%s %s", c.fn, part[i]);
    // the tables of the call, 8-byte items first
    const size_t b_start = t.start.size() * sizeof(long long), b_rec = t.recs.size() * sizeof(WinRec);
    if ((rc = h->d_vt.reserve(b_start + b_rec, what[0])) || (rc = h->d_vs.reserve(c.n_sums, what[1])) ||
        (rc = h->d_vc.reserve(c.n_cov, what[2])))
        return rc;
    long long* d_start = reinterpret_cast<long long*>(h->d_vt.p);
    WinRec* d_rec = reinterpret_cast<WinRec*>(h->d_vt.p + b_start);
    GPSMI_HIP(hipMemsetAsync(h->d_vs.p, 0, c.n_sums * sizeof(float2), h->stream));
    if ((rc = acq_tables(h, {{d_start, t.start.data(), b_start}, {d_rec, t.recs.data(), b_rec}})) ||
        (rc = launch(d_iq, d_rec, d_start)))
        return rc;
    GPSMI_HIP(hipMemcpyAsync(cov, h->d_vc.p, c.n_cov * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (sums)
        GPSMI_HIP(hipMemcpyAsync(sums, h->d_vs.p, c.n_sums * sizeof(float2), hipMemcpyDeviceToHost, h->stream));
    if ((rc = gpsmi_acq_wait(h))) return rc;
    acq_counts(t, counts);
    return GPSMI_OK;
}

static int acq_build(const gpsmi_cfg* cfg, gpsmi_acq* h) {
    h->direct = cfg->code_samples != kFftN;
    int rc = h->stream.create();
    // (order feeds hipStreamWaitEvent alone; ev0 / ev1 are stamps read behind gpsmi_acq_wait's stream
    // synchronisation, and the result table comes down by a copy command of its own)
    if (!rc) rc = h->order.create<Ev::AcqOrder, EventScope::DeviceOnly>();
    if (!rc) rc = h->ev0.create<Ev::AcqStamp, EventScope::DeviceOnly>();
    if (!rc) rc = h->ev1.create<Ev::AcqStamp, EventScope::DeviceOnly>();
    if (rc) return rc;
    std::vector<float2> tw;
    make_twiddles(tw);
    if ((rc = h->d_tw.upload(tw, "gpsmi_acq twiddles"))) return rc;
    // SEC_TIME (gpsrecv.py:32-33): float32(k+1) / SAMPLE_RATE in float32
    const int ngps = cfg->n_cyc * cfg->code_samples;
    const float fs = (float)(1000 * cfg->code_samples);
    std::vector<float> t32(ngps);
    for (int k = 0; k < ngps; ++k) t32[k] = (float)(k + 1) / fs;
    if ((rc = h->d_t32.upload(t32, "gpsmi_acq time base")) ||
        (rc = h->d_rep.reserve((size_t)(GPSMI_MAX_PRN + 1) * kFftN, "gpsmi_acq replica spectra")) ||
        (rc = h->d_slot.reserve(GPSMI_MAX_PRN + 1, "gpsmi_acq PRN table")))
        return rc;
    for (int k = 0; k < 2; ++k) {
        GPSMI_HIP(hipHostMalloc((void**)&h->h_om[k], 65536 * sizeof(float), hipHostMallocDefault));
        GPSMI_HIP(hipHostMalloc((void**)&h->h_slot[k], (GPSMI_MAX_PRN + 1) * sizeof(int32_t),
                                hipHostMallocDefault));
        // (acq_stage waits on it before the HOST rewrites h_om / h_slot, which the device only read)
        if ((rc = h->staged[k].create<Ev::AcqStaged, EventScope::DeviceOnly>())) return rc;
    }
    if (h->direct) {
        if ((rc = h->d_rep_time.reserve((size_t)(GPSMI_MAX_PRN + 1) * cfg->code_samples, "gpsmi_acq replicas")))
            return rc;
        return h->lc.build(cfg->code_samples, "gpsmi_acq");
    }
    return GPSMI_OK;
}

extern "C" {

int gpsmi_acq_create(const gpsmi_cfg* cfg, gpsmi_acq** out) {
    GPSMI_REQUIRE(cfg && out, "null argument");
    *out = nullptr;
    GPSMI_REQUIRE(cfg->code_samples >= 1024 && cfg->code_samples <= 65536 &&
                      cfg->code_samples % 16 == 0,
                  "code_samples must be a multiple of 16 in 1024..65536");
    GPSMI_REQUIRE(cfg->n_cyc >= 1 && cfg->n_cyc <= 64, "n_cyc out of range");
    GPSMI_HIP(hipSetDevice(cfg->device));
    gpsmi_acq* h = new (std::nothrow) gpsmi_acq();
    if (!h) return fail(GPSMI_E_NOMEM, "out of host memory");
    h->cfg = *cfg;
    const int rc = acq_build(cfg, h);
    if (rc) {                       // nothing half-built leaves this function
        (void)gpsmi_acq_destroy(h);
        return rc;
    }
    *out = h;
    return GPSMI_OK;
}

int gpsmi_acq_destroy(gpsmi_acq* h) {
    if (!h) return GPSMI_OK;
    (void)hipSetDevice(h->cfg.device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (int k = 0; k < 2; ++k) {
        if (h->h_om[k]) (void)hipHostFree(h->h_om[k]);
        if (h->h_slot[k]) (void)hipHostFree(h->h_slot[k]);
    }
    delete h;                                // (releases events, stream and device buffers, in this order)
    return GPSMI_OK;
}

int gpsmi_acq_set_replica_time(gpsmi_acq* h, int prn, const float* replica) {
    GPSMI_REQUIRE(h && replica, "null argument");
    GPSMI_REQUIRE(prn >= 1 && prn <= GPSMI_MAX_PRN, "prn out of range 1..37");
    GPSMI_HIP(hipSetDevice(h->cfg.device));
    int rc = GPSMI_OK;                       // (the FFT path has no use for it: kept for gpsmi_acq_refine)
    if (!h->direct && (rc = h->d_rep_time.reserve((size_t)(GPSMI_MAX_PRN + 1) * h->cfg.code_samples, "gpsmi_acq replicas")))
        return rc;
    GPSMI_HIP(hipMemcpy(h->d_rep_time.p + (size_t)prn * h->cfg.code_samples, replica,
                        (size_t)h->cfg.code_samples * sizeof(float), hipMemcpyHostToDevice));
    if (h->direct && (rc = h->lc.set_replica(h->stream, h->d_rep_time.p, prn, h->d_tw.p))) return rc;
    h->have_time[prn] = true;
    return GPSMI_OK;
}

int gpsmi_acq_set_replica(gpsmi_acq* h, int prn, const float* spectrum) {
    GPSMI_REQUIRE(h && spectrum, "null argument");
    GPSMI_REQUIRE(prn >= 1 && prn <= GPSMI_MAX_PRN, "prn out of range 1..37");
    if (h->direct) return fail(GPSMI_E_STATE, "code_samples != 2048: use gpsmi_acq_set_replica_time");
    GPSMI_HIP(hipSetDevice(h->cfg.device));
    GPSMI_HIP(hipMemcpy(h->d_rep.p + (size_t)prn * kFftN, spectrum, kFftN * sizeof(float2),
                        hipMemcpyHostToDevice));
    h->have_rep[prn] = true;
    return GPSMI_OK;
}

// parameter uploads: the caller's arrays are consumed before this function returns
// (copied into page-locked staging), the device copies are ordered on the stream
static int acq_stage(gpsmi_acq* h, const int32_t* prn, int nsv, const double* freqs, int nbins) {
    const int sg = h->stage ^= 1;
    if (h->staged_used[sg]) GPSMI_HIP(hipEventSynchronize(h->staged[sg]));
    for (int b = 0; b < nbins; ++b) h->h_om[sg][b] = (float)(2.0 * M_PI * freqs[b]);
    for (int i = 0; i < nsv; ++i) h->h_slot[sg][i] = prn[i];
    GPSMI_HIP(hipMemcpyAsync(h->d_omega.p, h->h_om[sg], nbins * sizeof(float), hipMemcpyHostToDevice,
                             h->stream));
    GPSMI_HIP(hipMemcpyAsync(h->d_slot.p, h->h_slot[sg], nsv * sizeof(int), hipMemcpyHostToDevice,
                             h->stream));
    GPSMI_HIP(hipEventRecord(h->staged[sg], h->stream));
    h->staged_used[sg] = true;
    return GPSMI_OK;
}

// the table of a search (and the neighbours) to where the caller wants it, behind the kernels
static int acq_copy_out(gpsmi_acq* h, int nbins, int nsv, gpsmi_peak* out, void* out_dev, float* nbr) {
    size_t bytes = (size_t)nbins * nsv * sizeof(gpsmi_peak);
    if (out_dev)
        GPSMI_HIP(hipMemcpyAsync(out_dev, h->d_peaks.p, bytes, hipMemcpyDeviceToDevice, h->stream));
    if (out)
        GPSMI_HIP(hipMemcpyAsync(out, h->d_peaks.p, bytes, hipMemcpyDeviceToHost, h->stream));
    if (nbr)
        GPSMI_HIP(hipMemcpyAsync(nbr, h->d_nbr.p, (size_t)nbins * nsv * sizeof(float2),
                                 hipMemcpyDeviceToHost, h->stream));
    return GPSMI_OK;
}

// Scratch of one chunk of bins of a segmented search: the spectra / folded samples of all its
// segments.  Longer searches take the bins in chunks; the magnitude sums stay in registers.
constexpr size_t kNcScratchMax = size_t(512) << 20;

// The deep search (gpsmi_acq_search_deep) is the non-coherent one plus a lag rotation per (bin,
// segment): what the rotation is computed from.
struct DeepShift { double carrier_hz, f_offset_hz; };

// m[b][s] mod cs of gpsmi.h, in 0 .. cs - 1: float64 in the order written there, ties to even
static int deep_shift(double f_hz, const DeepShift& d, int s, int n_coh, int cs) {
    const double m = std::nearbyint(-(f_hz - d.f_offset_hz) / d.carrier_hz * (double)s * (double)n_coh *
                                    (double)cs);
    const double r = std::fmod(m, (double)cs);           // exact: both are integers
    return (int)(r < 0.0 ? r + (double)cs : r);
}

// What tells the searches apart.  segmented = false: gpsmi_acq_search* (n_coh is its n_avg, n_seg 1,
// no rotation); true: gpsmi_acq_search_nc* and, with `deep`, gpsmi_acq_search_deep*.
struct AcqSearch {
    int n_coh, n_seg;
    const DeepShift* deep;
    bool wait;                               // false: the caller collects the table with gpsmi_acq_wait
    bool segmented;
    float* rows = nullptr;                   // deep only: where the surfaces go, [nsv][nbins][cs] on the device
};

// The arguments of every search entry point, before anything is uploaded or enqueued.  on_host: iq
// and out are the caller's host arrays (the host-input entry points have no out_dev).
static int acq_check_search(const gpsmi_acq* h, const void* iq, bool on_host, size_t n, const int32_t* prn,
                            int nsv, const double* freqs, int nbins, const AcqSearch& s,
                            const gpsmi_peak* out, const void* out_dev) {
    GPSMI_REQUIRE(h && iq && prn && freqs && (out || !on_host), "null argument");
    if (s.deep) {
        GPSMI_REQUIRE(std::isfinite(s.deep->carrier_hz) && s.deep->carrier_hz > 0.0, "carrier_hz must be positive");
        GPSMI_REQUIRE(std::isfinite(s.deep->f_offset_hz), "f_offset_hz must be finite");
    }
    GPSMI_REQUIRE(out || out_dev, "no output requested");
    GPSMI_REQUIRE(nsv >= 0 && nsv <= GPSMI_MAX_PRN, "nsv out of range");
    GPSMI_REQUIRE(nbins >= 0 && nbins <= 65535, "nbins out of range");
    const int cs = h->cfg.code_samples;
    if (!s.segmented) {
        GPSMI_REQUIRE(s.n_coh >= 1 && s.n_coh <= h->cfg.n_cyc, "n_avg out of range 1..n_cyc");
        GPSMI_REQUIRE(n >= (size_t)s.n_coh * cs, "iq shorter than n_avg code periods");
    } else {
        GPSMI_REQUIRE(s.n_coh >= 1 && s.n_coh <= h->cfg.n_cyc, "n_coh out of range 1..n_cyc");
        GPSMI_REQUIRE(s.n_seg >= 1 && s.n_seg <= 65535, "n_seg out of range 1..65535");
        GPSMI_REQUIRE(n / ((size_t)s.n_coh * cs) >= (size_t)s.n_seg, "iq shorter than n_seg * n_coh code periods");
    }
    for (int i = 0; i < nsv; ++i) {
        GPSMI_REQUIRE(prn[i] >= 1 && prn[i] <= GPSMI_MAX_PRN, "prn out of range 1..37");
        if (!(h->direct ? h->have_time[prn[i]] : h->have_rep[prn[i]]))
            return fail(GPSMI_E_STATE, "no replica set for PRN %d", (int)prn[i]);
    }
    if (s.segmented && h->direct && !h->lc.pfa())
        return fail(GPSMI_E_UNSUPPORTED, "%s: code_samples 2048 or the native 16368 "
                                         "correlation only (not the \"codephase\" time-domain paths)",
                    s.deep ? "gpsmi_acq_search_deep" : "gpsmi_acq_search_nc");
    if (s.deep) {
        for (int b = 0; b < nbins; ++b)
            GPSMI_REQUIRE(std::isfinite(freqs[b]), "freqs_hz must be finite");
        // a bin's rotated sums need all its segments in one launch: no chunking over segments
        if ((size_t)s.n_seg * cs * sizeof(float2) > kNcScratchMax)
            return fail(GPSMI_E_UNSUPPORTED, "gpsmi_acq_search_deep: the %d segments of one bin exceed the "
                                             "%zu MiB of scratch", s.n_seg, kNcScratchMax >> 20);
    }
    return GPSMI_OK;
}

// Code lengths other than 2048, bins b0 .. b0 + nb - 1: fold into x [bin][n_seg][cs], the cell tables,
// the correlation with its statistics into lc.d_stats.  The coherent search is b0 = 0, nb = nbins,
// n_seg = 1, and the only one with the time-domain correlations.
static void acq_direct_chunk(gpsmi_acq* h, const void* d_iq, const AcqSearch& s, float2* x, int b0, int nb,
                             int nsv, int nbins) {
    const int cs = h->cfg.code_samples, c0 = b0 * nsv, ncell = nb * nsv;
    LongCorr& lc = h->lc;
    with_fmt(h->iq_fmt, [&](auto fmt) {
        hipLaunchKernelGGL(acq_fold_kernel<decltype(fmt)::value>, dim3((cs + 255) / 256, nb, s.n_seg), dim3(256),
                           0, h->stream, d_iq, h->d_t32.p, h->d_omega.p + b0, s.n_coh, s.n_seg, cs, x);
    });
    hipLaunchKernelGGL(acq_cells_kernel, dim3((ncell + 255) / 256), dim3(256), 0, h->stream,
                       lc.d_xsel.p + c0, lc.d_rsel.p + c0, h->d_slot.p, nsv, ncell);
    if (!s.segmented) lc.correlate<0>(h->stream, x, c0, ncell, h->d_rep_time.p, h->d_tw.p);
    else if (!s.deep) lc.correlate<2>(h->stream, x, c0, ncell, h->d_rep_time.p, h->d_tw.p, s.n_seg);
    else if (!s.rows) lc.correlate<3>(h->stream, x, c0, ncell, h->d_rep_time.p, h->d_tw.p, s.n_seg,
                                      h->d_shift.p + (size_t)b0 * s.n_seg);
    else lc.correlate<4>(h->stream, x, c0, ncell, h->d_rep_time.p, h->d_tw.p, s.n_seg,
                         h->d_shift.p + (size_t)b0 * s.n_seg, PfaRows{s.rows, nsv, nbins, b0});
}

// Every search, on device-resident iq whose arguments acq_check_search has passed.
static int acq_search_run(gpsmi_acq* h, const void* d_iq, const int32_t* prn, int nsv, const double* freqs,
                          int nbins, AcqSearch s, gpsmi_peak* out, void* out_dev, float* nbr) {
    // one segment of the 16368 path: the coherent search itself (MODE 0 forms its statistics from the
    // unscaled squares; MODE 2's would differ in the last bits of std)
    if (h->lc.pfa() && s.segmented && s.n_seg == 1) {
        if (s.rows)
            return fail(GPSMI_E_UNSUPPORTED, "gpsmi_acq_search_deep_rows_dev: one segment at 16368 is the coherent "
                                             "search, which keeps no surface (n_seg >= 2)");
        s = AcqSearch{s.n_coh, 1, nullptr, s.wait, false};
    }
    int rc = acq_enter(h);
    if (rc || nsv == 0 || nbins == 0) return rc;            // empty search: nothing to do
    if ((rc = acq_reserve(h, nbins, nsv))) return rc;
    const int cs = h->cfg.code_samples, n_seg = s.n_seg;
    const size_t cells = (size_t)nbins * nsv;
    // where the folds go, and how many bins of them at a time: a coherent search is one chunk
    size_t nbc = (size_t)nbins;
    float2* x = nullptr;
    if (s.segmented) {
        nbc = kNcScratchMax / ((size_t)n_seg * cs * sizeof(float2));
        nbc = nbc < 1 ? 1 : nbc > (size_t)nbins ? (size_t)nbins : nbc;
        if ((rc = h->d_nc.reserve(nbc * n_seg * cs, "gpsmi_acq segment scratch"))) return rc;
        x = h->d_nc.p;
    } else if (h->direct) {
        if ((rc = h->d_fold.reserve((size_t)nbins * cs, "gpsmi_acq folded samples"))) return rc;
        x = h->d_fold.p;
    } else {
        x = h->d_spec.p;
    }
    if (h->direct && (rc = h->lc.reserve(cells))) return rc;
    rc = acq_stage(h, prn, nsv, freqs, nbins);
    if (rc) return rc;
    if (s.deep) {
        std::vector<int> shift;
        const size_t ns = (size_t)nbins * n_seg;
        try { shift.resize(ns); } catch (const std::bad_alloc&) {
            return fail(GPSMI_E_NOMEM, "gpsmi_acq_search_deep: out of host memory");
        }
        for (int b = 0; b < nbins; ++b)
            for (int sg = 0; sg < n_seg; ++sg)
                shift[(size_t)b * n_seg + sg] = deep_shift(freqs[b], *s.deep, sg, s.n_coh, cs);
        if ((rc = h->d_shift.reserve(ns, "gpsmi_acq lag rotations")) ||
            (rc = acq_tables(h, {{h->d_shift.p, shift.data(), ns * sizeof(int)}})))   // (it leaves scope here)
            return rc;
    }
    float2* d_nbr = nbr ? h->d_nbr.p : nullptr;
    if ((rc = acq_begin(h))) return rc;
    for (int b0 = 0; b0 < nbins; b0 += (int)nbc) {
        const int nb = nbins - b0 < (int)nbc ? nbins - b0 : (int)nbc;
        if (h->direct) {
            acq_direct_chunk(h, d_iq, s, x, b0, nb, nsv, nbins);
            continue;
        }
        // four groups of 256 threads for the long coherent integrations (acq_spectrum_kernel)
        with_value<4, 1>(s.n_coh >= 4 ? 4 : 1, [&](auto g) { with_fmt(h->iq_fmt, [&](auto fmt) {
            constexpr int G = decltype(g)::value;
            hipLaunchKernelGGL((acq_spectrum_kernel<G, decltype(fmt)::value>), dim3(nb, n_seg), dim3(256 * G), 0,
                               h->stream, d_iq, h->d_t32.p, h->d_omega.p + b0, s.n_coh, n_seg, x, h->d_tw.p);
        }); });
        with_value<0, 2, 3, 1>(!s.segmented ? 0 : !s.deep ? 1 : s.rows ? 3 : 2, [&](auto mode) {
            hipLaunchKernelGGL(acq_corr_kernel<decltype(mode)::value>, dim3(nsv, nb), dim3(256), 0, h->stream, x,
                               h->d_rep.p, h->d_slot.p, h->d_peaks.p, nsv, n_seg, b0, h->d_tw.p, d_nbr,
                               s.deep ? h->d_shift.p + (size_t)b0 * n_seg : nullptr, s.rows, nbins);
        });
    }
    if (h->direct)
        hipLaunchKernelGGL(acq_peaks_kernel, dim3(((int)cells + 255) / 256), dim3(256), 0, h->stream,
                           h->lc.d_stats.p, h->d_peaks.p, d_nbr, (int)cells);
    if ((rc = acq_end(h)) || (rc = acq_copy_out(h, nbins, nsv, out, out_dev, nbr)) || !s.wait) return rc;
    return gpsmi_acq_wait(h);
}

// An entry point: the checks, host input uploaded (as much of it as the search reads), the search.
static int acq_search(gpsmi_acq* h, const void* iq, bool on_host, size_t n, const int32_t* prn, int nsv,
                      const double* freqs, int nbins, const AcqSearch& s, gpsmi_peak* out, void* out_dev,
                      float* nbr) {
    int rc = acq_check_search(h, iq, on_host, n, prn, nsv, freqs, nbins, s, out, out_dev);
    if (rc) return rc;
    if (on_host) GPSMI_HIP(hipSetDevice(h->cfg.device));
    const void* d_iq;
    if ((rc = acq_input(h, iq, on_host, (size_t)s.n_seg * s.n_coh * h->cfg.code_samples, &d_iq))) return rc;
    return acq_search_run(h, d_iq, prn, nsv, freqs, nbins, s, out, out_dev, nbr);
}

int gpsmi_acq_wait(gpsmi_acq* h) {
    GPSMI_REQUIRE(h, "null handle");
    if (!h->pending) return GPSMI_OK;
    GPSMI_HIP(hipSetDevice(h->cfg.device));
    GPSMI_HIP(hipStreamSynchronize(h->stream));
    GPSMI_HIP(hipEventElapsedTime(&h->last_ms, h->ev0, h->ev1));
    h->pending = false;
    return GPSMI_OK;
}

int gpsmi_acq_search_dev_async(gpsmi_acq* h, const void* d_iq, size_t n, const int32_t* prn,
                               int nsv, const double* freqs, int nbins, int n_avg,
                               gpsmi_peak* out, void* out_dev) {
    return acq_search(h, d_iq, false, n, prn, nsv, freqs, nbins, {n_avg, 1, nullptr, false, false}, out, out_dev,
                      nullptr);
}

int gpsmi_acq_search_dev(gpsmi_acq* h, const void* d_iq, size_t n, const int32_t* prn, int nsv,
                         const double* freqs, int nbins, int n_avg, gpsmi_peak* out,
                         void* out_dev) {
    return acq_search(h, d_iq, false, n, prn, nsv, freqs, nbins, {n_avg, 1, nullptr, true, false}, out, out_dev,
                      nullptr);
}

int gpsmi_acq_search(gpsmi_acq* h, const float* iq, size_t n, const int32_t* prn, int nsv,
                     const double* freqs, int nbins, int n_avg, gpsmi_peak* out) {
    return gpsmi_acq_search_ex(h, iq, n, prn, nsv, freqs, nbins, n_avg, out, nullptr);
}

int gpsmi_acq_search_ex(gpsmi_acq* h, const float* iq, size_t n, const int32_t* prn, int nsv,
                        const double* freqs, int nbins, int n_avg, gpsmi_peak* out, float* nbr) {
    return acq_search(h, iq, true, n, prn, nsv, freqs, nbins, {n_avg, 1, nullptr, true, false}, out, nullptr, nbr);
}

int gpsmi_acq_search_nc_dev(gpsmi_acq* h, const void* d_iq, size_t n, const int32_t* prn, int nsv,
                            const double* freqs_hz, int nbins, int n_coh, int n_seg, gpsmi_peak* out,
                            void* out_dev) {
    return acq_search(h, d_iq, false, n, prn, nsv, freqs_hz, nbins, {n_coh, n_seg, nullptr, true, true}, out,
                      out_dev, nullptr);
}

int gpsmi_acq_search_nc(gpsmi_acq* h, const void* iq, size_t n, const int32_t* prn, int nsv,
                        const double* freqs_hz, int nbins, int n_coh, int n_seg, gpsmi_peak* out,
                        float* nbr) {
    return acq_search(h, iq, true, n, prn, nsv, freqs_hz, nbins, {n_coh, n_seg, nullptr, true, true}, out, nullptr,
                      nbr);
}

int gpsmi_acq_search_deep(gpsmi_acq* h, const void* iq, size_t n, const int32_t* prn, int nsv,
                          const double* freqs_hz, int nbins, int n_coh, int n_seg, double carrier_hz,
                          double f_offset_hz, gpsmi_peak* out, float* nbr) {
    const DeepShift d{carrier_hz, f_offset_hz};
    return acq_search(h, iq, true, n, prn, nsv, freqs_hz, nbins, {n_coh, n_seg, &d, true, true}, out, nullptr, nbr);
}

int gpsmi_acq_search_deep_dev(gpsmi_acq* h, const void* d_iq, size_t n, const int32_t* prn, int nsv,
                              const double* freqs_hz, int nbins, int n_coh, int n_seg, double carrier_hz,
                              double f_offset_hz, gpsmi_peak* out, void* out_dev) {
    const DeepShift d{carrier_hz, f_offset_hz};
    return acq_search(h, d_iq, false, n, prn, nsv, freqs_hz, nbins, {n_coh, n_seg, &d, true, true}, out, out_dev,
                      nullptr);
}

int gpsmi_acq_search_deep_rows_dev(gpsmi_acq* h, const void* d_iq, size_t n, const int32_t* prn, int nsv,
                                   const double* freqs_hz, int nbins, int n_coh, int n_seg, double carrier_hz,
                                   double f_offset_hz, gpsmi_peak* out, void* out_dev, void* d_rows) {
    GPSMI_REQUIRE(d_rows, "null d_rows");
    const DeepShift d{carrier_hz, f_offset_hz};
    return acq_search(h, d_iq, false, n, prn, nsv, freqs_hz, nbins,
                      {n_coh, n_seg, &d, true, true, static_cast<float*>(d_rows)}, out, out_dev, nullptr);
}

// ---- the array search (kernel: gpsmi_acq_array.h) ----------------------------------------------
// What gpsmi_acq_search_array_plan checks and sizes, without a handle: the scratch of one launch (the
// spectra of all segments and antennas of its bins) and how many bins a launch takes.
struct ArrayPlan { size_t count, scratch_bytes; int nbc; };

static int array_plan(int cs, size_t n, int antennas, int nbins, int n_coh, int n_seg, double carrier_hz,
                      double f_offset_hz, ArrayPlan* pl) {
    GPSMI_REQUIRE(cs >= 1024 && cs <= 65536 && cs % 16 == 0, "code_samples must be a multiple of 16 in 1024..65536");
    GPSMI_REQUIRE(antennas >= 2 && antennas <= 4, "antennas out of range 2..4");
    GPSMI_REQUIRE(n <= (size_t(1) << 40) / (size_t)antennas, "n * antennas beyond 2^40 samples");
    GPSMI_REQUIRE(nbins >= 0 && nbins <= 65535, "nbins out of range");
    GPSMI_REQUIRE(n_coh >= 1 && n_coh <= 64, "n_coh out of range");
    GPSMI_REQUIRE(n_seg >= 1 && n_seg <= 65535, "n_seg out of range 1..65535");
    GPSMI_REQUIRE(n / ((size_t)n_coh * cs) >= (size_t)n_seg, "rows shorter than n_seg * n_coh code periods");
    GPSMI_REQUIRE(std::isfinite(carrier_hz) && carrier_hz > 0.0, "carrier_hz must be positive");
    GPSMI_REQUIRE(std::isfinite(f_offset_hz), "f_offset_hz must be finite");
    if (cs != kFftN)
        return fail(GPSMI_E_UNSUPPORTED, "gpsmi_acq_search_array: code_samples 2048 only (not the native 16368 "
                                         "correlation, nor a time-domain path)");
    const size_t per_bin = (size_t)antennas * n_seg * cs * sizeof(float2);
    if (per_bin > kNcScratchMax)
        return fail(GPSMI_E_UNSUPPORTED, "gpsmi_acq_search_array: the %d segments of one bin over %d antennas "
                                         "exceed the %zu MiB of scratch", n_seg, antennas, kNcScratchMax >> 20);
    size_t nbc = kNcScratchMax / per_bin;
    nbc = nbc > (size_t)nbins ? (size_t)nbins : nbc;
    pl->count = (size_t)n_seg * n_coh * cs;
    pl->nbc = (int)nbc;
    pl->scratch_bytes = nbc * per_bin;
    return GPSMI_OK;
}

// iq: [antennas][n] in the handle's input format, host or device; rows: optional, on the device
static int acq_search_array(gpsmi_acq* h, const void* iq, bool on_host, size_t n, int antennas, const int32_t* prn,
                            int nsv, const double* freqs, int nbins, int n_coh, int n_seg, double carrier_hz,
                            double f_offset_hz, gpsmi_peak* out, void* out_dev, float* nbr, float* rows) {
    GPSMI_REQUIRE(h && iq && prn && freqs && (out || !on_host), "null argument");
    GPSMI_REQUIRE(out || out_dev, "no output requested");
    GPSMI_REQUIRE(nsv >= 0 && nsv <= GPSMI_MAX_PRN, "nsv out of range");
    ArrayPlan pl;
    int rc = array_plan(h->cfg.code_samples, n, antennas, nbins, n_coh, n_seg, carrier_hz, f_offset_hz, &pl);
    if (rc) return rc;
    GPSMI_REQUIRE(n_coh <= h->cfg.n_cyc, "n_coh out of range 1..n_cyc");
    for (int b = 0; b < nbins; ++b) GPSMI_REQUIRE(std::isfinite(freqs[b]), "freqs_hz must be finite");
    for (int i = 0; i < nsv; ++i) {
        GPSMI_REQUIRE(prn[i] >= 1 && prn[i] <= GPSMI_MAX_PRN, "prn out of range 1..37");
        if (!h->have_rep[prn[i]]) return fail(GPSMI_E_STATE, "no replica set for PRN %d", (int)prn[i]);
    }
    if ((rc = acq_enter(h)) || nsv == 0 || nbins == 0) return rc;            // empty search: nothing to do
    // host rows go up packed, only what the search reads of each: [antennas][count]
    const char* d_iq = static_cast<const char*>(iq);
    size_t stride = n;
    if (on_host) {
        if ((rc = h->d_iq.reserve((size_t)antennas * pl.count, "gpsmi_acq input block"))) return rc;
        for (int a = 0; a < antennas; ++a)
            GPSMI_HIP(hipMemcpyAsync(reinterpret_cast<char*>(h->d_iq.p) + a * h->iq_bytes(pl.count),
                                     d_iq + a * h->iq_bytes(n), h->iq_bytes(pl.count), hipMemcpyHostToDevice,
                                     h->stream));
        d_iq = reinterpret_cast<const char*>(h->d_iq.p);
        stride = pl.count;
    }
    const int cs = h->cfg.code_samples;
    const size_t ns = (size_t)nbins * n_seg;
    std::vector<int> shift;
    try { shift.resize(ns); } catch (const std::bad_alloc&) {
        return fail(GPSMI_E_NOMEM, "gpsmi_acq_search_array: out of host memory");
    }
    const DeepShift ds{carrier_hz, f_offset_hz};
    for (int b = 0; b < nbins; ++b)
        for (int sg = 0; sg < n_seg; ++sg) shift[(size_t)b * n_seg + sg] = deep_shift(freqs[b], ds, sg, n_coh, cs);
    if ((rc = acq_reserve(h, nbins, nsv)) ||
        (rc = h->d_nc.reserve(pl.scratch_bytes / sizeof(float2), "gpsmi_acq segment scratch")) ||
        (rc = acq_stage(h, prn, nsv, freqs, nbins)) || (rc = h->d_shift.reserve(ns, "gpsmi_acq lag rotations")) ||
        (rc = acq_tables(h, {{h->d_shift.p, shift.data(), ns * sizeof(int)}})) || (rc = acq_begin(h)))
        return rc;
    float2* d_nbr = nbr ? h->d_nbr.p : nullptr;
    for (int b0 = 0; b0 < nbins; b0 += pl.nbc) {
        const int nb = nbins - b0 < pl.nbc ? nbins - b0 : pl.nbc;
        for (int a = 0; a < antennas; ++a)       // the single-antenna search's spectra of row a
            with_value<4, 1>(n_coh >= 4 ? 4 : 1, [&](auto g) { with_fmt(h->iq_fmt, [&](auto fmt) {
                constexpr int G = decltype(g)::value;
                hipLaunchKernelGGL((acq_spectrum_kernel<G, decltype(fmt)::value>), dim3(nb, n_seg), dim3(256 * G), 0,
                                   h->stream, static_cast<const void*>(d_iq + a * h->iq_bytes(stride)), h->d_t32.p,
                                   h->d_omega.p + b0, n_coh, n_seg, h->d_nc.p + (size_t)a * nb * n_seg * cs,
                                   h->d_tw.p);
            }); });
        with_value<2, 3, 4>(antennas, [&](auto na) {
            hipLaunchKernelGGL(acq_corr_array_kernel<decltype(na)::value>, dim3(nsv, nb), dim3(256), 0, h->stream,
                               h->d_nc.p, h->d_rep.p, h->d_slot.p, h->d_peaks.p, nsv, n_seg, b0, nb, h->d_tw.p, d_nbr,
                               h->d_shift.p + (size_t)b0 * n_seg, rows, nbins);
        });
    }
    if ((rc = acq_end(h)) || (rc = acq_copy_out(h, nbins, nsv, out, out_dev, nbr))) return rc;
    return gpsmi_acq_wait(h);
}

int gpsmi_acq_search_array(gpsmi_acq* h, const void* iq, size_t n, int antennas, const int32_t* prn, int nsv,
                           const double* freqs_hz, int nbins, int n_coh, int n_seg, double carrier_hz,
                           double f_offset_hz, gpsmi_peak* out, float* nbr) {
    return acq_search_array(h, iq, true, n, antennas, prn, nsv, freqs_hz, nbins, n_coh, n_seg, carrier_hz,
                            f_offset_hz, out, nullptr, nbr, nullptr);
}

int gpsmi_acq_search_array_dev(gpsmi_acq* h, const void* d_iq, size_t n, int antennas, const int32_t* prn, int nsv,
                               const double* freqs_hz, int nbins, int n_coh, int n_seg, double carrier_hz,
                               double f_offset_hz, gpsmi_peak* out, void* out_dev, void* d_rows) {
    return acq_search_array(h, d_iq, false, n, antennas, prn, nsv, freqs_hz, nbins, n_coh, n_seg, carrier_hz,
                            f_offset_hz, out, out_dev, nullptr, static_cast<float*>(d_rows));
}

int gpsmi_acq_search_array_plan(int code_samples, size_t n, int antennas, int nbins, int n_coh, int n_seg,
                                double carrier_hz, double f_offset_hz, size_t* scratch_bytes,
                                int* bins_per_launch) {
    ArrayPlan pl;
    const int rc = array_plan(code_samples, n, antennas, nbins, n_coh, n_seg, carrier_hz, f_offset_hz, &pl);
    if (rc) return rc;
    if (scratch_bytes) *scratch_bytes = pl.scratch_bytes;
    if (bins_per_launch) *bins_per_launch = pl.nbc;
    return GPSMI_OK;
}

// ---- refinement of weak / deep hits (kernels and plan: gpsmi_refine.h) ------------------------
static int acq_refine_impl(gpsmi_acq* h, const void* iq, bool on_host, size_t n,
                           const gpsmi_refine_hit* hits, int nhits, const gpsmi_refine_cfg* cfg,
                           gpsmi_refine_out* out, float* grid, float* prompts) {
    GPSMI_REQUIRE(h && iq && hits && cfg && out, "null argument");
    RefPlan pl;
    int rc = ref_plan(h->cfg.code_samples, n, hits, nhits, cfg, &pl);
    if (rc) return rc;
    const void* d_iq;
    if ((rc = acq_need_time(h, "gpsmi_acq_refine", nhits, [&](int i) { return hits[i].prn; })) ||
        (rc = acq_enter(h)) || (rc = acq_input(h, iq, on_host, pl.hi, &d_iq)))   // (only what the windows read)
        return rc;
    const int cs = pl.cs, n_ms = pl.n_ms, n_df = pl.n_df;
    // the tables of the call, 8-byte items first
    const size_t b_start = pl.start.size() * sizeof(long long), b_inc = (size_t)n_df * sizeof(unsigned long long),
                 b_df = (size_t)n_df * sizeof(double), b_hit = (size_t)nhits * sizeof(RefHit);
    const size_t np = (size_t)nhits * 3 * n_ms, nm = (size_t)nhits * n_df * kRefEdges;
    if ((rc = h->d_rt.reserve(b_start + b_inc + b_df + b_hit, "gpsmi_acq_refine tables")) ||
        (rc = h->d_rp.reserve(np, "gpsmi_acq_refine prompts")) ||
        (rc = h->d_rm.reserve(nm, "gpsmi_acq_refine grid")) ||
        (rc = h->d_ro.reserve(kRefMaxHits, "gpsmi_acq_refine records")))
        return rc;
    long long* d_start = reinterpret_cast<long long*>(h->d_rt.p);
    unsigned long long* d_inc = reinterpret_cast<unsigned long long*>(h->d_rt.p + b_start);
    double* d_df = reinterpret_cast<double*>(h->d_rt.p + b_start + b_inc);
    RefHit* d_hit = reinterpret_cast<RefHit*>(h->d_rt.p + b_start + b_inc + b_df);
    const size_t lds_p = ((size_t)cs + kRefMsPerWg * 4 * 6) * sizeof(float);
    const size_t lds_g = (size_t)n_ms * sizeof(float2);
    if ((rc = acq_tables(h, {{d_start, pl.start.data(), b_start}, {d_inc, pl.dfinc.data(), b_inc},
                             {d_df, pl.dfs.data(), b_df}, {d_hit, pl.hits.data(), b_hit}})) ||
        (rc = acq_lds_optin(h, refine_prompt_kernel<1>, refine_prompt_kernel<0>, lds_p)) || (rc = acq_begin(h)))
        return rc;
    const dim3 gp((n_ms + kRefMsPerWg - 1) / kRefMsPerWg, nhits);
    with_fmt(h->iq_fmt, [&](auto fmt) {
        hipLaunchKernelGGL(refine_prompt_kernel<decltype(fmt)::value>, gp, dim3(256), lds_p, h->stream, d_iq,
                           h->d_rep_time.p, d_hit, d_start, cs, pl.tap, n_ms, h->d_rp.p);
    });
    hipLaunchKernelGGL(refine_grid_kernel, dim3((n_df + 3) / 4, nhits), dim3(256), lds_g, h->stream, h->d_rp.p,
                       d_inc, n_df, n_ms, h->d_rm.p);
    hipLaunchKernelGGL(refine_final_kernel, dim3(nhits), dim3(256), 0, h->stream, h->d_rp.p, h->d_rm.p, d_inc, d_df,
                       d_hit, n_df, n_ms, pl.tap, pl.step, pl.min_ratio, h->d_ro.p);
    if ((rc = acq_end(h))) return rc;
    GPSMI_HIP(hipMemcpyAsync(out, h->d_ro.p, (size_t)nhits * sizeof(gpsmi_refine_out), hipMemcpyDeviceToHost,
                             h->stream));
    if (grid)
        GPSMI_HIP(hipMemcpyAsync(grid, h->d_rm.p, nm * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (prompts)
        GPSMI_HIP(hipMemcpyAsync(prompts, h->d_rp.p, np * sizeof(float2), hipMemcpyDeviceToHost, h->stream));
    return gpsmi_acq_wait(h);
}

int gpsmi_acq_refine(gpsmi_acq* h, const void* iq, size_t n, const gpsmi_refine_hit* hits, int nhits,
                     const gpsmi_refine_cfg* cfg, gpsmi_refine_out* out, float* grid, float* prompts) {
    return acq_refine_impl(h, iq, true, n, hits, nhits, cfg, out, grid, prompts);
}

int gpsmi_acq_refine_dev(gpsmi_acq* h, const void* d_iq, size_t n, const gpsmi_refine_hit* hits, int nhits,
                         const gpsmi_refine_cfg* cfg, gpsmi_refine_out* out, float* grid, float* prompts) {
    return acq_refine_impl(h, d_iq, false, n, hits, nhits, cfg, out, grid, prompts);
}

int gpsmi_acq_refine_plan(int code_samples, size_t n, const gpsmi_refine_hit* hits, int nhits,
                          const gpsmi_refine_cfg* cfg, int* n_df) {
    RefPlan pl;
    const int rc = ref_plan(code_samples, n, hits, nhits, cfg, &pl);
    if (rc == GPSMI_OK && n_df) *n_df = pl.n_df;
    return rc;
}

// ---- bit-synchronous tracking of refined hits (kernel and plan: gpsmi_wtrk.h) ------------------
static int acq_track_impl(gpsmi_acq* h, const void* iq, bool on_host, size_t n, gpsmi_wtrk_state* states,
                          int nhits, const gpsmi_wtrk_cfg* cfg, gpsmi_wtrk_bit* bits) {
    GPSMI_REQUIRE(h && iq && states && cfg && bits, "null argument");
    WtrkPar par;
    int rc = wtrk_plan(h->cfg.code_samples, n, states, nhits, cfg, &par);
    if (rc) return rc;
    const void* d_iq;
    if ((rc = acq_need_time(h, "gpsmi_acq_track", nhits, [&](int i) { return states[i].prn; })) ||
        (rc = acq_enter(h)) || (rc = acq_input(h, iq, on_host, n, &d_iq)))
        return rc;
    const size_t nb = (size_t)nhits * par.n_bits * sizeof(gpsmi_wtrk_bit);
    if ((rc = h->d_wb.reserve((size_t)nhits * par.n_bits, "gpsmi_acq_track bit records")) ||
        (rc = h->d_ws.reserve(kWtrkMaxHits, "gpsmi_acq_track states")))
        return rc;
    GPSMI_HIP(hipMemcpyAsync(h->d_ws.p, states, (size_t)nhits * sizeof(gpsmi_wtrk_state), hipMemcpyHostToDevice,
                             h->stream));
    GPSMI_HIP(hipMemsetAsync(h->d_wb.p, 0, nb, h->stream));
    const size_t lds = wtrk_lds_bytes(par.cs);
    if ((rc = acq_lds_optin(h, wtrk_kernel<1>, wtrk_kernel<0>, lds)) || (rc = acq_begin(h))) return rc;
    with_fmt(h->iq_fmt, [&](auto fmt) {
        hipLaunchKernelGGL(wtrk_kernel<decltype(fmt)::value>, dim3(nhits), dim3(256), lds, h->stream, d_iq,
                           h->d_rep_time.p, par, h->d_ws.p, h->d_wb.p);
    });
    if ((rc = acq_end(h))) return rc;
    GPSMI_HIP(hipMemcpyAsync(states, h->d_ws.p, (size_t)nhits * sizeof(gpsmi_wtrk_state), hipMemcpyDeviceToHost,
                             h->stream));
    GPSMI_HIP(hipMemcpyAsync(bits, h->d_wb.p, nb, hipMemcpyDeviceToHost, h->stream));
    return gpsmi_acq_wait(h);
}

int gpsmi_acq_track(gpsmi_acq* h, const void* iq, size_t n, gpsmi_wtrk_state* states, int nhits,
                    const gpsmi_wtrk_cfg* cfg, gpsmi_wtrk_bit* bits) {
    return acq_track_impl(h, iq, true, n, states, nhits, cfg, bits);
}

int gpsmi_acq_track_dev(gpsmi_acq* h, const void* d_iq, size_t n, gpsmi_wtrk_state* states, int nhits,
                        const gpsmi_wtrk_cfg* cfg, gpsmi_wtrk_bit* bits) {
    return acq_track_impl(h, d_iq, false, n, states, nhits, cfg, bits);
}

int gpsmi_acq_track_plan(int code_samples, size_t n, const gpsmi_wtrk_state* states, int nhits,
                         const gpsmi_wtrk_cfg* cfg) {
    return wtrk_plan(code_samples, n, states, nhits, cfg, nullptr);
}

int gpsmi_wtrk_open(const gpsmi_refine_out* rec, int code_samples, int refine_tap_samples, int64_t data_start,
                    double carrier_hz, double f_offset_hz, gpsmi_wtrk_state* st) {
    return wtrk_open(rec, code_samples, refine_tap_samples, data_start, carrier_hz, f_offset_hz, st);
}

// ---- cancellation of strong satellites (kernels and plan: gpsmi_cancel.h) ---------------------
static int acq_cancel_impl(gpsmi_acq* h, const void* iq, bool on_host, size_t n, const gpsmi_cancel_sat* sats,
                           int nsat, const gpsmi_cancel_cfg* cfg, void* out_c64, gpsmi_cancel_out* out,
                           float* coef) {
    GPSMI_REQUIRE(h && iq && out_c64 && (out || nsat == 0), "null argument");
    CancelPlan pl;
    int rc = cancel_plan(h->cfg.code_samples, n, sats, nsat, cfg, &pl);
    if (rc) return rc;
    if ((rc = acq_need_time(h, "gpsmi_acq_cancel", nsat, [&](int i) { return sats[i].prn; }))) return rc;
    const bool u8 = h->iq_fmt == GPSMI_IQ_U8;
    const size_t out_bytes = n * sizeof(float2);
    bool in_place = false;
    if (!on_host) {
        const char *a = static_cast<const char*>(iq), *b = static_cast<const char*>(out_c64);
        in_place = !u8 && a == b;
        if (!in_place && a < b + out_bytes && b < a + h->iq_bytes(n))
            return fail(GPSMI_E_ARG, "gpsmi_acq_cancel_dev: d_iq and d_out_c64 overlap (only one complex64 "
                                     "buffer for both is cancelled in place)");
    }
    // where the input lies and where the satellites are taken out
    const void* d_in;
    if ((rc = acq_enter(h)) || (rc = acq_input(h, iq, on_host, n, &d_in))) return rc;
    float2* d_y = static_cast<float2*>(out_c64);
    if (on_host) {
        if (u8) {
            if ((rc = h->d_cx.reserve(n, "gpsmi_acq_cancel output"))) return rc;
            d_y = h->d_cx.p;
        } else {
            d_y = h->d_iq.p;
            in_place = true;
        }
    }
    const int mw = pl.max_windows;
    const size_t nres = (size_t)nsat * mw;
    std::vector<CancelRes> res;
    if (nres) {
        if ((rc = win_guarded("gpsmi_acq_cancel", [&] { res.resize(nres); return (int)GPSMI_OK; }))) return rc;
        if ((rc = h->d_cw.reserve(pl.wins.size(), "gpsmi_acq_cancel windows")) ||
            (rc = h->d_cr.reserve(nres, "gpsmi_acq_cancel results")))
            return rc;
        GPSMI_HIP(hipMemsetAsync(h->d_cr.p, 0, nres * sizeof(CancelRes), h->stream));
        if ((rc = acq_tables(h, {{h->d_cw.p, pl.wins.data(), pl.wins.size() * sizeof(CancelWin)}}))) return rc;
    }
    if ((rc = acq_begin(h))) return rc;
    // step 0: the input decoded or copied to where it is worked on
    if (u8) {
        const size_t blocks = (n + 255) / 256;
        hipLaunchKernelGGL(cancel_decode_kernel, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0,
                           h->stream, static_cast<const uint16_t*>(d_in), n, d_y);
    } else if (!in_place) {
        GPSMI_HIP(hipMemcpyAsync(d_y, d_in, out_bytes, hipMemcpyDeviceToDevice, h->stream));
    }
    // one launch per satellite, in the order given, each on the output of the one before: a
    // launch's workgroups own disjoint windows, the stream orders the launches
    for (int s = 0; s < nsat; ++s) {
        const int nw = pl.first[s + 1] - pl.first[s];
        hipLaunchKernelGGL(cancel_kernel, dim3(nw), dim3(256), 0, h->stream, d_y,
                           h->d_rep_time.p + (size_t)sats[s].prn * pl.cs, h->d_cw.p + pl.first[s], pl.inc[s], pl.cs,
                           pl.min_window, h->d_cr.p + (size_t)s * mw);
    }
    if ((rc = acq_end(h))) return rc;
    if (on_host)
        GPSMI_HIP(hipMemcpyAsync(out_c64, d_y, out_bytes, hipMemcpyDeviceToHost, h->stream));
    if (nres)
        GPSMI_HIP(hipMemcpyAsync(res.data(), h->d_cr.p, nres * sizeof(CancelRes), hipMemcpyDeviceToHost, h->stream));
    if ((rc = gpsmi_acq_wait(h))) return rc;
    // the windows' figures, added in window order
    for (int s = 0; s < nsat; ++s) {
        const int nw = pl.first[s + 1] - pl.first[s];
        gpsmi_cancel_out o = {sats[s].prn, nw, 0, 0, 0.0, 0.0};
        for (int w = 0; w < mw; ++w) {
            const CancelRes& r = res[(size_t)s * mw + w];
            if (w < nw && !r.done) ++o.n_skipped;
            if (w < nw && r.done) { o.energy_in += r.e_in; o.energy_removed += r.e_rem; }
            if (coef) std::memcpy(coef + ((size_t)s * mw + w) * 6, r.c, sizeof(r.c));
        }
        out[s] = o;
    }
    return GPSMI_OK;
}

int gpsmi_acq_cancel(gpsmi_acq* h, const void* iq, size_t n, const gpsmi_cancel_sat* sats, int nsat,
                     const gpsmi_cancel_cfg* cfg, float* out_c64, gpsmi_cancel_out* out, float* coef) {
    return acq_cancel_impl(h, iq, true, n, sats, nsat, cfg, out_c64, out, coef);
}

int gpsmi_acq_cancel_dev(gpsmi_acq* h, const void* d_iq, size_t n, const gpsmi_cancel_sat* sats, int nsat,
                         const gpsmi_cancel_cfg* cfg, void* d_out_c64, gpsmi_cancel_out* out, float* coef) {
    return acq_cancel_impl(h, d_iq, false, n, sats, nsat, cfg, d_out_c64, out, coef);
}

int gpsmi_acq_cancel_plan(int code_samples, size_t n, const gpsmi_cancel_sat* sats, int nsat,
                          const gpsmi_cancel_cfg* cfg, int* max_windows) {
    CancelPlan pl;
    const int rc = cancel_plan(code_samples, n, sats, nsat, cfg, &pl);
    if (rc == GPSMI_OK && max_windows) *max_windows = pl.max_windows;
    return rc;
}

// ---- the two covariance stages on refined records (their call: acq_cov_call above): spatial
// signatures over several antennas (gpsmi_sig.h), multi-tap correlation profiles (gpsmi_profile.h) --
static int acq_signature_impl(gpsmi_acq* h, const void* iq, bool on_host, size_t n, const gpsmi_sig_sat* sats,
                              int nsat, const gpsmi_sig_cfg* cfg, double* cov, int32_t* n_win, float* prompts) {
    GPSMI_REQUIRE(h && iq && sats && cov && n_win, "null argument");
    SigPlan pl;
    int rc = sig_plan(h->cfg.code_samples, n, sats, nsat, cfg, &pl);
    if (rc) return rc;
    const int cs = pl.cs, A = pl.A, mw = pl.max_windows;
    const CovCall c{"gpsmi_acq_signature", "prompts", (size_t)A * n, (size_t)nsat * A * mw, (size_t)nsat * A * A * 2};
    auto launch = [&](const void* d_iq, const WinRec* d_rec, const long long* d_start) -> int {
        const size_t lds = sig_lds_bytes(cs);
        if ((rc = acq_lds_optin(h, sig_prompt_kernel<1>, sig_prompt_kernel<0>, lds)) || (rc = acq_begin(h))) return rc;
        const dim3 gp((mw + kSigWinPerWg - 1) / kSigWinPerWg, nsat);
        with_fmt(h->iq_fmt, [&](auto fmt) {
            hipLaunchKernelGGL(sig_prompt_kernel<decltype(fmt)::value>, gp, dim3(256), lds, h->stream, d_iq, n, A,
                               h->d_rep_time.p, d_rec, d_start, cs, mw, h->d_vs.p);
        });
        hipLaunchKernelGGL(sig_cov_kernel, dim3(nsat), dim3(256), 0, h->stream, h->d_vs.p, d_rec, A, mw, h->d_vc.p);
        return acq_end(h);
    };
    return acq_cov_call(h, iq, on_host, c, pl, cov, n_win, prompts, launch);
}

int gpsmi_acq_signature(gpsmi_acq* h, const void* iq, size_t n, const gpsmi_sig_sat* sats, int nsat,
                        const gpsmi_sig_cfg* cfg, double* cov, int32_t* n_win, float* prompts) {
    return acq_signature_impl(h, iq, true, n, sats, nsat, cfg, cov, n_win, prompts);
}

int gpsmi_acq_signature_dev(gpsmi_acq* h, const void* d_iq, size_t n, const gpsmi_sig_sat* sats, int nsat,
                            const gpsmi_sig_cfg* cfg, double* cov, int32_t* n_win, float* prompts) {
    return acq_signature_impl(h, d_iq, false, n, sats, nsat, cfg, cov, n_win, prompts);
}

int gpsmi_acq_signature_plan(int code_samples, size_t n, const gpsmi_sig_sat* sats, int nsat,
                             const gpsmi_sig_cfg* cfg, int32_t* n_win, int* max_windows) {
    SigPlan pl;
    const int rc = sig_plan(code_samples, n, sats, nsat, cfg, &pl);
    if (rc != GPSMI_OK) return rc;
    acq_counts(pl, n_win);
    if (max_windows) *max_windows = pl.max_windows;
    return GPSMI_OK;
}

static int acq_profile_impl(gpsmi_acq* h, const void* iq, bool on_host, size_t n, const gpsmi_prof_sat* sats,
                            int nsat, const gpsmi_prof_cfg* cfg, double* cov, int32_t* n_runs, float* sums) {
    GPSMI_REQUIRE(h && iq && sats && cov && n_runs, "null argument");
    ProfPlan pl;
    int rc = prof_plan(h->cfg.code_samples, n, sats, nsat, cfg, &pl);
    if (rc) return rc;
    const int cs = pl.cs, Lh = pl.Lh, K = 2 * pl.Lh + 1, mr = pl.max_runs;
    const CovCall c{"gpsmi_acq_profile", "sums", n, (size_t)nsat * K * mr, (size_t)nsat * K * K * 2};
    auto launch = [&](const void* d_iq, const WinRec* d_rec, const long long* d_start) -> int {
        if ((rc = acq_begin(h))) return rc;
        const dim3 gp(mr, nsat);
        with_fmt(h->iq_fmt, [&](auto fmt) {
            with_value<8, kProfMaxHalf>(Lh <= 8 ? 8 : kProfMaxHalf, [&](auto lh) {
                hipLaunchKernelGGL((prof_sum_kernel<decltype(fmt)::value, decltype(lh)::value>), gp, dim3(256), 0,
                                   h->stream, d_iq, h->d_rep_time.p, d_rec, d_start, cs, Lh, pl.coh, mr, h->d_vs.p);
            });
        });
        hipLaunchKernelGGL(prof_cov_kernel, dim3(nsat), dim3(256), 0, h->stream, h->d_vs.p, d_rec, K, mr, h->d_vc.p);
        return acq_end(h);
    };
    return acq_cov_call(h, iq, on_host, c, pl, cov, n_runs, sums, launch);
}

int gpsmi_acq_profile(gpsmi_acq* h, const void* iq, size_t n, const gpsmi_prof_sat* sats, int nsat,
                      const gpsmi_prof_cfg* cfg, double* cov, int32_t* n_runs, float* sums) {
    return acq_profile_impl(h, iq, true, n, sats, nsat, cfg, cov, n_runs, sums);
}

int gpsmi_acq_profile_dev(gpsmi_acq* h, const void* d_iq, size_t n, const gpsmi_prof_sat* sats, int nsat,
                          const gpsmi_prof_cfg* cfg, double* cov, int32_t* n_runs, float* sums) {
    return acq_profile_impl(h, d_iq, false, n, sats, nsat, cfg, cov, n_runs, sums);
}

int gpsmi_acq_profile_plan(int code_samples, size_t n, const gpsmi_prof_sat* sats, int nsat,
                           const gpsmi_prof_cfg* cfg, int32_t* n_runs, int* max_runs, int* taps) {
    ProfPlan pl;
    const int rc = prof_plan(code_samples, n, sats, nsat, cfg, &pl);
    if (rc != GPSMI_OK) return rc;
    acq_counts(pl, n_runs);
    if (max_runs) *max_runs = pl.max_runs;
    if (taps) *taps = 2 * pl.Lh + 1;
    return GPSMI_OK;
}

// ---- collective detection (kernels and plan: gpsmi_collective.h) ------------------------------
int gpsmi_acq_collective_dev(gpsmi_acq* h, const void* d_rows, int nsv_rows, int nbins,
                             const gpsmi_collective_sat* sats, int nsat, const gpsmi_collective_grid* grid,
                             gpsmi_collective_cell* out_host, void* out_dev) {
    GPSMI_REQUIRE(h && d_rows, "null argument");
    GPSMI_REQUIRE(out_host || out_dev, "no output requested");
    ColPlan pl;
    int rc = collective_plan(h->cfg.code_samples, nsv_rows, nbins, sats, nsat, grid, &pl);
    if (rc || (rc = acq_enter(h))) return rc;
    const int cs = pl.cs;
    const size_t nz = (size_t)nsat * cs;
    if ((rc = h->d_cz.reserve(pl.scratch_bytes / sizeof(float), "gpsmi_acq_collective rows")) ||
        (rc = h->d_csat.reserve(kColMaxSats, "gpsmi_acq_collective satellites")) ||
        (rc = h->d_cc.reserve((size_t)pl.cells, "gpsmi_acq_collective cell map")) ||
        (rc = acq_tables(h, {{h->d_csat.p, sats, (size_t)nsat * sizeof(gpsmi_collective_sat)}})) ||
        (rc = acq_begin(h)))
        return rc;
    hipLaunchKernelGGL(collective_norm_kernel, dim3(nsat), dim3(256), 0, h->stream,
                       static_cast<const float*>(d_rows), nbins, cs, h->d_csat.p, h->d_cz.p);
    const float* z = h->d_cz.p;
    if (pl.pool > 1) {
        hipLaunchKernelGGL(collective_pool_kernel, dim3((cs + 255) / 256, nsat), dim3(256), 0, h->stream,
                           h->d_cz.p, cs, pl.pool, h->d_cz.p + nz);
        z = h->d_cz.p + nz;
    }
    hipLaunchKernelGGL(collective_kernel, dim3(pl.workgroups), dim3(256), 0, h->stream, z, h->d_csat.p, nsat, *grid,
                       cs, (int)pl.cells, h->d_cc.p);
    if ((rc = acq_end(h))) return rc;
    const size_t bytes = (size_t)pl.cells * sizeof(gpsmi_collective_cell);
    if (out_dev) GPSMI_HIP(hipMemcpyAsync(out_dev, h->d_cc.p, bytes, hipMemcpyDeviceToDevice, h->stream));
    if (out_host) GPSMI_HIP(hipMemcpyAsync(out_host, h->d_cc.p, bytes, hipMemcpyDeviceToHost, h->stream));
    return gpsmi_acq_wait(h);
}

int gpsmi_acq_collective_plan(int code_samples, int nsv_rows, int nbins, const gpsmi_collective_sat* sats, int nsat,
                              const gpsmi_collective_grid* grid, size_t* scratch_bytes, int* workgroups) {
    ColPlan pl;
    const int rc = collective_plan(code_samples, nsv_rows, nbins, sats, nsat, grid, &pl);
    if (rc == GPSMI_OK && scratch_bytes) *scratch_bytes = pl.scratch_bytes;
    if (rc == GPSMI_OK && workgroups) *workgroups = pl.workgroups;
    return rc;
}

// ---- auxiliary peaks per satellite (kernels and plan: gpsmi_peaks.h) ---------------------------
int gpsmi_acq_peaks_dev(gpsmi_acq* h, const void* d_rows, int nsv_rows, int nbins, const gpsmi_peaks_cfg* cfg,
                        gpsmi_peaks_pick* out_host, void* out_dev, float* cols_host, void* cols_dev) {
    GPSMI_REQUIRE(h && d_rows, "null argument");
    GPSMI_REQUIRE(out_host || out_dev, "no output requested");
    PeaksPlan pl;
    int rc = peaks_plan(h->cfg.code_samples, nsv_rows, nbins, cfg, &pl);
    if (rc || (rc = acq_enter(h))) return rc;
    const int cs = pl.cs;
    const bool want_cols = cols_host || cols_dev;
    const size_t npick = (size_t)nsv_rows * pl.k, ncol = npick * 2 * nbins;
    if ((rc = h->d_pst.reserve((size_t)nsv_rows * nbins, "gpsmi_acq_peaks statistics")) ||
        (rc = h->d_pz.reserve((size_t)nsv_rows * cs, "gpsmi_acq_peaks zmax")) ||
        (rc = h->d_pb.reserve((size_t)nsv_rows * cs, "gpsmi_acq_peaks bins")) ||
        (rc = h->d_pk.reserve(npick, "gpsmi_acq_peaks picks")) ||
        (want_cols && (rc = h->d_pcol.reserve(ncol, "gpsmi_acq_peaks columns"))) ||
        (rc = acq_begin(h)))
        return rc;
    const float* rows = static_cast<const float*>(d_rows);
    hipLaunchKernelGGL(peaks_stats_kernel, dim3(pl.hi - pl.lo + 1, nsv_rows), dim3(256), 0, h->stream, rows, nbins, cs,
                       pl.lo, h->d_pst.p);
    hipLaunchKernelGGL(peaks_zmax_kernel, dim3((cs + kPeaksLagTile - 1) / kPeaksLagTile, nsv_rows),
                       dim3(kPeaksLagTile), 0, h->stream, rows, nbins, cs, pl.lo, pl.hi, h->d_pst.p, h->d_pz.p,
                       h->d_pb.p);
    hipLaunchKernelGGL(peaks_pick_kernel, dim3(nsv_rows), dim3(256), 0, h->stream, rows, nbins, cs, pl.k, pl.guard,
                       pl.lo, pl.hi, h->d_pst.p, h->d_pz.p, h->d_pb.p, h->d_pk.p,
                       want_cols ? h->d_pcol.p : (float*)nullptr);
    if ((rc = acq_end(h))) return rc;
    const size_t bp = npick * sizeof(gpsmi_peaks_pick), bc = ncol * sizeof(float);
    if (out_dev) GPSMI_HIP(hipMemcpyAsync(out_dev, h->d_pk.p, bp, hipMemcpyDeviceToDevice, h->stream));
    if (out_host) GPSMI_HIP(hipMemcpyAsync(out_host, h->d_pk.p, bp, hipMemcpyDeviceToHost, h->stream));
    if (cols_dev) GPSMI_HIP(hipMemcpyAsync(cols_dev, h->d_pcol.p, bc, hipMemcpyDeviceToDevice, h->stream));
    if (cols_host) GPSMI_HIP(hipMemcpyAsync(cols_host, h->d_pcol.p, bc, hipMemcpyDeviceToHost, h->stream));
    return gpsmi_acq_wait(h);
}

int gpsmi_acq_peaks_plan(int code_samples, int nsv_rows, int nbins, const gpsmi_peaks_cfg* cfg, size_t* scratch_bytes,
                         int* workgroups) {
    PeaksPlan pl;
    const int rc = peaks_plan(code_samples, nsv_rows, nbins, cfg, &pl);
    if (rc == GPSMI_OK && scratch_bytes) *scratch_bytes = pl.scratch_bytes;
    if (rc == GPSMI_OK && workgroups) *workgroups = pl.workgroups;
    return rc;
}

int gpsmi_acq_set_input_format(gpsmi_acq* h, int fmt) {
    GPSMI_REQUIRE(h, "null handle");
    GPSMI_REQUIRE(fmt == GPSMI_IQ_C64 || fmt == GPSMI_IQ_U8, "unknown input format");
    GPSMI_HIP(hipSetDevice(h->cfg.device));
    GPSMI_HIP(hipStreamSynchronize(h->stream));
    h->iq_fmt = fmt;
    return GPSMI_OK;
}

int gpsmi_acq_last_ms(gpsmi_acq* h, float* ms) {
    GPSMI_REQUIRE(h && ms, "null argument");
    *ms = h->last_ms;
    return GPSMI_OK;
}

int gpsmi_acq_after_trk(gpsmi_acq* later, gpsmi_trk* earlier) {
    GPSMI_REQUIRE(later && earlier, "null handle");
    const HandleSync e = trk_sync(earlier);
    GPSMI_REQUIRE(e.device == later->cfg.device, "handles on different devices");
    GPSMI_HIP(hipSetDevice(e.device));
    if (e.tail) {                         // (an event record is a barrier packet in the queue: reuse one)
        GPSMI_HIP(hipStreamWaitEvent(later->stream, e.tail, 0));
        return GPSMI_OK;
    }
    GPSMI_HIP(hipEventRecord(e.order, e.stream));
    GPSMI_HIP(hipStreamWaitEvent(later->stream, e.order, 0));
    return GPSMI_OK;
}

}  // extern "C"

// ---- diagnostics: the statistics alone -----------------------------------------------------
namespace gpsmi {
// one workgroup per set of 2048 magnitudes, held and reduced as the correlation kernels do
__global__ __launch_bounds__(256) void corr_stats_kernel(const float* __restrict__ mags,
                                                         gpsmi_corr_stats* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float red[kStatsRedFloats];
    __shared__ float magbuf[kFftN];
    const int t = threadIdx.x;
    const float* m = mags + (size_t)blockIdx.x * kFftN;
    float mag[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) mag[q] = m[t + 256 * q];
    int amax; float peak, mean, sd, lo, hi;
    corr_stats8(mag, stats_sum8(mag), t, magbuf, red, amax, peak, mean, sd, lo, hi);
    if (t == 0) {
        gpsmi_corr_stats r;
        r.argmax = amax; r.peak = peak; r.mean = mean; r.std = sd; r.lo = lo; r.hi = hi;
        out[blockIdx.x] = r;
    }
}
}  // namespace gpsmi

extern "C" int gpsmi_dev_corr_stats(int device, const void* d_mags, int nsets, void* d_out) {
    GPSMI_REQUIRE(d_mags && d_out && nsets > 0, "null pointer or no sets");
    GPSMI_HIP(hipSetDevice(device));
    hipLaunchKernelGGL(gpsmi::corr_stats_kernel, dim3((unsigned)nsets), dim3(256), 0, 0,
                       static_cast<const float*>(d_mags), static_cast<gpsmi_corr_stats*>(d_out));
    GPSMI_HIP(hipGetLastError());
    GPSMI_HIP(hipDeviceSynchronize());
    return GPSMI_OK;
}
