// Tracking: all channels of one device per call, closed loop or replay.
//
// Replaces the numeric part of gpslib.SatStream.process (reference
// src/gpslib.py:1141-1210).  A "job" is one (channel, block) pair; the closed
// loop runs the open channels of one block, replay runs nb x nch jobs at once
// from a recorded state table.  A call is three stages in stream order (trk_launch), each with the
// paths a handle fixes at create time (CodePhase, Correlator):
//
//   code phase   carrier wipe-off and fold of the centre corr_avg code periods (demodDoppler
//                :1343-1346), circular correlation with the replica, |.|, mean / std / first argmax and
//                the neighbours of the peak (cacodeCorr :1315-1327, findCodePhase :1293-1304); CORR_MIN
//                threshold, fitCodePhase (:1268-1290) and the DELAY the block is decoded with (:1181-1182).
//                Fft2048: trk_corr_kernel (gpsmi_trk_corr.h), all of it in one workgroup per (block, up to
//                six channels), the 2048-point FFTs in LDS.  Long, any other code length:
//                trk_fold_general_kernel, the correlation of gpsmi_longcorr.h (native 16368-point,
//                32768-point pair or time domain), trk_decide_kernel (gpsmi_trk_general.h).
//   correlator   carrier-NCO mix of the whole block times the replica rolled by DELAY (decodeData
//                :1400-1401), summed per code-period window (:1408-1420) including the partial first
//                window and the carry into the next block (:1403-1405, :1440).  Span: trk_span_kernel on
//                the matrix pipe (gpsmi_trk_span.h), CS = 2048, a single-block form for small launches
//                and a batch form of persistent workgroups.  Span8: trk_span8_kernel (gpsmi_trk_span8.h),
//                CS = 16368 with N_CYC = 8.  Vector: trk_stream_kernel (gpsmi_trk_stream.h), everything
//                else; in chunks plus trk_partial_reduce_kernel where a code period exceeds one span.
//   epilogue     (gpsmi_trk_epilogue.h) window means, amplitude statistics (:1186-1188), phaseLockedLoop
//                (:1215-1262) and the state update (:1178, :1205-1208): from the records of Span8 or of
//                Span's single-block form, else from the window sums, eight lanes or a wave per job.
//
// Loop-carried state lives in device memory; the closed loop needs no host
// round trip between blocks.
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include <hip/hip_ext.h>

#include "gpsmi_common.h"
#include "gpsmi_devmem.h"
#include "gpsmi_fft.h"
#include "gpsmi_submit.h"

// Code that restates the reference's float32 arithmetic step by step (the phase
// argument of the carrier, the PLL, numpy's summation order) must not be fused into
// multiply-adds (hipcc contracts by default; see mul_rn/add_rn in gpsmi_common.h).  The streaming kernels (included below) keep the default.
#pragma clang fp contract(off)

namespace gpsmi {

constexpr float kTwoPiF = 6.28318530717958647692f;   // float32(2*pi), numpy's weak-scalar cast
constexpr float kPiF = 3.14159265358979323846f;

struct TrkParams {
    int cs;            // code samples (2048)
    int n_cyc;
    int corr_avg;
    float corr_min;
    float min_freq, max_freq;
    int nch;           // jobs per block
    int df_no;         // 1024 / n_cyc
    float t_last;      // SEC_TIME[NGPS-1]
    float om_min, om_max;   // float32(2*pi*MIN_FREQ), float32(2*pi*MAX_FREQ) from float64
    int flags;              // diagnostics, -DGPSMI_DIAG builds only (`make diag`, GPSMI_DEBUG_FLAGS): 1 no MAC,
                            // 2 no lane sums, 4 no mixed fix (vector correlator), 32 no fold, 64 no
                            // transforms (code-phase correlation); the shipped library ignores them
};

// per-job descriptor handed from the correlation kernel to the correlator and
// the epilogue: everything the correlator's set-up needs in one 32-byte load
struct __attribute__((aligned(32))) JobMid {
    int delay_used;    // DELAY the block is decoded with
    int active;
    int prn;
    float om;          // 2*pi*FREQ as the reference forms it
    float ph;          // PHASE at the start of the block
    int pad[3];
};

// a diagnostics bit of TrkParams::flags: constant false in the shipped library
__device__ __forceinline__ bool diag_flag(const TrkParams& P, int bit) {
#ifdef GPSMI_DIAG
    return (P.flags & bit) != 0;
#else
    (void)P; (void)bit;
    return false;
#endif
}

__device__ __forceinline__ float wave_sum_t(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
__device__ __forceinline__ void wave_argmax_t(float& v, int& i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        float ov = __shfl_down(v, o, 64);
        int oi = __shfl_down(i, o, 64);
        if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
}

// omega as the reference forms 2*pi*freq for a float32 FREQ (numpy >= 2):
// float32(2*pi) * freq in float32.
__device__ __host__ __forceinline__ float omega_of(float freq) {
    return mul_rn(kTwoPiF, freq);
}

// carrier factor exp(-j(phase + omega t[k])) with the float32 phase argument
__device__ __forceinline__ float2 wipe(float2 x, float phase, float om, float tk) {
    float p = add_rn(phase, mul_rn(om, tk));
    float s, c;
    sincosf(p, &s, &c);
    return make_float2(c * x.x + s * x.y, c * x.y - s * x.x);
}

// fitCodePhase (gpslib.py:1268-1290) in double on the float32 correlation values
__device__ inline double fit_code_phase(double lo, double pk, double hi, int mx) {
    double tri = (lo > hi) ? 0.5 * (hi - lo) / (pk - hi) : 0.5 * (hi - lo) / (pk - lo);
    double par = 0.5 * (hi - lo) / (2.0 * pk - hi - lo);
    return (double)mx + 0.5 * (tri + par);
}

}  // namespace gpsmi

#pragma clang fp contract(fast)
#include "gpsmi_trk_stream.h"
#include "gpsmi_trk_corr.h"
#include "gpsmi_longcorr.h"
#include "gpsmi_trk_general.h"
#pragma clang fp contract(off)
#include "gpsmi_trk_span.h"
#include "gpsmi_trk_span8.h"
#include "gpsmi_trk_epilogue.h"

namespace gpsmi {
// Upload of a streamed block by the GPU itself: the workgroups read the page-locked host block
// over PCIe (16 bytes per lane, everything requested at once) and write the staging block in
// HBM.  On its own stream it runs beside the tracking kernels of the previous block; the copy
// engines' own path (hipMemcpyAsync) measured anywhere between 40 and 240 us per step for the
// same 128 KiB - 1 MiB blocks from one run to the next.
typedef unsigned stage_u4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void stage_copy_kernel(stage_u4* __restrict__ dst,
                                                         const stage_u4* __restrict__ src, size_t n16) {
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * 256;
    for (; i < n16; i += stride) dst[i] = __builtin_nontemporal_load(src + i);
}
}  // namespace gpsmi

using namespace gpsmi;

struct gpsmi_trk {
    gpsmi_cfg cfg;
    int max_ch = 0;
    int n_streams = 1;                   // independent receivers (IQ streams) of the closed loop; a state
                                         // row is stream * max_ch + channel
    int rows() const { return n_streams * max_ch; }
    int span_single_max = 80;            // (block, channel group) units up to which the span correlator runs
                                         // its single-block form (GPSMI_SPAN_SINGLE_MAX; measured per step with
                                         // the round's final kernels: 50 against 56 us at 64 units, 69 against 63
                                         // at 96, 81 against 66 at 128)
    // streaming from host memory (gpsmi_trk_process_stream): two staging blocks filled on a stream
    // of their own (up_stream), so that the upload of block k + 1 runs under the kernels of block k
    DevBuf<char> d_stage[2];
    bool in_pending[2] = {false, false};
    bool stage_used[2] = {false, false};
    int stage_idx = 0;
    size_t stream_inline_max = 8u << 20;     // bytes up to which a streamed block is copied on the main stream
                                             // (GPSMI_STREAM_INLINE_MAX)
    hipEvent_t main_tail = nullptr;      // the event recorded behind the last work on `stream`, if any (borrowed)
    int cur = 0;                         // slot of the latest launch
    int timing = 1;                      // 1: record the four kernel-timing events per launch; 2: only the
                                         // begin / end stamps of the batch correlator's own dispatch (no
                                         // packet in the queue); 0: none
    // device memory: every buffer is a DevBuf (gpsmi_devmem.h) with a capacity of its own, in elements
    DevBuf<float2> d_tw;
    DevBuf<float> d_t32;
    DevBuf<float2> d_rep;            // [GPSMI_MAX_PRN + 1][cs] spectra
    DevBuf<float> d_code;            // [GPSMI_MAX_PRN + 1][cs] replica
    bool have_rep[GPSMI_MAX_PRN + 1] = {};
    DevBuf<float2> d_block;          // staging for host blocks
    // closed loop (max_ch jobs)
    DevBuf<gpsmi_trk_state> d_state;
    std::vector<gpsmi_trk_state> h_state;
    bool state_dirty_host = false;   // host copy newer than device
    // job buffers (trk_reserve).  njobs_cap is no allocation size -- each buffer has its own -- but the
    // job count the tables and both slots were last sized for, all of them together
    size_t njobs_cap = 0;
    DevBuf<gpsmi_trk_state> d_tab_in, d_tab_out;
    DevBuf<int> d_forced;
    float last_total_ms = 0.f, last_corr_ms = 0.f, last_cp_ms = 0.f;
    int replay_nb = 0;
    bool replay_forced = false;
    int corr_cg = 4;
    int corr_small1 = 384, corr_small2 = 1536;   // jobs per launch up to which 1 / 2 channels per correlation workgroup
    int done_by_dispatch = 1;          // 0: an event record behind the correlator instead
    bool want_matrix = true;           // the matrix-pipe correlators where they exist, as asked at create time
    // The path plan, fixed at create time: which kernels the code-phase stage and the correlator are.
    // One form per handle: the closed loop and the replay of a handle sum in the same order (bytewise
    // equal results).
    enum class CodePhase { Fft2048, Long };            // Long: code_samples != 2048, the method is lc's
    enum class Correlator { Span, Span8, Vector };     // Span: CS = 2048 (N_CYC 32 / 16 / 8 as template parameter
                                                       // NC); Span8: CS = 16368 with N_CYC = 8; both by default
                                                       // where they apply, Vector everywhere else
    CodePhase codephase = CodePhase::Fft2048;
    Correlator correlator = Correlator::Vector;
    LongCorr lc;                     // CodePhase::Long: method, replica spectra, job tables and statistics
    bool long_code() const { return codephase == CodePhase::Long; }
    // raw u8 input is read by trk_corr_kernel and trk_span_kernel alone
    bool takes_raw_u8() const { return correlator == Correlator::Span; }
    // the fold / correlation / statistics scratch of the long-code path exists once per handle, not per
    // result slot: two batches in flight on two streams would overwrite each other's intermediates
    bool scratch_per_handle() const { return long_code(); }
    // the vector correlator in more than one span per code period: partial sums, then a reduction
    bool chunked() const { return correlator == Correlator::Vector && nchunks > 1; }
    static constexpr int stream_j = 8;   // code positions per lane of the vector correlator
    int corr_overlap = 0;            // see gpsmi_trk_replay_run_async
    int fold_chunk = 0;              // blocks per fold -> correlation piece at CS = 16368
    int epilogue_form = 1;           // 1 = eight lanes per job in the batch epilogue (trk_epilogue8_kernel),
                                     // 0 = a wave per job (trk_epilogue_kernel); same bits
    DevBuf<float> d_code_eo;         // [GPSMI_MAX_PRN + 1][...]: the replica re-cut for the matrix correlators.  Span form
                                     // (2048): four planes by index mod 4, entry h of plane e = replica[(4 h + e) mod 2048],
                                     // 1024 entries each (a lane's run never wraps); span8 form: two planes by index
                                     // parity, each twice over
    int n_cu = 256;                  // compute units of the device
    int iq_fmt = GPSMI_IQ_C64;       // what the iq pointers of process / replay point to
    int nchunks = 1;                 // spans of 256 * stream_j positions per code period
    DevBuf<float2> d_fold;           // CodePhase::Long: the folded samples of one piece of a launch
    DevBuf<float2> d_partial_g;      // chunked(): [jobs][nchunks][n_cyc + 1] partial sums
    TrkParams P;
    int stream_thread = 1;
    int stream_depth = 2;            // calls a streamed step's buffers stay in use: 2 (gpsmi.h) or 3
    long long stat_backlog = 0;
    long long stat_quiesce_ns = 0, stat_evwait_ns = 0, stat_waits = 0;   // gpsmi_trk_wait behind streamed steps
    long long stat_wait_ns = 0, stat_launch_ns = 0, stat_steps = 0;   // streamed steps: host time waiting for the
                                                                      // step before last / making the runtime calls
    // What the runtime hands out comes last, in the order the members are released in, bottom up: the
    // submission thread is joined, then events go, then streams, then (above) the device buffers.  A
    // result slot goes as a whole, its buffers between its events and the streams.
    DevStream stream;
    DevStream epi_stream;                // replay: the epilogue of run k beside the code-phase
                                         // correlation of run k + 1 (the other slot's buffers), and the
                                         // result read-back behind it (trk_build says why not on a stream of its own)
    DevStream alt_stream;                // corr_overlap: the runs of result slot 1 (slot 0 keeps `stream`)
    DevStream up_stream;                 // uploads of streamed blocks beyond stream_inline_max
    // two result slots: a replay run writes one while the other is still being copied out
    struct Slot {
        DevBuf<gpsmi_trk_out> d_out;
        DevBuf<JobMid> d_mid;                // per-job descriptors and window sums of the slot's run
        DevBuf<float2> d_partial;
        DevBuf<float> d_rec;                 // raw sums of the single-block span correlator (gpsmi_trk_span.h):
                                             // per slot, the epilogue of run k reads them on its own stream
                                             // while run k + 1 writes the other slot's
        DevEvent ev[4];                      // start, corr done, correlator done, end
        DevEvent ready, copied;
        DevEvent corr_done, epi_done;        // correlator / epilogue of the slot's run
        hipEvent_t corr_stop = nullptr;      // the event that carries the end stamp of the slot's timed correlator (borrowed)
        bool copy_pending = false, epi_pending = false;
        int timing_pending = 0;              // the timing mode of the slot's run, until its times are taken
        hipStream_t run_stream = nullptr;    // corr_overlap: the stream the slot's runs are enqueued on (null: h->stream)
        // a replay run of this slot, or its read-back, is still outstanding
        bool in_flight() const { return copy_pending || epi_pending; }
    } slot[2];
    DevEvent order;                      // orders other handles' streams behind this one
    DevEvent up_done[2], stage_free[2];
    DevEvent in_done[2];                 // end of a streamed step (its iq read, its out written)
    // gpsmi_trk_process_stream's submission thread (default on; gpsmi_submit.h):
    // the four launches and the event record of a streamed step cost ~25 us of runtime calls on the
    // host -- as long as the step runs on the GPU -- so they are made by a thread of the handle's own
    // while the caller prepares its next block.  Every other entry point first waits for this thread
    // to have nothing queued (trk_quiesce), so at any time only one thread works on the handle.
    static int submit_step(void* h, const SubmitQueue::Job& job, SubmitQueue& q, char* errtext);
    SubmitQueue submit{submit_step, this};

    // A replay run, its read-back or its timing is still outstanding: the slots are not the closed
    // loop's to use.  (gpsmi_trk_replay_load asks the slots' in_flight() alone: times not yet taken
    // keep no kernel running, so they do not hold up a new table.)
    bool replay_busy() const {
        return slot[0].in_flight() || slot[1].in_flight() || slot[0].timing_pending || slot[1].timing_pending;
    }
    // bytes of `n` samples in the handle's input format
    size_t iq_bytes(size_t n) const { return n * (iq_fmt == GPSMI_IQ_U8 ? 2 : sizeof(float2)); }
};

using CodePhase = gpsmi_trk::CodePhase;
using Correlator = gpsmi_trk::Correlator;

constexpr int kSpanUnitsMax = 256;   // (block, channel group) units the single-block span form can serve (records)

// Everything sized by the job count, for njobs jobs, path by path.  A larger count reallocates all of
// it (a DevBuf whose size grows; the records of the single-block span form, of one fixed size, by hand).
static int trk_reserve(gpsmi_trk* h, size_t njobs) {
    if (njobs <= h->njobs_cap) return GPSMI_OK;
    h->njobs_cap = 0;
    const size_t cs = h->cfg.code_samples, per_job = h->cfg.n_cyc + 1;
    int rc = GPSMI_OK;
    // code phase, Long: the folded samples and LongCorr's tables (Fft2048 keeps everything in LDS)
    if (h->long_code()) {
        rc = h->d_fold.reserve(njobs * cs, "gpsmi_trk folded samples");
        if (!rc) rc = h->lc.reserve(njobs);
    }
    // correlator.  Span: 32 records per (block, channel group) of the single-block form; Span8: one
    // 2 KiB record per range of every (block, channel group); Vector in chunks: the partial sums
    if (h->correlator == Correlator::Span)
        for (auto& sl : h->slot) {
            sl.d_rec.release();
            if (!rc) rc = sl.d_rec.reserve((size_t)kSpanUnitsMax * 32 * kSpRecFloats, "gpsmi_trk span records");
        }
    if (h->correlator == Correlator::Span8) {
        const size_t units = ((njobs + h->max_ch - 1) / h->max_ch) * ((h->max_ch + kSpCh - 1) / kSpCh);
        for (auto& sl : h->slot)
            if (!rc) rc = sl.d_rec.reserve(units * kS8Ranges * kS8RecFloats, "gpsmi_trk span records");
    }
    if (!rc && h->chunked()) rc = h->d_partial_g.reserve(njobs * h->nchunks * per_job, "gpsmi_trk partial sums");
    // every path: the replay tables and, per result slot, descriptors, window sums and records
    if (!rc) rc = h->d_tab_in.reserve(njobs, "gpsmi_trk job table");
    if (!rc) rc = h->d_tab_out.reserve(njobs, "gpsmi_trk job table");
    if (!rc) rc = h->d_forced.reserve(njobs, "gpsmi_trk job table");
    for (auto& sl : h->slot) {
        if (!rc) rc = sl.d_mid.reserve(njobs, "gpsmi_trk job descriptors");
        if (!rc) rc = sl.d_partial.reserve(njobs * per_job, "gpsmi_trk window sums");
        if (!rc) rc = sl.d_out.reserve(njobs, "gpsmi_trk results");
    }
    if (!rc) h->njobs_cap = njobs;
    return rc;
}

// One kernel with an optional start and an optional stop event that carry the dispatch's own begin /
// end stamps and completion signal (hipExtLaunchKernelGGL) instead of event records around it; with
// neither, a plain launch.  The arguments are converted to the kernel's parameter types here
// (hipExtLaunchKernelGGL takes no others).
template <typename... KArgs, typename... Args>
static void launch_ev(void (*kernel)(KArgs...), dim3 grid, dim3 block, hipStream_t stream, hipEvent_t start,
                      hipEvent_t stop, Args... args) {
    if (start || stop)
        hipExtLaunchKernelGGL(kernel, grid, block, 0, stream, start, stop, 0, static_cast<KArgs>(args)...);
    else
        hipLaunchKernelGGL(kernel, grid, block, 0, stream, static_cast<KArgs>(args)...);
}

// The geometry of one launch of njobs = nblocks x nch jobs.
struct TrkGeom {
    int nblocks;
    int ngroups, ng_span;    // channel groups of the vector correlator / of the span forms and their epilogues
    // Span, a launch too small to fill the CUs with whole blocks (the closed loop): the single-block
    // form, every span of a block a wave of its own; same bits as the batch form (gpsmi_trk_span.h)
    bool span_single;
    bool span_batch;         // Span's other form: persistent workgroups, the one whose dispatch can carry events
    dim3 span_grid, vec_grid;
};
static TrkGeom trk_geometry(const gpsmi_trk* h, int njobs, int nch) {
    TrkGeom g{njobs / nch, (nch + kGroupCh - 1) / kGroupCh, (nch + kSpCh - 1) / kSpCh};
    const int span_units = g.nblocks * g.ng_span;
    g.span_single = h->correlator == Correlator::Span && span_units <= h->span_single_max;
    g.span_batch = h->correlator == Correlator::Span && !g.span_single;
    // batch form: two workgroups per CU, an equal number of (block, channel group) units each
    const int span_slots = sp_wg_per_cu(h->P.n_cyc) * h->n_cu;
    const int span_per = (span_units + span_slots - 1) / span_slots;
    g.span_grid = dim3(g.span_single ? span_units * 32 : (span_units + span_per - 1) / (span_per > 0 ? span_per : 1));
    g.vec_grid = dim3(((g.nblocks + 7) / 8) * 8 * g.ngroups, h->nchunks);
    return g;
}

// One launch: what its three stages share, and the stages.
struct TrkLaunch {
    gpsmi_trk* h; gpsmi_trk::Slot& sl; TrkParams P; TrkGeom g;
    const void* d_iq;                    // (raw uint16 when iq_fmt says so)
    const gpsmi_trk_state* st_in; gpsmi_trk_state* st_out; const int* forced;
    int njobs, nch;
    const float2* iq_c64() const { return static_cast<const float2*>(d_iq); }

    void launch_codephase(hipStream_t rs) const {
        const int nblocks = g.nblocks;
        if (h->long_code()) {
            // The folded samples (nch x cs complex64 per block: 805 MB for a 512-block batch at 16368) are an
            // intermediate between two kernels: with the native-length correlation they go through in
            // pieces of `fold_chunk` blocks that reuse one scratch area, so that what the fold writes is
            // still in the memory-side cache when the correlation reads it (0: the whole launch at once)
            const int chunk = (h->lc.pfa() && h->fold_chunk > 0 && h->fold_chunk < nblocks) ? h->fold_chunk : nblocks;
            for (int b0 = 0; b0 < nblocks; b0 += chunk) {
                const int nbc = nblocks - b0 < chunk ? nblocks - b0 : chunk;
                hipLaunchKernelGGL(trk_fold_general_kernel, dim3((P.cs + 255) / 256, nbc), dim3(256), 0, rs, iq_c64(),
                                   h->d_t32.p, st_in, P, h->d_fold.p, h->lc.d_xsel.p, h->lc.d_rsel.p, sl.d_mid.p, b0);
                h->lc.correlate(rs, h->d_fold.p, b0 * nch, nbc * nch, h->d_code.p, h->d_tw.p);
            }
            hipLaunchKernelGGL(trk_decide_kernel, dim3((njobs + 255) / 256), dim3(256), 0, rs, h->lc.d_stats.p,
                               forced, P, njobs, sl.d_out.p, sl.d_mid.p);
            return;
        }
        // channels per correlation workgroup: fewer channels = fewer live accumulators
        // = more workgroups per CU for the barrier-heavy FFT phase (GPSMI_CORR_CG to tune)
        // (a single block, the closed loop, is latency-bound: spread it over more CUs)
        // (GPSMI_CORR_SMALL: job counts up to which one / two channels per workgroup are taken; measured
        // with R batched receivers of 12 channels, tools/batched_bench.py)
        const int cg = njobs <= h->corr_small1 ? 1 : (njobs <= h->corr_small2 ? 2 : h->corr_cg);
        const int ng = (nch + cg - 1) / cg;
        with_value<6, 4, 2, 1>(cg, [&](auto cgv) { with_fmt(h->iq_fmt, [&](auto fmt) {
            hipLaunchKernelGGL((trk_corr_kernel<decltype(cgv)::value, decltype(fmt)::value>), dim3(corr_grid(nblocks, ng)),
                               dim3(256), 0, rs, d_iq, st_in, forced, h->d_rep.p, h->d_tw.p, P, ng, nblocks,
                               sl.d_out.p, sl.d_mid.p);
        }); });
    }

    // `start` / `stop` (either may be null) go to the span form's dispatch
    void launch_correlator(hipStream_t rs, hipEvent_t start, hipEvent_t stop) const {
        if (h->correlator == Correlator::Span) {
            // trk_span_kernel<NSPANS, WAVES, FMT, 0, NC>: <1, 1> the single-block form, <8, 4> the batch form
            with_value<32, 16, 8>(P.n_cyc, [&](auto ncv) { with_fmt(h->iq_fmt, [&](auto fmt) {
                with_value<1, 8>(g.span_single ? 1 : 8, [&](auto nsp) {
                    constexpr int NS = decltype(nsp)::value, W = NS == 1 ? 1 : 4;
                    launch_ev(trk_span_kernel<NS, W, decltype(fmt)::value, 0, decltype(ncv)::value>, g.span_grid,
                              dim3(64 * W), rs, start, stop, d_iq, sl.d_mid.p, h->d_code_eo.p, P, g.ng_span, g.nblocks,
                              sl.d_rec.p, sl.d_partial.p);
                });
            }); });
        } else if (h->correlator == Correlator::Span8) {
            const int nwaves = g.nblocks * g.ng_span * kS8Ranges;
            hipLaunchKernelGGL(trk_span8_kernel, dim3((nwaves + 3) / 4), dim3(256), 0, rs, iq_c64(), sl.d_mid.p,
                               h->d_code_eo.p, P, g.ng_span, g.nblocks, sl.d_rec.p);
        } else {                               // other block / code lengths
            float2* pdst = h->chunked() ? h->d_partial_g.p : sl.d_partial.p;
            with_value<32, 16, 8>(P.n_cyc, [&](auto ncv) { with_value<1, 0>(h->long_code() ? 0 : 1, [&](auto pow2) {
                hipLaunchKernelGGL((trk_stream_kernel<decltype(ncv)::value, decltype(pow2)::value != 0, 8>), g.vec_grid,
                                   dim3(kStreamThreads), 0, rs, iq_c64(), st_in, sl.d_mid.p, h->d_code.p, P, g.ngroups,
                                   g.nblocks, pdst);
            }); });
            if (h->chunked())
                hipLaunchKernelGGL(trk_partial_reduce_kernel, dim3((njobs * (P.n_cyc + 1) + 255) / 256), dim3(256), 0, rs,
                                   h->d_partial_g.p, h->nchunks, P.n_cyc + 1, njobs, sl.d_mid.p, sl.d_partial.p);
        }
    }

    // on `es`, with `tail_stop` (may be null) as its dispatch's stop event where the form at hand can
    // take it.  -> whether it did
    bool launch_epilogue(hipStream_t es, hipEvent_t tail_stop) const {
        if (h->correlator == Correlator::Span8) {      // (its epilogue does not take tail_stop)
            hipLaunchKernelGGL(trk_epilogue_span8_kernel, dim3((njobs + 3) / 4), dim3(256), 0, es, st_in, st_out,
                               sl.d_mid.p, sl.d_rec.p, g.ng_span, P, njobs, sl.d_out.p);
            return false;
        }
        if (g.span_single)
            with_value<32, 16, 8>(P.n_cyc, [&](auto ncv) {
                launch_ev(trk_epilogue_span_kernel<decltype(ncv)::value>, dim3(njobs), dim3(256), es, nullptr, tail_stop,
                          st_in, st_out, sl.d_mid.p, sl.d_rec.p, g.ng_span, P, njobs, sl.d_out.p);
            });
        else if (h->epilogue_form == 0)          // a wave per job
            launch_ev(trk_epilogue_kernel, dim3((njobs + 3) / 4), dim3(256), es, nullptr, tail_stop, st_in, st_out,
                      sl.d_mid.p, sl.d_partial.p, P, njobs, sl.d_out.p);
        else                                     // eight lanes per job (the default)
            with_value<32, 16, 8>(P.n_cyc, [&](auto ncv) {
                launch_ev(trk_epilogue8_kernel<decltype(ncv)::value>, dim3((njobs + 7) / 8), dim3(64), es, nullptr,
                          tail_stop, st_in, st_out, sl.d_mid.p, sl.d_partial.p, P, njobs, sl.d_out.p);
            });
        return tail_stop != nullptr;
    }
};

// the three stages over njobs jobs on the handle's stream, events around them
static int trk_launch(gpsmi_trk* h, gpsmi_trk::Slot& sl, const void* d_iq, const gpsmi_trk_state* st_in,
                      gpsmi_trk_state* st_out, const int* forced, int njobs, int nch, bool side_epilogue = false,
                      hipEvent_t tail_stop = nullptr, bool* tail_stop_used = nullptr) {
    // tail_stop: an event to carry the completion signal of the launch's LAST kernel (the epilogue),
    // instead of an event record behind it -- a record is a barrier packet, ~5 us of idle queue
    // between this step and the next (the streamed closed loop: 32.5 -> 27 us per block);
    // *tail_stop_used says whether the epilogue form at hand could take it
    TrkLaunch L{h, sl, h->P, trk_geometry(h, njobs, nch), d_iq, st_in, st_out, forced, njobs, nch};
    L.P.nch = nch;
    // the stream this launch goes to: the handle's, or (corr_overlap) the slot's own, so that the
    // code-phase correlation of this batch may run beside the correlator of the batch before
    hipStream_t rs = sl.run_stream ? sl.run_stream : h->stream;
    h->main_tail = nullptr;
    const bool timed = h->timing == 1;   // each event record is a barrier packet (~5 us of bubble)
    if (timed) GPSMI_HIP(hipEventRecord(sl.ev[0], rs));
    L.launch_codephase(rs);
    // When a launch is timed, the two events of the batch form of the span correlator are the
    // dispatch's own begin / end stamps (what a kernel trace reports), not event records around it:
    // no barrier packets next to the kernel and no launch gap inside the pair.
    const bool ext_timed = (timed || h->timing == 2) && L.g.span_batch;
    // replay: the event the epilogue stream (and a search) waits for is the completion signal of
    // the batch form's very dispatch, not a record behind it - a record is one more barrier packet
    // between this kernel and the next batch's first one
    const bool by_dispatch = L.g.span_batch && side_epilogue && h->done_by_dispatch;
    // (a timed launch that is also the one the epilogue stream waits for: ONE stop event serves
    // both -- the dispatch's completion signal -- instead of a record packet behind the kernel)
    sl.corr_stop = (ext_timed && by_dispatch) ? sl.corr_done : sl.ev[2];
    if (timed && !ext_timed) GPSMI_HIP(hipEventRecord(sl.ev[1], rs));
    L.launch_correlator(rs, ext_timed ? sl.ev[1].h : nullptr,
                        ext_timed ? sl.corr_stop : by_dispatch ? sl.corr_done.h : nullptr);
    if (timed && !ext_timed) GPSMI_HIP(hipEventRecord(sl.ev[2], rs));
    // replay: the epilogue goes to a stream of its own behind the correlator, so that the
    // code-phase correlation of the next run (other slot, main stream) starts at once
    hipStream_t es = rs;
    if (side_epilogue) {
        es = h->epi_stream;
        if (!by_dispatch) GPSMI_HIP(hipEventRecord(sl.corr_done, rs));     // (else the dispatch signals it)
        h->main_tail = sl.corr_done;          // (gpsmi_acq_after_trk orders the search behind this one)
        GPSMI_HIP(hipStreamWaitEvent(es, sl.corr_done, 0));
    }
    const bool stop_used = L.launch_epilogue(es, tail_stop);
    if (tail_stop_used) *tail_stop_used = stop_used;
    GPSMI_HIP(hipGetLastError());
    if (timed) GPSMI_HIP(hipEventRecord(sl.ev[3], es));
    if (side_epilogue) {
        GPSMI_HIP(hipEventRecord(sl.epi_done, es));
        sl.epi_pending = true;
    }
    return GPSMI_OK;
}

namespace gpsmi {
HandleSync acq_sync(gpsmi_acq* h);
HandleSync trk_sync(gpsmi_trk* h);
}  // namespace gpsmi

// kernel times of a finished launch into last_*_ms
static int trk_take_timing(gpsmi_trk* h, gpsmi_trk::Slot& sl) {
    if (!sl.timing_pending) return GPSMI_OK;
    if (sl.timing_pending == 1) {
        GPSMI_HIP(hipEventElapsedTime(&h->last_total_ms, sl.ev[0], sl.ev[3]));
        GPSMI_HIP(hipEventElapsedTime(&h->last_cp_ms, sl.ev[0], sl.ev[1]));
    }
    GPSMI_HIP(hipEventElapsedTime(&h->last_corr_ms, sl.ev[1], sl.corr_stop ? sl.corr_stop : sl.ev[2]));
    sl.timing_pending = 0;
    return GPSMI_OK;
}

// everything enqueued so far (kernels and read-backs) has finished
static int trk_settle(gpsmi_trk* h) {
    if (h->up_stream && (h->stage_used[0] || h->stage_used[1])) GPSMI_HIP(hipStreamSynchronize(h->up_stream));
    GPSMI_HIP(hipStreamSynchronize(h->stream));
    if (h->alt_stream) GPSMI_HIP(hipStreamSynchronize(h->alt_stream));
    GPSMI_HIP(hipStreamSynchronize(h->epi_stream));
    h->slot[0].epi_pending = h->slot[1].epi_pending = false;
    h->in_pending[0] = h->in_pending[1] = false;
    if (h->slot[0].copy_pending || h->slot[1].copy_pending)
        GPSMI_HIP(hipStreamSynchronize(h->epi_stream));
    for (int k = 0; k < 2; ++k) {          // older slot first: last_*_ms end up with the latest run
        gpsmi_trk::Slot& sl = h->slot[k == 0 ? (h->cur ^ 1) : h->cur];
        sl.copy_pending = false;
        int rc = trk_take_timing(h, sl);
        if (rc) return rc;
    }
    return GPSMI_OK;
}

static int trk_push_state(gpsmi_trk* h) {
    if (!h->state_dirty_host) return GPSMI_OK;
    h->main_tail = nullptr;              // (new work on `stream`: the recorded tail no longer covers it)
    GPSMI_HIP(hipMemcpyAsync(h->d_state.p, h->h_state.data(), h->rows() * sizeof(gpsmi_trk_state),
                             hipMemcpyHostToDevice, h->stream));
    GPSMI_HIP(hipStreamSynchronize(h->stream));
    h->state_dirty_host = false;
    return GPSMI_OK;
}

static int trk_pull_state(gpsmi_trk* h) {
    if (h->state_dirty_host) return GPSMI_OK;        // host copy is the newest
    GPSMI_HIP(hipMemcpyAsync(h->h_state.data(), h->d_state.p, h->rows() * sizeof(gpsmi_trk_state),
                             hipMemcpyDeviceToHost, h->stream));
    GPSMI_HIP(hipStreamSynchronize(h->stream));
    return GPSMI_OK;
}

// Wait for an event the GPU is about to signal by POLLING it: hipEventSynchronize may put the thread
// to sleep, and being woken by the driver measured ~250 us where the GPU had ~100 us of work left (the
// drop-in path waits like this once a second of signal: 353 -> ~110 us per report block).  After 2 ms
// the thread gives in and sleeps.
static hipError_t trk_spin_wait(hipEvent_t ev) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t q = hipEventQuery(ev);
        if (q != hipErrorNotReady) return q;
        if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
        __builtin_ia32_pause();
    }
    (void)hipGetLastError();                // (hipErrorNotReady is sticky in the thread's last-error slot)
    return hipEventSynchronize(ev);
}

// Is [p, p + bytes) page-locked host memory a kernel may address?  -> its device pointer.
// (memory from gpsmi_host_alloc is known without asking the runtime: hipPointerGetAttributes costs
// ~2 us a call, twice per step)
static bool trk_pinned_dev(const void* p, size_t bytes, void** dev) {
    if (bytes % 16 != 0 || ((uintptr_t)p & 15) != 0) return false;
    if (host_alloc_lookup(p, bytes, dev)) return true;
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();            // an unregistered pointer is not an error here
        return false;
    }
    if (at.type != hipMemoryTypeHost || at.devicePointer == nullptr) return false;
    hipPointerAttribute_t at_end{};
    const char* last = static_cast<const char*>(p) + bytes - 1;
    if (hipPointerGetAttributes(&at_end, last) != hipSuccess || at_end.type != hipMemoryTypeHost) {
        (void)hipGetLastError();
        return false;
    }
    *dev = at.devicePointer;
    return true;
}

// `cleared`: the submission queue whose thread runs the step (null: the caller's own thread does)
static int trk_stream_step(gpsmi_trk* h, const void* iq, size_t n, gpsmi_trk_out* out,
                           SubmitQueue* cleared = nullptr);

int gpsmi_trk::submit_step(void* h, const SubmitQueue::Job& job, SubmitQueue& q, char* errtext) {
    const int rc = trk_stream_step(static_cast<gpsmi_trk*>(h), job.iq, job.n, static_cast<gpsmi_trk_out*>(job.out), &q);
    if (rc) snprintf(errtext, SubmitQueue::kErrText, "%s", last_error_buf());
    return rc;
}

// Nothing is queued on the submission thread and it is idle: from here on the calling thread is the
// only one working on the handle.  A failure of a streamed step surfaces here (once).
static int trk_quiesce(gpsmi_trk* h) {
    if (!h) return GPSMI_OK;
    char report[SubmitQueue::kReport];
    const int rc = h->submit.quiesce(report);
    return rc ? fail(rc, "%s", report) : GPSMI_OK;
}

#define GPSMI_QUIESCE(h)                 \
    do {                                 \
        int rc_q__ = trk_quiesce(h);     \
        if (rc_q__) return rc_q__;       \
    } while (0)

namespace gpsmi {
HandleSync trk_sync(gpsmi_trk* h) {
    (void)trk_quiesce(h);                  // (a streamed step still being enqueued belongs in front)
    hipStream_t latest = h->slot[h->cur].run_stream ? h->slot[h->cur].run_stream : h->stream;
    return HandleSync{latest, h->order, h->cfg.device, h->main_tail};
}
}  // namespace gpsmi

// ---- the options of a tracking handle (gpsmi.h documents them), one row each, read-only counters last.
// trk_defaults, gpsmi_trk_set_option and gpsmi_trk_get_option walk this table; the process-wide defaults
// and the environment names are gpsmi_core.hip's, whose keys trk_defaults holds against these.
// Live: gpsmi_trk_set_option changes it on a live handle; LiveLower: ... and the next row bounds it from
// above, as it bounds that one from below; Create: taken at create time from its default, `set` is
// trk_defaults' alone; Stat: a counter, read only
enum class OptKind { Live, LiveLower, Create, Stat };
struct TrkOpt {
    const char* key; OptKind kind;
    long long builtin;                          // Create: the default of last resort (Live: the member's initialiser)
    long long (*get)(const gpsmi_trk*);
    // GPSMI_OK: stored; GPSMI_E_ARG: out of range (the caller words it); else the setter's own refusal
    int (*set)(gpsmi_trk*, long long);
};
#define OPT_GET(expr) [](const gpsmi_trk* h) -> long long { return (expr); }
#define OPT_SET(in_range, store) \
    [](gpsmi_trk* h, long long v) -> int { if (!(in_range)) return GPSMI_E_ARG; store; return GPSMI_OK; }
#define OPT_LIVE(key, field, in_range) {key, OptKind::Live, 0, OPT_GET(h->field), OPT_SET(in_range, h->field = (int)v)}
#define OPT_FLAG(key, field) {key, OptKind::Live, 0, OPT_GET(h->field), OPT_SET(true, h->field = v != 0)}
#define OPT_STAT(key, field) {key, OptKind::Stat, 0, OPT_GET(h->field), nullptr}
static const TrkOpt kTrkOpts[] = {
    // (reads as what runs, not what was asked)
    {"correlator", OptKind::Create, 1, OPT_GET(h->correlator != Correlator::Vector), OPT_SET(true, h->want_matrix = v != 0)},
    {"codephase", OptKind::Create, 0, OPT_GET(h->long_code() ? h->lc.option() : 0), nullptr},   // (LongCorr::build takes it)
    {"debug_flags", OptKind::Create, 0, OPT_GET(h->P.flags), OPT_SET(true, h->P.flags = (int)v)},
    OPT_LIVE("corr_cg", corr_cg, v == 2 || v == 4 || v == 6),
    // 0 <= corr_small1 <= corr_small2 <= 2^24 at every moment; trk_defaults takes the two together
    {"corr_small1", OptKind::LiveLower, 0, OPT_GET(h->corr_small1), OPT_SET(v >= 0 && v <= h->corr_small2, h->corr_small1 = (int)v)},
    OPT_LIVE("corr_small2", corr_small2, v >= h->corr_small1 && v <= (1 << 24)),
    OPT_LIVE("span_single_max", span_single_max, v >= 1 && v <= kSpanUnitsMax),
    {"stream_inline_max", OptKind::Live, 0, OPT_GET((long long)h->stream_inline_max), OPT_SET(v >= 0, h->stream_inline_max = (size_t)v)},
    OPT_FLAG("done_by_dispatch", done_by_dispatch), OPT_FLAG("stream_thread", stream_thread),
    {"corr_overlap", OptKind::Live, 0, OPT_GET(h->corr_overlap),
     [](gpsmi_trk* h, long long v) -> int {
         if (v != 0 && h->scratch_per_handle())
             return fail(GPSMI_E_STATE, "gpsmi_trk_set_option: corr_overlap needs CODE_SAMPLES = %d "
                         "(the general path's scratch is per handle)", kFftN);
         h->corr_overlap = v != 0;
         return GPSMI_OK;
     }},
    OPT_LIVE("fold_chunk", fold_chunk, v >= 0 && v <= (1 << 20)), OPT_LIVE("epilogue_form", epilogue_form, v == 0 || v == 1),
    OPT_LIVE("stream_depth", stream_depth, v >= 2 && v <= 64),
    OPT_STAT("stat_stream_steps", stat_steps), OPT_STAT("stat_waits", stat_waits), OPT_STAT("stat_backlog", stat_backlog),
    OPT_STAT("stat_quiesce_ns", stat_quiesce_ns), OPT_STAT("stat_evwait_ns", stat_evwait_ns),
    OPT_STAT("stat_stream_wait_ns", stat_wait_ns), OPT_STAT("stat_stream_launch_ns", stat_launch_ns),
};

static const TrkOpt* trk_find_opt(const char* key) {
    for (const TrkOpt& o : kTrkOpts)
        if (!strcmp(o.key, key)) return &o;
    return nullptr;
}

// The options of a new handle: their defaults come from gpsmi_set_default, else from the environment,
// else from the measurements quoted at the fields.  A default the handle refuses (out of range, or
// corr_overlap where the scratch is per handle) is ignored, and so is the error text of that refusal:
// the caller's last error stays what it was.
static int trk_defaults(gpsmi_trk* h) {
    char prev_err[512];
    snprintf(prev_err, sizeof(prev_err), "%s", last_error_buf());
    int known = 0;
    long long v = 0, v_up = 0;
    for (const TrkOpt* o = kTrkOpts; o->kind != OptKind::Stat; ++o, ++known) {
        const long long cur = o->kind == OptKind::Create ? o->builtin : o->get(h);
        if (!default_opt(o->key, &v, cur)) return fail(GPSMI_E_STATE, "gpsmi_trk_create: no process-wide option '%s'", o->key);
        if (o->kind == OptKind::LiveLower) {
            // with the row behind it, a pair that bounds each other: both or neither.  With the lower one
            // at 0 first, neither setter meets the other's old value
            const TrkOpt* up = ++o;
            const long long cur_up = up->get(h);
            known += default_opt(up->key, &v_up, cur_up);
            (up - 1)->set(h, 0);
            if (up->set(h, v_up) || (up - 1)->set(h, v)) { up->set(h, cur_up); (up - 1)->set(h, cur); }
        } else if (o->set && (o->kind == OptKind::Create || v != cur))
            o->set(h, v);
    }
    if (known != default_opt_count())
        return fail(GPSMI_E_STATE, "gpsmi_trk_create: the handle's option table and the process-wide one differ");
    snprintf(last_error_buf(), 512, "%s", prev_err);
    return GPSMI_OK;
}

static int trk_build(const gpsmi_cfg* cfg, int max_ch, gpsmi_trk* h) {
    GPSMI_HIP(hipDeviceGetAttribute(&h->n_cu, hipDeviceAttributeMultiprocessorCount, cfg->device));
    int rc = trk_defaults(h);
    if (!rc) rc = h->stream.create();
    if (!rc) rc = h->epi_stream.create();
    if (rc) return rc;
    // The read-back of a replay run follows the run's epilogue anyway and is over long before the next
    // epilogue is due, so it shares the epilogue's stream: the HIP runtime maps streams onto
    // four hardware queues (one per pipe of the command processor), and a process with this handle's
    // compute and epilogue streams, an acquisition handle's stream and the null stream has four.  A
    // fifth stream shares a queue with one of them -- which one differs from run to run -- and a step
    // whose epilogue or search queues behind the compute stream's kernels takes 0.33 ms instead of
    // 0.23 (GPU_MAX_HW_QUEUES=3 forces it; more queues than pipes cost as much: DESIGN.md 4.6).
    // The scope of each event is its row of gpsmi_event_scope.h (DESIGN.md 4.6 says who waits on what):
    // only `copied` stands in front of a host read of device-written memory.  The others order one
    // queue behind another or carry a stamp; made host-visible they would each write back and
    // invalidate the caches at completion, two of them under the next batch's code-phase correlation.
    rc = h->order.create<Ev::TrkOrder, EventScope::DeviceOnly>();
    for (auto& sl : h->slot) {
        for (auto& e : sl.ev)      // (stamps; gpsmi_trk_wait_prev synchronises on ev[3] / ev[2] to read stamps alone)
            if (!rc) rc = e.create<Ev::TrkStamp, EventScope::DeviceOnly>();
        if (!rc) rc = sl.ready.create<Ev::TrkReady, EventScope::DeviceOnly>();
        if (!rc) rc = sl.copied.create<Ev::TrkCopied, EventScope::HostVisible>();
        // corr_done (with timing: also a dispatch's stop event) is corr_stop as well, the stamp
        // gpsmi_trk_wait_prev synchronises on when no copy is pending: only stamps are read behind it,
        // never device-written memory, so it is device-only
        if (!rc) rc = sl.corr_done.create<Ev::TrkCorrDone, EventScope::DeviceOnly>();
        if (!rc) rc = sl.epi_done.create<Ev::TrkEpiDone, EventScope::DeviceOnly>();
    }
    if (rc) return rc;
    std::vector<float2> tw;
    make_twiddles(tw);
    if ((rc = h->d_tw.upload(tw, "gpsmi_trk twiddles"))) return rc;
    const int ngps = cfg->n_cyc * cfg->code_samples;
    const float fs = (float)(1000 * cfg->code_samples);
    std::vector<float> t32(ngps);
    for (int k = 0; k < ngps; ++k) t32[k] = (float)(k + 1) / fs;   // gpslib.py:1053-1054
    if ((rc = h->d_t32.upload(t32, "gpsmi_trk time base")) ||
        (rc = h->d_rep.reserve((size_t)(GPSMI_MAX_PRN + 1) * kFftN, "gpsmi_trk replica spectra")) ||
        // (zeroed for slot 0: closed channels)
        (rc = h->d_code.reserve_zeroed((size_t)(GPSMI_MAX_PRN + 1) * cfg->code_samples, "gpsmi_trk replicas")))
        return rc;
    // the rest of the path plan (gpsmi_trk_create set the code phase)
    if (h->want_matrix && !h->long_code()) {
        h->correlator = Correlator::Span;
        rc = h->d_code_eo.reserve_zeroed((size_t)(GPSMI_MAX_PRN + 1) * 2 * kFftN, "gpsmi_trk replica planes");
    } else if (h->want_matrix && cfg->code_samples == kS8Cs && cfg->n_cyc == kS8Rows) {
        h->correlator = Correlator::Span8;
        rc = h->d_code_eo.reserve_zeroed((size_t)(GPSMI_MAX_PRN + 1) * 2 * kS8Cs, "gpsmi_trk replica planes");
    }
    if (!rc && h->long_code()) rc = h->lc.build(cfg->code_samples, "gpsmi_trk");
    if (rc) return rc;
    if ((rc = h->d_block.reserve(ngps, "gpsmi_trk input block")) ||
        (rc = h->d_state.reserve_zeroed(max_ch, "gpsmi_trk states")))
        return rc;
    h->h_state.assign(max_ch, gpsmi_trk_state{});
    TrkParams& P = h->P;
    P.cs = cfg->code_samples; P.n_cyc = cfg->n_cyc;
    P.corr_avg = cfg->corr_avg < cfg->n_cyc ? cfg->corr_avg : cfg->n_cyc;   // gpslib.py:1071
    P.corr_min = cfg->corr_min; P.min_freq = cfg->min_freq; P.max_freq = cfg->max_freq;
    P.nch = max_ch; P.df_no = 1024 / cfg->n_cyc; P.t_last = t32[ngps - 1];
    P.om_min = (float)(2.0 * M_PI * (double)cfg->min_freq);
    P.om_max = (float)(2.0 * M_PI * (double)cfg->max_freq);
    return trk_reserve(h, max_ch);
}

extern "C" {

int gpsmi_trk_create(const gpsmi_cfg* cfg, int max_ch, gpsmi_trk** out) {
    GPSMI_REQUIRE(cfg && out, "null argument");
    *out = nullptr;
    GPSMI_REQUIRE(max_ch >= 1 && max_ch <= 4096, "max_ch out of range");
    GPSMI_REQUIRE(cfg->code_samples >= 1024 && cfg->code_samples <= 65536 &&
                      cfg->code_samples % 16 == 0,
                  "code_samples must be a multiple of 16 in 1024..65536");
    GPSMI_REQUIRE(cfg->n_cyc == 8 || cfg->n_cyc == 16 || cfg->n_cyc == 32,
                  "n_cyc must be 8, 16 or 32 (gpsglob.py:122)");
    GPSMI_REQUIRE(cfg->corr_avg >= 1, "corr_avg must be >= 1");
    GPSMI_REQUIRE(1024 / cfg->n_cyc <= GPSMI_MAX_DF, "n_cyc too small for the DF list");
    GPSMI_HIP(hipSetDevice(cfg->device));
    gpsmi_trk* h = new (std::nothrow) gpsmi_trk();
    if (!h) return fail(GPSMI_E_NOMEM, "out of host memory");
    h->cfg = *cfg;
    h->max_ch = max_ch;
    h->codephase = cfg->code_samples != kFftN ? CodePhase::Long : CodePhase::Fft2048;
    h->nchunks = (cfg->code_samples + 256 * h->stream_j - 1) / (256 * h->stream_j);
    const int rc = trk_build(cfg, max_ch, h);
    if (rc) {                       // nothing half-built leaves this function
        (void)gpsmi_trk_destroy(h);
        return rc;
    }
    *out = h;
    return GPSMI_OK;
}

int gpsmi_trk_destroy(gpsmi_trk* h) {
    if (!h) return GPSMI_OK;
    (void)trk_quiesce(h);
    h->submit.stop();
    (void)hipSetDevice(h->cfg.device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->epi_stream) (void)hipStreamSynchronize(h->epi_stream);
    if (h->up_stream) (void)hipStreamSynchronize(h->up_stream);
    if (h->alt_stream) (void)hipStreamSynchronize(h->alt_stream);
    delete h;                                // (releases events, streams and device buffers, in this order)
    return GPSMI_OK;
}

int gpsmi_trk_set_replica(gpsmi_trk* h, int prn, const float* replica, const float* spectrum) {
    GPSMI_REQUIRE(h && replica && (spectrum || h->long_code()), "null argument");
    GPSMI_REQUIRE(prn >= 1 && prn <= GPSMI_MAX_PRN, "prn out of range 1..37");
    GPSMI_QUIESCE(h);
    GPSMI_HIP(hipSetDevice(h->cfg.device));
    const size_t cs = h->cfg.code_samples;
    GPSMI_HIP(hipMemcpy(h->d_code.p + (size_t)prn * cs, replica, cs * sizeof(float),
                        hipMemcpyHostToDevice));
    if (h->correlator == Correlator::Span) {
        std::vector<float> eo(2 * kFftN);          // plane e of four, entry h = replica[(4 h + e) mod 2048], 1024 entries
        for (int e = 0; e < 4; ++e)
            for (int i = 0; i < kFftN / 2; ++i) eo[e * (kFftN / 2) + i] = replica[(4 * i + e) % kFftN];
        GPSMI_HIP(hipMemcpy(h->d_code_eo.p + (size_t)prn * 2 * kFftN, eo.data(), eo.size() * sizeof(float),
                            hipMemcpyHostToDevice));
    }
    if (h->correlator == Correlator::Span8) {   // plane e, entry s = replica[2 (s mod cs / 2) + e], each plane twice
        std::vector<float> eo(2 * cs);
        for (int e = 0; e < 2; ++e)
            for (size_t i = 0; i < cs; ++i) eo[e * cs + i] = replica[2 * (i % (cs / 2)) + e];
        GPSMI_HIP(hipMemcpy(h->d_code_eo.p + (size_t)prn * 2 * cs, eo.data(), eo.size() * sizeof(float),
                            hipMemcpyHostToDevice));
    }
    if (h->long_code()) {                  // (this path needs no 2048-point spectrum)
        const int rc = h->lc.set_replica(h->stream, h->d_code.p, prn, h->d_tw.p);
        if (rc) return rc;
    } else {
        GPSMI_HIP(hipMemcpy(h->d_rep.p + (size_t)prn * kFftN, spectrum, kFftN * sizeof(float2),
                            hipMemcpyHostToDevice));
    }
    h->have_rep[prn] = true;
    return GPSMI_OK;
}

int gpsmi_trk_open(gpsmi_trk* h, int ch, int prn, float freq_hz, int delay) {
    GPSMI_REQUIRE(h, "null handle");
    GPSMI_QUIESCE(h);
    GPSMI_REQUIRE(ch >= 0 && ch < h->rows(), "channel out of range");
    GPSMI_REQUIRE(prn >= 1 && prn <= GPSMI_MAX_PRN, "prn out of range 1..37");
    GPSMI_REQUIRE(delay >= 0 && delay < h->cfg.code_samples, "delay out of range");
    if (!h->have_rep[prn]) return fail(GPSMI_E_STATE, "no replica set for PRN %d", prn);
    GPSMI_HIP(hipSetDevice(h->cfg.device));
    int rc = trk_pull_state(h);
    if (rc) return rc;
    gpsmi_trk_state st{};                 // SatStream.__init__ (gpslib.py:1050-1091)
    st.prn = prn; st.delay = delay; st.freq = freq_hz; st.phase = 0.f;
    st.omega0 = (float)(2.0 * M_PI * (double)freq_hz);    // FREQ is a Python float here
    st.df_len = 1; st.df[0] = 0.f;
    st.std_dev = 0.005f;                  // STD_DEV "overwritten by 1st stream" (gpslib.py:1074)
    h->h_state[ch] = st;
    h->state_dirty_host = true;
    return GPSMI_OK;
}

int gpsmi_trk_close(gpsmi_trk* h, int ch) {
    GPSMI_REQUIRE(h, "null handle");
    GPSMI_QUIESCE(h);
    GPSMI_REQUIRE(ch >= 0 && ch < h->rows(), "channel out of range");
    GPSMI_HIP(hipSetDevice(h->cfg.device));
    int rc = trk_pull_state(h);
    if (rc) return rc;
    if (h->h_state[ch].prn == 0) return fail(GPSMI_E_STATE, "channel %d is not open", ch);
    h->h_state[ch] = gpsmi_trk_state{};
    h->state_dirty_host = true;
    return GPSMI_OK;
}

int gpsmi_trk_get_state(gpsmi_trk* h, int ch, gpsmi_trk_state* st) {
    GPSMI_REQUIRE(h && st, "null argument");
    GPSMI_QUIESCE(h);
    GPSMI_REQUIRE(ch >= 0 && ch < h->rows(), "channel out of range");
    GPSMI_HIP(hipSetDevice(h->cfg.device));
    int rc = trk_pull_state(h);
    if (rc) return rc;
    *st = h->h_state[ch];
    return GPSMI_OK;
}

int gpsmi_trk_set_state(gpsmi_trk* h, int ch, const gpsmi_trk_state* st) {
    GPSMI_REQUIRE(h && st, "null argument");
    GPSMI_QUIESCE(h);
    GPSMI_REQUIRE(ch >= 0 && ch < h->rows(), "channel out of range");
    GPSMI_REQUIRE(st->prn >= 0 && st->prn <= GPSMI_MAX_PRN, "prn out of range");
    GPSMI_REQUIRE(st->delay >= 0 && st->delay < h->cfg.code_samples, "delay out of range");
    GPSMI_REQUIRE(st->nps >= 0 && st->nps <= h->cfg.code_samples, "nps out of range");
    GPSMI_REQUIRE(st->df_len >= 1 && st->df_len <= h->P.df_no, "df_len out of range");
    GPSMI_REQUIRE(st->edge_state >= -1 && st->edge_state <= 2, "edge_state out of range");
    if (st->prn && !h->have_rep[st->prn])
        return fail(GPSMI_E_STATE, "no replica set for PRN %d", st->prn);
    GPSMI_HIP(hipSetDevice(h->cfg.device));
    int rc = trk_pull_state(h);
    if (rc) return rc;
    h->h_state[ch] = *st;
    h->state_dirty_host = true;
    return GPSMI_OK;
}

int gpsmi_trk_erase_prev(gpsmi_trk* h, int ch) {
    GPSMI_REQUIRE(h, "null handle");
    GPSMI_QUIESCE(h);
    GPSMI_REQUIRE(ch >= 0 && ch < h->rows(), "channel out of range");
    GPSMI_HIP(hipSetDevice(h->cfg.device));
    int rc = trk_pull_state(h);
    if (rc) return rc;
    h->h_state[ch].nps = 0;               // PREV_SAMPLES = [] (gpslib.py:1095-1099)
    h->h_state[ch].prev_sum_re = h->h_state[ch].prev_sum_im = 0.f;
    h->h_state[ch].edge_state = 0;        // EDGES = [0]
    h->state_dirty_host = true;
    return GPSMI_OK;
}

int gpsmi_trk_process_dev(gpsmi_trk* h, const void* d_iq, size_t n, gpsmi_trk_out* out) {
    GPSMI_REQUIRE(h && d_iq, "null argument");
    GPSMI_QUIESCE(h);
    GPSMI_REQUIRE(n == (size_t)h->n_streams * h->cfg.n_cyc * h->cfg.code_samples,
                  "input must hold one block of NGPS samples per stream");
    GPSMI_HIP(hipSetDevice(h->cfg.device));
    int rc = trk_push_state(h);
    if (rc) return rc;
    if (h->replay_busy() && (rc = trk_settle(h))) return rc;
    gpsmi_trk::Slot& sl = h->slot[0];      // the closed loop needs one slot only
    h->cur = 0;
    sl.run_stream = nullptr;
    // the streams of a handle are the "blocks" of one launch: stream r reads block r of d_iq and
    // owns the state rows r * max_ch ..., updated in place
    rc = trk_launch(h, sl, d_iq, h->d_state.p, h->d_state.p, nullptr, h->rows(), h->max_ch);
    if (rc) return rc;
    if (out)
        GPSMI_HIP(hipMemcpyAsync(out, sl.d_out.p, h->rows() * sizeof(gpsmi_trk_out),
                                 hipMemcpyDeviceToHost, h->stream));
    // nothing to hand back: the block is enqueued, the state stays on the device and the
    // next call queues behind it (get_state / wait / a call with `out` synchronise)
    if (!out && h->timing != 1) return GPSMI_OK;
    GPSMI_HIP(hipStreamSynchronize(h->stream));
    sl.timing_pending = h->timing == 1;    // (mode 2 is read out for replay runs only)
    return trk_take_timing(h, sl);
}

int gpsmi_trk_process(gpsmi_trk* h, const float* iq, size_t n, gpsmi_trk_out* out) {
    GPSMI_REQUIRE(h && iq && out, "null argument");
    GPSMI_QUIESCE(h);
    GPSMI_REQUIRE(n == (size_t)h->n_streams * h->cfg.n_cyc * h->cfg.code_samples,
                  "input must hold one block of NGPS samples per stream");
    GPSMI_HIP(hipSetDevice(h->cfg.device));
    h->main_tail = nullptr;
    GPSMI_HIP(hipMemcpyAsync(h->d_block.p, iq, h->iq_bytes(n), hipMemcpyHostToDevice, h->stream));
    return gpsmi_trk_process_dev(h, h->d_block.p, n, out);
}

// One streamed step: everything gpsmi_trk_process_stream promises, made by whichever thread works
// on the handle (the caller, or the handle's submission thread).  `cleared`, if given, is told as soon
// as the step before last is known to be complete.
static int trk_stream_step(gpsmi_trk* h, const void* iq, size_t n, gpsmi_trk_out* out, SubmitQueue* cleared) {
    GPSMI_HIP(hipSetDevice(h->cfg.device));
    const size_t bytes = h->iq_bytes(n);
    int rc = GPSMI_OK;
    if (!h->up_stream) {
        rc = h->up_stream.create();
        for (int k = 0; k < 2; ++k) {
            if (!rc) rc = h->up_done[k].create<Ev::TrkUpDone, EventScope::DeviceOnly>();
            if (!rc) rc = h->stage_free[k].create<Ev::TrkStageFree, EventScope::DeviceOnly>();
            // (with timing: also a dispatch's stop event, the step's tail_stop.  Host-visible: behind
            // trk_spin_wait on it the caller reads a page-locked `out` that the kernels stored into)
            if (!rc) rc = h->in_done[k].create<Ev::TrkInDone, EventScope::HostVisible>();
        }
        if (rc) return rc;
    }
    if (bytes > h->d_stage[0].n || bytes > h->d_stage[1].n) {
        if ((rc = trk_settle(h))) return rc;
        for (int k = 0; k < 2; ++k) {
            h->stage_used[k] = false;
            if ((rc = h->d_stage[k].reserve(bytes, "gpsmi_trk staging block"))) return rc;
        }
    }
    if ((rc = trk_push_state(h))) return rc;
    if (h->replay_busy() && (rc = trk_settle(h))) return rc;
    const int s = h->stage_idx;
    h->stage_idx ^= 1;
    // back-pressure: the step of the call before last has finished when this call returns (its iq may
    // be rewritten, its out is filled) -- the contract of gpsmi.h; the host therefore runs at most two
    // steps ahead of the device, which keeps one whole step queued behind the one that is running
    const auto t_w0 = std::chrono::steady_clock::now();
    if (h->in_pending[s]) {
        GPSMI_HIP(trk_spin_wait(h->in_done[s]));
        h->in_pending[s] = false;
    }
    const auto t_w1 = std::chrono::steady_clock::now();
    h->stat_wait_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(t_w1 - t_w0).count();
    if (cleared) cleared->step_cleared();
    // page-locked memory is read by a kernel (see stage_copy_kernel); anything else -- pageable
    // memory would fault under a kernel -- goes through the runtime's copy
    void* iq_dev = nullptr;
    const bool pinned = trk_pinned_dev(iq, bytes, &iq_dev);
    // the records of a step go straight into a page-locked `out` (the two kernels that fill a record
    // store over PCIe: 376 bytes per channel) instead of through d_out and a copy command behind them
    void* out_dev = nullptr;
    const bool out_direct = out && trk_pinned_dev(out, (size_t)h->rows() * sizeof(gpsmi_trk_out), &out_dev);
    // Up to 8 MiB per step (measured: one receiver's 128 KiB to 64 receivers' 8 MiB of raw samples)
    // the block goes up IN FRONT of its own kernels on the main stream: the two event packets that
    // order an upload stream against the main one cost ~7 us per step, and a copy kernel beside the
    // tracking kernels takes from them what it hides (27.7 against 34.6 us per block for one receiver,
    // 50 against 58 us for eight; equal at 64).  Beyond that it goes up on the upload stream under the
    // previous step's kernels, as soon as the kernels that read this staging block two calls ago have
    // finished.  Either way the host never waits.
    // (Letting the tracking kernels read the page-locked block where it lies, with no staging at all,
    // measured slower: DESIGN.md 8.)
    const bool in_line = pinned && bytes <= h->stream_inline_max;
    hipStream_t us = in_line ? h->stream : h->up_stream;
    if (!in_line && h->stage_used[s]) GPSMI_HIP(hipStreamWaitEvent(h->up_stream, h->stage_free[s], 0));
    if (pinned) {
        const size_t n16 = bytes / 16;
        const unsigned grid = (unsigned)((n16 + 255) / 256 < 512 ? (n16 + 255) / 256 : 512);
        hipLaunchKernelGGL(stage_copy_kernel, dim3(grid), dim3(256), 0, us,
                           static_cast<stage_u4*>(static_cast<void*>(h->d_stage[s].p)), static_cast<const stage_u4*>(iq_dev), n16);
    } else {
        GPSMI_HIP(hipMemcpyAsync(h->d_stage[s].p, iq, bytes, hipMemcpyHostToDevice, us));
    }
    if (!in_line) {
        GPSMI_HIP(hipEventRecord(h->up_done[s], h->up_stream));
        GPSMI_HIP(hipStreamWaitEvent(h->stream, h->up_done[s], 0));
    }
    gpsmi_trk::Slot& sl = h->slot[0];
    h->cur = 0;
    sl.run_stream = nullptr;
    const int timing = h->timing;
    h->timing = 0;                          // (no kernel-timing events in a streaming loop)
    gpsmi_trk_out* const d_out_keep = sl.d_out.p;
    if (out_direct) sl.d_out.p = static_cast<gpsmi_trk_out*>(out_dev);
    // the step's completion event = the completion signal of its last kernel, when nothing is
    // queued behind that kernel (no record copy, no upload-stream bookkeeping)
    const bool want_tail = in_line && (!out || out_direct);
    bool tail_used = false;
    rc = trk_launch(h, sl, h->d_stage[s].p, h->d_state.p, h->d_state.p, nullptr, h->rows(), h->max_ch,
                    /*side_epilogue=*/false, want_tail ? h->in_done[s].h : nullptr, &tail_used);
    sl.d_out.p = d_out_keep;
    h->timing = timing;
    if (rc) return rc;
    if (!in_line) {
        GPSMI_HIP(hipEventRecord(h->stage_free[s], h->stream));
        h->stage_used[s] = true;
    } else {
        h->stage_used[s] = false;           // (same stream: the next writer of this block queues behind its readers)
    }
    if (out && !out_direct)
        GPSMI_HIP(hipMemcpyAsync(out, sl.d_out.p, h->rows() * sizeof(gpsmi_trk_out),
                                 hipMemcpyDeviceToHost, h->stream));
    if (!tail_used) GPSMI_HIP(hipEventRecord(h->in_done[s], h->stream));
    h->in_pending[s] = true;
    h->stat_launch_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_w1).count();
    h->stat_steps += 1;
    return GPSMI_OK;
}

int gpsmi_trk_process_stream(gpsmi_trk* h, const void* iq, size_t n, gpsmi_trk_out* out) {
    GPSMI_REQUIRE(h && iq, "null argument");
    GPSMI_REQUIRE(n == (size_t)h->n_streams * h->cfg.n_cyc * h->cfg.code_samples,
                  "input must hold one block of NGPS samples per stream");
    if (!h->stream_thread) {
        GPSMI_QUIESCE(h);
        return trk_stream_step(h, iq, n, out);
    }
    if (!h->submit.running() && !h->submit.start()) {   // (no thread to be had: the caller's thread makes
        h->stream_thread = 0;                           // the runtime calls itself)
        return trk_stream_step(h, iq, n, out);
    }
    // the contract of gpsmi.h: return once the step of the call before last is complete -- the
    // submission thread says so when it has waited for that step on its way into this one
    // (stream_depth = 3: one step more -- the call returns when the step three calls back is
    // complete, so the caller can hand over its next block while this one is still being enqueued)
    char report[SubmitQueue::kReport];
    const int rc = h->submit.submit({iq, n, out}, h->stream_depth, report);
    return rc ? fail(rc, "%s", report) : GPSMI_OK;
}

int gpsmi_trk_replay_load(gpsmi_trk* h, int nb, const gpsmi_trk_state* table,
                          const int32_t* delay_used) {
    GPSMI_REQUIRE(h && table, "null argument");
    GPSMI_QUIESCE(h);
    GPSMI_REQUIRE(nb >= 1, "block count must be >= 1");
    if (h->n_streams != 1) return fail(GPSMI_E_STATE, "replay takes a handle with one stream");
    GPSMI_HIP(hipSetDevice(h->cfg.device));
    const int nch = h->max_ch;
    const size_t njobs = (size_t)nb * nch;
    for (size_t j = 0; j < njobs; ++j) {
        const gpsmi_trk_state& s = table[j];
        if (s.prn < 0 || s.prn > GPSMI_MAX_PRN || (s.prn && !h->have_rep[s.prn]))
            return fail(GPSMI_E_ARG, "replay table row %zu: bad PRN %d", j, s.prn);
        if (s.prn && (s.delay < 0 || s.delay >= h->cfg.code_samples || s.nps < 0 ||
                      s.nps > h->cfg.code_samples || s.df_len < 1 || s.df_len > h->P.df_no ||
                      s.edge_state < -1 || s.edge_state > 2))
            return fail(GPSMI_E_ARG, "replay table row %zu: state out of range", j);
        if (delay_used && delay_used[j] >= h->cfg.code_samples)
            return fail(GPSMI_E_ARG, "replay table row %zu: delay_used out of range", j);
    }
    // the epilogue of a run in flight reads d_tab_in and writes d_tab_out on its own stream: a new
    // table may only land once every outstanding run has finished (gpsmi.h states the rule)
    int rc = GPSMI_OK;
    if ((h->slot[0].in_flight() || h->slot[1].in_flight()) && (rc = trk_settle(h))) return rc;
    rc = trk_reserve(h, njobs);
    if (rc) return rc;
    h->main_tail = nullptr;
    GPSMI_HIP(hipMemcpyAsync(h->d_tab_in.p, table, njobs * sizeof(gpsmi_trk_state),
                             hipMemcpyHostToDevice, h->stream));
    if (delay_used)
        GPSMI_HIP(hipMemcpyAsync(h->d_forced.p, delay_used, njobs * sizeof(int),
                                 hipMemcpyHostToDevice, h->stream));
    GPSMI_HIP(hipStreamSynchronize(h->stream));
    h->replay_nb = nb;
    h->replay_forced = delay_used != nullptr;
    return GPSMI_OK;
}

int gpsmi_trk_replay_run_async(gpsmi_trk* h, const void* d_iq, int nb) {
    GPSMI_REQUIRE(h && d_iq, "null argument");
    GPSMI_QUIESCE(h);
    if (nb != h->replay_nb || nb < 1)
        return fail(GPSMI_E_STATE, "replay_run(nb=%d) without a matching replay_load (nb=%d)", nb,
                    h->replay_nb);
    GPSMI_HIP(hipSetDevice(h->cfg.device));
    const int nch = h->max_ch;
    h->cur ^= 1;                           // the other slot may still be on its way to the host
    gpsmi_trk::Slot& sl = h->slot[h->cur];
    // corr_overlap: consecutive runs are independent (two result slots), so they alternate between
    // two streams: the code-phase correlation of run k + 1 is then eligible while the correlator of
    // run k still runs, and the chip is never left to one kernel's tail.  Every kernel then shares
    // CUs with another one: throughput mode; the default keeps each kernel alone (its duration is
    // what the roofline is quoted on).
    if (h->corr_overlap && h->cur == 1 && !h->alt_stream) {
        const int rc = h->alt_stream.create();
        if (rc) return rc;
    }
    sl.run_stream = (h->corr_overlap && h->cur == 1) ? h->alt_stream : nullptr;
    hipStream_t rs = sl.run_stream ? sl.run_stream : h->stream;
    if (sl.copy_pending) {                 // its previous results must have left first
        // (that copy was queued behind the slot's epilogue -- replay_fetch_async -- so it stands for
        // both: one barrier packet between this run's first kernel and the previous run's last
        // instead of two, ~2 us of every step)
        GPSMI_HIP(hipStreamWaitEvent(rs, sl.copied, 0));
        sl.copy_pending = false;
        sl.epi_pending = false;
    }
    if (sl.epi_pending) {                  // ... or the epilogue that read its buffers be done
        GPSMI_HIP(hipStreamWaitEvent(rs, sl.epi_done, 0));
        sl.epi_pending = false;
    }
    // (mode 2 needs the batch form of the span correlator: its dispatch carries the stamps)
    sl.timing_pending = (h->timing == 2 && !trk_geometry(h, nb * nch, nch).span_batch) ? 0 : h->timing;
    return trk_launch(h, sl, d_iq, h->d_tab_in.p, h->d_tab_out.p,
                      h->replay_forced ? h->d_forced.p : nullptr, nb * nch, nch, /*side_epilogue=*/true);
}

int gpsmi_trk_wait(gpsmi_trk* h) {
    GPSMI_REQUIRE(h, "null handle");
    const auto t_q0 = std::chrono::steady_clock::now();
    h->stat_backlog += h->submit.submitted() - h->submit.finished();
    GPSMI_QUIESCE(h);
    const auto t_q1 = std::chrono::steady_clock::now();
    h->stat_quiesce_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(t_q1 - t_q0).count();
    GPSMI_HIP(hipSetDevice(h->cfg.device));
    // only streamed steps outstanding (in line on the main stream): the event behind the latest one
    // covers everything, and waiting for an event returns ~100 us sooner than the three stream
    // synchronisations of the general case
    if (!h->replay_busy() && !h->stage_used[0] && !h->stage_used[1] && (h->in_pending[0] || h->in_pending[1])) {
        const int latest = h->stage_idx ^ 1;               // (the slot of the step enqueued last)
        if (h->in_pending[latest]) {
            GPSMI_HIP(trk_spin_wait(h->in_done[latest]));
            h->in_pending[0] = h->in_pending[1] = false;
            h->stat_evwait_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_q1).count();
            h->stat_waits += 1;
            return GPSMI_OK;
        }
    }
    return trk_settle(h);
}

int gpsmi_trk_wait_prev(gpsmi_trk* h) {
    GPSMI_REQUIRE(h, "null handle");
    GPSMI_QUIESCE(h);
    GPSMI_HIP(hipSetDevice(h->cfg.device));
    gpsmi_trk::Slot& sl = h->slot[h->cur ^ 1];
    if (sl.copy_pending) {
        GPSMI_HIP(hipEventSynchronize(sl.copied));
        sl.copy_pending = false;
        sl.epi_pending = false;            // (the copy was queued behind the slot's epilogue)
    } else if (sl.timing_pending) {
        GPSMI_HIP(hipEventSynchronize(sl.timing_pending == 1 ? sl.ev[3] : (sl.corr_stop ? sl.corr_stop : sl.ev[2])));
    }
    return trk_take_timing(h, sl);
}

int gpsmi_trk_replay_run(gpsmi_trk* h, const void* d_iq, int nb) {
    int rc = gpsmi_trk_replay_run_async(h, d_iq, nb);
    if (rc) return rc;
    return gpsmi_trk_wait(h);
}

int gpsmi_trk_replay_fetch_async(gpsmi_trk* h, gpsmi_trk_out* out, size_t n) {
    GPSMI_REQUIRE(h && out, "null argument");
    GPSMI_QUIESCE(h);
    GPSMI_REQUIRE(n <= (size_t)h->replay_nb * h->max_ch, "more records than the last replay ran");
    GPSMI_HIP(hipSetDevice(h->cfg.device));
    gpsmi_trk::Slot& sl = h->slot[h->cur];
    // the copy runs on its own stream behind the run that produced the records, so the
    // next run (other slot) overlaps it
    if (sl.epi_pending) {                  // the records are complete when the slot's epilogue is
        GPSMI_HIP(hipStreamWaitEvent(h->epi_stream, sl.epi_done, 0));
    } else {
        GPSMI_HIP(hipEventRecord(sl.ready, sl.run_stream ? sl.run_stream : h->stream));
        GPSMI_HIP(hipStreamWaitEvent(h->epi_stream, sl.ready, 0));
    }
    GPSMI_HIP(hipMemcpyAsync(out, sl.d_out.p, n * sizeof(gpsmi_trk_out), hipMemcpyDeviceToHost,
                             h->epi_stream));
    GPSMI_HIP(hipEventRecord(sl.copied, h->epi_stream));
    sl.copy_pending = true;
    return GPSMI_OK;
}

int gpsmi_trk_replay_fetch(gpsmi_trk* h, gpsmi_trk_out* out, size_t n) {
    int rc = gpsmi_trk_replay_fetch_async(h, out, n);
    if (rc) return rc;
    return gpsmi_trk_wait(h);
}

int gpsmi_trk_replay(gpsmi_trk* h, const void* d_iq, int nb, const gpsmi_trk_state* table,
                     const int32_t* delay_used, gpsmi_trk_out* out) {
    GPSMI_REQUIRE(h && d_iq && table && out, "null argument");
    GPSMI_REQUIRE(nb >= 0, "negative block count");
    if (nb == 0) return GPSMI_OK;
    int rc = gpsmi_trk_replay_load(h, nb, table, delay_used);
    if (rc) return rc;
    rc = gpsmi_trk_replay_run(h, d_iq, nb);
    if (rc) return rc;
    return gpsmi_trk_replay_fetch(h, out, (size_t)nb * h->max_ch);
}

int gpsmi_trk_replay_states(gpsmi_trk* h, gpsmi_trk_state* states, size_t n) {
    GPSMI_REQUIRE(h && states, "null argument");
    GPSMI_QUIESCE(h);
    GPSMI_REQUIRE(n <= (size_t)h->replay_nb * h->max_ch,
                  "more states requested than the last replay produced");
    GPSMI_HIP(hipSetDevice(h->cfg.device));
    GPSMI_HIP(hipMemcpy(states, h->d_tab_out.p, n * sizeof(gpsmi_trk_state), hipMemcpyDeviceToHost));
    return GPSMI_OK;
}

int gpsmi_trk_last_ms(gpsmi_trk* h, float* total_ms, float* correlator_ms) {
    GPSMI_REQUIRE(h, "null handle");
    if (total_ms) *total_ms = h->last_total_ms;
    if (correlator_ms) *correlator_ms = h->last_corr_ms;
    return GPSMI_OK;
}

int gpsmi_trk_last_codephase_ms(gpsmi_trk* h, float* ms) {
    GPSMI_REQUIRE(h && ms, "null argument");
    *ms = h->last_cp_ms;
    return GPSMI_OK;
}

int gpsmi_trk_after_acq(gpsmi_trk* later, gpsmi_acq* earlier) {
    GPSMI_REQUIRE(later && earlier, "null handle");
    GPSMI_QUIESCE(later);
    const HandleSync e = acq_sync(earlier);
    GPSMI_REQUIRE(e.device == later->cfg.device, "handles on different devices");
    GPSMI_HIP(hipSetDevice(e.device));
    GPSMI_HIP(hipEventRecord(e.order, e.stream));
    GPSMI_HIP(hipStreamWaitEvent(later->stream, e.order, 0));
    return GPSMI_OK;
}

int gpsmi_trk_set_input_format(gpsmi_trk* h, int fmt) {
    GPSMI_REQUIRE(h, "null handle");
    GPSMI_QUIESCE(h);
    GPSMI_REQUIRE(fmt == GPSMI_IQ_C64 || fmt == GPSMI_IQ_U8, "unknown input format");
    if (fmt == GPSMI_IQ_U8 && !h->takes_raw_u8())
        return fail(GPSMI_E_UNSUPPORTED, "raw u8 IQ input needs CODE_SAMPLES = 2048 and the span "
                                         "correlator (option \"correlator\" = 1)");
    h->iq_fmt = fmt;
    return GPSMI_OK;
}

int gpsmi_trk_set_streams(gpsmi_trk* h, int n_streams) {
    GPSMI_REQUIRE(h, "null handle");
    GPSMI_QUIESCE(h);
    GPSMI_REQUIRE(n_streams >= 1 && (long long)n_streams * h->max_ch <= 65536,
                  "n_streams out of range (streams x channels <= 65536)");
    GPSMI_HIP(hipSetDevice(h->cfg.device));
    int rc = trk_settle(h);
    if (rc) return rc;
    const size_t rows = (size_t)n_streams * h->max_ch;
    const size_t ngps = (size_t)h->cfg.n_cyc * h->cfg.code_samples;
    // new buffers first, then the swap: a failed allocation leaves the handle as it was
    DevBuf<gpsmi_trk_state> d_state;
    DevBuf<float2> d_block;
    if (d_state.reserve(rows, "gpsmi_trk states") || d_block.reserve((size_t)n_streams * ngps, "gpsmi_trk input block"))
        return fail(GPSMI_E_NOMEM, "out of device memory for %d streams", n_streams);
    rc = hipMemset(d_state.p, 0, rows * sizeof(gpsmi_trk_state)) == hipSuccess ? trk_reserve(h, rows)
                                                                                : fail(GPSMI_E_HIP, "hipMemset of the state rows failed");
    if (rc) return rc;
    h->d_state = std::move(d_state);
    h->d_block = std::move(d_block);
    h->h_state.assign(rows, gpsmi_trk_state{});
    h->state_dirty_host = false;
    h->n_streams = n_streams;
    h->replay_nb = 0;
    return GPSMI_OK;
}

int gpsmi_trk_set_option(gpsmi_trk* h, const char* key, long long value) {
    GPSMI_REQUIRE(h && key, "null argument");
    GPSMI_QUIESCE(h);
    const TrkOpt* o = trk_find_opt(key);
    if (!o || o->kind == OptKind::Stat) return fail(GPSMI_E_ARG, "gpsmi_trk_set_option: unknown option '%s'", key);
    if (o->kind == OptKind::Create)
        return fail(GPSMI_E_STATE, "gpsmi_trk_set_option: '%s' is taken at create time (gpsmi_set_default)", key);
    const int rc = o->set(h, value);
    return rc == GPSMI_E_ARG ? fail(rc, "gpsmi_trk_set_option: %s = %lld out of range", key, value) : rc;
}

int gpsmi_trk_get_option(gpsmi_trk* h, const char* key, long long* value) {
    GPSMI_REQUIRE(h && key && value, "null argument");
    GPSMI_QUIESCE(h);
    const TrkOpt* o = trk_find_opt(key);
    if (!o) return fail(GPSMI_E_ARG, "gpsmi_trk_get_option: unknown option '%s'", key);
    *value = o->get(h);
    return GPSMI_OK;
}

int gpsmi_trk_corr_grid(int nblocks, int ngroups) {
    if (nblocks < 1 || ngroups < 1) return fail(GPSMI_E_ARG, "gpsmi_trk_corr_grid: counts must be >= 1");
    return corr_grid(nblocks, ngroups);
}

int gpsmi_trk_corr_wg_map(int nblocks, int ngroups, int wg, int* block, int* group) {
    GPSMI_REQUIRE(block && group, "null argument");
    GPSMI_REQUIRE(nblocks >= 1 && ngroups >= 1 && wg >= 0 && wg < corr_grid(nblocks, ngroups), "out of range");
    const CorrWg u = corr_wg_map(wg, nblocks, ngroups);
    *block = u.block;
    *group = u.group;
    return GPSMI_OK;
}

int gpsmi_trk_set_timing(gpsmi_trk* h, int on) {
    GPSMI_REQUIRE(h, "null handle");
    GPSMI_QUIESCE(h);
    h->timing = on == 2 ? 2 : (on != 0);
    return GPSMI_OK;
}

}  // extern "C"
