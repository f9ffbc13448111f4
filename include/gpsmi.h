/*
 * gpsmi.h -- C ABI of libgpsmi.so: GPS L1 C/A acquisition and tracking on MI355X.
 *
 * Plain C, plain pointers and sizes.  The reference receiver
 * (annappo/GPS-SDR-Receiver) has no FFI of its own: its hot path is three
 * Python call sites.  Each entry point below names the reference interface it
 * stands in for (file:line into the reference's src/); INTEGRATION.md shows the
 * ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *  - every function returns 0 (GPSMI_OK) or a negative GPSMI_E_* code and never
 *    throws or aborts; gpsmi_last_error() returns the text of the last failure
 *    on the calling thread (it carries the hipError_t string when there is one);
 *  - "no correlation" is in-band, as in the reference: delay = -1,
 *    code_phase = -1.0 (gpslib.py:1296-1304), not an error;
 *  - the caller owns all host buffers; no pointer is retained after return;
 *    device memory is owned by the handle (or by gpsmi_dev_alloc/free);
 *  - one handle is used by one host thread at a time; each handle has its own
 *    HIP stream; distinct handles are independent;
 *  - complex samples are interleaved float pairs (numpy complex64), "iq" counts
 *    are in complex samples.
 */
#ifndef GPSMI_H
#define GPSMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPSMI_OK            0
#define GPSMI_E_ARG        -1   /* bad argument (null, range, size)              */
#define GPSMI_E_HIP        -2   /* a HIP runtime call failed; see last_error     */
#define GPSMI_E_STATE      -3   /* channel not open / handle not configured      */
#define GPSMI_E_NOMEM      -4   /* out of host memory, or a device allocation the GPU cannot
                                 * serve (hipErrorOutOfMemory), from EVERY entry point that
                                 * sizes a buffer of its handle: the buffer is then absent,
                                 * the handle stays usable and a later, smaller call works.
                                 * (Any other failure of an allocation is GPSMI_E_HIP.)      */
#define GPSMI_E_UNSUPPORTED -5  /* e.g. code_samples that is not a power of two  */
#define GPSMI_E_COMM       -6   /* RCCL failure                                  */

#define GPSMI_MAX_PRN      37
#define GPSMI_MAX_DUMPS    33   /* N_CYC + 1 prompt dumps (gpslib.py:1418-1439)  */
#define GPSMI_MAX_DF       128  /* entries of the PLL drift list (1024 / N_CYC)  */
#define GPSMI_IQ_C64       0    /* input formats: numpy complex64 (the default) ... */
#define GPSMI_IQ_U8        1    /* ... or the recorder's uint16 (Q << 8 | I)      */

/* Module constants of gpsglob.py:35-131 that the path depends on. */
typedef struct gpsmi_cfg {
    int32_t code_samples;    /* CODE_SAMPLES  gpsglob.py:119; 2048 takes the LDS-FFT */
                             /*   path, any other multiple of 16 the direct one   */
    int32_t n_cyc;           /* N_CYC         gpsglob.py:122                     */
    int32_t corr_avg;        /* CORR_AVG      gpsglob.py:63                      */
    int32_t sweep_corr_avg;  /* SWEEP_CORR_AVG gpsglob.py:67                     */
    float   corr_min;        /* CORR_MIN      gpsglob.py:65                      */
    float   min_freq;        /* MIN_FREQ      gpsglob.py:72                      */
    float   max_freq;        /* MAX_FREQ      gpsglob.py:73                      */
    int32_t device;          /* HIP device ordinal                               */
} gpsmi_cfg;

const char* gpsmi_last_error(void);
const char* gpsmi_version(void);
/* sizeof() of the ABI structs as compiled: 0 cfg, 1 peak, 2 trk_state, 3 trk_out,
 * 4 offsetof(trk_out, code_phase), 5 fe_cfg, 6 pb_cfg, 7 refine_hit, 8 refine_cfg, 9 refine_out,
 * 10 wtrk_cfg, 11 wtrk_state, 12 wtrk_bit, 13 cancel_sat, 14 cancel_cfg, 15 cancel_out, 17 collective_sat,
 * 18 collective_grid, 19 collective_cell, 21 nul_cfg, 23 tfx_cfg, 24 peaks_cfg, 25 peaks_pick, 27 sig_sat, 28 sig_cfg (16, 20, 22 and 26 are not assigned); -1 otherwise.  Lets a binding verify its own struct declarations before the first real call.  */
int gpsmi_abi_sizeof(int which);
/* Kernel-variant selection and tuning thresholds, visible through the ABI (round 4: they used to
 * be environment variables read inside gpsmi_*_create, invisible to a C caller; the variables
 * still work, as the defaults of the options below when the ABI has not set them).
 *   gpsmi_set_default(key, value)    process-wide, for handles created afterwards
 *   gpsmi_clear_default(key)         back to the environment / built-in default
 *   gpsmi_trk_set_option / gpsmi_trk_get_option   one live handle (further down)
 * keys taken at create time:
 *   "correlator"        1 (default): the matrix-pipe correlators where they exist (CS = 2048 with
 *                       N_CYC = 32 / 16 / 8; CS = 16368 with N_CYC = 8); 0: the vector kernel
 *                       everywhere (env GPSMI_STREAM_MFMA)
 *   "codephase"         code_samples != 2048 only: 0 (default) native 16368-point LDS correlation
 *                       / zero-padded 32768-point pair, 1 the exact time-domain kernel, 2 the
 *                       32768-point pair at 16368 too (env GPSMI_DIRECT_CORR)
 *   "debug_flags"       diagnostics builds only (make diag): the ablation switches of the tuning tools
 *                       (env GPSMI_DEBUG_FLAGS); the shipped library stores and ignores them
 * keys a live tracking handle accepts as well (see DESIGN.md for the measurements behind them):
 *   "corr_cg"           channels per code-phase-correlation workgroup in batches: 2, 4 (default), 6
 *   "corr_small1/2"     jobs per launch up to which 1 / 2 channels per workgroup are taken (384, 1536;
 *                       0 <= corr_small1 <= corr_small2 <= 2^24 at every moment, so raise corr_small2
 *                       first and lower corr_small1 first).  These three change no result: a job's
 *                       record has the same bytes whichever of 1, 2, 4 or 6 channels share its
 *                       workgroup (tests/test_gpu_trk_corr.py)
 *   "span_single_max"   (block, channel group) units up to which the span correlator runs one wave
 *                       per span (80)
 *   "stream_inline_max" bytes up to which gpsmi_trk_process_stream uploads in front of the step's
 *                       own kernels (8 MiB)
 *   "done_by_dispatch"  1 (default): a replay's epilogue waits on the correlator dispatch's own
 *                       completion signal; 0: on an event record behind it
 *   "epilogue_form"     1 (default): the batch epilogue takes eight lanes per (block, channel) job
 *                       (1536 one-wave workgroups per 1024-block batch); 0: a wave per job (3072
 *                       four-wave workgroups).  Same bits; DESIGN.md 4.5
 *   "corr_overlap"      1: gpsmi_trk_replay_run_async queues a batch's code-phase correlation on a
 *                       second stream, so that it runs beside the previous batch's correlator
 *                       (throughput mode; 0, the default, keeps every kernel alone on the chip).
 *                       CODE_SAMPLES = 2048 only: a handle of the general path keeps its
 *                       correlation scratch once per handle, refuses 1 with GPSMI_E_STATE and
 *                       ignores a default of 1 (the option reads 0)
 *   "fold_chunk"        CODE_SAMPLES = 16368: blocks per fold -> correlation piece of a batch, so that the
 *                       folded samples stay in the memory-side cache (0, the default: the whole launch
 *                       at once; 0 .. 2^20)
 *   "stream_thread"     1 (default): the launches of a gpsmi_trk_process_stream step are made by a
 *                       submission thread of the handle while the caller prepares its next block
 *                       (they cost as much host time as the step takes on the GPU); 0: by the caller
 *   "stat_*"            (get only) counters of the streamed path, for tools/feed_split.py: steps, the
 *                       submission thread's time waiting for the step before last / making the runtime
 *                       calls, and gpsmi_trk_wait's time waiting for that thread / for the device
 *   "stream_depth"      2 (default): gpsmi_trk_process_stream returns once the step of the call
 *                       BEFORE LAST is complete (three caller buffers in rotation); D = 3 .. 64: the
 *                       step D calls back (D + 1 buffers) -- with the submission thread the caller
 *                       then hands over block k + 1 while block k is still being enqueued, and may
 *                       run up to D blocks ahead of the device (the jobs wait in the thread's queue;
 *                       the device still holds two steps at a time)                        */
int gpsmi_set_default(const char* key, long long value);
int gpsmi_clear_default(const char* key);
int gpsmi_device_count(int* n);
int gpsmi_device_name(int device, char* buf, size_t len);

/* ---- device buffers (IQ kept resident in HBM between calls) ------------- */
int gpsmi_dev_alloc(int device, size_t bytes, void** dptr);
int gpsmi_dev_free(int device, void* dptr);
int gpsmi_dev_upload(int device, void* dptr, const void* host, size_t bytes);
int gpsmi_dev_download(int device, void* host, const void* dptr, size_t bytes);
int gpsmi_dev_sync(int device);
/* Page-locked host memory (hipHostMalloc) for full-rate transfers.            */
int gpsmi_host_alloc(size_t bytes, void** hptr);
int gpsmi_host_free(void* hptr);
/* streamData's decode on the device (gpsrecv.py:168-173): raw uint16 (Q<<8|I)
 * -> complex64 (I + jQ)/127.5 - (1+1j); both pointers are device pointers.  */
int gpsmi_dev_unpack_u8iq(int device, void* d_iq_c64, const void* d_raw_u16,
                          size_t n_samples);
/* Diagnostics: the statistics that end every 2048-lag correlation (mean, population standard
 * deviation, first-index argmax, the peak's two circular neighbours) on magnitudes of the
 * caller's choosing, run exactly as the correlation kernels run them: nsets x 2048 floats, none
 * negative, one 256-thread workgroup per set.  Both pointers are device pointers; returns when
 * the records are written.                                                                  */
typedef struct gpsmi_corr_stats {
    int32_t argmax;
    float   peak, mean, std, lo, hi;
} gpsmi_corr_stats;
int gpsmi_dev_corr_stats(int device, const void* d_mags_f32, int nsets, void* d_out);

/* ========================================================================
 * Acquisition -- replaces the array arithmetic of gpsrecv.sweepAllSats
 * (gpsrecv.py:241-274): demodDoppler (:232-235), the n_avg folded FFTs
 * (:250-254), abs(ifft(X*conj(FFT_CACODE[sv]))) (:258) and the statistics of
 * findCodePhase (:217-223).  First-hit bookkeeping (:256-272), sorting (:274)
 * and getNewSats (:423-440) stay on the host over the returned table.
 * ======================================================================== */
typedef struct gpsmi_acq gpsmi_acq;

/* One cell of the search surface: first-index argmax, its value, mean and
 * population standard deviation of |corr| over the code_samples lags.        */
typedef struct gpsmi_peak {
    int32_t argmax;
    float   peak;
    float   mean;
    float   std;
} gpsmi_peak;

int gpsmi_acq_create(const gpsmi_cfg* cfg, gpsmi_acq** out);
int gpsmi_acq_destroy(gpsmi_acq* h);
/* FFT_CACODE[prn] (gpsrecv.py:574-577): spectrum of the sampled replica,
 * complex64 [code_samples]; the host computes it once (gpsmi.codes).         */
int gpsmi_acq_set_replica(gpsmi_acq* h, int prn, const float* spectrum_c64);
/* GPSCacode(prn) itself, float32 [code_samples]: needed when code_samples is not
 * 2048 (the correlation is then done in the time domain), and at 2048 by
 * gpsmi_acq_refine alone: there the first call allocates a table of 38 * 2048 floats on the device
 * and each call copies one row (it used to return at once; it can now return GPSMI_E_HIP).  */
int gpsmi_acq_set_replica_time(gpsmi_acq* h, int prn, const float* replica_f32);
/* Search nbins Doppler bins x nsv satellites on the first n_avg code periods of
 * iq.  freqs_hz[b] are the bin frequencies exactly as the reference steps them
 * (python floats); out is [nbins][nsv].  iq: host complex64, n >= n_avg*cs.   */
int gpsmi_acq_search(gpsmi_acq* h, const float* iq, size_t n,
                     const int32_t* prn, int nsv,
                     const double* freqs_hz, int nbins, int n_avg,
                     gpsmi_peak* out);
/* Same with iq already on the device; out_dev (optional) receives the table in
 * device memory as well (for the RCCL gather), out (optional) on the host.    */
int gpsmi_acq_search_dev(gpsmi_acq* h, const void* d_iq, size_t n,
                         const int32_t* prn, int nsv,
                         const double* freqs_hz, int nbins, int n_avg,
                         gpsmi_peak* out, void* out_dev);
/* As gpsmi_acq_search, plus the two circular neighbours of every peak,
 * nbr[(b*nsv + s)*2 + {0,1}] = corr[argmax-1], corr[argmax+1]: what
 * fitCodePhase (gpslib.py:1268-1290) needs when a channel re-acquires through
 * sweepFrequency / getCorrMax (gpslib.py:1350-1380).  first_period selects the
 * code period the n_avg periods start at (getCorrMax uses 0).                 */
int gpsmi_acq_search_ex(gpsmi_acq* h, const float* iq, size_t n,
                        const int32_t* prn, int nsv,
                        const double* freqs_hz, int nbins, int n_avg,
                        gpsmi_peak* out, float* nbr);
/* Non-blocking form for pipelines: enqueues the search (and the copies into
 * out / out_dev) on the handle's stream and returns; out must be page-locked
 * (gpsmi_host_alloc) and stay valid until gpsmi_acq_wait(), which blocks until
 * the work is done.  prn / freqs are consumed before the call returns.         */
int gpsmi_acq_search_dev_async(gpsmi_acq* h, const void* d_iq, size_t n,
                               const int32_t* prn, int nsv,
                               const double* freqs_hz, int nbins, int n_avg,
                               gpsmi_peak* out, void* out_dev);
int gpsmi_acq_wait(gpsmi_acq* h);
/* Non-coherent search for weak signals: the mean of the correlation magnitudes of n_seg
 * consecutive segments of n_coh code periods each (the reference integrates coherently only,
 * gpsrecv.py:249-259).  Segment s is what gpsmi_acq_search computes with n_avg = n_coh on iq
 * advanced by s * n_coh * code_samples samples: the carrier wipe-off restarts at phase 0 with
 * SEC_TIME[0 : n_coh * code_samples] in every segment (only magnitudes are kept, so the segment's
 * carrier phase does not matter).  Per cell
 *     S[lag] = (1 / n_seg) * sum_s |corr_s[lag]|      (float32, ascending s)
 * and out / nbr are gpsmi_acq_search_ex's records of S: first-index argmax, peak, mean, population
 * std, and S[argmax -+ 1] circularly (nbr may be NULL).  n_seg = 1 gives gpsmi_acq_search's bits.
 * n >= n_seg * n_coh * code_samples; iq in the handle's input format (gpsmi_acq_set_input_format),
 * host memory for gpsmi_acq_search_nc, device memory for gpsmi_acq_search_nc_dev (out_dev as in
 * gpsmi_acq_search_dev).  gpsmi_acq_last_ms reports the call.
 * The argmax is the code phase at the start of segment 0: code Doppler moves the code by
 * |f| / 1575.42e6 * fs * span samples over the span searched -- 0.65 samples per 100 ms at 5 kHz and
 * 2.048 Msps, 8 times that at 16.368 Msps -- which smears the peak and is not compensated (by this
 * call: gpsmi_acq_search_deep below compensates it).
 * code_samples = 2048 and the native 16368 correlation only: a handle forced onto a time-domain
 * path (option "codephase" 1 or 2, or another code length) returns GPSMI_E_UNSUPPORTED.  Scratch is
 * sized per call (bins are taken in chunks of at most 512 MiB of spectra); an allocation the device
 * cannot serve returns GPSMI_E_NOMEM and leaves the handle usable.                              */
int gpsmi_acq_search_nc(gpsmi_acq* h, const void* iq, size_t n,
                        const int32_t* prn, int nsv,
                        const double* freqs_hz, int nbins, int n_coh, int n_seg,
                        gpsmi_peak* out, float* nbr);
int gpsmi_acq_search_nc_dev(gpsmi_acq* h, const void* d_iq, size_t n,
                            const int32_t* prn, int nsv,
                            const double* freqs_hz, int nbins, int n_coh, int n_seg,
                            gpsmi_peak* out, void* out_dev);
/* Deep search: the non-coherent search with the code Doppler compensated, for spans of seconds.
 * The code slides against the sample clock by -f / carrier_hz samples per sample (f the Doppler),
 * so over s segments a satellite's correlation peak has moved by that times s * n_coh *
 * code_samples lags; the magnitudes of segment s are therefore added at the lag they had at the
 * start of iq.  Arguments as gpsmi_acq_search_nc[_dev], plus
 *   carrier_hz   the carrier the Doppler scales with (1575.42e6 for L1), finite and > 0;
 *   f_offset_hz  what the caller's bin frequencies differ from the true Doppler by (a tuner's ppm
 *                error appears as a common offset of every bin but does not move the code), finite;
 *                0 when freqs_hz are true Dopplers.
 * Segment s of bin b is computed exactly as in gpsmi_acq_search_nc (same wipe-off restart at phase
 * 0, same float32 arithmetic, same scaling).  With the integer circular shift
 *     m[b][s] = rint(-(freqs_hz[b] - f_offset_hz) / carrier_hz * s * n_coh * code_samples)
 * (float64, evaluated left to right, ties to even; computed on the host and uploaded as a table)
 *     S[i] = (1 / n_seg) * sum_s |corr_s[(i + m[b][s]) mod code_samples]|   (float32, ascending s)
 * and out / nbr / out_dev are gpsmi_acq_search_nc's records of S.  The argmax is the code phase at
 * the START of iq (segment 0 is never shifted), as in gpsmi_acq_search_nc.  Where every m is 0 -- a
 * 0 Hz bin, or a span too short to slide half a sample -- the records are gpsmi_acq_search_nc's,
 * byte for byte; the results of a bin do not depend on which other bins share the call.
 * n_seg 1..65535 as long as the segments of ONE bin fit the scratch of 512 MiB (n_seg *
 * code_samples * 8 bytes: 32768 segments at 2048, 4100 at 16368); beyond that GPSMI_E_UNSUPPORTED
 * (no chunking over segments).  Bins are taken in chunks as in gpsmi_acq_search_nc.
 * code_samples 2048 and the native 16368 correlation only: another length or a handle forced onto
 * a time-domain path (option "codephase" 1 or 2) returns GPSMI_E_UNSUPPORTED.  iq in the handle's
 * input format (GPSMI_IQ_U8 gives the same bytes as complex64); allocation failures as in
 * gpsmi_acq_search_nc; gpsmi_acq_last_ms reports the call.  Not compensated: fractions of a
 * sample, and a Doppler that changes over the span.                                           */
int gpsmi_acq_search_deep(gpsmi_acq* h, const void* iq, size_t n,
                          const int32_t* prn, int nsv,
                          const double* freqs_hz, int nbins, int n_coh, int n_seg,
                          double carrier_hz, double f_offset_hz,
                          gpsmi_peak* out, float* nbr);
int gpsmi_acq_search_deep_dev(gpsmi_acq* h, const void* d_iq, size_t n,
                              const int32_t* prn, int nsv,
                              const double* freqs_hz, int nbins, int n_coh, int n_seg,
                              double carrier_hz, double f_offset_hz,
                              gpsmi_peak* out, void* out_dev);
/* gpsmi_acq_search_deep_dev that also keeps the surfaces: d_rows receives S of every cell as float32
 * [nsv][nbins][code_samples] on the device (note the order: satellite first).  The records are
 * gpsmi_acq_search_deep_dev's byte for byte, and the rows are what they are statistics of: argmax is
 * the first index of a row's maximum and peak its value, exactly; mean and std are the row's mean and
 * population std, formed in the kernels' own summation orders (at 2048 the mean is the pinned sum of
 * gpsmi_acq_search_nc, which adds unrounded products: it is not a function of the rounded row alone
 * and differs from a sum over the row in the last bits).  code_samples 2048 and the native 16368, the
 * same bin chunking, either input format.  At 16368 n_seg must be at least 2 (one segment is the
 * coherent search, which keeps no surface: GPSMI_E_UNSUPPORTED).  d_rows == NULL is GPSMI_E_ARG.      */
int gpsmi_acq_search_deep_rows_dev(gpsmi_acq* h, const void* d_iq, size_t n,
                                   const int32_t* prn, int nsv,
                                   const double* freqs_hz, int nbins, int n_coh, int n_seg,
                                   double carrier_hz, double f_offset_hz,
                                   gpsmi_peak* out, void* out_dev, void* d_rows);
/* Array search (float64 restatement: tests/array_ref.py): the deep search over
 * antennas = A in 2 .. 4 antenna rows at once, for satellites that no single row shows.  The complex
 * correlations of the rows are combined per lag before anything is detected: a satellite's spatial
 * signature does not change over the span, so the cross products between antennas add coherently over
 * all segments, while the data bits, the residual carrier phase and the bin's frequency error are
 * common to the antennas and drop out of them.
 * Arguments as gpsmi_acq_search_deep[_dev], plus antennas.  iq is A rows of n samples, [A][n] with
 * antenna 0 first (the layout of gpsmi_nul_apply and gpsmi_acq_signature), in the handle's input
 * format; of each row the first n_seg * n_coh * code_samples samples are read.
 * For antenna a, bin b and segment s the wipe-off, the fold and the spectrum are exactly the deep
 * search's for that row alone (the same kernel, launched per row).  Let c[a][s][n] be the complex
 * circular correlation with the PRN's replica scaled by 1 / 2048, the value whose magnitude the deep
 * search takes, and m = m[b][s] the deep search's shift table, the same for all antennas.  Per cell
 *     D[i]    = sum_s sum_a |c[a][s][(i + m) mod cs]|^2
 *     R_ab[i] = sum_s c[a][s][(i + m) mod cs] * conj(c[b][s][(i + m) mod cs])           (a < b)
 *     T[i]    = (D[i] + 2 * sum_{a<b} |R_ab[i]|) * float32(1 / (A * n_seg))
 * in float32 in one fixed order: ascending s, then ascending a, then the pairs in lexicographic order
 * (0,1) (0,2) .. (1,2) ..; |R| is a float32 square root good to 1 ulp.  With C = sum_s c c^H,
 * T n_seg bounds w^H C w / A over weight vectors w of unit-modulus entries from above and reaches it
 * where every pair can be phased at once (always for A = 2, and for a satellite alone in its cell).
 * out / nbr / out_dev are the deep search's records of T: first-index argmax, peak, mean, population
 * std, and T[argmax -+ 1] circularly.  d_rows (gpsmi_acq_search_array_dev; may be NULL) receives T of
 * every cell as float32 [nsv][nbins][code_samples] on the device, and the rows are what the records are
 * statistics of: argmax and peak exactly.  T is a power, the deep search's S a magnitude: they are
 * not on one scale and no byte equality between the two searches is claimed.  The same arguments give
 * the same bytes from either entry point; GPSMI_IQ_U8 input gives the bytes of its complex64 decode; a
 * cell's record and row do not depend on which bins or PRNs share the call.
 * Bins are taken in chunks as in the deep search; the segments of ONE bin over all antennas must fit
 * the scratch of 512 MiB (A * n_seg * 2048 * 8 bytes), beyond that GPSMI_E_UNSUPPORTED.  Errors as
 * the deep search's; antennas outside 2 .. 4 and n * A beyond 2^40 are GPSMI_E_ARG; code_samples
 * other than 2048 -- the native 16368 path, whose sixteen lags per thread leave no registers for the
 * accumulators, and every time-domain path -- is GPSMI_E_UNSUPPORTED.  gpsmi_acq_last_ms reports the
 * call.  gpsmi_acq_search_array_plan makes the argument checks that need no handle (everything but
 * n_coh <= n_cyc, the replicas and the bin frequencies) without a GPU, and reports the scratch of a
 * launch and how many bins a launch takes.
 * Not done: more than four antennas (coherent groups of up to four, added non-coherently, would be
 * the way), spatial whitening against a jammer (a jammer raises every lag alike).                  */
int gpsmi_acq_search_array(gpsmi_acq* h, const void* iq, size_t n, int antennas,
                           const int32_t* prn, int nsv,
                           const double* freqs_hz, int nbins, int n_coh, int n_seg,
                           double carrier_hz, double f_offset_hz,
                           gpsmi_peak* out, float* nbr);
int gpsmi_acq_search_array_dev(gpsmi_acq* h, const void* d_iq, size_t n, int antennas,
                               const int32_t* prn, int nsv,
                               const double* freqs_hz, int nbins, int n_coh, int n_seg,
                               double carrier_hz, double f_offset_hz,
                               gpsmi_peak* out, void* out_dev, void* d_rows);
int gpsmi_acq_search_array_plan(int code_samples, size_t n, int antennas, int nbins, int n_coh, int n_seg,
                                double carrier_hz, double f_offset_hz,
                                size_t* scratch_bytes, int* bins_per_launch);
/* Collective detection (numpy restatement: tests/collective_ref.py): instead of a
 * decision per satellite, the normalised surfaces of all satellites are added at the lags that a
 * candidate receiver state (east, north, coarse time, clock) predicts, and the state where the sum
 * peaks is taken.  d_rows: the rows of gpsmi_acq_search_deep_rows_dev, [nsv_rows][nbins][code_samples].
 *
 * Step a, once per call and satellite p, all float32, no fused operations:
 *     mean[b] = sum(S[row][b]) / cs, std[b] = sqrt(sum((S - mean)^2) / cs)   (multiplications by
 *               float32(1) / float32(cs); the sums: thread t of 256 adds lags t, t + 256, ... in
 *               ascending order from 0, the 256 shares meet in an adjacent-pair tree -- at 2048
 *               gpsmi_stats.h's order)
 *     z[p][l] = max over b in [bin_lo, bin_hi] with std[b] > 0 of (S[row][b][l] - mean[b]) / std[b]
 * A bin whose std is not positive is skipped (no NaN enters a comparison); a satellite all of whose
 * bins are skipped has z = 0 everywhere.  With pool = w > 1, z is replaced by its circular running
 * maximum zw[l] = max_{k<w} z[(l + k) mod cs].
 * Step b, for grid point (i_t, i_n, i_e): E = e0 + i_e * d_e, N = n0 + i_n * d_n, T = t0 + i_t * d_t, and
 * for every clock lag c in {0, w, 2w, ...} < cs
 *     x_p = lag0_p + g_e_p * E + g_n_p * N + g_t_p * T + c     (float64, left to right, nothing fused)
 *     i_p = floor(x_p + 0.5) mod cs                            (non-negative)
 *     score = z_0[i_0] + z_1[i_1] + ...                        (float32, ascending p)
 * The cell of the point holds the largest score and its c, between equal scores the smallest c.
 * out_host / out_dev: gpsmi_collective_cell [n_t][n_n][n_e], at least one of them.  Limits: nsat
 * 1..32, pool 1..64, every |x_p| below 2^30, at most 2^22 grid points per call (more:
 * GPSMI_E_UNSUPPORTED, nothing is chunked silently), code_samples 2048 and 16368.  Argument errors are
 * GPSMI_E_ARG and need no GPU (gpsmi_acq_collective_plan makes the same checks without a handle, and
 * reports the scratch the call allocates and the workgroups of its grid launch, 64 grid points each).
 * The call returns when the work is done; gpsmi_acq_last_ms reports its three kernels.              */
typedef struct gpsmi_collective_sat {   /* no implicit padding: 48 bytes */
    int32_t row;                    /* the satellite's index in d_rows */
    int32_t bin_lo, bin_hi;         /* inclusive window of its bins */
    int32_t reserved;               /* 0 */
    double  lag0;                   /* predicted lag at E = N = T = 0, clock 0, samples */
    double  g_e, g_n, g_t;          /* samples per metre east / north, per second of coarse time */
} gpsmi_collective_sat;
typedef struct gpsmi_collective_grid {  /* no implicit padding: 64 bytes */
    int32_t n_e, n_n, n_t, pool;
    double  e0, n0, t0, d_e, d_n, d_t;
} gpsmi_collective_grid;
typedef struct gpsmi_collective_cell {  /* 8 bytes */
    float   score;
    int32_t lag;
} gpsmi_collective_cell;
int gpsmi_acq_collective_dev(gpsmi_acq* h, const void* d_rows, int nsv_rows, int nbins,
                             const gpsmi_collective_sat* sats, int nsat, const gpsmi_collective_grid* grid,
                             gpsmi_collective_cell* out_host, void* out_dev);
int gpsmi_acq_collective_plan(int code_samples, int nsv_rows, int nbins,
                              const gpsmi_collective_sat* sats, int nsat, const gpsmi_collective_grid* grid,
                              size_t* scratch_bytes, int* workgroups);
/* Auxiliary peaks per satellite (numpy restatement: tests/peaks_ref.py): the k largest
 * normalised peaks of every satellite's surfaces, more than a guard apart, so that a PRN that is in the
 * air twice (a spoofer beside the signal it replaces) yields two candidates where every search keeps
 * one.  d_rows: the rows of gpsmi_acq_search_deep_rows_dev, float32 [nsv_rows][nbins][code_samples],
 * finite (not checked).
 *
 * Step a, per satellite p and bin b of [bin_lo, bin_hi], all float32, no fused operations:
 *     mean[b], std[b]   exactly as step a of gpsmi_acq_collective forms them (the same operations and
 *                       summation order: 256 strided shares in ascending order, then the adjacent-pair
 *                       tree; the kernels share one device function)
 *     z[b][l] = (S[p][b][l] - mean[b]) / std[b]          (a subtraction and an IEEE division)
 * A bin whose std is not positive is skipped (no NaN enters a comparison).
 *     zmax[l] = max of z[b][l] over the bins of the window that are not skipped
 *     bin[l]  = the smallest such bin that attains it
 * Ranking by z and not by the excess over the mean keeps the cross-correlation ghosts of a strong
 * satellite out of the picks; which bin a peak belongs to is left to the caller, who gets the column
 * down the bins (a strong peak inflates its own bin's std, so the bin of largest z can lie beside it).
 * Step b, for pick i = 0 .. k - 1 of satellite p:
 *     lag    = the first index of the maximum of zmax among the lags still free
 *     pick   = {lag, bin[lag], zmax[lag], S[p][bin[lag]][lag]}
 *     cols[p][i][0][b] = S[p][b][lag] for every bin b of the row
 *     cols[p][i][1][b] = z[b][lag], or 0 for a skipped bin and for a bin outside the window
 * and every lag at circular distance <= guard_lags from `lag` stops being free.  When no lag is free,
 * or every bin of the window was skipped, the pick is {-1, -1, 0, 0} and its columns are zeros.
 * A satellite's picks depend on its own rows alone; two calls give the same bytes; there are no
 * atomics and no order that depends on scheduling.
 * out_host / out_dev: gpsmi_peaks_pick [nsv_rows][k], at least one of them; cols_host / cols_dev:
 * float32 [nsv_rows][k][2][nbins], optional.  Limits: code_samples 2048 and 16368 (anything else:
 * GPSMI_E_UNSUPPORTED), nsv_rows 1..38, nbins 1..4096, k 1..8, guard_lags -1 or 0..code_samples / 2.
 * Argument errors are GPSMI_E_ARG and need no GPU (gpsmi_acq_peaks_plan makes the same checks without
 * a handle, and reports the scratch the call allocates besides its outputs and the workgroups of its
 * statistics launch, one per satellite and bin of the window).  GPSMI_E_NOMEM leaves the handle
 * usable.  The call returns when the work is done; gpsmi_acq_last_ms reports its three kernels.     */
typedef struct gpsmi_peaks_cfg {   /* no implicit padding: 16 bytes */
    int32_t k;                      /* picks per satellite, 1..8 */
    int32_t guard_lags;             /* lags excluded either side of a pick, circular; -1: two chips
                                     * (4 at 2048, 32 at 16368); 0..code_samples / 2 */
    int32_t bin_lo, bin_hi;         /* inclusive bin window, 0 <= bin_lo <= bin_hi < nbins */
} gpsmi_peaks_cfg;
typedef struct gpsmi_peaks_pick {  /* 16 bytes */
    int32_t lag, bin;               /* -1, -1: no pick */
    float   z, s;                   /* z[bin][lag], S[bin][lag] */
} gpsmi_peaks_pick;
int gpsmi_acq_peaks_dev(gpsmi_acq* h, const void* d_rows, int nsv_rows, int nbins,
                        const gpsmi_peaks_cfg* cfg,
                        gpsmi_peaks_pick* out_host, void* out_dev,
                        float* cols_host, void* cols_dev);
int gpsmi_acq_peaks_plan(int code_samples, int nsv_rows, int nbins, const gpsmi_peaks_cfg* cfg,
                         size_t* scratch_bytes, int* workgroups);
/* Refinement of the hits of gpsmi_acq_search_nc / gpsmi_acq_search_deep: what a
 * high-sensitivity receiver runs between such a search and its loops.  Per hit (prn, delay = the
 * argmax the search returned, the code start at the start of iq; freq_hz = the bin) it integrates
 * coherently over each 20-ms data bit at the code phase found, over a fine frequency grid and all
 * 20 bit-edge positions, and returns Doppler to a few Hz, the bit edge, a sub-sample code phase, a
 * C/N0 estimate and a detection statistic of its own.
 * Stage 1, prompts.  cs = code_samples, fs = 1000 cs.  The window of millisecond k starts at
 *     n_k = k cs + delay + m[k],   m[k] = rint(-(freq_hz - f_offset_hz) / carrier_hz * k * cs)
 * (float64, left to right, ties to even; on the host, uploaded as a table); a hit with delay <
 * tap_samples takes delay + cs instead (its first window is the second code period; nothing else
 * changes).  For the taps tau = -tap_samples, 0, +tap_samples (early, prompt, late)
 *     P[tau][k] = sum_{i < cs} x[n_k + tau + i] exp(-j 2 pi freq_hz (n_k + tau + i) / fs) replica[i]
 * with replica = GPSCacode(prn) (gpsmi_acq_set_replica_time, which a handle of 2048 samples keeps
 * for this call alone).  The carrier phase is an integer: sample index * (freq_hz / fs in 0.64
 * fixed point) mod 2^64, its top 24 bits give sine and cosine (as gpsmi_fe's mixer): exact at any
 * index.  float32 sums in one fixed order.
 * Stage 2, grid.  df_d = -df_half_hz + d df_step_hz for d < n_df = floor(2 half / step) + 1,
 * B = n_ms / 20 - 1 bits, edges e = 0 .. 19:
 *     M[d][e] = sum_{b < B} | sum_{k = e + 20 b}^{e + 20 b + 19} P[0][k] exp(-j 2 pi df_d k / 1000) |^2
 * (the phase again an integer, k * (df_d / 1000 in 0.64 fixed point)).  The peak is the first-index
 * argmax over (d, e) in that order.
 * n >= (n_ms + 2) cs + tap_samples, and every window of the slide must lie inside iq (GPSMI_E_ARG).
 * nhits 1 .. 64; n_ms a multiple of 20, 40 .. GPSMI_REFINE_MAX_MS (what the grid kernel's LDS
 * holds; beyond it GPSMI_E_UNSUPPORTED); code_samples 2048 and 16368 only (GPSMI_E_UNSUPPORTED).
 * A hit's record depends on that hit alone, not on what shares the call, and two calls give the
 * same bytes.  iq in the handle's input format (GPSMI_IQ_U8 gives the same bytes as complex64),
 * host memory for gpsmi_acq_refine, device memory for gpsmi_acq_refine_dev.  Optional host arrays:
 * grid float [nhits][n_df][20] (M), prompts complex64 [nhits][3][n_ms] (P; early, prompt, late).
 * Argument errors are GPSMI_E_ARG and need no GPU (gpsmi_acq_refine_plan makes the same checks
 * without a handle); GPSMI_E_STATE: no time-domain replica for a PRN; GPSMI_E_NOMEM leaves the
 * handle usable.  The call returns when the work is done; gpsmi_acq_last_ms reports it.
 * Degenerate input: a bit whose 20 prompts are all exactly zero adds 0 to mu; all-zero iq therefore
 * gives mu = 0 and cn0_dbhz = NaN, and, the median being 0, ratio = 0 / 0 = NaN with confirmed = 0.   */
#define GPSMI_REFINE_MAX_MS 8000
typedef struct gpsmi_refine_hit {   /* no implicit padding: 16 bytes */
    int32_t prn;
    int32_t delay;                  /* 0 .. code_samples - 1 */
    double  freq_hz;
} gpsmi_refine_hit;
typedef struct gpsmi_refine_cfg {   /* no implicit padding: 48 bytes */
    int32_t n_ms;                   /* multiple of 20, >= 40 */
    int32_t tap_samples;            /* early / late spacing, >= 1; 0: 1 at 2048, 8 at 16368 */
    double  df_step_hz;             /* 0: 2 */
    double  df_half_hz;             /* 0: 120; below 500; at most 1024 grid points */
    double  carrier_hz;             /* 1575.42e6 for L1; finite, > 0 */
    double  f_offset_hz;            /* as in gpsmi_acq_search_deep; finite */
    float   min_ratio;              /* 0: 2.5 */
    int32_t reserved;               /* 0 */
} gpsmi_refine_cfg;
typedef struct gpsmi_refine_out {   /* no implicit padding: 64 bytes */
    int32_t prn;
    int32_t edge_ms;                /* e of the peak: milliseconds from the first window to the first bit boundary */
    int32_t n_bits;                 /* B */
    int32_t confirmed;              /* ratio > min_ratio */
    double  f_hz;                   /* freq_hz + df of the peak + the vertex of the parabola through
                                     * M[d - 1 .. d + 1][e] (dropped at a grid end) */
    double  code_phase;             /* delay + the vertex of the parabola through tap_metric, in samples;
                                     * -1.0 when the prompt tap is not the largest */
    float   peak;                   /* M at the peak */
    float   median;                 /* lower median of all M: rank (20 n_df - 1) / 2 from 0 */
    float   ratio;                  /* peak / median */
    float   mu;                     /* mean over the B bits of |sum P|^2 / sum |P|^2 at the peak */
    float   cn0_dbhz;               /* 10 log10(1000 (mu - 1) / (20 - mu)); NaN when mu <= 1 */
    float   tap_metric[3];          /* the bit sums of the peak's (d, e) for early, prompt, late */
} gpsmi_refine_out;
int gpsmi_acq_refine(gpsmi_acq* h, const void* iq, size_t n,
                     const gpsmi_refine_hit* hits, int nhits, const gpsmi_refine_cfg* cfg,
                     gpsmi_refine_out* out, float* grid, float* prompts);
int gpsmi_acq_refine_dev(gpsmi_acq* h, const void* d_iq, size_t n,
                         const gpsmi_refine_hit* hits, int nhits, const gpsmi_refine_cfg* cfg,
                         gpsmi_refine_out* out, float* grid, float* prompts);
/* host only, no GPU: the argument checks of gpsmi_acq_refine for a handle of code_samples, and the
 * number of grid points (n_df, optional) the grid array is sized by                            */
int gpsmi_acq_refine_plan(int code_samples, size_t n, const gpsmi_refine_hit* hits, int nhits,
                          const gpsmi_refine_cfg* cfg, int* n_df);
/* Bit-synchronous tracking of refined hits (float64 restatement: tests/wtrk_ref.py):
 * what takes a record of gpsmi_acq_refine on.  Per channel it integrates coherently over each 20-ms
 * data bit between the edges refinement found, closes a carrier loop (second-order PLL assisted by a
 * first-order FLL) and a code loop (first-order, carrier-aided DLL) once per bit, and returns one
 * record per bit and the state to go on from.  cs = code_samples, fs = 1000 cs, T = 0.020 s.
 * Positions are STREAM positions: sample iq[0] of a call has stream index cfg.first_sample, so a
 * recording is tracked in chunks by calling again with the states returned and each chunk's own
 * first_sample; nothing else is remembered between calls.
 * Windows.  For the next bit of a state (tau, f_hz, theta):
 *     Tc  = cs / (1 + (f_hz - f_offset_hz) / carrier_hz)             (the code period in samples)
 *     s_k = tau + k * Tc,  n_k = floor(s_k),  a_k = s_k - n_k         k = 0 .. 19, float64, unfused
 * The bit is tracked if min(n_0, n_19) - tap >= first_sample and max(n_0, n_19) + cs + tap <=
 * first_sample + n; otherwise the channel stops there, keeps its state for the next chunk and sets
 * GPSMI_WTRK_DATA_END in flags (cleared on entry).  A channel that fits no bit is not an error.
 * Replica.  R = GPSCacode(prn) (gpsmi_acq_set_replica_time, as gpsmi_acq_refine), interpolated
 * linearly between its samples: with the code start at n_k + a_k the replica at stream sample
 * n_k + o + i, i < cs, of the tap at offset o = -tap, 0, +tap (early, prompt, late) is
 * a_k R[(i - 1) mod cs] + (1 - a_k) R[i].  The device forms only the whole-sample float32 sums
 *     D[o][sh][k] = sum_{i < cs} x[n_k + o + i] c[n_k + o + i] R[(i - sh) mod cs],   sh = 0, 1
 * each in one fixed order; the tap value of millisecond k is a_k D[o][1][k] + (1 - a_k) D[o][0][k]
 * in float64, and E, P, L are its sums over k = 0 .. 19, H0 / H1 those of the prompt tap over k < 10
 * / k >= 10 (P = H0 + H1), all in ascending k.
 * Carrier.  c[n] = exp(-j 2 pi ph / 2^64), ph = theta + (n - floor(tau)) * inc mod 2^64 with inc =
 * f_hz / fs mod 1 in 0.64 fixed point; the top 24 bits of ph give sine and cosine, as in
 * gpsmi_acq_refine.  theta of the next bit is theta + (floor(tau') - floor(tau)) * inc: the NCO is
 * phase-continuous and the loops act on f_hz alone.
 * Update, float64, in this order, once per bit (b = bit_no before the bit):
 *     e_f = atan2(H0.re H1.im - H0.im H1.re, H0.re H1.re + H0.im H1.im) / (2 pi 0.010)         [Hz]
 *     e_p = atan(P.im / P.re) / (2 pi)   (P.re = 0: 0.25 sign(P.im))                        [cycles]
 *     e_d = (cs / 1023 - tap) (|L| - |E|) / (|E| + |L|)   (0 when |E| + |L| = 0)           [samples]
 *           e_d > 0: the late tap is the larger, the code start lies LATER than tau
 *     the PLL term is off (e_p taken as 0) while b < pull_in_bits and when pll_bw_hz < 0, the FLL
 *     term when fll_bw_hz < 0
 *     f_acc += w_p^2 T e_p + w_f T e_f          w_p = pll_bw_hz / 0.53, w_f = fll_bw_hz / 0.25
 *     f_hz'  = f_acc + 1.414 w_p e_p            (Kaplan & Hegarty ch. 5, table of loop filters;
 *     tau'   = (tau + 20 Tc) + 4 dll_bw_hz T e_d   w = B / 0.25 first order, B / 0.53 and a2 = 1.414
 *                                                  second order; plain, not bilinear, integrators)
 *     mu_ring[b mod 50] = |P|^2 / sum_k |prompt tap of k|^2 (0 for an all-zero bit); cn0_dbhz is
 *     gpsmi_acq_refine's estimator on the mean of the first min(b + 1, 50) ring entries, in index order
 *     lock  += 0.05 ((P.re^2 - P.im^2) / |P|^2 - lock)      (the term 0 when P = 0)
 * The record holds tau and f_hz as the bit USED them; the state holds tau', f_hz', theta'.
 * One workgroup per channel, no atomics, every sum in one order: a channel's records and final
 * state are the same bytes alone or among others, in any order, from complex64 or GPSMI_IQ_U8,
 * from host (gpsmi_acq_track) or device memory (gpsmi_acq_track_dev), in one call or in chunks.
 * bits is host memory [nhits][cfg.n_bits]; the records past a channel's last bit of the call are
 * zero.  nhits 1 .. 64, n_bits 1 .. 2^20; code_samples 2048 and 16368 only (GPSMI_E_UNSUPPORTED).
 * Argument errors are GPSMI_E_ARG and need no GPU (gpsmi_acq_track_plan makes the same checks without
 * a handle): among them a state whose next bit starts before the data, floor(tau) - tap <
 * first_sample.  GPSMI_E_STATE: no time-domain replica for a PRN; GPSMI_E_NOMEM leaves the handle
 * usable.  The call returns when the work is done; gpsmi_acq_last_ms reports it.                 */
#define GPSMI_WTRK_DATA_END 1u      /* flags: the channel stopped before n_bits because the data ended */
#define GPSMI_WTRK_RING 50
typedef struct gpsmi_wtrk_cfg {     /* no implicit padding: 64 bytes */
    int32_t n_bits;                 /* bits to track in this call, >= 1 */
    int32_t tap_samples;            /* early / late spacing; 0: 1 at 2048, 8 at 16368 */
    double  pll_bw_hz;              /* noise bandwidths; 0: the default (4, 1, 0.5); */
    double  fll_bw_hz;              /*   a negative pll_bw_hz / fll_bw_hz switches that term off; */
    double  dll_bw_hz;              /*   dll_bw_hz >= 0 */
    double  carrier_hz;             /* as in gpsmi_acq_refine */
    double  f_offset_hz;
    int64_t first_sample;           /* the stream index of iq[0] */
    int32_t pull_in_bits;           /* FLL-only bits of a fresh channel; 0: the default (10); < 0: none */
    int32_t reserved;               /* 0 */
} gpsmi_wtrk_cfg;
typedef struct gpsmi_wtrk_state {   /* no implicit padding: 256 bytes */
    int32_t  prn;
    int32_t  bit_no;                /* bits tracked so far */
    double   tau;                   /* stream position (samples) of the next bit's first code start */
    double   f_hz;                  /* NCO frequency of the next bit */
    uint64_t theta;                 /* carrier phase at sample floor(tau), cycles in 0.64 fixed point */
    double   f_acc;                 /* the carrier loop's integrator, Hz */
    double   lock;                  /* the phase-lock indicator, smoothed */
    uint32_t flags;                 /* GPSMI_WTRK_DATA_END */
    int32_t  reserved;              /* 0 */
    float    mu_ring[GPSMI_WTRK_RING];   /* the C/N0 estimator's last <= 50 bits */
} gpsmi_wtrk_state;
typedef struct gpsmi_wtrk_bit {     /* no implicit padding: 64 bytes */
    float   p_i, p_q;               /* P, the prompt of the bit */
    float   abs_e, abs_l;           /* |E|, |L| */
    float   h0_i, h0_q, h1_i, h1_q; /* H0, H1: the prompts of the two 10-ms halves */
    double  f_hz;                   /* as the bit used them */
    double  tau;
    float   cn0_dbhz;               /* running; NaN while the mean mu <= 1 */
    float   lock;                   /* after this bit */
    float   dll_err;                /* e_d, samples */
    int32_t bit_no;                 /* b */
} gpsmi_wtrk_bit;
int gpsmi_acq_track(gpsmi_acq* h, const void* iq, size_t n, gpsmi_wtrk_state* states, int nhits,
                    const gpsmi_wtrk_cfg* cfg, gpsmi_wtrk_bit* bits);
int gpsmi_acq_track_dev(gpsmi_acq* h, const void* d_iq, size_t n, gpsmi_wtrk_state* states, int nhits,
                        const gpsmi_wtrk_cfg* cfg, gpsmi_wtrk_bit* bits);
/* host only, no GPU: the argument checks of gpsmi_acq_track for a handle of code_samples */
int gpsmi_acq_track_plan(int code_samples, size_t n, const gpsmi_wtrk_state* states, int nhits,
                         const gpsmi_wtrk_cfg* cfg);
/* host only: a fresh channel from a record of gpsmi_acq_refine.  data_start is the stream index of
 * the first sample of the data that was refined, refine_tap_samples the tap_samples of that call (0:
 * its default).  The integer delay the hit was refined at is rint(code_phase - v), v the vertex the
 * record's tap_metric gives; as refinement does, a delay below the tap spacing counts from the next
 * code period (e = edge_ms + 1 then, else edge_ms).  tau = data_start + code_phase + e * Tc with Tc of
 * rec.f_hz as above, f_hz = f_acc = rec.f_hz, theta = 0, everything else 0.  GPSMI_E_ARG for a record
 * without a code phase (-1).                                                                    */
int gpsmi_wtrk_open(const gpsmi_refine_out* rec, int code_samples, int refine_tap_samples,
                    int64_t data_start, double carrier_hz, double f_offset_hz, gpsmi_wtrk_state* st);
/* Cancellation of strong satellites ahead of the weak searches (float64 restatement:
 * tests/cancel_ref.py): what removes the near-far problem from the samples themselves.  Each satellite
 * (prn, f_hz as gpsmi_refine_out.f_hz, tau = any of its code starts in samples from iq[0], float64) is
 * projected out code period by code period; data bits, carrier phase and amplitude are absorbed per
 * period, so there is no loop and nothing is remembered.  cs = code_samples, fs = 1000 cs.
 * Windows.  Tc = cs / (1 + (f_hz - f_offset_hz) / carrier_hz) as in gpsmi_acq_track; window k holds the
 * samples ceil(tau + k Tc) <= i < ceil(tau + (k + 1) Tc) cut to [0, n) (float64, unfused, on the host),
 * for every k that leaves one: the first and the last are partial, the others have cs - 1 .. cs + 1.
 * Basis.  With j = rint(tau + k Tc) (ties to even) and R = GPSCacode(prn) (gpsmi_acq_set_replica_time)
 *     b_d[i] = R[(i - j - d) mod cs] exp(+j 2 pi f_hz (i + 1) / fs),    d = -1, 0, +1
 * (the i + 1 is SEC_TIME's; the phase is the integer (i + 1) * (f_hz / fs in 0.64 fixed point) mod
 * 2^64, exact at any index, its top 24 bits give sine and cosine as in gpsmi_acq_refine).  Three
 * whole-sample shifts span every code phase within half a sample of the estimate (exactly for a
 * linearly interpolated replica; a short channel estimate otherwise).
 * Projection.  G = B^H B (real, symmetric: six float32 sums), p = B^H x (three complex float32 sums),
 * each sum in one fixed order; G c = p is solved in float64 (L D L^T, no permutation) and the window
 * becomes x - B c in float32.  A window of fewer than min_window samples, or one whose smallest pivot
 * is below 1e-6 trace(G), passes through bit for bit and is counted in n_skipped.
 * Satellites are cancelled one after another in the order given (pass the strongest first), each on
 * the output of the one before.  nsat 0 .. 32; nsat = 0 only decodes or copies.
 * iq: n samples in the handle's input format, host memory for gpsmi_acq_cancel, device memory for
 * gpsmi_acq_cancel_dev.  The output is complex64 [n] (host / device alike); GPSMI_IQ_U8 input is first
 * decoded with gpsmi_dev_unpack_u8iq's arithmetic, complex64 input is copied -- or, for
 * gpsmi_acq_cancel_dev with d_out_c64 == d_iq, cancelled in place.  Input and output that overlap
 * without being that one complex64 buffer are refused.  Samples outside the processed windows are
 * the decoded / copied input, bit for bit.
 * out [nsat]: energy_in = sum |x|^2 over the processed windows (as the satellite met them),
 * energy_removed = sum c^H G c; the windows' float64 figures are added in window order on the host.
 * coef: optional host array complex64 [nsat][max_windows][3] (taps d = -1, 0, +1; max_windows from
 * gpsmi_acq_cancel_plan), zeros for skipped windows and past a satellite's last one.
 * The same arguments give the same bytes, from either entry point.  Argument errors are GPSMI_E_ARG
 * and need no GPU (gpsmi_acq_cancel_plan makes the same checks without a handle): nsat, a PRN outside
 * 1 .. 37 or given twice, f_hz or tau not finite, |f_hz| >= fs / 2, (f_hz - f_offset_hz) beyond 1 % of
 * carrier_hz, n outside 1 .. 2^40.  code_samples 2048 and 16368 only (GPSMI_E_UNSUPPORTED);
 * GPSMI_E_STATE: no time-domain replica for a PRN; GPSMI_E_NOMEM leaves the handle usable.  cfg may be
 * null (all defaults).  The call returns when the work is done; gpsmi_acq_last_ms reports it.     */
typedef struct gpsmi_cancel_sat {   /* no implicit padding: 24 bytes */
    int32_t prn;
    int32_t reserved;               /* 0 */
    double  f_hz;
    double  tau;                    /* a code start, samples from iq[0]; any sign */
} gpsmi_cancel_sat;
typedef struct gpsmi_cancel_cfg {   /* no implicit padding: 24 bytes; 0 = the default */
    double  carrier_hz;             /* 0: 1575.42e6 */
    double  f_offset_hz;            /* as in gpsmi_acq_search_deep; finite */
    int32_t min_window;             /* 0: 16 */
    int32_t reserved;               /* 0 */
} gpsmi_cancel_cfg;
typedef struct gpsmi_cancel_out {   /* no implicit padding: 32 bytes */
    int32_t prn;
    int32_t n_windows;              /* windows that hold a sample of iq */
    int32_t n_skipped;              /* ... of which passed through */
    int32_t reserved;               /* 0 */
    double  energy_in;
    double  energy_removed;
} gpsmi_cancel_out;
int gpsmi_acq_cancel(gpsmi_acq* h, const void* iq, size_t n, const gpsmi_cancel_sat* sats, int nsat,
                     const gpsmi_cancel_cfg* cfg, float* out_c64, gpsmi_cancel_out* out, float* coef);
int gpsmi_acq_cancel_dev(gpsmi_acq* h, const void* d_iq, size_t n, const gpsmi_cancel_sat* sats, int nsat,
                         const gpsmi_cancel_cfg* cfg, void* d_out_c64, gpsmi_cancel_out* out, float* coef);
/* host only, no GPU: the argument checks of gpsmi_acq_cancel for a handle of code_samples, and the
 * largest number of windows of any satellite (max_windows, optional) the coef array is sized by  */
int gpsmi_acq_cancel_plan(int code_samples, size_t n, const gpsmi_cancel_sat* sats, int nsat,
                          const gpsmi_cancel_cfg* cfg, int* max_windows);
/* Spatial signatures of refined records over several coherent antennas (float64
 * restatement: tests/sig_ref.py): what tells signals that arrive from one direction -- a spoofer sends
 * every PRN from one antenna -- from satellites all over the sky.  Per record (prn, f_hz, tau, with the
 * meaning of gpsmi_cancel_sat; the same PRN may appear more than once: twin records are the point) the
 * 1-ms prompts of every antenna and their covariance over the antennas; the principal eigenvector of
 * that matrix is the record's signature (host: gpsmi/snapshot.py).  cs = code_samples, fs = 1000 cs.
 * iq: `antennas` rows of n samples each ([A][n], row a = antenna a, antenna 0 first: the layout of
 * gpsmi_nul_apply) in the handle's input format, host memory for gpsmi_acq_signature, device memory for
 * gpsmi_acq_signature_dev; GPSMI_IQ_U8 gives the same bytes as its complex64 decode.  A = 2 .. 8,
 * nsat = 1 .. 64.
 * Windows.  Tc = cs / (1 + (f_hz - f_offset_hz) / carrier_hz) and j_k = rint(tau + k Tc) (float64,
 * unfused, ties to even, on the host) as in gpsmi_acq_cancel; a record's windows are all k with
 * 0 <= j_k and j_k + cs <= n, in order, of which a positive n_ms keeps the first n_ms.  A record
 * without a window is GPSMI_E_ARG.
 * Prompts.  P[r][a][k] = sum_{i < cs} x_a[j_k + i] exp(-j 2 pi f_hz (j_k + i + 1) / fs) R[i] with
 * R = GPSCacode(prn) (gpsmi_acq_set_replica_time) and the integer carrier phase of gpsmi_acq_cancel
 * (0.64 fixed point, its top 24 bits give sine and cosine).  float32 sums in one fixed order that is the
 * same for every antenna and depends neither on A nor on nsat nor on what else shares the call.
 * Covariance.  C[r][a][b] = sum_k P[r][a][k] conj(P[r][b][k]): float64 sums of the widened float32
 * prompts in one fixed order over k; the upper triangle is computed, the lower one is its exact
 * conjugate, the diagonal's imaginary part is exactly 0.  A factor common to the antennas of a window
 * drops out -- the data bit, the residual carrier phase, a Doppler error of a few Hz -- so there is no
 * bit edge and no loop.
 * Outputs (host arrays): cov double [nsat][A][A][2]; n_win int32 [nsat]; prompts: optional complex64
 * [nsat][A][max_windows] (max_windows from gpsmi_acq_signature_plan), zero past a record's last window.
 * A record's result depends on that record alone.  The same arguments give the same bytes, from
 * either entry point.  Argument errors are GPSMI_E_ARG and need no GPU (gpsmi_acq_signature_plan makes
 * the same checks without a handle): a null pointer, antennas outside 2 .. 8, nsat, a PRN outside
 * 1 .. 37, f_hz or tau not finite, |f_hz| >= fs / 2, (f_hz - f_offset_hz) beyond 1 % of carrier_hz,
 * n outside 1 .. 2^40 / A, a reserved field that is not 0.  code_samples 2048 and 16368 only
 * (GPSMI_E_UNSUPPORTED); GPSMI_E_STATE: no time-domain replica for a PRN; GPSMI_E_NOMEM leaves the
 * handle usable.  cfg may be null (all defaults).  The call returns when the work is done;
 * gpsmi_acq_last_ms reports it.                                                                  */
typedef struct gpsmi_sig_sat {      /* no implicit padding: 24 bytes */
    int32_t prn;
    int32_t reserved;               /* 0 */
    double  f_hz;
    double  tau;                    /* a code start, samples from iq[0] of every row; any sign */
} gpsmi_sig_sat;
typedef struct gpsmi_sig_cfg {      /* no implicit padding: 24 bytes; 0 = the default */
    int32_t antennas;               /* 0: 2 */
    int32_t n_ms;                   /* 0: every window that fits */
    double  carrier_hz;             /* 0: 1575.42e6 */
    double  f_offset_hz;            /* as in gpsmi_acq_search_deep; finite */
} gpsmi_sig_cfg;
int gpsmi_acq_signature(gpsmi_acq* h, const void* iq, size_t n, const gpsmi_sig_sat* sats, int nsat,
                        const gpsmi_sig_cfg* cfg, double* cov, int32_t* n_win, float* prompts);
int gpsmi_acq_signature_dev(gpsmi_acq* h, const void* d_iq, size_t n, const gpsmi_sig_sat* sats, int nsat,
                            const gpsmi_sig_cfg* cfg, double* cov, int32_t* n_win, float* prompts);
/* host only, no GPU: the argument checks of gpsmi_acq_signature for a handle of code_samples, the
 * windows of every record (n_win [nsat], optional) and the largest of them (max_windows, optional)
 * the prompts array is sized by  */
int gpsmi_acq_signature_plan(int code_samples, size_t n, const gpsmi_sig_sat* sats, int nsat,
                             const gpsmi_sig_cfg* cfg, int32_t* n_win, int* max_windows);
/* Multi-tap correlation profiles of refined records on one antenna (float64
 * restatement: tests/profile_ref.py): what shows a second copy of a code within two chips of the first
 * -- a spoofer lifting off, or multipath -- where gpsmi_acq_peaks sees one peak.  Per record (prn, f_hz,
 * tau as gpsmi_sig_sat; the same PRN may appear more than once) the complex correlation at every
 * whole-sample lag l = -Lh .. +Lh around the code start, per 1-ms window, summed coherently over runs of
 * coh_ms windows (a data bit from its edge: skip_ms), and the covariance of those sums over the taps;
 * whether one code replica explains that matrix is decided on the host (gpsmi/snapshot.py,
 * profile_fit).  cs = code_samples, fs = 1000 cs, K = 2 Lh + 1.
 * iq: n samples in the handle's input format, host memory for gpsmi_acq_profile, device memory for
 * gpsmi_acq_profile_dev; GPSMI_IQ_U8 gives the same bytes as its complex64 decode.  nsat = 1 .. 64.
 * Windows.  Tc and j_k = rint(tau + k Tc) exactly as in gpsmi_acq_signature; a record's windows are all
 * k with j_k - Lh >= 0 and j_k + Lh + cs <= n, in order; the first skip_ms of them are dropped, the rest
 * are cut into runs of coh_ms consecutive windows, an incomplete last run is dropped, and a positive
 * n_runs keeps the first n_runs.  A record without a run is GPSMI_E_ARG.
 * Taps.  w[u] = x[u] exp(-j 2 pi f_hz (u + 1) / fs) with the integer carrier phase of gpsmi_acq_cancel
 * at the absolute sample index u (0.64 fixed point, its top 24 bits give sine s and cosine c):
 * Re w = fma(Re x, c, Im x * s), Im w = fma(Im x, c, -(Re x * s)) in float32 -- one value for all taps.
 * D[r][l][k] = sum_{i < cs} w[j_k + l + i] R[i], R = GPSCacode(prn) (gpsmi_acq_set_replica_time), in
 * float32 in this order: lane q = 0 .. 63 adds, by fused multiply-adds from 0, the points i with
 * (i mod 256) div 4 = q in ascending i; the 64 lane sums are folded by a butterfly (lane q takes
 * v[q] + v[q xor 32], then xor 16, 8, 4, 2, 1).  S[r][l][m] = the D[r][l][.] of run m's coh_ms windows
 * added in float32 in ascending order from the first, stored as complex64.  None of it depends on nsat,
 * on the record's place in the call, on half_taps or on what else shares the call.
 * Covariance.  Q[r][l][l'] = sum_m S[r][l][m] conj(S[r][l'][m]): float64 sums of the widened complex64
 * values in ascending m; the upper triangle is computed, the lower one is its exact conjugate, the
 * diagonal's imaginary part is exactly 0.
 * Outputs (host arrays): cov double [nsat][K][K][2]; n_runs int32 [nsat]; sums: optional complex64
 * [nsat][K][max_runs] (max_runs from gpsmi_acq_profile_plan), zero past a record's last run.
 * A record's result depends on that record alone.  The same arguments give the same bytes, from either
 * entry point.  Argument errors are GPSMI_E_ARG and need no GPU (gpsmi_acq_profile_plan makes the same
 * checks without a handle): a null pointer, nsat, a PRN outside 1 .. 37, skip_ms outside 0 .. 19, f_hz
 * or tau not finite, |f_hz| >= fs / 2, (f_hz - f_offset_hz) beyond 1 % of carrier_hz, half_taps outside
 * 0 .. 32, coh_ms outside 0 .. 20, n_runs < 0, a reserved field that is not 0, carrier_hz or f_offset_hz
 * not finite, n outside 1 .. 2^40, a record without a run.  code_samples 2048 and 16368 only
 * (GPSMI_E_UNSUPPORTED); GPSMI_E_STATE: no time-domain replica for a PRN; GPSMI_E_NOMEM leaves the
 * handle usable.  cfg may be null (all defaults).  The call returns when the work is done;
 * gpsmi_acq_last_ms reports it.                                                                  */
typedef struct gpsmi_prof_sat {     /* no implicit padding: 24 bytes */
    int32_t prn;
    int32_t skip_ms;                /* windows dropped before the first run: the bit edge, 0 .. 19 */
    double  f_hz;                   /* as gpsmi_sig_sat */
    double  tau;                    /* a code start, samples from iq[0]; any sign */
} gpsmi_prof_sat;
typedef struct gpsmi_prof_cfg {     /* no implicit padding: 32 bytes; 0 = the default */
    int32_t half_taps;              /* Lh, 1 .. 32; 0: 8 at 2048, 32 at 16368 (+-4 / +-2 chips) */
    int32_t coh_ms;                 /* windows summed coherently per run, 1 .. 20; 0: 20 */
    int32_t n_runs;                 /* 0: every run that fits */
    int32_t reserved;               /* 0 */
    double  carrier_hz;             /* 0: 1575.42e6 */
    double  f_offset_hz;            /* as in gpsmi_acq_search_deep; finite */
} gpsmi_prof_cfg;
int gpsmi_acq_profile(gpsmi_acq* h, const void* iq, size_t n, const gpsmi_prof_sat* sats, int nsat,
                      const gpsmi_prof_cfg* cfg, double* cov, int32_t* n_runs, float* sums);
int gpsmi_acq_profile_dev(gpsmi_acq* h, const void* d_iq, size_t n, const gpsmi_prof_sat* sats, int nsat,
                          const gpsmi_prof_cfg* cfg, double* cov, int32_t* n_runs, float* sums);
/* host only, no GPU: the argument checks of gpsmi_acq_profile for a handle of code_samples, the runs
 * of every record (n_runs [nsat], optional), the largest of them (max_runs, optional) the sums array
 * is sized by, and the taps K = 2 Lh + 1 (taps, optional)  */
int gpsmi_acq_profile_plan(int code_samples, size_t n, const gpsmi_prof_sat* sats, int nsat,
                           const gpsmi_prof_cfg* cfg, int32_t* n_runs, int* max_runs, int* taps);
/* Input format of the iq pointers of the search calls that follow (host or device), as
 * gpsmi_trk_set_input_format below: GPSMI_IQ_U8 = the raw recording of streamData
 * (gpsrecv.py:162-173), decoded where the carrier wipe-off reads it; same bits out.   */
int gpsmi_acq_set_input_format(gpsmi_acq* h, int fmt);
/* Timing of the last search on the handle's stream (HIP events), ms.          */
int gpsmi_acq_last_ms(gpsmi_acq* h, float* ms);

/* ========================================================================
 * Tracking -- replaces the numeric part of gpslib.SatStream.process
 * (gpslib.py:1141-1210) for all channels of one device in one call:
 * demodDoppler (:1343-1346), cacodeCorr (:1315-1327), findCodePhase and
 * fitCodePhase (:1293-1304, :1268-1290), decodeData's integrate-and-dump
 * (:1400-1420, :1439-1440), the amplitude statistics (:1186-1188) and
 * phaseLockedLoop (:1215-1262) with the state update (:1205-1208).
 * The per-SV worker processes of gpsrecv.runProc (gpsrecv.py:300-337)
 * collapse into channels of one handle.
 * ======================================================================== */
typedef struct gpsmi_trk gpsmi_trk;

/* Loop-carried state of one channel (SatStream.__init__, gpslib.py:1050-1091).
 * freq and phase are float32 because they are float32 in the reference under
 * numpy >= 2.                                                  */
typedef struct gpsmi_trk_state {
    int32_t prn;             /* SAT_NO; 0 = channel closed                     */
    int32_t delay;           /* DELAY                                          */
    float   freq;            /* FREQ, Hz                                       */
    float   phase;           /* PHASE, rad                                     */
    int32_t phase_locked;    /* PHASE_LOCKED                                   */
    int32_t nps;             /* len(PREV_SAMPLES)                              */
    float   prev_sum_re;     /* sum(PREV_SAMPLES): the carry is only ever used */
    float   prev_sum_im;     /*   inside the first window's mean (:1405-1419)  */
    int32_t df_len;          /* len(DF)                                        */
    float   omega0;          /* 2*pi*FREQ while FREQ is still a Python float    */
                             /*   (after initInst or a clamp): float32 of the   */
                             /*   float64 product.  0 = FREQ is float32 and the */
                             /*   factor is float32(2*pi)*FREQ (NEP 50)         */
    float   df[GPSMI_MAX_DF];/* DF, oldest first                               */
    /* decodeData's edge scan (gpslib.py:1394-1398, :1421-1436), carried on the device   */
    int32_t edge_state;      /* 0: EDGES[0] not set yet; +1 / -1: prevSign; 2: prevSign */
                             /*   is 0 (np.sign of an exact zero): no further edge until */
                             /*   erasePrevData.  A deviation: the reference re-derives  */
                             /*   prevSign at the start of every decodeData call, so it  */
                             /*   finds edges again from the next block on.  Reachable   */
                             /*   only when a dump's real part is exactly 0.             */
    float   prev_signal;     /* PREV_SIGNAL (:1434), the real part of the last dump      */
    float   std_dev;         /* STD_DEV before the block: MIN_EDGE_AMP = 3*STD_DEV       */
    int32_t reserved;        /* 0                                                        */
} gpsmi_trk_state;

/* Everything SatStream.process and its callers read back for one block.       */
typedef struct gpsmi_trk_out {
    int32_t prn;
    int32_t n_dumps;                     /* len(gpsData), N_CYC or N_CYC+1      */
    float   dumps[2 * GPSMI_MAX_DUMPS];  /* gpsData, complex64 (:1439)          */
    int32_t first_len;                   /* samples in the first window         */
    int32_t mx;                          /* argmax of corr                      */
    float   epl[3];                      /* corr[mx-1], corr[mx], corr[mx+1]    */
    float   corr_mean, corr_std;
    float   norm_max_corr;               /* MAX_CORR (:1188)                    */
    int32_t delay;                       /* findCodePhase delay, -1 below CORR_MIN */
    int32_t reserved0;                   /* 0 (keeps code_phase 8-aligned)      */
    double  code_phase;                  /* fitCodePhase, -1.0 below CORR_MIN   */
    int32_t delay_used;                  /* DELAY after the block (:1181-1182)  */
    float   std_dev, amplitude;          /* STD_DEV, AMPLITUDE (:1186-1187)     */
    float   df, phase_shift;             /* PLL outputs (:1205-1206)            */
    float   freq, phase;                 /* FREQ, PHASE after the block         */
    int32_t phase_locked;                /* PHASE_LOCKED after the block        */
    int32_t nps;                         /* len(PREV_SAMPLES) after the block   */
    /* decodeData's edge list for this block (gpslib.py:1421-1436): bit i of the mask =  */
    /* dump i appended an edge (MS_TIME before the block + i, ST + n0 of window i)       */
    uint32_t edge_mask;                  /* dumps 0..31                         */
    uint32_t edge_mask_hi;               /* bit 0: dump 32                      */
    int32_t edge_sign0;                  /* the sign this block stored into EDGES[0]  */
                                         /*   (first locked dump after a reset), else 0 */
    int32_t ms_count;                    /* dumps counted into MS_TIME: n_dumps while  */
                                         /*   PHASE_LOCKED was set before the block, else 0 */
    int32_t reserved1;                   /* 0 (no implicit tail padding)        */
} gpsmi_trk_out;

int gpsmi_trk_create(const gpsmi_cfg* cfg, int max_ch, gpsmi_trk** out);
int gpsmi_trk_destroy(gpsmi_trk* h);
/* GPSCacode(prn) as float32 [code_samples] and its spectrum, complex64 (the
 * spectrum is used, and required, only when code_samples == 2048).            */
int gpsmi_trk_set_replica(gpsmi_trk* h, int prn, const float* replica_f32,
                          const float* spectrum_c64);
/* ('initInst',(satNo,freq,delay)) of gpsrecv.py:312-321.                      */
int gpsmi_trk_open(gpsmi_trk* h, int ch, int prn, float freq_hz, int delay);
/* ('delInst',None) of gpsrecv.py:323-328.                                     */
int gpsmi_trk_close(gpsmi_trk* h, int ch);
int gpsmi_trk_get_state(gpsmi_trk* h, int ch, gpsmi_trk_state* st);
int gpsmi_trk_set_state(gpsmi_trk* h, int ch, const gpsmi_trk_state* st);
/* erasePrevData / setPhaseUnlocked (gpslib.py:1095-1107) for one channel.     */
int gpsmi_trk_erase_prev(gpsmi_trk* h, int ch);

/* ('runInst',(data,smpTime)) for every open channel (gpsrecv.py:330-334,
 * :404-417): one closed-loop block.  iq: host complex64 [NGPS].  out[ch] is
 * written for open channels, out[ch].prn = 0 for closed ones.                 */
int gpsmi_trk_process(gpsmi_trk* h, const float* iq, size_t n,
                      gpsmi_trk_out* out);
/* Same on a block that is already in device memory.  out may be NULL when the
 * caller only wants the state to advance (read it later with get_state); with
 * the timing events off as well (gpsmi_trk_set_timing) the call returns as soon
 * as the block is enqueued and consecutive blocks run back to back.            */
int gpsmi_trk_process_dev(gpsmi_trk* h, const void* d_iq, size_t n,
                          gpsmi_trk_out* out);

/* The same for a stream that arrives in host memory, without a host wait per block: the block
 * (page-locked memory from gpsmi_host_alloc for a full-rate, truly asynchronous copy; n and the
 * format as for gpsmi_trk_process) is uploaded into one of two staging blocks and the kernels are
 * enqueued behind the upload, so the call returns without waiting for its own step and the host
 * runs up to two steps ahead of the device; steps of more than 8 MiB upload on a stream of their
 * own under the kernels of the step before (GPSMI_STREAM_INLINE_MAX moves that size).  A call
 * returns once the step of the call BEFORE LAST has finished: from then on that step's iq may be
 * rewritten and its out (optional, page-locked) is filled; gpsmi_trk_wait finishes all of them.  This is
 * streamData -> pushToBuffer -> processData (gpsrecv.py:153-186, :76-104, :445-548) with the ring
 * buffer's consumer on the GPU.                                                        */
int gpsmi_trk_process_stream(gpsmi_trk* h, const void* iq, size_t n, gpsmi_trk_out* out);

/* Batched receivers: R independent IQ streams (receivers) tracked by one handle, so that the
 * closed loop -- a chain of three dependent launches per 32-ms block -- fills the GPU with the
 * jobs of R x max_ch channels instead of max_ch.  After the call the handle has R * max_ch state
 * rows, all closed; the channel index of open / close / get_state / set_state / erase_prev is
 * stream * max_ch + ch, process / process_dev take R blocks back to back (n = R * NGPS; stream r
 * reads block r) and write out[R * max_ch].  Every stream computes exactly what it computes alone
 * on a handle of its own (SatStream.process, gpslib.py:1141-1210, once per stream and channel).
 * Replay keeps to one stream.                                                          */
int gpsmi_trk_set_streams(gpsmi_trk* h, int n_streams);

/* Input format of the blocks that process / process_dev / replay* receive (default
 * GPSMI_IQ_C64).  GPSMI_IQ_U8: the raw recording format of streamData (gpsrecv.py:162-173),
 * uint16 (Q << 8 | I) per sample, 2 bytes instead of 8 over PCIe and from HBM; the kernels
 * that read IQ decode on load, bit for bit what gpsmi_dev_unpack_u8iq writes, so every
 * output equals the complex64 path's.  CODE_SAMPLES = 2048 with the span correlator only
 * (N_CYC = 32, 16 or 8; GPSMI_E_UNSUPPORTED otherwise); block sizes are still counted in
 * samples.                                                                             */
int gpsmi_trk_set_input_format(gpsmi_trk* h, int fmt);

/* Replay (open loop): nb blocks resident in device memory, the state at the
 * START of every block supplied as a table [nb][nch] (one row per block, one
 * column per open channel in channel order), all blocks processed in one batch.
 * delay_used[nb][nch] is the DELAY each block decodes with (the closed loop
 * derives it from the same block's correlation; in replay it comes from the
 * recorded trajectory and the kernel's own result is returned for comparison).
 * out is [nb][nch].  Running the closed loop and replaying its recorded
 * trajectory give the same outputs.                                           */
int gpsmi_trk_replay(gpsmi_trk* h, const void* d_iq, int nb,
                     const gpsmi_trk_state* table, const int32_t* delay_used,
                     gpsmi_trk_out* out);
/* The same in three steps, so that a caller can keep the table resident and
 * time the device work alone: load uploads table (+ delay_used, may be NULL),
 * run launches the kernels on nb device-resident blocks and waits for them,
 * fetch downloads the [nb][nch] output records (out may be pinned memory from
 * gpsmi_host_alloc for a full-rate copy).                                     */
int gpsmi_trk_replay_load(gpsmi_trk* h, int nb, const gpsmi_trk_state* table,
                          const int32_t* delay_used);
int gpsmi_trk_replay_run(gpsmi_trk* h, const void* d_iq, int nb);
int gpsmi_trk_replay_fetch(gpsmi_trk* h, gpsmi_trk_out* out, size_t n);
/* Non-blocking run / fetch and the matching waits.  The read-back runs on a copy
 * stream of its own from one of two result slots, so run k+1 overlaps the copy of
 * run k: run_async, fetch_async(out_k), wait_prev (= run k-1 and its copy are
 * done, gpsmi_trk_last_ms reports run k-1), ... , wait (everything is done).  out
 * must be page-locked and stay valid until the wait that covers it; at most two
 * runs may be outstanding.  The state table is shared by the runs in flight:
 * gpsmi_trk_replay_load first waits for every outstanding run (and its read-back),
 * so load(k+1) after run_async(k) is safe, and costs that wait.                 */
int gpsmi_trk_replay_run_async(gpsmi_trk* h, const void* d_iq, int nb);
int gpsmi_trk_replay_fetch_async(gpsmi_trk* h, gpsmi_trk_out* out, size_t n);
int gpsmi_trk_wait(gpsmi_trk* h);
int gpsmi_trk_wait_prev(gpsmi_trk* h);
/* Device-side ordering between an acquisition and a tracking handle, no host wait:
 * what is enqueued on `later` after the call starts when everything enqueued on
 * `earlier` so far has finished (a search between two tracking batches without the
 * kernels of the two competing for the CUs).  Of an asynchronous replay batch that is its
 * correlators: its epilogue and read-back run on streams of their own, beside what
 * follows.                                                                        */
int gpsmi_trk_after_acq(gpsmi_trk* later, gpsmi_acq* earlier);
int gpsmi_acq_after_trk(gpsmi_acq* later, gpsmi_trk* earlier);
/* State at the END of every job of the last replay, [nb][nch]: equals the next
 * row of the table when the table is a closed-loop trajectory.               */
int gpsmi_trk_replay_states(gpsmi_trk* h, gpsmi_trk_state* states, size_t n);
/* Device time of the last process/replay call (HIP events on the handle's
 * stream), total and for the correlator kernel alone, ms.                     */
/* Kernel-timing events around the launches that follow (default on = 1).  Each of the four
 * event records is a barrier packet in the queue, ~5 us of pipeline bubble: a caller
 * that does not read gpsmi_trk_last_ms switches them off (0), a benchmark samples.  on = 2:
 * only the begin / end stamps of the batch correlator's own dispatch are taken (no packet in
 * the queue: free), gpsmi_trk_last_ms then updates correlator_ms alone.                  */
int gpsmi_trk_set_timing(gpsmi_trk* h, int on);
/* Options of one handle (keys: the table at gpsmi_set_default).  get reports what is in effect --
 * for "correlator" / "codephase" the variant the handle actually runs.                  */
int gpsmi_trk_set_option(gpsmi_trk* h, const char* key, long long value);
int gpsmi_trk_get_option(gpsmi_trk* h, const char* key, long long* value);
/* Introspection for tests (no GPU needed): grid size of the code-phase correlation launch over
 * nblocks blocks x ngroups channel groups (negative: error), and the (block, group) workgroup wg
 * of that launch serves -- block >= nblocks for a padding workgroup.  In batches the groups of a
 * block are consecutive slots of ONE XCD (workgroup w runs on XCD w % 8): they share the block's
 * rows through that XCD's L2 (csrc/gpsmi_wgmap.h).                                        */
int gpsmi_trk_corr_grid(int nblocks, int ngroups);
int gpsmi_trk_corr_wg_map(int nblocks, int ngroups, int wg, int* block, int* group);
int gpsmi_trk_last_ms(gpsmi_trk* h, float* total_ms, float* correlator_ms);
/* ... and from the start of the call's device work to the start of its correlator: the
 * code-phase correlation (cacodeCorr, gpslib.py:1315-1327) with everything in front of it.  */
int gpsmi_trk_last_codephase_ms(gpsmi_trk* h, float* ms);

/* ========================================================================
 * Narrowband interference excision: an opt-in input filter ahead of acquisition and tracking
 * (DESIGN.md 4.2b).  A continuous-wave tone some 30 dB above the noise defeats the C/A code's
 * processing gain; this finds such tones in the spectrum of each block and removes their bins.
 * One block of block_samples complex samples (a multiple of 1024, >= 4096: CODE_SAMPLES 2048 at
 * N_CYC 32 / 16 / 8; anything else, the 16368-sample configs among them, is GPSMI_E_UNSUPPORTED)
 * is cut into frames of 2048 samples at hop 1024, frame m covering block samples
 * [1024 m - 1024, 1024 m + 1024); frame 0 starts in the carry, the previous block's last 1024
 * input samples (zero after create / reset).  Window: periodic Hann sin^2(pi i / 2048), except
 * the last frame, whose second half is weighted 1, so that the frames sum to 1 everywhere and
 * output block k depends on input blocks k - 1 and k only (no latency, same sample bookkeeping).
 * Detection: P[k] = mean over frames 0 .. n/1024 - 2 of |FFT(w x_m)|^2; a bin is flagged when
 * P[k] > median(P) * 10^(thresh_db / 10) (median: the mean of the two middle values), then widened
 * by +-dilate bins circularly.  More than max_bins flagged bins: wideband interference, the block
 * passes through unchanged (bit for bit), its count is -1 and its mask empty.  Otherwise every frame
 * is transformed, the flagged bins zeroed, transformed back and overlap-added; out is complex64.
 * Every sum has a fixed order: the bits do not depend on nb or on the run.
 * counts: int32 [nb] (flagged bins, -1 wideband); masks: uint32 [nb * 64], bin k of block b in
 * bit k % 32 of masks[b * 64 + k / 32] (the bins removed).  Both optional host arrays.
 * nb consecutive blocks in order: block b's carry is block b - 1's tail (the handle's carry for
 * b = 0), and the handle's carry is the last block's tail afterwards.  Input and output must not
 * overlap (GPSMI_E_ARG: no in-place excision).  Both calls return when the work is done;
 * gpsmi_ifx_last_ms reports its device time.  thresh_db = +inf flags nothing.
 * The first block after create / reset stands behind a zero carry: a strong tone then starts with a
 * step at sample 0, which leaks across frame 0's spectrum.  A short block (4096 or 5120 samples:
 * 3 or 4 frames in P) is classed wideband by it and passes through jammed (count -1); a longer one
 * is excised with a wider mask than its successors (35 dB tone: some 170 bins at 20480, some 95
 * at 65536).
 * gpsmi_ifx_last_psd (a diagnostic) copies out the float32 P[k] that the last call thresholded,
 * bit for bit: psd is a host array of nb * 2048 floats, nb that call's; GPSMI_E_STATE before the
 * first call.
 * ======================================================================== */
typedef struct gpsmi_ifx gpsmi_ifx;
typedef struct gpsmi_ifx_cfg {
    int32_t block_samples;   /* n, multiple of 1024, >= 4096               */
    float   thresh_db;       /* 6.0 (not NaN)                              */
    int32_t dilate;          /* 2 (0 .. 64)                                */
    int32_t max_bins;        /* 256 (0 .. 2048)                            */
    int32_t device;
} gpsmi_ifx_cfg;
int gpsmi_ifx_create(const gpsmi_ifx_cfg* cfg, gpsmi_ifx** out);
int gpsmi_ifx_destroy(gpsmi_ifx* h);
/* GPSMI_IQ_C64 (default) or GPSMI_IQ_U8 (the recorder's uint16, decoded on load) */
int gpsmi_ifx_set_input_format(gpsmi_ifx* h, int fmt);
int gpsmi_ifx_reset(gpsmi_ifx* h);                            /* carry := 0 */
/* host iq (nb * n samples in the input format) -> host out (complex64 [nb * n])               */
int gpsmi_ifx_apply(gpsmi_ifx* h, const void* iq, float* out, int nb,
                    int32_t* counts, uint32_t* masks);
/* the same from device memory to device memory                                                */
int gpsmi_ifx_apply_dev(gpsmi_ifx* h, const void* d_iq, void* d_out, int nb,
                        int32_t* counts, uint32_t* masks);
int gpsmi_ifx_last_ms(gpsmi_ifx* h, float* ms);
int gpsmi_ifx_last_psd(gpsmi_ifx* h, float* psd);

/* ========================================================================
 * Front end: recordings of other SDR front ends -> complex64 at the engine's rate.
 * A streaming stage ahead of acquisition, excision and tracking: decode the samples, mix the IF
 * or tuner offset to 0 Hz, band-limit and resample from fs_in to fs_out (whole Hz, fs_in / fs_out
 * in 0.5 .. 64); the output is complex64 at fs_out (1000 * CODE_SAMPLES for the engines).
 * Decode: GPSMI_FE_C64 complex64; GPSMI_FE_U8IQ the recorder's uint16 (Q << 8 | I), the arithmetic
 * of gpsmi_dev_unpack_u8iq; GPSMI_FE_SC8 int8 I, Q / 128; GPSMI_FE_SC16 int16 little-endian I, Q
 * / 32768; GPSMI_FE_R8 real int8 / 128, times 2 (a cosine of amplitude A at IF + f becomes a
 * complex tone of amplitude A at f).  flags GPSMI_FE_CONJUGATE mirrors complex input.
 * Mix: x[i] exp(-j 2 pi if_hz i / fs_in), i the absolute input index since create / reset; the
 * phase is i * inc mod 2^64 in integers (inc = if_hz / fs_in in 0.64 fixed point), its top 24 bits
 * give the sine and cosine: exact at any offset, whatever the cut of the input into calls.
 * Resample: output n is the band-limited input at t_n = n fs_in / fs_out input samples, kept as
 * exact integers (no drift); the filter is centred on t_n (no group delay: output n and a scene
 * rendered at fs_out share one time base); input before index 0 is zero.  Filter: a Kaiser-windowed
 * sinc designed in double at create time, K taps, tabulated at L phases per input sample (table
 * [(L + 1) * K], row j = h(j / L + K/2 - 1 - m)), the two rows around t_n's fraction combined
 * linearly.  Passband |f| <= passband_hz (0: 0.44 min(fs_in, fs_out)), ripple <= 0.1 dB; anything
 * that aliases (or, real input, images) into the passband is attenuated by >= atten_db (0: 60).
 * A configuration that cannot meet this is GPSMI_E_UNSUPPORTED with the reason in
 * gpsmi_last_error (e.g. the real-input image inside the passband: pass a narrower passband_hz).
 * push emits every output whose filter support (floor(t_n) - K/2 + 1 .. floor(t_n) + K/2) is in,
 * so the outputs over a sequence of calls depend only on the total input; a call that would emit
 * more than max_out is GPSMI_E_ARG and changes nothing.  flush takes zeros past the end and emits
 * the outputs up to the last input sample; push / flush after it are GPSMI_E_ARG until reset.
 * Every output is one fixed-order sum computed by one thread (no atomics): the bits do not depend
 * on the cut of the input, the batch size or the run.  The calls return when the work is done;
 * gpsmi_fe_last_ms reports the device time of the last one.
 * ======================================================================== */
#define GPSMI_FE_C64       0
#define GPSMI_FE_U8IQ      1
#define GPSMI_FE_SC8       2
#define GPSMI_FE_SC16      3
#define GPSMI_FE_R8        4
#define GPSMI_FE_CONJUGATE 1    /* gpsmi_fe_cfg.flags bit 0 */
typedef struct gpsmi_fe gpsmi_fe;
typedef struct gpsmi_fe_cfg {   /* no implicit padding: 48 bytes                        */
    int64_t fs_in_hz;           /* input rate, 1 .. 2^31 - 1                           */
    int64_t fs_out_hz;          /* output rate (1000 * CODE_SAMPLES for the engines)   */
    double  if_hz;              /* IF (real input) or tuner offset (complex); sign = sideband */
    float   passband_hz;        /* 0: 0.44 min(fs_in, fs_out)                          */
    float   atten_db;           /* 0: 60 (20 .. 120)                                   */
    int32_t format;             /* GPSMI_FE_*                                          */
    int32_t flags;              /* GPSMI_FE_CONJUGATE (complex input only)             */
    int32_t max_out;            /* largest output count of one host call (scratch)     */
    int32_t device;
} gpsmi_fe_cfg;
/* host only, no GPU: validates cfg (max_out and device aside) and returns the filter; table
 * (optional) receives (n_phases + 1) * n_taps floats, row-major as above                       */
int gpsmi_fe_design(const gpsmi_fe_cfg* cfg, int* n_taps, int* n_phases, float* table);
int gpsmi_fe_create(const gpsmi_fe_cfg* cfg, gpsmi_fe** out);
int gpsmi_fe_destroy(gpsmi_fe* h);
int gpsmi_fe_reset(gpsmi_fe* h);                 /* input index := 0, carry := 0, not flushed */
/* host in (n_in samples of the format) -> host out (complex64, *n_out of at most max_out)      */
int gpsmi_fe_push(gpsmi_fe* h, const void* in, size_t n_in, float* out, size_t max_out, size_t* n_out);
/* the same from device memory to device memory (no max_out limit of the handle)                */
int gpsmi_fe_push_dev(gpsmi_fe* h, const void* d_in, size_t n_in, void* d_out, size_t max_out,
                      size_t* n_out);
/* end of stream: zeros past the last sample; the outputs up to it -> host out                  */
int gpsmi_fe_flush(gpsmi_fe* h, float* out, size_t max_out, size_t* n_out);
int gpsmi_fe_last_ms(gpsmi_fe* h, float* ms);

/* ========================================================================
 * Pulse blanking: an opt-in input stage against pulsed and swept (chirp) interference, ahead of
 * acquisition and tracking.  Works in the time domain, at any block length.
 * Per block of n = block_samples samples x (complex64, or the recorder's uint16 decoded as
 * gpsmi_dev_unpack_u8iq does), every step exact in float32 or in integers:
 *   power      p_i = re*re + im*im in float32 (two products and one add, never fused);
 *   floor      m = the order statistic of rank (n - 1) / 2 (from 0, ascending) of the block's p,
 *              ties and zeros included (the lower median);
 *   threshold  f = (float)10^(thresh_db / 10) in double on the host, T = m * f in float32; sample j
 *              is a detection when p_j > T (thresh_db = +inf, an all-zero block: none);
 *   guard      sample i is blanked when a detection j of the same block has i - post <= j <= i + pre,
 *              or when i < carry, carry = max(0, j + post - n + 1) over the previous block's
 *              detections (0 after create / reset): output block k depends on input blocks k - 1
 *              and k only;
 *   output     blanked samples are 0 + 0j, every other sample is the input bit for bit (complex64);
 *   too much   more than floor(max_frac * n) blanked samples: the block passes through (the input,
 *              decoded for u8), count -1, mask empty; its floor is still reported and its carry
 *              still taken from its detections.
 * counts int32 [nb] (blanked samples, -1 passed through), floors float32 [nb] (m) and masks uint32
 * [nb * n / 32] (sample i of block b in bit i % 32 of masks[b * n / 32 + i / 32]) are host arrays;
 * floors and masks may be null.  nb consecutive blocks in order: block b's carry comes from block
 * b - 1 (the handle's for b = 0), the handle keeps the last block's.  Input and output must not
 * overlap (GPSMI_E_ARG); device complex64 input and the output must be 16-byte aligned, device u8
 * input 4-byte aligned.  Every output word is written by one thread: the bits do not depend on the
 * grid, the batch size or the cut of the input into calls.  Both calls return when the work is
 * done; gpsmi_pb_last_ms reports its device time.  Argument errors (a null cfg or handle, a bad n,
 * pre / post out of range, a NaN threshold, max_frac outside [0, 1], nb <= 0) are GPSMI_E_ARG and
 * need no GPU; a failed allocation is GPSMI_E_NOMEM and leaves the handle usable.  Tuning only:
 * the environment variable GPSMI_PB_CHUNK_MIB (read at create; default 0 = the whole call) sets
 * the input bytes the passes run over at a time; it changes no result.
 * ======================================================================== */
typedef struct gpsmi_pb gpsmi_pb;
typedef struct gpsmi_pb_cfg {
    int32_t block_samples;      /* n: multiple of 32, >= 2048 (65536, 130944, ...)      */
    float   thresh_db;          /* 10.0; not NaN; +inf detects nothing                   */
    int32_t pre, post;          /* guard samples before / after a detection, 0 .. 1024   */
    float   max_frac;           /* 0.5; in [0, 1]                                        */
    int32_t device;
} gpsmi_pb_cfg;
int gpsmi_pb_create(const gpsmi_pb_cfg* cfg, gpsmi_pb** out);
int gpsmi_pb_destroy(gpsmi_pb* h);
/* GPSMI_IQ_C64 (default) or GPSMI_IQ_U8 (the recorder's uint16, decoded on load) */
int gpsmi_pb_set_input_format(gpsmi_pb* h, int fmt);
int gpsmi_pb_reset(gpsmi_pb* h);                              /* carry := 0 */
/* host iq (nb * n samples in the input format) -> host out (complex64 [nb * n])                */
int gpsmi_pb_apply(gpsmi_pb* h, const void* iq, float* out, int nb, int32_t* counts, float* floors,
                   uint32_t* masks);
/* the same from device memory to device memory (the result arrays are host memory)             */
int gpsmi_pb_apply_dev(gpsmi_pb* h, const void* d_iq, void* d_out, int nb, int32_t* counts,
                       float* floors, uint32_t* masks);
int gpsmi_pb_last_ms(gpsmi_pb* h, float* ms);

/* ========================================================================
 * Null steering (power inversion): an opt-in input stage against interference that is wide in
 * frequency and continuous in time, for recordings of A coherent, sample-aligned antennas, ahead of
 * everything else (float64 restatement: tests/nul_ref.py).  It minimises the output
 * power with the gain of antenna 0 (the reference element) held at one; no calibration, no antenna
 * positions, no satellite directions.  A call takes A antennas x nb consecutive blocks of
 * n = block_samples samples, antenna-major: [A][nb * n], complex64 or the recorder's uint16 decoded
 * as gpsmi_dev_unpack_u8iq does.  Every block is worked on alone (no carry, no state):
 *   covariance C[a][b] = sum_i x_a[i] conj(x_b[i]), a >= b, the float32 samples converted to float64
 *              (every product is exact), the sums float64 in this order: the block is cut into
 *              slices of 8192 samples (the last one may be shorter); in a slice, lane t of 256 takes
 *              the samples 2048 r + 8 t .. 2048 r + 8 t + 7 for r = 0, 1, 2, 3 (those the slice
 *              has) in ascending order, from zero, per sample
 *                  re += ar * br;  re += ai * bi;  im += ai * br;  im -= ar * bi;
 *              the 256 lane sums are added as a binary tree of neighbours (lanes 2k and 2k + 1, then
 *              pairs of those, eight levels); the slice sums are added in ascending slice order,
 *              starting from slice 0's.  The order depends on n alone;
 *   loading    R = C / n + delta I, delta = load * (sum_a C[a][a] / n) / A (the trace summed in
 *              ascending a, each term divided by n first);
 *   weights    R = L L^H by Cholesky without pivoting, in float64, column by column j = 0 .. A - 1:
 *              d = R[j][j] - sum_{k<j} |L[j][k]|^2, L[j][j] = sqrt(d), then for i > j
 *              L[i][j] = (R[i][j] - sum_{k<j} L[i][k] conj(L[j][k])) / L[j][j]; every sum subtracts
 *              its terms one at a time in ascending k, nothing is fused; complex products are
 *              (ar br - ai bi) + j (ar bi + ai br) with conj() a sign flip; L y = e0 forward
 *              (y[i] = -(sum_{k<i} L[i][k] y[k]) / L[i][i], y[0] = 1 / L[0][0]) and L^H u = y backward
 *              (u[i] = (y[i] - sum_{k>i} conj(L[k][i]) u[k]) / L[i][i], i descending, k ascending);
 *              w[0] = 1, w[a] = u[a] / Re u[0]; predicted gain g = (C[0][0] / n) * Re u[0], the
 *              power of antenna 0 over the output power; gain_db = (float)(10 log10 g);
 *   decision   a pivot d that is not positive and finite (an all-zero block: its first pivot is
 *              0), or 10 log10 g < min_gain_db: the block passes through: the output is
 *              antenna 0's block bit for bit (decoded for u8), flag 0, weights e0; gain_db is 0
 *              when the solve did not finish.  Otherwise flag 1;
 *   apply      w32 = complex64(w); y[i] = sum_a conj(w32[a]) x_a[i] in float32, ascending a from
 *              antenna 0's term, each term (wr xr + wi xi) + j (wr xi - wi xr): two products and
 *              one add / subtract each, then one add per component into y; nothing is fused.
 * The covariance runs on several workgroups per block (one per slice), a second kernel adds the
 * slice sums and solves with one thread per block on the device, a third applies; no atomics.  One
 * thread writes each output word: the bits do not depend on the grid, on nb or on the cut of the
 * input into calls.  flags int32 [nb], gain_db float32 [nb] and weights float64 [nb][A][2] (re, im
 * of w) are host arrays, each may be null.  Input and output must not overlap (GPSMI_E_ARG); device
 * complex64 input and the output must be 16-byte aligned, device u8 input 4-byte aligned.  Both
 * calls return when the work is done; gpsmi_nul_last_ms reports its device time.  Argument errors (a
 * null cfg or handle, a bad n, antennas outside 2..8, a NaN or negative load or min_gain_db,
 * nb <= 0) are GPSMI_E_ARG and need no GPU; a failed allocation is GPSMI_E_NOMEM and leaves the
 * handle usable.
 *
 * Space-time taps (cfg.taps = T in {3, 5, 7}; restatement: tests/stap_ref.py).  taps 0
 * or 1 is everything above, byte for byte; any other value is GPSMI_E_ARG and needs no GPU.  Every A in
 * 2..8 goes with every T: K = A T <= 56 weights per block, w[a][t] at k(a, t) = a T + t, c = (T - 1) / 2.
 * A filter of T taps per antenna compensates what one complex weight cannot: delay and filter mismatch
 * between the channels, and more than A - 1 narrowband interferers.  Each block is worked on alone:
 *   lag sums   r_ab(l) = sum_{i=l}^{n-1} x_a[i] conj(x_b[i - l]) for l = 0 .. T - 1 and all (a, b); at
 *              l = 0 only a >= b is kept.  The block is zero outside 0 .. n - 1, no sample of a
 *              neighbouring block is read.  Accumulators are float64 (every product of two float32
 *              samples is exact there).  The four real sums of a pair, RR = sum Re Re, II, IR =
 *              sum Im x_a Re x_b and RI, are accumulated apart and combined after the last sample:
 *              re = RR + II, im = IR - RI; the imaginary part of r_aa(0) is exactly 0.  The order of
 *              each sum is fixed by n alone -- it does not depend on the grid, on nb or on how the
 *              input is cut into calls -- and is not otherwise specified (the kernel forms the sums
 *              on the float64 matrix pipe, four samples per instruction, per wave and slice of 8192
 *              samples; waves and slices are added in ascending order);
 *   matrix     R[k(a,t)][k(b,s)] = r_ab(s - t) / n for s >= t and conj(r_ba(t - s)) / n for s < t: the
 *              Gram matrix of the zero-extended, shifted rows Z[k(a,t)][i] = x_a[i - t],
 *              i = 0 .. n + T - 2, over n: Hermitian, block-Toeplitz, positive semidefinite;
 *   loading    delta = load * (sum_a r_aa(0) / n) / A on the diagonal, load as above;
 *   weights    R = L L^H by Cholesky without pivoting in float64, column by column as above (K for
 *              A); L y = e_{k(0,c)} forward, every row subtracting its terms in ascending column
 *              order from its right-hand side, and L^H u = y backward as above; w = u / Re u_{k(0,c)}
 *              with w[0][c] exactly 1; predicted gain g = (r_00(0) / n) * Re u_{k(0,c)},
 *              gain_db = (float)(10 log10 g).  Nothing is fused;
 *   decision   as above: a pivot that is not positive and finite, or 10 log10 g < min_gain_db: the
 *              output is antenna 0's whole block bit for bit (decoded for u8), flag 0, weights
 *              e_{k(0,c)};
 *   apply      w32 = complex64(w).  For c <= i < n - c:
 *                  y[i] = sum_a sum_t conj(w32[a][t]) x_a[i + c - t]
 *              in float32, ascending a, ascending t within a, starting from (0, 0)'s term; each term
 *              (wr xr + wi xi) + j (wr xi - wi xr) and one add per component into y as above.  For
 *              i < c and i >= n - c the output is +0.0 + 0.0j: a tap there would reach outside the
 *              block and the cancellation would be incomplete.  The output is aligned with antenna 0:
 *              code phases do not move.
 * weights is float64 [nb][A][T][2] ([nb][A][2] for taps <= 1).  Formats, alignment, the overlap
 * refusal, last_ms and GPSMI_E_NOMEM are as above.
 * ======================================================================== */
typedef struct gpsmi_nul gpsmi_nul;
typedef struct gpsmi_nul_cfg {
    int32_t block_samples;      /* n: multiple of 32, >= 2048 (65536, 130944, ...)      */
    int32_t antennas;           /* A: 2 .. 8, antenna 0 is the reference element         */
    float   load;               /* diagonal loading; 0 means 1e-6; not NaN, not negative */
    float   min_gain_db;        /* 0 means 3.0; not NaN, not negative                    */
    int32_t device;
    int32_t taps;               /* 0 or 1: one weight per antenna; 3, 5 or 7: space-time */
} gpsmi_nul_cfg;
int gpsmi_nul_create(const gpsmi_nul_cfg* cfg, gpsmi_nul** out);
int gpsmi_nul_destroy(gpsmi_nul* h);
/* GPSMI_IQ_C64 (default) or GPSMI_IQ_U8 (the recorder's uint16, decoded on load) */
int gpsmi_nul_set_input_format(gpsmi_nul* h, int fmt);
/* host iq ([A][nb * n] samples in the input format) -> host out (complex64 [nb * n])           */
int gpsmi_nul_apply(gpsmi_nul* h, const void* iq, float* out, int nb, int32_t* flags, float* gain_db,
                    double* weights);
/* the same from device memory to device memory (the result arrays are host memory)             */
int gpsmi_nul_apply_dev(gpsmi_nul* h, const void* d_iq, void* d_out, int nb, int32_t* flags,
                        float* gain_db, double* weights);
int gpsmi_nul_last_ms(gpsmi_nul* h, float* ms);
/* device time of the three kernels of the last finished call: ms[0] covariance, ms[1] solve, ms[2] apply */
int gpsmi_nul_last_kernel_ms(gpsmi_nul* h, float* ms);

/* ------------------------------------------------------------------------
 * Per-satellite beams on the same handle (restatement: tests/beam_ref.py).  Where
 * gpsmi_nul_apply holds antenna 0 at one and knows no direction, a beam holds a given steering vector
 * s at one (w^H s = 1), holds up to four given null vectors u_q at zero (w^H u_q = 0) and minimises
 * the output power under those constraints: w = R^-1 G (G^H R^-1 G)^-1 e0, G = [s, u_q ...].  One call
 * forms nbeam beams from the same A rows: the samples are read once.  The handle must have been made
 * with taps 0 or 1 (a space-time handle: GPSMI_E_STATE); nothing of gpsmi_nul_apply changes, and a
 * beams call leaves the results of the last gpsmi_nul_apply call alone.
 *   input      A rows of nb blocks of n = block_samples samples in the handle's input format; row a
 *              starts a * in_stride samples behind row 0 (gpsmi_nul_beams_dev; 0 means nb * n, the
 *              layout of gpsmi_nul_apply and of the host entry);
 *   output     nbeam rows of nb * n complex64 samples, row b at b * out_stride samples (0: nb * n);
 *   beams      nbeam 1 .. 64; steer float64 [nbeam][A][2] (re, im); nulls float64 [nnull][A][2],
 *              nnull 0 .. 4, shared by the beams; null_mask uint32 [nbeam], bit q set: beam b carries
 *              null q (null_mask may be a null pointer when nnull is 0).  A beam has
 *              m = 1 + popcount(null_mask[b]) <= A constraints, G's columns: s_b, then its nulls in
 *              ascending q.
 * Every block is worked on alone, in float64, nothing fused, complex products and conj() as above:
 *   covariance, loading, Cholesky   C, R = C / n + delta I and R = L L^H exactly as gpsmi_nul_apply
 *              forms them, with the handle's load (min_gain_db plays no part).  A pivot that is not
 *              positive and finite (an all-zero block): L = I in everything below, the beam is the
 *              quiescent one, flag 0; else flag 1;
 *   columns    z = L^-1 g for every column g of G, forward: z[i] = (g[i] - sum_{k<i} L[i][k] z[k]) /
 *              L[i][i], the terms subtracted one at a time in ascending k;
 *   M = Z^H Z  M[i][j] = sum_a conj(z_i[a]) z_j[a] for i > j, from 0 + 0j in ascending a, one complex
 *              add per term; M[i][i] = sum_a (re^2 + im^2) of z_i[a], from 0 in ascending a;
 *   M q = e0   M = K K^H by the Cholesky above (m for A), K y = e0 forward and K^H q = y backward as
 *              above.  A pivot of M that is not positive and finite: flag -1, the beam's block of
 *              output is +0.0 + 0.0j, its weights are 0 and gain_db is 0;
 *   weights    t[a] = sum_j z_j[a] q[j], from 0 + 0j in ascending j; L^H w = t backward:
 *              w[i] = (t[i] - sum_{k>i} conj(L[k][i]) w[k]) / L[i][i], i descending, k ascending.
 *              Then w^H s = 1 and w^H u_q = 0 to rounding, and the output power w^H R w is p = Re q[0];
 *   gain       gain_db = (float)(10 log10(tr / (|s|^2 p))), tr = sum_a C[a][a] / n as in the loading
 *              (without delta), |s|^2 = sum_a (re^2 + im^2) from 0 in ascending a: the mean antenna
 *              power over the output power referred to one antenna; 10 log10 A in white noise;
 *   apply      w32 = complex64(w), y_b[i] = sum_a conj(w32_b[a]) x_a[i] in float32, exactly the apply
 *              of gpsmi_nul_apply.
 * flags int32 [nb][nbeam], gain_db float32 [nb][nbeam] and weights float64 [nb][nbeam][A][2] are host
 * arrays, each may be null.  The bytes of a beam's block depend on that block and that beam (its
 * steering vector, its null vectors, the load) alone: not on nbeam, the other beams, the bits of
 * null_mask beyond its own, nb, the cut of the input into calls, the strides or the entry point; u8
 * input gives the bytes of its complex64 decode.  One thread writes each output word, no atomics;
 * samples between the rows of a strided output are not touched.
 * Argument errors are GPSMI_E_ARG and need no GPU; gpsmi_nul_beams_plan makes those of the beam
 * description without a handle: a null pointer; nbeam, nnull or antennas out of range; a mask bit
 * >= nnull; m > A; a vector that is zero or not finite; dependent constraints -- the Gram matrix of a
 * beam's columns, each divided by its length, must have a float64 Cholesky whose every pivot (the
 * value under the square root) is >= 1 / 64: for one null, |s^H u| / (|s| |u|) <= 0.992, beyond which
 * the null costs more than 18 dB of noise gain.  On a handle also: nb <= 0; a stride below nb * n or
 * negative; device rows that break the alignment of gpsmi_nul_apply_dev (16 bytes for complex64 input
 * and the output, 4 for u8 input: strides must be even); an input row that overlaps an output row.
 * A failed allocation is GPSMI_E_NOMEM and leaves the handle usable.
 * ------------------------------------------------------------------------ */
int gpsmi_nul_beams_plan(int antennas, int nbeam, const double* steer, int nnull, const double* nulls,
                         const uint32_t* null_mask);
/* host iq ([A][nb * n] in the input format) -> host out (complex64 [nbeam][nb * n])             */
int gpsmi_nul_beams(gpsmi_nul* h, const void* iq, float* out, int nb, int nbeam, const double* steer,
                    int nnull, const double* nulls, const uint32_t* null_mask, int32_t* flags,
                    float* gain_db, double* weights);
/* the same from device memory to device memory, strides in samples (the other arrays are host memory) */
int gpsmi_nul_beams_dev(gpsmi_nul* h, const void* d_iq, int64_t in_stride, void* d_out, int64_t out_stride,
                        int nb, int nbeam, const double* steer, int nnull, const double* nulls,
                        const uint32_t* null_mask, int32_t* flags, float* gain_db, double* weights);
/* device time of the three kernels of the last finished beams call: covariance, solve, apply   */
int gpsmi_nul_last_beam_kernel_ms(gpsmi_nul* h, float* ms);

/* ========================================================================
 * Time-frequency (sweep) excision: an opt-in input stage against swept and chirp interference, for
 * one antenna, ahead of acquisition and tracking (float64 restatement:
 * tests/tfx_ref.py).  A slow in-band sweep is continuous in time and wide in a block's mean spectrum,
 * so neither the tone excision nor the blanker grips it, but it is narrow in every short time slice.
 * Per block of n = block_samples samples x (complex64, or the recorder's uint16 decoded as
 * gpsmi_dev_unpack_u8iq does), L = frame, H = L / 2, nf = n / H frames:
 *   frames     frame f = 0 .. nf - 1 covers block samples f H - H .. f H + H - 1; frame 0 starts in the
 *              carry, the previous block's last H input samples (zero after create / reset; a format
 *              switch keeps it).  Window: periodic Hann w[i] = (float)(0.5 - 0.5 cos(2 pi i / L)), the
 *              formula in double; the last frame's second half is weighted 1, so that the frames sum
 *              to 1 everywhere and output block k needs input blocks k - 1 and k only;
 *   power      P[f][k] = re*re + im*im (float32: two products and one add, never fused) of the L-point
 *              transform of the windowed frame, computed in float32;
 *   floor      m = the order statistic of rank (c - 1) / 2 (from 0, ascending; the lower median) of
 *              the c = (nf - 1) L values P[f][k] of all frames but the last;
 *   threshold  F = (float)10^(thresh_db / 10) in double on the host, T = m * F in float32; the last
 *              frame's threshold is T * (float)(11.0 / 6.0) in float32 (its window carries 11/6 of
 *              Hann's power); cell (f, k) is a detection when P[f][k] > T, strictly (thresh_db = +inf,
 *              an all-zero block: none);
 *   widening   cell (f, k) is flagged when a detection (f, k') has (k - k') mod L within -dilate ..
 *              dilate: circular inside the frame, none in time;
 *   too much   count = the flagged cells of the block; count > floor(max_frac * nf * L) (in double):
 *              the block passes through bit for bit (decoded for u8), count -1, mask empty; its
 *              floor is still reported.  The carry for the next block is the input's tail always;
 *   output     the flagged cells of every frame's transform are set to zero, each frame is
 *              transformed back with scale 1 / L and the frames are overlap-added; out is complex64.
 * counts int32 [nb] (flagged cells, -1 passed through), floors float32 [nb] (m) and masks uint32
 * [nb][nf L / 32] (cell (f, k) of block b in bit k % 32 of word f L / 32 + k / 32 of the block's
 * words) are host arrays, each may be null.  nb consecutive blocks in order: block b's carry is
 * block b - 1's tail (the handle's for b = 0), the handle keeps the last block's.  Input and output
 * must not overlap (GPSMI_E_ARG); device complex64 input and the output must be 16-byte aligned,
 * device u8 input 4-byte aligned.  Floors, masks and counts follow from the stored P by comparisons
 * and integer operations alone; every output sample is written once by one thread, no float
 * atomics: the bits do not depend on the grid, on nb or on the cut of the input into calls.  Both
 * calls return when the work is done; gpsmi_tfx_last_ms reports its device time.
 * gpsmi_tfx_last_power copies out the float32 P of the last call, [nb][nf][L], nb that call's;
 * GPSMI_E_STATE unless the handle was made with keep_power and a call has run.
 * A bad block_samples or frame is GPSMI_E_UNSUPPORTED with the field's name in the message; the
 * other argument errors (a null cfg or handle, a NaN threshold, dilate, max_frac or keep_power out
 * of range, nb <= 0) are GPSMI_E_ARG; none needs a GPU.  A failed allocation is GPSMI_E_NOMEM and
 * leaves the handle usable.
 * Limits: a sweep that crosses more than about one bin width (fs / L) per frame length (L / fs),
 * i.e. a rate above some (fs / L)^2, is wide in every frame and is not gripped at that L; at most
 * max_frac of the plane is removed; the first block after create / reset stands behind a zero
 * carry (a step at sample 0 in its frame 0).
 * ======================================================================== */
typedef struct gpsmi_tfx gpsmi_tfx;
typedef struct gpsmi_tfx_cfg {
    int32_t block_samples;      /* n: multiple of 128 in 1024 .. 2^24 (65536, 130944, 523776, ...) */
    int32_t frame;              /* L: 32, 64, 128 or 256; 0 means 64                             */
    float   thresh_db;          /* 0 means 12.0; not NaN; +inf flags nothing                     */
    int32_t dilate;             /* 0 .. 8 bins each way; -1 means the default, 1                 */
    float   max_frac;           /* in [0, 1]; 0 means 0.5                                        */
    int32_t keep_power;         /* 0, or 1: gpsmi_tfx_last_power may be called                   */
    int32_t device;
    int32_t reserved;           /* 0 */
} gpsmi_tfx_cfg;
int gpsmi_tfx_create(const gpsmi_tfx_cfg* cfg, gpsmi_tfx** out);
int gpsmi_tfx_destroy(gpsmi_tfx* h);
/* GPSMI_IQ_C64 (default) or GPSMI_IQ_U8 (the recorder's uint16, decoded on load) */
int gpsmi_tfx_set_input_format(gpsmi_tfx* h, int fmt);
int gpsmi_tfx_reset(gpsmi_tfx* h);                            /* carry := 0 */
/* host iq (nb * n samples in the input format) -> host out (complex64 [nb * n])                */
int gpsmi_tfx_apply(gpsmi_tfx* h, const void* iq, float* out, int nb, int32_t* counts, float* floors,
                    uint32_t* masks);
/* the same from device memory to device memory (the result arrays are host memory)             */
int gpsmi_tfx_apply_dev(gpsmi_tfx* h, const void* d_iq, void* d_out, int nb, int32_t* counts,
                        float* floors, uint32_t* masks);
int gpsmi_tfx_last_ms(gpsmi_tfx* h, float* ms);
int gpsmi_tfx_last_power(gpsmi_tfx* h, float* P);

/* ========================================================================
 * Multi-GPU: one process per GPU; SVs / blocks are sharded by the host and
 * the only exchange is a gather of fixed-size peak records over RCCL.
 * ======================================================================== */
typedef struct gpsmi_comm gpsmi_comm;
#define GPSMI_COMM_ID_BYTES 128
int gpsmi_comm_unique_id(void* id_bytes);             /* rank 0, then broadcast */
int gpsmi_comm_create(const void* id_bytes, int nranks, int rank, int device,
                      gpsmi_comm** out);
int gpsmi_comm_destroy(gpsmi_comm* c);
/* The communicator's size and this process's rank as RCCL reports them (ncclCommCount,
 * ncclCommUserRank): evidence that the collective really spans the ranks.        */
int gpsmi_comm_count(gpsmi_comm* c, int* nranks, int* rank);
/* all-gather of `count` peak records per rank: every rank must pass the SAME count (a
 * collective with unequal counts does not return; gpsmi.sharding.agree_on_count checks it on
 * the host before the call, as bench.py does); d_send [count], d_recv
 * [nranks*count], both device pointers; host_recv (optional) gets a copy.     */
int gpsmi_comm_allgather_peaks(gpsmi_comm* c, const void* d_send, void* d_recv,
                               int count, gpsmi_peak* host_recv);

#ifdef __cplusplus
}
#endif
#endif /* GPSMI_H */
