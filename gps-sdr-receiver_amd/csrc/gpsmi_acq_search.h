// Kernels of the acquisition searches (gpsmi_acq_search*, include/gpsmi.h; DESIGN.md 4.2, 4.2a,
// 4.2e).  The handle and the entry points sit in gpsmi_acq.hip; the native 16368 correlation in
// gpsmi_pfa.h.  Replaces the array arithmetic of reference src/gpsrecv.py:241-274.
//
//   acq_spectrum_kernel   CS 2048, one workgroup per (Doppler bin, segment): carrier wipe-off with
//                         the reference's float32 phase argument (gpsrecv.py:232-235), fold of the
//                         n_coh code periods (sum of FFTs = FFT of the sum, :250-254), 2048-point
//                         FFT in LDS, spectrum to a small L2-resident scratch.
//   acq_fold_kernel       any other code length: the same wipe-off and fold, left in the time domain.
//   acq_corr_kernel<MODE> one workgroup per (SV, bin): conj(X) * R from coalesced reads of the
//                         replica spectra, the same FFT as the inverse (|ifft(Y)| = |fft(conj Y)| / N,
//                         :258), |.|, then mean / population std / first-index argmax
//                         (findCodePhase, :217-223) by wave64 shuffles.  The nbins x nsv x 2048
//                         correlation surface never reaches HBM; 16 bytes per cell do.
//                         MODE 0: the coherent search, one segment.  MODE 1: the non-coherent search,
//                         the mean of |corr| over the segments, summed in registers.  MODE 2: the deep
//                         search, the same mean with every segment's magnitudes rotated by the
//                         code-Doppler slide.  MODE 3: MODE 2 that also keeps the surface S of every
//                         cell, rows [sv][nbins][2048] (gpsmi_acq_search_deep_rows_dev).
//   acq_cells_kernel, acq_peaks_kernel
//                         the cell tables of the time-domain and native-length correlations, and
//                         their statistics as peak records.
#pragma once
#include "gpsmi_common.h"
#include "gpsmi_direct.h"
#include "gpsmi_fft.h"
#include "gpsmi_stats.h"

namespace gpsmi {

// Segment `seg` = blockIdx.y of a search reads iq advanced by seg * n_coh * 2048 samples; the wipe-off
// restarts at phase 0 and SEC_TIME[0] in every segment.  Grid (bins, segments); the spectrum of
// (bin b, segment s) goes to spectra[(b * nseg + s) * 2048].  The coherent search is nseg = 1.
// G = 1: 256 threads, the code periods folded one after the other.  G = 4 (long coherent
// integrations): 1024 threads, the periods dealt round-robin to four groups of 256 whose partial
// folds meet in LDS (the sine / cosine per sample is what this kernel spends its time on);
// group 0 then adds them in group order and transforms.
// (FMT 1: iq holds the recorder's raw uint16 samples, decoded on load: gpsmi_acq_set_input_format)
template <int G, int FMT = 0>
__global__ __launch_bounds__(256 * G) void acq_spectrum_kernel(
    const void* __restrict__ iq, const float* __restrict__ t32,
    const float* __restrict__ omega, int n_coh, int nseg, float2* __restrict__ spectra,
    const float2* __restrict__ tw) {
    __shared__ __attribute__((aligned(16))) float lds[kFftLdsFloats];
    __shared__ __attribute__((aligned(16))) float lds_tw[kFftTwFloats];
    __shared__ float2 part[G > 1 ? G - 1 : 1][G > 1 ? kFftN : 1];
    const int t = threadIdx.x & 255, grp = threadIdx.x >> 8, bin = blockIdx.x, seg = blockIdx.y;
    const FftTw ftw = fft_setup(lds_tw, tw, t);           // (every group writes the same tables)
    const float om = omega[bin];
    const size_t base = (size_t)seg * n_coh * kFftN;
    float2 v[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] = make_float2(0.f, 0.f);
    for (int i = grp; i < n_coh; i += G) {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            int k = i * kFftN + t + 256 * r;
            float2 x = load_iq<FMT>(iq, base + k);
            float p = mul_rn(om, t32[k]);      // float32 phase argument, phase0 = 0
            float s, c;
            sincosf(p, &s, &c);
            // factor = (c, -s); factor * x as numpy multiplies complex64
            v[r].x += c * x.x + s * x.y;
            v[r].y += c * x.y - s * x.x;
        }
    }
    if (G > 1) {
        if (grp > 0) {
#pragma unroll
            for (int r = 0; r < 8; ++r) part[grp - 1][t + 256 * r] = v[r];
        }
        __syncthreads();
        if (grp > 0) return;                   // (a wave that has ended no longer counts at a barrier)
#pragma unroll
        for (int g = 1; g < G; ++g)
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const float2 o = part[g - 1][t + 256 * r];
                v[r].x += o.x; v[r].y += o.y;
            }
    }
    __syncthreads();
    fft2048(v, lds, ftw, t);
    const float sc = 1.0f / (float)n_coh;
    float2* out = spectra + ((size_t)bin * nseg + seg) * kFftN;
#pragma unroll
    for (int q = 0; q < 8; ++q) out[t + 256 * q] = make_float2(v[q].x * sc, v[q].y * sc);
}

// ---- general code length: wipe-off + fold in the time domain ----------------
// x[bin][seg][m] = (1/n_coh) sum_i iq[(seg n_coh + i) L + m] exp(-j fl32(om t32[i L + m]))
// Grid (lag blocks, bins of this launch, segments).
template <int FMT = 0>
__global__ __launch_bounds__(256) void acq_fold_kernel(
    const void* __restrict__ iq, const float* __restrict__ t32,
    const float* __restrict__ omega, int n_coh, int nseg, int L, float2* __restrict__ xout) {
    const int m = blockIdx.x * 256 + threadIdx.x, bin = blockIdx.y, seg = blockIdx.z;
    if (m >= L) return;
    const float om = omega[bin];
    const size_t base = (size_t)seg * n_coh * L;
    float ar = 0.f, ai = 0.f;
    for (int i = 0; i < n_coh; ++i) {
        const int k = i * L + m;
        const float2 v = load_iq<FMT>(iq, base + k);
        float sn, co;
        sincosf(mul_rn(om, t32[k]), &sn, &co);
        ar += co * v.x + sn * v.y;
        ai += co * v.y - sn * v.x;
    }
    const float sc = 1.0f / (float)n_coh;
    xout[((size_t)bin * nseg + seg) * L + m] = make_float2(ar * sc, ai * sc);
}

// the record of cell c, and its circular neighbours where they are asked for
__device__ __forceinline__ void acq_store_peak(gpsmi_peak* __restrict__ out, float2* __restrict__ nbr,
                                               size_t c, int amax, float peak, float mean, float sd,
                                               float lo, float hi) {
    gpsmi_peak p; p.argmax = amax; p.peak = peak; p.mean = mean; p.std = sd;
    out[c] = p;
    if (nbr) nbr[c] = make_float2(lo, hi);
}

// spectra: this launch's bins, [bin][nseg][2048]; out / nbr: [bin0 + bin][sv].  MODE 0 is one launch
// of one segment per bin: nseg, bin0 and shift are not read.
// MODE 1, 2: the product, the transform and |.| / 2048 of MODE 0 for every segment, the magnitudes
// summed in registers in ascending segment order and scaled by 1 / nseg, then the statistics once.
// The next segment's spectrum is requested before the current one is transformed (the cells are
// latency-bound chains).
// MODE 2, 3: segment s is added at the lag it had at the start of the data, S[i] += |corr_s[(i + m) mod
// 2048]|, m = shift[bin][s] in 0 .. 2047 (the code-Doppler slide, one integer per bin and segment
// from the host).  The magnitude a sum needs now comes from another thread: a segment's 2048
// magnitudes go through LDS once, unscaled, in the plane the statistics use as their copy (the
// transform's buffer 1, free once its last exchange barrier is passed), and thread t picks up its
// eight lags at (t + 256 q + m) mod 2048 -- consecutive lanes read consecutive floats, rotated as a
// whole: no bank conflicts.  m is uniform per workgroup and segment (a scalar load, issued ahead of
// the transform like the next spectrum).  Barriers per segment: the loop's own (the reads of the
// previous segment's magnitudes are done before the next transform's second pass overwrites the
// plane) and one between writing and reading.
template <int MODE>
__global__ __launch_bounds__(256) void acq_corr_kernel(
    const float2* __restrict__ spectra, const float2* __restrict__ rep,
    const int* __restrict__ slot, gpsmi_peak* __restrict__ out, int nsv, int nseg, int bin0,
    const float2* __restrict__ tw, float2* __restrict__ nbr, const int* __restrict__ shift,
    float* __restrict__ rows, int nbins) {
    constexpr bool DEEP = MODE >= 2;
    __shared__ __attribute__((aligned(16))) float lds[kFftLdsFloats];
    __shared__ __attribute__((aligned(16))) float red[kStatsRedFloats];
    __shared__ __attribute__((aligned(16))) float lds_tw[kFftTwFloats];
    // the statistics' copy of the magnitudes lives in the second FFT buffer, which the transform
    // leaves free when it returns: 40.4 KiB of LDS, four workgroups per CU instead of three
    float* magbuf = lds + 2 * kFftPlane;
    static_assert(kFftN <= 2 * kFftPlane1, "the alias must fit buffer 1");
    const int t = threadIdx.x, sv = blockIdx.x, bin = blockIdx.y;
    const FftTw ftw = fft_setup(lds_tw, tw, t);
    const float2* X = spectra + (size_t)bin * (MODE == 0 ? 1 : nseg) * kFftN;
    const float2* R = rep + (size_t)slot[sv] * kFftN;
    const int* M = DEEP ? shift + (size_t)bin * nseg : nullptr;
    float2 x[8], r[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        x[q] = X[t + 256 * q];
        r[q] = R[t + 256 * q];
    }
    float mag[8];                              // MODE 0: the magnitudes; else their sum over the segments
    // segment s: x holds its spectrum on entry and, MODE 1 / 2, the next segment's on return
    auto segment = [&](int s) {
        float2 v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q)            // conj(x) * r
            v[q] = make_float2(x[q].x * r[q].x + x[q].y * r[q].y, x[q].x * r[q].y - x[q].y * r[q].x);
        int m = 0;
        if constexpr (MODE != 0) {
            // the next segment (past the last one the last again, never used: no branch around the loads)
            const float2* Xn = X + (size_t)(s + 1 < nseg ? s + 1 : s) * kFftN;
#pragma unroll
            for (int q = 0; q < 8; ++q) x[q] = Xn[t + 256 * q];
            if constexpr (DEEP) m = __builtin_amdgcn_readfirstlane(M[s]);
        }
        // (the previous transform's last LDS reads, MODE 2 the previous segment's, are done)
        if constexpr (DEEP) lds_barrier(); else __syncthreads();
        fft2048(v, lds, ftw, t);
        // fft(conj Y)[n] = conj(N ifft(Y)[n]): same lag index, no reversal
        float a[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) a[q] = __builtin_amdgcn_sqrtf(v[q].x * v[q].x + v[q].y * v[q].y);   // v_sqrt_f32, 1 ulp
        if constexpr (DEEP) {
#pragma unroll
            for (int q = 0; q < 8; ++q) magbuf[t + 256 * q] = a[q];
            lds_barrier();
#pragma unroll
            for (int q = 0; q < 8; ++q) a[q] = magbuf[(t + 256 * q + m) & (kFftN - 1)];
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            if constexpr (MODE == 0) mag[q] = a[q] * (1.0f / kFftN);
            else mag[q] += a[q] * (1.0f / kFftN);
        }
    };
    float sm;                                  // the thread's share of the statistics' sum
    if constexpr (MODE == 0) {
        segment(0);
        sm = stats_sum8(mag);
    } else {
#pragma unroll
        for (int q = 0; q < 8; ++q) mag[q] = 0.f;
#pragma unroll 1
        for (int s = 0; s < nseg; ++s) segment(s);
        if constexpr (DEEP) lds_barrier();   // (the statistics write the plane the sums just read)
        const float sc = 1.0f / (float)nseg;
        // The means of these searches are pinned bytewise (tests/golden/acq_parent_tables.npz) to a
        // build in which the compiler had taken the scale into the sum from the third row on: the
        // first two rows add their rounded magnitudes, the others add the unrounded product in one
        // fused step.  Written out, so that it no longer depends on what the compiler fuses; every
        // other use of a magnitude takes the rounded value.
        float raw[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) { raw[q] = mag[q]; mag[q] = mul_rn(raw[q], sc); }
        sm = add_rn(add_rn(0.f, mag[0]), mag[1]);
#pragma unroll
        for (int q = 2; q < 8; ++q) sm = __builtin_fmaf(raw[q], sc, sm);
        if constexpr (MODE == 3) {             // the surface the statistics below are formed of
            float* row = rows + ((size_t)sv * nbins + bin0 + bin) * kFftN;
#pragma unroll
            for (int q = 0; q < 8; ++q) row[t + 256 * q] = mag[q];
        }
    }
    int amax; float peak, mean, sd, lo, hi;
    corr_stats8(mag, sm, t, magbuf, red, amax, peak, mean, sd, lo, hi);
    if (t == 0)
        acq_store_peak(out, nbr, (size_t)(MODE == 0 ? bin : bin0 + bin) * nsv + sv, amax, peak, mean, sd, lo, hi);
}

__global__ void acq_cells_kernel(int* __restrict__ xsel, int* __restrict__ rsel,
                                 const int* __restrict__ slot, int nsv, int ncell) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncell) return;
    xsel[c] = c / nsv;                       // the bin's folded block
    rsel[c] = slot[c % nsv];                 // the SV's replica
}

__global__ void acq_peaks_kernel(const DirStats* __restrict__ st, gpsmi_peak* __restrict__ out,
                                 float2* __restrict__ nbr, int ncell) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncell) return;
    acq_store_peak(out, nbr, c, st[c].argmax, st[c].peak, st[c].mean, st[c].std, st[c].lo, st[c].hi);
}

}  // namespace gpsmi
