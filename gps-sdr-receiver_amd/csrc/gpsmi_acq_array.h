// Kernel of the array search (gpsmi_acq_search_array*, include/gpsmi.h): the deep
// search over A = 2 .. 4 antennas whose complex correlations are combined per lag before anything is
// detected.  The spectra are acq_spectrum_kernel's (gpsmi_acq_search.h), one launch per antenna row,
// unchanged; the plan and the entry points sit in gpsmi_acq.hip.
//
//   acq_corr_array_kernel<A>   the geometry of acq_corr_kernel<2>: one 256-thread workgroup per (SV,
//                              bin), eight lags per thread.  Per segment s and antenna a: conj(X_a) * R,
//                              the 2048-point transform, and the complex correlation
//                              c[a][s] = conj(transform) / 2048 read back through LDS rotated by
//                              m[bin][s] (the transform of the conjugated product is the conjugate of
//                              N ifft: taken back here, since the phases between antennas matter).
//                              Per lag, in registers across all segments:
//                                  D     += |c_a|^2                      ascending s, then ascending a
//                                  R_ab  += c_a conj(c_b)                a < b, one addition per segment
//                              and at the end T = (D + 2 sum_{a<b} |R_ab|) / (A n_seg), the pairs in
//                              lexicographic order, its row where asked for, corr_stats8 and
//                              acq_store_peak as the searches of one antenna use them.
//
// Registers: 1 + A (A - 1) accumulators per lag, 8 lags: 24, 56, 104 VGPRs for A = 2, 3, 4, beside the
// earlier antennas' values of the segment (16 VGPRs each), the replica, the next spectrum and the
// transform (about 86).  Every A is compiled for two waves per SIMD, 256 registers, without scratch;
// at A = 4 that takes two of the three waiting antennas out of the registers (STASH below).
// LDS: acq_corr_kernel's 40 KiB -- the complex plane the rotation goes through is the transform's
// buffer 1 (2048 complex of its 2304), free once the transform's last exchange barrier is passed,
// and the statistics' copy of T later lives in the same place -- plus, at A = 4, 32 KiB of stash.
#pragma once
#include "gpsmi_acq_search.h"

namespace gpsmi {

// index of the pair (a, b), a < b, in lexicographic order: (0,1) (0,2) .. (1,2) ..
template <int A>
__device__ __host__ constexpr int array_pair(int a, int b) { return a * A - a * (a + 1) / 2 + (b - a - 1); }

// spectra: this launch's bins of every antenna, [A][nb][nseg][2048]; shift: [nb][nseg] of this
// launch's bins, every entry in 0 .. 2047; out / nbr: [bin0 + bin][sv]; rows (optional):
// [sv][nbins][2048].  Grid (nsv, nb).
// Barriers per transform: one between writing the plane and reading it.  None is needed in front of
// the next transform: its first pass writes buffer 0, which every thread has finished reading
// before it wrote the plane, and its second pass writes buffer 1 (the plane) only behind the
// exchange barrier of the first, which no thread reaches before it has read its rotated values.
template <int A>
__global__ __launch_bounds__(256, 2) void acq_corr_array_kernel(
    const float2* __restrict__ spectra, const float2* __restrict__ rep, const int* __restrict__ slot,
    gpsmi_peak* __restrict__ out, int nsv, int nseg, int bin0, int nb, const float2* __restrict__ tw,
    float2* __restrict__ nbr, const int* __restrict__ shift, float* __restrict__ rows, int nbins) {
    static_assert(A >= 2 && A <= 4, "2 .. 4 antennas");
    constexpr int NP = A * (A - 1) / 2;
    // At A = 4 the transform of the last antenna would run beside 104 accumulators, 48 registers of
    // the earlier antennas' values, the replica and the next spectrum: more than the 256 registers
    // of two waves per SIMD.  The values of antennas 0 and 1 therefore wait in LDS, each thread's
    // own eight where it alone writes and reads them (no barrier), 32 KiB: 72 KiB per workgroup
    // still leaves two workgroups per CU.
    constexpr int STASH = A == 4 ? 2 : 0;
    __shared__ float2 stash[STASH ? STASH * kFftN : 1];
    __shared__ __attribute__((aligned(16))) float lds[kFftLdsFloats];
    __shared__ __attribute__((aligned(16))) float red[kStatsRedFloats];
    __shared__ __attribute__((aligned(16))) float lds_tw[kFftTwFloats];
    float* magbuf = lds + 2 * kFftPlane;                       // buffer 1: the statistics' copy of T
    float2* plane = reinterpret_cast<float2*>(magbuf);         // ... and, before that, a transform's output
    static_assert(kFftN <= kFftPlane1, "the complex plane must fit buffer 1");
    const int t = threadIdx.x, sv = blockIdx.x, bin = blockIdx.y;
    const FftTw ftw = fft_setup(lds_tw, tw, t);
    const size_t row_stride = (size_t)nb * nseg * kFftN;       // from one antenna's spectra to the next's
    const float2* X = spectra + (size_t)bin * nseg * kFftN;
    const float2* R = rep + (size_t)slot[sv] * kFftN;
    const int* M = shift + (size_t)bin * nseg;
    float2 x[8], r[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        x[q] = X[t + 256 * q];
        r[q] = R[t + 256 * q];
    }
    float d[8];
    float2 rr[NP][8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        d[q] = 0.f;
#pragma unroll
        for (int p = 0; p < NP; ++p) rr[p][q] = make_float2(0.f, 0.f);
    }
    __syncthreads();                                           // the twiddle tables are written
#pragma unroll 1
    for (int s = 0; s < nseg; ++s) {
        const int m = __builtin_amdgcn_readfirstlane(M[s]);
        float2 c[A][8];                        // (rows below STASH are never kept: they go to the stash)
#pragma unroll
        for (int a = 0; a < A; ++a) {
            float2 v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q)        // conj(x) * r
                v[q] = make_float2(x[q].x * r[q].x + x[q].y * r[q].y, x[q].x * r[q].y - x[q].y * r[q].x);
            // the next spectrum: the next antenna's of this segment, else antenna 0's of the next
            // segment (past the last one the last again, never used: no branch around the loads)
            const float2* Xn = a + 1 < A ? X + (size_t)(a + 1) * row_stride + (size_t)s * kFftN
                                         : X + (size_t)(s + 1 < nseg ? s + 1 : s) * kFftN;
#pragma unroll
            for (int q = 0; q < 8; ++q) x[q] = Xn[t + 256 * q];
            fft2048(v, lds, ftw, t);
#pragma unroll
            for (int q = 0; q < 8; ++q) plane[t + 256 * q] = v[q];
            lds_barrier();
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                // fft(conj Y)[n] = conj(N ifft(Y)[n]): same lag index, the conjugate taken back
                const float2 w = plane[(t + 256 * q + m) & (kFftN - 1)];
                c[a][q] = make_float2(w.x * (1.0f / kFftN), -w.y * (1.0f / kFftN));
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const float2 ca = c[a][q];
                if constexpr (STASH > 0)
                    if (a < STASH) stash[a * kFftN + t + 256 * q] = ca;
                d[q] += ca.x * ca.x + ca.y * ca.y;
#pragma unroll
                for (int b = 0; b < a; ++b) {                  // R_ba += c_b conj(c_a)
                    const float2 cb = b < STASH ? stash[b * kFftN + t + 256 * q] : c[b][q];
                    float2& acc = rr[array_pair<A>(b, a)][q];
                    acc.x += cb.x * ca.x + cb.y * ca.y;
                    acc.y += cb.y * ca.x - cb.x * ca.y;
                }
            }
        }
    }
    lds_barrier();                             // (the statistics write the plane the last reads came from)
    const float sc = 1.0f / (float)(A * nseg);
    float T[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        float cross = 0.f;
#pragma unroll
        for (int p = 0; p < NP; ++p)
            cross += __builtin_amdgcn_sqrtf(rr[p][q].x * rr[p][q].x + rr[p][q].y * rr[p][q].y);   // v_sqrt_f32, 1 ulp
        T[q] = (d[q] + 2.0f * cross) * sc;
    }
    if (rows) {                                // the surface the statistics below are formed of
        float* row = rows + ((size_t)sv * nbins + bin0 + bin) * kFftN;
#pragma unroll
        for (int q = 0; q < 8; ++q) row[t + 256 * q] = T[q];
    }
    int amax; float peak, mean, sd, lo, hi;
    corr_stats8(T, stats_sum8(T), t, magbuf, red, amax, peak, mean, sd, lo, hi);
    if (t == 0)
        acq_store_peak(out, nbr, (size_t)(bin0 + bin) * nsv + sv, amax, peak, mean, sd, lo, hi);
}

}  // namespace gpsmi
