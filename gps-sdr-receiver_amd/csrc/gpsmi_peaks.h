// Auxiliary correlation peaks per satellite over the surfaces of a deep search (gpsmi_acq_peaks,
// include/gpsmi.h; numpy restatement: tests/peaks_ref.py).  Kernels and their
// host-side plan; the entry points sit beside the acquisition handle in gpsmi_acq.hip.
//
//   peaks_stats_kernel  step a, first half: one 256-thread workgroup per (satellite, bin of the
//                       window).  mean and std of the row by col_row_stats (gpsmi_collective.h): the
//                       operations and the summation order of collective detection, one copy.
//   peaks_zmax_kernel   step a, second half: one wave per (satellite, 64 lags), a lane per lag, down
//                       the bins of the window in ascending order: zmax[l] and the smallest bin that
//                       attains it.  Lanes read consecutive lags of a row: coalesced; the quotient of
//                       every bin is formed and a skipped bin's dropped by a select, so that the reads
//                       of eight bins are in flight together.  A satellite all of whose bins are
//                       skipped gets bin -1 at every lag.
//   peaks_pick_kernel   step b: one 256-thread workgroup per satellite takes the k picks one after
//                       the other.  A pick is an argmax over the free lags: thread t scans lags t,
//                       t + 256, ... in ascending order, the waves reduce by lane exchange, the four
//                       wave results meet in LDS.  Between equal values the smaller lag wins at every
//                       stage, so the result is the first index of the maximum whatever the order of
//                       the exchange.  Whether a lag is free is computed from the picks before it (at
//                       most seven), not kept as a mask.  zmax stays in L2 (64 KiB a satellite at
//                       16368): k passes over it cost less than the statistics' one read of the rows.
//                       Then the columns: a thread per bin reads S[b][lag].
//
// Races: every workgroup writes cells of its own (statistics: its (satellite, bin); zmax: its 64 lags;
// picks: its satellite), every cell from one thread; the three kernels follow one another on the
// handle's stream.  No atomics, no communication between workgroups: two calls give the same bytes,
// and a satellite's picks do not depend on which other satellites share the call.
#pragma once
#include "gpsmi_collective.h"

namespace gpsmi {

constexpr int kPeaksMaxK = 8;
constexpr int kPeaksMaxRows = GPSMI_MAX_PRN + 1;
constexpr int kPeaksMaxBins = 4096;
constexpr int kPeaksLagTile = 64;                 // lags of a workgroup of peaks_zmax_kernel: one wave

struct PeaksPlan {
    int cs, nsv, nbins, k, guard, lo, hi;
    int workgroups;                               // of the statistics launch: one per satellite and bin of the window
    size_t scratch_bytes;                         // the statistics, zmax and its bins
};

// The checks of gpsmi_acq_peaks*, without a GPU.
inline int peaks_plan(int cs, int nsv_rows, int nbins, const gpsmi_peaks_cfg* c, PeaksPlan* pl) {
    const char* fn = "gpsmi_acq_peaks";
    if (!c) return fail(GPSMI_E_ARG, "%s: null argument", fn);
    if (cs != 2048 && cs != 16368)
        return fail(GPSMI_E_UNSUPPORTED, "%s: code_samples 2048 and 16368 only", fn);
    if (nsv_rows < 1 || nsv_rows > kPeaksMaxRows)
        return fail(GPSMI_E_ARG, "%s: nsv_rows out of range 1..%d", fn, kPeaksMaxRows);
    if (nbins < 1 || nbins > kPeaksMaxBins) return fail(GPSMI_E_ARG, "%s: nbins out of range 1..%d", fn, kPeaksMaxBins);
    if (c->k < 1 || c->k > kPeaksMaxK) return fail(GPSMI_E_ARG, "%s: k out of range 1..%d", fn, kPeaksMaxK);
    if (c->guard_lags < -1 || c->guard_lags > cs / 2)
        return fail(GPSMI_E_ARG, "%s: guard_lags must be -1 (two chips) or 0..code_samples / 2", fn);
    if (c->bin_lo < 0 || c->bin_lo > c->bin_hi || c->bin_hi >= nbins)
        return fail(GPSMI_E_ARG, "%s: bins must satisfy 0 <= bin_lo <= bin_hi < nbins", fn);
    if (pl) {
        pl->cs = cs; pl->nsv = nsv_rows; pl->nbins = nbins; pl->k = c->k;
        pl->guard = c->guard_lags < 0 ? (cs == 2048 ? 4 : 32) : c->guard_lags;    // two chips
        pl->lo = c->bin_lo; pl->hi = c->bin_hi;
        pl->workgroups = nsv_rows * (c->bin_hi - c->bin_lo + 1);
        pl->scratch_bytes = (size_t)nsv_rows * nbins * sizeof(float2) + (size_t)nsv_rows * cs * (sizeof(float) + sizeof(int));
    }
    return GPSMI_OK;
}

#pragma clang fp contract(off)

// stats: [nsv][nbins] (mean, std), written for the bins of the window alone
__global__ __launch_bounds__(256) void peaks_stats_kernel(const float* __restrict__ rows, int nbins, int cs, int lo,
                                                          float2* __restrict__ stats) {
    __shared__ float red[256];
    const int t = threadIdx.x, b = lo + blockIdx.x, p = blockIdx.y;
    const size_t cell = (size_t)p * nbins + b;
    float mean, sd;
    col_row_stats(rows + cell * cs, cs, 1.0f / (float)cs, red, t, mean, sd);
    if (t == 0) stats[cell] = make_float2(mean, sd);
}

__global__ __launch_bounds__(kPeaksLagTile) void peaks_zmax_kernel(const float* __restrict__ rows, int nbins, int cs,
                                                                   int lo, int hi, const float2* __restrict__ stats,
                                                                   float* __restrict__ zmax, int* __restrict__ zbin) {
    const int l = blockIdx.x * kPeaksLagTile + threadIdx.x, p = blockIdx.y;
    if (l >= cs) return;
    const float2* st = stats + (size_t)p * nbins;
    const float* S = rows + (size_t)p * nbins * cs + l;
    float best = 0.f;
    int bin = -1;
    // (no branch on the skipped bins, so that the reads of eight bins are in flight together: the
    // quotient of a skipped bin is formed and dropped)
#pragma unroll 8
    for (int b = lo; b <= hi; ++b) {
        const float2 ms = st[b];
        const float v = (S[(size_t)b * cs] - ms.x) / ms.y;
        const bool take = ms.y > 0.f && (bin < 0 || v > best);
        best = take ? v : best;
        bin = take ? b : bin;
    }
    zmax[(size_t)p * cs + l] = best;
    zbin[(size_t)p * cs + l] = bin;
}

// picks: [nsv][k]; cols: [nsv][k][2][nbins] or null
__global__ __launch_bounds__(256) void peaks_pick_kernel(const float* __restrict__ rows, int nbins, int cs, int k,
                                                         int guard, int lo, int hi, const float2* __restrict__ stats,
                                                         const float* __restrict__ zmax, const int* __restrict__ zbin,
                                                         gpsmi_peaks_pick* __restrict__ picks,
                                                         float* __restrict__ cols) {
    __shared__ float w_v[4];
    __shared__ int w_l[4];
    __shared__ int taken[kPeaksMaxK];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, p = blockIdx.x;
    const float* zp = zmax + (size_t)p * cs;
    const int* bp = zbin + (size_t)p * cs;
    const float* Sp = rows + (size_t)p * nbins * cs;
    const float2* st = stats + (size_t)p * nbins;
    const bool any = bp[0] >= 0;                  // (a skipped bin is skipped at every lag)
    for (int i = 0; i < k; ++i) {
        float bv = 0.f;
        int bl = -1;
        if (any)
#pragma unroll 4
            for (int l = t; l < cs; l += 256) {
                bool is_free = true;
                for (int j = 0; j < i; ++j) {
                    int d = l - taken[j];
                    d = d < 0 ? -d : d;
                    d = d < cs - d ? d : cs - d;
                    is_free = is_free && (taken[j] < 0 || d > guard);
                }
                const float v = zp[l];
                if (is_free && (bl < 0 || v > bv)) { bv = v; bl = l; }
            }
        for (int o = 32; o; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int ol = __shfl_xor(bl, o, 64);
            if (ol >= 0 && (bl < 0 || ov > bv || (ov == bv && ol < bl))) { bv = ov; bl = ol; }
        }
        if (lane == 0) { w_v[wave] = bv; w_l[wave] = bl; }
        __syncthreads();
        bv = w_v[0]; bl = w_l[0];
        for (int w = 1; w < 4; ++w) {
            const float ov = w_v[w];
            const int ol = w_l[w];
            if (ol >= 0 && (bl < 0 || ov > bv || (ov == bv && ol < bl))) { bv = ov; bl = ol; }
        }
        const int lag = bl;                       // (the same in every thread)
        const int bin = lag < 0 ? -1 : bp[lag];
        if (t == 0) {
            taken[i] = lag;
            gpsmi_peaks_pick pk;
            pk.lag = lag; pk.bin = bin;
            pk.z = lag < 0 ? 0.f : bv;
            pk.s = lag < 0 ? 0.f : Sp[(size_t)bin * cs + lag];
            picks[(size_t)p * k + i] = pk;
        }
        if (cols) {
            float* c0 = cols + ((size_t)p * k + i) * 2 * nbins;
            for (int b = t; b < nbins; b += 256) {
                float s = 0.f, z = 0.f;
                if (lag >= 0) {
                    s = Sp[(size_t)b * cs + lag];
                    if (b >= lo && b <= hi) {
                        const float2 ms = st[b];
                        if (ms.y > 0.f) z = (s - ms.x) / ms.y;
                    }
                }
                c0[b] = s;
                c0[nbins + b] = z;
            }
        }
        __syncthreads();                          // (taken[i] is written, w_v / w_l have been read)
    }
}

#pragma clang fp contract(fast)

}  // namespace gpsmi
