// Collective detection over the surfaces of a deep search (gpsmi_acq_collective, include/gpsmi.h;
// DESIGN.md 4.2k; numpy restatement: tests/collective_ref.py).  Kernels and their host-side plan; the
// entry points sit beside the acquisition handle in gpsmi_acq.hip.
//
//   collective_norm_kernel  step a: one 256-thread workgroup per satellite.  Per bin of its window the
//                           mean and the population std of the row (thread t sums lags t, t + 256, ...
//                           in ascending order, the 256 shares meet in an adjacent-pair tree: at 2048
//                           the order of gpsmi_stats.h), then z[l] = max over the bins of
//                           (S[l] - mean) / std.  A bin whose std is not positive is skipped; a
//                           satellite all of whose bins are skipped has z = 0 and adds nothing.
//   collective_pool_kernel  pool = w > 1: zw[l] = max_{k<w} z[(l + k) mod cs], into a second block.
//   collective_kernel       step b: one workgroup per tile of 64 grid points, a wave per 16 of them,
//                           a lane per clock lag.  Lanes read consecutive lags of a row, so LDS reads
//                           are conflict-free and global ones coalesced; the best lag of a point is
//                           found inside the wave that owns the point and written by its lane 0.
//
// What is held in LDS.  256 KiB of z rows at 32 satellites and 2048 lags exceed a CU's LDS, and the
// rows of 16368 never fit, so the kernel holds fewer bytes instead of taking satellites in groups:
// the clock lags are tiled.  The 64 points of a tile are neighbours on the grid, so for a chunk of
// clock lags c0 .. c0 + span - 1 satellite p is read only inside the window
//     floor(min_j base_pj) + c0 - 1  ..  floor(max_j base_pj) + c0 + span + 1
// (base_pj: x_p of point j at clock 0).  The windows of all satellites of one chunk share
// kColWinFloats floats; a workgroup whose windows do not fit (steep gradients across its tile, or a
// large pool step) reads the rows through L2 instead, with the same result.  The sum over the
// satellites stays in ascending p in one thread: no partial sums cross threads.
//
// Races: a workgroup writes the cells of its own tile, every cell from one lane; the three kernels
// follow one another on the handle's stream.  No atomics, no communication between workgroups.
#pragma once
#include <cmath>

#include "gpsmi_common.h"

namespace gpsmi {

constexpr int kColMaxSats = 32;
constexpr int kColMaxPool = 64;
constexpr int kColPoints = 64;                    // grid points of a workgroup: 16 per wave
constexpr int kColWavePoints = 16;
constexpr int kColWinFloats = 11264;              // 44 KiB of windows; with the bases 60 KiB: two workgroups per CU
constexpr long long kColMaxCells = 1ll << 22;     // grid points of a call (a 32 MiB cell map)
constexpr double kColMaxLag = 1073741824.0;       // |x_p| stays below 2^30: the index is an int32

struct ColPlan {
    int cs, nsat, pool;
    long long cells;
    int workgroups;
    size_t scratch_bytes;                         // the z rows, and the pooled ones beside them
};

// The checks of gpsmi_acq_collective*, without a GPU.
inline int collective_plan(int cs, int nsv_rows, int nbins, const gpsmi_collective_sat* sats, int nsat,
                           const gpsmi_collective_grid* g, ColPlan* pl) {
    const char* fn = "gpsmi_acq_collective";
    if (!sats || !g) return fail(GPSMI_E_ARG, "%s: null argument", fn);
    if (cs != 2048 && cs != 16368)
        return fail(GPSMI_E_UNSUPPORTED, "%s: code_samples 2048 and 16368 only", fn);
    if (nsv_rows < 1 || nsv_rows > GPSMI_MAX_PRN) return fail(GPSMI_E_ARG, "%s: nsv_rows out of range 1..37", fn);
    if (nbins < 1 || nbins > 65535) return fail(GPSMI_E_ARG, "%s: nbins out of range 1..65535", fn);
    if (nsat < 1 || nsat > kColMaxSats) return fail(GPSMI_E_ARG, "%s: nsat out of range 1..%d", fn, kColMaxSats);
    if (g->pool < 1 || g->pool > kColMaxPool) return fail(GPSMI_E_ARG, "%s: pool out of range 1..%d", fn, kColMaxPool);
    if (g->n_e < 1 || g->n_n < 1 || g->n_t < 1) return fail(GPSMI_E_ARG, "%s: a grid dimension below 1", fn);
    const double v[6] = {g->e0, g->n0, g->t0, g->d_e, g->d_n, g->d_t};
    for (double x : v)
        if (!std::isfinite(x)) return fail(GPSMI_E_ARG, "%s: the grid must be finite", fn);
    if ((double)g->n_e * g->n_n * g->n_t > (double)kColMaxCells)
        return fail(GPSMI_E_UNSUPPORTED, "%s: more than %lld grid points in one call (split the grid)", fn,
                    kColMaxCells);
    const long long cells = (long long)g->n_e * g->n_n * g->n_t;
    // the farthest a coordinate gets from 0
    auto far = [](double x0, double d, int n) { return std::fmax(std::fabs(x0), std::fabs(x0 + d * (n - 1))); };
    const double fe = far(g->e0, g->d_e, g->n_e), fn_ = far(g->n0, g->d_n, g->n_n), ft = far(g->t0, g->d_t, g->n_t);
    for (int p = 0; p < nsat; ++p) {
        const gpsmi_collective_sat& s = sats[p];
        if (s.row < 0 || s.row >= nsv_rows) return fail(GPSMI_E_ARG, "%s: satellite %d: row out of range", fn, p);
        if (s.bin_lo < 0 || s.bin_lo > s.bin_hi || s.bin_hi >= nbins)
            return fail(GPSMI_E_ARG, "%s: satellite %d: bins must satisfy 0 <= bin_lo <= bin_hi < nbins", fn, p);
        if (!std::isfinite(s.lag0) || !std::isfinite(s.g_e) || !std::isfinite(s.g_n) || !std::isfinite(s.g_t))
            return fail(GPSMI_E_ARG, "%s: satellite %d: lag0 and the gradients must be finite", fn, p);
        const double reach = std::fabs(s.lag0) + std::fabs(s.g_e) * fe + std::fabs(s.g_n) * fn_ +
                             std::fabs(s.g_t) * ft + (double)cs;
        if (!(reach < kColMaxLag))
            return fail(GPSMI_E_ARG, "%s: satellite %d: predicted lags reach 2^30 samples", fn, p);
    }
    if (pl) {
        pl->cs = cs; pl->nsat = nsat; pl->pool = g->pool; pl->cells = cells;
        pl->workgroups = (int)((cells + kColPoints - 1) / kColPoints);
        pl->scratch_bytes = (size_t)nsat * cs * sizeof(float) * (g->pool > 1 ? 2 : 1);
    }
    return GPSMI_OK;
}

#pragma clang fp contract(off)

// sum of the 256 threads' shares in the order of an adjacent-pair tree, in every thread
__device__ __forceinline__ float col_tree_sum(float v, float* red, int t) {
    __syncthreads();                              // (the previous sum has been read)
    red[t] = v;
    __syncthreads();
    for (int s = 1; s < 256; s *= 2) {
        if ((t & (2 * s - 1)) == 0) red[t] = red[t] + red[t + s];
        __syncthreads();
    }
    return red[0];
}

// mean and population std of one surface S[cs] as step a forms them, in every thread of a 256-thread
// workgroup (inv = 1 / cs): the one copy, shared with gpsmi_peaks.h
__device__ __forceinline__ void col_row_stats(const float* __restrict__ S, int cs, float inv, float* red, int t,
                                              float& mean, float& sd) {
    float a = 0.f;
    for (int l = t; l < cs; l += 256) a = a + S[l];
    mean = col_tree_sum(a, red, t) * inv;
    a = 0.f;
    for (int l = t; l < cs; l += 256) { const float d = S[l] - mean; a = a + d * d; }
    sd = sqrtf(col_tree_sum(a, red, t) * inv);    // (correctly rounded, as the divisions by it)
}

__global__ __launch_bounds__(256) void collective_norm_kernel(const float* __restrict__ rows, int nbins, int cs,
                                                              const gpsmi_collective_sat* __restrict__ sats,
                                                              float* __restrict__ z) {
    __shared__ float red[256];
    const int t = threadIdx.x, p = blockIdx.x;
    const gpsmi_collective_sat sat = sats[p];
    float* zp = z + (size_t)p * cs;
    const float inv = 1.0f / (float)cs;
    bool any = false;
    for (int b = sat.bin_lo; b <= sat.bin_hi; ++b) {
        const float* S = rows + ((size_t)sat.row * nbins + b) * cs;
        float mean, sd;
        col_row_stats(S, cs, inv, red, t, mean, sd);
        if (!(sd > 0.f)) continue;                // (the same in every thread)
        for (int l = t; l < cs; l += 256) {
            const float v = (S[l] - mean) / sd;
            zp[l] = any ? fmaxf(zp[l], v) : v;
        }
        any = true;
    }
    if (!any)
        for (int l = t; l < cs; l += 256) zp[l] = 0.f;
}

__global__ __launch_bounds__(256) void collective_pool_kernel(const float* __restrict__ z, int cs, int w,
                                                              float* __restrict__ zw) {
    const int l = blockIdx.x * 256 + threadIdx.x, p = blockIdx.y;
    if (l >= cs) return;
    const float* zp = z + (size_t)p * cs;
    float m = zp[l];
    int i = l;
    for (int k = 1; k < w; ++k) {
        i = i + 1 == cs ? 0 : i + 1;
        m = fmaxf(m, zp[i]);
    }
    zw[(size_t)p * cs + l] = m;
}

// z: the rows the sums are taken from, [nsat][cs] (pooled where pool > 1).  out: [n_t][n_n][n_e].
__global__ __launch_bounds__(256) void collective_kernel(const float* __restrict__ z,
                                                         const gpsmi_collective_sat* __restrict__ sats, int nsat,
                                                         gpsmi_collective_grid g, int cs, int npoints,
                                                         gpsmi_collective_cell* __restrict__ out) {
    __shared__ float win[kColWinFloats];
    __shared__ double base[kColMaxSats * kColPoints];     // [p][j]
    __shared__ int s_lo[kColMaxSats], s_hi[kColMaxSats];  // floor of the smallest / largest base of p
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int tile0 = blockIdx.x * kColPoints;
    for (int idx = t; idx < nsat * kColPoints; idx += 256) {
        const int p = idx >> 6, j = idx & 63;
        int pt = tile0 + j;
        pt = pt < npoints ? pt : npoints - 1;             // (past the grid: the last point again, never stored)
        const int ie = pt % g.n_e, in = (pt / g.n_e) % g.n_n, it = pt / (g.n_e * g.n_n);
        const double E = g.e0 + (double)ie * g.d_e, N = g.n0 + (double)in * g.d_n, T = g.t0 + (double)it * g.d_t;
        const gpsmi_collective_sat s = sats[p];
        base[idx] = s.lag0 + s.g_e * E + s.g_n * N + s.g_t * T;
    }
    __syncthreads();
    for (int p = wave; p < nsat; p += 4) {
        double lo = base[p * kColPoints + lane], hi = lo;
        for (int o = 32; o; o >>= 1) {
            lo = fmin(lo, __shfl_xor(lo, o, 64));
            hi = fmax(hi, __shfl_xor(hi, o, 64));
        }
        if (lane == 0) { s_lo[p] = (int)floor(lo); s_hi[p] = (int)floor(hi); }
    }
    __syncthreads();
    const int w = g.pool, ncl = (cs + w - 1) / w;         // the clock lags are c = w k, k < ncl
    const int rounds = 4 / w > 0 ? 4 / w : 1;             // rounds of 64 clock lags per chunk
    const int span = (64 * rounds - 1) * w + 1;           // lags from a chunk's first clock lag to its last
    const int W = kColWinFloats / nsat;
    bool fits = true;
    for (int p = 0; p < nsat; ++p) fits = fits && s_hi[p] - s_lo[p] + span + 4 <= W;
    float best[kColWavePoints];
    int bestc[kColWavePoints];
#pragma unroll
    for (int q = 0; q < kColWavePoints; ++q) { best[q] = -INFINITY; bestc[q] = 0; }
    for (int k0 = 0; k0 < ncl; k0 += 64 * rounds) {
        const int c0 = k0 * w;
        if (fits) {
            __syncthreads();                              // (the previous chunk's windows have been read)
            for (int p = 0; p < nsat; ++p) {
                const int width = s_hi[p] - s_lo[p] + span + 4;
                int m0 = (s_lo[p] + c0 - 1) % cs;
                m0 += m0 < 0 ? cs : 0;
                const float* zp = z + (size_t)p * cs;
                for (int k = t; k < width; k += 256) win[p * W + k] = zp[(m0 + k) % cs];
            }
            __syncthreads();
        }
        for (int r = 0; r < rounds; ++r) {
            int k = k0 + 64 * r + lane;
            const bool valid = k < ncl;
            k = valid ? k : ncl - 1;                      // (a lane past the last lag repeats it, and is not counted)
            const int c = k * w;
            const double cd = (double)c;
            float score[kColWavePoints];
            for (int p = 0; p < nsat; ++p) {
                const double* bp = base + p * kColPoints + wave * kColWavePoints;
                const int w0 = s_lo[p] + c0 - 1;
                const float* zp = z + (size_t)p * cs;
                const float* wp = win + p * W;
#pragma unroll
                for (int q = 0; q < kColWavePoints; ++q) {
                    const double x = bp[q] + cd;
                    const int i = (int)floor(x + 0.5);
                    float v;
                    if (fits) {
                        v = wp[i - w0];
                    } else {
                        int m = i % cs;
                        m += m < 0 ? cs : 0;
                        v = zp[m];
                    }
                    score[q] = p == 0 ? v : score[q] + v;
                }
            }
#pragma unroll
            for (int q = 0; q < kColWavePoints; ++q)
                if (valid && score[q] > best[q]) { best[q] = score[q]; bestc[q] = c; }
        }
    }
    // the best lag of every point of this wave: the largest score, between equal ones the smallest lag
#pragma unroll
    for (int q = 0; q < kColWavePoints; ++q) {
        float s = best[q];
        int c = bestc[q];
        for (int o = 32; o; o >>= 1) {
            const float os = __shfl_xor(s, o, 64);
            const int oc = __shfl_xor(c, o, 64);
            if (os > s || (os == s && oc < c)) { s = os; c = oc; }
        }
        const int pt = tile0 + wave * kColWavePoints + q;
        if (lane == 0 && pt < npoints) {
            gpsmi_collective_cell cell; cell.score = s; cell.lag = c;
            out[pt] = cell;
        }
    }
}

#pragma clang fp contract(fast)

}  // namespace gpsmi
