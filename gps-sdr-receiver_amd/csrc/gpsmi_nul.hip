// Null steering (power inversion) over A coherent antennas, ahead of everything else (gpsmi_nul_*,
// include/gpsmi.h; float64 restatement: tests/nul_ref.py).
//
// Per block of n samples, alone: the A x A covariance of the antennas in float64 (the products of
// float32 samples are exact there), R = C / n + delta I, R u = e0 by Cholesky, w = u / u[0], and the
// output y = sum_a conj(w32[a]) x_a in float32; a block whose predicted gain is below min_gain_db (or
// whose R has no Cholesky factor) passes antenna 0 through.  With cfg.taps = 3, 5 or 7 every antenna has a
// filter of that many taps instead: the kernels of gpsmi_nul_stap.h, dispatched from nul_run below.
//
//   nul_cov_kernel<FMT, A>    one workgroup per (block, slice of 8192 samples): lane t takes the samples
//                             2048 r + 8 t .. + 7, r = 0 .. 3, as b128 loads (two complex64 or
//                             eight raw samples per load and antenna), A (A + 1) / 2 complex float64
//                             accumulators in registers, then the 256 lane sums as a tree of
//                             neighbours: six levels of lane swaps in the wave, two over the four
//                             waves through LDS -> part[block][slice][A (A + 1)].  No atomics.
//   nul_solve_kernel<A>       one workgroup per block: thread v adds value v of the slice sums in
//                             ascending slice order, thread 0 loads, factors, solves and decides
//                             (A <= 8: a few hundred float64 operations) -> w32, weights, flag, gain.
//   nul_apply_kernel<FMT, A>  a streaming pass: two (complex64) or eight (raw) samples per thread,
//                             w32 and the flag in SGPRs (uniform loads), one float4 store per sample
//                             pair; a pass-through block copies antenna 0.
//
// The order of every float64 sum is fixed by n alone (the slice and the lane a sample falls to), so
// the output does not depend on the grid, on nb or on how the input is cut into calls.  The float64
// fused multiply-adds of the covariance are products that are exact before the add: they round as a
// multiply and an add would.  The solve and the apply are compiled with contraction off.
#include <cmath>

#include "gpsmi_common.h"
#include "gpsmi_stage.h"

namespace gpsmi {

constexpr int kNulSlice = 8192;                      // samples per workgroup of the covariance
constexpr int kNulGroup = 8;                         // consecutive samples a lane takes at a time
constexpr int kNulThreads = 256;
constexpr int kNulMaxA = 8;
constexpr int kNulApplyC64 = 2, kNulApplyU8 = 8;     // samples per thread of the apply

// values of a covariance: pair p = a (a + 1) / 2 + b (a >= b), re at 2 p, im at 2 p + 1
__host__ __device__ constexpr int nul_values(int A) { return A * (A + 1); }

// is value v the imaginary part of a diagonal element (pair a (a + 1) / 2 + a)?
__host__ __device__ constexpr bool nul_diag_im(int v) {
    for (int a = 0; a < kNulMaxA; ++a)
        if (v == 2 * (a * (a + 3) / 2) + 1) return true;
    return false;
}

// 16 bytes of raw samples, 4-byte aligned
typedef uint32_t nul_u32x4 __attribute__((ext_vector_type(4), aligned(4)));

template <int A>
__device__ __forceinline__ void nul_accumulate(double (&acc)[nul_values(A)], const float2 (&x)[A]) {
    double xr[A], xi[A];
#pragma unroll
    for (int a = 0; a < A; ++a) {
        xr[a] = (double)x[a].x;
        xi[a] = (double)x[a].y;
    }
#pragma unroll
    for (int a = 0; a < A; ++a) {
#pragma unroll
        for (int b = 0; b <= a; ++b) {
            const int p = a * (a + 1) / 2 + b;
            acc[2 * p] = fma(xr[a], xr[b], acc[2 * p]);
            acc[2 * p] = fma(xi[a], xi[b], acc[2 * p]);
            if (a != b) {                             // (the diagonal's imaginary part is exactly 0)
                acc[2 * p + 1] = fma(xi[a], xr[b], acc[2 * p + 1]);
                acc[2 * p + 1] = fma(-xr[a], xi[b], acc[2 * p + 1]);
            }
        }
    }
}

// iq: [A][astride] samples of the call; block b of antenna a starts at a * astride + b * n
template <int FMT, int A>
__global__ __launch_bounds__(kNulThreads) void nul_cov_kernel(const void* __restrict__ iq, int n, int ns,
                                                              size_t astride, double* __restrict__ part) {
    constexpr int NV = nul_values(A);
    __shared__ double red[4][NV];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int b = blockIdx.x / ns, s = blockIdx.x % ns;
    const int i0 = s * kNulSlice, len = min(kNulSlice, n - i0);    // (a multiple of 32)
    const size_t base = (size_t)b * n + i0;
    double acc[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = 0.0;
    for (int o = kNulGroup * t; o < len; o += kNulGroup * kNulThreads) {
        if constexpr (FMT == 0) {
            const float2* src = static_cast<const float2*>(iq) + base + o;
#pragma unroll
            for (int q = 0; q < kNulGroup; q += 2) {
                float4 v[A];
#pragma unroll
                for (int a = 0; a < A; ++a) v[a] = *reinterpret_cast<const float4*>(src + a * astride + q);
                float2 x[A];
#pragma unroll
                for (int a = 0; a < A; ++a) x[a] = make_float2(v[a].x, v[a].y);
                nul_accumulate<A>(acc, x);
#pragma unroll
                for (int a = 0; a < A; ++a) x[a] = make_float2(v[a].z, v[a].w);
                nul_accumulate<A>(acc, x);
            }
        } else {
            const uint16_t* src = static_cast<const uint16_t*>(iq) + base + o;
            nul_u32x4 v[A];
#pragma unroll
            for (int a = 0; a < A; ++a) v[a] = *reinterpret_cast<const nul_u32x4*>(src + a * astride);
#pragma unroll
            for (int q = 0; q < kNulGroup; ++q) {
                float2 x[A];
#pragma unroll
                for (int a = 0; a < A; ++a) {
                    const uint32_t w = v[a][q / 2];
                    x[a] = decode_u8iq(q % 2 ? w >> 16 : w & 0xFFFFu);
                }
                nul_accumulate<A>(acc, x);
            }
        }
    }
    // lanes 2k + (2k + 1), then pairs of those, ...: six levels in the wave, two over the waves
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        if (nul_diag_im(v)) continue;                 // (zero in every lane)
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) acc[v] += __shfl_xor(acc[v], off);
    }
    if (lane == 0) {
#pragma unroll
        for (int v = 0; v < NV; ++v) red[wave][v] = acc[v];
    }
    __syncthreads();
    if (t < NV) part[(size_t)blockIdx.x * NV + t] = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
}

#pragma clang fp contract(off)
struct NulZ { double re, im; };
__device__ __forceinline__ NulZ nul_mul(NulZ a, NulZ b) {             // a * b
    return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
}
__device__ __forceinline__ NulZ nul_conj(NulZ a) { return {a.re, -a.im}; }
__device__ __forceinline__ NulZ nul_sub(NulZ a, NulZ b) { return {a.re - b.re, a.im - b.im}; }

// w32: [nb][8] (A used), w64: [nb][A][2]
template <int A>
__global__ __launch_bounds__(128) void nul_solve_kernel(const double* __restrict__ part, int n, int ns,
                                                        double load, double min_db,
                                                        float2* __restrict__ w32, double* __restrict__ w64,
                                                        int32_t* __restrict__ flags, float* __restrict__ gain) {
    constexpr int NV = nul_values(A);
    __shared__ double Cs[NV];
    const int t = threadIdx.x, b = blockIdx.x;
    if (t < NV) {
        const double* src = part + (size_t)b * ns * NV + t;
        double c = src[0];
        for (int s = 1; s < ns; ++s) c += src[(size_t)s * NV];
        Cs[t] = c;
    }
    __syncthreads();
    if (t != 0) return;
    const double dn = (double)n;
    NulZ R[A][A];                                      // lower triangle
    double tr = 0.0;
#pragma unroll
    for (int a = 0; a < A; ++a) {
#pragma unroll
        for (int c = 0; c <= a; ++c) {
            const int p = a * (a + 1) / 2 + c;
            R[a][c] = {Cs[2 * p] / dn, a == c ? 0.0 : Cs[2 * p + 1] / dn};
        }
        tr += R[a][a].re;
    }
    const double p00 = R[0][0].re;
    const double delta = load * tr / (double)A;
#pragma unroll
    for (int a = 0; a < A; ++a) R[a][a].re += delta;
    // R = L L^H, column by column
    NulZ L[A][A];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < A; ++j) {
        double d = R[j][j].re;
#pragma unroll
        for (int k = 0; k < j; ++k) d -= L[j][k].re * L[j][k].re + L[j][k].im * L[j][k].im;
        if (!(d > 0.0) || !(d < INFINITY)) ok = false;
        const double l = sqrt(d);
        L[j][j] = {l, 0.0};
#pragma unroll
        for (int i = j + 1; i < A; ++i) {
            NulZ v = R[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) v = nul_sub(v, nul_mul(L[i][k], nul_conj(L[j][k])));
            L[i][j] = {v.re / l, v.im / l};
        }
    }
    NulZ y[A], u[A];
    y[0] = {1.0 / L[0][0].re, 0.0};
#pragma unroll
    for (int i = 1; i < A; ++i) {
        NulZ v = {0.0, 0.0};
#pragma unroll
        for (int k = 0; k < i; ++k) v = nul_sub(v, nul_mul(L[i][k], y[k]));
        y[i] = {v.re / L[i][i].re, v.im / L[i][i].re};
    }
#pragma unroll
    for (int i = A - 1; i >= 0; --i) {
        NulZ v = y[i];
#pragma unroll
        for (int k = i + 1; k < A; ++k) v = nul_sub(v, nul_mul(nul_conj(L[k][i]), u[k]));
        u[i] = {v.re / L[i][i].re, v.im / L[i][i].re};
    }
    double gdb = 0.0;
    if (ok) {
        gdb = 10.0 * log10(p00 * u[0].re);
        if (!(gdb >= min_db)) ok = false;              // (a NaN passes through as well)
    }
    flags[b] = ok ? 1 : 0;
    gain[b] = (float)gdb;
#pragma unroll
    for (int a = 0; a < A; ++a) {
        NulZ w = {a == 0 ? 1.0 : 0.0, 0.0};
        if (ok && a > 0) w = {u[a].re / u[0].re, u[a].im / u[0].re};
        w64[((size_t)b * A + a) * 2] = w.re;
        w64[((size_t)b * A + a) * 2 + 1] = w.im;
        w32[(size_t)b * kNulMaxA + a] = make_float2((float)w.re, (float)w.im);
    }
}

// y += conj(w) x: two products and one add / subtract per component, then one add into y
__device__ __forceinline__ float2 nul_term(float2 w, float2 x) {
    return make_float2(add_rn(mul_rn(w.x, x.x), mul_rn(w.y, x.y)), sub_rn(mul_rn(w.x, x.y), mul_rn(w.y, x.x)));
}
__device__ __forceinline__ float2 nul_add(float2 y, float2 z) { return make_float2(add_rn(y.x, z.x), add_rn(y.y, z.y)); }
#pragma clang fp contract(fast)

template <int FMT, int A>
__global__ __launch_bounds__(kNulThreads) void nul_apply_kernel(const void* __restrict__ iq, int n, int nc,
                                                                size_t astride,
                                                                const float2* __restrict__ w32,
                                                                const int32_t* __restrict__ flags,
                                                                float2* __restrict__ out) {
    constexpr int V = FMT == 0 ? kNulApplyC64 : kNulApplyU8;
    const int b = blockIdx.x / nc, c = blockIdx.x % nc;
    const int i = (c * kNulThreads + (int)threadIdx.x) * V;
    if (i >= n) return;                                // (n is a multiple of 32: whole groups)
    const size_t at = (size_t)b * n + i;
    const bool on = flags[b] != 0;
    float2 w[A];
#pragma unroll
    for (int a = 0; a < A; ++a) w[a] = w32[(size_t)b * kNulMaxA + a];
    float2 y[V];
    if constexpr (FMT == 0) {
        const float2* src = static_cast<const float2*>(iq) + at;
        const float4 v0 = *reinterpret_cast<const float4*>(src);
        y[0] = make_float2(v0.x, v0.y);
        y[1] = make_float2(v0.z, v0.w);
        if (on) {
            y[0] = nul_term(w[0], y[0]);
            y[1] = nul_term(w[0], y[1]);
#pragma unroll
            for (int a = 1; a < A; ++a) {
                const float4 v = *reinterpret_cast<const float4*>(src + a * astride);
                y[0] = nul_add(y[0], nul_term(w[a], make_float2(v.x, v.y)));
                y[1] = nul_add(y[1], nul_term(w[a], make_float2(v.z, v.w)));
            }
        }
    } else {
        const uint16_t* src = static_cast<const uint16_t*>(iq) + at;
        const nul_u32x4 v0 = *reinterpret_cast<const nul_u32x4*>(src);
#pragma unroll
        for (int q = 0; q < V; ++q) y[q] = decode_u8iq(q % 2 ? v0[q / 2] >> 16 : v0[q / 2] & 0xFFFFu);
        if (on) {
#pragma unroll
            for (int q = 0; q < V; ++q) y[q] = nul_term(w[0], y[q]);
#pragma unroll
            for (int a = 1; a < A; ++a) {
                const nul_u32x4 v = *reinterpret_cast<const nul_u32x4*>(src + a * astride);
#pragma unroll
                for (int q = 0; q < V; ++q)
                    y[q] = nul_add(y[q], nul_term(w[a], decode_u8iq(q % 2 ? v[q / 2] >> 16 : v[q / 2] & 0xFFFFu)));
            }
        }
    }
#pragma unroll
    for (int q = 0; q < V; q += 2)
        *reinterpret_cast<float4*>(out + at + q) = make_float4(y[q].x, y[q].y, y[q + 1].x, y[q + 1].y);
}

}  // namespace gpsmi

#include "gpsmi_nul_stap.h"

using namespace gpsmi;

struct gpsmi_nul {
    gpsmi_nul_cfg cfg;
    DevBuf<double> d_part;                                // [blocks][slices][A (A + 1)] (taps: stap_values)
    DevBuf<float2> d_w32;                                 // [blocks][8] (taps: [blocks][56])
    DevBuf<double> d_w64;                                 // [blocks][A][2] (taps: [blocks][A][T][2])
    DevBuf<int32_t> d_flags; DevBuf<float> d_gain;        // [blocks]
    double load = 0.0, min_db = 0.0;                      // the cfg's, defaults filled in
    int taps = 1;                                         // 1: one weight per antenna, else 3, 5 or 7
    DevEvent ev_cov, ev_solve;                            // stamps behind the first and the second kernel
    float kernel_ms[3] = {0.f, 0.f, 0.f};                 // covariance, solve, apply of the last finished call
    BlockStage blk;
    StageSync sync;                                       // last: see gpsmi_stage.h
};

static int nul_build(gpsmi_nul* h) {
    h->blk.block_samples = h->cfg.block_samples;
    h->blk.fan_in = h->cfg.antennas;
    h->load = (double)(h->cfg.load == 0.f ? 1e-6f : h->cfg.load);
    h->min_db = (double)(h->cfg.min_gain_db == 0.f ? 3.0f : h->cfg.min_gain_db);
    h->taps = h->cfg.taps <= 1 ? 1 : h->cfg.taps;
    int rc = h->ev_cov.create<Ev::StageStamp, EventScope::DeviceOnly>();
    if (!rc) rc = h->ev_solve.create<Ev::StageStamp, EventScope::DeviceOnly>();
    return rc;
}

// The three passes over nb blocks of every antenna at d_iq (device, the handle's input format) into d_out.
static int nul_run(gpsmi_nul* h, const void* d_iq, void* d_out, int nb) {
    const int n = h->cfg.block_samples, A = h->cfg.antennas, T = h->taps;
    const int ns = (n + kNulSlice - 1) / kNulSlice;
    const size_t astride = (size_t)nb * n;
    int rc = h->d_part.reserve((size_t)nb * ns * stap_values(A, T), "null steering slice sums");   // (T = 1: nul_values)
    if (!rc) rc = h->d_w32.reserve((size_t)nb * (T == 1 ? kNulMaxA : kStapMaxK), "null steering results");
    if (!rc) rc = h->d_w64.reserve((size_t)nb * A * T * 2, "null steering results");
    if (!rc) rc = h->d_flags.reserve(nb, "null steering results");
    if (!rc) rc = h->d_gain.reserve(nb, "null steering results");
    if (rc) return rc;
    const hipStream_t st = h->sync.stream;
    float2* out = static_cast<float2*>(d_out);
    if ((rc = h->sync.begin())) return rc;
    with_fmt(h->blk.fmt, [&](auto fmt) {
        constexpr int FMT = decltype(fmt)::value;
        constexpr int V = FMT == 0 ? kNulApplyC64 : kNulApplyU8;
        const int nc = (n + kNulThreads * V - 1) / (kNulThreads * V);
        if (T > 1) {
            with_value<3, 5, 7>(T, [&](auto nt) {
                constexpr int NT = decltype(nt)::value;
                hipLaunchKernelGGL((stap_cov_kernel<FMT, NT>), dim3((unsigned)(nb * ns)), dim3(kNulThreads), 0, st,
                                   d_iq, n, ns, A, astride, h->d_part.p);
                (void)hipEventRecord(h->ev_cov, st);
                hipLaunchKernelGGL(stap_solve_kernel, dim3((unsigned)nb), dim3(64), 0, st, h->d_part.p, n, ns, A,
                                   NT, h->load, h->min_db, h->d_w32.p, h->d_w64.p, h->d_flags.p, h->d_gain.p);
                (void)hipEventRecord(h->ev_solve, st);
                hipLaunchKernelGGL((stap_apply_kernel<FMT, NT>), dim3((unsigned)(nb * nc)), dim3(kNulThreads), 0,
                                   st, d_iq, n, nc, A, astride, h->d_w32.p, h->d_flags.p, out);
            });
            return;
        }
        with_value<2, 3, 4, 5, 6, 7, 8>(A, [&](auto na) {
            constexpr int NA = decltype(na)::value;
            hipLaunchKernelGGL((nul_cov_kernel<FMT, NA>), dim3((unsigned)(nb * ns)), dim3(kNulThreads), 0, st,
                               d_iq, n, ns, astride, h->d_part.p);
            (void)hipEventRecord(h->ev_cov, st);
            hipLaunchKernelGGL(nul_solve_kernel<NA>, dim3((unsigned)nb), dim3(128), 0, st, h->d_part.p, n, ns,
                               h->load, h->min_db, h->d_w32.p, h->d_w64.p, h->d_flags.p, h->d_gain.p);
            (void)hipEventRecord(h->ev_solve, st);
            hipLaunchKernelGGL((nul_apply_kernel<FMT, NA>), dim3((unsigned)(nb * nc)), dim3(kNulThreads), 0, st,
                               d_iq, n, nc, astride, h->d_w32.p, h->d_flags.p, out);
        });
    });
    return h->sync.end();
}

static int nul_finish(gpsmi_nul* h, int nb, int32_t* flags, float* gain_db, double* weights) {
    const hipStream_t st = h->sync.stream;
    if (flags)
        GPSMI_HIP(hipMemcpyAsync(flags, h->d_flags.p, (size_t)nb * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (gain_db)
        GPSMI_HIP(hipMemcpyAsync(gain_db, h->d_gain.p, (size_t)nb * sizeof(float), hipMemcpyDeviceToHost, st));
    if (weights)
        GPSMI_HIP(hipMemcpyAsync(weights, h->d_w64.p, (size_t)nb * h->cfg.antennas * h->taps * 2 * sizeof(double),
                                 hipMemcpyDeviceToHost, st));
    const int rc = h->sync.finish();
    if (rc) return rc;
    GPSMI_HIP(hipEventElapsedTime(&h->kernel_ms[0], h->sync.ev0, h->ev_cov));
    GPSMI_HIP(hipEventElapsedTime(&h->kernel_ms[1], h->ev_cov, h->ev_solve));
    GPSMI_HIP(hipEventElapsedTime(&h->kernel_ms[2], h->ev_solve, h->sync.ev1));
    return GPSMI_OK;
}

extern "C" {

int gpsmi_nul_create(const gpsmi_nul_cfg* cfg, gpsmi_nul** out) {
    GPSMI_REQUIRE(cfg && out, "null argument");
    *out = nullptr;
    const int32_t n = cfg->block_samples;
    GPSMI_REQUIRE(n >= 2048 && n <= (1 << 24) && n % 32 == 0,
                  "block_samples is not a multiple of 32 in 2048..2^24");
    GPSMI_REQUIRE(cfg->antennas >= 2 && cfg->antennas <= kNulMaxA, "antennas out of range 2..8");
    GPSMI_REQUIRE(cfg->load >= 0.f && std::isfinite(cfg->load), "load is negative, NaN or infinite");
    GPSMI_REQUIRE(cfg->min_gain_db >= 0.f && std::isfinite(cfg->min_gain_db),
                  "min_gain_db is negative, NaN or infinite");
    GPSMI_REQUIRE(cfg->taps == 0 || cfg->taps == 1 || cfg->taps == 3 || cfg->taps == 5 || cfg->taps == 7,
                  "taps is not 0, 1, 3, 5 or 7");
    return stage_create(cfg, out, nul_build);
}

int gpsmi_nul_destroy(gpsmi_nul* h) { return stage_destroy(h); }

int gpsmi_nul_set_input_format(gpsmi_nul* h, int fmt) { return stage_set_input_format(h, fmt, __func__); }

int gpsmi_nul_apply_dev(gpsmi_nul* h, const void* d_iq, void* d_out, int nb, int32_t* flags, float* gain_db,
                        double* weights) {
    int rc = stage_check_call(h, d_iq, d_out, nb, __func__, "null steering", true);
    if (rc) return rc;
    GPSMI_HIP(hipSetDevice(h->cfg.device));
    rc = nul_run(h, d_iq, d_out, nb);
    if (rc) return rc;
    return nul_finish(h, nb, flags, gain_db, weights);
}

int gpsmi_nul_apply(gpsmi_nul* h, const void* iq, float* out, int nb, int32_t* flags, float* gain_db,
                    double* weights) {
    int rc = stage_check_call(h, iq, out, nb, __func__, "null steering", false);
    if (rc) return rc;
    GPSMI_HIP(hipSetDevice(h->cfg.device));
    return h->blk.apply_host(
        iq, out, nb, h->sync.stream, "null steering staging",
        [&](const void* d_iq, void* d_out) { return nul_run(h, d_iq, d_out, nb); },
        [&] { return nul_finish(h, nb, flags, gain_db, weights); });
}

int gpsmi_nul_last_ms(gpsmi_nul* h, float* ms) { return stage_last_ms(h, ms, __func__); }

int gpsmi_nul_last_kernel_ms(gpsmi_nul* h, float* ms) {
    GPSMI_REQUIRE(h && ms, "null argument");
    for (int k = 0; k < 3; ++k) ms[k] = h->kernel_ms[k];
    return GPSMI_OK;
}

}  // extern "C"
