// Null steering (power inversion) over A coherent antennas, ahead of everything else (gpsmi_nul_*,
// include/gpsmi.h; float64 restatement: tests/nul_ref.py).
//
// Per block of n samples, alone: the A x A covariance of the antennas in float64 (the products of
// float32 samples are exact there), R = C / n + delta I, R u = e0 by Cholesky, w = u / u[0], and the
// output y = sum_a conj(w32[a]) x_a in float32; a block whose predicted gain is below min_gain_db (or
// whose R has no Cholesky factor) passes antenna 0 through.  With cfg.taps = 3, 5 or 7 every antenna has a
// filter of that many taps instead: the kernels of gpsmi_nul_stap.h, dispatched from nul_run below.
// gpsmi_nul_beams forms per-satellite beams from the same covariance: the kernels of gpsmi_nul_beam.h,
// dispatched from beam_run below; it shares nul_cov_kernel and leaves everything else here alone.
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
#include "gpsmi_nul_beam.h"

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
    // gpsmi_nul_beams: its own results, so that a call leaves gpsmi_nul_apply's alone
    DevBuf<double> d_bvec;                                // [nbeam + nnull][A][2]: steer, then nulls
    DevBuf<uint32_t> d_bmask;                             // [nbeam]
    DevBuf<float2> d_bw32;                                // [blocks][nbeam][8]
    DevBuf<double> d_bw64;                                // [blocks][nbeam][A][2]
    DevBuf<int32_t> d_bflags; DevBuf<float> d_bgain;      // [blocks][nbeam]
    DevBuf<char> d_bout;                                  // host entry: the staged beams
    float beam_ms[3] = {0.f, 0.f, 0.f};                   // covariance, solve, apply of the last finished beams call
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

// ---- beams -------------------------------------------------------------------------------------

struct BeamPlan {
    int nbeam, nnull;
    const double *steer, *nulls;
    const uint32_t* mask;
};

// The checks of a beam description that need neither a handle nor a GPU (gpsmi_nul_beams_plan).
static int beam_check_plan(const char* fn, int A, const BeamPlan& p) {
    if (A < 2 || A > kNulMaxA) return fail(GPSMI_E_ARG, "%s: antennas out of range 2..8", fn);
    if (p.nbeam < 1 || p.nbeam > kBeamMax) return fail(GPSMI_E_ARG, "%s: nbeam out of range 1..64", fn);
    if (p.nnull < 0 || p.nnull > kBeamMaxNull) return fail(GPSMI_E_ARG, "%s: nnull out of range 0..4", fn);
    if (!p.steer || (p.nnull > 0 && (!p.nulls || !p.mask))) return fail(GPSMI_E_ARG, "%s: null argument", fn);
    // every vector finite and not zero; unit[j]: vector j over its length (steer, then nulls)
    auto unit = [&](const double* g, double (*u)[2]) {
        double s2 = 0.0;
        for (int a = 0; a < A; ++a) {
            if (!std::isfinite(g[2 * a]) || !std::isfinite(g[2 * a + 1])) return false;
            s2 += g[2 * a] * g[2 * a] + g[2 * a + 1] * g[2 * a + 1];
        }
        const double len = std::sqrt(s2);
        if (!(len > 0.0) || !std::isfinite(len)) return false;
        for (int a = 0; a < A; ++a) {
            u[a][0] = g[2 * a] / len;
            u[a][1] = g[2 * a + 1] / len;
        }
        return true;
    };
    double un[kBeamMaxNull][kNulMaxA][2];
    for (int q = 0; q < p.nnull; ++q)
        if (!unit(p.nulls + (size_t)q * A * 2, un[q]))
            return fail(GPSMI_E_ARG, "%s: null vector %d is zero or not finite", fn, q);
    for (int b = 0; b < p.nbeam; ++b) {
        double (*col[kBeamMaxM])[2];
        double us[kNulMaxA][2];
        if (!unit(p.steer + (size_t)b * A * 2, us))
            return fail(GPSMI_E_ARG, "%s: steering vector %d is zero or not finite", fn, b);
        const uint32_t mk = p.mask ? p.mask[b] : 0u;
        if (p.nnull < 32 && (mk >> p.nnull) != 0u)
            return fail(GPSMI_E_ARG, "%s: null_mask of beam %d names a null vector the call does not have", fn, b);
        int m = 0;
        col[m++] = us;
        for (int q = 0; q < p.nnull; ++q)
            if ((mk >> q) & 1u) col[m++] = un[q];
        if (m > A) return fail(GPSMI_E_ARG, "%s: beam %d has more constraints than antennas", fn, b);
        // the Gram matrix of the unit columns and its Cholesky: every pivot >= 1 / 64
        double Lr[kBeamMaxM][kBeamMaxM], Li[kBeamMaxM][kBeamMaxM];
        for (int j = 0; j < m; ++j) {
            for (int i = j; i < m; ++i) {
                double re = 0.0, im = 0.0;                // conj(col i) . col j
                for (int a = 0; a < A; ++a) {
                    re += col[i][a][0] * col[j][a][0] + col[i][a][1] * col[j][a][1];
                    im += col[i][a][0] * col[j][a][1] - col[i][a][1] * col[j][a][0];
                }
                for (int k = 0; k < j; ++k) {             // - L[i][k] conj(L[j][k])
                    re -= Lr[i][k] * Lr[j][k] + Li[i][k] * Li[j][k];
                    im -= Li[i][k] * Lr[j][k] - Lr[i][k] * Li[j][k];
                }
                if (i == j) {
                    if (!(re >= 1.0 / 64.0))
                        return fail(GPSMI_E_ARG, "%s: the constraints of beam %d are dependent (pivot %.4g < 1/64)",
                                    fn, b, re);
                    Lr[j][j] = std::sqrt(re);
                    Li[j][j] = 0.0;
                } else {
                    Lr[i][j] = re / Lr[j][j];
                    Li[i][j] = im / Lr[j][j];
                }
            }
        }
    }
    return GPSMI_OK;
}

// The checks of a beams call on a live handle, before any GPU work.  Strides in samples, 0 filled in.
static int beam_check_call(const gpsmi_nul* h, const char* fn, const void* iq, size_t in_stride, const void* out,
                           size_t out_stride, int nb, const BeamPlan& p, bool dev) {
    if (!h || !iq || !out) return fail(GPSMI_E_ARG, "%s: null argument", fn);
    if (h->taps != 1) return fail(GPSMI_E_STATE, "%s: the handle is a space-time one (taps %d)", fn, h->taps);
    const int n = h->cfg.block_samples, A = h->cfg.antennas;
    if (nb < 1 || (size_t)nb * n > ((size_t)1 << 31))
        return fail(GPSMI_E_ARG, "%s: nb out of range: 1 .. 2^31 samples per call", fn);
    const int rc = beam_check_plan(fn, A, p);
    if (rc) return rc;
    const size_t row = (size_t)nb * n, ss = h->blk.fmt == GPSMI_IQ_U8 ? sizeof(uint16_t) : sizeof(float2);
    if (in_stride < row || out_stride < row || in_stride > ((size_t)1 << 40) || out_stride > ((size_t)1 << 40))
        return fail(GPSMI_E_ARG, "%s: a row stride is shorter than the nb * n samples of a row", fn);
    if (dev && ((uintptr_t)iq % (ss == 2 ? 4 : 16) != 0 || (uintptr_t)out % 16 != 0 || in_stride % 2 != 0 ||
                out_stride % 2 != 0))
        return fail(GPSMI_E_ARG,
                    "%s: device input / output rows not aligned (4 bytes for u8, 16 for complex64: even strides)", fn);
    const char* i0 = static_cast<const char*>(iq);
    const char* o0 = static_cast<const char*>(out);
    for (int a = 0; a < A; ++a) {
        const char* ia = i0 + a * in_stride * ss;
        for (int b = 0; b < p.nbeam; ++b) {
            const char* ob = o0 + b * out_stride * sizeof(float2);
            if (!(ob + row * sizeof(float2) <= ia || ia + row * ss <= ob))
                return fail(GPSMI_E_ARG, "%s: input and output overlap (no in-place beams)", fn);
        }
    }
    return GPSMI_OK;
}

// The three passes over nb blocks: nul_cov_kernel as gpsmi_nul_apply runs it, then the beams' own two.
static int beam_run(gpsmi_nul* h, const void* d_iq, size_t in_stride, void* d_out, size_t out_stride, int nb,
                    const BeamPlan& p) {
    const int n = h->cfg.block_samples, A = h->cfg.antennas, B = p.nbeam, Q = p.nnull;
    const int ns = (n + kNulSlice - 1) / kNulSlice;
    const char* what = "beam results";
    int rc = h->d_part.reserve((size_t)nb * ns * nul_values(A), "null steering slice sums");
    if (!rc) rc = h->d_bvec.reserve((size_t)(kBeamMax + kBeamMaxNull) * kNulMaxA * 2, what);
    if (!rc) rc = h->d_bmask.reserve(kBeamMax, what);
    if (!rc) rc = h->d_bw32.reserve((size_t)nb * B * kNulMaxA, what);
    if (!rc) rc = h->d_bw64.reserve((size_t)nb * B * A * 2, what);
    if (!rc) rc = h->d_bflags.reserve((size_t)nb * B, what);
    if (!rc) rc = h->d_bgain.reserve((size_t)nb * B, what);
    if (rc) return rc;
    const hipStream_t st = h->sync.stream;
    uint32_t mask[kBeamMax];
    for (int b = 0; b < B; ++b) mask[b] = p.mask ? p.mask[b] : 0u;
    double* d_nulls = h->d_bvec.p + (size_t)B * A * 2;
    GPSMI_HIP(hipMemcpyAsync(h->d_bvec.p, p.steer, (size_t)B * A * 2 * sizeof(double), hipMemcpyHostToDevice, st));
    if (Q > 0)
        GPSMI_HIP(hipMemcpyAsync(d_nulls, p.nulls, (size_t)Q * A * 2 * sizeof(double), hipMemcpyHostToDevice, st));
    GPSMI_HIP(hipMemcpyAsync(h->d_bmask.p, mask, (size_t)B * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    GPSMI_HIP(hipStreamSynchronize(st));                  // (mask is on this stack)
    if ((rc = h->sync.begin())) return rc;
    const int nc = (n + kNulThreads * kBeamApply - 1) / (kNulThreads * kBeamApply);
    with_fmt(h->blk.fmt, [&](auto fmt) {
        constexpr int FMT = decltype(fmt)::value;
        with_value<2, 3, 4, 5, 6, 7, 8>(A, [&](auto na) {
            constexpr int NA = decltype(na)::value;
            hipLaunchKernelGGL((nul_cov_kernel<FMT, NA>), dim3((unsigned)(nb * ns)), dim3(kNulThreads), 0, st,
                               d_iq, n, ns, in_stride, h->d_part.p);
            (void)hipEventRecord(h->ev_cov, st);
            hipLaunchKernelGGL(beam_solve_kernel<NA>, dim3((unsigned)nb), dim3(kBeamSolveThreads), 0, st,
                               h->d_part.p, n, ns, h->load, B, Q, h->d_bvec.p, d_nulls, h->d_bmask.p, h->d_bw32.p,
                               h->d_bw64.p, h->d_bflags.p, h->d_bgain.p);
            (void)hipEventRecord(h->ev_solve, st);
            hipLaunchKernelGGL((beam_apply_kernel<FMT, NA>), dim3((unsigned)(nb * nc)), dim3(kNulThreads), 0, st,
                               d_iq, n, nc, in_stride, B, h->d_bw32.p, h->d_bflags.p, static_cast<float2*>(d_out),
                               out_stride);
        });
    });
    return h->sync.end();
}

static int beam_finish(gpsmi_nul* h, int nb, int B, int32_t* flags, float* gain_db, double* weights) {
    const hipStream_t st = h->sync.stream;
    const size_t r = (size_t)nb * B;
    if (flags) GPSMI_HIP(hipMemcpyAsync(flags, h->d_bflags.p, r * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (gain_db) GPSMI_HIP(hipMemcpyAsync(gain_db, h->d_bgain.p, r * sizeof(float), hipMemcpyDeviceToHost, st));
    if (weights)
        GPSMI_HIP(hipMemcpyAsync(weights, h->d_bw64.p, r * h->cfg.antennas * 2 * sizeof(double),
                                 hipMemcpyDeviceToHost, st));
    const int rc = h->sync.finish();
    if (rc) return rc;
    GPSMI_HIP(hipEventElapsedTime(&h->beam_ms[0], h->sync.ev0, h->ev_cov));
    GPSMI_HIP(hipEventElapsedTime(&h->beam_ms[1], h->ev_cov, h->ev_solve));
    GPSMI_HIP(hipEventElapsedTime(&h->beam_ms[2], h->ev_solve, h->sync.ev1));
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

int gpsmi_nul_beams_plan(int antennas, int nbeam, const double* steer, int nnull, const double* nulls,
                         const uint32_t* null_mask) {
    return beam_check_plan(__func__, antennas, BeamPlan{nbeam, nnull, steer, nulls, null_mask});
}

int gpsmi_nul_beams_dev(gpsmi_nul* h, const void* d_iq, int64_t in_stride, void* d_out, int64_t out_stride, int nb,
                        int nbeam, const double* steer, int nnull, const double* nulls, const uint32_t* null_mask,
                        int32_t* flags, float* gain_db, double* weights) {
    GPSMI_REQUIRE(h, "null argument");
    GPSMI_REQUIRE(in_stride >= 0 && out_stride >= 0, "negative row stride");
    const BeamPlan p{nbeam, nnull, steer, nulls, null_mask};
    const size_t row = (size_t)(nb > 0 ? nb : 0) * h->cfg.block_samples;
    const size_t is = in_stride ? (size_t)in_stride : row, os = out_stride ? (size_t)out_stride : row;
    int rc = beam_check_call(h, __func__, d_iq, is, d_out, os, nb, p, true);
    if (rc) return rc;
    GPSMI_HIP(hipSetDevice(h->cfg.device));
    rc = beam_run(h, d_iq, is, d_out, os, nb, p);
    if (rc) return rc;
    return beam_finish(h, nb, nbeam, flags, gain_db, weights);
}

int gpsmi_nul_beams(gpsmi_nul* h, const void* iq, float* out, int nb, int nbeam, const double* steer, int nnull,
                    const double* nulls, const uint32_t* null_mask, int32_t* flags, float* gain_db,
                    double* weights) {
    GPSMI_REQUIRE(h, "null argument");
    const BeamPlan p{nbeam, nnull, steer, nulls, null_mask};
    const size_t row = (size_t)(nb > 0 ? nb : 0) * h->cfg.block_samples;
    int rc = beam_check_call(h, __func__, iq, row, out, row, nb, p, false);
    if (rc) return rc;
    GPSMI_HIP(hipSetDevice(h->cfg.device));
    const hipStream_t st = h->sync.stream;
    const size_t ib = h->blk.in_bytes(nb), ob = (size_t)nbeam * row * sizeof(float2);
    rc = h->blk.io.in.reserve(ib, "beam staging");
    if (!rc) rc = h->d_bout.reserve(ob, "beam staging");
    if (rc) return rc;
    GPSMI_HIP(hipMemcpyAsync(h->blk.io.in.p, iq, ib, hipMemcpyHostToDevice, st));
    rc = beam_run(h, h->blk.io.in.p, row, h->d_bout.p, row, nb, p);
    if (rc) return rc;
    GPSMI_HIP(hipMemcpyAsync(out, h->d_bout.p, ob, hipMemcpyDeviceToHost, st));
    return beam_finish(h, nb, nbeam, flags, gain_db, weights);
}

int gpsmi_nul_last_beam_kernel_ms(gpsmi_nul* h, float* ms) {
    GPSMI_REQUIRE(h && ms, "null argument");
    for (int k = 0; k < 3; ++k) ms[k] = h->beam_ms[k];
    return GPSMI_OK;
}

}  // extern "C"
