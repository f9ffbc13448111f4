// Null steering (power inversion) over A coherent antennas, ahead of everything else (gpsmi_nul_*,
// include/gpsmi.h; float64 restatement: tests/nul_ref.py).
//
// Per block of n samples, alone: the A x A covariance of the antennas in float64 (the products of
// float32 samples are exact there), R = C / n + delta I, R u = e0 by Cholesky, w = u / u[0], and the
// output y = sum_a conj(w32[a]) x_a in float32; a block whose predicted gain is below min_gain_db (or
// whose R has no Cholesky factor) passes antenna 0 through.  With cfg.taps = 3, 5 or 7 every antenna has a
// filter of that many taps instead: the kernels of gpsmi_nul_stap.h, dispatched from nul_run below.
// gpsmi_nul_beams forms per-satellite beams from the same covariance: the kernels of gpsmi_nul_beam.h,
// dispatched from beam_run below.  What the three forms share stands here, once: NulSamples (a row's
// samples in either input format), nul_slice_sum, nul_factor (R = L L^H) and nul_back on the device;
// NulResults, nul_launch and nul_finish (a call's results and its one body) on the host.
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
#include <type_traits>

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

// 16 and 8 bytes of raw samples, 4-byte aligned
typedef uint32_t nul_u32x4 __attribute__((ext_vector_type(4), aligned(4)));
typedef uint32_t nul_u32x2 __attribute__((ext_vector_type(2), aligned(4)));

// sample q of a call's raw samples from the word w that holds it: the even sample in the low half
__device__ __forceinline__ float2 nul_raw(uint32_t w, int q) { return decode_u8iq(q % 2 ? w >> 16 : w & 0xFFFFu); }

// V samples of the call's input in format FMT as a thread holds them: loaded as b128 words (two complex64
// or eight raw samples each; four raw samples: one b64 word), a raw sample decoded where it is used.
template <int FMT, int V>
struct NulSamples {
    static_assert(V % 2 == 0 && (FMT == 0 || V == 4 || V == 8));
    using Raw = std::conditional_t<V == 8, nul_u32x4, nul_u32x2>;
    std::conditional_t<FMT == 0, float4[V / 2], Raw> v;

    // samples at .. at + V - 1 (at: a multiple of V) of the row that starts `row` samples into the input
    __device__ __forceinline__ void load(const void* __restrict__ iq, size_t at, size_t row = 0) {
        if constexpr (FMT == 0) {
#pragma unroll
            for (int q = 0; q < V; q += 2)
                v[q / 2] = *reinterpret_cast<const float4*>(static_cast<const float2*>(iq) + at + row + q);
        } else {
            v = *reinterpret_cast<const Raw*>(static_cast<const uint16_t*>(iq) + at + row);
        }
    }
    __device__ __forceinline__ float2 operator[](int q) const {
        if constexpr (FMT == 0) return q % 2 ? make_float2(v[q / 2].z, v[q / 2].w) : make_float2(v[q / 2].x, v[q / 2].y);
        else return nul_raw(v[q / 2], q);
    }
};

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
    // (the loads written out, not NulSamples: at A = 8 this kernel fills the register file, and the
    // complex64 form measured 6 % slower with the address arithmetic of the shared loader)
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
                for (int a = 0; a < A; ++a) x[a] = nul_raw(v[a][q / 2], q);
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

// value v (of nv) of block b: its ns slice sums, added in ascending slice order
__device__ __forceinline__ double nul_slice_sum(const double* __restrict__ part, int b, int ns, int nv, int v) {
    const double* src = part + (size_t)b * ns * nv + v;
    double c = src[0];
    for (int s = 1; s < ns; ++s) c += src[(size_t)s * nv];
    return c;
}

// R = C / n + delta I = L L^H, column by column, from the values Cs of a block of n samples; delta = load
// times the mean of R's diagonal.  -> every pivot was positive and finite.  tr, r00: the trace and
// R[0][0] ahead of the loading.  L: the lower triangle; only constants index it (registers).
template <int A>
__device__ __forceinline__ bool nul_factor(const double* Cs, int n, double load, NulZ (&L)[A][A], double& tr,
                                           double& r00) {
    const double dn = (double)n;
    NulZ R[A][A];                                      // lower triangle
    tr = 0.0;
#pragma unroll
    for (int a = 0; a < A; ++a) {
#pragma unroll
        for (int c = 0; c <= a; ++c) {
            const int p = a * (a + 1) / 2 + c;
            R[a][c] = {Cs[2 * p] / dn, a == c ? 0.0 : Cs[2 * p + 1] / dn};
        }
        tr += R[a][a].re;
    }
    r00 = R[0][0].re;
    const double delta = load * tr / (double)A;
#pragma unroll
    for (int a = 0; a < A; ++a) R[a][a].re += delta;
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
    return ok;
}

// L^H x = y for a lower triangle L (registers or LDS): rows descending, each sum in ascending column order
template <int A, typename Tri>
__device__ __forceinline__ void nul_back(const Tri& L, const NulZ (&y)[A], NulZ (&x)[A]) {
#pragma unroll
    for (int i = A - 1; i >= 0; --i) {
        NulZ v = y[i];
#pragma unroll
        for (int k = i + 1; k < A; ++k) v = nul_sub(v, nul_mul(nul_conj(L[k][i]), x[k]));
        x[i] = {v.re / L[i][i].re, v.im / L[i][i].re};
    }
}

// w32: [nb][8] (A used), w64: [nb][A][2]
template <int A>
__global__ __launch_bounds__(128) void nul_solve_kernel(const double* __restrict__ part, int n, int ns,
                                                        double load, double min_db,
                                                        float2* __restrict__ w32, double* __restrict__ w64,
                                                        int32_t* __restrict__ flags, float* __restrict__ gain) {
    constexpr int NV = nul_values(A);
    __shared__ double Cs[NV];
    const int t = threadIdx.x, b = blockIdx.x;
    if (t < NV) Cs[t] = nul_slice_sum(part, b, ns, NV, t);
    __syncthreads();
    if (t != 0) return;
    NulZ L[A][A];
    double tr, p00;
    bool ok = nul_factor<A>(Cs, n, load, L, tr, p00);
    NulZ y[A], u[A];                                   // L y = e0, L^H u = y
    y[0] = {1.0 / L[0][0].re, 0.0};
#pragma unroll
    for (int i = 1; i < A; ++i) {
        NulZ v = {0.0, 0.0};
#pragma unroll
        for (int k = 0; k < i; ++k) v = nul_sub(v, nul_mul(L[i][k], y[k]));
        y[i] = {v.re / L[i][i].re, v.im / L[i][i].re};
    }
    nul_back<A>(L, y, u);
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
    NulSamples<FMT, V> x;
    x.load(iq, at);
    float2 y[V];
#pragma unroll
    for (int q = 0; q < V; ++q) y[q] = x[q];
    if (on) {
#pragma unroll
        for (int q = 0; q < V; ++q) y[q] = nul_term(w[0], y[q]);
#pragma unroll
        for (int a = 1; a < A; ++a) {
            x.load(iq, at, a * astride);
#pragma unroll
            for (int q = 0; q < V; ++q) y[q] = nul_add(y[q], nul_term(w[a], x[q]));
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

// What a call leaves besides the samples, a row per block (gpsmi_nul_apply) or per beam of a block
// (gpsmi_nul_beams): what the solve kernel writes, and the device time of the three kernels.
struct NulResults {
    DevBuf<float2> w32;                                   // [rows][8] (taps: [rows][56]): what the apply reads
    DevBuf<double> w64;                                   // [rows][A][2] (taps: [rows][A][T][2])
    DevBuf<int32_t> flags; DevBuf<float> gain;            // [rows]
    size_t rows = 0, w64_row = 0;                         // of the last call: rows, doubles of a row of w64
    float ms[3] = {0.f, 0.f, 0.f};                        // covariance, solve, apply of the last finished call

    int reserve(size_t rows_, size_t w32_row, size_t w64_row_, const char* what) {
        rows = rows_;
        w64_row = w64_row_;
        int rc = w32.reserve(rows * w32_row, what);
        if (!rc) rc = w64.reserve(rows * w64_row, what);
        if (!rc) rc = flags.reserve(rows, what);
        if (!rc) rc = gain.reserve(rows, what);
        return rc;
    }
};

struct gpsmi_nul {
    gpsmi_nul_cfg cfg;
    DevBuf<double> d_part;                                // [blocks][slices][A (A + 1)] (taps: stap_values)
    double load = 0.0, min_db = 0.0;                      // the cfg's, defaults filled in
    int taps = 1;                                         // 1: one weight per antenna, else 3, 5 or 7
    DevEvent ev_cov, ev_solve;                            // stamps behind the first and the second kernel
    NulResults res, beam;                                 // gpsmi_nul_apply's; gpsmi_nul_beams', which leaves res alone
    DevBuf<double> d_bvec;                                // [nbeam + nnull][A][2]: steer, then nulls
    DevBuf<uint32_t> d_bmask;                             // [nbeam]
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

// One call's three kernels on the handle's stream with the stamps between them; cov, solve and apply
// launch one kernel each.
template <typename Cov, typename Solve, typename Apply>
static int nul_launch(gpsmi_nul* h, Cov&& cov, Solve&& solve, Apply&& apply) {
    const hipStream_t st = h->sync.stream;
    const int rc = h->sync.begin();
    if (rc) return rc;
    cov();
    (void)hipEventRecord(h->ev_cov, st);
    solve();
    (void)hipEventRecord(h->ev_solve, st);
    apply();
    return h->sync.end();
}

// The three passes over nb blocks of every antenna at d_iq (device, the handle's input format) into d_out.
static int nul_run(gpsmi_nul* h, const void* d_iq, void* d_out, int nb) {
    const int n = h->cfg.block_samples, A = h->cfg.antennas, T = h->taps;
    const int ns = (n + kNulSlice - 1) / kNulSlice;
    const size_t astride = (size_t)nb * n;
    NulResults& r = h->res;
    int rc = h->d_part.reserve((size_t)nb * ns * stap_values(A, T), "null steering slice sums");   // (T = 1: nul_values)
    if (!rc) rc = r.reserve(nb, T == 1 ? kNulMaxA : kStapMaxK, (size_t)A * T * 2, "null steering results");
    if (rc) return rc;
    const hipStream_t st = h->sync.stream;
    float2* out = static_cast<float2*>(d_out);
    with_fmt(h->blk.fmt, [&](auto fmt) {
        constexpr int FMT = decltype(fmt)::value;
        constexpr int V = FMT == 0 ? kNulApplyC64 : kNulApplyU8;
        const int nc = (n + kNulThreads * V - 1) / (kNulThreads * V);
        const dim3 slices((unsigned)(nb * ns)), chunks((unsigned)(nb * nc)), blocks((unsigned)nb), wg(kNulThreads);
        if (T > 1) {
            with_value<3, 5, 7>(T, [&](auto nt) {
                constexpr int NT = decltype(nt)::value;
                rc = nul_launch(
                    h,
                    [&] {
                        hipLaunchKernelGGL((stap_cov_kernel<FMT, NT>), slices, wg, 0, st, d_iq, n, ns, A, astride,
                                           h->d_part.p);
                    },
                    [&] {
                        hipLaunchKernelGGL(stap_solve_kernel, blocks, dim3(64), 0, st, h->d_part.p, n, ns, A, NT,
                                           h->load, h->min_db, r.w32.p, r.w64.p, r.flags.p, r.gain.p);
                    },
                    [&] {
                        hipLaunchKernelGGL((stap_apply_kernel<FMT, NT>), chunks, wg, 0, st, d_iq, n, nc, A, astride,
                                           r.w32.p, r.flags.p, out);
                    });
            });
            return;
        }
        with_value<2, 3, 4, 5, 6, 7, 8>(A, [&](auto na) {
            constexpr int NA = decltype(na)::value;
            rc = nul_launch(
                h,
                [&] {
                    hipLaunchKernelGGL((nul_cov_kernel<FMT, NA>), slices, wg, 0, st, d_iq, n, ns, astride, h->d_part.p);
                },
                [&] {
                    hipLaunchKernelGGL(nul_solve_kernel<NA>, blocks, dim3(128), 0, st, h->d_part.p, n, ns, h->load,
                                       h->min_db, r.w32.p, r.w64.p, r.flags.p, r.gain.p);
                },
                [&] {
                    hipLaunchKernelGGL((nul_apply_kernel<FMT, NA>), chunks, wg, 0, st, d_iq, n, nc, astride, r.w32.p,
                                       r.flags.p, out);
                });
        });
    });
    return rc;
}

// Behind nul_launch: the results of r the caller asked for on their way down, the end of the call
// (StageSync::finish), the device time of its three kernels.
static int nul_finish(gpsmi_nul* h, NulResults& r, int32_t* flags, float* gain_db, double* weights) {
    const hipStream_t st = h->sync.stream;
    if (flags) GPSMI_HIP(hipMemcpyAsync(flags, r.flags.p, r.rows * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (gain_db) GPSMI_HIP(hipMemcpyAsync(gain_db, r.gain.p, r.rows * sizeof(float), hipMemcpyDeviceToHost, st));
    if (weights)
        GPSMI_HIP(hipMemcpyAsync(weights, r.w64.p, r.rows * r.w64_row * sizeof(double), hipMemcpyDeviceToHost, st));
    const int rc = h->sync.finish();
    if (rc) return rc;
    GPSMI_HIP(hipEventElapsedTime(&r.ms[0], h->sync.ev0, h->ev_cov));
    GPSMI_HIP(hipEventElapsedTime(&r.ms[1], h->ev_cov, h->ev_solve));
    GPSMI_HIP(hipEventElapsedTime(&r.ms[2], h->ev_solve, h->sync.ev1));
    return GPSMI_OK;
}

static int nul_kernel_ms(const gpsmi_nul* h, NulResults gpsmi_nul::*of, float* ms, const char* fn) {
    if (!h || !ms) return fail(GPSMI_E_ARG, "%s: null argument", fn);
    for (int k = 0; k < 3; ++k) ms[k] = (h->*of).ms[k];
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

// What a beams call checks on a live handle behind stage_check_blocks, before any GPU work: the handle's
// taps, the beams, and the rows' strides (in samples, 0 filled in), alignment and overlap.
static int beam_check_call(const gpsmi_nul* h, const char* fn, const void* iq, size_t in_stride, const void* out,
                           size_t out_stride, int nb, const BeamPlan& p, bool dev) {
    int rc = stage_check_blocks(h, iq, out, nb, fn);
    if (rc) return rc;
    if (h->taps != 1) return fail(GPSMI_E_STATE, "%s: the handle is a space-time one (taps %d)", fn, h->taps);
    const int n = h->cfg.block_samples, A = h->cfg.antennas;
    if ((rc = beam_check_plan(fn, A, p))) return rc;
    const size_t row = (size_t)nb * n, ss = h->blk.fmt == GPSMI_IQ_U8 ? sizeof(uint16_t) : sizeof(float2);
    if (in_stride < row || out_stride < row || in_stride > ((size_t)1 << 40) || out_stride > ((size_t)1 << 40))
        return fail(GPSMI_E_ARG, "%s: a row stride is shorter than the nb * n samples of a row", fn);
    if (dev && (!stage_aligned(h->blk, iq, out) || in_stride % 2 != 0 || out_stride % 2 != 0))
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
    NulResults& r = h->beam;
    int rc = h->d_part.reserve((size_t)nb * ns * nul_values(A), "null steering slice sums");
    if (!rc) rc = h->d_bvec.reserve((size_t)(kBeamMax + kBeamMaxNull) * kNulMaxA * 2, what);
    if (!rc) rc = h->d_bmask.reserve(kBeamMax, what);
    if (!rc) rc = r.reserve((size_t)nb * B, kNulMaxA, (size_t)A * 2, what);
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
    const int nc = (n + kNulThreads * kBeamApply - 1) / (kNulThreads * kBeamApply);
    const dim3 slices((unsigned)(nb * ns)), chunks((unsigned)(nb * nc)), blocks((unsigned)nb), wg(kNulThreads);
    with_fmt(h->blk.fmt, [&](auto fmt) {
        constexpr int FMT = decltype(fmt)::value;
        with_value<2, 3, 4, 5, 6, 7, 8>(A, [&](auto na) {
            constexpr int NA = decltype(na)::value;
            rc = nul_launch(
                h,
                [&] {
                    hipLaunchKernelGGL((nul_cov_kernel<FMT, NA>), slices, wg, 0, st, d_iq, n, ns, in_stride, h->d_part.p);
                },
                [&] {
                    hipLaunchKernelGGL(beam_solve_kernel<NA>, blocks, dim3(kBeamSolveThreads), 0, st, h->d_part.p, n, ns,
                                       h->load, B, Q, h->d_bvec.p, d_nulls, h->d_bmask.p, r.w32.p, r.w64.p, r.flags.p,
                                       r.gain.p);
                },
                [&] {
                    hipLaunchKernelGGL((beam_apply_kernel<FMT, NA>), chunks, wg, 0, st, d_iq, n, nc, in_stride, B,
                                       r.w32.p, r.flags.p, static_cast<float2*>(d_out), out_stride);
                });
        });
    });
    return rc;
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
    return nul_finish(h, h->res, flags, gain_db, weights);
}

int gpsmi_nul_apply(gpsmi_nul* h, const void* iq, float* out, int nb, int32_t* flags, float* gain_db,
                    double* weights) {
    int rc = stage_check_call(h, iq, out, nb, __func__, "null steering", false);
    if (rc) return rc;
    GPSMI_HIP(hipSetDevice(h->cfg.device));
    return h->blk.apply_host(
        iq, out, nb, h->blk.out_bytes(nb), h->sync.stream, "null steering staging",
        [&](const void* d_iq, void* d_out) { return nul_run(h, d_iq, d_out, nb); },
        [&] { return nul_finish(h, h->res, flags, gain_db, weights); });
}

int gpsmi_nul_last_ms(gpsmi_nul* h, float* ms) { return stage_last_ms(h, ms, __func__); }

int gpsmi_nul_last_kernel_ms(gpsmi_nul* h, float* ms) { return nul_kernel_ms(h, &gpsmi_nul::res, ms, __func__); }

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
    return nul_finish(h, h->beam, flags, gain_db, weights);
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
    return h->blk.apply_host(
        iq, out, nb, (size_t)nbeam * h->blk.out_bytes(nb), h->sync.stream, "beam staging",
        [&](const void* d_iq, void* d_out) { return beam_run(h, d_iq, row, d_out, row, nb, p); },
        [&] { return nul_finish(h, h->beam, flags, gain_db, weights); });
}

int gpsmi_nul_last_beam_kernel_ms(gpsmi_nul* h, float* ms) {
    return nul_kernel_ms(h, &gpsmi_nul::beam, ms, __func__);
}

}  // extern "C"
