// Per-satellite beams on the null-steering handle (gpsmi_nul_beams*, include/gpsmi.h; DESIGN.md 4.2q;
// restatement: tests/beam_ref.py).  Included by gpsmi_nul.hip behind the kernels of gpsmi_nul_apply: the
// covariance of a block is nul_cov_kernel's, and the slice sums, the factor of R, the back substitution
// and the loading of a row's samples are the helpers that stand there.
//
// Per block, alone: R = C / n + delta I = L L^H (nul_factor), and per beam b the linearly
// constrained minimum-variance weights w = R^-1 G (G^H R^-1 G)^-1 e0 with G = [s_b, u_q ...]: the
// steering vector of the beam held at one, the null vectors its mask names at zero.
//
//   beam_solve_kernel<A>       one workgroup per block.  Thread v adds value v of the slice sums in
//                              ascending slice order; thread 0 loads and factors R -> L in LDS (the
//                              identity when a pivot fails); thread j < nbeam + nnull solves
//                              L z_j = g_j, one column of constraints each (a null vector's column
//                              serves every beam that carries it) -> LDS; thread b < nbeam forms
//                              M = Z^H Z of its m <= 5 columns, factors it, solves M q = e0, forms
//                              t = Z q and w = L^-H t -> w32, weights, flag, gain.  float64, nothing
//                              fused; all arrays of a thread are indexed by constants (registers).
//   beam_apply_kernel<FMT, A>  the hot path.  Four samples per thread: the A rows are loaded once
//                              (two b128 loads per antenna for complex64, one b64 for raw) and held in
//                              registers, 8 A floats; then a loop over the beams: the beam's A weights
//                              and its flag by uniform loads (SGPRs), nul_apply_kernel's arithmetic,
//                              two float4 stores into the beam's row.  No atomics, no LDS, no scratch;
//                              one thread writes each output word.
#pragma once

namespace gpsmi {

constexpr int kBeamMax = 64;                         // beams per call
constexpr int kBeamMaxNull = 4;                      // null vectors per call
constexpr int kBeamMaxM = 1 + kBeamMaxNull;          // constraints of a beam
constexpr int kBeamSolveThreads = 128;               // >= nul_values(8) = 72 and >= kBeamMax + kBeamMaxNull
constexpr int kBeamApply = 4;                        // samples per thread of the apply

#pragma clang fp contract(off)
__device__ __forceinline__ NulZ beam_add(NulZ a, NulZ b) { return {a.re + b.re, a.im + b.im}; }
__device__ __forceinline__ double beam_abs2(NulZ a) { return a.re * a.re + a.im * a.im; }

// steer: [nbeam][A][2], nulls: [nnull][A][2], mask: [nbeam]; w32: [nb][nbeam][8] (A used),
// w64: [nb][nbeam][A][2], flags, gain: [nb][nbeam]
template <int A>
__global__ __launch_bounds__(kBeamSolveThreads) void beam_solve_kernel(
    const double* __restrict__ part, int n, int ns, double load, int nbeam, int nnull,
    const double* __restrict__ steer, const double* __restrict__ nulls, const uint32_t* __restrict__ mask,
    float2* __restrict__ w32, double* __restrict__ w64, int32_t* __restrict__ flags, float* __restrict__ gain) {
    constexpr int NV = nul_values(A);
    static_assert(NV <= kBeamSolveThreads && kBeamMax + kBeamMaxNull <= kBeamSolveThreads);
    __shared__ double Cs[NV];
    __shared__ NulZ Ls[A][A];                          // lower triangle
    __shared__ NulZ Zs[kBeamMax + kBeamMaxNull][A];    // column j: L^-1 g_j
    __shared__ double s_tr;
    __shared__ int s_ok;
    const int t = threadIdx.x, b = blockIdx.x;
    if (t < NV) Cs[t] = nul_slice_sum(part, b, ns, NV, t);
    __syncthreads();
    if (t == 0) {
        NulZ L[A][A];
        double tr, r00;
        const bool ok = nul_factor<A>(Cs, n, load, L, tr, r00);
#pragma unroll
        for (int i = 0; i < A; ++i) {
#pragma unroll
            for (int j = 0; j <= i; ++j) Ls[i][j] = ok ? L[i][j] : NulZ{i == j ? 1.0 : 0.0, 0.0};
        }
        s_tr = tr;
        s_ok = ok ? 1 : 0;
    }
    __syncthreads();
    if (t < nbeam + nnull) {                           // L z = g, forward
        const double* g = t < nbeam ? steer + (size_t)t * A * 2 : nulls + (size_t)(t - nbeam) * A * 2;
        NulZ z[A];
#pragma unroll
        for (int i = 0; i < A; ++i) {
            NulZ v = {g[2 * i], g[2 * i + 1]};
#pragma unroll
            for (int k = 0; k < i; ++k) v = nul_sub(v, nul_mul(Ls[i][k], z[k]));
            z[i] = {v.re / Ls[i][i].re, v.im / Ls[i][i].re};
            Zs[t][i] = z[i];
        }
    }
    __syncthreads();
    if (t >= nbeam) return;
    // the beam's columns: its own, then those of its nulls in ascending q (one byte each, no array)
    const uint32_t mk = mask[t];
    uint32_t pack = 0;
    int m = 1;
#pragma unroll
    for (int q = 0; q < kBeamMaxNull; ++q) {
        if (q < nnull && ((mk >> q) & 1u)) {
            pack |= (uint32_t)(nbeam + q) << (8 * (m - 1));
            ++m;
        }
    }
    auto col = [&](int j) { return j == 0 ? t : (int)((pack >> (8 * (j - 1))) & 0xFFu); };
    // M = Z^H Z (lower triangle), then M = K K^H in place
    NulZ K[kBeamMaxM][kBeamMaxM];
#pragma unroll
    for (int i = 0; i < kBeamMaxM; ++i) {
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            K[i][j] = {0.0, 0.0};
            if (i < m) {
                const NulZ* zi = Zs[col(i)];
                const NulZ* zj = Zs[col(j)];
                NulZ acc = {0.0, 0.0};
#pragma unroll
                for (int a = 0; a < A; ++a) {
                    if (i == j) acc.re += beam_abs2(zi[a]);
                    else acc = beam_add(acc, nul_mul(nul_conj(zi[a]), zj[a]));
                }
                K[i][j] = acc;
            }
        }
    }
    bool ok = true;
#pragma unroll
    for (int j = 0; j < kBeamMaxM; ++j) {
        if (j < m) {
            double d = K[j][j].re;
#pragma unroll
            for (int k = 0; k < j; ++k) d -= K[j][k].re * K[j][k].re + K[j][k].im * K[j][k].im;
            if (!(d > 0.0) || !(d < INFINITY)) ok = false;
            const double l = sqrt(d);
            K[j][j] = {l, 0.0};
#pragma unroll
            for (int i = j + 1; i < kBeamMaxM; ++i) {
                if (i < m) {
                    NulZ v = K[i][j];
#pragma unroll
                    for (int k = 0; k < j; ++k) v = nul_sub(v, nul_mul(K[i][k], nul_conj(K[j][k])));
                    K[i][j] = {v.re / l, v.im / l};
                }
            }
        }
    }
    // K y = e0 forward, K^H q = y backward
    NulZ y[kBeamMaxM], q[kBeamMaxM];
    y[0] = {1.0 / K[0][0].re, 0.0};
#pragma unroll
    for (int i = 1; i < kBeamMaxM; ++i) {
        y[i] = {0.0, 0.0};
        if (i < m) {
            NulZ v = {0.0, 0.0};
#pragma unroll
            for (int k = 0; k < i; ++k) v = nul_sub(v, nul_mul(K[i][k], y[k]));
            y[i] = {v.re / K[i][i].re, v.im / K[i][i].re};
        }
    }
#pragma unroll
    for (int i = kBeamMaxM - 1; i >= 0; --i) {
        q[i] = {0.0, 0.0};
        if (i < m) {
            NulZ v = y[i];
#pragma unroll
            for (int k = i + 1; k < kBeamMaxM; ++k)
                if (k < m) v = nul_sub(v, nul_mul(nul_conj(K[k][i]), q[k]));
            q[i] = {v.re / K[i][i].re, v.im / K[i][i].re};
        }
    }
    // t = Z q, then L^H w = t backward
    NulZ tq[A], w[A];
#pragma unroll
    for (int a = 0; a < A; ++a) {
        NulZ acc = {0.0, 0.0};
#pragma unroll
        for (int j = 0; j < kBeamMaxM; ++j)
            if (j < m) acc = beam_add(acc, nul_mul(Zs[col(j)][a], q[j]));
        tq[a] = acc;
    }
    nul_back<A>(Ls, tq, w);
    double s2 = 0.0;
#pragma unroll
    for (int a = 0; a < A; ++a) {
        const NulZ g = {steer[((size_t)t * A + a) * 2], steer[((size_t)t * A + a) * 2 + 1]};
        s2 += beam_abs2(g);
    }
    const size_t r = (size_t)b * nbeam + t;
    flags[r] = ok ? s_ok : -1;
    gain[r] = ok ? (float)(10.0 * log10(s_tr / (s2 * q[0].re))) : 0.f;
#pragma unroll
    for (int a = 0; a < A; ++a) {
        const NulZ v = ok ? w[a] : NulZ{0.0, 0.0};
        w64[(r * A + a) * 2] = v.re;
        w64[(r * A + a) * 2 + 1] = v.im;
        w32[r * kNulMaxA + a] = make_float2((float)v.re, (float)v.im);
    }
}
#pragma clang fp contract(fast)

// iq: row a of the call at a * istride samples, block b of it n b further; out: row of beam k at
// k * ostride samples.  Both strides keep the rows' alignment (even).
template <int FMT, int A>
__global__ __launch_bounds__(kNulThreads) void beam_apply_kernel(const void* __restrict__ iq, int n, int nc,
                                                                 size_t istride, int nbeam,
                                                                 const float2* __restrict__ w32,
                                                                 const int32_t* __restrict__ flags,
                                                                 float2* __restrict__ out, size_t ostride) {
    constexpr int V = kBeamApply;
    const int b = blockIdx.x / nc, c = blockIdx.x % nc;
    const int i = (c * kNulThreads + (int)threadIdx.x) * V;
    if (i >= n) return;                                // (n is a multiple of 32: whole groups)
    const size_t at = (size_t)b * n + i;
    float2 x[A][V];
#pragma unroll
    for (int a = 0; a < A; ++a) {
        NulSamples<FMT, V> v;
        v.load(iq, at, a * istride);
#pragma unroll
        for (int q = 0; q < V; ++q) x[a][q] = v[q];
    }
    const float2* wb = w32 + (size_t)b * nbeam * kNulMaxA;
    const int32_t* fb = flags + (size_t)b * nbeam;
    float2* dst = out + at;
    for (int k = 0; k < nbeam; ++k, wb += kNulMaxA, dst += ostride) {
        float2 y[V];
        if (fb[k] < 0) {                               // no weights: +0.0
#pragma unroll
            for (int q = 0; q < V; ++q) y[q] = make_float2(0.f, 0.f);
        } else {
            float2 w[A];
#pragma unroll
            for (int a = 0; a < A; ++a) w[a] = wb[a];
#pragma unroll
            for (int q = 0; q < V; ++q) y[q] = nul_term(w[0], x[0][q]);
#pragma unroll
            for (int a = 1; a < A; ++a) {
#pragma unroll
                for (int q = 0; q < V; ++q) y[q] = nul_add(y[q], nul_term(w[a], x[a][q]));
            }
        }
#pragma unroll
        for (int q = 0; q < V; q += 2)
            *reinterpret_cast<float4*>(dst + q) = make_float4(y[q].x, y[q].y, y[q + 1].x, y[q + 1].y);
    }
}

}  // namespace gpsmi
