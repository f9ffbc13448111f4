// Space-time null steering: T = 3, 5 or 7 taps per antenna (gpsmi_nul_cfg.taps, include/gpsmi.h;
// DESIGN.md 4.2o; restatement: tests/stap_ref.py).  Included by gpsmi_nul.hip behind the kernels of
// the one-weight form, whose nul_slice_sum, NulSamples, nul_raw, nul_term and nul_add it uses.
//
//   stap_cov_kernel<FMT, T>    one workgroup per (block, slice of 8192 samples), four waves.  The slice
//                              is staged 256 samples at a time (and the 8 before them: the halo of
//                              the lags, from inside the block, zeros before sample 0) as float64 in
//                              LDS, sample-major: 16 rows per sample, Re x_0..7 then Im x_0..7, rows
//                              of antennas the handle does not have stay zero.  Wave w walks samples
//                              64 w .. 64 w + 63 of the staged chunk four at a time: one 8-byte LDS read
//                              per lane for the A operand (row lane & 15 at sample i + (lane >> 4)), one
//                              per lag l for the B operand (the same row at i - l + (lane >> 4)), one
//                              v_mfma_f64_16x16x4_f64 per lag into T accumulators of 4 doubles per
//                              lane: D_l[p][q] = sum_i row_p[i] row_q[i - l].  After the last sample
//                              the four waves' tiles are added in wave order through LDS and
//                              re = RR + II, im = IR - RI go to part[block][slice][values].  No atomics.
//   stap_solve_kernel          one wave per block: the slice sums in ascending slice order, the lower
//                              triangle of R (K = A T <= 56) in LDS, column Cholesky with lanes over
//                              rows, forward substitution with lanes over rows (each row subtracts in
//                              ascending column order), backward substitution in the header's order.
//   stap_apply_kernel<FMT, T>  a streaming pass like nul_apply_kernel: two (complex64) or eight (raw)
//                              samples per thread plus the taps' halo from inside the block, the A T
//                              weights by uniform loads, the 2 c edge samples zeroed, one float4
//                              store per sample pair; a pass-through block copies antenna 0.
//
// Sample-major staging with a stride of 17 doubles keeps both sides of LDS clean: a wave's operand read
// touches 64 distinct doubles of four neighbouring samples, and the threads that stage neighbouring
// samples write 34 banks apart.  The order of every sum depends on n alone.
#pragma once

namespace gpsmi {

constexpr int kStapChunk = 256;                      // samples staged per pass (64 per wave)
constexpr int kStapHalo = 8;                         // staged ahead of them: >= taps - 1, keeps the alignment
constexpr int kStapRow = 17;                         // doubles per staged sample (16 rows and one of padding)
constexpr int kStapMaxT = 7;
constexpr int kStapMaxK = kNulMaxA * kStapMaxT;      // 56

// values of a slice: lag 0 as nul_values (pairs a >= b), then per lag l >= 1 every (a, b):
// re at A (A + 1) + (l - 1) 2 A^2 + 2 (a A + b), im behind it
__host__ __device__ constexpr int stap_values(int A, int T) { return A * (A + 1) + (T - 1) * 2 * A * A; }

typedef double stap_d4 __attribute__((ext_vector_type(4)));

template <int FMT, int T>
__global__ __launch_bounds__(kNulThreads) void stap_cov_kernel(const void* __restrict__ iq, int n, int ns, int A,
                                                               size_t astride, double* __restrict__ part) {
    static_assert(T - 1 <= kStapHalo && kStapChunk == kNulThreads && kNulSlice % kStapChunk == 0);
    constexpr int V = FMT == 0 ? 1 : 2;              // samples a thread stages per load
    constexpr int ROWS = kStapHalo + kStapChunk;
    constexpr int STAGE = ROWS * kStapRow, TILES = T * 256;
    __shared__ double S[STAGE > TILES ? STAGE : TILES];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int r = lane & 15, k = lane >> 4;
    const int b = blockIdx.x / ns, s = blockIdx.x % ns;
    const int i0 = s * kNulSlice, len = min(kNulSlice, n - i0);    // (a multiple of 32)
    const size_t base = (size_t)b * n;
    for (int j = t; j < STAGE; j += kNulThreads) S[j] = 0.0;
    stap_d4 acc[T];
#pragma unroll
    for (int l = 0; l < T; ++l) acc[l] = stap_d4{0.0, 0.0, 0.0, 0.0};

    for (int c0 = 0; c0 < len; c0 += kStapChunk) {
        __syncthreads();                             // (the chunk before has been read; the zero fill)
        // staged row jj holds sample c0 + jj - 8 of the slice: zero before the block and behind the slice
        auto stage = [&](int jj) {
            const int rel = c0 + jj - kStapHalo;
            const bool in = i0 + rel >= 0 && rel < len;
            const size_t at = base + (size_t)(in ? i0 + rel : 0);
#pragma unroll
            for (int a = 0; a < kNulMaxA; ++a) {
                if (a >= A) break;
                float2 x[V];
                if constexpr (FMT == 0) {
                    x[0] = in ? static_cast<const float2*>(iq)[a * astride + at] : make_float2(0.f, 0.f);
                } else {
                    const uint32_t w = in ? *reinterpret_cast<const uint32_t*>(static_cast<const uint16_t*>(iq) +
                                                                               a * astride + at)
                                          : 0u;
                    x[0] = in ? decode_u8iq(w & 0xFFFFu) : make_float2(0.f, 0.f);
                    x[1] = in ? decode_u8iq(w >> 16) : make_float2(0.f, 0.f);
                }
#pragma unroll
                for (int q = 0; q < V; ++q) {
                    S[(jj + q) * kStapRow + a] = (double)x[q].x;
                    S[(jj + q) * kStapRow + 8 + a] = (double)x[q].y;
                }
            }
        };
        if (t < kStapChunk / V) stage(kStapHalo + V * t);
        if (t < kStapHalo / V) stage(V * t);
        __syncthreads();
        const int w0 = c0 + 64 * wave;               // the wave's run of this chunk
        if (w0 < len) {
            const int steps = min(64, len - w0) / 4;
            for (int q = 0; q < steps; ++q) {
                const int j = kStapHalo + 64 * wave + 4 * q + k;
                const double av = S[j * kStapRow + r];
#pragma unroll
                for (int l = 0; l < T; ++l)
                    acc[l] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, S[(j - l) * kStapRow + r], acc[l], 0, 0, 0);
            }
        }
    }
    // the waves' tiles in wave order: ((w0 + w1) + w2) + w3; element (row, col) of lag l at l 256 + 16 row + col
    for (int w = 0; w < 4; ++w) {
        __syncthreads();
        if (wave == w) {
#pragma unroll
            for (int l = 0; l < T; ++l) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int at = l * 256 + (k + 4 * g) * 16 + r;
                    S[at] = w == 0 ? acc[l][g] : S[at] + acc[l][g];
                }
            }
        }
    }
    __syncthreads();
    const int NV = stap_values(A, T), N0 = A * (A + 1);
    for (int v = t; v < NV; v += kNulThreads) {
        int l = 0, a = 0, c;
        if (v < N0) {
            const int p = v >> 1;
            while ((a + 1) * (a + 2) / 2 <= p) ++a;
            c = p - a * (a + 1) / 2;
        } else {
            const int u = v - N0;
            l = 1 + u / (2 * A * A);
            const int p = (u % (2 * A * A)) >> 1;
            a = p / A;
            c = p % A;
        }
        const double* D = S + l * 256;
        double val;
        if (v & 1) val = (l == 0 && a == c) ? 0.0 : D[(a + 8) * 16 + c] - D[a * 16 + c + 8];     // IR - RI
        else val = D[a * 16 + c] + D[(a + 8) * 16 + c + 8];                                      // RR + II
        part[(size_t)blockIdx.x * NV + v] = val;
    }
}

#pragma clang fp contract(off)
__device__ __forceinline__ int stap_tri(int i, int j) { return i * (i + 1) / 2 + j; }    // i >= j

// w32: [nb][56] (K used), w64: [nb][A][T][2]
__global__ __launch_bounds__(64) void stap_solve_kernel(const double* __restrict__ part, int n, int ns, int A, int T,
                                                        double load, double min_db, float2* __restrict__ w32,
                                                        double* __restrict__ w64, int32_t* __restrict__ flags,
                                                        float* __restrict__ gain) {
    constexpr int NT = kStapMaxK * (kStapMaxK + 1) / 2;
    __shared__ double Cs[stap_values(kNulMaxA, kStapMaxT)];
    __shared__ double Lr[NT], Li[NT];
    __shared__ double Yr[kStapMaxK], Yi[kStapMaxK], Ur[kStapMaxK], Ui[kStapMaxK];
    const int t = threadIdx.x, b = blockIdx.x;
    const int K = A * T, kc = (T - 1) / 2, NV = stap_values(A, T);
    for (int v = t; v < NV; v += 64) Cs[v] = nul_slice_sum(part, b, ns, NV, v);
    __syncthreads();
    const double dn = (double)n;
    auto lag = [&](int a, int c, int l) -> NulZ {      // r_ac(l) / n, l >= 0
        if (l == 0) {
            if (a >= c) {
                const int p = a * (a + 1) / 2 + c;
                return {Cs[2 * p] / dn, a == c ? 0.0 : Cs[2 * p + 1] / dn};
            }
            const int p = c * (c + 1) / 2 + a;
            return {Cs[2 * p] / dn, -(Cs[2 * p + 1] / dn)};
        }
        const int o = A * (A + 1) + (l - 1) * 2 * A * A + 2 * (a * A + c);
        return {Cs[o] / dn, Cs[o + 1] / dn};
    };
    double tr = 0.0;
    for (int a = 0; a < A; ++a) tr += lag(a, a, 0).re;
    const double p00 = lag(0, 0, 0).re;
    const double delta = load * tr / (double)A;
    if (t < K) {                                       // row t = k(a, ta) of the lower triangle
        const int a = t / T, ta = t % T;
        for (int j = 0; j <= t; ++j) {
            const int c = j / T, tc = j % T;
            NulZ v = tc >= ta ? lag(a, c, tc - ta) : nul_conj(lag(c, a, ta - tc));
            if (j == t) v = {v.re + delta, 0.0};
            Lr[stap_tri(t, j)] = v.re;
            Li[stap_tri(t, j)] = v.im;
        }
    }
    __syncthreads();
    // R = L L^H in place, column by column, lane t on row t
    bool ok = true;
    for (int j = 0; j < K; ++j) {
        NulZ v = {0.0, 0.0};
        if (t >= j && t < K) {
            v = {Lr[stap_tri(t, j)], Li[stap_tri(t, j)]};
            if (t == j) {
                double d = v.re;
                for (int q = 0; q < j; ++q) {
                    const double lr = Lr[stap_tri(j, q)], li = Li[stap_tri(j, q)];
                    d -= lr * lr + li * li;
                }
                v = {d, 0.0};
            } else {
                for (int q = 0; q < j; ++q) {
                    const NulZ li = {Lr[stap_tri(t, q)], Li[stap_tri(t, q)]};
                    const NulZ lj = {Lr[stap_tri(j, q)], Li[stap_tri(j, q)]};
                    v = nul_sub(v, nul_mul(li, nul_conj(lj)));
                }
            }
        }
        const double d = __shfl(v.re, j);
        if (!(d > 0.0) || !(d < INFINITY)) ok = false;
        const double l = sqrt(d);
        if (t == j) {
            Lr[stap_tri(j, j)] = l;
            Li[stap_tri(j, j)] = 0.0;
        } else if (t > j && t < K) {
            Lr[stap_tri(t, j)] = v.re / l;
            Li[stap_tri(t, j)] = v.im / l;
        }
        __syncthreads();
    }
    // L y = e_kc: lane t holds row t's right-hand side and subtracts column after column
    {
        NulZ v = {t == kc ? 1.0 : 0.0, 0.0};
        for (int q = 0; q < K; ++q) {
            const double lqq = Lr[stap_tri(q, q)];
            NulZ y = {v.re / lqq, v.im / lqq};
            y.re = __shfl(y.re, q);
            y.im = __shfl(y.im, q);
            if (t == q) {
                Yr[q] = y.re;
                Yi[q] = y.im;
            } else if (t > q && t < K) {
                const NulZ lt = {Lr[stap_tri(t, q)], Li[stap_tri(t, q)]};
                v = nul_sub(v, nul_mul(lt, y));
            }
        }
    }
    __syncthreads();
    // L^H u = y: rows descending, each sum in ascending column order
    if (t == 0) {
        for (int i = K - 1; i >= 0; --i) {
            NulZ v = {Yr[i], Yi[i]};
            for (int q = i + 1; q < K; ++q) {
                const NulZ lq = {Lr[stap_tri(q, i)], Li[stap_tri(q, i)]};
                const NulZ uq = {Ur[q], Ui[q]};
                v = nul_sub(v, nul_mul(nul_conj(lq), uq));
            }
            const double lii = Lr[stap_tri(i, i)];
            Ur[i] = v.re / lii;
            Ui[i] = v.im / lii;
        }
    }
    __syncthreads();
    const double uc = Ur[kc];
    double gdb = 0.0;
    if (ok) {
        gdb = 10.0 * log10(p00 * uc);
        if (!(gdb >= min_db)) ok = false;              // (a NaN passes through as well)
    }
    if (t == 0) {
        flags[b] = ok ? 1 : 0;
        gain[b] = (float)gdb;
    }
    if (t < K) {
        NulZ w = {t == kc ? 1.0 : 0.0, 0.0};
        if (ok && t != kc) w = {Ur[t] / uc, Ui[t] / uc};
        w64[((size_t)b * K + t) * 2] = w.re;
        w64[((size_t)b * K + t) * 2 + 1] = w.im;
        w32[(size_t)b * kStapMaxK + t] = make_float2((float)w.re, (float)w.im);
    }
}

// y[i] = sum_a sum_t conj(w32[a][t]) x_a[i + c - t], ascending a, ascending t within a
template <int FMT, int T>
__global__ __launch_bounds__(kNulThreads) void stap_apply_kernel(const void* __restrict__ iq, int n, int nc, int A,
                                                                 size_t astride, const float2* __restrict__ w32,
                                                                 const int32_t* __restrict__ flags,
                                                                 float2* __restrict__ out) {
    constexpr int V = FMT == 0 ? kNulApplyC64 : kNulApplyU8;
    constexpr int C = (T - 1) / 2, H = (C + 1) / 2 * 2;  // halo either side, whole sample pairs
    constexpr int W = V + 2 * H;
    const int b = blockIdx.x / nc, cc = blockIdx.x % nc;
    const int i = (cc * kNulThreads + (int)threadIdx.x) * V;
    if (i >= n) return;                                // (n is a multiple of 32: whole groups)
    const size_t at = (size_t)b * n + i;
    const bool on = flags[b] != 0;
    const float2* w = w32 + (size_t)b * kStapMaxK;
    float2 y[V];
    // the window i - H .. i + V + H - 1 of antenna a, zeros outside the block
    auto window = [&](int a, float2 (&win)[W]) {
#pragma unroll
        for (int p = 0; p < W; p += 2) {
            const int s = i - H + p;
            const bool in = s >= 0 && s < n;
            if constexpr (FMT == 0) {
                const float2* src = static_cast<const float2*>(iq) + a * astride + at;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (in) v = *reinterpret_cast<const float4*>(src + (p - H));
                win[p] = make_float2(v.x, v.y);
                win[p + 1] = make_float2(v.z, v.w);
            } else {
                const uint16_t* src = static_cast<const uint16_t*>(iq) + a * astride + at;
                win[p] = win[p + 1] = make_float2(0.f, 0.f);
                if (in) {
                    const uint32_t v = *reinterpret_cast<const uint32_t*>(src + (p - H));
                    win[p] = nul_raw(v, 0);
                    win[p + 1] = nul_raw(v, 1);
                }
            }
        }
    };
    if (!on) {
        NulSamples<FMT, V> x;
        x.load(iq, at);
#pragma unroll
        for (int q = 0; q < V; ++q) y[q] = x[q];
    } else {
        for (int a = 0; a < A; ++a) {
            float2 win[W];
            window(a, win);
#pragma unroll
            for (int tt = 0; tt < T; ++tt) {
                const float2 wt = w[a * T + tt];
#pragma unroll
                for (int q = 0; q < V; ++q) {
                    const float2 term = nul_term(wt, win[H + q + C - tt]);
                    y[q] = (a == 0 && tt == 0) ? term : nul_add(y[q], term);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < V; ++q)
            if (i + q < C || i + q >= n - C) y[q] = make_float2(0.f, 0.f);
    }
#pragma unroll
    for (int q = 0; q < V; q += 2)
        *reinterpret_cast<float4*>(out + at + q) = make_float4(y[q].x, y[q].y, y[q + 1].x, y[q + 1].y);
}
#pragma clang fp contract(fast)

}  // namespace gpsmi
