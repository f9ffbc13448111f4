// Time-frequency excision against swept and chirp interference, ahead of acquisition and tracking
// (gpsmi_tfx_*, include/gpsmi.h; numpy restatement: tests/tfx_ref.py).
//
// A block of n complex samples is cut into short frames of L = 32 / 64 / 128 / 256 samples at hop
// H = L / 2: frame f covers block samples [f H - H, f H + H), frame 0 starts in the carry (the previous
// block's last H input samples).  Periodic Hann window, except the last frame, whose second half is
// weighted 1: the frames sum to 1 at every sample and output block k needs input blocks k - 1 and k
// only.  A sweep is narrow in every frame: the cells P[f][k] = |FFT(w x_f)[k]|^2 far above the block's
// lower median are zeroed, each widened by +-dilate bins inside its frame, and the frames transformed
// back and overlap-added.
//
//   tfx_power_kernel   one workgroup per (block, run of frames): L / 8 lanes transform one frame, 8
//                      points per lane (the butterflies of gpsmi_fft.h, one or two exchanges through
//                      LDS), 2048 / L frames at a time; P -> scratch [block][frame][L].
//   tfx_select_kernel  one workgroup per block: the lower median of the (nf - 1) L cells of all frames
//                      but the last, an exact radix select on the float bits in three digit passes of
//                      11, 10 and 10 bits (LDS integer histograms, as gpsmi_pb), then T and the last
//                      frame's T * 11/6.
//   tfx_mask_kernel    one workgroup per (block, slice of cells): P > T per cell from the scratch, the
//                      detection words by wave ballots, widened circularly inside each frame on the
//                      words -> masks, and the slice's count.
//   tfx_apply_kernel   one workgroup per (block, 2048 / L runs of K output segments): a group of L / 8
//                      lanes walks the frames of its run in order: forward transform, the masked
//                      cells zeroed, back (ifft(Y) = conj(fft(conj Y)) / L), segment s = frame s's
//                      second half + frame s + 1's first half, both in the same lane's registers.
//                      A block whose count (the sum of its slice counts) is over the limit is copied
//                      through instead, its mask words cleared, count -1.
//   tfx_carry_kernel   the last block's final H input samples (decoded) -> the handle's carry.
//
// The mask is made from the stored P alone, by comparisons and integer operations: floors, masks and
// counts follow exactly from gpsmi_tfx_last_power.  No float atomics, every output sample is written
// once by one lane, every frame is transformed by the same instructions wherever it lands: the bits
// do not depend on the grid, on nb or on the cut of the input into calls.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gpsmi_common.h"
#include "gpsmi_fft.h"
#include "gpsmi_stage.h"

namespace gpsmi {

constexpr int kTfxMaxL = 256;
constexpr int kTfxMaxDilate = 8;
constexpr int kTfxTile = 2048;                      // cells (and frame points) a workgroup holds at a time
constexpr int kTfxSliceSteps = 8;                   // tiles per workgroup of the mask pass

#pragma clang fp contract(off)
// the power of one cell: two products and one add, each rounded
__device__ __forceinline__ float tfx_power(fft_c x) { return add_rn(mul_rn(x.x, x.x), mul_rn(x.y, x.y)); }
#pragma clang fp contract(fast)

// The last pass of a transform, radix R with Ns = L / R: a lane holds z[j + M i] in v[i] and makes the
// 8 / R butterflies jj = j + M b, inputs and outputs in the slots b + (8 / R) r.
template <int R, int L>
__device__ __forceinline__ void tfx_last_pass(fft_c* v, const fft_c* tw, int j) {
    constexpr int M = L / 8, NBF = 8 / R;
#pragma unroll
    for (int b = 0; b < NBF; ++b) {
        const int jj = j + M * b;
        if constexpr (R == 4) {
            fft_c z0 = v[b];
            fft_c z1 = cmulp(v[b + NBF], tw[jj]);
            fft_c z2 = cmulp(v[b + 2 * NBF], tw[2 * jj]);
            fft_c z3 = cmulp(v[b + 3 * NBF], tw[3 * jj]);
            dft4p<false>(z0, z1, z2, z3);
            v[b] = z0; v[b + NBF] = z1; v[b + 2 * NBF] = z2; v[b + 3 * NBF] = z3;
        } else {
            const fft_c z0 = v[b], z1 = cmulp(v[b + NBF], tw[jj]);
            v[b] = z0 + z1;
            v[b + NBF] = z0 - z1;
        }
    }
}

// one pad element per 8 in the exchange buffer: the stride-8 scatters and the unit-stride gathers of a
// wave then fall on different banks
__device__ __forceinline__ int tfx_pad(int i) { return i + (i >> 3); }
constexpr int kTfxBuf = kTfxTile + kTfxTile / 8;

// L-point forward transform on L / 8 lanes, Stockham radix 8-4 (L = 32), 8-8 (64), 8-8-2 (128),
// 8-8-4 (256).  Lane j enters with x[j + M r] in v[r] and leaves with X[j + M q] in v[q], M = L / 8.
// buf: the L + L / 8 elements of this frame in LDS; tw[k] = exp(-2 pi i k / L) in LDS.  Every lane of the
// workgroup calls it (the exchanges are workgroup barriers); the caller puts a barrier between the
// last read of one transform and the first write of the next.
template <int L>
__device__ __forceinline__ void tfx_fft(fft_c* v, fft_c* buf, const fft_c* tw, int j) {
    constexpr int M = L / 8;
    dft8p(v);                                        // Ns = 1: out index 8 j + r
#pragma unroll
    for (int r = 0; r < 8; ++r) buf[9 * j + r] = v[r];            // (tfx_pad(8 j + r))
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] = buf[tfx_pad(j + M * r)];
    if constexpr (L == 32) {
        tfx_last_pass<4, L>(v, tw, j);
    } else {
        const int k = j & 7;                         // Ns = 8: twiddle exp(-2 pi i r k / 64)
#pragma unroll
        for (int r = 1; r < 8; ++r) v[r] = cmulp(v[r], tw[r * k * (L / 64)]);
        dft8p(v);                                    // out index (j / 8) 64 + k + 8 r (L = 64: j + M r)
        if constexpr (L > 64) {
            __syncthreads();
            const int base = (j >> 3) * 64 + k;
#pragma unroll
            for (int r = 0; r < 8; ++r) buf[tfx_pad(base) + 9 * r] = v[r];
            __syncthreads();
#pragma unroll
            for (int r = 0; r < 8; ++r) v[r] = buf[tfx_pad(j + M * r)];
            tfx_last_pass<L / 64, L>(v, tw, j);
        }
    }
}

// sample g (block offset, >= -H) of block b: negative offsets of block 0 of a call come from the carry,
// those of later blocks from the block before (contiguous)
template <int FMT, int L>
__device__ __forceinline__ float2 tfx_load(const void* iq, const float2* carry, int b, int n, int g) {
    if (b == 0 && g < 0) return carry[g + L / 2];
    return load_iq<FMT>(iq, (size_t)((long long)b * n + g));
}

// the windowed frame f of block b in the layout of tfx_fft (zeros when the frame does not exist)
template <int FMT, int L>
__device__ __forceinline__ void tfx_frame(const void* iq, const float2* carry, const float* w, int b, int n,
                                          int f, bool act, bool last, int j, fft_c* v) {
    constexpr int M = L / 8, H = L / 2;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        float2 x = make_float2(0.f, 0.f);
        if (act) x = tfx_load<FMT, L>(iq, carry, b, n, f * H - H + j + M * r);
        const float wr = (last && r >= 4) ? 1.0f : w[r];
        v[r] = fft_c{x.x * wr, x.y * wr};
    }
}

// grid: nb * wgs workgroups; workgroup wg of a block takes the frames (wg K + it) G + grp
template <int FMT, int L>
__global__ __launch_bounds__(256) void tfx_power_kernel(const void* __restrict__ iq,
                                                        const float2* __restrict__ carry,
                                                        const float* __restrict__ win,
                                                        const float2* __restrict__ tw, int n, int wgs, int K,
                                                        float* __restrict__ P) {
    constexpr int M = L / 8, G = 256 / M, H = L / 2;
    __shared__ __attribute__((aligned(16))) fft_c buf[kTfxBuf];
    __shared__ __attribute__((aligned(16))) fft_c twl[kTfxMaxL];
    const int t = threadIdx.x, grp = t / M, j = t % M;
    const int b = blockIdx.x / wgs, wg = blockIdx.x % wgs;
    const int nf = n / H;
    if (t < L) twl[t] = fft_c{tw[t].x, tw[t].y};
    float w[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) w[r] = win[j + M * r];
    for (int it = 0; it < K; ++it) {
        const int f = (wg * K + it) * G + grp;
        const bool act = f < nf;
        __syncthreads();
        fft_c v[8];
        tfx_frame<FMT, L>(iq, carry, w, b, n, f, act, f == nf - 1, j, v);
        tfx_fft<L>(v, buf + grp * (L + L / 8), twl, j);
        if (act) {
            float* o = P + ((size_t)b * nf + f) * L;
#pragma unroll
            for (int q = 0; q < 8; ++q) o[j + M * q] = tfx_power(v[q]);
        }
    }
}

// One workgroup per block: floors[b] = the order statistic (m - 1) / 2 of P[b][0 .. m), thr[b] = (T, T 11/6).
__global__ __launch_bounds__(1024) void tfx_select_kernel(const float* __restrict__ P, size_t stride, int m,
                                                          float f, float* __restrict__ floors,
                                                          float2* __restrict__ thr) {
    __shared__ uint32_t h[2048];
    __shared__ uint32_t scan[1024];
    __shared__ uint32_t s_prefix, s_rank;
    const int t = threadIdx.x, b = blockIdx.x;
    const float4* src = reinterpret_cast<const float4*>(P + (size_t)b * stride);   // (m % 32 == 0)
    uint32_t prefix = 0, rank = (uint32_t)(m - 1) / 2u;
    for (int pass = 0; pass < 3; ++pass) {
        const int bits = pass == 0 ? 11 : 10, shift = pass == 0 ? 20 : pass == 1 ? 10 : 0;
        const uint32_t nbins = 1u << bits;
        h[t] = 0;
        h[t + 1024] = 0;
        __syncthreads();
        for (int i = t; i < m / 4; i += 1024) {
            const float4 p = src[i];
            const uint32_t key[4] = {__float_as_uint(p.x) & 0x7FFFFFFFu, __float_as_uint(p.y) & 0x7FFFFFFFu,
                                     __float_as_uint(p.z) & 0x7FFFFFFFu, __float_as_uint(p.w) & 0x7FFFFFFFu};
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (pass == 0 || (key[e] >> (shift + bits)) == prefix)
                    atomicAdd(&h[(key[e] >> shift) & (nbins - 1)], 1u);
        }
        __syncthreads();
        const uint32_t c0 = h[2 * t], c1 = h[2 * t + 1];     // (bins past nbins stay 0)
        const uint32_t tot = c0 + c1;
        scan[t] = tot;
        __syncthreads();
        for (int off = 1; off < 1024; off <<= 1) {           // inclusive prefix sum over the threads
            const uint32_t v = t >= off ? scan[t - off] : 0u;
            __syncthreads();
            scan[t] += v;
            __syncthreads();
        }
        const uint32_t before = scan[t] - tot;
        if (rank >= before && rank < before + tot) {         // (exactly one thread)
            const bool second = rank >= before + c0;
            s_prefix = (prefix << bits) | (uint32_t)(2 * t + (second ? 1 : 0));
            s_rank = rank - before - (second ? c0 : 0u);
        }
        __syncthreads();
        prefix = s_prefix;
        rank = s_rank;
        __syncthreads();
    }
    if (t == 0) {
        const float fl = __uint_as_float(prefix);
        const float T = mul_rn(fl, f);
        floors[b] = fl;
        thr[b] = make_float2(T, mul_rn(T, (float)(11.0 / 6.0)));
    }
}

// grid: nb * ns workgroups, slice s of a block = the cells [s S, s S + S), S = kTfxSliceSteps tiles
// (whole frames: L divides the tile).  cells = nf L, lastc = (nf - 1) L: the last frame's first cell.
__global__ __launch_bounds__(256) void tfx_mask_kernel(const float* __restrict__ P, int cells, int lastc,
                                                       int ns, int mw, int dilate,
                                                       const float2* __restrict__ thr,
                                                       uint32_t* __restrict__ masks, int* __restrict__ scount) {
    __shared__ uint32_t raw[kTfxTile / 32];
    __shared__ int cnt;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int b = blockIdx.x / ns, s = blockIdx.x % ns;
    const float2 T = thr[b];
    const float* src = P + (size_t)b * cells;
    uint32_t* dst = masks + (size_t)b * (cells / 32);
    if (t == 0) cnt = 0;
    int my = 0;
    for (int step = 0; step < kTfxSliceSteps; ++step) {
        const int c0 = (s * kTfxSliceSteps + step) * kTfxTile;
        if (c0 >= cells) break;                              // (uniform)
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int c = c0 + 256 * q + t;
            bool d = false;
            if (c < cells) d = src[c] > (c >= lastc ? T.y : T.x);
            const unsigned long long bal = __ballot(d);      // cells c0 + 256 q + 64 wave + lane
            if (lane == 0) {
                raw[8 * q + 2 * wave] = (uint32_t)bal;
                raw[8 * q + 2 * wave + 1] = (uint32_t)(bal >> 32);
            }
        }
        __syncthreads();
        if (t < kTfxTile / 32 && c0 + 32 * t < cells) {
            const int i = t % mw, f0 = t - i;                // word i of its frame's mw words
            const uint32_t w = raw[t], lo = raw[f0 + (i + mw - 1) % mw], hi = raw[f0 + (i + 1) % mw];
            uint32_t m = w;
            for (int d = 1; d <= dilate; ++d)
                m |= (w << d) | (lo >> (32 - d)) | (w >> d) | (hi << (32 - d));
            dst[c0 / 32 + t] = m;
            my += __popc(m);
        }
    }
    __syncthreads();
    if (my) atomicAdd(&cnt, my);
    __syncthreads();
    if (t == 0) scount[(size_t)b * ns + s] = cnt;
}

// grid: nb * wgs workgroups; group grp of workgroup wg takes the output segments [s0, s0 + K),
// s0 = (wg G + grp) K, of its block: the frames s0 .. min(s0 + K, nf - 1).
template <int FMT, int L>
__global__ __launch_bounds__(256) void tfx_apply_kernel(const void* __restrict__ iq,
                                                        const float2* __restrict__ carry,
                                                        const float* __restrict__ win,
                                                        const float2* __restrict__ tw, int n, int wgs, int K,
                                                        int ns, int limit, const int* __restrict__ scount,
                                                        uint32_t* __restrict__ masks, int32_t* __restrict__ counts,
                                                        float2* __restrict__ out) {
    constexpr int M = L / 8, G = 256 / M, H = L / 2, MW = L / 32;
    __shared__ __attribute__((aligned(16))) fft_c buf[kTfxBuf];
    __shared__ __attribute__((aligned(16))) fft_c twl[kTfxMaxL];
    __shared__ int total;
    const int t = threadIdx.x, grp = t / M, j = t % M;
    const int b = blockIdx.x / wgs, wg = blockIdx.x % wgs;
    const int nf = n / H;
    if (t == 0) total = 0;
    if (t < L) twl[t] = fft_c{tw[t].x, tw[t].y};
    __syncthreads();
    {                                                         // the block's count: its slice counts, integers
        int c = 0;
        for (int s = t; s < ns; s += 256) c += scount[(size_t)b * ns + s];
        if (c) atomicAdd(&total, c);
    }
    __syncthreads();
    if (t == 0 && wg == 0) counts[b] = total > limit ? -1 : total;
    float2* o = out + (size_t)b * n;
    uint32_t* mk = masks + (size_t)b * nf * MW;
    if (total > limit) {                                      // too much of the plane: the block passes through
        const int a0 = min(wg * G * K, nf), a1 = min(a0 + G * K, nf);       // this workgroup's segments
        for (int i = a0 * H + t; i < a1 * H; i += 256) o[i] = load_iq<FMT>(iq, (size_t)b * n + i);
        for (int i = a0 * MW + t; i < a1 * MW; i += 256) mk[i] = 0u;
        return;
    }
    float w[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) w[r] = win[j + M * r];
    const int s0 = (wg * G + grp) * K, s1 = min(s0 + K, nf);
    const int f_end = min(s1, nf - 1);
    const float sc = 1.0f / (float)L;
    fft_c prev[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) prev[r] = fft_c{0.f, 0.f};
    for (int it = 0; it <= K; ++it) {
        const int f = s0 + it;
        const bool act = s0 < nf && f <= f_end;
        const bool last = f == nf - 1;
        __syncthreads();
        fft_c v[8];
        tfx_frame<FMT, L>(iq, carry, w, b, n, f, act, last, j, v);
        tfx_fft<L>(v, buf + grp * (L + L / 8), twl, j);
#pragma unroll
        for (int q = 0; q < 8; ++q) {                         // zero the flagged cells, conjugate for the inverse
            const int k = j + M * q;
            const bool z = act && ((mk[(size_t)f * MW + (k >> 5)] >> (k & 31)) & 1u);
            v[q] = z ? fft_c{0.f, 0.f} : fft_c{v[q].x, -v[q].y};
        }
        __syncthreads();
        tfx_fft<L>(v, buf + grp * (L + L / 8), twl, j);
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = fft_c{v[r].x * sc, -v[r].y * sc};
        if (act) {
            if (it > 0) {                                     // segment f - 1 is complete
                float2* d = o + (size_t)(f - 1) * H;
#pragma unroll
                for (int r = 0; r < 4; ++r) d[j + M * r] = make_float2(prev[r].x + v[r].x, prev[r].y + v[r].y);
            }
            if (last && f < s1) {                             // the last segment: frame nf - 1 alone
                float2* d = o + (size_t)f * H;
#pragma unroll
                for (int r = 0; r < 4; ++r) d[j + M * r] = make_float2(v[r + 4].x, v[r + 4].y);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) prev[r] = v[r + 4];
    }
}

template <int FMT>
__global__ __launch_bounds__(256) void tfx_carry_kernel(const void* __restrict__ iq, size_t tail, int H,
                                                        float2* __restrict__ carry) {
    for (int i = threadIdx.x; i < H; i += 256) carry[i] = load_iq<FMT>(iq, tail + i);
}

}  // namespace gpsmi

using namespace gpsmi;

struct gpsmi_tfx {
    gpsmi_tfx_cfg cfg;                       // as given; the resolved values follow
    int L = 64, dilate = 1, limit = 0;       // frame, widening, floor(max_frac nf L)
    float f = 0.f;                           // 10^(thresh_db / 10) as float32
    DevBuf<float2> d_tw;                     // exp(-2 pi i k / L)
    DevBuf<float> d_win;                     // periodic Hann, float32 of the double value
    DevBuf<float2> d_carry;                  // [H] complex64
    DevBuf<float> d_P;                       // [nb][nf][L]
    DevBuf<float> d_floors; DevBuf<float2> d_thr;         // [nb]
    DevBuf<int32_t> d_counts; DevBuf<int> d_scount;       // [nb], [nb][slices]
    DevBuf<uint32_t> d_masks;                // [nb][nf L / 32]
    int last_nb = 0;                         // blocks of the last call (0: none yet)
    BlockStage blk;
    StageSync sync;                          // last: see gpsmi_stage.h
};

static int tfx_build(gpsmi_tfx* h) {
    const gpsmi_tfx_cfg& c = h->cfg;
    h->blk.block_samples = c.block_samples;
    h->L = c.frame ? c.frame : 64;
    h->dilate = c.dilate < 0 ? 1 : c.dilate;
    const float db = c.thresh_db == 0.f ? 12.0f : c.thresh_db;
    h->f = (float)pow(10.0, (double)db / 10.0);
    const float frac = c.max_frac == 0.f ? 0.5f : c.max_frac;
    const int L = h->L;
    h->limit = (int)floor((double)frac * (double)(c.block_samples / (L / 2)) * (double)L);
    std::vector<float2> tw(L);
    std::vector<float> win(L);
    for (int k = 0; k < L; ++k) {
        const double a = 2.0 * M_PI * (double)k / (double)L;
        tw[k] = make_float2((float)cos(a), (float)-sin(a));
        win[k] = (float)(0.5 - 0.5 * cos(a));
    }
    int rc;
    if ((rc = h->d_tw.upload(tw, "sweep excision twiddles")) || (rc = h->d_win.upload(win, "sweep excision window")))
        return rc;
    return h->d_carry.reserve_zeroed(kTfxMaxL / 2, "sweep excision carry");
}

// Runs the passes over nb blocks at d_iq (device, the handle's input format) into d_out.
static int tfx_run(gpsmi_tfx* h, const void* d_iq, void* d_out, int nb) {
    const int n = h->cfg.block_samples, L = h->L, H = L / 2, nf = n / H;
    const int cells = nf * L, G = kTfxTile / L;
    h->last_nb = 0;                          // (the scratch is re-reserved: nothing to copy out until this call ran)
    const int ns = (cells + kTfxTile * kTfxSliceSteps - 1) / (kTfxTile * kTfxSliceSteps);
    int rc = h->d_P.reserve((size_t)nb * cells, "sweep excision powers");
    if (!rc) rc = h->d_masks.reserve((size_t)nb * (cells / 32), "sweep excision masks");
    if (!rc) rc = h->d_floors.reserve(nb, "sweep excision results");
    if (!rc) rc = h->d_thr.reserve(nb, "sweep excision results");
    if (!rc) rc = h->d_counts.reserve(nb, "sweep excision results");
    if (!rc) rc = h->d_scount.reserve((size_t)nb * ns, "sweep excision slice counts");
    if (rc) return rc;
    // frames per workgroup: runs of up to 8 steps (power) / 16 segments per group (apply) once the grid
    // has a few thousand workgroups anyway (same bits either way)
    const long long tiles = (long long)nb * ((nf + G - 1) / G);
    const int KP = tiles >= 16384 ? 8 : tiles >= 4096 ? 2 : 1;
    const int KA = tiles >= 16384 ? 16 : tiles >= 2048 ? 8 : 4;
    const int wgs_p = (nf + G * KP - 1) / (G * KP), wgs_a = (nf + G * KA - 1) / (G * KA);
    const size_t tail = (size_t)nb * n - H;
    const hipStream_t st = h->sync.stream;
    if ((rc = h->sync.begin())) return rc;
    with_fmt(h->blk.fmt, [&](auto fmt) {
        with_value<32, 128, 256, 64>(L, [&](auto len) {
            constexpr int FMT = decltype(fmt)::value, LL = decltype(len)::value;
            hipLaunchKernelGGL((tfx_power_kernel<FMT, LL>), dim3((unsigned)(nb * wgs_p)), dim3(256), 0, st, d_iq,
                               h->d_carry.p, h->d_win.p, h->d_tw.p, n, wgs_p, KP, h->d_P.p);
            hipLaunchKernelGGL(tfx_select_kernel, dim3((unsigned)nb), dim3(1024), 0, st, h->d_P.p, (size_t)cells,
                               cells - L, h->f, h->d_floors.p, h->d_thr.p);
            hipLaunchKernelGGL(tfx_mask_kernel, dim3((unsigned)(nb * ns)), dim3(256), 0, st, h->d_P.p, cells,
                               cells - L, ns, L / 32, h->dilate, h->d_thr.p, h->d_masks.p, h->d_scount.p);
            hipLaunchKernelGGL((tfx_apply_kernel<FMT, LL>), dim3((unsigned)(nb * wgs_a)), dim3(256), 0, st, d_iq,
                               h->d_carry.p, h->d_win.p, h->d_tw.p, n, wgs_a, KA, ns, h->limit, h->d_scount.p,
                               h->d_masks.p, h->d_counts.p, (float2*)d_out);
            hipLaunchKernelGGL(tfx_carry_kernel<FMT>, dim3(1), dim3(256), 0, st, d_iq, tail, H, h->d_carry.p);
        });
    });
    if (!(rc = h->sync.end())) h->last_nb = nb;
    return rc;
}

static int tfx_finish(gpsmi_tfx* h, int nb, int32_t* counts, float* floors, uint32_t* masks) {
    const size_t words = (size_t)(h->cfg.block_samples / (h->L / 2)) * (h->L / 32);
    const hipStream_t st = h->sync.stream;
    if (counts)
        GPSMI_HIP(hipMemcpyAsync(counts, h->d_counts.p, (size_t)nb * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (floors)
        GPSMI_HIP(hipMemcpyAsync(floors, h->d_floors.p, (size_t)nb * sizeof(float), hipMemcpyDeviceToHost, st));
    if (masks)
        GPSMI_HIP(hipMemcpyAsync(masks, h->d_masks.p, (size_t)nb * words * sizeof(uint32_t), hipMemcpyDeviceToHost,
                                 st));
    return h->sync.finish();
}

extern "C" {

int gpsmi_tfx_create(const gpsmi_tfx_cfg* cfg, gpsmi_tfx** out) {
    GPSMI_REQUIRE(cfg && out, "null argument");
    *out = nullptr;
    GPSMI_REQUIRE(!std::isnan(cfg->thresh_db), "thresh_db is NaN");
    GPSMI_REQUIRE(cfg->dilate >= -1 && cfg->dilate <= kTfxMaxDilate, "dilate out of range 0..8 (-1: the default, 1)");
    GPSMI_REQUIRE(cfg->max_frac >= 0.f && cfg->max_frac <= 1.f, "max_frac out of range 0..1");
    GPSMI_REQUIRE(cfg->keep_power == 0 || cfg->keep_power == 1, "keep_power is not 0 or 1");
    const int32_t n = cfg->block_samples, L = cfg->frame;
    if (n < 1024 || n > (1 << 24) || n % 128 != 0)
        return fail(GPSMI_E_UNSUPPORTED, "gpsmi_tfx_create: block_samples %d is not a multiple of 128 in 1024..2^24",
                    (int)n);
    if (L != 0 && L != 32 && L != 64 && L != 128 && L != 256)
        return fail(GPSMI_E_UNSUPPORTED, "gpsmi_tfx_create: frame %d is not 32, 64, 128 or 256 (0: 64)", (int)L);
    return stage_create(cfg, out, tfx_build);
}

int gpsmi_tfx_destroy(gpsmi_tfx* h) { return stage_destroy(h); }

int gpsmi_tfx_set_input_format(gpsmi_tfx* h, int fmt) { return stage_set_input_format(h, fmt, __func__); }

int gpsmi_tfx_reset(gpsmi_tfx* h) {
    GPSMI_REQUIRE(h, "null handle");
    GPSMI_HIP(hipSetDevice(h->cfg.device));
    GPSMI_HIP(hipMemsetAsync(h->d_carry.p, 0, (kTfxMaxL / 2) * sizeof(float2), h->sync.stream));
    GPSMI_HIP(hipStreamSynchronize(h->sync.stream));
    return GPSMI_OK;
}

int gpsmi_tfx_apply_dev(gpsmi_tfx* h, const void* d_iq, void* d_out, int nb, int32_t* counts, float* floors,
                        uint32_t* masks) {
    int rc = stage_check_call(h, d_iq, d_out, nb, __func__, "sweep excision", true);
    if (rc) return rc;
    GPSMI_HIP(hipSetDevice(h->cfg.device));
    rc = tfx_run(h, d_iq, d_out, nb);
    if (rc) return rc;
    return tfx_finish(h, nb, counts, floors, masks);
}

int gpsmi_tfx_apply(gpsmi_tfx* h, const void* iq, float* out, int nb, int32_t* counts, float* floors,
                    uint32_t* masks) {
    int rc = stage_check_call(h, iq, out, nb, __func__, "sweep excision", false);
    if (rc) return rc;
    GPSMI_HIP(hipSetDevice(h->cfg.device));
    return h->blk.apply_host(
        iq, out, nb, h->blk.out_bytes(nb), h->sync.stream, "sweep excision staging",
        [&](const void* d_iq, void* d_out) { return tfx_run(h, d_iq, d_out, nb); },
        [&] { return tfx_finish(h, nb, counts, floors, masks); });
}

int gpsmi_tfx_last_ms(gpsmi_tfx* h, float* ms) { return stage_last_ms(h, ms, __func__); }

int gpsmi_tfx_last_power(gpsmi_tfx* h, float* P) {
    GPSMI_REQUIRE(h && P, "null argument");
    if (!h->cfg.keep_power) return fail(GPSMI_E_STATE, "gpsmi_tfx_last_power: the handle was made without keep_power");
    if (h->last_nb <= 0) return fail(GPSMI_E_STATE, "gpsmi_tfx_last_power: no call yet");
    GPSMI_HIP(hipSetDevice(h->cfg.device));
    GPSMI_HIP(hipMemcpyAsync(P, h->d_P.p, (size_t)h->last_nb * h->cfg.block_samples * 2 * sizeof(float),
                             hipMemcpyDeviceToHost, h->sync.stream));
    GPSMI_HIP(hipStreamSynchronize(h->sync.stream));
    return GPSMI_OK;
}

}  // extern "C"
