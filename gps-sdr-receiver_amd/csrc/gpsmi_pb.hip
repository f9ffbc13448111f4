// Pulse blanking ahead of acquisition and tracking (gpsmi_pb_*, include/gpsmi.h; DESIGN.md 4.2d;
// numpy restatement: tests/pb_ref.py).
//
// Per block of n samples: p_i = re*re + im*im in float32 (never fused), floor m = the lower median of
// p (order statistic (n - 1) / 2), T = m * 10^(thresh_db / 10); samples with p_i > T are detections,
// and every sample within [j - pre, j + post] of a detection j of the same block is zeroed, as are the
// first `carry` samples (the previous block's detections reaching past its end).  More than
// floor(max_frac * n) blanked samples: the block passes through, count -1, empty mask.
//
// The floor is an exact radix select on the float bits (p >= 0: the uint32 pattern orders like the
// float, bit 31 is 0; a NaN power, bit 31 cleared, sorts above +inf) in three digit passes of 11, 10
// and 10 bits:
//
//   pb_hist_kernel<PASS>    one workgroup per (block, slice of S samples): an LDS histogram of the
//                           pass's digit over the slice's samples whose higher digits equal the prefix
//                           found so far -> hist[block][slice][bins].  Integer LDS atomics only.
//   pb_select_kernel<PASS>  one workgroup per block: adds the slice histograms, finds the digit that
//                           holds the remaining rank, extends the prefix.  After the last pass: the
//                           floor, T, and the carry into the next block (its detections in the last
//                           `post` samples).
//   pb_apply_kernel         one workgroup per (block, slice): detection bits of the slice and a halo of
//                           post / pre samples into LDS as words, the last detection at or before each
//                           word by a prefix max, then every output sample, its mask bit and the
//                           slice's count.
//   pb_fixup_kernel         one workgroup per block: the block's count from the slice counts; over the
//                           limit, the block is rewritten from the input (decoded) and its mask cleared.
//                           Hands the last block's carry to the handle.
//
// The passes can run over chunks of blocks (GPSMI_PB_CHUNK_MIB), so that the re-reads of the second and
// third pass and of the apply come from the Infinity Cache; measured, the launches this adds cost more
// than the traffic saved, and one chunk is the default.  Everything is integer or one float32
// operation per value: the output does not depend on the grid, the slice size, the chunking, the
// number of blocks per call or the run.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "gpsmi_common.h"
#include "gpsmi_stage.h"

namespace gpsmi {

constexpr int kPbMaxGuard = 1024;                   // pre, post <= 1024
constexpr int kPbSliceBig = 8192;                   // samples per workgroup in a large call
constexpr int kPbSliceSmall = 2048;                 // ... and in a call of a few blocks
constexpr int kPbHaloWords = (kPbMaxGuard + 31) / 32;
constexpr int kPbMaxWords = kPbSliceBig / 32 + 2 * kPbHaloWords;     // detection words of a slice
constexpr int kPbNone = INT_MIN / 2;                // "no detection" (below any i - post)

// digit layout of pass 0 / 1 / 2: bits [shift, shift + bits) of the 31-bit key
template <int PASS> struct PbDigit;
template <> struct PbDigit<0> { static constexpr int shift = 20, bits = 11; };
template <> struct PbDigit<1> { static constexpr int shift = 10, bits = 10; };
template <> struct PbDigit<2> { static constexpr int shift = 0, bits = 10; };

#pragma clang fp contract(off)
// the power of one sample: two products and one add, each rounded (restated as numpy float32)
__device__ __forceinline__ float pb_power(float2 x) { return add_rn(mul_rn(x.x, x.x), mul_rn(x.y, x.y)); }
#pragma clang fp contract(fast)

__device__ __forceinline__ uint32_t pb_key(float p) { return __float_as_uint(p) & 0x7FFFFFFFu; }

// samples k and k + 1 (k even) of the input; complex64 rows must be 16-byte aligned (checked on entry)
template <int FMT>
__device__ __forceinline__ void pb_load2(const void* iq, size_t k, float2& a, float2& b) {
    if constexpr (FMT == 0) {
        const float4 v = *reinterpret_cast<const float4*>(static_cast<const float2*>(iq) + k);
        a = make_float2(v.x, v.y);
        b = make_float2(v.z, v.w);
    } else {
        const uint32_t v = *reinterpret_cast<const uint32_t*>(static_cast<const uint16_t*>(iq) + k);
        a = decode_u8iq(v & 0xFFFFu);
        b = decode_u8iq(v >> 16);
    }
}

// bits 0..15 of x to the even bits of the result
__device__ __forceinline__ uint32_t pb_spread(uint32_t x) {
    x = (x | (x << 8)) & 0x00FF00FFu;
    x = (x | (x << 4)) & 0x0F0F0F0Fu;
    x = (x | (x << 2)) & 0x33333333u;
    x = (x | (x << 1)) & 0x55555555u;
    return x;
}

// A wave covers 128 consecutive samples (4 words), lane l the samples 2 l and 2 l + 1: word k of the
// group from the two ballots (lanes 16 k .. 16 k + 15), bit i % 32 = sample i.
__device__ __forceinline__ uint32_t pb_word(unsigned long long even, unsigned long long odd, int k) {
    const uint32_t e = (uint32_t)(even >> (16 * k)) & 0xFFFFu, o = (uint32_t)(odd >> (16 * k)) & 0xFFFFu;
    return pb_spread(e) | (pb_spread(o) << 1);
}

template <int FMT, int PASS>
__global__ __launch_bounds__(256) void pb_hist_kernel(const void* __restrict__ iq, int n, int ns, int S,
                                                      int b0, const uint2* __restrict__ sel,
                                                      uint32_t* __restrict__ hist) {
    constexpr int NB = 1 << PbDigit<PASS>::bits, SH = PbDigit<PASS>::shift;
    constexpr int SH_HI = SH + PbDigit<PASS>::bits;
    __shared__ uint32_t h[NB];
    const int t = threadIdx.x;
    for (int d = t; d < NB; d += 256) h[d] = 0;
    const int bl = blockIdx.x / ns, s = blockIdx.x % ns;
    const int b = b0 + bl;
    const uint32_t prefix = PASS ? sel[b].x : 0u;
    const int i0 = s * S, i1 = min(i0 + S, n);
    const size_t base = (size_t)b * n;
    __syncthreads();
    for (int i = i0 + 2 * t; i < i1; i += 512) {
        float2 x0, x1;
        pb_load2<FMT>(iq, base + i, x0, x1);
        const uint32_t k0 = pb_key(pb_power(x0)), k1 = pb_key(pb_power(x1));
        if (PASS == 0 || (k0 >> SH_HI) == prefix) atomicAdd(&h[(k0 >> SH) & (NB - 1)], 1u);
        if (PASS == 0 || (k1 >> SH_HI) == prefix) atomicAdd(&h[(k1 >> SH) & (NB - 1)], 1u);
    }
    __syncthreads();
    uint32_t* o = hist + (size_t)blockIdx.x * NB;
    for (int d = t; d < NB; d += 256) o[d] = h[d];
}

// sel[b] = (prefix of the digits found, remaining rank inside it).  After PASS 2 the prefix is the
// floor's bit pattern: floors[b], thr[b] = floor * f, carries[b + 1] = the carry into block b + 1.
template <int FMT, int PASS>
__global__ __launch_bounds__(256) void pb_select_kernel(const uint32_t* __restrict__ hist, int ns, int n,
                                                        int b0, uint2* __restrict__ sel, float f,
                                                        const void* __restrict__ iq, int post,
                                                        float* __restrict__ floors, float* __restrict__ thr,
                                                        int* __restrict__ carries) {
    constexpr int NB = 1 << PbDigit<PASS>::bits, K = NB / 256;
    __shared__ uint32_t scan[256];
    __shared__ uint32_t res_key;
    __shared__ int last_det;
    __shared__ uint2 st_s;
    const int t = threadIdx.x, bl = blockIdx.x, b = b0 + bl;
    if (t == 0) st_s = PASS ? sel[b] : make_uint2(0u, (uint32_t)(n - 1) / 2u);   // (read before any write)
    uint32_t c[K], tot = 0;
#pragma unroll
    for (int q = 0; q < K; ++q) c[q] = 0;
    const uint32_t* src = hist + (size_t)bl * ns * NB + (size_t)t * K;
    for (int s = 0; s < ns; ++s) {
#pragma unroll
        for (int q = 0; q < K; ++q) c[q] += src[(size_t)s * NB + q];
    }
#pragma unroll
    for (int q = 0; q < K; ++q) tot += c[q];
    scan[t] = tot;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {           // inclusive prefix sum over the threads
        const uint32_t v = t >= off ? scan[t - off] : 0u;
        __syncthreads();
        scan[t] += v;
        __syncthreads();
    }
    const uint2 st = st_s;
    uint32_t before = scan[t] - tot;                     // samples in the bins below thread t's
    const uint32_t rank = st.y;
    if (rank >= before && rank < before + tot) {         // (exactly one thread)
#pragma unroll
        for (int q = 0; q < K; ++q) {
            if (rank >= before && rank < before + c[q]) {
                const uint32_t key = (st.x << PbDigit<PASS>::bits) | (uint32_t)(t * K + q);
                sel[b] = make_uint2(key, rank - before);
                res_key = key;
            }
            before += c[q];
        }
    }
    if constexpr (PASS == 2) {
        if (t == 0) last_det = -1;
        __syncthreads();
        const float m = __uint_as_float(res_key);
        const float T = mul_rn(m, f);
        if (t == 0) {
            floors[b] = m;
            thr[b] = T;
        }
        const size_t base = (size_t)b * n;
        for (int j = n - post + t; j < n; j += 256) {   // (n - post >= n - 1024 >= 1024: whole samples)
            const float2 x = load_iq<FMT>(iq, base + j);
            if (pb_power(x) > T) atomicMax(&last_det, j);
        }
        __syncthreads();
        if (t == 0) carries[b + 1] = last_det >= 0 ? last_det + post - n + 1 : 0;
    }
}

template <int FMT>
__global__ __launch_bounds__(256) void pb_apply_kernel(const void* __restrict__ iq, int n, int ns, int S,
                                                       int b0, int pre, int post,
                                                       const float* __restrict__ thr,
                                                       const int* __restrict__ carries,
                                                       const int* __restrict__ state,
                                                       float2* __restrict__ out, uint32_t* __restrict__ masks,
                                                       int* __restrict__ scount) {
    __shared__ uint32_t D[kPbMaxWords];                  // detection words [wa, wb)
    __shared__ int P[2 * 256];                           // prefix max of the last detection per word
    __shared__ int cnt;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int b = b0 + blockIdx.x / ns, s = blockIdx.x % ns;
    const int nw = n / 32;
    const int ws0 = s * (S / 32), ws1 = min(ws0 + S / 32, nw);
    const int wa = max(0, ws0 - (post + 31) / 32), wb = min(nw, ws1 + (pre + 31) / 32);
    const int W = wb - wa;
    const size_t base = (size_t)b * n;
    const float T = thr[b];
    const int carry = b == 0 ? state[0] : carries[b];
    if (t == 0) cnt = 0;
    // detection words: group g = words wa + 4 g .. wa + 4 g + 3
    for (int g = wave; 4 * g < W; g += 4) {
        const int w = wa + 4 * g + (lane >> 4);
        bool d0 = false, d1 = false;
        if (w < wb) {
            float2 x0, x1;
            pb_load2<FMT>(iq, base + (size_t)w * 32 + 2 * (lane & 15), x0, x1);
            d0 = pb_power(x0) > T;
            d1 = pb_power(x1) > T;
        }
        const unsigned long long e = __ballot(d0), o = __ballot(d1);
        if (lane < 4 && 4 * g + lane < W) D[4 * g + lane] = pb_word(e, o, lane);
    }
    __syncthreads();
    // P[w] = the last detection (sample index in the block) in words wa .. wa + w
    for (int r = 0; r < 2; ++r) {
        const int w = t + 256 * r;
        int v = kPbNone;
        if (w < W && D[w]) v = 32 * (wa + w) + 31 - __clz(D[w]);
        P[w] = v;
    }
    __syncthreads();
    for (int off = 1; off < W; off <<= 1) {
        int v[2];
        for (int r = 0; r < 2; ++r) {
            const int w = t + 256 * r;
            v[r] = w >= off ? max(P[w], P[w - off]) : P[w];
        }
        __syncthreads();
        for (int r = 0; r < 2; ++r) P[t + 256 * r] = v[r];
        __syncthreads();
    }
    // output: the slice's words [ws0, ws1), 4 per wave step
    int my = 0;
    for (int w4 = ws0 + 4 * wave; w4 < ws1; w4 += 16) {
        const int w = w4 + (lane >> 4);
        bool z0 = false, z1 = false;
        if (w < ws1) {
            const int i = 32 * w + 2 * (lane & 15);
            float2 x0, x1;
            pb_load2<FMT>(iq, base + i, x0, x1);
            bool z[2];
            for (int e = 0; e < 2; ++e) {
                const int ie = i + e;
                const int k = min(ie + pre, n - 1);
                const int wk = k / 32 - wa;
                const uint32_t bits = D[wk] & (0xFFFFFFFFu >> (31 - (k & 31)));
                const int last = bits ? 32 * (wk + wa) + 31 - __clz(bits) : (wk > 0 ? P[wk - 1] : kPbNone);
                z[e] = last >= ie - post || ie < carry;
            }
            z0 = z[0];
            z1 = z[1];
            const float4 v = make_float4(z0 ? 0.f : x0.x, z0 ? 0.f : x0.y, z1 ? 0.f : x1.x, z1 ? 0.f : x1.y);
            *reinterpret_cast<float4*>(out + base + i) = v;
        }
        const unsigned long long e = __ballot(z0), o = __ballot(z1);
        if (lane < 4 && w4 + lane < ws1) {
            const uint32_t word = pb_word(e, o, lane);
            if (masks) masks[(size_t)b * nw + w4 + lane] = word;
            my += __popc(word);
        }
    }
    __syncthreads();
    if (my) atomicAdd(&cnt, my);
    __syncthreads();
    if (t == 0) scount[(size_t)b * ns + s] = cnt;
}

// counts[b] from the slice counts; a block over the limit passes through.  The last block of the call
// hands its carry to the handle (after every apply has read the handle's carry for block 0).
template <int FMT>
__global__ __launch_bounds__(256) void pb_fixup_kernel(const void* __restrict__ iq, int n, int ns, int nb,
                                                       int limit, const int* __restrict__ scount,
                                                       const int* __restrict__ carries,
                                                       int* __restrict__ state, int32_t* __restrict__ counts,
                                                       float2* __restrict__ out, uint32_t* __restrict__ masks) {
    __shared__ int total;
    const int t = threadIdx.x, b = blockIdx.x;
    if (t == 0) {
        int c = 0;
        for (int s = 0; s < ns; ++s) c += scount[(size_t)b * ns + s];
        total = c;
        counts[b] = c > limit ? -1 : c;
        if (b == nb - 1) state[0] = carries[nb];
    }
    __syncthreads();
    if (total <= limit) return;
    const size_t base = (size_t)b * n;
    for (int i = 2 * t; i < n; i += 512) {
        float2 x0, x1;
        pb_load2<FMT>(iq, base + i, x0, x1);
        *reinterpret_cast<float4*>(out + base + i) = make_float4(x0.x, x0.y, x1.x, x1.y);
    }
    if (masks)
        for (int w = t; w < n / 32; w += 256) masks[(size_t)b * (n / 32) + w] = 0u;
}

}  // namespace gpsmi

using namespace gpsmi;

struct gpsmi_pb {
    gpsmi_pb_cfg cfg;
    DevBuf<int> d_state;                                  // the carry into the next call's block 0
    DevBuf<uint32_t> d_hist;                              // [chunk blocks][slices][2048]
    DevBuf<uint2> d_sel; DevBuf<float> d_floors, d_thr;   // [blocks]
    DevBuf<int> d_carries; DevBuf<int32_t> d_counts;      // [blocks + 1], [blocks]
    DevBuf<int> d_scount;                                 // [blocks][slices]
    DevBuf<uint32_t> d_masks;                             // [blocks][n / 32]
    float f = 0.f;                                        // 10^(thresh_db / 10) as float32
    int limit = 0;                                        // floor(max_frac * n)
    size_t chunk_bytes = 0;                               // input bytes per chunk (0: one chunk)
    BlockStage blk;
    StageSync sync;                                       // last: see gpsmi_stage.h
};

static int pb_build(gpsmi_pb* h) {
    h->blk.block_samples = h->cfg.block_samples;
    const int rc = h->d_state.reserve_zeroed(1, "pulse blanking carry");
    if (rc) return rc;
    h->f = (float)pow(10.0, (double)h->cfg.thresh_db / 10.0);
    h->limit = (int)floor((double)h->cfg.max_frac * (double)h->cfg.block_samples);
    if (const char* e = getenv("GPSMI_PB_CHUNK_MIB")) h->chunk_bytes = (size_t)strtoull(e, nullptr, 10) << 20;
    return GPSMI_OK;
}

// per-block result arrays for nb blocks (the carries: nb + 1)
static int pb_results(gpsmi_pb* h, int nb) {
    int rc = h->d_sel.reserve(nb, "pulse blanking results");
    if (!rc) rc = h->d_floors.reserve(nb, "pulse blanking results");
    if (!rc) rc = h->d_thr.reserve(nb, "pulse blanking results");
    if (!rc) rc = h->d_carries.reserve((size_t)nb + 1, "pulse blanking results");
    if (!rc) rc = h->d_counts.reserve(nb, "pulse blanking results");
    return rc;
}

// Every pass over nb blocks at d_iq (device, the handle's input format) into d_out; want_masks: write
// the mask words into the handle's buffer.
static int pb_run(gpsmi_pb* h, const void* d_iq, void* d_out, int nb, bool want_masks) {
    const int n = h->cfg.block_samples;
    const size_t blk_bytes = h->blk.in_bytes(1);
    const int S = nb >= 16 ? kPbSliceBig : kPbSliceSmall;
    const int ns = (n + S - 1) / S;
    int cb = h->chunk_bytes ? (int)std::max<size_t>(1, h->chunk_bytes / blk_bytes) : nb;
    cb = std::min(cb, nb);
    int rc = pb_results(h, nb);
    if (!rc) rc = h->d_hist.reserve((size_t)cb * ns * 2048, "pulse blanking histograms");
    if (!rc) rc = h->d_scount.reserve((size_t)nb * ns, "pulse blanking slice counts");
    if (!rc && want_masks) rc = h->d_masks.reserve((size_t)nb * (n / 32), "pulse blanking masks");
    if (rc) return rc;
    uint32_t* masks = want_masks ? h->d_masks.p : nullptr;
    float2* out = static_cast<float2*>(d_out);
    const int pre = h->cfg.pre, post = h->cfg.post;
    const hipStream_t st = h->sync.stream;
    if ((rc = h->sync.begin())) return rc;
    for (int b0 = 0; b0 < nb; b0 += cb) {
        const int m = std::min(cb, nb - b0);
        const dim3 g((unsigned)(m * ns)), gb((unsigned)m), blk(256);
        with_fmt(h->blk.fmt, [&](auto fmt) {
            constexpr int FMT = decltype(fmt)::value;
            hipLaunchKernelGGL((pb_hist_kernel<FMT, 0>), g, blk, 0, st, d_iq, n, ns, S, b0, h->d_sel.p,
                               h->d_hist.p);
            hipLaunchKernelGGL((pb_select_kernel<FMT, 0>), gb, blk, 0, st, h->d_hist.p, ns, n, b0, h->d_sel.p,
                               h->f, d_iq, post, h->d_floors.p, h->d_thr.p, h->d_carries.p);
            hipLaunchKernelGGL((pb_hist_kernel<FMT, 1>), g, blk, 0, st, d_iq, n, ns, S, b0, h->d_sel.p,
                               h->d_hist.p);
            hipLaunchKernelGGL((pb_select_kernel<FMT, 1>), gb, blk, 0, st, h->d_hist.p, ns, n, b0, h->d_sel.p,
                               h->f, d_iq, post, h->d_floors.p, h->d_thr.p, h->d_carries.p);
            hipLaunchKernelGGL((pb_hist_kernel<FMT, 2>), g, blk, 0, st, d_iq, n, ns, S, b0, h->d_sel.p,
                               h->d_hist.p);
            hipLaunchKernelGGL((pb_select_kernel<FMT, 2>), gb, blk, 0, st, h->d_hist.p, ns, n, b0, h->d_sel.p,
                               h->f, d_iq, post, h->d_floors.p, h->d_thr.p, h->d_carries.p);
            hipLaunchKernelGGL((pb_apply_kernel<FMT>), g, blk, 0, st, d_iq, n, ns, S, b0, pre, post,
                               h->d_thr.p, h->d_carries.p, h->d_state.p, out, masks, h->d_scount.p);
        });
    }
    with_fmt(h->blk.fmt, [&](auto fmt) {
        hipLaunchKernelGGL(pb_fixup_kernel<decltype(fmt)::value>, dim3((unsigned)nb), dim3(256), 0, st, d_iq,
                           n, ns, nb, h->limit, h->d_scount.p, h->d_carries.p, h->d_state.p, h->d_counts.p, out, masks);
    });
    return h->sync.end();
}

static int pb_finish(gpsmi_pb* h, int nb, int32_t* counts, float* floors, uint32_t* masks) {
    const int n = h->cfg.block_samples;
    const hipStream_t st = h->sync.stream;
    if (counts)
        GPSMI_HIP(hipMemcpyAsync(counts, h->d_counts.p, (size_t)nb * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (floors)
        GPSMI_HIP(hipMemcpyAsync(floors, h->d_floors.p, (size_t)nb * sizeof(float), hipMemcpyDeviceToHost, st));
    if (masks)
        GPSMI_HIP(hipMemcpyAsync(masks, h->d_masks.p, (size_t)nb * (n / 32) * sizeof(uint32_t),
                                 hipMemcpyDeviceToHost, st));
    return h->sync.finish();
}

extern "C" {

int gpsmi_pb_create(const gpsmi_pb_cfg* cfg, gpsmi_pb** out) {
    GPSMI_REQUIRE(cfg && out, "null argument");
    *out = nullptr;
    const int32_t n = cfg->block_samples;
    GPSMI_REQUIRE(n >= 2048 && n <= (1 << 24) && n % 32 == 0,
                  "block_samples is not a multiple of 32 in 2048..2^24");
    GPSMI_REQUIRE(!std::isnan(cfg->thresh_db), "thresh_db is NaN");
    GPSMI_REQUIRE(cfg->pre >= 0 && cfg->pre <= kPbMaxGuard, "pre out of range 0..1024");
    GPSMI_REQUIRE(cfg->post >= 0 && cfg->post <= kPbMaxGuard, "post out of range 0..1024");
    GPSMI_REQUIRE(cfg->max_frac >= 0.f && cfg->max_frac <= 1.f, "max_frac out of range 0..1");
    return stage_create(cfg, out, pb_build);
}

int gpsmi_pb_destroy(gpsmi_pb* h) { return stage_destroy(h); }

int gpsmi_pb_set_input_format(gpsmi_pb* h, int fmt) { return stage_set_input_format(h, fmt, __func__); }

int gpsmi_pb_reset(gpsmi_pb* h) {
    GPSMI_REQUIRE(h, "null handle");
    GPSMI_HIP(hipSetDevice(h->cfg.device));
    GPSMI_HIP(hipMemsetAsync(h->d_state.p, 0, sizeof(int), h->sync.stream));
    GPSMI_HIP(hipStreamSynchronize(h->sync.stream));
    return GPSMI_OK;
}

int gpsmi_pb_apply_dev(gpsmi_pb* h, const void* d_iq, void* d_out, int nb, int32_t* counts, float* floors,
                       uint32_t* masks) {
    int rc = stage_check_call(h, d_iq, d_out, nb, __func__, "blanking", true);
    if (rc) return rc;
    GPSMI_HIP(hipSetDevice(h->cfg.device));
    rc = pb_run(h, d_iq, d_out, nb, masks != nullptr);
    if (rc) return rc;
    return pb_finish(h, nb, counts, floors, masks);
}

int gpsmi_pb_apply(gpsmi_pb* h, const void* iq, float* out, int nb, int32_t* counts, float* floors,
                   uint32_t* masks) {
    int rc = stage_check_call(h, iq, out, nb, __func__, "blanking", false);
    if (rc) return rc;
    GPSMI_HIP(hipSetDevice(h->cfg.device));
    return h->blk.apply_host(
        iq, out, nb, h->blk.out_bytes(nb), h->sync.stream, "pulse blanking staging",
        [&](const void* d_iq, void* d_out) { return pb_run(h, d_iq, d_out, nb, masks != nullptr); },
        [&] { return pb_finish(h, nb, counts, floors, masks); });
}

int gpsmi_pb_last_ms(gpsmi_pb* h, float* ms) { return stage_last_ms(h, ms, __func__); }

}  // extern "C"
