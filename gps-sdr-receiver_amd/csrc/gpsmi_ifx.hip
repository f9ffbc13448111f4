// Narrowband interference excision ahead of acquisition and tracking (gpsmi_ifx_*, include/gpsmi.h;
// DESIGN.md 4.2b; numpy restatement: tests/ifx_ref.py).
//
// A block of n complex samples is cut into frames of L = 2048 at hop H = 1024: frame m covers block
// samples [m H - H, m H + H), frame 0 starts in the carry (the previous block's last H samples).
// Periodic Hann window, except the last frame, whose second half is weighted 1: the frames sum to 1
// at every sample of the block and the output of block k depends on input blocks k - 1 and k only.
//
//   ifx_psd_kernel    one workgroup per (block, group of kPsdGroup frames): sum of |FFT(w x_m)|^2
//                     over the group's frames in ascending order -> partial[block][group][2048].
//                     Frames 0 .. n/H - 2 take part (the flat-window last frame does not).
//   ifx_mask_kernel   one workgroup per block: P = (sum of the partials in group order) / (n/H - 1),
//                     floor = median(P) (bitonic sort of the 2048 values in LDS, the mean of the two
//                     middle ones), flag P > floor * 10^(thresh_db / 10), widen by +-dilate bins
//                     circularly, count; more than max_bins: count -1 and an empty mask.  The P it
//                     thresholded is kept per block for gpsmi_ifx_last_psd (a diagnostic).
//   ifx_apply_kernel  one workgroup per (block, run of consecutive output segments [s H, s H + H)):
//                     transforms the frames s0 .. s0 + S in order, zeroes the masked bins, transforms
//                     back (ifft(Y) = conj(fft(conj Y)) / L) and writes segment s = frame s's second
//                     half + frame s + 1's first half, in that order.  A thread holds samples
//                     t + 256 r of a frame (gpsmi_fft.h), so the two halves of a segment meet in the
//                     same thread's registers: every output sample is written once, by one add whose
//                     operands do not depend on the grid.  A block with count -1 is copied through.
//   ifx_carry_kernel  the last block's final H input samples (decoded) -> the handle's carry.
//
// No atomics: every sum has a fixed order, so the output bits do not depend on the grid, on the
// number of blocks per call or on the run.
//
// The first block after create / reset stands behind a zero carry: a strong tone then starts with a
// step at sample 0, which leaks across frame 0's spectrum.  A short block (4096 or 5120 samples:
// 3 or 4 frames in P) is classed wideband by it and passes through jammed (count -1); a longer one
// is excised with a wider mask than its successors (35 dB tone: some 170 bins at 20480, some 95
// at 65536).
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gpsmi_common.h"
#include "gpsmi_fft.h"
#include "gpsmi_stage.h"

namespace gpsmi {

constexpr int kIfxL = kFftN;             // frame length
constexpr int kIfxH = kFftN / 2;         // hop
constexpr int kPsdGroup = 8;             // frames per workgroup of the PSD pass (fixes the sum order)
constexpr int kMaskWords = kIfxL / 32;

// frame sample i (thread t holds i = t + 256 r) of frame `f` of block `b`; negative block offsets of
// block 0 of a call come from the carry, those of later blocks from the block before (contiguous)
template <int FMT>
__device__ __forceinline__ float2 ifx_load(const void* iq, const float2* carry, int b, int n, int g) {
    if (b == 0 && g < 0) return carry[g + kIfxH];
    return load_iq<FMT>(iq, (size_t)b * n + g);
}

template <int FMT>
__global__ __launch_bounds__(256) void ifx_psd_kernel(const void* __restrict__ iq,
                                                      const float2* __restrict__ carry,
                                                      const float* __restrict__ win, int n, int groups,
                                                      float* __restrict__ partial,
                                                      const float2* __restrict__ tw) {
    __shared__ __attribute__((aligned(16))) float lds[kFftLdsFloats];
    __shared__ __attribute__((aligned(16))) float lds_tw[kFftTwFloats];
    const int t = threadIdx.x;
    const int b = blockIdx.x / groups, grp = blockIdx.x % groups;
    const FftTw ftw = fft_setup(lds_tw, tw, t);
    float w[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) w[r] = win[t + 256 * r];
    const int f_end = min((grp + 1) * kPsdGroup, n / kIfxH - 1);
    float acc[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] = 0.f;
    __syncthreads();
    for (int f = grp * kPsdGroup; f < f_end; ++f) {
        float2 v[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const float2 x = ifx_load<FMT>(iq, carry, b, n, f * kIfxH - kIfxH + t + 256 * r);
            v[r] = make_float2(x.x * w[r], x.y * w[r]);
        }
        fft2048(v, lds, ftw, t);
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[q] += v[q].x * v[q].x + v[q].y * v[q].y;
        lds_barrier();               // (the next transform overwrites buffer 0)
    }
    float* out = partial + (size_t)blockIdx.x * kIfxL;
#pragma unroll
    for (int q = 0; q < 8; ++q) out[t + 256 * q] = acc[q];
}

__global__ __launch_bounds__(256) void ifx_mask_kernel(const float* __restrict__ partial, int groups,
                                                       int nframes, float scale, int dilate,
                                                       int max_bins, int32_t* __restrict__ counts,
                                                       uint32_t* __restrict__ masks,
                                                       float* __restrict__ psd) {
    __shared__ float P[kIfxL];
    __shared__ float srt[kIfxL];
    __shared__ int flag[kIfxL];
    __shared__ uint32_t words[kMaskWords];
    const int t = threadIdx.x, b = blockIdx.x;
    const float* src = partial + (size_t)b * groups * kIfxL;
    const float inv = (float)nframes;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int k = t + 256 * q;
        float s = 0.f;
        for (int g = 0; g < groups; ++g) s += src[(size_t)g * kIfxL + k];
        s = s / inv;
        P[k] = s;
        srt[k] = s;
        psd[(size_t)b * kIfxL + k] = s;
    }
    __syncthreads();
    // bitonic sort, ascending: 1024 compare-exchanges per stage, four per thread
    for (int k = 2; k <= kIfxL; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int p = t + 256 * q;
                const int i = 2 * j * (p / j) + (p % j), l = i + j;
                const bool up = (i & k) == 0;
                const float a = srt[i], c = srt[l];
                if ((a > c) == up) { srt[i] = c; srt[l] = a; }
            }
            __syncthreads();
        }
    }
    const float thr = 0.5f * (srt[kIfxL / 2 - 1] + srt[kIfxL / 2]) * scale;
#pragma unroll
    for (int q = 0; q < 8; ++q) flag[t + 256 * q] = P[t + 256 * q] > thr ? 1 : 0;
    __syncthreads();
    const int lane = t & 63, wave = t >> 6;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int k = t + 256 * q;
        int f = 0;
        for (int d = -dilate; d <= dilate; ++d) f |= flag[(k + d) & (kIfxL - 1)];
        const unsigned long long bal = __ballot(f);       // bins 256 q + 64 wave + lane
        if (lane == 0) {
            const int w0 = (256 * q + 64 * wave) / 32;
            words[w0] = (uint32_t)bal;
            words[w0 + 1] = (uint32_t)(bal >> 32);
        }
    }
    __syncthreads();
    int count = 0;
    for (int w = 0; w < kMaskWords; ++w) count += __popc(words[w]);   // (every thread, same value)
    const bool wide = count > max_bins;
    if (t < kMaskWords) masks[(size_t)b * kMaskWords + t] = wide ? 0u : words[t];
    if (t == 0) counts[b] = wide ? -1 : count;
}

// grid: nb * runs workgroups, run = S consecutive segments of one block
template <int FMT>
__global__ __launch_bounds__(256) void ifx_apply_kernel(const void* __restrict__ iq,
                                                        const float2* __restrict__ carry,
                                                        const float* __restrict__ win, int n, int runs,
                                                        int S, const int32_t* __restrict__ counts,
                                                        const uint32_t* __restrict__ masks,
                                                        float2* __restrict__ out,
                                                        const float2* __restrict__ tw) {
    __shared__ __attribute__((aligned(16))) float lds[kFftLdsFloats];
    __shared__ __attribute__((aligned(16))) float lds_tw[kFftTwFloats];
    const int t = threadIdx.x;
    const int b = blockIdx.x / runs, run = blockIdx.x % runs;
    const int nf = n / kIfxH;
    const int s0 = run * S, s1 = min(s0 + S, nf);            // segments [s0, s1)
    float2* o = out + (size_t)b * n;
    if (counts[b] < 0) {                                      // wideband: the block passes through
        for (int i = s0 * kIfxH + t; i < s1 * kIfxH; i += 256) o[i] = load_iq<FMT>(iq, (size_t)b * n + i);
        return;
    }
    const FftTw ftw = fft_setup(lds_tw, tw, t);
    float w[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) w[r] = win[t + 256 * r];
    unsigned keep = 0;                                        // bit q: bin t + 256 q survives
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int k = t + 256 * q;
        keep |= ((masks[(size_t)b * kMaskWords + (k >> 5)] >> (k & 31)) & 1u) ? 0u : (1u << q);
    }
    const float sc = 1.0f / (float)kIfxL;
    __syncthreads();
    float2 prev[4];
    const int f_end = min(s1, nf - 1);                        // last frame transformed
    for (int f = s0; f <= f_end; ++f) {
        const bool last = f == nf - 1;
        float2 v[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const float2 x = ifx_load<FMT>(iq, carry, b, n, f * kIfxH - kIfxH + t + 256 * r);
            const float wr = (last && r >= 4) ? 1.0f : w[r];
            v[r] = make_float2(x.x * wr, x.y * wr);
        }
        fft2048(v, lds, ftw, t);
#pragma unroll
        for (int q = 0; q < 8; ++q)          // zero the masked bins, conjugate for the inverse
            v[q] = ((keep >> q) & 1u) ? make_float2(v[q].x, -v[q].y) : make_float2(0.f, 0.f);
        lds_barrier();
        fft2048(v, lds, ftw, t);
        lds_barrier();
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = make_float2(v[r].x * sc, -v[r].y * sc);
        if (f > s0) {                                         // segment f - 1 is complete
            float2* d = o + (size_t)(f - 1) * kIfxH;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                d[t + 256 * r] = make_float2(prev[r].x + v[r].x, prev[r].y + v[r].y);
        }
        if (last && f < s1) {                                 // the last segment: frame nf - 1 alone
            float2* d = o + (size_t)f * kIfxH;
#pragma unroll
            for (int r = 0; r < 4; ++r) d[t + 256 * r] = v[r + 4];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) prev[r] = v[r + 4];
    }
}

template <int FMT>
__global__ __launch_bounds__(256) void ifx_carry_kernel(const void* __restrict__ iq, size_t tail,
                                                        float2* __restrict__ carry) {
    for (int i = threadIdx.x; i < kIfxH; i += 256) carry[i] = load_iq<FMT>(iq, tail + i);
}

}  // namespace gpsmi

using namespace gpsmi;

struct gpsmi_ifx {
    gpsmi_ifx_cfg cfg;
    DevBuf<float2> d_tw;
    DevBuf<float> d_win;                     // periodic Hann, float32 of the double value
    DevBuf<float2> d_carry;                  // [H] complex64
    DevBuf<float> d_partial;                 // [nb][groups][2048]
    DevBuf<int32_t> d_counts;                // [nb]
    DevBuf<uint32_t> d_masks;                // [nb][kMaskWords]
    DevBuf<float> d_psd;                     // [nb][2048]: the P the mask pass thresholded
    int last_nb = 0;                         // blocks of the last call (0: none yet)
    float scale = 0.f;                       // 10^(thresh_db / 10) as float32
    BlockStage blk;
    StageSync sync;                          // last: see gpsmi_stage.h
};

static bool ifx_block_ok(int32_t n) { return n >= 4 * kIfxH && n <= (1 << 24) && n % kIfxH == 0; }

static int ifx_build(gpsmi_ifx* h) {
    h->blk.block_samples = h->cfg.block_samples;
    std::vector<float2> tw;
    make_twiddles(tw);
    int rc;
    if ((rc = h->d_tw.upload(tw, "excision twiddles"))) return rc;
    std::vector<float> win(kIfxL);
    for (int i = 0; i < kIfxL; ++i) {
        const double s = sin(M_PI * (double)i / (double)kIfxL);
        win[i] = (float)(s * s);
    }
    if ((rc = h->d_win.upload(win, "excision window")) || (rc = h->d_carry.reserve_zeroed(kIfxH, "excision carry")))
        return rc;
    h->scale = (float)pow(10.0, (double)h->cfg.thresh_db / 10.0);
    return GPSMI_OK;
}

// Runs the four passes over nb blocks at d_iq (device, the handle's input format) into d_out.
static int ifx_run(gpsmi_ifx* h, const void* d_iq, void* d_out, int nb) {
    const int n = h->cfg.block_samples, nf = n / kIfxH;
    const int groups = (nf - 1 + kPsdGroup - 1) / kPsdGroup;
    int rc = h->d_partial.reserve((size_t)nb * groups * kIfxL, "excision spectra");
    if (!rc) rc = h->d_counts.reserve(nb, "excision results");
    if (!rc) rc = h->d_masks.reserve((size_t)nb * kMaskWords, "excision results");
    if (!rc) rc = h->d_psd.reserve((size_t)nb * kIfxL, "excision results");
    if (rc) return rc;
    const hipStream_t st = h->sync.stream;
    // segments per apply workgroup: one frame transform pair per segment plus one per workgroup;
    // runs of up to 8 segments once the grid has some 2048 workgroups anyway (same bits either way)
    const long long segs = (long long)nb * nf;
    const int S = segs >= 16384 ? 8 : segs >= 8192 ? 4 : segs >= 4096 ? 2 : 1;
    const int runs = (nf + S - 1) / S;
    const size_t tail = (size_t)nb * n - kIfxH;
    if ((rc = h->sync.begin())) return rc;
    with_fmt(h->blk.fmt, [&](auto fmt) {
        constexpr int FMT = decltype(fmt)::value;
        hipLaunchKernelGGL(ifx_psd_kernel<FMT>, dim3((unsigned)(nb * groups)), dim3(256), 0, st, d_iq,
                           h->d_carry.p, h->d_win.p, n, groups, h->d_partial.p, h->d_tw.p);
        hipLaunchKernelGGL(ifx_mask_kernel, dim3((unsigned)nb), dim3(256), 0, st, h->d_partial.p, groups,
                           nf - 1, h->scale, h->cfg.dilate, h->cfg.max_bins, h->d_counts.p, h->d_masks.p,
                           h->d_psd.p);
        hipLaunchKernelGGL(ifx_apply_kernel<FMT>, dim3((unsigned)(nb * runs)), dim3(256), 0, st, d_iq,
                           h->d_carry.p, h->d_win.p, n, runs, S, h->d_counts.p, h->d_masks.p, (float2*)d_out,
                           h->d_tw.p);
        hipLaunchKernelGGL(ifx_carry_kernel<FMT>, dim3(1), dim3(256), 0, st, d_iq, tail, h->d_carry.p);
    });
    if (!(rc = h->sync.end())) h->last_nb = nb;
    return rc;
}

static int ifx_finish(gpsmi_ifx* h, int nb, int32_t* counts, uint32_t* masks) {
    const hipStream_t st = h->sync.stream;
    if (counts)
        GPSMI_HIP(hipMemcpyAsync(counts, h->d_counts.p, (size_t)nb * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (masks)
        GPSMI_HIP(hipMemcpyAsync(masks, h->d_masks.p, (size_t)nb * kMaskWords * sizeof(uint32_t),
                                 hipMemcpyDeviceToHost, st));
    return h->sync.finish();
}

extern "C" {

int gpsmi_ifx_create(const gpsmi_ifx_cfg* cfg, gpsmi_ifx** out) {
    GPSMI_REQUIRE(cfg && out, "null argument");
    *out = nullptr;
    GPSMI_REQUIRE(!std::isnan(cfg->thresh_db), "thresh_db is NaN");
    GPSMI_REQUIRE(cfg->dilate >= 0 && cfg->dilate <= 64, "dilate out of range 0..64");
    GPSMI_REQUIRE(cfg->max_bins >= 0 && cfg->max_bins <= kIfxL, "max_bins out of range 0..2048");
    if (!ifx_block_ok(cfg->block_samples))
        return fail(GPSMI_E_UNSUPPORTED,
                    "gpsmi_ifx_create: block_samples %d is not a multiple of 1024 in 4096..2^24",
                    (int)cfg->block_samples);
    return stage_create(cfg, out, ifx_build);
}

int gpsmi_ifx_destroy(gpsmi_ifx* h) { return stage_destroy(h); }

int gpsmi_ifx_set_input_format(gpsmi_ifx* h, int fmt) { return stage_set_input_format(h, fmt, __func__); }

int gpsmi_ifx_reset(gpsmi_ifx* h) {
    GPSMI_REQUIRE(h, "null handle");
    GPSMI_HIP(hipSetDevice(h->cfg.device));
    GPSMI_HIP(hipMemsetAsync(h->d_carry.p, 0, kIfxH * sizeof(float2), h->sync.stream));
    GPSMI_HIP(hipStreamSynchronize(h->sync.stream));
    return GPSMI_OK;
}

int gpsmi_ifx_apply_dev(gpsmi_ifx* h, const void* d_iq, void* d_out, int nb, int32_t* counts,
                        uint32_t* masks) {
    int rc = stage_check_call(h, d_iq, d_out, nb, __func__, "excision", false);
    if (rc) return rc;
    GPSMI_HIP(hipSetDevice(h->cfg.device));
    rc = ifx_run(h, d_iq, d_out, nb);
    if (rc) return rc;
    return ifx_finish(h, nb, counts, masks);
}

int gpsmi_ifx_apply(gpsmi_ifx* h, const void* iq, float* out, int nb, int32_t* counts, uint32_t* masks) {
    int rc = stage_check_call(h, iq, out, nb, __func__, nullptr, false);   // (host buffers: overlap not checked)
    if (rc) return rc;
    GPSMI_HIP(hipSetDevice(h->cfg.device));
    return h->blk.apply_host(
        iq, out, nb, h->blk.out_bytes(nb), h->sync.stream, "excision staging",
        [&](const void* d_iq, void* d_out) { return ifx_run(h, d_iq, d_out, nb); },
        [&] { return ifx_finish(h, nb, counts, masks); });
}

int gpsmi_ifx_last_ms(gpsmi_ifx* h, float* ms) { return stage_last_ms(h, ms, __func__); }

int gpsmi_ifx_last_psd(gpsmi_ifx* h, float* psd) {
    GPSMI_REQUIRE(h && psd, "null argument");
    if (h->last_nb <= 0) return fail(GPSMI_E_STATE, "gpsmi_ifx_last_psd: no call yet");
    GPSMI_HIP(hipSetDevice(h->cfg.device));
    GPSMI_HIP(hipMemcpyAsync(psd, h->d_psd.p, (size_t)h->last_nb * kIfxL * sizeof(float), hipMemcpyDeviceToHost,
                             h->sync.stream));
    GPSMI_HIP(hipStreamSynchronize(h->sync.stream));
    return GPSMI_OK;
}

}  // extern "C"
