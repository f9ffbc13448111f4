// findCodePhase statistics (reference src/gpsrecv.py:222-238, src/gpslib.py:1293-1304)
// of a 2048-lag correlation held 8 magnitudes per thread by a 256-thread workgroup:
// mean, population standard deviation, first-index argmax and the two circular
// neighbours of the peak.  Wave reductions use DPP (row-local steps plus the two
// row broadcasts), not ds_bpermute; two workgroup barriers per call.
//
// The magnitudes are square roots times a positive factor: never negative, never -0.  The
// order of two such floats is the order of their bit patterns as integers, and the maximum
// and its first lag are found on the bit patterns (v_max_i32 takes a DPP operand directly;
// fmaxf asks for a canonicalising copy of every partner).  The sums are float additions in a
// fixed order: per thread in ascending q from 0, the DPP tree in the order of wave_sum_dpp,
// (w0 + w1) + (w2 + w3) across the waves, the deviations from the mean formed first.
// NaN magnitudes (NaN or Inf in the IQ) are outside the contract.  What happens to them: a NaN
// of positive sign has a larger bit pattern than every number, so it is reported as the peak, at
// the first lag that holds exactly those bits; mean and standard deviation come out NaN as before.
#pragma once
#include <hip/hip_runtime.h>

#include "gpsmi_fft.h"

namespace gpsmi {

template <int CTRL, int ROWS>
__device__ __forceinline__ float dpp_add0(float v) {      // v + partner, 0 where no partner
    const float o = __builtin_bit_cast(
        float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROWS, 0xF, false));
    return v + o;
}
// sum over the 64 lanes, in lane 63 only.  The two row broadcasts run over all four rows like the
// row-local steps (lanes without a partner add 0), so that every step is one v_add_f32 with a DPP
// operand; lane 63 is ((r3 + r2) + (r1 + r0)) of the four row sums, as it is with the broadcasts
// masked to rows 1, 3 and 2, 3: it reads lane 47 before the first broadcast reaches it and
// lane 31 after.
__device__ __forceinline__ float wave_sum_dpp_l63(float v) {
    v = dpp_add0<0xB1, 0xF>(v);        // quad_perm [1,0,3,2]
    v = dpp_add0<0x4E, 0xF>(v);        // quad_perm [2,3,0,1]
    v = dpp_add0<0x141, 0xF>(v);       // row_half_mirror: 8 lanes
    v = dpp_add0<0x140, 0xF>(v);       // row_mirror: 16 lanes
    v = dpp_add0<0x142, 0xF>(v);       // row_bcast15: lane 15 of a row into the next row
    v = dpp_add0<0x143, 0xF>(v);       // row_bcast31: lane 31 into rows 2 and 3
    asm volatile("" : "+v"(v));        // (the last addition stays with its DPP operand: not sunk into lane 63's branch)
    return v;
}
// the same sum, broadcast to all lanes
__device__ __forceinline__ float wave_sum_dpp(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, wave_sum_dpp_l63(v)), 63));
}

// v + partner for a double, the partner's halves fetched by two DPP moves
template <int CTRL>
__device__ __forceinline__ double dpp_add_f64(double v) {
    const long long b = __builtin_bit_cast(long long, v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(b & 0xffffffffll), CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, 0xF, 0xF, false);
    return v + __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned)lo);
}
// sum over the 16 lanes of a DPP row, in every lane of the row (the adds commute: the partners of a
// step hold the same bits)
__device__ __forceinline__ double row_sum_f64_dpp(double v) {
    v = dpp_add_f64<0xB1>(v);          // quad_perm [1,0,3,2]
    v = dpp_add_f64<0x4E>(v);          // quad_perm [2,3,0,1]
    v = dpp_add_f64<0x141>(v);         // row_half_mirror
    v = dpp_add_f64<0x140>(v);         // row_mirror
    return v;
}

template <int CTRL, int ROWS>
__device__ __forceinline__ float dpp_max_own(float v) {   // max(v, partner), v where no partner
    const int vi = __builtin_bit_cast(int, v);
    return fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(vi, vi, CTRL, ROWS, 0xF, false)));
}
template <int CTRL, int ROWS>
__device__ __forceinline__ int dpp_min_own(int v) {
    return min(v, __builtin_amdgcn_update_dpp(v, v, CTRL, ROWS, 0xF, false));
}
// maximum and its smallest index over the 64 lanes, broadcast to all of them: the maximum
// first, then the smallest index among the lanes that hold it (12 DPP steps, no branches)
__device__ __forceinline__ void wave_argmax_dpp(float& v, int& i) {
    float m = v;
    m = dpp_max_own<0xB1, 0xF>(m);
    m = dpp_max_own<0x4E, 0xF>(m);
    m = dpp_max_own<0x141, 0xF>(m);
    m = dpp_max_own<0x140, 0xF>(m);
    m = dpp_max_own<0x142, 0xA>(m);
    m = dpp_max_own<0x143, 0xC>(m);
    m = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, m), 63));
    int k = v == m ? i : 0x7fffffff;
    k = dpp_min_own<0xB1, 0xF>(k);
    k = dpp_min_own<0x4E, 0xF>(k);
    k = dpp_min_own<0x141, 0xF>(k);
    k = dpp_min_own<0x140, 0xF>(k);
    k = dpp_min_own<0x142, 0xA>(k);
    k = dpp_min_own<0x143, 0xC>(k);
    v = m;
    i = __builtin_amdgcn_readlane(k, 63);
}

template <int CTRL>
__device__ __forceinline__ int dpp_max0(int v) {           // max(v, partner) of v >= 0; 0 where no partner
    return max(v, __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, false));
}
// maximum of non-negative integers (the bit patterns of non-negative floats) over the 64 lanes,
// in lane 63 only: one v_max_i32 with a DPP operand per step
__device__ __forceinline__ int wave_max_nn_dpp_l63(int v) {
    v = dpp_max0<0xB1>(v);
    v = dpp_max0<0x4E>(v);
    v = dpp_max0<0x141>(v);
    v = dpp_max0<0x140>(v);
    v = dpp_max0<0x142>(v);
    v = dpp_max0<0x143>(v);
    asm volatile("" : "+v"(v));
    return v;
}

// LDS of the statistics, 16-byte aligned: [0..3] the waves' sums, [4..11] the waves' peaks as
// 64-bit keys, [12..15] the waves' sums of squared deviations
constexpr int kStatsRedFloats = 16;

// a thread's share of the sum: its eight magnitudes in ascending q, from 0
__device__ __forceinline__ float stats_sum8(const float* mag) {
    float sm = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) sm += mag[q];
    return sm;
}

// mag[q] = correlation magnitude at lag t + 256 q, not negative; sm = the thread's share of their
// sum (stats_sum8, or the caller's own where it forms the magnitudes and the sum in one).  magbuf:
// 2048 floats of LDS of its own (not the FFT buffers), red: kStatsRedFloats floats, 16-byte
// aligned.  Every thread returns the same values.  Safe to call again after any later workgroup
// barrier.
//
// A wave first finds its maximum as a value alone; the lag follows from it in scalar code: lag
// t + 256 q grows with q first and with the lane second, so the first lag is the lowest set bit of
// the lowest q whose lanes hold the maximum at all.  Lane 63, where the DPP trees end, parks sum
// and peak; the peak as the key (value bits << 32 | ~lag), so that the larger key is the larger value
// and, between equal values, the smaller lag.  Between the barriers the deviations are summed and
// the four keys compared, without a branch.  The neighbours of the peak are read back from the
// copy in magbuf (handing them over from the two threads that hold them, a wave-uniform select
// of one register in eight, would save the 8 KiB of stores; it measured 0.5 % slower per step:
// DESIGN.md section 4.4).
__device__ __forceinline__ void corr_stats8(const float* mag, float sm, int t, float* magbuf, float* red,
                                            int& amax, float& peak, float& mean, float& sd,
                                            float& lo, float& hi) {
    constexpr int N = 2048;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
    int bits[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        bits[q] = __builtin_bit_cast(int, mag[q]);
        magbuf[t + 256 * q] = mag[q];
    }
    int mx = max(max(bits[0], bits[1]), bits[2]);
    mx = max(max(mx, bits[3]), bits[4]);
    mx = max(max(mx, bits[5]), bits[6]);
    mx = max(mx, bits[7]);
    sm = wave_sum_dpp_l63(sm);
    mx = wave_max_nn_dpp_l63(mx);
    const int wmax = __builtin_amdgcn_readlane(mx, 63);
    int first = 0;
#pragma unroll
    for (int q = 7; q >= 0; --q) {                              // descending: the lowest q stays
        const unsigned long long has = __builtin_amdgcn_ballot_w64(bits[q] == wmax);
        if (has) first = __builtin_ctzll(has) + 256 * q;
    }
    first += 64 * wave;
    if (lane == 63) {
        red[wave] = sm;
        ((int*)red)[4 + 2 * wave] = ~first;
        ((int*)red)[5 + 2 * wave] = mx;
    }
    lds_barrier();
    const float4 ws = *reinterpret_cast<const float4*>(red);
    mean = ((ws.x + ws.y) + (ws.z + ws.w)) * (1.0f / N);
    float d2 = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) { const float d = mag[q] - mean; d2 += d * d; }
    d2 = wave_sum_dpp_l63(d2);
    if (lane == 63) red[12 + wave] = d2;
    // (nothing below has to be done before the barrier: the keys are read with the sums)
    using u64 = unsigned long long;
    const ulonglong2 k01 = *reinterpret_cast<const ulonglong2*>(red + 4);
    const ulonglong2 k23 = *reinterpret_cast<const ulonglong2*>(red + 8);
    const u64 ka = k01.x > k01.y ? k01.x : k01.y, kb = k23.x > k23.y ? k23.x : k23.y;
    const u64 key = ka > kb ? ka : kb;
    const int bi = ~(int)(unsigned)key;
    lds_barrier();
    const float4 wd = *reinterpret_cast<const float4*>(red + 12);
    sd = sqrtf(((wd.x + wd.y) + (wd.z + wd.w)) * (1.0f / N));
    amax = bi;
    peak = __builtin_bit_cast(float, (int)(key >> 32));
    lo = magbuf[(bi + N - 1) & (N - 1)];
    hi = magbuf[(bi + 1) & (N - 1)];
}

}  // namespace gpsmi
