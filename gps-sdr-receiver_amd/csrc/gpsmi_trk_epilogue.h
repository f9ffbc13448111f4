// The tracking epilogue: the per-job part of a block behind the correlator -- window means,
// edge scan of decodeData, amplitude statistics, phaseLockedLoop, state update -- and its four
// kernels.  Included by gpsmi_trk.hip with floating-point contraction OFF: this code restates the
// reference's float32 arithmetic step by step.
//
// Two lane layouts share one copy of the per-job arithmetic (epi_*): a wave per job, lane = prompt
// dump (epilogue_job: trk_epilogue_kernel, trk_epilogue_span_kernel, trk_epilogue_span8_kernel) and
// eight lanes per job, lane j = dumps j, j + 8, ... (trk_epilogue8_kernel).  What differs between
// them -- where a dump lives, how its neighbour is fetched, how the unwrap count is formed, LDS
// arrays against registers -- stays in the two forms.
#pragma once
namespace gpsmi {

// np.mean of a float32 array of n <= 128 elements: numpy's pairwise kernel
// (eight strided accumulators, tree-combined, tail added in order).
__device__ inline float np_sum_f32(const float* a, int n) {
    if (n < 8) {
        float r = 0.f;
        for (int i = 0; i < n; ++i) r = add_rn(r, a[i]);
        return r;
    }
    float r[8];
    for (int j = 0; j < 8; ++j) r[j] = a[j];
    int i = 8;
    for (; i < n - (n % 8); i += 8)
        for (int j = 0; j < 8; ++j) r[j] = add_rn(r[j], a[i + j]);
    float res = add_rn(add_rn(add_rn(r[0], r[1]), add_rn(r[2], r[3])),
                          add_rn(add_rn(r[4], r[5]), add_rn(r[6], r[7])));
    for (; i < n; ++i) res = add_rn(res, a[i]);
    return res;
}

// The tree ((r0+r1)+(r2+r3)) + ((r4+r5)+(r6+r7)) over numpy's eight strided accumulators, one per
// lane of a group of eight, in every lane of the group: three DPP steps (the adds commute, so the
// partners of a step hold the same bits).
constexpr int kQuadSwap1 = 0xB1, kQuadSwap2 = 0x4E, kHalfMirror = 0x141;
__device__ __forceinline__ float tree8(float r) {
    r = dpp_add0<kQuadSwap1, 0xF>(r);    // quad_perm [1,0,3,2]: r0+r1 | r2+r3 | r4+r5 | r6+r7
    r = dpp_add0<kQuadSwap2, 0xF>(r);    // quad_perm [2,3,0,1]: (r0+r1)+(r2+r3) | (r4+r5)+(r6+r7)
    r = dpp_add0<kHalfMirror, 0xF>(r);   // row_half_mirror: lane j with lane 7 - j
    return r;
}
// The same sum by a group of eight lanes, every lane of it returning it: lane j carries accumulator j
// (n / 8 - 1 dependent adds instead of n), the tail is added in order.  a: LDS, n <= 128.
__device__ __forceinline__ float np_sum_f32_grp(const float* a, int n, int j) {
    if (n < 8) return np_sum_f32(a, n);
    const int body = n - (n % 8);
    float r = a[j];
    for (int i = 8; i < body; i += 8) r = add_rn(r, a[i + j]);
    r = tree8(r);
    for (int i = body; i < n; ++i) r = add_rn(r, a[i]);
    return r;
}
// ... by one wave, every lane returning it (the first group's, as a scalar)
__device__ __forceinline__ float np_sum_f32_wave(const float* a, int n, int lane) {
    if (n < 8) return np_sum_f32(a, n);
    const float r = np_sum_f32_grp(a, n, lane & 7);
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, r)));
}

// ---- The per-job arithmetic both lane layouts share.  A job's lanes all call these with the same
// scalars; `j` of `nl` is the lane's index within its job (nl = 64: a wave, 8: a group of eight).

// the scalars of a job's state row (the same address in every lane of the job: one broadcast load each)
struct EpiState {
    int nps, df_len, was_locked, edge_state0;
    float freq0, phase0, omega0, prev_r, prev_i, prev_signal0, std_dev0;
};
__device__ __forceinline__ EpiState epi_load(const gpsmi_trk_state& si) {
    EpiState s;
    s.nps = si.nps; s.df_len = si.df_len; s.was_locked = si.phase_locked;
    s.freq0 = si.freq; s.phase0 = si.phase; s.omega0 = si.omega0;
    s.prev_r = si.prev_sum_re; s.prev_i = si.prev_sum_im;
    s.edge_state0 = si.edge_state;
    s.prev_signal0 = si.prev_signal; s.std_dev0 = si.std_dev;
    return s;
}

// what a job computes besides its dumps: everything epi_store writes
struct EpiResult {
    int n1, nd, nps_new = 0;                       // windows: first length, dumps, carry
    float car_r = 0.f, car_i = 0.f;
    unsigned long long edge_mask = 0;              // edge scan (unchanged state while not locked)
    int edge_sign0 = 0, edge_state, ms_count = 0;
    float prev_signal;
    float mmean, sdev;                             // amplitude statistics
    float offset, df;                              // PLL
    int new_len, locked;
    float freq, phase, om_new;                     // carrier
};

// windows of decodeData (gpslib.py:1403-1420, :1440): S[0] head, S[q+1] window q, S[nc] tail.  With
// neither carry nor delay the rows are the windows; at delay 0 behind a carry the last code period is
// complete (nc + 1 dumps); any other delay leaves the tail as the carry into the next block.
__device__ __forceinline__ void epi_windows(const float2* S, int nc, int cs, int d, const EpiState& s,
                                            EpiResult& R) {
    R.n1 = s.nps + d;
    R.nd = (R.n1 != 0 && d == 0) ? nc + 1 : nc;
    R.edge_state = s.edge_state0;                  // (the edge words stay while not locked)
    R.prev_signal = s.prev_signal0;
    if (d != 0) { R.car_r = S[nc].x; R.car_i = S[nc].y; R.nps_new = cs - d; }   // (n1 = 0 only at delay 0)
}
// prompt dump i of these windows (0 past the last)
__device__ __forceinline__ void epi_dump(const float2* S, int i, int cs, const EpiState& s, const EpiResult& R,
                                         float& gr, float& gi) {
    gr = gi = 0.f;
    if (R.n1 == 0) {
        if (i < R.nd) { gr = S[i + 1].x / (float)cs; gi = S[i + 1].y / (float)cs; }
    } else if (i == 0) {
        gr = (s.prev_r + S[0].x) / (float)R.n1;
        gi = (s.prev_i + S[0].y) / (float)R.n1;
    } else if (i < R.nd) {
        gr = S[i].x / (float)cs;
        gi = S[i].y / (float)cs;
    }
}

// Edge scan of decodeData (gpslib.py:1394-1398, :1421-1436): while PHASE_LOCKED (the flag before this
// block's PLL), a dump is an edge when its sign differs from prevSign, the dump before it carried
// prevSign's sign (prevSign * PREV_SIGNAL > 0) and the step between the two exceeds MIN_EDGE_AMP =
// 3 * STD_DEV (of the block before).  prevSign only changes at an edge, so the scan jumps from edge to
// edge over three per-job bit masks of the nd dumps (scalar arithmetic, the same in every lane of the
// job): Pm / Nm = dump positive / negative, Bm = step to the dump before large enough.
// edge_state 2 (an edge onto a dump whose real part is exactly 0) stays 0 = "no prevSign" until
// erasePrevData, where the reference re-derives prevSign in every call: to be changed here alone.
__device__ __forceinline__ void epi_edge_scan(unsigned long long Pm, unsigned long long Nm, unsigned long long Bm,
                                              int nd, float prev_signal0, int edge_state0,
                                              unsigned long long& edge_mask, int& edge_sign0, int& edge_state) {
    const unsigned long long V = (1ull << nd) - 1;                 // nd <= 33
    const unsigned long long Pp = (Pm << 1) | (prev_signal0 > 0.f ? 1ull : 0ull);   // the dump before
    const unsigned long long Np = (Nm << 1) | (prev_signal0 < 0.f ? 1ull : 0ull);
    unsigned long long todo = V;
    int p = edge_state0 == 2 ? 0 : edge_state0;
    if (edge_state0 == 0) {            // EDGES[0] == 0: every dump stores its sign until one is non-zero
        const unsigned long long nz = Pm | Nm;
        if (nz == 0) {
            todo = 0;
        } else {
            const int q = __builtin_ctzll(nz);
            p = ((Pm >> q) & 1) ? 1 : -1;
            edge_sign0 = p;
            todo = V & ~((2ull << q) - 1);
        }
    }
    while (p != 0 && todo != 0) {
        const unsigned long long cand = (p > 0 ? (Pp & ~Pm) : (Np & ~Nm)) & Bm & todo;
        if (cand == 0) break;
        const int i = __builtin_ctzll(cand);
        edge_mask |= 1ull << i;
        p = ((Pm >> i) & 1) ? 1 : (((Nm >> i) & 1) ? -1 : 0);
        todo &= ~((2ull << i) - 1);
    }
    if (edge_state0 != 0 || edge_sign0 != 0) edge_state = p == 0 ? 2 : p;
}

// Loop filter of phaseLockedLoop (gpslib.py:1215-1262) on the mean unwrapped phase `pdev`; mean_df:
// the mean of the drift list s_df (LDS, df_len entries; only read when locked).  Writes the new list.
__device__ __forceinline__ void epi_loop_filter(float pdev, float mean_df, int df_len, int was_locked,
                                                const TrkParams& P, const float* s_df, gpsmi_trk_state& so,
                                                int j, int nl, float& df, int& new_len, int& locked) {
    const float max_df = 20.0f / (float)P.df_no;
    locked = was_locked;
    if (locked) {
        df = add_rn(pdev, mean_df);                 // DF_GAIN2 = 1
        if (fabsf(df) > max_df) df = (df > 0.f ? 1.f : -1.f) * max_df;
        const int shift = df_len >= P.df_no ? 1 : 0;   // drop the oldest entry
        new_len = df_len - shift + 1;
        for (int i = j; i < new_len - 1; i += nl) so.df[i] = s_df[i + shift];
        if (j == 0) so.df[new_len - 1] = df;
    } else {
        df = mul_rn(10.0f, pdev);                   // DF_GAIN1 = 10
        new_len = 1;
        if (j == 0) so.df[0] = df;
    }
    if (fabsf(pdev) < 0.1f) locked = 1;
}

// Carrier of the next block (gpslib.py:1178 via :1345-1346, then :1205-1208)
__device__ __forceinline__ void epi_carrier(float freq0, float phase0, float omega0, float offset, float df,
                                            const TrkParams& P, float& freq, float& phase, float& om_new) {
    const float om = omega0 != 0.f ? omega0 : omega_of(freq0);
    phase = add_rn(phase0, mul_rn(om, P.t_last));
    float mod = fmodf(phase, kTwoPiF);                 // np.remainder(phase, 2*pi)
    if (mod != 0.f && mod < 0.f) mod = add_rn(mod, kTwoPiF);
    phase = add_rn(mod, offset);
    freq = add_rn(freq0, df);
    om_new = 0.f;                                      // FREQ is float32 from here on ...
    if (freq > P.max_freq) { freq = P.max_freq; om_new = P.om_max; }   // ... unless clamped to
    else if (freq < P.min_freq) { freq = P.min_freq; om_new = P.om_min; }  // a Python float
}

// the next state row and the record, but for the dumps and the drift list (one lane of the job)
__device__ __forceinline__ void epi_store(const gpsmi_trk_state& si, gpsmi_trk_state& so, gpsmi_trk_out& o,
                                          int d, int cs, const EpiResult& R) {
    so.prn = si.prn;
    so.delay = d;
    so.freq = R.freq;
    so.phase = R.phase;
    so.phase_locked = R.locked;
    so.nps = R.nps_new;
    so.prev_sum_re = R.car_r;
    so.prev_sum_im = R.car_i;
    so.df_len = R.new_len;
    so.omega0 = R.om_new;
    so.edge_state = R.edge_state;
    so.prev_signal = R.prev_signal;
    so.std_dev = R.sdev;
    so.reserved = 0;
    o.n_dumps = R.nd;
    o.first_len = (R.n1 == 0) ? cs : R.n1;
    o.std_dev = R.sdev;
    o.amplitude = R.mmean / R.sdev;
    o.df = R.df;
    o.phase_shift = R.offset;
    o.freq = R.freq;
    o.phase = R.phase;
    o.phase_locked = R.locked;
    o.nps = R.nps_new;
    o.edge_mask = (uint32_t)R.edge_mask;
    o.edge_mask_hi = (uint32_t)(R.edge_mask >> 32);
    o.edge_sign0 = R.edge_sign0;
    o.ms_count = R.ms_count;
    o.reserved1 = 0;
}

// The per-job part of a block behind the correlator, one wave, lane i = prompt dump i.
// Element-wise work (windows, |g|, atan, phase unwrapping by a lane prefix sum) is spread
// over the lanes; the few float32 sums are evaluated redundantly by every lane over small
// LDS arrays in numpy's own order (np_sum_f32), so the result does not depend on how lanes
// are scheduled.  S[0] head, S[q+1] window q, S[nc] tail (global memory or LDS).
__device__ __forceinline__ void epilogue_job(const gpsmi_trk_state& si, gpsmi_trk_state& so, int d,
                                             const float2* S, const TrkParams& P, gpsmi_trk_out& o,
                                             int lane, float* s_mag_w, float* s_dev_w, float* s_real_w,
                                             float* s_df_w) {
    const int cs = P.cs;
    const EpiState s = epi_load(si);
    for (int i = lane; i < s.df_len; i += 64) s_df_w[i] = si.df[i];

    // ---- prompt dumps
    EpiResult R;
    epi_windows(S, P.n_cyc, cs, d, s, R);
    const int nd = R.nd;
    float gr, gi;
    epi_dump(S, lane, cs, s, R, gr, gi);
    if (lane < GPSMI_MAX_DUMPS) {
        o.dumps[2 * lane] = gr;
        o.dumps[2 * lane + 1] = gi;
    }

    // ---- edge scan: the masks by ballot, the dump before from the lane below
    if (s.was_locked) {
        const unsigned long long V = (1ull << nd) - 1;
        const float thr = mul_rn(3.0f, s.std_dev0);
        const float re_up = __shfl_up(gr, 1, 64);
        const float re_prev = lane == 0 ? s.prev_signal0 : re_up;
        const unsigned long long Pm = __ballot(gr > 0.f) & V, Nm = __ballot(gr < 0.f) & V;
        const unsigned long long Bm = __ballot(fabsf(sub_rn(gr, re_prev)) > thr) & V;
        epi_edge_scan(Pm, Nm, Bm, nd, s.prev_signal0, s.edge_state0, R.edge_mask, R.edge_sign0, R.edge_state);
        R.prev_signal = __shfl(gr, nd - 1, 64);                    // PREV_SIGNAL = m.real of the last dump
        R.ms_count = nd;
    }

    // ---- amplitude statistics (gpslib.py:1186-1187), float32 like numpy
    const float mag = hypotf(gr, gi);
    if (lane < nd) s_mag_w[lane] = mag;
    __builtin_amdgcn_wave_barrier();
    R.mmean = np_sum_f32_wave(s_mag_w, nd, lane) / (float)nd;
    {
        const float e = sub_rn(mag, R.mmean);
        if (lane < nd) s_dev_w[lane] = mul_rn(e, e);
    }
    __builtin_amdgcn_wave_barrier();
    R.sdev = sqrtf(np_sum_f32_wave(s_dev_w, nd, lane) / (float)nd);

    // ---- phaseLockedLoop (gpslib.py:1215-1262): unwrap by a lane prefix sum
    const float ph = atanf(gi / gr);
    const float ph_prev = __shfl_up(ph, 1, 64);
    float jump = 0.f;
    if (lane >= 1 && lane < nd) {
        const float delta = sub_rn(ph, ph_prev);
        if (fabsf(delta) > 2.0f) jump = (delta > 0.f) ? -1.f : 1.f;
    }
#pragma unroll
    for (int o2 = 1; o2 < 64; o2 <<= 1) {            // inclusive scan (small integers: exact)
        const float v = __shfl_up(jump, o2, 64);
        if (lane >= o2) jump += v;
    }
    const float real = (lane == 0) ? ph : add_rn(ph, mul_rn(jump, kPiF));
    if (lane < nd) s_real_w[lane] = real;
    __builtin_amdgcn_wave_barrier();
    R.offset = np_sum_f32(s_real_w + (nd - 4), 4) / 4.0f;
    const float pdev = np_sum_f32_wave(s_real_w, nd, lane) / (float)nd;
    const float mean_df = s.was_locked ? np_sum_f32_wave(s_df_w, s.df_len, lane) / (float)s.df_len : 0.f;
    epi_loop_filter(pdev, mean_df, s.df_len, s.was_locked, P, s_df_w, so, lane, 64, R.df, R.new_len, R.locked);

    epi_carrier(s.freq0, s.phase0, s.omega0, R.offset, R.df, P, R.freq, R.phase, R.om_new);
    if (lane == 0) epi_store(si, so, o, d, cs, R);
}

// a closed channel: its state row is copied through, its record is all-zero (prn = 0); every
// byte of an open channel's record is written by the correlation kernel and the epilogue, so
// the result buffer needs no memset per launch
__device__ __forceinline__ void epilogue_closed(const gpsmi_trk_state& si, gpsmi_trk_state& so,
                                                gpsmi_trk_out& out, bool copy, int lane, int nlanes = 64) {
    if (copy) {
        const int* a = reinterpret_cast<const int*>(&si);
        int* b = reinterpret_cast<int*>(&so);
        for (int i = lane; i < (int)(sizeof(gpsmi_trk_state) / 4); i += nlanes) b[i] = a[i];
    }
    int* z = reinterpret_cast<int*>(&out);
    for (int i = lane; i < (int)(sizeof(gpsmi_trk_out) / 4); i += nlanes) z[i] = 0;
}

// One wave per job (four jobs per workgroup): the batch form.
__global__ __launch_bounds__(256) void trk_epilogue_kernel(
    const gpsmi_trk_state* __restrict__ st_in, gpsmi_trk_state* __restrict__ st_out,
    const JobMid* __restrict__ mid, const float2* __restrict__ partial, TrkParams P,
    int njobs, gpsmi_trk_out* __restrict__ out) {
    __shared__ float s_mag[4][40], s_dev[4][40], s_real[4][40], s_df[4][GPSMI_MAX_DF];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int job = blockIdx.x * 4 + wave;
    if (job >= njobs) return;
    if (!mid[job].active) {
        epilogue_closed(st_in[job], st_out[job], out[job], st_out != st_in, lane);
        return;
    }
    epilogue_job(st_in[job], st_out[job], mid[job].delay_used, partial + (size_t)job * (P.n_cyc + 1), P,
                 out[job], lane, s_mag[wave], s_dev[wave], s_real[wave], s_df[wave]);
}

// ---- The batch form with EIGHT LANES per job (round 4; option "epilogue_form" = 1, the default).
// The wave-per-job kernel above spends a whole wave -- and, beside the code-phase correlation of the
// next batch, a wave slot with its registers on every SIMD of a CU for the ~10 us of its dependent
// chain -- on 33 dumps: 12288 jobs = 3072 workgroups that each keep one of that kernel's workgroups
// off a CU while they wait for their own loads.  Here lane j of a job's eight carries the dumps
// i = j, j + 8, j + 16, ... (slot k = i / 8; the (N_CYC + 1)-th dump is slot N_CYC / 8 of lane 0), a
// wave is a workgroup and takes eight jobs: 1536 one-wave workgroups instead of 3072 four-wave ones,
// an eighth of the wave slots.  The arithmetic is epilogue_job's -- the epi_* functions above -- and where
// the layout differs, the same operations:
//   * numpy's pairwise sum IS this layout: its eight strided accumulators r[j] = a[j] + a[j + 8] + ...
//     are the lanes' own slots added in slot order, the tree is the same three DPP steps (they stay
//     inside a group of eight lanes), the tail element comes from lane 0's last slot;
//   * the masks of the edge scan (dump positive / negative / step large) and the +-1 jumps of the phase
//     unwrapping are bits i of per-job 64-bit words, OR-ed over the eight lanes by DPP; the scan is the
//     same arithmetic on them in every lane of the group, the unwrap count of dump i is two popcounts
//     (small integers: exact, like the float prefix sum of the wave form);
//   * the neighbour dump (i - 1) is lane j - 1's slot k, or lane 7's slot k - 1 for j = 0: one
//     rotation inside the group per slot.
// Same bits as the wave form (tests/test_gpu_trk.py: both forms against each other and replay ==
// closed loop, whose single-block epilogue is the wave form).
// OR over the eight lanes of a group, in every lane of it (tree8's steps)
template <int CTRL>
__device__ __forceinline__ unsigned dpp_or(unsigned v) {
    return v | (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false);
}
__device__ __forceinline__ unsigned long long or8(unsigned long long m) {
    unsigned lo = (unsigned)m, hi = (unsigned)(m >> 32);
    lo = dpp_or<kQuadSwap1>(lo); hi = dpp_or<kQuadSwap1>(hi);
    lo = dpp_or<kQuadSwap2>(lo); hi = dpp_or<kQuadSwap2>(hi);
    lo = dpp_or<kHalfMirror>(lo); hi = dpp_or<kHalfMirror>(hi);
    return ((unsigned long long)hi << 32) | lo;
}
// lane `l` of this lane's group of eight
__device__ __forceinline__ float grp_get(float v, int lane, int l) { return __shfl(v, (lane & ~7) | l, 64); }
// np.sum of a[0 .. n), element i in slot i / 8 of lane i % 8; n = 8 (K - 1) or 8 (K - 1) + 1
template <int K>
__device__ __forceinline__ float np_sum8(const float (&a)[K], int n, int lane) {
    float r = a[0];
#pragma unroll
    for (int k = 1; k < K - 1; ++k) r = add_rn(r, a[k]);
    r = tree8(r);
    const float t = grp_get(a[K - 1], lane, 0);
    if (n > 8 * (K - 1)) r = add_rn(r, t);
    return r;
}

template <int NCV>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(6, 6))) void trk_epilogue8_kernel(
    const gpsmi_trk_state* __restrict__ st_in, gpsmi_trk_state* __restrict__ st_out,
    const JobMid* __restrict__ mid, const float2* __restrict__ partial, TrkParams P,
    int njobs, gpsmi_trk_out* __restrict__ out) {
    constexpr int nc = NCV, K = NCV / 8 + 1, KD = (GPSMI_MAX_DUMPS + 7) / 8;
    static_assert(NCV % 8 == 0 && NCV + 1 <= GPSMI_MAX_DUMPS, "slots of eight dumps");
    __shared__ float s_real[8][NCV + 8], s_df[8][GPSMI_MAX_DF];
    const int lane = threadIdx.x & 63, j = lane & 7, jw = lane >> 3;
    const int job = blockIdx.x * 8 + jw;
    if (job >= njobs) return;                       // (whole groups: nothing below leaves a group)
    const gpsmi_trk_state& si = st_in[job];
    gpsmi_trk_state& so = st_out[job];
    gpsmi_trk_out& o = out[job];
    const JobMid md = mid[job];
    if (!md.active) {
        epilogue_closed(si, so, o, st_out != st_in, j, 8);
        return;
    }
    const float2* S = partial + (size_t)job * (nc + 1);
    const int d = md.delay_used, cs = P.cs;
    float* s_real_w = s_real[jw];
    float* s_df_w = s_df[jw];
    const EpiState s = epi_load(si);
    for (int i = j; i < s.df_len; i += 8) s_df_w[i] = si.df[i];

    // ---- prompt dumps: slot k of lane j is dump j + 8 k
    EpiResult R;
    epi_windows(S, nc, cs, d, s, R);
    const int nd = R.nd;
    float gr[K], gi[K];
#pragma unroll
    for (int k = 0; k < K; ++k) epi_dump(S, j + 8 * k, cs, s, R, gr[k], gi[k]);
#pragma unroll
    for (int k = 0; k < KD; ++k) {
        const int i = j + 8 * k;
        if (i < GPSMI_MAX_DUMPS) {
            o.dumps[2 * i] = k < K ? gr[k < K ? k : 0] : 0.f;
            o.dumps[2 * i + 1] = k < K ? gi[k < K ? k : 0] : 0.f;
        }
    }
    // the dump before dump i: slot k of lane j - 1, for j = 0 slot k - 1 of lane 7
    const int rot = (lane & ~7) | ((j + 7) & 7);

    // ---- edge scan: the masks bit by bit, OR-ed over the group
    if (s.was_locked) {
        const float thr = mul_rn(3.0f, s.std_dev0);
        unsigned long long Pm = 0, Nm = 0, Bm = 0;
        float before = s.prev_signal0;                 // lane 0: slot k - 1 of lane 7
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int i = j + 8 * k;
            const float up = __shfl(gr[k], rot, 64);
            const float re_prev = j == 0 ? before : up;
            before = up;
            if (i < nd) {
                if (gr[k] > 0.f) Pm |= 1ull << i;
                if (gr[k] < 0.f) Nm |= 1ull << i;
                if (fabsf(sub_rn(gr[k], re_prev)) > thr) Bm |= 1ull << i;
            }
        }
        Pm = or8(Pm); Nm = or8(Nm); Bm = or8(Bm);
        epi_edge_scan(Pm, Nm, Bm, nd, s.prev_signal0, s.edge_state0, R.edge_mask, R.edge_sign0, R.edge_state);
        const float last_full = grp_get(gr[K - 2], lane, 7), last_extra = grp_get(gr[K - 1], lane, 0);
        R.prev_signal = nd == nc + 1 ? last_extra : last_full;     // the real part of dump nd - 1
        R.ms_count = nd;
    }

    // ---- amplitude statistics (gpslib.py:1186-1187)
    float mag[K], dev[K];
#pragma unroll
    for (int k = 0; k < K; ++k) mag[k] = hypotf(gr[k], gi[k]);
    R.mmean = np_sum8<K>(mag, nd, lane) / (float)nd;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const float e = sub_rn(mag[k], R.mmean);
        dev[k] = mul_rn(e, e);
    }
    R.sdev = sqrtf(np_sum8<K>(dev, nd, lane) / (float)nd);

    // ---- phaseLockedLoop (gpslib.py:1215-1262): unwrap by two popcounts
    float ph[K], real[K];
    unsigned long long Jp = 0, Jn = 0;                 // dumps whose unwrap step is +1 / -1
    {
        float before = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int i = j + 8 * k;
            ph[k] = atanf(gi[k] / gr[k]);
            const float up = __shfl(ph[k], rot, 64);
            const float ph_prev = j == 0 ? before : up;
            before = up;
            if (i >= 1 && i < nd) {
                const float delta = sub_rn(ph[k], ph_prev);
                if (fabsf(delta) > 2.0f) {
                    if (delta > 0.f) Jn |= 1ull << i;
                    else Jp |= 1ull << i;
                }
            }
        }
    }
    Jp = or8(Jp); Jn = or8(Jn);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int i = j + 8 * k;
        const unsigned long long upto = (2ull << i) - 1;               // dumps 0 .. i
        const float jump = (float)(__builtin_popcountll(Jp & upto) - __builtin_popcountll(Jn & upto));
        real[k] = (i == 0) ? ph[k] : add_rn(ph[k], mul_rn(jump, kPiF));
        if (i < nd) s_real_w[i] = real[k];
    }
    __builtin_amdgcn_wave_barrier();
    R.offset = np_sum_f32(s_real_w + (nd - 4), 4) / 4.0f;
    const float pdev = np_sum8<K>(real, nd, lane) / (float)nd;
    const float mean_df = s.was_locked ? np_sum_f32_grp(s_df_w, s.df_len, j) / (float)s.df_len : 0.f;
    epi_loop_filter(pdev, mean_df, s.df_len, s.was_locked, P, s_df_w, so, j, 8, R.df, R.new_len, R.locked);

    epi_carrier(s.freq0, s.phase0, s.omega0, R.offset, R.df, P, R.freq, R.phase, R.om_new);
    if (j == 0) epi_store(si, so, o, d, cs, R);
}

// One workgroup per job: behind the single-block form of the span correlator (the closed
// loop).  The four waves add up the spans of one quarter each (independent loads, issued
// together), wave 0 adds the quarters in their fixed order, forms the windows and runs the
// per-job part.
template <int NC>
__global__ __launch_bounds__(256) void trk_epilogue_span_kernel(
    const gpsmi_trk_state* __restrict__ st_in, gpsmi_trk_state* __restrict__ st_out,
    const JobMid* __restrict__ mid, const float* __restrict__ rec, int ng_span, TrkParams P,
    int njobs, gpsmi_trk_out* __restrict__ out) {
    __shared__ float s_mag[40], s_dev[40], s_real[40], s_df[GPSMI_MAX_DF];
    __shared__ float q_hi[4][64], q_lo[4][64], s_hi[64], s_lo[64];
    __shared__ float2 s_S[GPSMI_MAX_DUMPS];
    __shared__ gpsmi_trk_state s_si;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int job = blockIdx.x;
    // the state row is requested with the job entry (one trip to memory for both) and waits in
    // LDS for the per-job part
    if (wave == 0) {
        const int* a = reinterpret_cast<const int*>(&st_in[job]);
        int* sa = reinterpret_cast<int*>(&s_si);
        for (int i = lane; i < (int)(sizeof(gpsmi_trk_state) / 4); i += 64) sa[i] = a[i];
    }
    const JobMid md = mid[job];
    if (!md.active) {
        if (wave == 0) epilogue_closed(st_in[job], st_out[job], out[job], st_out != st_in, lane);
        return;
    }
    span_collect_quarter<1, NC>(rec, ng_span, job / P.nch, job % P.nch, md.delay_used, lane, wave,
                                q_hi[wave][lane], q_lo[wave][lane]);
    __syncthreads();
    if (wave != 0) return;
    float h = 0.f, l = 0.f;
#pragma unroll
    for (int Q = 0; Q < 4; ++Q) { h += q_hi[Q][lane]; l += q_lo[Q][lane]; }
    s_hi[lane] = h;
    s_lo[lane] = l;
    __builtin_amdgcn_wave_barrier();
    span_windows<NC>(s_hi, s_lo, md.om, lane, s_S);
    __builtin_amdgcn_wave_barrier();
    epilogue_job(s_si, st_out[job], md.delay_used, s_S, P, out[job], lane, s_mag, s_dev, s_real, s_df);
}

// One wave per job (four jobs per workgroup) behind trk_span8_kernel: the wave adds up the 11 range
// records of its job (span8_collect) and runs the per-job part on the windows: no separate collect
// launch, no round trip of the window sums through memory.
__global__ __launch_bounds__(256) void trk_epilogue_span8_kernel(
    const gpsmi_trk_state* __restrict__ st_in, gpsmi_trk_state* __restrict__ st_out,
    const JobMid* __restrict__ mid, const float* __restrict__ rec, int ngroups, TrkParams P, int njobs,
    gpsmi_trk_out* __restrict__ out) {
    __shared__ float s_mag[4][40], s_dev[4][40], s_real[4][40], s_df[4][GPSMI_MAX_DF];
    __shared__ float s_hi[4][16], s_lo[4][16];
    __shared__ float2 s_S[4][GPSMI_MAX_DUMPS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int job = blockIdx.x * 4 + wave;
    if (job >= njobs) return;
    const JobMid md = mid[job];
    if (!md.active) {
        epilogue_closed(st_in[job], st_out[job], out[job], st_out != st_in, lane);
        return;
    }
    span8_collect(rec, ngroups, job / P.nch, job % P.nch, md.delay_used, md.om, lane, s_hi[wave], s_lo[wave],
                  s_S[wave]);
    epilogue_job(st_in[job], st_out[job], md.delay_used, s_S[wave], P, out[job], lane, s_mag[wave], s_dev[wave],
                 s_real[wave], s_df[wave]);
}

}  // namespace gpsmi
