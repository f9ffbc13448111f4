// Streaming front end: sample decode, IF / tuner-offset mix, band-limiting filter and resampler to the
// engine's rate (gpsmi_fe_*, include/gpsmi.h; numpy restatement: tests/fe_ref.py).
//
// Time: input sample i sits at time i / fs_in, output sample n at n / fs_out, i.e. at the input
// position t_n = n P / Q with P / Q = fs_in / fs_out reduced.  The handle keeps two integers, the
// input samples taken (a) and the outputs emitted (n_next); every call derives (floor t_n, t_n mod 1)
// exactly from them (n P divmod Q), so nothing drifts however long the stream runs.
//
// Filter: y[n] = sum over the K input samples i = floor(t_n) - K/2 + 1 .. floor(t_n) + K/2 of
// x[i] h(t_n - i), h a Kaiser-windowed sinc centred on t_n (no group delay; input before index 0 is
// zero).  h is tabulated at L phases per input sample: row j (0 .. L) holds h(j / L + K/2 - 1 - m),
// m = 0 .. K - 1, and the row pair (j, j + 1) around the fraction is combined linearly,
// y = A_j + mu (A_{j+1} - A_j), A_j the dot product with row j.
//
//   fe_stage_kernel   one thread per sample of [carry | new input]: the carry (the last Kc mixed
//                     samples of the previous call, zero after create / reset) is copied in front,
//                     each new sample is decoded and mixed by exp(-j 2 pi if_hz i / fs_in), the
//                     phase i * inc mod 2^64 in integers (inc = if_hz / fs_in in 0.64 fixed point).
//   fe_filter_kernel  one workgroup per run of R consecutive outputs: the tap table and the input
//                     span of the run go to LDS once, then thread t computes output t of the run:
//                     two dot products in ascending tap order, one thread, no atomics.
//   fe_carry_kernel   the last Kc samples of [carry | new input] -> the handle's carry.
//
// Every output sample is one fixed-order sum computed by one thread from values that depend only on
// the input sample and its absolute index, so the output bits do not depend on how the input was cut
// into calls, on the grid or on the run.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gpsmi_common.h"
#include "gpsmi_stage.h"

namespace gpsmi {

constexpr int kFeMaxTaps = 8192;
constexpr int kFeMaxPhases = 1024;
constexpr size_t kFeLdsBudget = 64 * 1024;        // preferred dynamic LDS per workgroup
constexpr size_t kFeLdsMax = 160 * 1024;          // gfx950: LDS of one CU
constexpr int kFeZero = 5;                        // stage "format": zeros (flush)

// sample k of the caller's input, as a complex float of full scale 1
template <int FMT>
__device__ __forceinline__ float2 fe_decode(const void* in, long long k) {
    if constexpr (FMT == GPSMI_FE_C64) return static_cast<const float2*>(in)[k];
    else if constexpr (FMT == GPSMI_FE_U8IQ) return decode_u8iq(static_cast<const uint16_t*>(in)[k]);
    else if constexpr (FMT == GPSMI_FE_SC8) {
        const int8_t* v = static_cast<const int8_t*>(in) + 2 * k;
        return make_float2((float)v[0] * (1.0f / 128.0f), (float)v[1] * (1.0f / 128.0f));
    } else if constexpr (FMT == GPSMI_FE_SC16) {
        const int16_t* v = static_cast<const int16_t*>(in) + 2 * k;
        return make_float2((float)v[0] * (1.0f / 32768.0f), (float)v[1] * (1.0f / 32768.0f));
    } else if constexpr (FMT == GPSMI_FE_R8) {      // real: x 2, so a cosine of amplitude A -> tone A
        return make_float2((float)static_cast<const int8_t*>(in)[k] * (2.0f / 128.0f), 0.0f);
    } else {
        return make_float2(0.0f, 0.0f);
    }
}

// vbuf[j], j < kc: carry[j]; vbuf[kc + k]: input sample k (absolute index a + k) decoded and mixed
template <int FMT>
__global__ __launch_bounds__(256) void fe_stage_kernel(const void* __restrict__ in,
                                                       const float2* __restrict__ carry, int kc,
                                                       long long n_in, long long a, unsigned long long inc,
                                                       int conj, float2* __restrict__ vbuf) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= kc + n_in) return;
    if (j < kc) {
        vbuf[j] = carry[j];
        return;
    }
    const long long k = j - kc;
    float2 v = fe_decode<FMT>(in, k);
    if (conj) v.y = -v.y;
    // phase / 2 pi = ((a + k) inc mod 2^64) / 2^64; its top 24 bits as a signed fraction of pi
    const unsigned long long ph = (unsigned long long)(a + k) * inc;
    const float x = (float)((long long)ph >> 40) * 0x1p-23f;           // [-1, 1), exact
    float sn, cs;
    sincospif(x, &sn, &cs);
    vbuf[j] = make_float2(v.x * cs + v.y * sn, v.y * cs - v.x * sn);   // v exp(-j pi x)
}

// Outputs k = 0 .. n_out - 1 of this call (absolute n_next + k) at input position I0 + (r0 + k P) / Q;
// vbuf[0] is the input sample of absolute index vbase.  LDS: the table [(L + 1) K] (tab_floats,
// padded to even), then the span of the run (complex).
__global__ __launch_bounds__(256) void fe_filter_kernel(const float2* __restrict__ vbuf, long long vbase,
                                                        long long I0, long long r0, long long P, long long Q,
                                                        int K, int L, const float* __restrict__ table,
                                                        int tab_floats, int R, long long n_out,
                                                        float2* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float fe_lds[];
    float* tab = fe_lds;
    float2* xs = reinterpret_cast<float2*>(fe_lds + tab_floats);
    const int t = threadIdx.x;
    const long long k0 = (long long)blockIdx.x * R;
    const long long k1 = min(k0 + (long long)R, n_out) - 1;
    const long long first = I0 + (r0 + k0 * P) / Q - K / 2 + 1;      // input span of the run
    const long long last = I0 + (r0 + k1 * P) / Q + K / 2;
    const int len = (int)(last - first + 1);
    const int ntab = (L + 1) * K;
    for (int i = t; i < ntab; i += blockDim.x) tab[i] = table[i];
    const float2* src = vbuf + (first - vbase);
    for (int i = t; i < len; i += blockDim.x) xs[i] = src[i];
    __syncthreads();
    const long long k = k0 + t;
    if (t >= R || k >= n_out) return;
    const long long num = r0 + k * P;
    const long long I = I0 + num / Q, r = num % Q;
    const long long rl = r * L;
    const int j = (int)(rl / Q);
    const float mu = (float)(rl % Q) / (float)Q;
    const float* h0 = tab + j * K;
    const float* h1 = h0 + K;
    const float2* x = xs + (I - K / 2 + 1 - first);
    float a0r = 0.f, a0i = 0.f, a1r = 0.f, a1i = 0.f;
#pragma unroll 4
    for (int m = 0; m < K; ++m) {
        const float2 v = x[m];
        const float w0 = h0[m], w1 = h1[m];
        a0r += w0 * v.x;
        a0i += w0 * v.y;
        a1r += w1 * v.x;
        a1i += w1 * v.y;
    }
    out[k] = make_float2(a0r + mu * (a1r - a0r), a0i + mu * (a1i - a0i));
}

__global__ __launch_bounds__(256) void fe_carry_kernel(const float2* __restrict__ vbuf, long long n_in,
                                                       int kc, float2* __restrict__ carry) {
    for (int j = threadIdx.x; j < kc; j += 256) carry[j] = vbuf[n_in + j];
}

static long long gcd_ll(long long a, long long b) {
    while (b) {
        const long long c = a % b;
        a = b;
        b = c;
    }
    return a;
}

static double bessel_i0(double x) {
    double s = 1.0, term = 1.0;
    for (int k = 1; k < 500; ++k) {
        const double q = x / (2.0 * k);
        term *= q * q;
        s += term;
        if (term < 1e-18 * s) break;
    }
    return s;
}

// Everything create needs that does not touch HIP: the validated configuration and the filter.
struct FePlan {
    long long P = 0, Q = 0;           // fs_in / fs_out reduced
    int K = 0, L = 0;                 // taps, phases per input sample
    int kc = 0;                       // carry length: K + ceil(P / Q)
    int R = 0;                        // outputs per workgroup
    int tab_floats = 0;               // (L + 1) K rounded up to even
    size_t lds = 0;                   // dynamic LDS bytes of the filter kernel
    unsigned long long inc = 0;       // if_hz / fs_in in 0.64 fixed point (two's complement)
    double p = 0, s = 0;              // passband edge, stopband edge (Hz)
    std::vector<float> table;         // [(L + 1) K]
};

static int fe_plan(const gpsmi_fe_cfg* c, FePlan* pl) {
    GPSMI_REQUIRE(c, "null argument");
    GPSMI_REQUIRE(c->fs_in_hz > 0 && c->fs_in_hz <= 0x7FFFFFFFLL, "fs_in_hz out of range 1 .. 2^31 - 1");
    GPSMI_REQUIRE(c->fs_out_hz > 0 && c->fs_out_hz <= 0x7FFFFFFFLL, "fs_out_hz out of range 1 .. 2^31 - 1");
    GPSMI_REQUIRE(c->format >= GPSMI_FE_C64 && c->format <= GPSMI_FE_R8, "unknown sample format");
    GPSMI_REQUIRE((c->flags & ~GPSMI_FE_CONJUGATE) == 0, "unknown flag bits");
    GPSMI_REQUIRE(!(c->format == GPSMI_FE_R8 && (c->flags & GPSMI_FE_CONJUGATE)),
                  "conjugate needs complex input (the sign of if_hz picks the sideband of real input)");
    GPSMI_REQUIRE(std::isfinite(c->if_hz), "if_hz is not finite");
    GPSMI_REQUIRE(std::isfinite(c->passband_hz) && c->passband_hz >= 0.f, "passband_hz negative or not finite");
    GPSMI_REQUIRE(std::isfinite(c->atten_db) && (c->atten_db == 0.f || (c->atten_db >= 20.f && c->atten_db <= 120.f)),
                  "atten_db out of range 20 .. 120 (0: 60)");
    const double fi = (double)c->fs_in_hz, fo = (double)c->fs_out_hz;
    const bool real = c->format == GPSMI_FE_R8;
    if (fi < 0.5 * fo || fi > 64.0 * fo)
        return fail(GPSMI_E_UNSUPPORTED, "gpsmi_fe: fs_in / fs_out = %g outside 0.5 .. 64", fi / fo);
    const double fmin = fi < fo ? fi : fo;
    const double p = c->passband_hz > 0.f ? (double)c->passband_hz : 0.44 * fmin;
    if (p >= 0.5 * fmin)
        return fail(GPSMI_E_UNSUPPORTED, "gpsmi_fe: passband %.0f Hz not below min(fs_in, fs_out) / 2 = %.0f Hz",
                    p, 0.5 * fmin);
    double s = fmin - p;                       // the nearest frequency that aliases into |f| <= p
    const double ifr = c->if_hz - fi * std::floor(c->if_hz / fi + 0.5);    // IF in [-fs_in/2, fs_in/2)
    if (real) {
        // after the mix, the mirror half of the real spectrum occupies [fs_in/2 - IF, fs_in - IF] mod fs_in
        // (IF > 0; the other side for IF < 0): it starts d = min(|IF|, fs_in/2 - |IF|) from 0
        const double d = std::fmin(std::fabs(ifr), 0.5 * fi - std::fabs(ifr));
        if (d <= p)
            return fail(GPSMI_E_UNSUPPORTED,
                        "gpsmi_fe: the image of real input at IF %.0f Hz reaches %.0f Hz from 0, inside the "
                        "passband %.0f Hz (pass a narrower passband_hz)", c->if_hz, d, p);
        s = std::fmin(s, d);
    }
    const double A = (c->atten_db > 0.f ? (double)c->atten_db : 60.0) + 6.0;   // 6 dB design margin
    const double beta = A > 50.0 ? 0.1102 * (A - 8.7) : 0.5842 * std::pow(A - 21.0, 0.4) + 0.07886 * (A - 21.0);
    const double dw = 2.0 * M_PI * (s - p) / fi;                               // transition, rad / sample
    const double kf = std::ceil((A - 7.95) / (2.285 * dw)) + 1.0;
    if (!(kf <= kFeMaxTaps))
        return fail(GPSMI_E_UNSUPPORTED, "gpsmi_fe: transition %.0f .. %.0f Hz needs %.0f taps (at most %d)", p, s,
                    kf, kFeMaxTaps);
    int K = (int)kf;
    K += K & 1;
    if (K < 4) K = 4;
    // linear interpolation between phases: gain error <= (2 pi f / fs_in / L)^2 / 8 at f <= s, kept below 1e-4
    int L = 1;
    while (L < kFeMaxPhases && L < 2.0 * M_PI * (s / fi) / std::sqrt(8e-4)) L <<= 1;
    const long long g = gcd_ll(c->fs_in_hz, c->fs_out_hz);
    pl->P = c->fs_in_hz / g;
    pl->Q = c->fs_out_hz / g;
    pl->K = K;
    pl->L = L;
    pl->kc = K + (int)((pl->P + pl->Q - 1) / pl->Q);
    pl->p = p;
    pl->s = s;
    pl->tab_floats = ((L + 1) * K + 1) & ~1;
    pl->R = 0;
    for (int R = 256; R >= 64 && !pl->R; R >>= 1) {
        const long long span = (long long)(R - 1) * pl->P / pl->Q + 1 + K;
        const size_t lds = (size_t)pl->tab_floats * sizeof(float) + (size_t)span * sizeof(float2);
        if (lds <= kFeLdsBudget || (R == 64 && lds <= kFeLdsMax)) {
            pl->R = R;
            pl->lds = lds;
        }
    }
    if (!pl->R)
        return fail(GPSMI_E_UNSUPPORTED, "gpsmi_fe: %d taps x %d phases do not fit the LDS of one CU", K, L);
    // the prototype: h(tau) = 2 fc sinc(2 fc tau) kaiser(tau), tau in input samples, |tau| < K / 2
    const double fc = 0.5 * (p + s) / fi;
    const double i0b = bessel_i0(beta), half = 0.5 * K;
    auto h = [&](double tau) {
        const double u = tau / half;
        if (u <= -1.0 || u >= 1.0) return 0.0;
        const double a = 2.0 * M_PI * fc * tau;
        const double sinc = std::fabs(a) < 1e-12 ? 1.0 : std::sin(a) / a;
        return 2.0 * fc * sinc * bessel_i0(beta * std::sqrt(1.0 - u * u)) / i0b;
    };
    // unit gain at 0 Hz of the interpolated prototype: its integral is the grid sum / L
    double area = 0.0;
    for (long long q = -(long long)half * L; q <= (long long)half * L; ++q) area += h((double)q / L);
    area /= L;
    pl->table.assign((size_t)(L + 1) * K, 0.f);
    for (int j = 0; j <= L; ++j)
        for (int m = 0; m < K; ++m)
            pl->table[(size_t)j * K + m] = (float)(h((double)j / L + half - 1 - m) / area);
    // mix increment: frac(if_hz / fs_in) in 0.64 fixed point
    double f = c->if_hz / fi;
    f -= std::floor(f);
    long double scaled = std::ldexp((long double)f, 64);
    if (scaled >= std::ldexp((long double)1.0, 64)) scaled = 0.0L;
    pl->inc = (unsigned long long)scaled;
    return GPSMI_OK;
}

}  // namespace gpsmi

using namespace gpsmi;

struct gpsmi_fe {
    gpsmi_fe_cfg cfg;
    FePlan plan;
    DevBuf<float> d_table;
    DevBuf<float2> d_carry;                                 // [kc]
    DevBuf<float2> d_vbuf;                                  // [kc + n_in]
    DevBuf<char> d_in;                                      // host entry: staged input (bytes: five formats)
    DevBuf<float2> d_out;                                   // host entry: [max_out], fixed at create
    long long taken = 0;                                    // input samples since create / reset
    long long emitted = 0;                                  // outputs since create / reset
    bool flushed = false;
    StageSync sync;                                         // last: see gpsmi_stage.h
};

static size_t fe_sample_bytes(int fmt) {
    switch (fmt) {
        case GPSMI_FE_C64: return 8;
        case GPSMI_FE_U8IQ: return 2;
        case GPSMI_FE_SC8: return 2;
        case GPSMI_FE_SC16: return 4;
        default: return 1;
    }
}

// outputs complete once `total` input samples are in: n with floor(n P / Q) + K / 2 <= total - 1
static long long fe_complete(const FePlan& pl, long long total) {
    const long long M = total - 1 - pl.K / 2;
    if (M < 0) return 0;
    const __int128 num = (__int128)(M + 1) * pl.Q;
    return (long long)((num + pl.P - 1) / pl.P);
}

// One call: n_in samples at d_in (device, the handle's format; null: zeros) -> n_out outputs at d_out.
static int fe_run(gpsmi_fe* h, const void* d_in, long long n_in, float2* d_out, long long n_out) {
    const FePlan& pl = h->plan;
    const hipStream_t st = h->sync.stream;
    int rc = h->d_vbuf.reserve((size_t)(pl.kc + n_in), "front-end sample scratch");
    if (!rc) rc = h->sync.begin();
    if (rc) return rc;
    with_value<kFeZero, GPSMI_FE_C64, GPSMI_FE_U8IQ, GPSMI_FE_SC8, GPSMI_FE_SC16, GPSMI_FE_R8>(
        d_in ? h->cfg.format : kFeZero, [&](auto fmt) {
            const long long n = pl.kc + n_in;
            hipLaunchKernelGGL(fe_stage_kernel<decltype(fmt)::value>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                               st, d_in, h->d_carry.p, pl.kc, n_in, h->taken, pl.inc,
                               (h->cfg.flags & GPSMI_FE_CONJUGATE) ? 1 : 0, h->d_vbuf.p);
        });
    if (n_out > 0) {
        const __int128 t0 = (__int128)h->emitted * pl.P;
        const long long I0 = (long long)(t0 / pl.Q), r0 = (long long)(t0 % pl.Q);
        const long long vbase = h->taken - pl.kc;
        const unsigned groups = (unsigned)((n_out + pl.R - 1) / pl.R);
        hipLaunchKernelGGL(fe_filter_kernel, dim3(groups), dim3((unsigned)pl.R), pl.lds, st, h->d_vbuf.p, vbase, I0,
                           r0, pl.P, pl.Q, pl.K, pl.L, h->d_table.p, pl.tab_floats, pl.R, n_out, d_out);
    }
    hipLaunchKernelGGL(fe_carry_kernel, dim3(1), dim3(256), 0, st, h->d_vbuf.p, n_in, pl.kc, h->d_carry.p);
    return h->sync.end();
}

// The tail of every entry point: run, the n outputs on their way to `host_out` (null: they stay at
// d_out), finish, bookkeeping.
static int fe_call(gpsmi_fe* h, const void* d_in, long long n_in, float2* d_out, long long n, float* host_out,
                   size_t* n_out) {
    int rc = fe_run(h, d_in, n_in, d_out, n);
    if (rc) return rc;
    if (host_out && n > 0)
        GPSMI_HIP(hipMemcpyAsync(host_out, d_out, (size_t)n * sizeof(float2), hipMemcpyDeviceToHost,
                                 h->sync.stream));
    if ((rc = h->sync.finish())) return rc;
    h->taken += n_in;
    h->emitted += n;
    *n_out = (size_t)n;
    return GPSMI_OK;
}

static int fe_check_call(gpsmi_fe* h, size_t n_in, size_t max_out, long long* n_out) {
    GPSMI_REQUIRE(!h->flushed, "the stream was flushed: reset the handle first");
    GPSMI_REQUIRE(n_in <= ((size_t)1 << 31), "n_in out of range 0 .. 2^31");
    const long long n = fe_complete(h->plan, h->taken + (long long)n_in) - h->emitted;
    *n_out = n > 0 ? n : 0;
    if ((size_t)*n_out > max_out)
        return fail(GPSMI_E_ARG, "gpsmi_fe: this call emits %lld samples, max_out is %zu", *n_out, max_out);
    return GPSMI_OK;
}

extern "C" {

int gpsmi_fe_design(const gpsmi_fe_cfg* cfg, int* n_taps, int* n_phases, float* table) {
    GPSMI_REQUIRE(cfg && n_taps && n_phases, "null argument");
    FePlan pl;
    const int rc = fe_plan(cfg, &pl);
    if (rc) return rc;
    *n_taps = pl.K;
    *n_phases = pl.L;
    if (table) memcpy(table, pl.table.data(), pl.table.size() * sizeof(float));
    return GPSMI_OK;
}

int gpsmi_fe_create(const gpsmi_fe_cfg* cfg, gpsmi_fe** out) {
    GPSMI_REQUIRE(cfg && out, "null argument");
    *out = nullptr;
    GPSMI_REQUIRE(cfg->max_out >= 1, "max_out must be >= 1");
    FePlan pl;
    int rc = fe_plan(cfg, &pl);
    if (rc) return rc;
    return stage_create(cfg, out, [&](gpsmi_fe* h) {
        h->plan = std::move(pl);
        const FePlan& p = h->plan;
        if (p.lds > kFeLdsBudget)
            GPSMI_HIP(hipFuncSetAttribute((const void*)fe_filter_kernel,
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds));
        int rc = h->d_table.upload(p.table, "front-end filter table");
        if (!rc) rc = h->d_carry.reserve_zeroed(p.kc, "front-end carry");
        if (!rc) rc = h->d_out.reserve(h->cfg.max_out, "front-end output block");
        return rc;
    });
}

int gpsmi_fe_destroy(gpsmi_fe* h) { return stage_destroy(h); }

int gpsmi_fe_reset(gpsmi_fe* h) {
    GPSMI_REQUIRE(h, "null handle");
    GPSMI_HIP(hipSetDevice(h->cfg.device));
    GPSMI_HIP(hipMemsetAsync(h->d_carry.p, 0, (size_t)h->plan.kc * sizeof(float2), h->sync.stream));
    GPSMI_HIP(hipStreamSynchronize(h->sync.stream));
    h->taken = 0;
    h->emitted = 0;
    h->flushed = false;
    return GPSMI_OK;
}

int gpsmi_fe_push_dev(gpsmi_fe* h, const void* d_in, size_t n_in, void* d_out, size_t max_out, size_t* n_out) {
    GPSMI_REQUIRE(h && n_out && (d_in || n_in == 0), "null argument");
    long long n = 0;
    int rc = fe_check_call(h, n_in, max_out, &n);
    if (rc) return rc;
    GPSMI_REQUIRE(d_out || n == 0, "null output");
    *n_out = 0;
    if (n_in == 0) return GPSMI_OK;
    GPSMI_HIP(hipSetDevice(h->cfg.device));
    return fe_call(h, d_in, (long long)n_in, static_cast<float2*>(d_out), n, nullptr, n_out);
}

int gpsmi_fe_push(gpsmi_fe* h, const void* in, size_t n_in, float* out, size_t max_out, size_t* n_out) {
    GPSMI_REQUIRE(h && n_out && (in || n_in == 0), "null argument");
    long long n = 0;
    int rc = fe_check_call(h, n_in, max_out, &n);
    if (rc) return rc;
    GPSMI_REQUIRE(out || n == 0, "null output");
    if (n > h->cfg.max_out)
        return fail(GPSMI_E_ARG, "gpsmi_fe_push: this call emits %lld samples, the handle's max_out is %d", n,
                    (int)h->cfg.max_out);
    *n_out = 0;
    if (n_in == 0) return GPSMI_OK;
    GPSMI_HIP(hipSetDevice(h->cfg.device));
    const size_t ib = n_in * fe_sample_bytes(h->cfg.format);
    rc = h->d_in.reserve(ib, "front-end staging");
    if (rc) return rc;
    GPSMI_HIP(hipMemcpyAsync(h->d_in.p, in, ib, hipMemcpyHostToDevice, h->sync.stream));
    return fe_call(h, h->d_in.p, (long long)n_in, h->d_out.p, n, out, n_out);
}

int gpsmi_fe_flush(gpsmi_fe* h, float* out, size_t max_out, size_t* n_out) {
    GPSMI_REQUIRE(h && n_out, "null argument");
    const long long pad = h->plan.K / 2;
    long long n = 0;
    int rc = fe_check_call(h, (size_t)pad, max_out, &n);
    if (rc) return rc;
    GPSMI_REQUIRE(out || n == 0, "null output");
    if (n > h->cfg.max_out)
        return fail(GPSMI_E_ARG, "gpsmi_fe_flush: emits %lld samples, the handle's max_out is %d", n,
                    (int)h->cfg.max_out);
    GPSMI_HIP(hipSetDevice(h->cfg.device));
    rc = fe_call(h, nullptr, pad, h->d_out.p, n, out, n_out);
    if (!rc) h->flushed = true;
    return rc;
}

int gpsmi_fe_last_ms(gpsmi_fe* h, float* ms) { return stage_last_ms(h, ms, __func__); }

}  // extern "C"
