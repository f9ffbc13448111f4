// What the scope of an event costs at the boundaries of the replay step.
// Two dependent kernels shaped like the step's pair -- A: 3072 workgroups x 256 threads, 40 KiB of
// LDS, ~100 us (the code-phase correlation, corr_grid); B: 512 persistent workgroups x 256 threads,
// 75 KiB of LDS, ~95 us, a few MB written (the batch form of the span correlator, trk_geometry) --
// are chained A B A B ... on one stream, B launched each of the ways trk_launch launches the
// correlator, with a small kernel behind it on a second stream where the engine has its epilogue:
//   plain                              hipLaunchKernelGGL, nothing else
//   stop                               hipExtLaunchKernelGGL with a stop event; the side stream waits on it
//   start+stop                         ... and a start event as well
//   record                             plain launch, hipEventRecord behind it, the side stream waits on it
//   ...; next A waits back             the stop form, and A waits for the side stream's event of two steps ago
// each event form with default flags and with hipEventDisableSystemFence.  The gaps are taken from
// stamps the kernels take themselves (the constant 100 MHz clock: first wave in, last wave out), so no
// form is disturbed by the measurement.  Second table: the duration of a consumer kernel that re-reads
// 4 MiB of L2-resident data while events of either kind complete on another stream.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/probe/boundary_scope.hip -o tools/probe/boundary_scope
//   timeout -k 10 120 tools/probe/boundary_scope
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cstdio>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

typedef unsigned long long u64;
constexpr int kTableFloats = 1 << 20;            // 4 MiB, read through L2 by every kernel (index masked)
constexpr int kSteps = 120, kSkip = 20;
struct Stamps { u64 a0, a1, b0, b1; };           // begin / end of A and B of one step

__device__ __forceinline__ void stamp_in(u64* first) {
    if (threadIdx.x == 0) atomicMin(first, (u64)wall_clock64());
}
__device__ __forceinline__ void stamp_out(u64* last) {
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(last, (u64)wall_clock64());
}

// `iters` trips of: one L2-resident load, a few FMAs, a round through LDS.  out has gridDim.x * 256 floats.
template <int LDS_FLOATS>
__device__ __forceinline__ float body(const float* __restrict__ table, const float* __restrict__ dep, int iters,
                                      float* lds) {
    const int t = threadIdx.x;
    float acc = dep[(blockIdx.x * 256 + t) & (kTableFloats - 1)];       // what the kernel before wrote
    for (int i = 0; i < iters; ++i) {
        const float v = table[(blockIdx.x * 4099 + i * 256 + t) & (kTableFloats - 1)];
        acc = fmaf(acc, 0.999f, v);
        lds[(t + i * 257) % LDS_FLOATS] = acc;
        __syncthreads();
        acc += lds[(t * 5 + i) % LDS_FLOATS] * 0.5f;
    }
    return acc;
}

__global__ __launch_bounds__(256) void k_a(const float* __restrict__ table, const float* __restrict__ dep, int iters,
                                           float* __restrict__ out, u64* first, u64* last) {
    __shared__ float lds[40 * 256];              // 40 KiB
    stamp_in(first);
    out[blockIdx.x * 256 + threadIdx.x] = body<40 * 256>(table, dep, iters, lds);
    stamp_out(last);
}

// persistent: each workgroup writes `units` rows of 256 floats (out has gridDim.x * units * 256 floats)
__global__ __launch_bounds__(256) void k_b(const float* __restrict__ table, const float* __restrict__ dep, int iters,
                                           int units, float* __restrict__ out, u64* first, u64* last) {
    __shared__ float lds[75 * 256];              // 75 KiB
    stamp_in(first);
    for (int u = 0; u < units; ++u)
        out[(blockIdx.x * units + u) * 256 + threadIdx.x] = body<75 * 256>(table, dep, iters, lds) + u;
    stamp_out(last);
}

__global__ void k_side(const float* __restrict__ in, float* __restrict__ out) {      // the epilogue's place
    out[blockIdx.x * 64 + threadIdx.x] = in[blockIdx.x * 64 + threadIdx.x] + 1.f;
}

// the consumer: every workgroup walks the table `rounds` times, one word of every other 128-byte line
// (2 MiB of lines, which stay in L2)
__global__ __launch_bounds__(256) void k_reread(const float* __restrict__ table, int rounds, float* __restrict__ out,
                                                u64* first, u64* last) {
    stamp_in(first);
    float acc = 0.f;
    for (int r = 0; r < rounds; ++r)
        for (int i = threadIdx.x; i < kTableFloats / 64; i += 256)
            acc += table[(i * 64 + blockIdx.x * 16 + r) & (kTableFloats - 1)];
    out[blockIdx.x * 256 + threadIdx.x] = acc;
    stamp_out(last);
}

static double median(std::vector<double> v) {
    std::sort(v.begin(), v.end());
    return v.empty() ? 0.0 : v[v.size() / 2];
}

// a trip count for `want_us` from one that took `got_us`: at most 20 times more per pass, 100000 in all
// (a stamp that was never written must not turn into a kernel that runs for seconds)
static int rescale(int trips, double want_us, double got_us) {
    const double f = std::min(20.0, want_us / std::max(got_us, 1.0));
    return std::max(1, std::min(100000, (int)(trips * f)));
}

enum Form { Plain, Stop, StartStop, Record };

int main() {
    constexpr int kGridA = 3072, kGridB = 512, kUnitsB = 6;          // B writes 512 * 6 * 1 KiB = 3 MiB
    float *table, *out_a, *out_b, *side;
    Stamps* d_st;
    CK(hipMalloc(&table, kTableFloats * sizeof(float)));
    CK(hipMalloc(&out_a, kTableFloats * sizeof(float)));             // (read back masked to kTableFloats: same size)
    CK(hipMalloc(&out_b, kTableFloats * sizeof(float)));
    CK(hipMalloc(&side, 64 * 64 * sizeof(float)));
    CK(hipMalloc(&d_st, kSteps * sizeof(Stamps)));
    static_assert(kGridA * 256 <= kTableFloats && kGridB * kUnitsB * 256 <= kTableFloats, "outputs fit their buffers");
    CK(hipMemset(table, 0, kTableFloats * sizeof(float)));
    CK(hipMemset(out_a, 0, kTableFloats * sizeof(float)));
    CK(hipMemset(out_b, 0, kTableFloats * sizeof(float)));
    CK(hipMemset(side, 0, 64 * 64 * sizeof(float)));
    hipStream_t s1, s2;
    CK(hipStreamCreate(&s1)); CK(hipStreamCreate(&s2));
    std::vector<Stamps> st(kSteps);
    auto reset_stamps = [&]() -> int {
        for (auto& s : st) s = Stamps{~0ull, 0, ~0ull, 0};
        CK(hipMemcpy(d_st, st.data(), kSteps * sizeof(Stamps), hipMemcpyHostToDevice));
        return 0;
    };
    auto fetch_stamps = [&]() -> int {
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(st.data(), d_st, kSteps * sizeof(Stamps), hipMemcpyDeviceToHost));
        return 0;
    };
    const double tick_us = 0.01;                                     // the constant clock: 100 MHz

    // iteration counts for ~100 us (A) and ~95 us (B), from one run of each alone
    int it_a = 64, it_b = 64;
    for (int pass = 0; pass < 3; ++pass) {
        if (reset_stamps()) return 1;
        for (int k = 0; k < 8; ++k) {
            hipLaunchKernelGGL(k_a, dim3(kGridA), dim3(256), 0, s1, table, out_b, it_a, out_a, &d_st[k].a0, &d_st[k].a1);
            hipLaunchKernelGGL(k_b, dim3(kGridB), dim3(256), 0, s1, table, out_a, it_b, kUnitsB, out_b, &d_st[k].b0, &d_st[k].b1);
        }
        if (fetch_stamps()) return 1;
        const double da = (st[7].a1 - st[7].a0) * tick_us, db = (st[7].b1 - st[7].b0) * tick_us;
        it_a = rescale(it_a, 100.0, da);
        it_b = rescale(it_b, 95.0, db);
    }
    printf("A: %d x 256 threads, 40 KiB LDS, %d trips; B: %d x 256 threads, 75 KiB LDS, %d x %d trips\n\n", kGridA, it_a,
           kGridB, kUnitsB, it_b);

    printf("%-48s %8s %8s %8s %8s\n", "form of B's launch (us, medians of 100 steps)", "A", "B", "A->B", "B->A");
    // wait_back: the next A waits for the side stream's event of two steps ago (a wait packet in front of
    // A; the engine has none in the benchmark's step, whose host waits for that slot's copy first)
    struct Case { const char* name; Form form; unsigned flags; bool wait_back; };
    const unsigned kDev = hipEventDisableSystemFence;
    const Case cases[] = {
        {"plain, nothing on the side", Plain, 0, false},
        {"stop event, default flags", Stop, hipEventDefault, false},
        {"stop event, DisableSystemFence", Stop, kDev, false},
        {"start + stop events, default flags", StartStop, hipEventDefault, false},
        {"start + stop events, DisableSystemFence", StartStop, kDev, false},
        {"record + side stream waits, default flags", Record, hipEventDisableTiming, false},
        {"record + side stream waits, DisableSystemFence", Record, hipEventDisableTiming | kDev, false},
        {"stop event, default; next A waits back", Stop, hipEventDefault, true},
        {"stop event, DisableSystemFence; A waits back", Stop, kDev, true},
    };
    for (const Case& c : cases) {
        hipEvent_t start[2], stop[2], side_done[2];
        for (int k = 0; k < 2; ++k) {
            CK(hipEventCreateWithFlags(&start[k], c.flags & ~hipEventDisableTiming));
            CK(hipEventCreateWithFlags(&stop[k], c.flags));
            CK(hipEventCreateWithFlags(&side_done[k], c.flags | hipEventDisableTiming));
        }
        if (reset_stamps()) return 1;
        for (int k = 0; k < kSteps; ++k) {
            const int p = k & 1;
            if (c.wait_back && k >= 2) CK(hipStreamWaitEvent(s1, side_done[p], 0));
            hipLaunchKernelGGL(k_a, dim3(kGridA), dim3(256), 0, s1, table, out_b, it_a, out_a, &d_st[k].a0, &d_st[k].a1);
            if (c.form == Stop || c.form == StartStop)
                hipExtLaunchKernelGGL(k_b, dim3(kGridB), dim3(256), 0, s1, c.form == StartStop ? start[p] : nullptr, stop[p],
                                      0, (const float*)table, (const float*)out_a, it_b, (int)kUnitsB, out_b, &d_st[k].b0,
                                      &d_st[k].b1);          // (this form takes the kernel's own parameter types)
            else
                hipLaunchKernelGGL(k_b, dim3(kGridB), dim3(256), 0, s1, table, out_a, it_b, kUnitsB, out_b, &d_st[k].b0,
                                   &d_st[k].b1);
            if (c.form == Record) CK(hipEventRecord(stop[p], s1));
            if (c.form != Plain) {
                CK(hipStreamWaitEvent(s2, stop[p], 0));
                hipLaunchKernelGGL(k_side, dim3(64), dim3(64), 0, s2, out_b, side);
                CK(hipEventRecord(side_done[p], s2));
            }
        }
        CK(hipGetLastError());
        if (fetch_stamps()) return 1;
        std::vector<double> da, db, gab, gba;
        for (int k = kSkip; k < kSteps - 1; ++k) {
            da.push_back((st[k].a1 - st[k].a0) * tick_us);
            db.push_back((st[k].b1 - st[k].b0) * tick_us);
            gab.push_back(((double)st[k].b0 - (double)st[k].a1) * tick_us);
            gba.push_back(((double)st[k + 1].a0 - (double)st[k].b1) * tick_us);
        }
        printf("%-48s %8.2f %8.2f %8.2f %8.2f\n", c.name, median(da), median(db), median(gab), median(gba));
        for (int k = 0; k < 2; ++k) { CK(hipEventDestroy(start[k])); CK(hipEventDestroy(stop[k])); CK(hipEventDestroy(side_done[k])); }
    }

    // the consumer: 256 workgroups re-read the table on s1 for ~100 us while, on s2, small kernels
    // each followed by an event record complete
    printf("\n%-48s %8s\n", "consumer re-reading 4 MiB through L2 (us)", "median");
    int rounds = 8;
    for (int pass = 0; pass < 2; ++pass) {
        if (reset_stamps()) return 1;
        for (int k = 0; k < 4; ++k)
            hipLaunchKernelGGL(k_reread, dim3(256), dim3(256), 0, s1, table, rounds, out_a, &d_st[k].a0, &d_st[k].a1);
        if (fetch_stamps()) return 1;
        rounds = rescale(rounds, 100.0, (st[3].a1 - st[3].a0) * tick_us);
    }
    struct Side { const char* name; int events; unsigned flags; };
    const Side sides[] = {
        {"alone", 0, 0},
        {"beside 8 small kernels, no events", -8, 0},
        {"beside 8 events, default flags", 8, hipEventDisableTiming},
        {"beside 8 events, DisableSystemFence", 8, hipEventDisableTiming | hipEventDisableSystemFence},
    };
    for (const Side& sd : sides) {
        hipEvent_t ev;
        CK(hipEventCreateWithFlags(&ev, sd.flags));
        if (reset_stamps()) return 1;
        for (int k = 0; k < 40; ++k) {
            hipLaunchKernelGGL(k_reread, dim3(256), dim3(256), 0, s1, table, rounds, out_a, &d_st[k].a0, &d_st[k].a1);
            for (int e = 0; e < (sd.events < 0 ? -sd.events : sd.events); ++e) {
                hipLaunchKernelGGL(k_side, dim3(64), dim3(64), 0, s2, out_b, side);
                if (sd.events > 0) CK(hipEventRecord(ev, s2));
            }
            CK(hipStreamSynchronize(s1));            // (one consumer at a time; the side stream runs beside it)
            CK(hipStreamSynchronize(s2));
        }
        if (fetch_stamps()) return 1;
        std::vector<double> d;
        for (int k = 8; k < 40; ++k) d.push_back((st[k].a1 - st[k].a0) * tick_us);
        printf("%-48s %8.2f\n", sd.name, median(d));
        CK(hipEventDestroy(ev));
    }
    return 0;
}
