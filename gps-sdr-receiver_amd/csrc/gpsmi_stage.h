// The host skeleton of a conditioning handle (gpsmi_fe, gpsmi_ifx, gpsmi_pb, gpsmi_nul): the
// stream and the timing events, create / destroy, and for the block filters the input format, the
// staged host entry and the argument checks of a call.  The kernels and what a handle computes stay
// in its own file.
#pragma once
#include <new>

#include "gpsmi_common.h"
#include "gpsmi_devmem.h"

namespace gpsmi {

// The stream of a handle and the two events that time a call on it.  Every handle holds one as its
// LAST member (`sync`): members are released bottom up, so the events go first, then the stream, and
// only then the device buffers declared above it that work on the stream may still touch.  (Not a
// base class: a base is destroyed after the members of the derived struct.)
struct StageSync {
    DevStream stream;
    DevEvent ev0, ev1;
    float last_ms = 0.f;                     // device time of the last finished call

    int create() {
        int rc = stream.create();
        // (stamps alone, read behind finish()'s stream synchronisation)
        if (!rc) rc = ev0.create<Ev::StageStamp, EventScope::DeviceOnly>();
        if (!rc) rc = ev1.create<Ev::StageStamp, EventScope::DeviceOnly>();
        return rc;
    }
    int begin() {                            // ahead of a call's first launch
        GPSMI_HIP(hipEventRecord(ev0, stream));
        return GPSMI_OK;
    }
    int end() {                              // behind its last one
        GPSMI_HIP(hipGetLastError());
        GPSMI_HIP(hipEventRecord(ev1, stream));
        return GPSMI_OK;
    }
    int finish() {                           // the call is complete, last_ms is its device time
        GPSMI_HIP(hipStreamSynchronize(stream));
        GPSMI_HIP(hipEventElapsedTime(&last_ms, ev0, ev1));
        return GPSMI_OK;
    }
};

// H: a handle struct with `cfg` (a device in it) and `StageSync sync`.
template <typename H>
int stage_destroy(H* h) {
    if (!h) return GPSMI_OK;
    (void)hipSetDevice(h->cfg.device);
    if (h->sync.stream) (void)hipStreamSynchronize(h->sync.stream);
    delete h;                                // (events, stream, device buffers: see StageSync)
    return GPSMI_OK;
}

// After the caller's own argument checks: a handle with cfg copied and stream and events made, then
// build(h) for everything else; a failure leaves nothing behind.
template <typename H, typename Cfg, typename Build>
int stage_create(const Cfg* cfg, H** out, Build&& build) {
    GPSMI_HIP(hipSetDevice(cfg->device));
    H* h = new (std::nothrow) H();
    if (!h) return fail(GPSMI_E_NOMEM, "out of host memory");
    h->cfg = *cfg;
    int rc = h->sync.create();
    if (!rc) rc = build(h);
    if (rc) {
        (void)stage_destroy(h);
        return rc;
    }
    *out = h;
    return GPSMI_OK;
}

template <typename H>
int stage_last_ms(const H* h, float* ms, const char* fn) {
    if (!h || !ms) return fail(GPSMI_E_ARG, "%s: null argument", fn);
    *ms = h->sync.last_ms;
    return GPSMI_OK;
}

// Device copies of the input and the output of a host entry point that works block by block
// (gpsmi_pb_apply, gpsmi_ifx_apply): room for both, then the input on its way up on `stream`.
struct StagedIO {
    DevBuf<char> in, out;
    int upload(const void* src, size_t in_bytes, size_t out_bytes, hipStream_t stream, const char* what) {
        int rc = in.reserve(in_bytes, what);
        if (!rc) rc = out.reserve(out_bytes, what);
        if (rc) return rc;
        GPSMI_HIP(hipMemcpyAsync(in.p, src, in_bytes, hipMemcpyHostToDevice, stream));
        return GPSMI_OK;
    }
};

// What the block filters (`blk` of gpsmi_ifx, gpsmi_pb and gpsmi_nul) share: blocks of block_samples
// samples in one of two input formats, complex64 out.  fan_in: input blocks per output block (the
// antennas of gpsmi_nul).
struct BlockStage {
    int block_samples = 0;
    int fmt = GPSMI_IQ_C64;
    int fan_in = 1;
    StagedIO io;                             // host entry: staged input and output

    size_t in_bytes(int nb) const {
        return (size_t)nb * block_samples * fan_in * (fmt == GPSMI_IQ_U8 ? sizeof(uint16_t) : sizeof(float2));
    }
    size_t out_bytes(int nb) const { return (size_t)nb * block_samples * sizeof(float2); }

    // The host entry: upload, run(d_in, d_out) on the staged buffers, the ob bytes of output (out_bytes(nb)
    // per output row of the call) on their way down, finish() (the handle's result copies and
    // StageSync::finish).
    template <typename Run, typename Finish>
    int apply_host(const void* iq, void* out, int nb, size_t ob, hipStream_t stream, const char* what, Run&& run,
                   Finish&& finish) {
        int rc = io.upload(iq, in_bytes(nb), ob, stream, what);
        if (!rc) rc = run(static_cast<const void*>(io.in.p), static_cast<void*>(io.out.p));
        if (rc) return rc;
        GPSMI_HIP(hipMemcpyAsync(out, io.out.p, ob, hipMemcpyDeviceToHost, stream));
        return finish();
    }
};

// What every call on nb blocks checks first: the pointers, and nb against the samples a call may hold.
template <typename H>
int stage_check_blocks(const H* h, const void* iq, const void* out, int nb, const char* fn) {
    if (!h || !iq || !out) return fail(GPSMI_E_ARG, "%s: null argument", fn);
    if (nb < 1 || (size_t)nb * h->blk.block_samples > ((size_t)1 << 31))
        return fail(GPSMI_E_ARG, "%s: nb out of range: 1 .. 2^31 samples per call", fn);
    return GPSMI_OK;
}

// Device pointers as the kernels read them: 4-byte (u8) / 16-byte (complex64) words in, 16-byte words out.
inline bool stage_aligned(const BlockStage& b, const void* iq, const void* out) {
    return (uintptr_t)iq % (b.fmt == GPSMI_IQ_U8 ? 4 : 16) == 0 && (uintptr_t)out % 16 == 0;
}

// The argument checks of a call on nb blocks, before any GPU work.  no_overlap: the filter's name
// when input and output must not overlap (the output of one block is made of the input of the block
// before it), null where that is not checked; aligned: the pointers are device pointers that the
// kernels read as 4-byte (u8) / 16-byte (complex64) words.
template <typename H>
int stage_check_call(const H* h, const void* iq, const void* out, int nb, const char* fn, const char* no_overlap,
                     bool aligned) {
    const int rc = stage_check_blocks(h, iq, out, nb, fn);
    if (rc) return rc;
    const BlockStage& b = h->blk;
    const char* i0 = static_cast<const char*>(iq);
    const char* o0 = static_cast<const char*>(out);
    if (no_overlap && !(o0 + b.out_bytes(nb) <= i0 || i0 + b.in_bytes(nb) <= o0))
        return fail(GPSMI_E_ARG, "%s: input and output overlap (no in-place %s)", fn, no_overlap);
    if (aligned && !stage_aligned(b, iq, out))
        return fail(GPSMI_E_ARG, "%s: device input / output not aligned (4 bytes for u8, 16 for complex64)", fn);
    return GPSMI_OK;
}

template <typename H>
int stage_set_input_format(H* h, int fmt, const char* fn) {
    if (!h) return fail(GPSMI_E_ARG, "%s: null handle", fn);
    if (fmt != GPSMI_IQ_C64 && fmt != GPSMI_IQ_U8) return fail(GPSMI_E_ARG, "%s: unknown input format", fn);
    GPSMI_HIP(hipSetDevice(h->cfg.device));
    GPSMI_HIP(hipStreamSynchronize(h->sync.stream));
    h->blk.fmt = fmt;
    return GPSMI_OK;
}

}  // namespace gpsmi
