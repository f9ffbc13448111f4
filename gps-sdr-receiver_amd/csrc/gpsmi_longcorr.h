// LongCorr: the code-phase correlation at code lengths other than 2048 samples, once for the
// acquisition and the tracking handle.  It owns the choice of the method, the replica spectra, the
// cell tables and the statistics; the folded samples it correlates stay with the caller (tracking
// reuses one scratch area piece by piece, acquisition keeps a chunk of bins per call).
//   Pfa     natively in LDS at 16368 = 16 * 3 * 11 * 31 samples (gpsmi_pfa.h): transform, product,
//           transform and statistics in one launch, and the only method with the segmented modes
//   BigFft  zero-padded through one 32768-point FFT pair where the code period fits (gpsmi_bigfft.h)
//   Direct  the exact time-domain kernel (gpsmi_direct.h)
// BigFft and Direct leave magnitudes that corr_stats_kernel reduces; either way a cell ends as one
// DirStats record.
#pragma once
#include <cmath>
#include <cstdio>
#include <vector>

#include "gpsmi_common.h"
#include "gpsmi_devmem.h"
#include "gpsmi_bigfft.h"
#include "gpsmi_pfa.h"
#include "gpsmi_direct.h"

namespace gpsmi {

struct LongCorr {
    enum class Method { Pfa, BigFft, Direct };
    // option "codephase" (gpsmi.h): 0 the native correlation at 16368 and the 32768-point pair where
    // it fits, 1 keeps the time-domain kernel, 2 takes the pair at 16368 too
    static Method choose(int cs, long long option) {
        if (cs == kPfaL && option == 0) return Method::Pfa;
        return 2 * cs - 1 <= kBigN && option != 1 ? Method::BigFft : Method::Direct;
    }
    Method method = Method::Direct;
    int cs = 0;
    DevBuf<float2> d_twN, d_RS, d_S;        // BigFft: 32768-point twiddles, [GPSMI_MAX_PRN + 1][32768] replica
                                            // spectra, the scratch of one chunk of cells
    DevBuf<float2> d_RSp;                   // Pfa: [GPSMI_MAX_PRN + 1][16368] replica spectra, P3's order
    DevBuf<float> d_mag;                    // [cells][cs], not with Pfa
    DevBuf<DirStats> d_stats;               // [cells], as d_xsel (row of the folded samples) and d_rsel (replica slot)
    DevBuf<int> d_xsel, d_rsel;
    char what[64] = "";                     // the allocation labels: "<owner> <buffer>"
    const char* owner = "";
    const char* label(const char* buffer) { return snprintf(what, sizeof(what), "%s %s", owner, buffer), what; }

    bool pfa() const { return method == Method::Pfa; }
    // the value of option "codephase" that names what runs
    int option() const { return pfa() ? 0 : method == Method::BigFft ? 2 : 1; }

    // the method from (cs, default of "codephase"), the twiddles and the replica spectra: zeroed, for
    // tracking's slot 0 (closed channels).  `owner_name`: "gpsmi_acq" / "gpsmi_trk"
    int build(int code_samples, const char* owner_name) {
        cs = code_samples, owner = owner_name;
        long long option = 0;
        default_opt("codephase", &option, 0);
        method = choose(cs, option);
        const size_t slots = GPSMI_MAX_PRN + 1;
        if (pfa()) return d_RSp.reserve_zeroed(slots * kPfaL, label("replica spectra"));
        if (method != Method::BigFft) return GPSMI_OK;
        std::vector<float2> twn(kBigN);
        for (int k = 0; k < kBigN; ++k) {
            const double a = -2.0 * M_PI * (double)k / (double)kBigN;
            twn[k] = make_float2((float)cos(a), (float)sin(a));
        }
        int rc = d_twN.upload(twn, label("twiddles"));
        if (!rc) rc = d_RS.reserve_zeroed(slots * kBigN, label("replica spectra"));
        if (!rc) rc = d_S.reserve((size_t)kBigChunkCells * kBigN, label("correlation scratch"));
        return rc;
    }
    // the spectrum of replica `prn` of d_time [slots][cs] (d_tw: the 2048-point twiddles), complete on return
    int set_replica(hipStream_t stream, const float* d_time, int prn, const float2* d_tw) {
        if (method == Method::Direct) return GPSMI_OK;
        if (pfa()) pfa_replica_launch(stream, d_time, prn, d_RSp.p);
        else big_replica_launch(stream, d_time, prn, cs, d_RS.p, d_tw, d_twN.p);
        GPSMI_HIP(hipGetLastError());
        GPSMI_HIP(hipStreamSynchronize(stream));
        return GPSMI_OK;
    }
    // tables and statistics of `cells` cells
    int reserve(size_t cells) {
        int rc = d_stats.reserve(cells, label("cell statistics"));
        if (!rc) rc = d_xsel.reserve(cells, label("cell table"));
        if (!rc) rc = d_rsel.reserve(cells, label("cell table"));
        if (!rc && !pfa()) rc = d_mag.reserve(cells * cs, label("magnitudes"));
        return rc;
    }

    // Cells cell0 .. cell0 + ncell - 1 of the tables on `stream`: folded rows x [d_xsel[cell]][cs] against
    // replica d_rsel[cell] (d_time and d_tw as in set_replica) into d_stats.  A piece of a launch is as
    // good as the whole: tracking folds and correlates piece by piece.  MODE 2 (non-coherent), 3 (deep)
    // and 4 (deep, the surfaces kept in `rows`) are gpsmi_pfa.h's, with Pfa only (acq_check_search
    // refuses the others): x is then [d_xsel[cell]][nseg][cs], and MODE 3 / 4 add `shift`, the lag
    // rotation of every (row, segment).
    template <int MODE = 0>
    void correlate(hipStream_t stream, const float2* x, int cell0, int ncell, const float* d_time, const float2* d_tw,
                   int nseg = 1, const int* shift = nullptr, PfaRows rows = PfaRows{nullptr, 1, 0, 0}) {
        const int *xsel = d_xsel.p + cell0, *rsel = d_rsel.p + cell0;
        DirStats* stats = d_stats.p + cell0;
        if (pfa() && MODE == 0)          // (its kernel takes the first cell beside the tables)
            return pfa_corr_launch<0>(stream, x, d_xsel.p, d_rsel.p, ncell, d_RSp.p, d_stats.p, cell0);
        if (pfa()) return pfa_corr_launch<MODE>(stream, x, xsel, rsel, ncell, d_RSp.p, stats, nseg, shift, rows);
        float* mag = d_mag.p + (size_t)cell0 * cs;
        if (method == Method::BigFft)
            big_corr_launch(stream, x, xsel, rsel, ncell, cs, d_RS.p, d_S.p, d_tw, d_twN.p, mag);
        else
            hipLaunchKernelGGL(circ_corr_direct_kernel, dim3((cs + kDirLagsPerWg - 1) / kDirLagsPerWg, ncell),
                               dim3(256), 0, stream, x, d_time, xsel, rsel, cs, mag);
        hipLaunchKernelGGL(corr_stats_kernel, dim3(ncell), dim3(256), 0, stream, mag, cs, stats);
    }
};

}  // namespace gpsmi
