// The window rule (csrc/gpsmi_windows.h) as a program of its own, for tests/test_windows_host.py: no
// GPU header, built with the host compiler under AddressSanitizer + UBSan.  It prints what the header
// makes of the cases on its command line, one line per case; the test compares the lines with the
// numpy restatements (sig_ref.py, profile_ref.py, cancel_ref.py).  Numbers that are float64 come as
// hexadecimal floats, so that the program sees the bits the test has.
//
//   starts cs n f_hz tau carrier_hz f_offset_hz guard skip cap   the record's checks, then win_starts
//   edges  cs n f_hz tau carrier_hz f_offset_hz k0 count         ceil and rint of win_edge, k0 .. k0 + count - 1
//   pad    per                                                   win_pad over the `starts` cases so far
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "gpsmi_windows.h"

static char g_error[512];

namespace gpsmi {
int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
    return code;
}
}  // namespace gpsmi

using namespace gpsmi;

// the checks every stage runs ahead of its windows -> Tc; a refusal is printed
static bool record(char** a, int* cs, double* Tc) {
    WinCall w{"windows_check"};
    unsigned long long inc;
    *cs = atoi(a[0]);
    int rc = win_cfg(w, strtod(a[4], nullptr), strtod(a[5], nullptr));
    if (!rc) rc = win_code(w, *cs);
    if (!rc) rc = win_record(w, 1, nullptr, strtod(a[2], nullptr), strtod(a[3], nullptr), Tc, &inc);
    if (rc) printf("refused %d %s\n", rc, g_error);
    return rc == GPSMI_OK;
}

int main(int argc, char** argv) {
    std::vector<std::vector<long long>> all;
    for (int i = 1; i < argc;) {
        const int left = argc - i - 1;
        int cs;
        double Tc;
        if (!strcmp(argv[i], "starts") && left >= 9) {
            char** a = argv + i + 1;
            i += 10;
            if (!record(a, &cs, &Tc)) continue;
            std::vector<long long> out;
            win_starts(strtod(a[3], nullptr), Tc, cs, (size_t)atoll(a[1]), atoi(a[6]), atoi(a[7]), atoll(a[8]), out);
            printf("starts");
            for (long long j : out) printf(" %lld", j);
            printf("\n");
            all.push_back(out);
        } else if (!strcmp(argv[i], "edges") && left >= 8) {
            char** a = argv + i + 1;
            i += 9;
            if (!record(a, &cs, &Tc)) continue;
            printf("edges");
            for (long long k = atoll(a[6]), end = k + atoll(a[7]); k < end; ++k) {
                const double e = win_edge(strtod(a[3], nullptr), Tc, k);
                printf(" %lld %lld", (long long)std::ceil(e), (long long)std::nearbyint(e));
            }
            printf("\n");
        } else if (!strcmp(argv[i], "pad") && left >= 1) {
            const int per = atoi(argv[i + 1]);
            i += 2;
            WinTable t;
            for (const auto& w : all) t.recs.push_back(WinRec{0ull, 1, (int)(w.size() / (size_t)per)});
            const int most = win_pad(all, per, t);
            printf("pad %d", most);
            for (long long j : t.start) printf(" %lld", j);
            printf("\n");
        } else {
            fprintf(stderr, "windows_check: bad case at argument %d\n", i);
            return 2;
        }
    }
    printf("windows_check ok\n");
    return 0;
}
