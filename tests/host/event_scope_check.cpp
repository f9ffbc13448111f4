// The classification of the handles' events (csrc/gpsmi_event_scope.h) checked on the CPU, with the
// host compiler alone: every event behind which the host reads device-written memory is host-visible,
// the rows the engine's waits name are classified as the code uses them, and the table is complete.
// A program of its own (tests/test_event_scope_host.py builds and runs it).
#include <cstdio>
#include <cstring>

#include "gpsmi_event_scope.h"

using namespace gpsmi;

static int failures = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) {                                                                \
            fprintf(stderr, "event_scope_check: line %d: %s\n", __LINE__, #cond);     \
            ++failures;                                                               \
        }                                                                             \
    } while (0)

int main() {
    CHECK(kEventClasses == static_cast<int>(Ev::kCount));
    int host_visible = 0;
    for (int k = 0; k < kEventClasses; ++k) {
        const EventClass& c = kEventClass[k];
        CHECK(static_cast<int>(c.which) == k);
        CHECK(c.name && strlen(c.name) > 0);
        // the rule itself
        if (c.host == HostWait::Data) CHECK(c.scope == EventScope::HostVisible);
        // ... and nothing is host-visible without a reader on the host: a fence wider than needed
        if (c.scope == EventScope::HostVisible) CHECK(c.host == HostWait::Data);
        // a stamp the host reads needs an event that records time
        if (c.host == HostWait::Stamps) CHECK(c.stamps);
        host_visible += c.scope == EventScope::HostVisible;
        printf("%-22s %-12s %s\n", c.name, c.scope == EventScope::HostVisible ? "host-visible" : "device-only",
               c.host == HostWait::Data     ? "host reads device-written memory behind it"
               : c.host == HostWait::Stamps ? "host reads its stamp"
               : c.host == HostWait::Reuse  ? "host rewrites memory the device has read"
                                            : "no host wait");
    }
    // what the host synchronises on, by entry point:
    //   gpsmi_trk_wait_prev / replay_fetch: `copied`, then the pinned record array is read
    CHECK(event_class(Ev::TrkCopied).scope == EventScope::HostVisible);
    //   trk_spin_wait in a streamed step and in gpsmi_trk_wait: `in_done` (a step's tail_stop), then a
    //   page-locked `out` the kernels stored into is read
    CHECK(event_class(Ev::TrkInDone).scope == EventScope::HostVisible);
    //   gpsmi_trk_wait_prev with no copy pending: corr_stop (corr_done or ev[2]) or ev[3], stamps alone
    CHECK(event_class(Ev::TrkCorrDone).host == HostWait::Stamps);
    CHECK(event_class(Ev::TrkStamp).host == HostWait::Stamps);
    //   acq_stage: `staged`, then the host REWRITES its own staging arrays
    CHECK(event_class(Ev::AcqStaged).host == HostWait::Reuse);
    CHECK(host_visible == 2);
    if (failures) return 1;
    printf("event_scope_check ok\n");
    return 0;
}
