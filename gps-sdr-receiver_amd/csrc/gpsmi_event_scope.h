// The scope of every event a handle creates (DESIGN.md section 4.6 has the same table in words).
//
// An event made with the runtime's default flags performs a SYSTEM-scope release when it completes:
// the device's caches are written back and invalidated so that the host may inspect memory.  Only an
// event behind which the host reads what the device wrote, with no copy command of its own in
// between, needs that.  Every other event orders device work against device work, or carries a time
// stamp, and is made device-only (hipEventDisableSystemFence): its completion leaves the caches
// alone, which the kernel running beside it on another queue is reading.
//
// No runtime header in here: tests/host/event_scope_check.cpp compiles this file with the host
// compiler alone.
#pragma once

namespace gpsmi {

enum class EventScope { HostVisible, DeviceOnly };

// What the host does behind a wait on the event (hipEventSynchronize, hipEventQuery, trk_spin_wait).
enum class HostWait {
    None,      // the host never waits on it: it feeds hipStreamWaitEvent, or its stamp is read behind a
               // stream synchronisation
    Stamps,    // ... reads the event's own time stamp and nothing else
    Reuse,     // ... rewrites page-locked memory of its own that the device has finished READING
    Data,      // ... reads memory the device wrote, with no copy command between the writer and the event
};

enum class Ev {
    TrkStamp,        // gpsmi_trk::Slot::ev[0..3]
    TrkReady,        // Slot::ready
    TrkCopied,       // Slot::copied
    TrkCorrDone,     // Slot::corr_done (also Slot::corr_stop)
    TrkEpiDone,      // Slot::epi_done
    TrkOrder,        // gpsmi_trk::order
    TrkUpDone,       // gpsmi_trk::up_done[2]
    TrkStageFree,    // gpsmi_trk::stage_free[2]
    TrkInDone,       // gpsmi_trk::in_done[2] (a streamed step's tail_stop)
    AcqStamp,        // gpsmi_acq::ev0, ev1
    AcqOrder,        // gpsmi_acq::order
    AcqStaged,       // gpsmi_acq::staged[2]
    StageStamp,      // StageSync::ev0, ev1 (the conditioning handles)
    kCount
};

struct EventClass {
    Ev which;
    const char* name;
    EventScope scope;
    bool stamps;         // the event records time (else hipEventDisableTiming)
    HostWait host;
};

// One row per event, in the order of Ev.
constexpr EventClass kEventClass[] = {
    {Ev::TrkStamp, "trk.slot.ev[0..3]", EventScope::DeviceOnly, true, HostWait::Stamps},
    {Ev::TrkReady, "trk.slot.ready", EventScope::DeviceOnly, false, HostWait::None},
    {Ev::TrkCopied, "trk.slot.copied", EventScope::HostVisible, false, HostWait::Data},
    {Ev::TrkCorrDone, "trk.slot.corr_done", EventScope::DeviceOnly, true, HostWait::Stamps},
    {Ev::TrkEpiDone, "trk.slot.epi_done", EventScope::DeviceOnly, false, HostWait::None},
    {Ev::TrkOrder, "trk.order", EventScope::DeviceOnly, false, HostWait::None},
    {Ev::TrkUpDone, "trk.up_done", EventScope::DeviceOnly, false, HostWait::None},
    {Ev::TrkStageFree, "trk.stage_free", EventScope::DeviceOnly, false, HostWait::None},
    {Ev::TrkInDone, "trk.in_done", EventScope::HostVisible, true, HostWait::Data},
    {Ev::AcqStamp, "acq.ev0/ev1", EventScope::DeviceOnly, true, HostWait::None},
    {Ev::AcqOrder, "acq.order", EventScope::DeviceOnly, false, HostWait::None},
    {Ev::AcqStaged, "acq.staged", EventScope::DeviceOnly, false, HostWait::Reuse},
    {Ev::StageStamp, "stage.ev0/ev1", EventScope::DeviceOnly, true, HostWait::None},
};

constexpr int kEventClasses = sizeof(kEventClass) / sizeof(kEventClass[0]);

constexpr const EventClass& event_class(Ev e) { return kEventClass[static_cast<int>(e)]; }

// The rule: the host reads device-written memory only behind a host-visible event.
constexpr bool event_class_sound(const EventClass& c) {
    return c.host != HostWait::Data || c.scope == EventScope::HostVisible;
}
constexpr bool event_classes_sound() {
    if (kEventClasses != static_cast<int>(Ev::kCount)) return false;
    for (int k = 0; k < kEventClasses; ++k)
        if (static_cast<int>(kEventClass[k].which) != k || !event_class_sound(kEventClass[k])) return false;
    return true;
}
static_assert(event_classes_sound(), "an event the host reads device-written memory behind must be host-visible");

}  // namespace gpsmi
