// Host check of gpsmi::SubmitQueue (csrc/gpsmi_submit.h), the submission thread behind
// gpsmi_trk_process_stream, with a stub in place of the streamed step.  No GPU, no library: built
// with -fsanitize=thread and with -fsanitize=address,undefined by tests/test_submit_host.py, which
// runs it and reads its exit status.  Any violation prints a line and ends the program with 1.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "gpsmi_submit.h"

using gpsmi::SubmitQueue;

#define CHECK(cond, ...)                                    \
    do {                                                    \
        if (!(cond)) {                                      \
            fprintf(stderr, "submit_check: %s:%d: ", __func__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);                   \
            fprintf(stderr, "\n");                          \
            exit(1);                                        \
        }                                                   \
    } while (0)

namespace {

constexpr int kStubErr = -7;

// The stub step: job.n is the job's ordinal.  It notes the order, idles for a pseudo-random
// 0-50 us (fixed seed) on either side of the cleared notification, and fails when asked to.
struct Stub {
    std::vector<long long> ran;              // the queue's thread writes, the caller reads after quiesce / stop
    std::atomic<long long> passed{0};        // ordinal of the latest job that gave its cleared notification
    unsigned rng = 12345u;
    long long fail_at = 0;                   // this job fails (before its cleared notification) ...
    long long fail_once_submitted = 0;       // ... once this many jobs have been handed over

    void idle() {
        rng = rng * 1664525u + 1013904223u;
        const unsigned us = (rng >> 16) % 51;
        if (us % 4 == 0) { std::this_thread::yield(); return; }
        if (us % 4 == 1) { std::this_thread::sleep_for(std::chrono::microseconds(us)); return; }
        const auto t0 = std::chrono::steady_clock::now();
        while (std::chrono::steady_clock::now() - t0 < std::chrono::microseconds(us)) {}
    }

    static int step(void* ctx, const SubmitQueue::Job& job, SubmitQueue& q, char* errtext) {
        Stub& s = *static_cast<Stub*>(ctx);
        const long long k = (long long)job.n;
        s.ran.push_back(k);
        s.idle();
        if (k == s.fail_at) {
            while (q.submitted() < s.fail_once_submitted) std::this_thread::yield();
            snprintf(errtext, SubmitQueue::kErrText, "stub step %lld said no", k);
            return kStubErr;
        }
        s.passed.store(k, std::memory_order_release);
        q.step_cleared();
        s.idle();
        return 0;
    }
};

SubmitQueue::Job job_of(long long k) { return SubmitQueue::Job{nullptr, (size_t)k, nullptr}; }

void expect_order(const Stub& s, long long first, long long last) {
    CHECK((long long)s.ran.size() == last - first + 1, "%zu jobs ran, expected %lld", s.ran.size(), last - first + 1);
    for (size_t i = 0; i < s.ran.size(); ++i)
        CHECK(s.ran[i] == first + (long long)i, "job %lld ran in place %zu", s.ran[i], i);
}

// a few thousand jobs at one depth: the depth contract at every return, every job once and in order,
// quiesce after the burst; beside it a thread that only polls the counters
void depth_contract(int depth, long long njobs) {
    Stub s;
    SubmitQueue q(Stub::step, &s);
    CHECK(q.start(), "no thread");
    std::atomic<bool> done{false};
    std::thread poller([&] {
        while (!done.load(std::memory_order_acquire)) {
            const long long f = q.finished(), c = q.cleared(), sub = q.submitted();
            if (c > sub || f > sub || f > c) {
                fprintf(stderr, "submit_check: polled finished %lld, cleared %lld, then submitted %lld\n", f, c, sub);
                exit(1);
            }
        }
    });
    char report[SubmitQueue::kReport];
    for (long long k = 1; k <= njobs; ++k) {
        CHECK(q.submit(job_of(k), depth, report) == 0, "submit %lld failed: %s", k, report);
        const long long need = k - (depth - 2);
        CHECK(q.cleared() >= need, "depth %d: submit %lld returned with cleared = %lld", depth, k, q.cleared());
        CHECK(s.passed.load(std::memory_order_acquire) >= need, "depth %d: submit %lld returned before step %lld cleared",
              depth, k, need);
        CHECK(q.submitted() == k, "submitted = %lld after job %lld", q.submitted(), k);
    }
    CHECK(q.quiesce(report) == 0, "quiesce failed: %s", report);
    CHECK(q.finished() == njobs && q.submitted() == njobs && q.cleared() == njobs, "counters %lld / %lld / %lld after %lld jobs",
          q.submitted(), q.cleared(), q.finished(), njobs);
    done.store(true, std::memory_order_release);
    poller.join();
    q.stop();
    expect_order(s, 1, njobs);
}

// Step j fails with j + 1 and j + 2 already handed over: they are not run but counted, the call that
// handed them over returned 0 (the failure surfaces one call late: pinned here so that a change of it
// is deliberate), the next submit or quiesce reports it once with the step's text, and the queue
// then works as before.
void failing_step(bool surfaces_at_submit) {
    constexpr long long j = 40;
    constexpr int depth = 4;                 // (lets the caller run two jobs ahead of the failing one)
    Stub s;
    s.fail_at = j;
    s.fail_once_submitted = j + 2;
    SubmitQueue q(Stub::step, &s);
    CHECK(q.start(), "no thread");
    char report[SubmitQueue::kReport] = "";
    for (long long k = 1; k <= j + 2; ++k)
        CHECK(q.submit(job_of(k), depth, report) == 0, "submit %lld reported a failure early: %s", k, report);
    const char* want = "a streamed step failed: stub step 40 said no";
    if (surfaces_at_submit) {
        CHECK(q.submit(job_of(j + 3), depth, report) == kStubErr, "the submit after a failed step returned 0");
        CHECK(!strcmp(report, want), "report '%s'", report);
        CHECK(q.submitted() == j + 2, "the reporting submit queued its job");
        CHECK(q.quiesce(report) == 0, "the failure was reported twice: %s", report);
    } else {
        CHECK(q.quiesce(report) == kStubErr, "the quiesce after a failed step returned 0");
        CHECK(!strcmp(report, want), "report '%s'", report);
        CHECK(q.quiesce(nullptr) == 0, "the failure was reported twice");
    }
    CHECK(q.finished() == j + 2 && q.cleared() == j + 2, "skipped jobs not counted: cleared %lld, finished %lld", q.cleared(),
          q.finished());
    expect_order(s, 1, j);                   // (j + 1 and j + 2 never reached the step)
    s.ran.clear();
    s.fail_at = 0;
    for (long long k = j + 3; k <= j + 300; ++k)
        CHECK(q.submit(job_of(k), 2, report) == 0, "submit %lld after the report failed: %s", k, report);
    CHECK(q.quiesce(report) == 0, "quiesce after the report failed: %s", report);
    expect_order(s, j + 3, j + 300);
}

// stop with work outstanding (it is run first), stop when idle, stop without a start; many times over
void start_and_stop() {
    for (int round = 0; round < 200; ++round) {
        Stub s;
        long long n = 0;
        {
            SubmitQueue q(Stub::step, &s);
            if (round % 4 == 3) continue;    // never started
            CHECK(q.start(), "no thread");
            char report[SubmitQueue::kReport];
            n = round % 4 == 0 ? 0 : 1 + round % 7;
            for (long long k = 1; k <= n; ++k)       // (depth 64: the calls return with the jobs still queued)
                CHECK(q.submit(job_of(k), 64, report) == 0, "submit %lld failed: %s", k, report);
            if (round % 2) q.stop();                 // else the destructor stops it
            if (round % 2) CHECK(q.finished() == n && !q.running(), "stop left %lld of %lld jobs", n - q.finished(), n);
        }
        expect_order(s, 1, n);
    }
}

}  // namespace

int main() {
    depth_contract(2, 3000);
    depth_contract(3, 3000);
    failing_step(true);
    failing_step(false);
    start_and_stop();
    printf("submit_check ok\n");
    return 0;
}
