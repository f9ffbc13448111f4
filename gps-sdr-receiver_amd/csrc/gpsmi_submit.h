// SubmitQueue: the submission thread behind gpsmi_trk_process_stream, as a host-only type (no GPU
// header: tests/host/submit_check.cpp runs it under ThreadSanitizer and AddressSanitizer).
//
// One thread (the handle's caller) calls start / submit / quiesce / stop, one at a time; the queue's
// own thread runs `step` for each job in submission order and nothing else touches what the step
// works on -- so after quiesce() the caller is the only thread working on the handle.
//
// A failed step: the first failure is kept, the jobs queued behind it are not run (they still count
// as finished and cleared), and the NEXT submit or quiesce returns its code once, with the text
// "a streamed step failed: ...", without queueing anything; after that the queue works as before.
#pragma once
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstddef>
#include <cstdio>
#include <deque>
#include <mutex>
#include <thread>

namespace gpsmi {

class SubmitQueue {
public:
    struct Job { const void* iq; size_t n; void* out; };
    static constexpr size_t kErrText = 512;      // room for a step's error text
    static constexpr size_t kReport = kErrText + 32;   // ... and for the report made of it
    // One step.  It calls q.step_cleared() once the step before last is known to be complete, and on
    // failure returns non-zero with its reason in errtext[kErrText].
    using Step = int (*)(void* ctx, const Job& job, SubmitQueue& q, char* errtext);

    SubmitQueue(Step step, void* ctx) : step_(step), ctx_(ctx) {}
    ~SubmitQueue() { stop(); }
    SubmitQueue(const SubmitQueue&) = delete;
    SubmitQueue& operator=(const SubmitQueue&) = delete;

    bool running() const { return th_.joinable(); }

    // -> false when no thread is to be had (the caller then runs its steps itself)
    bool start() {
        try {
            th_ = std::thread([this] { run(); });
        } catch (...) {                          // (nothing may be thrown across the C ABI)
            return false;
        }
        return true;
    }

    // the jobs still queued are run, then the thread ends
    void stop() {
        if (!running()) return;
        {
            std::lock_guard<std::mutex> lock(m_);
            stop_ = true;
        }
        cv_job_.notify_all();
        th_.join();
        stop_ = false;
    }

    // Hand over job k (counted from 1) and return once cleared >= k - (depth - 2): at depth 2 the step
    // before last is complete, at depth 3 the one before that.  -> 0, or a kept failure (report[kReport]).
    int submit(const Job& job, int depth, char* report) {
        std::unique_lock<std::mutex> lock(m_);
        if (err_) {                              // an earlier step failed: report it instead of queueing more
            cv_done_.wait(lock, [&] { return finished_ == submitted_; });
            return take_error(report);
        }
        q_.push_back(job);
        const long long k = submitted_ + 1;
        set_submitted(k);
        cv_job_.notify_one();
        const long long need = k - (depth - 2);
        if (cleared_ < need) {
            lock.unlock();
            spin_until([&] { return cleared() >= need; }, kSubmitSpinUs);
            lock.lock();
        }
        cv_done_.wait(lock, [&] { return cleared_ >= need; });
        return 0;
    }

    // Nothing is queued and the thread is idle.  -> 0, or a kept failure (report[kReport], may be null).
    int quiesce(char* report) {
        if (!running()) return 0;
        spin_until([&] { return finished() == a_submitted_.load(std::memory_order_relaxed); }, kQuiesceSpinUs);
        std::unique_lock<std::mutex> lock(m_);
        cv_done_.wait(lock, [&] { return finished_ == submitted_; });
        return err_ ? take_error(report) : 0;
    }

    // from the step, on the queue's thread: the caller of the job in hand may go on
    void step_cleared() {
        {
            std::lock_guard<std::mutex> lock(m_);
            set_cleared(finished_ + 1);
        }
        cv_done_.notify_all();
    }

    // The counters as any thread may POLL them: jobs handed over, jobs whose caller may go on, jobs
    // fully run.  Neither of the latter two is ever seen ahead of `submitted` read after it.
    long long submitted() const { return a_submitted_.load(std::memory_order_acquire); }
    long long cleared() const { return a_cleared_.load(std::memory_order_acquire); }
    long long finished() const { return a_finished_.load(std::memory_order_acquire); }

private:
    // Being woken from a futex measured 50-100 us on the hosts this was tuned on (three hand-overs per
    // report block made gpsmi_trk_wait 290 us where the work outstanding was 60 us), so each side polls
    // the other's counter for a while before it sleeps on its condition variable.
    static constexpr int kSubmitSpinUs = 300, kJobSpinUs = 300, kQuiesceSpinUs = 1000;

    template <class F>
    static void spin_until(F&& done, int us) {
        const auto t0 = std::chrono::steady_clock::now();
        while (!done()) {
            if (std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(us)) return;
            __builtin_ia32_pause();
        }
    }

    // each counter and its polled mirror change here and nowhere else (m_ held)
    void set_submitted(long long v) { submitted_ = v; a_submitted_.store(v, std::memory_order_release); }
    void set_cleared(long long v) { cleared_ = v; a_cleared_.store(v, std::memory_order_release); }
    void set_finished(long long v) { finished_ = v; a_finished_.store(v, std::memory_order_release); }

    // the kept failure, once (m_ held)
    int take_error(char* report) {
        const int rc = err_;
        err_ = 0;
        if (report) snprintf(report, kReport, "a streamed step failed: %s", errmsg_);
        return rc;
    }

    void run() {
        for (;;) {
            Job job;
            int rc;
            spin_until([&] { return submitted() > a_finished_.load(std::memory_order_relaxed); }, kJobSpinUs);
            {
                std::unique_lock<std::mutex> lock(m_);
                cv_job_.wait(lock, [&] { return stop_ || !q_.empty(); });
                if (q_.empty()) return;          // (stop, and nothing left to run)
                job = q_.front();
                rc = err_;                       // behind a failure nothing more is run
            }
            char text[kErrText] = "";
            if (!rc) rc = step_(ctx_, job, *this, text);
            {
                std::lock_guard<std::mutex> lock(m_);
                if (rc && !err_) {               // the first failure is kept for the caller
                    err_ = rc;
                    snprintf(errmsg_, sizeof(errmsg_), "%s", text);
                }
                q_.pop_front();
                if (cleared_ < finished_ + 1) set_cleared(finished_ + 1);
                set_finished(finished_ + 1);
            }
            cv_done_.notify_all();
        }
    }

    const Step step_;
    void* const ctx_;
    std::thread th_;
    std::mutex m_;
    std::condition_variable cv_job_, cv_done_;
    std::deque<Job> q_;
    bool stop_ = false;
    long long submitted_ = 0, cleared_ = 0, finished_ = 0;
    std::atomic<long long> a_submitted_{0}, a_cleared_{0}, a_finished_{0};
    int err_ = 0;
    char errmsg_[kErrText] = "";
};

}  // namespace gpsmi
