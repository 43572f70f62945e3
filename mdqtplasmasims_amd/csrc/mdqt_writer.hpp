// Output files of the reference program (SpeedUp:725-1032, `%lg` text) written off the time loop.
//
// The reference formats every number with fprintf("%lg") on the simulation thread, so at the
// reference cadence (output() every sampleFreq MD steps, writeConditions at the end) text
// formatting is most of an MD interval at N = 3.5k.  Here:
//   * LgText (mdqt_lgtext.hpp) formats with std::to_chars(general, precision 6), which is specified to produce
//     exactly printf("%.6g") in the C locale (= "%lg") — same bytes, several times faster; non-
//     finite values go through snprintf so "inf"/"-nan" spellings stay glibc's;
//   * FileWriter formats and writes whole files on a few background threads from snapshots the
//     caller hands over, so the device keeps stepping while the text is produced (SURVEY §8(f)1,
//     "async writers").  flush() is the only join point: the engine calls it before anything
//     reads the files back (readConditions), at the end of mdqt_run and in mdqt_destroy, and
//     reports the first I/O error there.  A writer made with a cap holds at most that many
//     submitted-but-unwritten files: submit() blocks at the cap, so the snapshots in flight stay
//     bounded however far the caller runs ahead (the QT tagging programs' recorded stage: one
//     4,001-row file per job and step).  Without a cap (the default) submit() never blocks.
#pragma once

#include <cerrno>
#include <charconv>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <deque>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "mdqt_lgtext.hpp"

namespace mdqt {

class FileWriter {
  public:
    using Fill = std::function<void(LgText&)>;

    // cap: the most files submitted and not yet written (queued or being written); 0 = no limit
    explicit FileWriter(int threads = 4, size_t cap = 0) : cap_(cap) {
        if (threads < 1) threads = 1;
        for (int i = 0; i < threads; ++i) pool_.emplace_back([this] { loop(); });
    }
    ~FileWriter() {
        flush(nullptr);
        {
            std::lock_guard<std::mutex> g(m_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto& t : pool_) t.join();
    }
    FileWriter(const FileWriter&) = delete;
    FileWriter& operator=(const FileWriter&) = delete;

    // format and write `path` (mode "w" or "a") on a pool thread; `fill` owns its data.  With a cap,
    // waits until fewer than `cap` files are unwritten
    void submit(std::string path, const char* mode, Fill fill) {
        {
            std::unique_lock<std::mutex> g(m_);
            if (cap_) room_.wait(g, [this] { return pending_ < cap_; });
            q_.push_back(Job{std::move(path), mode, std::move(fill)});
            ++pending_;
        }
        cv_.notify_one();
    }

    // wait until every submitted file is on disk; 0, or -1 with the first error in *err
    int flush(std::string* err) {
        std::unique_lock<std::mutex> g(m_);
        done_.wait(g, [this] { return pending_ == 0; });
        if (err_.empty()) return 0;
        if (err) *err = err_;
        err_.clear();
        return -1;
    }

  private:
    struct Job {
        std::string path;
        const char* mode;
        Fill fill;
    };

    void loop() {
        for (;;) {
            Job j;
            {
                std::unique_lock<std::mutex> g(m_);
                cv_.wait(g, [this] { return stop_ || !q_.empty(); });
                if (q_.empty()) return;
                j = std::move(q_.front());
                q_.pop_front();
            }
            std::string e;
            FILE* f = fopen(j.path.c_str(), j.mode);
            if (!f) {
                e = "cannot open " + j.path + ": " + strerror(errno);
            } else {
                bool ok;
                {
                    LgText t(f);
                    j.fill(t);
                    t.spill();
                    ok = t.ok();
                }
                if (fclose(f) != 0 || !ok) e = "write error on " + j.path;
            }
            j.fill = nullptr;                  // release the snapshot before signalling
            {
                std::lock_guard<std::mutex> g(m_);
                if (!e.empty() && err_.empty()) err_ = e;
                if (--pending_ == 0) done_.notify_all();
                if (cap_) room_.notify_one();
            }
        }
    }

    std::mutex m_;
    std::condition_variable cv_, done_, room_;
    std::deque<Job> q_;
    std::vector<std::thread> pool_;
    size_t pending_ = 0;
    const size_t cap_;
    bool stop_ = false;
    std::string err_;
};

}  // namespace mdqt
