// Driver of tests/test_writer_bounded.py: a FileWriter with a cap on submitted-but-unwritten jobs
// (mdqtplasmasims_amd/csrc/mdqt_writer.hpp), fed as the QT tagging programs' recorded stage feeds it —
// one snapshot of 4,001 values per file, rows "(i - 2000) 0.0025 \t value".
//   writer_bound_check <outdir> [jobs]
// checks that the snapshots alive at once never exceed cap + threads, that every file's bytes are
// fprintf("%lg\t%lg\n")'s, and that an unwritable path comes back from flush() with its name.
// Exit 0 and one line "max_live=<n> cap=<c> threads=<t>" on success; a message on stderr and 1 otherwise.
#include <unistd.h>

#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "mdqt_writer.hpp"

namespace {

constexpr int kBins = 4001, kThreads = 4, kCap = 8;

std::atomic<int> g_live{0}, g_max_live{0};

double value(int job, int i) {            // any spread of magnitudes, and one NaN row per 97 files
    if (job % 97 == 5 && i == 1234) return NAN;
    uint64_t x = (uint64_t)job * 0x9E3779B97F4A7C15ull + (uint64_t)i * 0xBF58476D1CE4E5B9ull;
    x ^= x >> 31; x *= 0x94D049BB133111EBull; x ^= x >> 29;
    const double m = (double)(x >> 11) / 9007199254740992.0;          // [0, 1)
    const int e = (int)(x % 41) - 30;                                  // 1e-30 .. 1e10
    return (x & 1 ? -m : m) * std::pow(10., e);
}

struct Snapshot {
    std::vector<double> v;
    explicit Snapshot(int job) : v(kBins) {
        const int n = ++g_live;
        int seen = g_max_live.load();
        while (n > seen && !g_max_live.compare_exchange_weak(seen, n)) {}
        for (int i = 0; i < kBins; ++i) v[i] = value(job, i);
    }
    ~Snapshot() { --g_live; }
};

std::string path_of(const std::string& dir, int job) {
    char b[64];
    snprintf(b, sizeof b, "/vel_distX_timestep%06d.dat", job);
    return dir + b;
}

bool same_as_fprintf(const std::string& path, int job) {
    std::string want;
    want.reserve(kBins * 24);
    char b[96];
    for (int i = 0; i < kBins; ++i) {
        const int n = snprintf(b, sizeof b, "%lg\t%lg\n", (double)(i - 2000) * 0.0025, value(job, i));
        want.append(b, n);
    }
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    std::string got(want.size() + 16, '\0');
    got.resize(fread(&got[0], 1, got.size(), f));
    fclose(f);
    return got == want;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) return fprintf(stderr, "usage: writer_bound_check <outdir> [jobs]\n"), 2;
    const std::string dir = argv[1];
    const int jobs = argc > 2 ? atoi(argv[2]) : 2000;
    {
        mdqt::FileWriter w(kThreads, kCap);
        for (int job = 0; job < jobs; ++job) {
            auto snap = std::make_shared<const Snapshot>(job);
            w.submit(path_of(dir, job), "w", [snap](mdqt::LgText& t) {
                for (int i = 0; i < kBins; ++i) {
                    t.num((double)(i - 2000) * 0.0025); t.ch('\t'); t.num(snap->v[i]); t.ch('\n');
                }
            });
        }
        std::string err;
        if (w.flush(&err)) return fprintf(stderr, "flush: %s\n", err.c_str()), 1;
        if (g_live.load() != 0) return fprintf(stderr, "%d snapshots alive after flush\n", g_live.load()), 1;
        // an unwritable path: reported by the next flush, with its name; the writer goes on working after it
        const std::string bad = dir + "/no_such_directory/vel_distX_timestep000000.dat";
        w.submit(bad, "w", [](mdqt::LgText& t) { t.num(1.); });
        if (w.flush(&err) == 0) return fprintf(stderr, "flush did not report %s\n", bad.c_str()), 1;
        if (err.find(bad) == std::string::npos) return fprintf(stderr, "error without the name: %s\n", err.c_str()), 1;
        if (w.flush(&err) != 0) return fprintf(stderr, "the error was reported twice\n"), 1;
    }
    if (g_max_live.load() > kCap + kThreads)
        return fprintf(stderr, "%d snapshots alive at once > cap %d + threads %d\n", g_max_live.load(), kCap, kThreads), 1;
    std::atomic<int> bad_file{-1};
    std::vector<std::thread> pool;
    for (int t = 0; t < 8; ++t)
        pool.emplace_back([&, t] {
            for (int job = t; job < jobs; job += 8) {
                const std::string p = path_of(dir, job);
                if (!same_as_fprintf(p, job)) bad_file = job;
                unlink(p.c_str());
            }
        });
    for (auto& t : pool) t.join();
    if (bad_file.load() >= 0) return fprintf(stderr, "file of job %d differs from fprintf's bytes\n", bad_file.load()), 1;
    printf("max_live=%d cap=%d threads=%d\n", g_max_live.load(), kCap, kThreads);
    return 0;
}
