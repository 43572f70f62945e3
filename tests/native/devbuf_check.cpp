// mdqt_devbuf.hpp's Buf<T, Space> over a Space of this file's that counts its calls and live bytes and can be
// told to fail its k-th allocation (tests/test_devbuf.py builds and runs it, plain and with
// -fsanitize=address,undefined: the blocks are malloc'ed, so a double release or a leak stops that run).
// One line per check: "ok <name>" or "FAIL <name>: ..."; exit status 1 after any FAIL.
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <string>
#include <utility>
#include <vector>

#include "mdqt_devbuf.hpp"

namespace {

struct FakeSpace {
    static inline std::atomic<long long> live{0};   // Buf's own count
    static inline int allocs = 0, handed = 0, releases = 0;   // alloc calls, those that gave a block, release calls
    static inline int fail_at = 0;                  // k > 0: the k-th alloc call from now fails
    static inline long long bytes = 0;              // this Space's count of what it handed out
    static inline std::map<void*, size_t> blocks;
    static inline std::vector<std::string> log;     // "a<bytes>" / "r<bytes>" in call order
    static inline unsigned last_flags = 0;
    static inline int bad_release = 0;              // releases of a pointer it does not hold

    static hipError_t alloc(void** p, size_t n, unsigned flags) {
        ++allocs;
        last_flags = flags;
        if (fail_at > 0 && --fail_at == 0) { *p = nullptr; return hipErrorOutOfMemory; }
        *p = malloc(n);
        ++handed;
        blocks[*p] = n;
        bytes += (long long)n;
        log.push_back("a" + std::to_string(n));
        return hipSuccess;
    }
    static hipError_t release(void* p) {
        ++releases;
        auto it = blocks.find(p);
        if (it == blocks.end()) { ++bad_release; return hipErrorInvalidValue; }
        bytes -= (long long)it->second;
        log.push_back("r" + std::to_string(it->second));
        blocks.erase(it);
        free(p);
        return hipSuccess;
    }
};

template <class T> using FBuf = mdqt::Buf<T, FakeSpace>;

int failures = 0;
void check(bool ok, const char* name, const std::string& why = "") {
    if (ok) printf("ok %s\n", name);
    else { printf("FAIL %s: %s\n", name, why.c_str()); ++failures; }
}
std::string state() {
    return "allocs " + std::to_string(FakeSpace::allocs) + " handed " + std::to_string(FakeSpace::handed) + " releases " +
           std::to_string(FakeSpace::releases) + " bytes " + std::to_string(FakeSpace::bytes) + " live " +
           std::to_string(FakeSpace::live.load());
}
bool balanced() {   // nothing held, every block released exactly once
    return FakeSpace::blocks.empty() && FakeSpace::bytes == 0 && FakeSpace::live.load() == 0 && FakeSpace::bad_release == 0 &&
           FakeSpace::handed == FakeSpace::releases;
}

// a function holding two local buffers that returns early between them (fail_at set by the caller)
hipError_t two_locals(size_t n) {
    FBuf<double> a, b;
    hipError_t r;
    if ((r = a.alloc(n)) != hipSuccess) return r;
    if ((r = b.alloc(2 * n)) != hipSuccess) return r;   // the early return: a is held
    return hipSuccess;
}

}  // namespace

int main() {
    {   // reserve(0) on an empty buffer; reserve within the capacity
        FBuf<double> b;
        check(b.reserve(0) == hipSuccess && FakeSpace::allocs == 0 && !b && b.capacity() == 0, "reserve0_empty", state());
        check(b.reserve(100) == hipSuccess && b && b.capacity() == 100 && FakeSpace::allocs == 1 && FakeSpace::bytes == 800 &&
                  FakeSpace::live == 800, "reserve_first", state());
        double* p = b;
        const int a0 = FakeSpace::allocs, r0 = FakeSpace::releases;
        bool same = b.reserve(100) == hipSuccess && b.reserve(1) == hipSuccess && b.reserve(0) == hipSuccess;
        check(same && FakeSpace::allocs == a0 && FakeSpace::releases == r0 && (double*)b == p && b.capacity() == 100,
              "reserve_within_capacity_no_call", state());
        // a grow: the old block goes before the new one comes
        FakeSpace::log.clear();
        check(b.reserve(101) == hipSuccess && b.capacity() == 101 && FakeSpace::log.size() == 2 && FakeSpace::log[0] == "r800" &&
                  FakeSpace::log[1] == "a808" && FakeSpace::bytes == 808 && FakeSpace::live == 808, "grow_frees_then_allocates", state());
        // alloc: exactly n, also a smaller n
        FakeSpace::log.clear();
        check(b.alloc(10) == hipSuccess && b.capacity() == 10 && FakeSpace::log.size() == 2 && FakeSpace::log[0] == "r808" &&
                  FakeSpace::log[1] == "a80" && FakeSpace::live == 80, "alloc_exact", state());
        p = b;
        p[0] = 1.; p[9] = 2.;                           // the block is the buffer's to write
        check(b[0] + b[9] == 3. && *(b + 9) == 2., "reads_like_a_pointer");
        b.reset();
        check(!b && b.capacity() == 0 && FakeSpace::bytes == 0 && FakeSpace::live == 0, "reset", state());
        b.reset();
        check(FakeSpace::bad_release == 0 && FakeSpace::handed == FakeSpace::releases, "reset_twice_one_release", state());
    }
    check(balanced(), "balanced_after_scope", state());

    {   // a failed alloc / reserve leaves the buffer empty, and the next reserve asks again
        FBuf<int> b;
        check(b.alloc(50) == hipSuccess, "fail_setup");
        FakeSpace::fail_at = 1;
        check(b.reserve(60) != hipSuccess && !b && b.capacity() == 0 && FakeSpace::bytes == 0 && FakeSpace::live == 0,
              "failed_reserve_empty", state());
        int a0 = FakeSpace::allocs;
        check(b.reserve(60) == hipSuccess && FakeSpace::allocs == a0 + 1 && b && b.capacity() == 60, "reserve_after_failure_allocates",
              state());
        FakeSpace::fail_at = 1;
        check(b.alloc(5) != hipSuccess && !b && b.capacity() == 0 && FakeSpace::bytes == 0 && FakeSpace::live == 0,
              "failed_alloc_empty", state());
        a0 = FakeSpace::allocs;
        check(b.reserve(5) == hipSuccess && FakeSpace::allocs == a0 + 1 && b.capacity() == 5, "reserve_after_failed_alloc", state());
        check(b.alloc(7, 0x0b) == hipSuccess && FakeSpace::last_flags == 0x0b, "flags_reach_the_space");
    }
    check(balanced(), "balanced_after_failures", state());

    {   // moves and swap
        FBuf<double> a, b;
        check(a.alloc(3) == hipSuccess && b.alloc(4) == hipSuccess, "move_setup");
        double *pa = a, *pb = b;
        FBuf<double> c(std::move(a));
        check(!a && a.capacity() == 0 && (double*)c == pa && c.capacity() == 3, "move_construct_empties_source");
        std::swap(b, c);
        check((double*)b == pa && b.capacity() == 3 && (double*)c == pb && c.capacity() == 4 && FakeSpace::bytes == 56 &&
                  FakeSpace::live == 56, "swap_pointer_and_capacity", state());
        const int r0 = FakeSpace::releases;
        b = std::move(c);                              // b's block goes, c's moves in
        check(FakeSpace::releases == r0 + 1 && (double*)b == pb && b.capacity() == 4 && !c && c.capacity() == 0 &&
                  FakeSpace::live == 32, "move_assign", state());
        FBuf<double>& self = b;
        b = std::move(self);
        check((double*)b == pb && b.capacity() == 4, "self_move_keeps");
        std::vector<FBuf<double>> v(3);                // a container of them (the contexts hold arrays)
        check(v[1].alloc(2) == hipSuccess, "vector_setup");
        v.resize(40);
        check(v[1].capacity() == 2 && FakeSpace::live == 48, "vector_growth_moves", state());
    }
    check(balanced(), "balanced_after_moves", state());

    {   // the early return of a function with two local buffers
        FakeSpace::fail_at = 2;
        check(two_locals(8) != hipSuccess && balanced(), "early_return_releases_first_local", state());
        check(two_locals(8) == hipSuccess && balanced(), "normal_return_releases_both", state());
    }

    // the HIP spaces' aliases are a pointer and a count (named only: this program links no HIP runtime)
    static_assert(sizeof(mdqt::DevBuf<double>) == sizeof(double*) + sizeof(size_t), "DevBuf layout");
    static_assert(sizeof(mdqt::PinBuf<volatile int>) == sizeof(int*) + sizeof(size_t), "PinBuf layout");
    check(balanced(), "live_bytes_zero_at_exit", state());
    return failures ? 1 : 0;
}
