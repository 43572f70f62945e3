// mdqt_batch.hpp's pinned argument ring and launch timer
#include "mdqt_batch.hpp"

#include <algorithm>

#include "mdqt_error.hpp"   // HIPCHK, mdqt::set_error, kTimingEventFlags

using namespace mdqt;

int PinRing::create(size_t bytes, int slots, unsigned event_flags) {
    slot_bytes = bytes;
    if (base.alloc(bytes * (size_t)slots) != hipSuccess)
        return set_error("pinned allocation of %d argument slots of %zu bytes failed", slots, bytes);
    busy.assign((size_t)slots, 0);
    for (int i = 0; i < slots; ++i) {
        hipEvent_t e = nullptr;
        HIPCHK(hipEventCreateWithFlags(&e, event_flags));
        ev.push_back(e);
    }
    return 0;
}

int PinRing::take(char** slot, int* idx) {
    const int i = next;
    next = (i + 1) % (int)ev.size();
    // the one wait before reuse: the host writes the slot next, and a queued copy may not have read it yet
    if (busy[(size_t)i]) HIPCHK(hipEventSynchronize(ev[(size_t)i]));
    busy[(size_t)i] = 0;
    *slot = base + slot_bytes * (size_t)i;
    *idx = i;
    return 0;
}

int PinRing::send(int idx, void* dst, size_t bytes, hipStream_t s) {
    HIPCHK(hipMemcpyAsync(dst, base + slot_bytes * (size_t)idx, bytes, hipMemcpyHostToDevice, s));
    HIPCHK(hipEventRecord(ev[(size_t)idx], s));
    busy[(size_t)idx] = 1;
    return 0;
}

void PinRing::destroy() {
    base.reset();
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    ev.clear();
    busy.clear();
}

int LaunchTimer::next(hipEvent_t* e) {
    if (used == (int)pool.size()) {
        hipEvent_t x;
        HIPCHK(hipEventCreateWithFlags(&x, kTimingEventFlags));
        pool.push_back(x);
    }
    *e = pool[(size_t)used++];
    return 0;
}

int LaunchTimer::stats(double* v) {
    std::vector<double> ms;
    double tot = 0.;
    for (int i = 0; i + 1 < used; i += 2) {
        float x = 0.f;
        HIPCHK(hipEventElapsedTime(&x, pool[(size_t)i], pool[(size_t)i + 1]));
        ms.push_back(x);
        tot += x;
    }
    std::sort(ms.begin(), ms.end());
    v[0] = tot;
    v[1] = (double)ms.size();
    v[2] = ms.empty() ? 0. : ms[ms.size() / 2];
    v[3] = ms.empty() ? 0. : ms.front();
    v[4] = ms.empty() ? 0. : ms.back();
    used = 0;
    return 0;
}

void LaunchTimer::destroy() {
    for (hipEvent_t e : pool) (void)hipEventDestroy(e);
    pool.clear();
    used = 0;
}
