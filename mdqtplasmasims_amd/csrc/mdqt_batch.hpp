// What the ensembles' batched launches share on the host (mdqt_ensemble.cpp, mdqt_pump_ensemble.cpp,
// mdmc_ensemble.cpp; LaunchTimer also in a single context): the pinned ring their argument blocks travel
// through and the pool of event pairs that times a launch.  Host only: no .hip file includes it.
#pragma once

#include <hip/hip_runtime.h>
#include <string.h>

#include <vector>

#include "mdqt_devbuf.hpp"

namespace mdqt {

constexpr int kEnsembleMaxJobs = 1024;   // njobs of every ensemble: 1 .. kEnsembleMaxJobs

// A pinned ring of equal slots for argument blocks on their way to the device: the host fills a slot, one
// hipMemcpyAsync reads it in stream order, and the event recorded behind the copy says when the slot may be
// written again (the host queues far ahead of the device, so a slot is not free when the call returns).
struct PinRing {
    PinBuf<char> base;
    size_t slot_bytes = 0;
    int next = 0;
    std::vector<hipEvent_t> ev;        // one per slot
    std::vector<char> busy;            // a copy of the slot has been queued

    int create(size_t slot_bytes, int slots, unsigned event_flags);
    int take(char** slot, int* idx);   // the next slot, once the copy that last read it has run
    int send(int idx, void* dst, size_t bytes, hipStream_t s);   // one copy of the slot, its event behind it
    void destroy();
    ~PinRing() { destroy(); }

    // blocks that seldom change: h goes to dst (through a slot) when it differs from `held`, what dst holds
    template <class T>
    int send_if_changed(const std::vector<T>& h, std::vector<T>& held, void* dst, hipStream_t s) {
        const size_t bytes = h.size() * sizeof(T);
        if (h.empty() || (h.size() == held.size() && !memcmp(h.data(), held.data(), bytes))) return 0;
        char* slot = nullptr;
        int idx = 0;
        if (take(&slot, &idx)) return -1;
        memcpy(slot, h.data(), bytes);
        if (send(idx, dst, bytes, s)) return -1;
        held = h;
        return 0;
    }
};

// Start / stop events for launches that record their own dispatch timestamps, and what they measured
struct LaunchTimer {
    std::vector<hipEvent_t> pool;      // start, stop, start, stop, ...
    int used = 0;

    int next(hipEvent_t* e);           // one event (a caller that brackets several launches records it itself)
    int take(hipEvent_t* e0, hipEvent_t* e1) { return next(e0) || next(e1); }
    // v[5] = sum (ms), launches, median, minimum, maximum (ms) of the pairs taken since the last call; resets.
    // The caller has synchronised the stream the events were recorded on.
    int stats(double* v);
    void reset() { used = 0; }
    void destroy();
    ~LaunchTimer() { destroy(); }
};

}  // namespace mdqt
