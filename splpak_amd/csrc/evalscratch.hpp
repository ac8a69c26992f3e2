// Per-thread device scratch of an evaluation path: N buffers and the event that marks the end of their last use.  The region
// sort, the run path, the persistent path and the grid route each keep a thread_local instance (regrowing one leaves the others alone):
//   ensure     the buffers hold at least the asked sizes on this device (regrown together, never shrunk)
//   wait_on    a stream about to use them waits for the previous use (which may have been on another stream)
//   mark_used  records the end of this use (ScratchUse below: on every exit of a scope)
//   release    frees everything (splpak_shutdown, a failed ensure)
#pragma once
#include "kernels.hpp"

namespace splpak {

template <int N>
struct DevScratch {
    void *buf[N] = {};
    size_t bytes[N] = {};
    hipEvent_t last = nullptr;
    int dev = -1;
    bool used = false;            // `last` has been recorded since the buffers were allocated
    long long allocs = 0;         // hipMalloc calls that succeeded, over the life of the object (the entries' debug counters)

    template <typename T> T *as(int i) const { return static_cast<T *>(buf[i]); }

    void release()
    {
        for (int i = 0; i < N; ++i) {
            if (buf[i]) (void)hipFree(buf[i]);      // (hipFree waits for the work that uses the buffer)
            buf[i] = nullptr;
            bytes[i] = 0;
        }
        if (last) (void)hipEventDestroy(last);
        last = nullptr;
        dev = -1;
        used = false;
    }

    // may_release_plan: after a failed allocation give up the one-shot fit's cached plan and try once more.
    // On failure nothing is held and the hipMalloc error is returned (the caller decides what it means for its path).
    hipError_t ensure(int device, const size_t (&need)[N], bool may_release_plan)
    {
        bool fits = dev == device && last;
        for (int i = 0; i < N; ++i) fits = fits && need[i] <= bytes[i];
        if (fits) return hipSuccess;
        size_t want[N];
        for (int i = 0; i < N; ++i) want[i] = (dev == device && bytes[i] > need[i]) ? bytes[i] : need[i];
        release();
        hipError_t e = hipEventCreateWithFlags(&last, hipEventDisableTiming);
        for (int i = 0; i < N && e == hipSuccess; ++i) {
            bool released = false;
            e = may_release_plan ? hip_malloc_retry(&buf[i], want[i], &released) : hipMalloc(&buf[i], want[i]);
            if (released) may_release_plan = false;
            if (e == hipSuccess) { bytes[i] = want[i]; ++allocs; }
            else buf[i] = nullptr;
        }
        if (e != hipSuccess) { release(); return e; }
        dev = device;
        return hipSuccess;
    }

    hipError_t wait_on(hipStream_t st) { return used ? hipStreamWaitEvent(st, last, 0) : hipSuccess; }

    hipError_t mark_used(hipStream_t st)
    {
        const hipError_t e = hipEventRecord(last, st);
        used = used || e == hipSuccess;
        return e;
    }
};

// Held from wait_on to the end of a call (the grid routes, the grid fit): records the end of this use of the scratch on
// every exit, the error returns included: what was queued before them still reads and writes the buffers, and a later call
// on another stream has to wait for it.  (Nothing to record while the scratch holds nothing: before or after a failed ensure.)
template <int N>
struct ScratchUse {
    DevScratch<N> &s;
    hipStream_t st;
    ~ScratchUse() { if (s.last) (void)s.mark_used(st); }
};

}  // namespace splpak
