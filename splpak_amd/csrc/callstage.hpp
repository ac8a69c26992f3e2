// Device memory of one call, released with it: what a host entry stages its arrays and results through.
#pragma once
#include "kernels.hpp"

#include <cstdio>
#include <vector>

namespace splpak {

struct CallStage {
    std::vector<void *> held;
    CallStage() = default;
    CallStage(const CallStage &) = delete;
    CallStage &operator=(const CallStage &) = delete;
    ~CallStage() { for (void *p : held) (void)hipFree(p); }      // (hipFree waits for the work that uses the buffer)

    // count elements (one for none); false = set_error says why, the entry returns SPLPAK_E_NOMEM
    template <typename U> bool get(U **out, size_t count)
    {
        void *q = nullptr;
        if (count == 0) count = 1;
        const hipError_t e = hip_malloc_retry(&q, count * sizeof(U));      // (the one-shot fit's cached plan -- 35 GB at 64^3 -- may be in the way)
        if (e != hipSuccess) {
            char buf[160];
            snprintf(buf, sizeof buf, "hipMalloc of %.3f GB failed: %s", (double)(count * sizeof(U)) / 1e9, hipGetErrorString(e));
            set_error(buf);
            (void)hipGetLastError();
            return false;
        }
        held.push_back(q);
        *out = static_cast<U *>(q);
        return true;
    }
};

}  // namespace splpak
