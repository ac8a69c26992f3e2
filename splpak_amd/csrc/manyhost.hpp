// The host layer the batch families share (splpak_fit_many_* and its variants through fitmanyentry.hpp; splpak_eval_many_*,
// splpak_residuals_many_* and splpak_mad_many_* in evalmanyapi.hip): the span of a batch's points, the copies a host entry stages through memory of the call,
// the calling thread's device scratch for the tables of a call, and the status after the device part.
#pragma once
#include "callstage.hpp"
#include "evalscratch.hpp"
#include "../../include/splpak_hip.h"

namespace splpak {

// The points of a batch: the global indices lo .. lo + n - 1.  A host entry uploads that span alone, and the kernels address
// its device copies at the global index minus lo (`base`).
struct ManySpan {
    long long lo, n;
};
inline ManySpan many_span(const int64_t *offsets, int nbatch) { return {offsets[0], offsets[nbatch] - offsets[0]}; }

// n coefficient sets ld apart, ncol each: what a host entry copies in one block with the caller's ld
inline size_t coef_block_len(long long n, long long ld, long long ncol) { return (size_t)(n - 1) * (size_t)ld + (size_t)ncol; }

// *dst = a device copy of src[0 .. count-1] that lives as long as cs (src has been read when this returns).
// hipErrorOutOfMemory: no room for it (set_error says how much was asked).
template <typename T>
hipError_t stage_copy(CallStage &cs, const T *src, size_t count, const T **dst)
{
    T *d = nullptr;
    if (!cs.get(&d, count)) return hipErrorOutOfMemory;
    *dst = d;
    return hipMemcpy(d, src, sizeof(T) * count, hipMemcpyHostToDevice);
}

// the span's x (ld per point) and, where they are not null, y and w
template <typename T>
hipError_t stage_span(CallStage &cs, ManySpan sp, const T *x, int ld, const T *y, const T *w, const T **xd, const T **yd, const T **wd)
{
    hipError_t e = stage_copy(cs, x + sp.lo * ld, (size_t)sp.n * (size_t)ld, xd);
    if (e == hipSuccess && y) e = stage_copy(cs, y + sp.lo, (size_t)sp.n, yd);
    if (e == hipSuccess && w) e = stage_copy(cs, w + sp.lo, (size_t)sp.n, wd);
    return e;
}

// The calling thread's device scratch of the batch entries (evalmany.hip; released by splpak_shutdown through
// eval_scratch_shutdown): the offsets of a call, for all three families, and fit_many's problem list [nrun] and result block
// [nrun][FM_RESULT].  Two scratches, so that a regrow of one leaves the other alone.
extern thread_local DevScratch<1> t_many_offsets;
extern thread_local DevScratch<2> t_fit_many_tables;
// .. and the weighted residuals of splpak_fit_many_clip_mad_*: a double per point of the batch's span (fitmanymad.hip selects
// its medians from them)
extern thread_local DevScratch<1> t_fit_many_mad_t;
void many_scratch_shutdown();

// The scratch holds `need` on the current device and st waits for the previous use of it (which may have been on another
// stream).  The caller holds a ScratchUse{s, st} from before this call to its return.  hipErrorOutOfMemory: no room.
template <int N>
hipError_t scratch_begin(DevScratch<N> &s, const size_t (&need)[N], hipStream_t st)
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (s.ensure(dev, need, /*may_release_plan=*/true) != hipSuccess) {
        (void)hipGetLastError();
        set_error("the device tables of the batch (offsets, problem list, results) could not be allocated");
        return hipErrorOutOfMemory;
    }
    return s.wait_on(st);
}

// *offsets_dev = the copy of a call's nbatch + 1 offsets in t_many_offsets, uploaded on st (scratch_begin's rules)
inline hipError_t many_offsets_upload(const int64_t *offsets, int nbatch, hipStream_t st, const long long **offsets_dev)
{
    static_assert(sizeof(long long) == sizeof(int64_t), "offsets are uploaded as they are");
    const size_t need[1] = {sizeof(int64_t) * ((size_t)nbatch + 1)};
    hipError_t e = scratch_begin(t_many_offsets, need, st);
    // (pageable memory: the copy has left `offsets` when the call returns)
    if (e == hipSuccess) e = hipMemcpyAsync(t_many_offsets.buf[0], offsets, need[0], hipMemcpyHostToDevice, st);
    *offsets_dev = t_many_offsets.as<long long>(0);
    return e;
}

// What an entry returns after its device part: rc when all went well, SPLPAK_E_NOMEM where an allocation failed (the error
// text was set there), SPLPAK_E_NODEVICE otherwise.
inline int32_t many_status(hipError_t e, const char *what, int rc)
{
    if (e == hipErrorOutOfMemory) return SPLPAK_E_NOMEM;
    return hip_ok(e, what) ? rc : SPLPAK_E_NODEVICE;
}

}  // namespace splpak
