// pinned.h -- what the host side stages for the device: a pinned host buffer with a device buffer of the same size
// (PinnedPair), and a ring of them for the small arrays that go with a launch (UploadRing).
#pragma once

#include <cstring>

#include "host_common.h"
#include "worker_pool.h"

namespace h263mi {

inline int make_event(hipEvent_t &e)
{
    HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return H263MI_OK;
}

// n elements of T in pinned host memory (h) and on the device (d): filled on the host, copied across.  All or nothing: an
// allocation that fails leaves the pair empty.  The host half lies on the NUMA node of the device (worker_pool.h): the
// placement is set around the allocations only.
template <typename T>
struct PinnedPair {
    T *h = nullptr, *d = nullptr;
    size_t cap = 0;                            // elements

    PinnedPair() = default;
    PinnedPair(const PinnedPair &) = delete;
    PinnedPair &operator=(const PinnedPair &) = delete;
    ~PinnedPair() { release(); }

    // room for `need` elements; when the pair has to grow, it is made anew with room for need + slack
    int reserve(size_t need, size_t slack, const HostPlacement &where)
    {
        if (h && need <= cap) return H263MI_OK;
        release();
        PlacementScope near_device(where);
        const int rc = allocate(need + slack);
        if (rc != H263MI_OK) release();
        return rc;
    }
    void release()
    {
        if (h) (void)hipHostFree(h);
        if (d) (void)hipFree(d);
        h = d = nullptr;
        cap = 0;
    }

private:
    int allocate(size_t n)
    {
        HIP_TRY(hipHostMalloc((void **)&h, n * sizeof(T), hipHostMallocDefault));
        HIP_TRY(hipMalloc((void **)&d, n * sizeof(T)));
        cap = n;
        return H263MI_OK;
    }
};

// kSlots pinned slots of n elements each, their device copies and a copy event per slot: push() fills the next slot, once the
// copy queued from it kSlots pushes ago has left it, and queues its copy.
template <typename T>
struct UploadRing {
    static constexpr unsigned kSlots = 4;
    PinnedPair<T> buf;
    hipEvent_t copied[kSlots] = {};
    unsigned next = 0;
    size_t n = 0;

    ~UploadRing() { release(); }

    bool made() const { return buf.h != nullptr; }
    // all or nothing, like PinnedPair
    int make(size_t n_elems, const HostPlacement &where)
    {
        if (made()) return H263MI_OK;
        int rc = buf.reserve(n_elems * kSlots, 0, where);
        for (unsigned k = 0; k < kSlots && rc == H263MI_OK; k++) rc = make_event(copied[k]);
        if (rc != H263MI_OK) release();
        n = rc == H263MI_OK ? n_elems : 0;
        return rc;
    }
    // `src`: n elements; *d_out: their device copy, queued on `on` in front of whatever is queued there next
    int push(const T *src, const T **d_out, hipStream_t on)
    {
        const unsigned slot = next++ % kSlots;
        HIP_TRY(hipEventSynchronize(copied[slot]));
        T *h = buf.h + slot * n, *d = buf.d + slot * n;
        memcpy(h, src, n * sizeof(T));
        HIP_TRY(hipMemcpyAsync(d, h, n * sizeof(T), hipMemcpyHostToDevice, on));
        HIP_TRY(hipEventRecord(copied[slot], on));
        *d_out = d;
        return H263MI_OK;
    }
    void release()
    {
        buf.release();
        for (hipEvent_t &e : copied) {
            if (e) (void)hipEventDestroy(e);
            e = nullptr;
        }
    }
};

}  // namespace h263mi
