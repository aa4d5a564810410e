// Owners of what the evaluator holds on a device -- allocations, streams, events: released when the owner goes, never
// copied.  Whoever destroys them has set the device and made sure nothing queued still uses them.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

#include "evaluator.h"  // HIP_CHECK

namespace ieache {
namespace dev {

// Scratch sized by what calls have needed so far, not by the largest chunk a launch may take (65 536 gate instances are
// ~1 GB of accumulators, extracted samples and key-switch digits): at least `need` (<= cap) items, doubling from `floor` so
// that a run of growing batches does not reallocate every time.
inline size_t grown(size_t have, size_t need, size_t cap, size_t floor = 4096) {
    return std::max(need, std::min(std::max(cap, need), std::max(2 * have, floor)));
}

// A device allocation and its capacity, counted in items of whatever size its owner reserves in (rows, gate instances, bytes).
template <class T>
class DeviceBuffer {
public:
    DeviceBuffer() = default;
    DeviceBuffer(const DeviceBuffer&) = delete;
    DeviceBuffer& operator=(const DeviceBuffer&) = delete;
    ~DeviceBuffer() { (void)hipFree(ptr_); }
    operator T*() const { return ptr_; }
    size_t items() const { return items_; }
    // A new allocation of `items` x `item_bytes` (+ `slack`) bytes, zero-filled on request, in place of the old one, whose
    // contents are not kept.  Every hipMalloc / hipFree is a device-wide synchronisation; after a failure the buffer is empty.
    void allocate(size_t items, size_t item_bytes = sizeof(T), size_t slack = 0, bool zero = false) {
        T* old = ptr_;
        ptr_ = nullptr;
        items_ = 0;
        if (old) HIP_CHECK(hipFree(old));
        void* p = nullptr;
        HIP_CHECK(hipMalloc(&p, items * item_bytes + slack));
        if (zero) {
            const hipError_t e = hipMemset(p, 0, items * item_bytes + slack);
            if (e != hipSuccess) (void)hipFree(p);
            HIP_CHECK(e);
        }
        ptr_ = static_cast<T*>(p);
        items_ = items;
    }
    // room for `need` items: exactly that many, or grown() under a cap when the need is expected to rise from call to call
    void reserve_exact(size_t need, size_t item_bytes = sizeof(T)) {
        if (items_ < need) allocate(need, item_bytes);
    }
    void reserve(size_t need, size_t cap, size_t item_bytes = sizeof(T), size_t floor = 4096) {
        if (items_ < need) allocate(grown(items_, need, cap, floor), item_bytes);
    }

private:
    T* ptr_ = nullptr;
    size_t items_ = 0;
};

// a non-blocking stream / an event without timing, created on first use
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    ~Stream() {
        if (s) (void)hipStreamDestroy(s);
    }
    operator hipStream_t() const { return s; }
    void ensure() {
        if (!s) HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    }
};
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    ~Event() {
        if (e) (void)hipEventDestroy(e);
    }
    operator hipEvent_t() const { return e; }
    void ensure() {
        if (!e) HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
};

}  // namespace dev
}  // namespace ieache
