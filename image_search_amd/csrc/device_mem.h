// device_mem.h — memory that frees itself: a handle's device arrays (DevArray), one call's private device memory (Scratch)
// and pinned host memory (PinnedBuf).  hipFree / hipHostFree find the memory's device by themselves, whichever is selected
// when an owner goes out of scope.
#pragma once
#include <algorithm>
#include <utility>
#include <vector>

#include "common.h"

namespace mi {

// A device array of `cap` elements of T.  It reads as the pointer it owns: kernel launches, copies and pointer arithmetic
// take the field as they would a T* (where a cast or a templated callee cannot see through the conversion: .p).
template <class T>
struct DevArray {
    T* p = nullptr;
    size_t cap = 0;
    DevArray() = default;
    DevArray(const DevArray&) = delete;
    DevArray& operator=(const DevArray&) = delete;
    ~DevArray() {
        if (p) (void)hipFree(p);
    }
    operator T*() const { return p; }
    void swap(DevArray& o) { std::swap(p, o.p); std::swap(cap, o.cap); }
    void release() {
        if (p) HIP_CHECK(hipFree(p));
        p = nullptr; cap = 0;
    }
    // n elements, nothing kept, on an array that holds nothing yet
    void alloc(size_t n) {
        HIP_CHECK(hipMalloc((void**)&p, n * sizeof(T)));
        cap = n;
    }
    // room for n elements, the contents not kept.  Enough already: nothing is touched; otherwise whatever `order` counts (the
    // searches in flight, for a handle's workspace) has finished before the old array is freed
    void reserve(WorkOrder& order, size_t n) {
        if (cap >= n) return;
        order.sync();
        release();
        alloc(n);
    }
    // as reserve(), keeping the first `keep` elements (a mirror that grows with the table must not be rebuilt from the fp32 rows)
    void reserve_keep(WorkOrder& order, size_t n, size_t keep) {
        if (cap >= n) return;
        order.sync();
        DevArray grown;
        grown.alloc(n);
        if (p && keep) HIP_CHECK(hipMemcpy(grown.p, p, std::min(keep, cap) * sizeof(T), hipMemcpyDeviceToDevice));
        swap(grown);
    }
};

// device memory of one call, freed on every way out
struct Scratch {
    std::vector<void*> p;
    void* get(size_t bytes) {
        void* q = nullptr;
        HIP_CHECK(hipMalloc(&q, std::max<size_t>(bytes, 16)));
        p.push_back(q);
        return q;
    }
    ~Scratch() {
        for (void* q : p) (void)hipFree(q);
    }
};

// pinned host memory; `flags`: hipHostMallocPortable where streams of several devices read and write it
struct PinnedBuf {
    void* p = nullptr;
    size_t cap = 0;   // bytes
    unsigned flags;
    explicit PinnedBuf(unsigned flags_ = hipHostMallocDefault) : flags(flags_) {}
    PinnedBuf(size_t b, unsigned flags_) : flags(flags_) { reserve(b); }
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    ~PinnedBuf() {
        if (p) (void)hipHostFree(p);
    }
    // room for b bytes, the contents not kept; nothing in flight may read or write the old buffer
    void reserve(size_t b) {
        if (b <= cap) return;
        if (p) HIP_CHECK(hipHostFree(p));
        p = nullptr; cap = 0;
        HIP_CHECK(hipHostMalloc(&p, b, flags));
        cap = b;
    }
    template <class T>
    T* as() const { return static_cast<T*>(p); }
};

}  // namespace mi
