// device_mem.h — what a handle or a call holds of the runtime, each in an owner that gives it back: events (Event), streams
// (Stream), a handle's device arrays (DevArray), a bag of untyped device memory (Scratch: one call's, or a handle's weights and
// workspace) and pinned host memory (PinnedBuf).  hipFree / hipHostFree / hipEventDestroy find their device by themselves,
// whichever is selected when an owner goes out of scope.  No owner ever waits: whoever frees or replaces something that work
// in flight may still use waits first, where it does so.
#pragma once
#include <algorithm>
#include <utility>
#include <vector>

#include "common.h"

namespace mi {

// An event, created on first use.  It reads as the hipEvent_t it owns.
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; }
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    ~Event() {
        if (e) (void)hipEventDestroy(e);
    }
    operator hipEvent_t() const { return e; }
    // the event, created with `flags` by the first call (hipEventDefault: a timing event, through hipEventCreate)
    hipEvent_t get(unsigned flags) {
        if (!e) HIP_CHECK(flags == hipEventDefault ? hipEventCreate(&e) : hipEventCreateWithFlags(&e, flags));
        return e;
    }
};

// A stream, created on first use.  It reads as the hipStream_t it owns.  A stream is given back with its own device selected:
// the handles' free functions reset() theirs so, with the stream idle, and a stream that lives for one call goes with its scope,
// under the call's DeviceGuard.  The destructor of a handle's stream is a backstop only: nothing may rest on it.
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(Stream&& o) noexcept : s(o.s) { o.s = nullptr; }
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    ~Stream() { reset(); }
    operator hipStream_t() const { return s; }
    hipStream_t get(unsigned flags) {
        if (!s) HIP_CHECK(hipStreamCreateWithFlags(&s, flags));
        return s;
    }
    void reset() {
        if (s) (void)hipStreamDestroy(s);
        s = nullptr;
    }
};

// Order of the work of ONE handle across streams.  Every entry point that enqueues work which touches
// the handle's buffers calls begin(s) first (s waits for whatever the handle enqueued last, on any
// stream) and end(s) last.  Work on a handle therefore runs in call order whichever streams the
// callers pass; the host never blocks.  sync() is for the few places that free or move buffers.
struct WorkOrder {
    Event ev;
    bool pending = false;
    void begin(hipStream_t s) {
        if (pending) HIP_CHECK(hipStreamWaitEvent(s, ev, 0));
    }
    void end(hipStream_t s) {
        HIP_CHECK(hipEventRecord(ev.get(hipEventDisableTiming), s));
        pending = true;
    }
    void sync() {
        if (pending) HIP_CHECK(hipEventSynchronize(ev));
        pending = false;
    }
};

// A device array of `cap` elements of T.  It reads as the pointer it owns: kernel launches, copies and pointer arithmetic
// take the field as they would a T* (where a cast or a templated callee cannot see through the conversion: .p).
template <class T>
struct DevArray {
    T* p = nullptr;
    size_t cap = 0;
    DevArray() = default;
    DevArray(DevArray&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
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
    // room for n elements, the contents not kept; the caller has made sure that nothing in flight uses the old array
    void reserve(size_t n) {
        if (cap >= n) return;
        release();
        alloc(n);
    }
    // ... for callers with an order word.  Enough already: nothing is touched; otherwise whatever `order` counts (the
    // searches in flight, for a handle's workspace) has finished before the old array is freed
    void reserve(WorkOrder& order, size_t n) {
        if (cap >= n) return;
        order.sync();
        reserve(n);
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

// untyped device memory that goes together: one call's, freed on every way out, or what a handle keeps until it drops it all
struct Scratch {
    std::vector<void*> p;
    Scratch() = default;
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
    void* get(size_t bytes) { return exact(std::max<size_t>(bytes, 16)); }
    void* exact(size_t bytes) {
        void* q = nullptr;
        HIP_CHECK(hipMalloc(&q, bytes));
        p.push_back(q);
        return q;
    }
    // exactly `bytes`, filled with zeros on s (a workspace: the caller waits for s before the first use on another stream)
    void* zeroed(size_t bytes, hipStream_t s) {
        void* q = exact(bytes);
        HIP_CHECK(hipMemsetAsync(q, 0, bytes, s));
        return q;
    }
    // everything freed now; the caller has made sure that nothing in flight uses it
    void clear() {
        for (void* q : p) HIP_CHECK(hipFree(q));
        p.clear();
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
    PinnedBuf(PinnedBuf&& o) noexcept : p(o.p), cap(o.cap), flags(o.flags) { o.p = nullptr; o.cap = 0; }
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
