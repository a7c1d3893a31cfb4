// common.h — error plumbing shared by the C-ABI translation units of libmi355clip.so.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <cstdio>
#include <string>

#include "error.h"

namespace mi {

void set_last_error(const std::string& m);

inline void hip_check(hipError_t e, const char* what, const char* file, int line) {
    if (e != hipSuccess) {
        int code = (e == hipErrorOutOfMemory) ? MI_ERR_OOM : MI_ERR_HIP;
        fail(code, "%s failed: %s (%s:%d)", what, hipGetErrorString(e), file, line);
    }
}
#define HIP_CHECK(x) ::mi::hip_check((x), #x, __FILE__, __LINE__)

// Every extern "C" body runs inside this: nothing may unwind across the ABI.
template <class F>
int guarded(F&& f) noexcept {
    try {
        f();
        return MI_OK;
    } catch (const Error& e) {
        set_last_error(e.what());
        return e.code;
    } catch (const std::bad_alloc&) {
        set_last_error("host allocation failed");
        return MI_ERR_OOM;
    } catch (const std::exception& e) {
        set_last_error(e.what());
        return MI_ERR_INVALID;
    } catch (...) {
        set_last_error("unknown error");
        return MI_ERR_INVALID;
    }
}

// what a public mi_* call made inside the library returned: its code and message go on as they are (`as`: the code to report
// in its place)
inline void call_ok(int e, int as = MI_OK) {
    if (e != MI_OK) fail(as != MI_OK ? as : e, "%s", mi_last_error());
}

// Select `device` and require it to be a gfx950 part: there is no fallback path.
void use_device(int device);

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int device) {
        (void)hipGetDevice(&prev);
        use_device(device);
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is per (device, function): one DevOnce per call site
// remembers which devices already have it (a second handle on another GPU of the same process, or two
// threads loading handles at once, must not skip it; setting it twice is harmless).
struct DevOnce {
    std::atomic<uint64_t> mask{0};
};
template <class K>
inline void allow_lds_once(DevOnce& once, K kernel, int bytes) {
    int dev = 0;
    HIP_CHECK(hipGetDevice(&dev));
    const uint64_t bit = 1ull << (dev & 63);
    if (once.mask.load(std::memory_order_acquire) & bit) return;
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    once.mask.fetch_or(bit, std::memory_order_release);
}

}  // namespace mi
