// Device errors as exceptions, and the device allocations of one owner (a handle's loaded LP, a relp_many): every buffer is freed
// by free_all(), so no list of pointers has to follow the allocation sites.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <stdexcept>
#include <string>
#include <vector>

namespace relp {

struct DeviceError : std::runtime_error {
    explicit DeviceError(const std::string& what) : std::runtime_error(what) {}
};

#define RELP_HIP(call)                                                                                   \
    do {                                                                                                 \
        hipError_t err__ = (call);                                                                       \
        if (err__ != hipSuccess)                                                                         \
            throw ::relp::DeviceError(std::string(#call) + ": " + hipGetErrorString(err__));             \
    } while (0)

class DeviceAllocations {
public:
    DeviceAllocations() = default;
    DeviceAllocations(const DeviceAllocations&) = delete;
    DeviceAllocations& operator=(const DeviceAllocations&) = delete;
    template <class T>
    T* alloc(size_t count) {  // (never a zero-byte request: an empty array still has an address)
        const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
        ptrs_.reserve(ptrs_.size() + 1);  // so that nothing can throw between the allocation and its registration
        void* p = nullptr;
        RELP_HIP(hipMalloc(&p, bytes));
        ptrs_.push_back(p);
        bytes_ += bytes;
        return static_cast<T*>(p);
    }
    void free_all() {  // the owner's device must be current
        for (void* p : ptrs_) (void)hipFree(p);
        ptrs_.clear();
        bytes_ = 0;
    }
    size_t bytes() const { return bytes_; }

private:
    std::vector<void*> ptrs_;
    size_t bytes_ = 0;
};

// The pinned, host-mapped buffers of one owner: what the host and the device hand each other around the kernels (the mirror of
// the control block, the read-backs of a solve).  A copy to or from pageable memory is staged by the runtime through a copy
// kernel and blocks the caller; a copy to or from these is not, and a kernel may store into them directly.  Host memory: it
// does not count as device bytes.
class PinnedAllocations {
public:
    PinnedAllocations() = default;
    PinnedAllocations(const PinnedAllocations&) = delete;
    PinnedAllocations& operator=(const PinnedAllocations&) = delete;
    ~PinnedAllocations() { free_all(); }
    template <class T>
    T* alloc(size_t count) {
        const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
        ptrs_.reserve(ptrs_.size() + 1);
        void* p = nullptr;
        RELP_HIP(hipHostMalloc(&p, bytes, hipHostMallocMapped));
        ptrs_.push_back(p);
        return static_cast<T*>(p);
    }
    // the address a kernel uses for `host` (the owner's device must be current)
    template <class T>
    static T* device_pointer(T* host) {
        void* p = nullptr;
        RELP_HIP(hipHostGetDevicePointer(&p, host, 0));
        return static_cast<T*>(p);
    }
    void free_all() {
        for (void* p : ptrs_) (void)hipHostFree(p);
        ptrs_.clear();
    }

private:
    std::vector<void*> ptrs_;
};

}  // namespace relp
