// hip_owners.h -- the owners of the device resources and of the current device: the only places that allocate and release them, one
// owning type each, shared by the handle (gcsadmm.hip) and the scene of graph construction (polytope_lp.hip).  Host code only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <type_traits>

// The owners release in their destructors, so whoever destroys one has its device current (gcsadmm_destroy, gcsadmm_scene_destroy
// and the failure paths of the two creates hold the guard).
struct HipRelease {
    void operator()(void *p) const { (void)hipFree(p); }
    void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); }
    void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); }
};
using Stream = std::unique_ptr<std::remove_pointer_t<hipStream_t>, HipRelease>;
using Event = std::unique_ptr<std::remove_pointer_t<hipEvent_t>, HipRelease>;
// Copies: typed, counted in elements, the direction in the name.  A count of 0 or a null pointer (an array the caller does not want, a
// buffer the call never needed) copies nothing.
template <class T> hipError_t copy_elements(T *dst, const T *src, size_t count, hipMemcpyKind kind)
{
    return (count > 0 && dst && src) ? hipMemcpy(dst, src, sizeof(T) * count, kind) : hipSuccess;
}
template <class T> hipError_t to_device(T *dst, const T *src, size_t count) { return copy_elements(dst, src, count, hipMemcpyHostToDevice); }
template <class T> hipError_t to_host(T *dst, const T *src, size_t count) { return copy_elements(dst, src, count, hipMemcpyDeviceToHost); }
template <class T> hipError_t on_device(T *dst, const T *src, size_t count) { return copy_elements(dst, src, count, hipMemcpyDeviceToDevice); }

template <class T> class DevBuf {
    std::unique_ptr<T, HipRelease> p_;
    size_t count_ = 0;
public:
    T *get() const { return p_.get(); }
    size_t size() const { return p_ ? count_ : 0; }      // elements asked for (a count of 0 still allocates one)
    explicit operator bool() const { return (bool)p_; }
    void reset() { p_.reset(); }
    hipError_t alloc(size_t count)              // uninitialised
    {
        T *p = nullptr;
        const hipError_t e = hipMalloc((void **)&p, std::max<size_t>(count, 1) * sizeof(T));
        p_.reset(e == hipSuccess ? p : nullptr);
        count_ = count;
        return e;
    }
    hipError_t upload(const T *src, size_t count)      // src == nullptr: zero-filled
    {
        const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
        const hipError_t e = alloc(count);
        if (e != hipSuccess) return e;
        return src ? hipMemcpy(get(), src, bytes, hipMemcpyHostToDevice) : hipMemset(get(), 0, bytes);
    }
    hipError_t zero(hipStream_t s) const { return size() ? hipMemsetAsync(get(), 0, size() * sizeof(T), s) : hipSuccess; }
    // a new buffer with `count` host elements in it (reads none for a count of 0)
    hipError_t put(const T *src, size_t count) { const hipError_t e = alloc(count); return e == hipSuccess ? to_device(get(), src, count) : e; }
    // room for `count` elements in a buffer that is kept from call to call and only ever grows
    hipError_t reserve(size_t count) { return p_ && count_ >= count ? hipSuccess : (reset(), alloc(count)); }
};
template <class T> hipError_t to_host(T *dst, const DevBuf<T> &src) { return to_host(dst, src.get(), src.size()); }      // all of a buffer
// fills an empty Stream / Event through the HIP call that creates one with flags
template <class O> static hipError_t create_owned(O &owner, hipError_t (*create)(typename O::pointer *, unsigned), unsigned flags)
{
    typename O::pointer x = nullptr;
    const hipError_t e = create(&x, flags);
    owner.reset(x);
    return e;
}

// Entry points work on the handle's device and leave the caller's current device as they found it (a process may hold
// handles on several devices, and PyTorch tracks "its" current device on its own).
struct DeviceGuard {
    int prev = -1;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int dev)
    {
        int cur = -1;
        err = hipGetDevice(&cur);
        if (err == hipSuccess && cur != dev) { err = hipSetDevice(dev); if (err == hipSuccess) prev = cur; }
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};
