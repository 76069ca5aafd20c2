// buffers.hpp -- owning handles of the host layer's device and pinned memory: every buffer of a context (ctx.hpp), of a
// gather communicator (gather_rccl.cpp) and of a single call is one of these, released once, by its destructor.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

namespace emme {

// ---- ctx_cache.hip: the process-wide pool of node-cache buffers, and hipMalloc with one retry ----------------------
hipError_t pool_alloc(void** out, size_t bytes, int device);
hipError_t malloc_retry(void** out, size_t bytes);
void pool_free(void* p, size_t bytes, int device);

// T[] in device memory (through malloc_retry) or pinned host memory (hipHostMalloc).  grow(bytes) reallocates, to
// exactly `bytes`, when the buffer holds fewer; the old contents are not kept.
template <class T, bool Pinned>
class Buffer {
public:
    Buffer() = default;
    Buffer(const Buffer&) = delete;
    Buffer& operator=(const Buffer&) = delete;
    Buffer(Buffer&& o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
    Buffer& operator=(Buffer&& o) noexcept {
        std::swap(p_, o.p_), std::swap(bytes_, o.bytes_);
        return *this;
    }
    ~Buffer() { reset(); }

    hipError_t grow(size_t bytes) {
        if (bytes <= bytes_) return hipSuccess;
        reset();
        void* p = nullptr;
        const hipError_t e = Pinned ? hipHostMalloc(&p, bytes) : malloc_retry(&p, bytes);
        if (e == hipSuccess) p_ = static_cast<T*>(p), bytes_ = bytes;
        return e;
    }
    void reset() {
        if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr, bytes_ = 0;
    }
    operator T*() const { return p_; }
    T* get() const { return p_; }
    size_t bytes() const { return bytes_; }

private:
    T* p_ = nullptr;
    size_t bytes_ = 0;
};
template <class T = void>
using DeviceBuffer = Buffer<T, false>;
template <class T = void>
using PinnedBuffer = Buffer<T, true>;

// Node-cache records: memory from the process-wide pool, handed back to it (not to the driver) on release.
class PooledBuffer {
public:
    PooledBuffer() = default;
    PooledBuffer(const PooledBuffer&) = delete;
    PooledBuffer& operator=(const PooledBuffer&) = delete;
    ~PooledBuffer() { reset(); }

    hipError_t alloc(size_t bytes, int device) {
        reset();
        void* p = nullptr;
        const hipError_t e = pool_alloc(&p, bytes, device);
        if (e == hipSuccess) p_ = p, bytes_ = bytes, device_ = device;
        return e;
    }
    void reset() {
        pool_free(p_, bytes_, device_);
        p_ = nullptr, bytes_ = 0;
    }
    operator void*() const { return p_; }

private:
    void* p_ = nullptr;
    size_t bytes_ = 0;
    int device_ = 0;
};

// Pinned staging of the small per-launch index lists (omega order | chunk table | position map of a fill, the live
// matrices of an LU).  The host fills a slot; launch_stage_ints copies it to device memory later, in stream order.  A
// slot is written again only once the event recorded behind that copy has completed.  With at least as many slots as
// lists are staged between two synchronisations of the stream (a Newton step stages three), that wait returns at once.
class StagingRing {
public:
    static constexpr int kSlots = 4;
    StagingRing() = default;
    StagingRing(const StagingRing&) = delete;
    StagingRing& operator=(const StagingRing&) = delete;
    ~StagingRing() {
        (void)wait_all();
        for (hipEvent_t e : ev_)
            if (e) (void)hipEventDestroy(e);
    }

    // slots of at least `ints` integers each
    hipError_t reserve(size_t ints) {
        if (ints <= slot_ints_) return hipSuccess;
        for (hipEvent_t& e : ev_)
            if (!e) {
                const hipError_t r = hipEventCreateWithFlags(&e, hipEventDisableTiming);
                if (r != hipSuccess) return r;
            }
        hipError_t e = wait_all();  // (the old block is freed: nothing may still read it)
        slot_ints_ = 0;
        if (e == hipSuccess) e = mem_.grow(sizeof(int) * kSlots * ints);
        if (e == hipSuccess) slot_ints_ = ints;
        return e;
    }
    // the next slot, for `ints` integers, once the device has read what it held before
    hipError_t take(size_t ints, int** slot) {
        if (ints > slot_ints_) return hipErrorInvalidValue;
        const int k = (int)(next_++ % kSlots);
        if (recorded_[k]) {
            const hipError_t e = hipEventSynchronize(ev_[k]);
            if (e != hipSuccess) return e;
            recorded_[k] = false;
        }
        taken_ = k;
        *slot = mem_ + (size_t)k * slot_ints_;
        return hipSuccess;
    }
    // after the launch on `stream` that reads the slot last taken
    hipError_t read_on(hipStream_t stream) {
        const hipError_t e = hipEventRecord(ev_[taken_], stream);
        recorded_[taken_] = e == hipSuccess;
        return e;
    }

private:
    hipError_t wait_all() {
        hipError_t r = hipSuccess;
        for (int k = 0; k < kSlots; ++k)
            if (recorded_[k]) {
                const hipError_t e = hipEventSynchronize(ev_[k]);
                if (e != hipSuccess) r = e;
                recorded_[k] = false;
            }
        return r;
    }

    PinnedBuffer<int> mem_;
    size_t slot_ints_ = 0;
    hipEvent_t ev_[kSlots] = {};
    bool recorded_[kSlots] = {};
    unsigned int next_ = 0;
    int taken_ = 0;
};

}  // namespace emme
