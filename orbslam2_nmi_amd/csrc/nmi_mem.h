// nmi_mem.h -- internal: who owns device memory.  Move-only owners of a device buffer, a pinned host buffer, an event and a
// stream, whose destructors release what they hold, and the ring of small parameter uploads.  Runtime API only (no kernels,
// no device code): tests/native/device_memory.cpp compiles it with g++ against a runtime of its own.
//
// The grow rule (DeviceBuffer::grow, PinnedBuffer::grow): a request that fits is no HIP call at all.  Otherwise wait for
// `wait_on` if a buffer is held and a stream was given (a kernel in flight may still read it), free, become empty, allocate.
// Any failure -- of the free too -- leaves the object empty: nothing is ever left behind to be freed twice.  How much to ask
// for (floors, headroom) is the call site's business.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>

namespace nmi_mem {

class DeviceBuffer {
public:
    DeviceBuffer() = default;
    DeviceBuffer(DeviceBuffer &&o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr, o.bytes_ = 0; }
    DeviceBuffer &operator=(DeviceBuffer &&o) noexcept
    {
        if (this != &o) {
            (void)reset();
            p_ = o.p_, bytes_ = o.bytes_;
            o.p_ = nullptr, o.bytes_ = 0;
        }
        return *this;
    }
    ~DeviceBuffer() { (void)reset(); }
    template <class T = void> T *as() const { return static_cast<T *>(p_); }
    size_t size() const { return bytes_; }
    explicit operator bool() const { return p_ != nullptr; }
    hipError_t reset()
    {
        void *q = p_;
        p_ = nullptr, bytes_ = 0;
        return q ? hipFree(q) : hipSuccess;
    }
    hipError_t alloc(size_t bytes)
    {
        hipError_t e = reset();
        if (e == hipSuccess && (e = hipMalloc(&p_, bytes)) != hipSuccess) p_ = nullptr;
        if (e == hipSuccess) bytes_ = bytes;
        return e;
    }
    // zero: the new buffer is cleared on wait_on (which is then required), ordered before whatever that stream runs next
    hipError_t grow(size_t bytes, hipStream_t wait_on = nullptr, bool zero = false)
    {
        if (bytes <= bytes_) return hipSuccess;
        hipError_t e = p_ && wait_on ? hipStreamSynchronize(wait_on) : hipSuccess;
        const hipError_t freed = reset();
        if (e == hipSuccess) e = freed;
        if (e == hipSuccess) e = alloc(bytes);
        if (e == hipSuccess && zero && (e = hipMemsetAsync(p_, 0, bytes, wait_on)) != hipSuccess) (void)reset();
        return e;
    }

private:
    void *p_ = nullptr;
    size_t bytes_ = 0;
};

// Pinned host memory: kPinned for staging copies, kPosted (mapped, fine-grained) for words the device posts and the host polls
// or the other way round.  A mapped buffer's device address is looked up once, at allocation.
constexpr unsigned kPinned = hipHostMallocDefault, kPosted = hipHostMallocMapped | hipHostMallocCoherent;

class PinnedBuffer {
public:
    PinnedBuffer() = default;
    PinnedBuffer(PinnedBuffer &&o) noexcept : p_(o.p_), dev_(o.dev_), bytes_(o.bytes_) { o.p_ = o.dev_ = nullptr, o.bytes_ = 0; }
    PinnedBuffer &operator=(PinnedBuffer &&o) noexcept
    {
        if (this != &o) {
            (void)reset();
            p_ = o.p_, dev_ = o.dev_, bytes_ = o.bytes_;
            o.p_ = o.dev_ = nullptr, o.bytes_ = 0;
        }
        return *this;
    }
    ~PinnedBuffer() { (void)reset(); }
    template <class T = void> T *as() const { return static_cast<T *>(p_); }
    template <class T = void> T *device() const { return static_cast<T *>(dev_); }  // null unless mapped
    size_t size() const { return bytes_; }
    explicit operator bool() const { return p_ != nullptr; }
    hipError_t reset()
    {
        void *q = p_;
        p_ = dev_ = nullptr, bytes_ = 0;
        return q ? hipHostFree(q) : hipSuccess;
    }
    hipError_t alloc(size_t bytes, unsigned flags)
    {
        hipError_t e = reset();
        if (e == hipSuccess && (e = hipHostMalloc(&p_, bytes, flags)) != hipSuccess) p_ = nullptr;
        if (e == hipSuccess) bytes_ = bytes;
        if (e == hipSuccess && (flags & hipHostMallocMapped) && (e = hipHostGetDevicePointer(&dev_, p_, 0)) != hipSuccess) (void)reset();
        return e;
    }
    hipError_t grow(size_t bytes, unsigned flags, hipStream_t wait_on = nullptr)
    {
        if (bytes <= bytes_) return hipSuccess;
        hipError_t e = p_ && wait_on ? hipStreamSynchronize(wait_on) : hipSuccess;
        const hipError_t freed = reset();
        if (e == hipSuccess) e = freed;
        return e == hipSuccess ? alloc(bytes, flags) : e;
    }

private:
    void *p_ = nullptr, *dev_ = nullptr;
    size_t bytes_ = 0;
};

// hipEvent_t / hipStream_t, destroyed with their owner.  Both convert to the handle (null while empty).
template <class Handle, hipError_t (*Destroy)(Handle)> class Owned {
public:
    Owned() = default;
    Owned(Owned &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    Owned &operator=(Owned &&o) noexcept
    {
        if (this != &o) {
            (void)reset();
            h_ = o.h_;
            o.h_ = nullptr;
        }
        return *this;
    }
    ~Owned() { (void)reset(); }
    operator Handle() const { return h_; }
    hipError_t reset()
    {
        Handle q = h_;
        h_ = nullptr;
        return q ? Destroy(q) : hipSuccess;
    }
    hipError_t create(unsigned flags);  // only while empty

private:
    Handle h_ = nullptr;
};
using Event = Owned<hipEvent_t, hipEventDestroy>;
using Stream = Owned<hipStream_t, hipStreamDestroy>;
template <> inline hipError_t Event::create(unsigned flags) { return hipEventCreateWithFlags(&h_, flags); }
template <> inline hipError_t Stream::create(unsigned flags) { return hipStreamCreateWithFlags(&h_, flags); }

// Small host->device parameter uploads (inverse homographies, view matrices) go through a ring of (pinned staging, device
// copy, "consumed" event), so that back-to-back submissions never wait for the stream: a slot comes round again only after
// the work that read it.  acquire -> fill slot.h -> upload -> launch what reads slot.d -> release.
class UploadRing {
public:
    static constexpr int kSlots = 4;
    struct Slot {
        float *h = nullptr, *d = nullptr;
        size_t n = 0;
        hipEvent_t consumed = nullptr;
    };
    // n floats; all slots grow together (after a wait for `stream` when they exist), then the next slot's event is waited for
    hipError_t acquire(size_t n, hipStream_t stream, Slot *out)
    {
        if (n > cap_) {
            const bool held = cap_ != 0;
            cap_ = 0;
            hipError_t e = held ? hipStreamSynchronize(stream) : hipSuccess;
            for (Entry &s : slots_) {
                const hipError_t fd = s.d.reset(), fh = s.h.reset();
                if (e == hipSuccess) e = fd != hipSuccess ? fd : fh;
            }
            for (Entry &s : slots_) {
                if (e == hipSuccess) e = s.d.alloc(n * sizeof(float));
                if (e == hipSuccess) e = s.h.alloc(n * sizeof(float), kPinned);
                if (e == hipSuccess && !s.ev) e = s.ev.create(hipEventDisableTiming);
            }
            if (e != hipSuccess) return e;
            cap_ = n;
        }
        Entry &s = slots_[uses_++ % kSlots];
        *out = Slot{s.h.as<float>(), s.d.as<float>(), n, s.ev};
        return hipEventSynchronize(s.ev);
    }
    static hipError_t upload(const Slot &s, hipStream_t stream)
    {
        return hipMemcpyAsync(s.d, s.h, s.n * sizeof(float), hipMemcpyHostToDevice, stream);
    }
    static hipError_t release(const Slot &s, hipStream_t stream) { return hipEventRecord(s.consumed, stream); }

private:
    struct Entry {
        PinnedBuffer h;
        DeviceBuffer d;
        Event ev;
    };
    Entry slots_[kSlots];
    size_t cap_ = 0;  // floats per slot
    unsigned uses_ = 0;
};

}  // namespace nmi_mem
