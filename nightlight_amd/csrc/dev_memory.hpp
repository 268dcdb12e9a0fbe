// dev_memory.hpp -- the library's device allocations and the scratch types built on them: the allocator (defined in
// nlstack_api.hip), a buffer grown on demand, a block parked between handles, and the carving of one allocation
// into arrays.  Host code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace nl {

// EVERY device allocation of the library goes through dev_malloc (it hands parked blocks back when HIP runs out);
// cached_malloc / cached_free park large blocks for the next handle of the same sizes (the caller has selected `device`)
hipError_t dev_malloc(void **p, size_t bytes);
template <class T>
hipError_t dev_malloc(T **p, size_t bytes) { return dev_malloc(reinterpret_cast<void **>(p), bytes); }
hipError_t cached_malloc(void **p, size_t bytes, int device);
void cached_free(void *p, size_t bytes, int device);

// device scratch grown on demand, never shrunk: the old buffer goes only once `stream`, its last user, is idle
struct DevBuffer {
    void *ptr = nullptr;
    size_t bytes = 0;
    hipError_t reserve(size_t want, hipStream_t stream);
    void release() { if (ptr) (void)hipFree(ptr); ptr = nullptr; bytes = 0; }
};

// device scratch of one size for the life of its handle, taken from and returned to the parked blocks
struct ParkedBuffer {
    void *ptr = nullptr;
    size_t bytes = 0;
    hipError_t reserve(size_t want, int device)
    {
        if (ptr) return hipSuccess;
        const hipError_t e = cached_malloc(&ptr, want, device);
        if (e == hipSuccess) bytes = want;
        return e;
    }
    void release(int device) { cached_free(ptr, bytes, device); ptr = nullptr; bytes = 0; }
};

constexpr size_t align_up(size_t b) { return (b + 255) & ~(size_t)255; }

// One allocation carved into arrays, each starting on a 256-byte boundary: take<T>(count) in layout order, then
// bytes() is the end of the last array.  Over a null base it only measures (every take gives nullptr).
struct Carver {
    char *base;
    size_t end = 0;
    explicit Carver(void *b) : base(static_cast<char *>(b)) {}
    template <class T>
    T *take(size_t count)
    {
        const size_t at = align_up(end);
        end = at + sizeof(T) * count;
        return base ? reinterpret_cast<T *>(base + at) : nullptr;
    }
    size_t bytes() const { return end; }
};

}  // namespace nl
