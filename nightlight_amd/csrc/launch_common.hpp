// launch_common.hpp -- what everything that launches a kernel shares (the launch_* functions of the stack passes and of
// the per-frame operators, find_stars_run, back_extract_run): the run-time -> template dispatch, one error path for
// everything a launcher enqueues, kernel names as rocprofv3 prints them, the lanes per pixel of the 129 ... 512-frame
// kernels, and the two inputs of a FastArgs pass.  Host code only.
#pragma once
#include <string>
#include <type_traits>
#include <utility>

#include "stack_kernels.h"

namespace nl {

// f(std::integral_constant<int, C>) for the first class C >= n; the last class takes everything above it
template <int C, int... MORE, class F>
decltype(auto) with_class(int n, F &&f)
{
    if constexpr (sizeof...(MORE) == 0) {
        return f(std::integral_constant<int, C>{});
    } else {
        if (n <= C) return f(std::integral_constant<int, C>{});
        return with_class<MORE...>(n, std::forward<F>(f));
    }
}

// f(std::bool_constant<b>): a run-time switch between two instantiations
template <class F>
decltype(auto) with_bool(bool b, F &&f)
{
    if (b) return f(std::true_type{});
    return f(std::false_type{});
}

// 129 ... 512 frames: f(std::integral_constant<int, LPP>) with LPP = 2 lanes per pixel up to 2 kMlNS frames, else 4
template <class F>
decltype(auto) with_ml_lanes(int n_frames, F &&f)
{
    if (n_frames <= 2 * kMlNS) return f(std::integral_constant<int, 2>{});
    return f(std::integral_constant<int, 4>{});
}

// 513 ... 2048 frames (include/nlstack_deepstack.h): LPP = 8 lanes per pixel up to 8 kMlNS frames, else 16
template <class F>
decltype(auto) with_deep_lanes(int n_frames, F &&f)
{
    if (n_frames <= 8 * kMlNS) return f(std::integral_constant<int, 8>{});
    return f(std::integral_constant<int, 16>{});
}

// workgroups of `block` threads over npix pixels at lpp lanes per pixel
inline unsigned pixel_grid(int64_t npix, int lpp = 1, int block = 256)
{
    const int64_t per_wg = block / lpp;
    return (unsigned)((npix + per_wg - 1) / per_wg);
}

// The kernels one launcher enqueues on one stream, and the first error of any of them: every launch and every event
// record is checked at once (hipGetLastError() also clears the error, so a check left for the end can miss one).
struct Launcher {
    hipStream_t stream;
    hipError_t err = hipSuccess;

    explicit Launcher(hipStream_t s) : stream(s) {}
    void keep(hipError_t e) { if (err == hipSuccess) err = e; }
    // dynamic LDS above 64 KiB needs the kernel's attribute raised first
    template <class... P, class... A>
    void operator()(void (*kernel)(P...), dim3 grid, unsigned block, size_t lds, A &&... args)
    {
        if (lds > 64 * 1024) {
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) { keep(e); return; }
        }
        hipLaunchKernelGGL(kernel, grid, dim3(block), lds, stream, std::forward<A>(args)...);
        keep(hipGetLastError());
    }
    void record(hipEvent_t event) { if (event) keep(hipEventRecord(event, stream)); }
};

// In a function that returns an NL_* code and reports through std::string *msg (find_stars_run, back_extract_run):
// leave with NL_ERR_HIP when a HIP call -- or, as NL_RUN_LAUNCHED(L), anything Launcher L enqueued -- failed
#define NL_RUN_CHECK(e, what)                                                                           \
    do {                                                                                                \
        hipError_t e_ = (e);                                                                            \
        if (e_ != hipSuccess) {                                                                         \
            *msg = std::string(what " failed: ") + hipGetErrorString(e_);                               \
            return NL_ERR_HIP;                                                                          \
        }                                                                                               \
    } while (0)
#define NL_RUN_HIP(call) NL_RUN_CHECK(call, #call)
#define NL_RUN_LAUNCHED(L) NL_RUN_CHECK((L).err, "hipGetLastError()")

template <class T>
std::string name_arg(T v)
{
    if constexpr (std::is_same_v<T, bool>) return v ? "true" : "false";
    else return std::to_string(v);
}

// "BASE<a, b, ...>", the name of the kernel BASE<ARGS...> as rocprofv3 prints it (what bench.py and the tests key on):
// built on first use, one function-local static per instantiation -- thread-safe (nl_group drives its tiles from worker
// threads) and valid for the library's life (handles keep the pointer as their last kernel's name)
template <const char *BASE, auto... ARGS>
const char *kernel_name()
{
    static const std::string name = [] {
        std::string s = BASE;
        const char *sep = "<";
        ((s += sep, s += name_arg(ARGS), sep = ", "), ...);
        return s + ">";
    }();
    return name.c_str();
}

// "BASE<a, b, ..., maps>" ("BASE<maps>" without arguments): the display name of a Form::Maps instantiation -- the default
// pass's name of the same kernel with "maps" as its last argument
template <const char *BASE, auto... ARGS>
const char *maps_kernel_name()
{
    static const std::string name = [] {
        std::string s = BASE;
        s += "<";
        ((s += name_arg(ARGS), s += ", "), ...);
        return s + "maps>";
    }();
    return name.c_str();
}

// a FastArgs pass over the whole tile / over the generic list (the pixels the dominant kernel handed over)
inline FastArgs whole_tile(FastArgs f)
{
    f.in_list = nullptr;
    f.in_count = nullptr;
    f.in_capacity = 0;
    return f;
}

inline FastArgs over_generic_list(FastArgs f)
{
    f.in_list = f.gen_list;
    f.in_count = f.gen_count;
    f.in_capacity = f.gen_capacity;
    return f;
}

}  // namespace nl
