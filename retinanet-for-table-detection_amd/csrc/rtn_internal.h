// rtn_internal.h — shared by the librtn.so translation units (not part of the C-ABI): the handle, error and launch helpers
// (rtn_launch_lds, rtn_with_epi), environment knobs and the entry points one translation unit offers the others.  Device-only
// helpers are in rtn_device.h (descriptors, LDS-DMA, packers, the store-data guard) and rtn_conv_epilogue.h (the register epilogue
// of the persistent convolution kernels).
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <type_traits>
#include "rtn.h"
#include "rtn_conv_persistent.h"

struct rtn_ctx {
    int device;
    hipStream_t stream;
    void* zero_page;        // 256 B of zeros on the device: source for out-of-image taps
    int num_cus;
    int last_conv_streamk;        // rtn_debug_last_conv_streamk: workgroups of the last conv launch if it ran in stream-K form, else 0
    int last_conv_tile;           // rtn_debug_last_conv_tile: (tile rows << 16) | tile columns of the last conv launch
    int last_conv_impl;           // rtn_debug_last_conv_impl: kernel generation of the last conv launch on this handle
    int last_wgrad_impl;          // rtn_debug_last_wgrad_impl: 2 = 256x256 LDS-DMA, 3 = 128x128 LDS-DMA, 4 = rtn_wgrad_win.hip, 0 = register-staged
    char err[512];
};

inline int rtn_fail(rtn_ctx* h, int code, const char* fmt, ...) {
    if (h) {
        va_list ap; va_start(ap, fmt);
        vsnprintf(h->err, sizeof(h->err), fmt, ap);
        va_end(ap);
    }
    return code;
}

#define RTN_HIP(h, call)                                                                   \
    do {                                                                                   \
        hipError_t e_ = (call);                                                            \
        if (e_ != hipSuccess)                                                              \
            return rtn_fail((h), RTN_EHIP, "%s failed: %s (%s:%d)", #call,                 \
                            hipGetErrorString(e_), __FILE__, __LINE__);                    \
    } while (0)

#define RTN_CHECK_LAUNCH(h, name)                                                          \
    do {                                                                                   \
        hipError_t e_ = hipGetLastError();                                                 \
        if (e_ != hipSuccess)                                                              \
            return rtn_fail((h), RTN_EHIP, "launch of %s failed: %s", name,                \
                            hipGetErrorString(e_));                                        \
    } while (0)

// Launch `Kernel(args...)` with `lds` bytes of dynamic LDS on the handle's stream.  The first launch of a kernel instance on a device raises that
// instance's dynamic-LDS limit to `lds_limit` (the 64 KiB default refuses the launch).  The template is keyed on the kernel itself, so
// every instance owns a flag word, one bit per device.  The caller checks the launch (RTN_CHECK_LAUNCH).
template <auto Kernel, class... Args>
inline int rtn_launch_lds(rtn_ctx* h, dim3 grid, dim3 block, unsigned lds, int lds_limit, const Args&... args) {
    static std::atomic<unsigned long long> attr_set{0ull};
    const unsigned long long bit = 1ull << (h->device & 63);
    if (!(attr_set.load(std::memory_order_relaxed) & bit)) {
        RTN_HIP(h, hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_limit));
        attr_set.fetch_or(bit, std::memory_order_relaxed);
    }
    hipLaunchKernelGGL(Kernel, grid, block, lds, h->stream, args...);
    return RTN_OK;
}

// Run-time epilogue mode `epi` (bit 0 = residual, bit 1 = mask) -> compile-time constant: calls f(std::integral_constant<int, E>) for
// E = epi; `epi` >= LAST takes LAST (the instances a launcher has are E = 0 .. LAST, no others are emitted).
template <int LAST, int E = 0, class F>
inline int rtn_with_epi(int epi, F&& f) {
    if constexpr (E < LAST) {
        if (epi == E) return f(std::integral_constant<int, E>{});
        return rtn_with_epi<LAST, E + 1>(epi, f);
    } else {
        return f(std::integral_constant<int, LAST>{});
    }
}

// integer environment knob (name must be a string literal): cached per thread, re-read when the environment changed, so one process
// can still A/B kernel variants (tools/ab_conv.py).  rtn_env_sync() revalidates the cache: call it at the top of an entry point.
int rtn_env_int(const char* name, int dflt);
void rtn_env_sync();

// The persistent convolution kernels (generations 4 / 5 / 6).  rtn_conv_persistent.h decides, without HIP, whether a layer is theirs
// (*_takes) and on which tile, slices, grid and scratch it runs (*_choose); these entries fill the kernel's parameters from the call and
// that choice and launch.  `scratch`: the caller's workspace behind its sync block (`sync`), used as the choice says.
// RTN_OK = launched, < 0 = error.
int rtn_conv_halo8_run(rtn_handle_t h, const ConvCall& c, const H8Choice& ch, float* scratch);
int rtn_conv_gemm8_run(rtn_handle_t h, const ConvCall& c, const G8Choice& ch, unsigned* sync, void* scratch);
int rtn_conv_halon_run(rtn_handle_t h, const ConvCall& c, const HNChoice& ch);
// rtn_conv_ksplit.hip: sums the K-slice slabs of a conv launch in slice order and applies bias / ReLU
int rtn_conv_ksplit_finish(rtn_handle_t h, const float* slab, int S, long long M, int N, int ld, const float* bias, int relu, void* out,
                           int out_ld);

// rtn_wgrad.hip: the ordered reduction of the pixel splits of every weight-gradient kernel
struct rtn_wgrad_frag_t { int ncb, C, Ktot, wpt, co_tile; };   // slabs in the accumulator-fragment order of rtn_wgrad_win.hip (ncb > 0): waves per tile in the slab (8 / 4), filters per tile (128 / 64)
int rtn_wgrad_finish(rtn_handle_t h, float* dW, const float* slab, int S, long long NK, float* db, const float* bslab, int N, int db_n,
                     int bS = 0 /* parts of bslab when not S */, const rtn_wgrad_frag_t* frag = nullptr);
// rtn_wgrad_win.hip: all nine taps of a 128-filter x 64-channel block per workgroup over a sliding window of the input
size_t rtn_wgrad_win_workspace_bytes(const rtn_conv_desc_t* d);
int rtn_wgrad_win_try(rtn_handle_t h, const rtn_conv_desc_t* d, float* dW, float* db, int db_n, void* workspace, size_t workspace_bytes);

// rtn_elementwise.hip: text of the calling thread's last failed host-only call made without a handle (rtn_last_error(NULL))
const char* rtn_host_error_text();
// ... and sets it (the host-only entry points of the page codecs)
void rtn_set_host_error(const char* text);
// rtn_fail with a handle; without one the formatted message becomes the calling thread's host-error text
int rtn_fail_host(rtn_handle_t h, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));

static inline int rtn_dtype_size(int dt) { return dt == RTN_F32 ? 4 : (dt == RTN_FP8 ? 1 : 2); }

// log2 of a power of two, -1 for anything else
static inline int ilog2_exact(int v) {
    if (v <= 0 || (v & (v - 1))) return -1;
    int s = 0;
    while ((1 << s) < v) ++s;
    return s;
}

// workgroups of 256 threads for `work` items of a grid-stride loop: at least one, at most `cap`
static inline unsigned rtn_grid_for(long long work, int cap = 4096) {
    long long g = (work + 255) / 256;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (unsigned)g;
}

// bf16 helpers on raw bits (device + host)
__host__ __device__ static inline float rtn_bf16_to_f32(unsigned short b) {
    unsigned int u = ((unsigned int)b) << 16;
    float f;
#if defined(__HIP_DEVICE_COMPILE__)
    f = __uint_as_float(u);
#else
    memcpy(&f, &u, 4);
#endif
    return f;
}
