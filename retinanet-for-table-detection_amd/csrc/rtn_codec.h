// rtn_codec.h — what the seven page-codec files (rtn_jpeg.hip, rtn_jpeg_enc.hip, rtn_png_enc.hip, rtn_png_dec.hip, rtn_png_stream.hip,
// rtn_tiff.hip, rtn_tiff_enc.hip) and the page-analysis files share, device and host; the codec entries' host side: rtn_codec_launch.h.
#pragma once
#include <hip/hip_runtime.h>

constexpr int RTN_CODEC_BATCH = 32;            // pages per launch (kernel-argument table)

inline long long rtn_align256(long long v) { return (v + 255) & ~255LL; }

// in-place exclusive scan of one value per thread over a workgroup of THREADS; returns the total
template <int THREADS, typename T>
__device__ inline T rtn_wg_exclusive_scan(T* sh, T& v) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int d = 1; d < THREADS; d <<= 1) {
        const T a = t >= d ? sh[t - d] : (T)0;
        __syncthreads();
        sh[t] += a;
        __syncthreads();
    }
    const T total = sh[THREADS - 1];
    v = sh[t] - v;
    __syncthreads();
    return total;
}
