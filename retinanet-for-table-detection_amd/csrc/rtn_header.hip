// rtn_header.hip — header detection on the device (HeaderDetect.py main()): four launches per batch of table crops.
//
//   sample_kernel    one thread per destination pixel: the exact box resample to 500 x dh, then cv2's 8-bit BGR2HSV.
//   cluster_kernel   the hot path.  One workgroup of 512 threads per crop runs k = 1 .. 9 in a chain; no workgroup waits on another.
//                    A pass gives each thread four points at a time (three dwords of H,S,V, one dword of labels), keeps the sums
//                    of the first K clusters in registers (the pass is a template on K), adds them across the wave with
//                    shuffles and then into LDS with one integer atomic per wave and sum.  Every sum is an integer: the result
//                    does not depend on the order of the adds.  Thread 0 turns the sums into centres and splits a cluster for
//                    the next k.  Every loop is bounded by max_iter and N, every barrier is reached by all threads (the
//                    "changed" flag is read from LDS by all between two barriers).
//   stats_kernel     one workgroup per crop: 9 x 3 x 256 histograms of the chosen k in LDS (integer atomics), written once.
//   patches_kernel   one thread per patch pixel: the 3x3 in-range test and cv2's 8-bit HSV2BGR.
// The per-element rules are the text the CPU twins run (rtn_header.h).
#include <algorithm>
#include <vector>
#include "rtn_page_launch.h"
#include "rtn_header.h"

namespace {

// ---- kernels --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HDR_PIX_THREADS) void sample_kernel(const HCrop* crops, uint8_t* hsv) {
    const HCrop c = crops[blockIdx.y];
    const int64_t i = (int64_t)blockIdx.x * HDR_PIX_THREADS + threadIdx.x;
    if (i < (int64_t)c.dh * HDR_W) hdr_sample_point(c, i, hsv);
}

template <typename T>
__device__ inline T wave_sum(T v) {
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// one assignment pass over the crop's points: labels, "did any label change", and the sums of the new labels into `acc`
template <int K>
__device__ inline void assign_pass(const uint32_t* pts, uint32_t* lab, int groups, bool first, const float* cen_sh, HAcc* acc,
                                   int* changed) {
    float cen[3 * K];
#pragma unroll
    for (int i = 0; i < 3 * K; ++i) cen[i] = cen_sh[i];
    uint32_t n[K], s[K][3], q[K][3];               // q per thread: <= 4096 points * 255^2 < 2^32
#pragma unroll
    for (int c = 0; c < K; ++c) {
        n[c] = 0;
#pragma unroll
        for (int j = 0; j < 3; ++j) s[c][j] = q[c][j] = 0;
    }
    bool ch = false;
    for (int g = threadIdx.x; g < groups; g += HDR_THREADS) {
        const uint32_t w0 = pts[3 * g], w1 = pts[3 * g + 1], w2 = pts[3 * g + 2];
        const uint32_t b[12] = {w0 & 255, (w0 >> 8) & 255, (w0 >> 16) & 255, w0 >> 24, w1 & 255, (w1 >> 8) & 255,
                                (w1 >> 16) & 255, w1 >> 24, w2 & 255, (w2 >> 8) & 255, (w2 >> 16) & 255, w2 >> 24};
        uint32_t neu = 0;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            float d;
            const uint32_t H = b[3 * p], S = b[3 * p + 1], V = b[3 * p + 2];
            const int best = hdr_nearest<K>((int)H, (int)S, (int)V, cen, &d);
            neu |= (uint32_t)best << (8 * p);
#pragma unroll
            for (int c = 0; c < K; ++c) {
                const bool m = best == c;
                n[c] += m ? 1u : 0u;
                s[c][0] += m ? H : 0u; s[c][1] += m ? S : 0u; s[c][2] += m ? V : 0u;
                q[c][0] += m ? H * H : 0u; q[c][1] += m ? S * S : 0u; q[c][2] += m ? V * V : 0u;
            }
        }
        if (first || lab[g] != neu) { ch = true; lab[g] = neu; }
    }
    const bool lane0 = (threadIdx.x & 63) == 0;
#pragma unroll
    for (int c = 0; c < K; ++c) {
        const uint32_t nn = wave_sum(n[c]);
        if (lane0 && nn) atomicAdd(&acc->n[c], nn);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const uint32_t ss = wave_sum(s[c][j]);
            const unsigned long long qq = wave_sum((unsigned long long)q[c][j]);
            if (lane0 && nn) {
                atomicAdd(&acc->s[c][j], ss);
                atomicAdd(reinterpret_cast<unsigned long long*>(&acc->q[c][j]), qq);
            }
        }
    }
    if (__any(ch) && lane0) atomicOr(changed, 1);
}

template <int K>
__device__ inline void distortion_pass(const uint32_t* pts, int groups, const float* cen_sh, unsigned long long* dsum) {
    float cen[3 * K];
#pragma unroll
    for (int i = 0; i < 3 * K; ++i) cen[i] = cen_sh[i];
    unsigned long long sum = 0;
    for (int g = threadIdx.x; g < groups; g += HDR_THREADS) {
        const uint32_t w0 = pts[3 * g], w1 = pts[3 * g + 1], w2 = pts[3 * g + 2];
        const uint32_t b[12] = {w0 & 255, (w0 >> 8) & 255, (w0 >> 16) & 255, w0 >> 24, w1 & 255, (w1 >> 8) & 255,
                                (w1 >> 16) & 255, w1 >> 24, w2 & 255, (w2 >> 8) & 255, (w2 >> 16) & 255, w2 >> 24};
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            float d;
            hdr_nearest<K>((int)b[3 * p], (int)b[3 * p + 1], (int)b[3 * p + 2], cen, &d);
            sum += hdr_distortion_fx(d);
        }
    }
    sum = wave_sum(sum);
    if ((threadIdx.x & 63) == 0) atomicAdd(dsum, sum);
}

__global__ __launch_bounds__(HDR_THREADS) void cluster_kernel(const HCrop* crops, const uint8_t* hsv, int max_iter, float* centres,
                                                              uint32_t* counts, int32_t* passes, uint64_t* distortion,
                                                              uint8_t* labels) {
    __shared__ HAcc acc;
    __shared__ float cen[3 * HDR_K];
    __shared__ unsigned long long dsum;
    __shared__ int changed;
    const int tid = threadIdx.x, crop = blockIdx.x;
    const HCrop c = crops[crop];
    const int N = c.dh * HDR_W, groups = N / 4;
    const uint32_t* pts = reinterpret_cast<const uint32_t*>(hsv + 3 * c.off);
    for (int k = 1; k <= HDR_K; ++k) {                                   // k is uniform: every barrier below is reached by all
        uint32_t* lab = reinterpret_cast<uint32_t*>(labels + HDR_K * c.off + (int64_t)(k - 1) * N);
        if (tid == 0) {
            if (k == 1) cen[0] = cen[1] = cen[2] = 0.0f;
            else hdr_split(acc, k - 1, cen);
            dsum = 0;
        }
        __syncthreads();
        int used = 0;
        for (int pass = 1; pass <= max_iter; ++pass) {
            for (int i = tid; i < (int)(sizeof(HAcc) / 4); i += HDR_THREADS) reinterpret_cast<uint32_t*>(&acc)[i] = 0;
            if (tid == 0) changed = 0;
            __syncthreads();
#define HDR_ASSIGN(K) assign_pass<K>(pts, lab, groups, pass == 1, cen, &acc, &changed)
            HDR_DISPATCH_K(k, HDR_ASSIGN)
#undef HDR_ASSIGN
            __syncthreads();
            const int chg = changed;
            if (tid == 0) hdr_update_centres(acc, k, cen);
            used = pass;
            __syncthreads();
            if (!chg) break;                                             // uniform: `changed` was read between two barriers
        }
#define HDR_DISTORTION(K) distortion_pass<K>(pts, groups, cen, &dsum)
        HDR_DISPATCH_K(k, HDR_DISTORTION)
#undef HDR_DISTORTION
        __syncthreads();
        const size_t row = (size_t)crop * HDR_K + (k - 1);
        if (tid < 3 * HDR_K) centres[row * 3 * HDR_K + tid] = tid < 3 * k ? cen[tid] : 0.0f;
        if (tid < HDR_K) counts[row * HDR_K + tid] = tid < k ? acc.n[tid] : 0u;
        if (tid == 0) {
            passes[row] = used;
            distortion[row] = dsum;
        }
        __syncthreads();                                                 // before thread 0 splits for k + 1
    }
}

__global__ __launch_bounds__(HDR_THREADS) void stats_kernel(const HCrop* crops, const uint8_t* hsv, const uint8_t* labels,
                                                            uint32_t* hist) {
    __shared__ uint32_t sh[HDR_K * 3 * 256];
    const int tid = threadIdx.x;
    const HCrop c = crops[blockIdx.x];
    const int N = c.dh * HDR_W, groups = N / 4;
    const uint32_t* pts = reinterpret_cast<const uint32_t*>(hsv + 3 * c.off);
    const uint32_t* lab = reinterpret_cast<const uint32_t*>(labels + HDR_K * c.off + (int64_t)(c.k - 1) * N);
    for (int i = tid; i < HDR_K * 3 * 256; i += HDR_THREADS) sh[i] = 0;
    __syncthreads();
    for (int g = tid; g < groups; g += HDR_THREADS) {
        const uint32_t w[3] = {pts[3 * g], pts[3 * g + 1], pts[3 * g + 2]};
        const uint32_t l4 = lab[g];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const uint32_t l = (l4 >> (8 * p)) & 255;
            if (l >= (uint32_t)c.k) continue;                           // labels are the caller's memory: never index past the table
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int byte = 3 * p + j;
                atomicAdd(&sh[(l * 3 + j) * 256 + ((w[byte >> 2] >> (8 * (byte & 3))) & 255)], 1u);
            }
        }
    }
    __syncthreads();
    uint32_t* out = hist + (size_t)blockIdx.x * HDR_K * 3 * 256;
    for (int i = tid; i < HDR_K * 3 * 256; i += HDR_THREADS) out[i] = sh[i];
}

__global__ __launch_bounds__(HDR_PIX_THREADS) void patches_kernel(const HCrop* crops, const HPatch* patches, const uint8_t* hsv,
                                                                  uint8_t* out) {
    const HPatch p = patches[blockIdx.y];
    const HCrop c = crops[p.crop];
    const int64_t i = (int64_t)blockIdx.x * HDR_PIX_THREADS + threadIdx.x;
    if (i >= (int64_t)c.dh * HDR_W) return;
    hdr_patch_pixel(hsv + 3 * c.off, c.dh, (int)(i / HDR_W), (int)(i % HDR_W), p.lo, p.hi, out + p.out_off + 3 * i);
}

// ---- argument checks and tables -------------------------------------------------------------------------------------------------
struct HPlan {
    std::vector<HCrop> crops;
    std::vector<HPatch> patches;
    int64_t points = 0;
    int max_dh = 0;
};

// `align`: 3 for the device entries, whose kernels read dwords; 0 for the twins
const char* plan_crops(int n, const int32_t* dst_heights, const int64_t* offsets, size_t hsv_bytes, const void* hsv, HPlan* pl,
                       unsigned align) {
    if (const char* why = hdr_check_layout(n, dst_heights, offsets, hsv_bytes)) return why;
    if (n && (!hsv || ((uintptr_t)hsv & align))) return "a 4-byte aligned H,S,V buffer expected";
    pl->crops.resize((size_t)n);
    for (int i = 0; i < n; ++i) {
        pl->crops[i] = HCrop{nullptr, offsets[i], 0, 0, dst_heights[i], 0};
        pl->points += (int64_t)dst_heights[i] * HDR_W;
        pl->max_dh = std::max(pl->max_dh, dst_heights[i]);
    }
    return nullptr;
}

const char* plan_sample(int n, const uint8_t* const* crops, const int32_t* heights, const int32_t* widths, HPlan* pl) {
    if (n && (!crops || !heights || !widths)) return "the crops with their heights and widths expected";
    for (int i = 0; i < n; ++i) {
        const int h = heights[i], w = widths[i];
        if (!crops[i] || h < 1 || w < 1 || h > HDR_MAX_SIDE || w > HDR_MAX_SIDE) return "a crop is missing or has a side outside 1 .. 65500";
        if ((int)((double)h * (500.0 / (double)w)) != pl->crops[i].dh) return "a destination height is not int(h * (500 / w))";
        pl->crops[i].src = crops[i];
        pl->crops[i].h = h;
        pl->crops[i].w = w;
    }
    return nullptr;
}

const char* plan_labels(const HPlan& pl, const void* labels, size_t labels_bytes, unsigned align) {
    if (pl.crops.empty()) return nullptr;
    if (!labels || ((uintptr_t)labels & align)) return "a 4-byte aligned labels buffer expected";
    if ((uint64_t)pl.points * HDR_K > labels_bytes) return "the labels buffer is smaller than 9 bytes per point";
    return nullptr;
}

const char* plan_ks(const int32_t* ks, HPlan* pl) {
    if (!pl->crops.empty() && !ks) return "the chosen k of every crop expected";
    for (size_t i = 0; i < pl->crops.size(); ++i) {
        if (ks[i] < 1 || ks[i] > HDR_K) return "a chosen k is outside 1 .. RTN_HEADER_MAX_K";
        pl->crops[i].k = ks[i];
    }
    return nullptr;
}

const char* plan_patches(int n_patches, const int32_t* patch_crop, const uint8_t* low, const uint8_t* high,
                         const int64_t* out_offsets, const void* out, size_t out_bytes, HPlan* pl) {
    if (n_patches < 0 || (n_patches && (!patch_crop || !low || !high || !out_offsets || !out))) return "n_patches patches with their tables and an output buffer expected";
    pl->patches.resize((size_t)n_patches);
    int64_t pos = 0;
    for (int i = 0; i < n_patches; ++i) {
        if (patch_crop[i] < 0 || (size_t)patch_crop[i] >= pl->crops.size()) return "a patch names a crop outside the batch";
        if (out_offsets[i] < pos) return "patch offsets must increase without overlap";
        HPatch& p = pl->patches[i];
        memset(&p, 0, sizeof(p));
        p.out_off = out_offsets[i];
        p.crop = patch_crop[i];
        for (int j = 0; j < 3; ++j) { p.lo[j] = low[3 * i + j]; p.hi[j] = high[3 * i + j]; }
        pos = out_offsets[i] + (int64_t)pl->crops[p.crop].dh * HDR_W * 3;
        if ((uint64_t)pos > out_bytes) return "a patch ends past the output buffer";
    }
    return nullptr;
}

// the workspace: the crop table at 0, then the patch table -> the patch table's offset; with a plan, its two tables are staged
size_t ws_layout(rtn_stage& st, size_t n_crops, size_t n_patches, const HPlan* pl) {
    const size_t crops = st.reserve((int64_t)(n_crops * sizeof(HCrop))), patches = st.reserve((int64_t)(n_patches * sizeof(HPatch)));
    if (pl) {
        st.put(crops, pl->crops);
        st.put(patches, pl->patches);
    }
    return patches;
}

unsigned pixel_blocks(const HPlan& pl) { return (unsigned)(((int64_t)pl.max_dh * HDR_W + HDR_PIX_THREADS - 1) / HDR_PIX_THREADS); }

}  // namespace

// rtn_header_*: see include/rtn.h
extern "C" size_t rtn_header_workspace_bytes(int n_crops, int n_patches) {
    if (n_crops < 0 || n_patches < 0) return 0;
    rtn_stage st;
    ws_layout(st, (size_t)n_crops, (size_t)n_patches, nullptr);
    return st.bytes();
}

extern "C" int rtn_header_sample(rtn_handle_t h, int n, const uint8_t* const* crops, const int32_t* heights, const int32_t* widths,
                                 const int32_t* dst_heights, const int64_t* offsets, uint8_t* hsv, size_t hsv_bytes, void* workspace,
                                 size_t workspace_bytes) {
    if (!h) return RTN_EINVAL;
    HPlan pl;
    RTN_PLAN(h, "rtn_header_sample", plan_crops(n, dst_heights, offsets, hsv_bytes, hsv, &pl, 3));
    RTN_PLAN(h, "rtn_header_sample", plan_sample(n, crops, heights, widths, &pl));
    if (n == 0) return RTN_OK;
    rtn_stage st;
    ws_layout(st, pl.crops.size(), pl.patches.size(), &pl);
    if (const int rc = st.commit(h, "rtn_header_sample", workspace, workspace_bytes)) return rc;
    const HCrop* t = st.at<const HCrop>(0);
    sample_kernel<<<dim3(pixel_blocks(pl), (unsigned)n), dim3(HDR_PIX_THREADS), 0, h->stream>>>(t, hsv);
    RTN_CHECK_LAUNCH(h, "sample_kernel");
    return RTN_OK;
}

extern "C" int rtn_header_cluster(rtn_handle_t h, int n, const int32_t* dst_heights, const int64_t* offsets, const uint8_t* hsv,
                                  size_t hsv_bytes, int max_iter, float* centres, uint32_t* counts, int32_t* passes,
                                  uint64_t* distortion_fx, uint8_t* labels, size_t labels_bytes, void* workspace,
                                  size_t workspace_bytes) {
    if (!h) return RTN_EINVAL;
    HPlan pl;
    RTN_PLAN(h, "rtn_header_cluster", plan_crops(n, dst_heights, offsets, hsv_bytes, hsv, &pl, 3));
    RTN_PLAN(h, "rtn_header_cluster", plan_labels(pl, labels, labels_bytes, 3));
    if (max_iter < 1 || (n && (!centres || !counts || !passes || !distortion_fx)))
        return rtn_fail(h, RTN_EINVAL, "rtn_header_cluster: max_iter >= 1 and the four per-k outputs expected");
    if (n == 0) return RTN_OK;
    rtn_stage st;
    ws_layout(st, pl.crops.size(), pl.patches.size(), &pl);
    if (const int rc = st.commit(h, "rtn_header_cluster", workspace, workspace_bytes)) return rc;
    const HCrop* t = st.at<const HCrop>(0);
    cluster_kernel<<<dim3((unsigned)n), dim3(HDR_THREADS), 0, h->stream>>>(t, hsv, max_iter, centres, counts, passes, distortion_fx, labels);
    RTN_CHECK_LAUNCH(h, "cluster_kernel");
    return RTN_OK;
}

extern "C" int rtn_header_stats(rtn_handle_t h, int n, const int32_t* dst_heights, const int64_t* offsets, const int32_t* ks,
                                const uint8_t* hsv, size_t hsv_bytes, const uint8_t* labels, size_t labels_bytes, uint32_t* hist,
                                void* workspace, size_t workspace_bytes) {
    if (!h) return RTN_EINVAL;
    HPlan pl;
    RTN_PLAN(h, "rtn_header_stats", plan_crops(n, dst_heights, offsets, hsv_bytes, hsv, &pl, 3));
    RTN_PLAN(h, "rtn_header_stats", plan_labels(pl, labels, labels_bytes, 3));
    RTN_PLAN(h, "rtn_header_stats", plan_ks(ks, &pl));
    if (n && !hist) return rtn_fail(h, RTN_EINVAL, "rtn_header_stats: the histogram output expected");
    if (n == 0) return RTN_OK;
    rtn_stage st;
    ws_layout(st, pl.crops.size(), pl.patches.size(), &pl);
    if (const int rc = st.commit(h, "rtn_header_stats", workspace, workspace_bytes)) return rc;
    const HCrop* t = st.at<const HCrop>(0);
    stats_kernel<<<dim3((unsigned)n), dim3(HDR_THREADS), 0, h->stream>>>(t, hsv, labels, hist);
    RTN_CHECK_LAUNCH(h, "stats_kernel");
    return RTN_OK;
}

extern "C" int rtn_header_patches(rtn_handle_t h, int n, const int32_t* dst_heights, const int64_t* offsets, const uint8_t* hsv,
                                  size_t hsv_bytes, int n_patches, const int32_t* patch_crop, const uint8_t* low, const uint8_t* high,
                                  const int64_t* out_offsets, uint8_t* out, size_t out_bytes, void* workspace,
                                  size_t workspace_bytes) {
    if (!h) return RTN_EINVAL;
    HPlan pl;
    RTN_PLAN(h, "rtn_header_patches", plan_crops(n, dst_heights, offsets, hsv_bytes, hsv, &pl, 3));
    RTN_PLAN(h, "rtn_header_patches", plan_patches(n_patches, patch_crop, low, high, out_offsets, out, out_bytes, &pl));
    if (n_patches == 0) return RTN_OK;
    rtn_stage st;
    const size_t off_patches = ws_layout(st, pl.crops.size(), pl.patches.size(), &pl);
    if (const int rc = st.commit(h, "rtn_header_patches", workspace, workspace_bytes)) return rc;
    const HCrop* t = st.at<const HCrop>(0);
    const HPatch* tp = st.at<const HPatch>(off_patches);
    patches_kernel<<<dim3(pixel_blocks(pl), (unsigned)n_patches), dim3(HDR_PIX_THREADS), 0, h->stream>>>(t, tp, hsv, out);
    RTN_CHECK_LAUNCH(h, "patches_kernel");
    return RTN_OK;
}

// ---- the CPU twins: host pointers, no handle, the same header functions ----------------------------------------------------------
extern "C" int rtn_header_sample_host(int n, const uint8_t* const* crops, const int32_t* heights, const int32_t* widths,
                                      const int32_t* dst_heights, const int64_t* offsets, uint8_t* hsv, size_t hsv_bytes) {
    HPlan pl;
    RTN_PLAN(nullptr, "rtn_header_sample_host", plan_crops(n, dst_heights, offsets, hsv_bytes, hsv, &pl, 0));
    RTN_PLAN(nullptr, "rtn_header_sample_host", plan_sample(n, crops, heights, widths, &pl));
    for (const HCrop& c : pl.crops)
        for (int64_t i = 0; i < (int64_t)c.dh * HDR_W; ++i) hdr_sample_point(c, i, hsv);
    return RTN_OK;
}

extern "C" int rtn_header_cluster_host(int n, const int32_t* dst_heights, const int64_t* offsets, const uint8_t* hsv, size_t hsv_bytes,
                                       int max_iter, float* centres, uint32_t* counts, int32_t* passes, uint64_t* distortion_fx,
                                       uint8_t* labels, size_t labels_bytes) {
    HPlan pl;
    RTN_PLAN(nullptr, "rtn_header_cluster_host", plan_crops(n, dst_heights, offsets, hsv_bytes, hsv, &pl, 0));
    RTN_PLAN(nullptr, "rtn_header_cluster_host", plan_labels(pl, labels, labels_bytes, 0));
    if (max_iter < 1 || (n && (!centres || !counts || !passes || !distortion_fx)))
        return rtn_fail_host(nullptr, RTN_EINVAL, "rtn_header_cluster_host: max_iter >= 1 and the four per-k outputs expected");
    for (int i = 0; i < n; ++i) {
        const HCrop& c = pl.crops[i];
        cluster_crop_host(hsv + 3 * c.off, c.dh * HDR_W, max_iter, centres + (size_t)i * HDR_K * HDR_K * 3,
                          counts + (size_t)i * HDR_K * HDR_K, passes + (size_t)i * HDR_K, distortion_fx + (size_t)i * HDR_K,
                          labels + HDR_K * c.off);
    }
    return RTN_OK;
}

extern "C" int rtn_header_stats_host(int n, const int32_t* dst_heights, const int64_t* offsets, const int32_t* ks, const uint8_t* hsv,
                                     size_t hsv_bytes, const uint8_t* labels, size_t labels_bytes, uint32_t* hist) {
    HPlan pl;
    RTN_PLAN(nullptr, "rtn_header_stats_host", plan_crops(n, dst_heights, offsets, hsv_bytes, hsv, &pl, 0));
    RTN_PLAN(nullptr, "rtn_header_stats_host", plan_labels(pl, labels, labels_bytes, 0));
    RTN_PLAN(nullptr, "rtn_header_stats_host", plan_ks(ks, &pl));
    if (n && !hist) return rtn_fail_host(nullptr, RTN_EINVAL, "rtn_header_stats_host: the histogram output expected");
    for (int i = 0; i < n; ++i) {
        const HCrop& c = pl.crops[i];
        const int N = c.dh * HDR_W;
        const uint8_t* pts = hsv + 3 * c.off;
        const uint8_t* lab = labels + HDR_K * c.off + (size_t)(c.k - 1) * N;
        uint32_t* out = hist + (size_t)i * HDR_K * 3 * 256;
        memset(out, 0, sizeof(uint32_t) * HDR_K * 3 * 256);
        for (int p = 0; p < N; ++p) {
            if (lab[p] >= c.k) continue;
            for (int j = 0; j < 3; ++j) out[(lab[p] * 3 + j) * 256 + pts[3 * p + j]] += 1;
        }
    }
    return RTN_OK;
}

extern "C" int rtn_header_patches_host(int n, const int32_t* dst_heights, const int64_t* offsets, const uint8_t* hsv, size_t hsv_bytes,
                                       int n_patches, const int32_t* patch_crop, const uint8_t* low, const uint8_t* high,
                                       const int64_t* out_offsets, uint8_t* out, size_t out_bytes) {
    HPlan pl;
    RTN_PLAN(nullptr, "rtn_header_patches_host", plan_crops(n, dst_heights, offsets, hsv_bytes, hsv, &pl, 0));
    RTN_PLAN(nullptr, "rtn_header_patches_host", plan_patches(n_patches, patch_crop, low, high, out_offsets, out, out_bytes, &pl));
    for (const HPatch& p : pl.patches) {
        const HCrop& c = pl.crops[p.crop];
        for (int64_t i = 0; i < (int64_t)c.dh * HDR_W; ++i)
            hdr_patch_pixel(hsv + 3 * c.off, c.dh, (int)(i / HDR_W), (int)(i % HDR_W), p.lo, p.hi, out + p.out_off + 3 * i);
    }
    return RTN_OK;
}
