// rtn_effect.hip — the colour effects of the training generator on the device (VisualEffect, model/transform.py:397-512):
// three launches for a whole batch of pages of different sizes.
//
//   colsum_kernel   integer sums of every (x, channel) over y, only for pages whose contrast step runs.  A workgroup adds a strip of
//                   EFX_STRIP rows of up to 256 (1024 where rows are dword aligned) byte columns in registers, then adds its partial
//                   sums into the zeroed workspace with integer atomics, 256 contiguous bytes per wave: exact in any order.
//   tables_kernel   one workgroup per page.  The column means (sum / H) pass through LDS in chunks; lane c adds those of channel c
//                   from x = 0 upwards in float64, which is the order that defines the bits, and divides by W.  Then thread x
//                   fills entry x of the page's tables.
//   pixels_kernel   the tables in LDS, with the two 256-entry tables of BGR2HSV's rounded divisions; a lane takes 16 pixels as
//                   three 16-byte words, the tail of a page and unaligned pages go byte by byte.  A lane reads its pixels before
//                   it writes them and no other lane touches them, so a page may be its own output.
// The means are complete before any pixel is written, by launch order.  The per-element rules are the text the CPU twin runs
// (rtn_effect.h).
#include <algorithm>
#include <vector>
#include "rtn_page_launch.h"
#include "rtn_effect.h"

namespace {

// ---- kernels --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EFX_THREADS) void colsum_kernel(const EfxPage* pages, uint32_t* sums) {
    const EfxPage p = pages[blockIdx.z];
    if (!(p.mode & EFX_CONTRAST)) return;
    const int y0 = (int)blockIdx.y * EFX_STRIP;
    if (y0 >= p.h) return;
    const int y1 = y0 + EFX_STRIP < p.h ? y0 + EFX_STRIP : p.h;
    const int64_t row_bytes = 3 * (int64_t)p.w;
    uint32_t* s = sums + p.sum_off;
    const int tid = threadIdx.x;
    const int64_t lane = (int64_t)blockIdx.x * EFX_THREADS + tid;
    if ((row_bytes & 3) == 0 && ((uintptr_t)p.src & 3) == 0) {               // every row starts on a dword: four columns per lane
        __shared__ uint32_t part[4 * EFX_THREADS];
        const int64_t j = 4 * lane;
        uint32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;
        if (j < row_bytes) {
            const uint8_t* q = p.src + (int64_t)y0 * row_bytes + j;
#pragma unroll 8
            for (int y = y0; y < y1; ++y, q += row_bytes) {
                const uint32_t v = *reinterpret_cast<const uint32_t*>(q);
                a0 += v & 255u;
                a1 += (v >> 8) & 255u;
                a2 += (v >> 16) & 255u;
                a3 += v >> 24;
            }
        }
        part[4 * tid] = a0;
        part[4 * tid + 1] = a1;
        part[4 * tid + 2] = a2;
        part[4 * tid + 3] = a3;
        __syncthreads();                                                     // the branch is uniform: all threads arrive
        // through LDS so that a wave adds 256 contiguous bytes at a time, not 64 words 16 bytes apart
        const int64_t j0 = 4 * (int64_t)blockIdx.x * EFX_THREADS;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = tid + EFX_THREADS * k;
            if (j0 + c < row_bytes) atomicAdd(&s[j0 + c], part[c]);
        }
    } else {
        if (lane >= row_bytes) return;
        const uint8_t* q = p.src + (int64_t)y0 * row_bytes + lane;
        uint32_t a = 0;
#pragma unroll 8
        for (int y = y0; y < y1; ++y, q += row_bytes) a += *q;
        atomicAdd(&s[lane], a);
    }
}

__global__ __launch_bounds__(EFX_THREADS) void tables_kernel(const EfxPage* pages, const uint32_t* sums, uint8_t* tables) {
    __shared__ double cm[3 * EFX_CHUNK];
    __shared__ double mean[3];
    const int tid = threadIdx.x;
    const EfxPage p = pages[blockIdx.x];
    if (p.mode & EFX_CONTRAST) {                                             // uniform: every barrier below is reached by all
        const uint32_t* s = sums + p.sum_off;
        double acc = 0.0;
        for (int x0 = 0; x0 < p.w; x0 += EFX_CHUNK) {
            const int m = p.w - x0 < EFX_CHUNK ? p.w - x0 : EFX_CHUNK;
            for (int i = tid; i < 3 * m; i += EFX_THREADS) cm[i] = efx_column_mean(s[3 * (int64_t)x0 + i], p.h);
            __syncthreads();
            if (tid < 3) {                                                   // eight LDS reads ahead of the adds, which stay in order
                int x = 0;
                for (; x + 8 <= m; x += 8) {
                    double v[8];
#pragma unroll
                    for (int k = 0; k < 8; ++k) v[k] = cm[3 * (x + k) + tid];
#pragma unroll
                    for (int k = 0; k < 8; ++k) acc = acc + v[k];
                }
                for (; x < m; ++x) acc = acc + cm[3 * x + tid];
            }
            __syncthreads();
        }
        if (tid < 3) mean[tid] = acc / (double)p.w;
    }
    __syncthreads();
    efx_table_entry(p.p, p.mode, mean, tid, tables + (size_t)blockIdx.x * EFX_TABLE_BYTES);
}

__device__ inline uint32_t byte_of(const uint32_t* w, int i) { return (w[i >> 2] >> (8 * (i & 3))) & 255u; }

__global__ __launch_bounds__(EFX_THREADS) void pixels_kernel(const EfxPage* pages, const uint8_t* tables) {
    __shared__ __attribute__((aligned(16))) uint8_t tab[EFX_TABLE_BYTES];
    __shared__ int32_t sdiv[256], hdiv[256];
    const int tid = threadIdx.x;
    const EfxPage p = pages[blockIdx.y];
    const int64_t npix = (int64_t)p.h * p.w;
    const int64_t first = (int64_t)blockIdx.x * EFX_BLOCK_PIXELS;
    if (first >= npix) return;
    const int64_t end = first + EFX_BLOCK_PIXELS < npix ? first + EFX_BLOCK_PIXELS : npix;
    const uint32_t mode = p.mode;
    if (tid < EFX_TABLE_BYTES / 16)                                          // tables of steps that do not run are never indexed
        reinterpret_cast<uint4*>(tab)[tid] = reinterpret_cast<const uint4*>(tables + (size_t)blockIdx.y * EFX_TABLE_BYTES)[tid];
    sdiv[tid] = hdr_sdiv(tid);
    hdiv[tid] = hdr_hdiv(tid);
    __syncthreads();
    // whole groups of 16 pixels: 3 * first is a multiple of 16, so with aligned pages every group is three aligned 16-byte words
    const int64_t vend = (mode & EFX_VECTOR) ? first + ((end - first) & ~(int64_t)(EFX_GROUP - 1)) : first;
    for (int64_t g = first + (int64_t)EFX_GROUP * tid; g < vend; g += (int64_t)EFX_GROUP * EFX_THREADS) {
        const uint4* src = reinterpret_cast<const uint4*>(p.src + 3 * g);
        const uint4 q0 = src[0], q1 = src[1], q2 = src[2];
        const uint32_t w[12] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
        uint32_t o[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < EFX_GROUP; ++k) {
            int b = (int)byte_of(w, 3 * k), gg = (int)byte_of(w, 3 * k + 1), r = (int)byte_of(w, 3 * k + 2);
            efx_pixel(mode, tab, sdiv, hdiv, &b, &gg, &r);
            o[(3 * k) >> 2] |= (uint32_t)b << (8 * ((3 * k) & 3));
            o[(3 * k + 1) >> 2] |= (uint32_t)gg << (8 * ((3 * k + 1) & 3));
            o[(3 * k + 2) >> 2] |= (uint32_t)r << (8 * ((3 * k + 2) & 3));
        }
        uint4* dst = reinterpret_cast<uint4*>(p.dst + 3 * g);
        dst[0] = make_uint4(o[0], o[1], o[2], o[3]);
        dst[1] = make_uint4(o[4], o[5], o[6], o[7]);
        dst[2] = make_uint4(o[8], o[9], o[10], o[11]);
    }
    for (int64_t i = vend + tid; i < end; i += EFX_THREADS) {
        int b = p.src[3 * i], gg = p.src[3 * i + 1], r = p.src[3 * i + 2];
        efx_pixel(mode, tab, sdiv, hdiv, &b, &gg, &r);
        p.dst[3 * i] = (uint8_t)b;
        p.dst[3 * i + 1] = (uint8_t)gg;
        p.dst[3 * i + 2] = (uint8_t)r;
    }
}

// ---- workspace: the page table, the tables, the column sums -----------------------------------------------------------------------
struct EfxLayout { size_t pages, tables, sums, sums_bytes; };

EfxLayout ws_layout(rtn_stage& st, int n, const int32_t* widths) {
    EfxLayout l;
    l.pages = st.reserve((int64_t)n * sizeof(EfxPage));
    l.tables = st.reserve((int64_t)n * EFX_TABLE_BYTES);
    int64_t cols = 0;
    for (int i = 0; i < n; ++i) cols += 3LL * widths[i];
    l.sums = st.reserve(cols * 4);
    l.sums_bytes = st.bytes() - l.sums;
    return l;
}

}  // namespace

// rtn_visual_effect_*: see include/rtn.h
extern "C" size_t rtn_visual_effect_workspace_bytes(int n, const int32_t* heights, const int32_t* widths) {
    if (efx_check_sizes(n, heights, widths)) return 0;
    rtn_stage st;
    ws_layout(st, n, widths);
    return st.bytes();
}

extern "C" int rtn_visual_effect_u8(rtn_handle_t h, int n, const uint8_t* const* pages, const int32_t* heights, const int32_t* widths,
                                    const double* params, const uint32_t* flags, uint8_t* const* outs, void* workspace,
                                    size_t workspace_bytes) {
    if (!h) return RTN_EINVAL;
    std::vector<EfxPage> table((size_t)(n > 0 && n <= EFX_MAX_PAGES ? n : 0));
    RTN_PLAN(h, "rtn_visual_effect_u8", efx_plan(n, pages, heights, widths, params, flags, outs, true, table.data()));
    if (n == 0) return RTN_OK;
    rtn_stage st;
    const EfxLayout l = ws_layout(st, n, widths);
    st.put(l.pages, table);
    if (const int rc = st.commit(h, "rtn_visual_effect_u8", workspace, workspace_bytes)) return rc;
    // the grids: the largest page decides, smaller pages' spare workgroups return at once
    unsigned sum_x = 0, sum_y = 0, pix_x = 0;
    for (const EfxPage& e : table) {
        const int64_t row_bytes = 3 * (int64_t)e.w, npix = (int64_t)e.h * e.w;
        if (e.mode & EFX_CONTRAST) {
            const int64_t per_lane = (row_bytes & 3) == 0 && ((uintptr_t)e.src & 3) == 0 ? 4 : 1;
            sum_x = std::max(sum_x, (unsigned)((row_bytes + per_lane * EFX_THREADS - 1) / (per_lane * EFX_THREADS)));
            sum_y = std::max(sum_y, (unsigned)((e.h + EFX_STRIP - 1) / EFX_STRIP));
        }
        pix_x = std::max(pix_x, (unsigned)((npix + EFX_BLOCK_PIXELS - 1) / EFX_BLOCK_PIXELS));
    }
    const EfxPage* t = st.at<const EfxPage>(l.pages);
    uint32_t* sums = st.at<uint32_t>(l.sums);
    uint8_t* tabs = st.at<uint8_t>(l.tables);
    if (sum_x) {
        RTN_HIP(h, hipMemsetAsync(sums, 0, l.sums_bytes, h->stream));
        colsum_kernel<<<dim3(sum_x, sum_y, (unsigned)n), dim3(EFX_THREADS), 0, h->stream>>>(t, sums);
        RTN_CHECK_LAUNCH(h, "colsum_kernel");
    }
    tables_kernel<<<dim3((unsigned)n), dim3(EFX_THREADS), 0, h->stream>>>(t, sums, tabs);
    RTN_CHECK_LAUNCH(h, "tables_kernel");
    pixels_kernel<<<dim3(pix_x, (unsigned)n), dim3(EFX_THREADS), 0, h->stream>>>(t, tabs);
    RTN_CHECK_LAUNCH(h, "pixels_kernel");
    return RTN_OK;
}

// ---- the CPU twin: host pointers, no handle, the same header functions -----------------------------------------------------------
extern "C" int rtn_visual_effect_host(int n, const uint8_t* const* pages, const int32_t* heights, const int32_t* widths,
                                      const double* params, const uint32_t* flags, uint8_t* const* outs) {
    std::vector<EfxPage> table((size_t)(n > 0 && n <= EFX_MAX_PAGES ? n : 0));
    RTN_PLAN(nullptr, "rtn_visual_effect_host", efx_plan(n, pages, heights, widths, params, flags, outs, false, table.data()));
    int32_t sdiv[256], hdiv[256];
    for (int i = 0; i < 256; ++i) {
        sdiv[i] = hdr_sdiv(i);
        hdiv[i] = hdr_hdiv(i);
    }
    std::vector<uint32_t> sums;
    for (const EfxPage& e : table) {
        double mean[3] = {0.0, 0.0, 0.0};
        if (e.mode & EFX_CONTRAST) {
            const size_t cols = 3 * (size_t)e.w;
            sums.assign(cols, 0u);
            for (int y = 0; y < e.h; ++y) {
                const uint8_t* row = e.src + (size_t)y * cols;
                for (size_t j = 0; j < cols; ++j) sums[j] += row[j];
            }
            for (int c = 0; c < 3; ++c) {
                double acc = 0.0;
                for (int x = 0; x < e.w; ++x) acc = acc + efx_column_mean(sums[3 * (size_t)x + c], e.h);
                mean[c] = acc / (double)e.w;
            }
        }
        uint8_t tab[EFX_TABLE_BYTES];
        memset(tab, 0, sizeof(tab));
        for (int x = 0; x < 256; ++x) efx_table_entry(e.p, e.mode, mean, x, tab);
        const int64_t npix = (int64_t)e.h * e.w;
        for (int64_t i = 0; i < npix; ++i) {
            int b = e.src[3 * i], g = e.src[3 * i + 1], r = e.src[3 * i + 2];
            efx_pixel(e.mode, tab, sdiv, hdiv, &b, &g, &r);
            e.dst[3 * i] = (uint8_t)b;
            e.dst[3 * i + 1] = (uint8_t)g;
            e.dst[3 * i + 2] = (uint8_t)r;
        }
    }
    return RTN_OK;
}
