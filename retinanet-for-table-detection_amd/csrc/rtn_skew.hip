// rtn_skew.hip — the skew angle of scanned pages on the device: a profile sweep over sheared band counts, for a whole
// batch of pages of different sizes and channel counts.  The per-pixel and per-candidate rules are the text the CPU twin runs
// (rtn_skew.h).  One call queues, on the handle's stream and with no host round trip between them:
//   a clear          of the histograms (Otsu only) and of the ink counters
//   skew_hist        (Otsu only) a workgroup owns SKW_TILE_ROWS rows of a page, a lane takes four pixels a step; the histogram lives in
//                    LDS, the value a wave's first lane holds is counted once for all lanes that hold it (a scan is mostly paper),
//                    and the non-empty bins go to the page's histogram by integer atomics
//   skew_threshold   a workgroup a page: thread t evaluates Otsu's candidate t; the page's threshold goes to device memory
//   skew_counts      the same tiles and loads; four ballots of gray < t and a popcount per band give a byte per (row, band)
//   skew_sweep       a workgroup per (angle, page): the shifts of the bands and the profile (uint16) in LDS, then the sum of squared
//                    differences
//   skew_pick        a workgroup a page: the best angle by the tie rule
#include <algorithm>
#include <vector>
#include "rtn_page_launch.h"
#include "rtn_skew.h"

namespace {

constexpr int WAVES = SKW_THREADS / 64;
constexpr int SWEEP_LDS_LIMIT = 96 * 1024;          // 4 bytes x 4096 bands (32767 / 8) + 2 bytes x 32767 rows, rounded up

// the grays of pixels x .. x + 3 of a row of w pixels, one a byte, lowest first; *valid: how many of them the row holds (0 .. 4), the
// bytes of the others are 255 (never ink).  Four whole pixels are read as one or three dwords of any alignment.
__device__ inline uint32_t load_gray4(const uint8_t* row, int x, int w, int c, int* valid) {
    const int nv = w - x >= 4 ? 4 : (w - x > 0 ? w - x : 0);
    *valid = nv;
    if (nv == 4) {
        if (c == 1) {
            uint32_t v;
            __builtin_memcpy(&v, row + x, 4);
            return v;
        }
        uint32_t q[3];
        __builtin_memcpy(q, row + (size_t)x * 3, 12);
        const uint32_t g0 = skw_gray3(q[0] & 255, (q[0] >> 8) & 255, (q[0] >> 16) & 255);
        const uint32_t g1 = skw_gray3(q[0] >> 24, q[1] & 255, (q[1] >> 8) & 255);
        const uint32_t g2 = skw_gray3((q[1] >> 16) & 255, q[1] >> 24, q[2] & 255);
        const uint32_t g3 = skw_gray3((q[2] >> 8) & 255, (q[2] >> 16) & 255, q[2] >> 24);
        return g0 | g1 << 8 | g2 << 16 | g3 << 24;
    }
    uint32_t out = 0xffffffffu;
    for (int j = 0; j < nv; ++j) {
        const uint8_t* q = row + (size_t)(x + j) * c;
        const uint32_t g = c == 3 ? (uint32_t)skw_gray3(q[0], q[1], q[2]) : (uint32_t)q[0];
        out = (out & ~(255u << (8 * j))) | g << (8 * j);
    }
    return out;
}

struct Tile {
    SkwPage p;
    int page, y0, y1;
};

__device__ inline Tile tile_of(const SkwPage* pages, int n) {
    Tile t;
    const int64_t tile = blockIdx.x;
    t.page = skw_page_of_tile(pages, n, tile);
    t.p = pages[t.page];
    t.y0 = (int)(tile - t.p.tile_begin) * SKW_TILE_ROWS;
    t.y1 = t.y0 + SKW_TILE_ROWS < t.p.h ? t.y0 + SKW_TILE_ROWS : t.p.h;
    return t;
}

__global__ __launch_bounds__(SKW_THREADS) void skew_hist_kernel(const SkwPage* pages, int n, uint32_t* hist) {
    __shared__ uint32_t lh[256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    lh[tid] = 0;
    __syncthreads();
    const Tile t = tile_of(pages, n);
    const int64_t row_bytes = (int64_t)t.p.w * t.p.c;
    for (int y = t.y0 + wave; y < t.y1; y += WAVES) {
        const uint8_t* row = t.p.src + (int64_t)y * row_bytes;
        for (int x0 = 0; x0 < t.p.w; x0 += SKW_CHUNK) {
            int nv;
            const uint32_t g4 = load_gray4(row, x0 + 4 * lane, t.p.w, t.p.c, &nv);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int v = j < nv ? (int)((g4 >> (8 * j)) & 255) : -1;
                const int v0 = __builtin_amdgcn_readfirstlane(v);
                const unsigned long long m = __ballot(v == v0);
                if (v == v0) {
                    if (v0 >= 0 && lane == __ffsll((long long)m) - 1) atomicAdd(&lh[v0], (uint32_t)__popcll(m));
                } else if (v >= 0) {
                    atomicAdd(&lh[v], 1u);
                }
            }
        }
    }
    __syncthreads();
    if (lh[tid]) atomicAdd(&hist[(size_t)t.page * 256 + tid], lh[tid]);
}

// fixed: the caller's threshold, or 0 for Otsu's of the page's histogram
__global__ __launch_bounds__(SKW_THREADS) void skew_threshold_kernel(const uint32_t* hist, int fixed, int32_t* thresholds) {
    __shared__ uint32_t lh[256];
    __shared__ double bv[256];
    __shared__ int bt[256];
    const int tid = threadIdx.x, page = blockIdx.x;
    if (fixed) {
        if (tid == 0) thresholds[page] = fixed;
        return;
    }
    lh[tid] = hist[(size_t)page * 256 + tid];
    __syncthreads();
    int64_t N = 0, M = 0, w0 = 0, m0 = 0;
    for (int g = 0; g < 256; ++g) {
        const int64_t c = lh[g];
        N += c;
        M += g * c;
        if (g < tid) {
            w0 += c;
            m0 += g * c;
        }
    }
    bv[tid] = tid ? skw_otsu_term(w0, m0, N, M) : -1.0;
    bt[tid] = tid;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s && skw_otsu_better(bv[tid + s], bt[tid + s], bv[tid], bt[tid])) {
            bv[tid] = bv[tid + s];
            bt[tid] = bt[tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) thresholds[page] = bv[0] >= 0.0 ? bt[0] : 0;
}

__global__ __launch_bounds__(SKW_THREADS) void skew_counts_kernel(const SkwPage* pages, int n, const int32_t* thresholds, int band, uint8_t* counts,
                                                                  unsigned long long* ink) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const Tile t = tile_of(pages, n);
    const uint32_t thr = (uint32_t)thresholds[t.page];
    const int64_t row_bytes = (int64_t)t.p.w * t.p.c;
    const int lanes_per_band = band / 4, bands_per_chunk = SKW_CHUNK / band;
    // the lanes whose pixels lie in band `lane` of a chunk (lanes past the chunk's bands: none)
    const unsigned long long range = lane < bands_per_chunk ? ((1ull << lanes_per_band) - 1ull) << (lane * lanes_per_band) : 0ull;
    uint8_t* ct = counts + t.p.counts_off;
    uint32_t mine = 0;
    for (int y = t.y0 + wave; y < t.y1; y += WAVES) {
        const uint8_t* row = t.p.src + (int64_t)y * row_bytes;
        for (int x0 = 0; x0 < t.p.w; x0 += SKW_CHUNK) {
            int nv;
            const uint32_t g4 = load_gray4(row, x0 + 4 * lane, t.p.w, t.p.c, &nv);
            uint32_t cnt = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) cnt += (uint32_t)__popcll(__ballot(((g4 >> (8 * j)) & 255) < thr) & range);
            const int b = x0 / band + lane;
            if (lane < bands_per_chunk && b < t.p.nb) {
                ct[(int64_t)b * t.p.h + y] = (uint8_t)cnt;
                mine += cnt;
            }
        }
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) mine += __shfl_down(mine, s);
    if (lane == 0 && mine) atomicAdd(&ink[t.page], (unsigned long long)mine);
}

// dynamic LDS: the shifts of the page's bands (int32, max_nb of the batch rounded up to a multiple of four), then the profile (uint16)
__global__ __launch_bounds__(SKW_THREADS) void skew_sweep_kernel(const SkwPage* pages, const int32_t* shear, int band, int K, int shift_slots,
                                                                 const uint8_t* counts, unsigned long long* scores) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    __shared__ unsigned long long part[SKW_THREADS];
    int32_t* shift = reinterpret_cast<int32_t*>(lds);
    uint16_t* profile = reinterpret_cast<uint16_t*>(lds + (size_t)shift_slots * 4);
    const int tid = threadIdx.x, k = blockIdx.x, page = blockIdx.y;
    const SkwPage p = pages[page];
    const int32_t T = shear[k];
    for (int b = tid; b < p.nb; b += SKW_THREADS) shift[b] = skw_shift(b, band, p.w, T);
    __syncthreads();
    const uint8_t* ct = counts + p.counts_off;
    // a thread owns four consecutive profile rows: a band's four counts are one dword of any alignment, summed as two pairs of
    // 16-bit fields (a profile entry is at most W <= 32767, so no field carries into its neighbour)
    for (int r4 = 4 * tid; r4 < p.h; r4 += 4 * SKW_THREADS) {
        uint32_t even = 0, odd = 0;                                          // rows r4, r4 + 2 and rows r4 + 1, r4 + 3
        const uint8_t* col = ct;
        for (int b = 0; b < p.nb; ++b, col += p.h) {
            const int yy = r4 + shift[b];
            uint32_t v = 0;
            if (yy >= 0 && yy + 3 < p.h) {
                __builtin_memcpy(&v, col + yy, 4);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if ((unsigned)(yy + j) < (unsigned)p.h) v |= (uint32_t)col[yy + j] << (8 * j);
            }
            even += v & 0x00ff00ffu;
            odd += (v >> 8) & 0x00ff00ffu;
        }
        const uint32_t out[4] = {even & 0xffffu, odd & 0xffffu, even >> 16, odd >> 16};
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (r4 + j < p.h) profile[r4 + j] = (uint16_t)out[j];
    }
    __syncthreads();
    unsigned long long s = 0;
    for (int r = tid; r + 1 < p.h; r += SKW_THREADS) {
        const long long d = (long long)profile[r + 1] - (long long)profile[r];
        s += (unsigned long long)(d * d);
    }
    part[tid] = s;
    __syncthreads();
    for (int w = SKW_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) part[tid] += part[tid + w];
        __syncthreads();
    }
    if (tid == 0) scores[(size_t)page * K + k] = part[0];
}

__global__ __launch_bounds__(SKW_THREADS) void skew_pick_kernel(const unsigned long long* scores, int K, int32_t* best) {
    __shared__ unsigned long long bs[SKW_THREADS];
    __shared__ int bk[SKW_THREADS];
    const int tid = threadIdx.x, page = blockIdx.x, n_steps = K / 2;
    const unsigned long long* sc = scores + (size_t)page * K;
    unsigned long long s = sc[tid < K ? tid : 0];
    int k = tid < K ? tid : 0;
    for (int j = tid + SKW_THREADS; j < K; j += SKW_THREADS)
        if (skw_pick_better(sc[j], j, s, k, n_steps)) {
            s = sc[j];
            k = j;
        }
    bs[tid] = s;
    bk[tid] = k;
    __syncthreads();
    for (int w = SKW_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w && skw_pick_better(bs[tid + w], bk[tid + w], bs[tid], bk[tid], n_steps)) {
            bs[tid] = bs[tid + w];
            bk[tid] = bk[tid + w];
        }
        __syncthreads();
    }
    if (tid == 0) best[page] = bk[0];
}

// the workspace: the page table, the shear factors, the histograms, the counts
struct Layout { size_t table, shear, hist, counts; };

Layout layout_of(rtn_stage& st, int n, int K, int64_t counts_bytes) {
    Layout l;
    l.table = st.reserve((int64_t)n * sizeof(SkwPage));
    l.shear = st.reserve((int64_t)K * 4);
    l.hist = st.reserve((int64_t)n * 1024);
    l.counts = st.reserve(counts_bytes);
    return l;
}

int64_t counts_bytes_of(int n, const int32_t* heights, const int32_t* widths, int band, int64_t* offsets) {
    int64_t pos = 0;
    for (int i = 0; i < n; ++i) {
        if (offsets) offsets[i] = pos;
        pos += skw_align((int64_t)heights[i] * ((widths[i] + band - 1) / band), 16);
    }
    return pos;
}

}  // namespace

// rtn_skew_*: see include/rtn.h
extern "C" size_t rtn_skew_workspace_bytes(int n, const int32_t* heights, const int32_t* widths, int band, int K) {
    if (n < 1 || skw_check_sizes(n, heights, widths, band, K)) return 0;
    rtn_stage st;
    layout_of(st, n, K, counts_bytes_of(n, heights, widths, band, nullptr));
    return st.bytes();
}

extern "C" int rtn_skew_counts_layout(int n, const int32_t* heights, const int32_t* widths, int band, int K, int64_t* offsets) {
    if (!offsets || n < 1 || skw_check_sizes(n, heights, widths, band, K)) return RTN_EINVAL;
    rtn_stage st;
    const Layout l = layout_of(st, n, K, counts_bytes_of(n, heights, widths, band, offsets));
    for (int i = 0; i < n; ++i) offsets[i] += (int64_t)l.counts;
    return RTN_OK;
}

extern "C" int rtn_skew_estimate(rtn_handle_t h, int n, const uint8_t* const* pages, const int32_t* heights, const int32_t* widths,
                                 const int32_t* channels, int threshold, int band, int K, const int32_t* shear_q16, int32_t* thresholds,
                                 int64_t* ink, int32_t* best, uint64_t* scores, void* workspace, size_t workspace_bytes) {
    if (!h) return RTN_EINVAL;
    std::vector<SkwPage> table((size_t)(n > 0 && n <= SKW_MAX_PAGES ? n : 0));
    int64_t counts_bytes = 0, tiles = 0;
    int max_h = 0, max_nb = 0;
    RTN_PLAN(h, "rtn_skew_estimate", skw_plan(n, pages, heights, widths, channels, threshold, band, K, shear_q16, table.data(), &counts_bytes, &tiles, &max_h, &max_nb));
    if (n == 0) return RTN_OK;
    if (!thresholds || !ink || !best || !scores) return rtn_fail(h, RTN_EINVAL, "rtn_skew_estimate: the four result arrays expected");
    rtn_stage st;
    const Layout l = layout_of(st, n, K, counts_bytes);
    st.put(l.table, table);
    st.put(l.shear, shear_q16, (size_t)K * 4);
    if (const int rc = st.commit(h, "rtn_skew_estimate", workspace, workspace_bytes)) return rc;
    const SkwPage* d_table = st.at<const SkwPage>(l.table);
    const int32_t* d_shear = st.at<const int32_t>(l.shear);
    uint32_t* d_hist = st.at<uint32_t>(l.hist);
    uint8_t* d_counts = st.at<uint8_t>(l.counts);
    RTN_HIP(h, hipMemsetAsync(ink, 0, (size_t)n * 8, h->stream));
    if (!threshold) {
        RTN_HIP(h, hipMemsetAsync(d_hist, 0, (size_t)n * 1024, h->stream));
        skew_hist_kernel<<<dim3((unsigned)tiles), dim3(SKW_THREADS), 0, h->stream>>>(d_table, n, d_hist);
        RTN_CHECK_LAUNCH(h, "skew_hist_kernel");
    }
    skew_threshold_kernel<<<dim3((unsigned)n), dim3(SKW_THREADS), 0, h->stream>>>(d_hist, threshold, thresholds);
    RTN_CHECK_LAUNCH(h, "skew_threshold_kernel");
    skew_counts_kernel<<<dim3((unsigned)tiles), dim3(SKW_THREADS), 0, h->stream>>>(d_table, n, thresholds, band, d_counts,
                                                                                   reinterpret_cast<unsigned long long*>(ink));
    RTN_CHECK_LAUNCH(h, "skew_counts_kernel");
    const int shift_slots = (max_nb + 3) & ~3;
    const unsigned lds = (unsigned)shift_slots * 4u + (((unsigned)max_h * 2u + 15u) & ~15u);
    // the 64 KiB default refuses the tallest pages
    if (const int rc = rtn_launch_lds<skew_sweep_kernel>(h, dim3((unsigned)K, (unsigned)n), dim3(SKW_THREADS), lds, SWEEP_LDS_LIMIT, d_table, d_shear, band, K,
                                                         shift_slots, d_counts, reinterpret_cast<unsigned long long*>(scores)))
        return rc;
    RTN_CHECK_LAUNCH(h, "skew_sweep_kernel");
    skew_pick_kernel<<<dim3((unsigned)n), dim3(SKW_THREADS), 0, h->stream>>>(reinterpret_cast<const unsigned long long*>(scores), K, best);
    RTN_CHECK_LAUNCH(h, "skew_pick_kernel");
    return RTN_OK;
}

// ---- the CPU twin: host pointers, no handle (rtn_skew.h) --------------------------------------------------------------------------------
extern "C" int rtn_skew_estimate_host(int n, const uint8_t* const* pages, const int32_t* heights, const int32_t* widths, const int32_t* channels,
                                      int threshold, int band, int K, const int32_t* shear_q16, int32_t* thresholds, int64_t* ink,
                                      int32_t* best, uint64_t* scores) {
    RTN_PLAN(nullptr, "rtn_skew_estimate_host", skw_host(n, pages, heights, widths, channels, threshold, band, K, shear_q16, thresholds, ink, best, scores));
    return RTN_OK;
}
