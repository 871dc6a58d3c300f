// rtn_cca_rows.h — the device text that the row kernels of scan analysis (csrc/rtn_cca.hip) and of table structure
// (csrc/rtn_lattice.hip) share: the tile of the box-mean threshold, the workgroup prefix sum, the binary window step on
// 64-bit masks, the byte transpose through LDS and the row opening, and the host launch of the last two.  Every file that includes it gets
// kernels of its own.
#pragma once
#include "rtn_cca.h"

namespace {

// Tile blockIdx.x (64 x 32) of the thresholded image of the region [y0, y0 + h) x [x0, x0 + w) of page p into dst, the region's (h, w)
// plane: bitwise_not(gray) with the PAGE's replicated borders, the 15x15 box sum (row sums, then column sums, in LDS), the mean
// threshold.  Every thread of the workgroup calls it.
__device__ inline void bw_tile(const CPage& p, int y0, int x0, int h, int w, uint8_t* dst) {
    __shared__ uint8_t g[CCA_BW_TH + 14][CCA_BW_TW + 16];
    __shared__ uint16_t rs[CCA_BW_TH + 14][CCA_BW_TW];
    const int tiles_x = (w + CCA_BW_TW - 1) / CCA_BW_TW, tiles_y = (h + CCA_BW_TH - 1) / CCA_BW_TH;
    if ((int)blockIdx.x >= tiles_x * tiles_y) return;                          // uniform
    const int tx0 = ((int)blockIdx.x % tiles_x) * CCA_BW_TW, ty0 = ((int)blockIdx.x / tiles_x) * CCA_BW_TH;
    const int tid = threadIdx.x;
    for (int i = tid; i < (CCA_BW_TH + 14) * (CCA_BW_TW + 14); i += CCA_PIX_THREADS) {
        const int ly = i / (CCA_BW_TW + 14), lx = i % (CCA_BW_TW + 14);
        g[ly][lx] = (uint8_t)cca_ginv(p, y0 + ty0 + ly - 7, x0 + tx0 + lx - 7);
    }
    __syncthreads();
    for (int i = tid; i < (CCA_BW_TH + 14) * CCA_BW_TW; i += CCA_PIX_THREADS) {
        const int ly = i / CCA_BW_TW, lx = i % CCA_BW_TW;
        int s = 0;
#pragma unroll
        for (int d = 0; d < 15; ++d) s += g[ly][lx + d];
        rs[ly][lx] = (uint16_t)s;
    }
    __syncthreads();
    for (int i = tid; i < CCA_BW_TH * CCA_BW_TW; i += CCA_PIX_THREADS) {
        const int ly = i / CCA_BW_TW, lx = i % CCA_BW_TW, y = ty0 + ly, x = tx0 + lx;
        if (y >= h || x >= w) continue;
        int S = 0;
#pragma unroll
        for (int d = 0; d < 15; ++d) S += rs[ly + d][lx];
        dst[(int64_t)y * w + x] = cca_bw(g[ly + 7][lx + 7], S);
    }
}

// dst (cols, rows) = transpose of src (rows, cols); the CRows table names both
__global__ __launch_bounds__(CCA_PIX_THREADS) void transpose_kernel(const CRows* imgs) {
    __shared__ uint8_t t[32][33];
    const CRows m = imgs[blockIdx.y];
    const int tiles_x = (m.cols + 31) / 32, tiles_y = (m.rows + 31) / 32;
    if ((int)blockIdx.x >= tiles_x * tiles_y) return;                          // uniform
    const int x0 = ((int)blockIdx.x % tiles_x) * 32, y0 = ((int)blockIdx.x / tiles_x) * 32;
    const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
    for (int j = ly; j < 32; j += 8)
        if (y0 + j < m.rows && x0 + lx < m.cols) t[j][lx] = m.src[(size_t)(y0 + j) * m.cols + x0 + lx];
    __syncthreads();
    for (int j = ly; j < 32; j += 8)
        if (x0 + j < m.cols && y0 + lx < m.rows) m.dst[(size_t)(x0 + j) * m.rows + y0 + lx] = t[lx][j];
}

// exclusive prefix sum of v over the 256 threads of the workgroup; every thread calls it
__device__ inline int block_scan(int v, int* wave_sums, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(inc, d);
        if (lane >= d) inc += t;
    }
    __syncthreads();                                                            // the previous use of wave_sums has been read
    if (lane == 63) wave_sums[wave] = inc;
    __syncthreads();
    int base = 0;
#pragma unroll
    for (int i = 0; i < CCA_ROW_THREADS / 64; ++i) base += i < wave ? wave_sums[i] : 0;
    *total = wave_sums[0] + wave_sums[1] + wave_sums[2] + wave_sums[3];
    return base + inc - v;
}

// one window step over a row of n pixels: the thread's `cnt` pixels from x0 are the low bits of m.  P holds n + 1 counts.
__device__ inline uint64_t window_step(uint64_t m, int x0, int cnt, int n, int L, int anchor, bool is_min, uint16_t* P, int* wave_sums) {
    int total;
    int run = block_scan(__popcll(m), wave_sums, &total);
    for (int i = 0; i < cnt; ++i) {
        P[x0 + i] = (uint16_t)run;
        run += (int)((m >> i) & 1);
    }
    if (threadIdx.x == 0) P[n] = (uint16_t)total;
    __syncthreads();
    uint64_t r = 0;
    for (int i = 0; i < cnt; ++i) {
        int lo, hi;
        cca_window(x0 + i, L, anchor, n, &lo, &hi);
        if (cca_win_bit((int)P[hi + 1] - (int)P[lo], lo, hi, is_min)) r |= 1ull << i;
    }
    __syncthreads();                                                            // P is free for the next step
    return r;
}

// dynamic LDS of the row kernels: the 16-bit counts of the longest row of the launch, so that short rows leave room for more workgroups
inline unsigned row_lds_bytes(int max_cols) { return (unsigned)(2 * (max_cols + 2) + 15) & ~15u; }

__global__ __launch_bounds__(CCA_ROW_THREADS) void open_rows_kernel(const CRows* imgs) {
    extern __shared__ uint16_t P[];
    __shared__ int wave_sums[CCA_ROW_THREADS / 64];
    const CRows m = imgs[blockIdx.y];
    if ((int)blockIdx.x >= m.rows) return;                                      // uniform
    const int n = m.cols, per = (n + CCA_ROW_THREADS - 1) / CCA_ROW_THREADS;    // per <= 64
    const int x0 = threadIdx.x * per, cnt = max(0, min(per, n - x0));
    const uint8_t* src = m.src + (size_t)blockIdx.x * n;
    uint64_t bits = 0;
    for (int i = 0; i < cnt; ++i)
        if (src[x0 + i]) bits |= 1ull << i;
    bits = window_step(bits, x0, cnt, n, m.L, m.L / 2, true, P, wave_sums);
    bits = window_step(bits, x0, cnt, n, m.L, m.L / 2, false, P, wave_sums);
    uint8_t* dst = m.dst + (size_t)blockIdx.x * n;
    for (int i = 0; i < cnt; ++i) dst[x0 + i] = (bits >> i) & 1 ? 255 : 0;
}

// The middle of the two line-mask pipelines on the handle's stream (host; the includer has rtn_internal.h): rows[0 .. n) transposed,
// then rows[n .. 3 n) opened.  No image is larger than max_h x max_w; *t_tiles receives the 32x32 tiles of that size, for the
// caller's own last launch.
inline int launch_transpose_open(rtn_ctx* h, const CRows* rows, int n, int max_h, int max_w, unsigned* t_tiles) {
    *t_tiles = (unsigned)((max_w + 31) / 32) * (unsigned)((max_h + 31) / 32);
    const int longest = max_h > max_w ? max_h : max_w;
    transpose_kernel<<<dim3(*t_tiles, (unsigned)n), dim3(CCA_PIX_THREADS), 0, h->stream>>>(rows);
    RTN_CHECK_LAUNCH(h, "transpose_kernel");
    open_rows_kernel<<<dim3((unsigned)longest, (unsigned)(2 * n)), dim3(CCA_ROW_THREADS), row_lds_bytes(longest), h->stream>>>(rows + n);
    RTN_CHECK_LAUNCH(h, "open_rows_kernel");
    return RTN_OK;
}

}  // namespace
