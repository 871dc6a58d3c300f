// rtn_resize_u8.h — the text that the 8-bit bicubic resize (csrc/rtn_resize_u8.hip) and its CPU twin share:
// cv2.resize(INTER_CUBIC) of an 8-bit page in OpenCV's portable C form (interpolateImages, DetectTablesUtils.py:296-316;
// Shapes.Image.data, FasterRCNN/Shapes.py:27-28) as __host__ __device__ functions.  A plain C++17 compiler compiles this header
// (no HIP).  Its users are compiled with -ffp-contract=off: every float statement below is one rounding.  The kernel, the twin and
// the NumPy oracle (tests/resize_u8_ref.py) give the same bits.
//
// Two caveats.  This is OpenCV's text as recalled; it cannot be verified offline (OpenCV is not a dependency and was not available
// when this was written).  And OpenCV's vectorised builds evaluate the vertical pass in float32, so they can differ from this C
// form by 1 at rare samples.
//
// Per axis, for destination index d and inverse scale inv (a double): f = (d + 0.5) * inv - 0.5 in float64, s = floor(f),
// x = (float)(f - s); four float32 coefficients from x with A = -0.75 (oracle/ref_preprocess.py cubic_coeffs), each turned into
// saturate_cast<short>(c * 2048) (rint, half to even); taps at clip(s - 1 + k, 0, n - 1).  Horizontal sums and vertical sums are
// int32, the output is clip((v + 2^21) >> 22, 0, 255) with an arithmetic shift.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <vector>
#include "rtn.h"
#if !defined(__HIPCC__) && !defined(__host__)      // a plain C++ compiler (host-only sanitizer builds)
#define __host__
#define __device__
#endif

constexpr int RSZ_MAX_SIDE = 65500;                // the image readers' limit
constexpr int RSZ_MAX_PAGES = 65535;
constexpr int RSZ_THREADS = 256;
constexpr int RSZ_TILE_ROWS = 32;                  // destination rows of a tile
constexpr int RSZ_TILE_BYTES = 256;                // destination bytes (samples) of a tile row: one per thread in the horizontal pass
constexpr int RSZ_CHUNK = 16;                      // destination bytes a lane produces per row in the vertical pass: one 16-byte store
constexpr int RSZ_LDS_ROWS = RSZ_TILE_ROWS + 4;    // source rows a tile may hold: floor(f + 31 inv) - floor(f) <= 31 for inv <= 1, plus
                                                   // the taps -1 .. +2, plus one row of slack for the rounding of f
constexpr double RSZ_MAX_INV = 2147483648.0;      // far above any scale of two sides within the limit; keeps f finite
constexpr int64_t RSZ_MAX_TILES = (1ll << 24) - 1;   // one workgroup of 256 threads each: the grid stays below 2^32 threads
constexpr int RSZ_PATH_TILED = 1, RSZ_PATH_DIRECT = 2;
constexpr int RSZ_COEF_BITS = 11, RSZ_COEF_ONE = 1 << RSZ_COEF_BITS;
// int32 is enough: sum |alpha| is 1.375 * 2048 = 2816 at x = 0.5, its maximum, and at most 2 more after the four roundings (taken
// as 2820 here), so |h| <= 255 * 2820 < 2^24 and |v| + 2^21 <= 255 * 2820^2 + 2^21 < 2^31
constexpr int64_t RSZ_COEF_SUM = 2820;
static_assert(255 * RSZ_COEF_SUM < (1ll << 23), "a horizontal sum fits 24 signed bits");
static_assert(255 * RSZ_COEF_SUM * RSZ_COEF_SUM + (1ll << 21) < (1ll << 31), "a vertical sum and its rounding term fit int32");
static_assert(RSZ_TILE_BYTES == RSZ_THREADS && RSZ_TILE_BYTES % (4 * RSZ_CHUNK) == 0 && RSZ_TILE_ROWS % (RSZ_THREADS / (RSZ_TILE_BYTES / RSZ_CHUNK)) == 0,
              "one thread per tile column; whole passes of the vertical walk");

struct RszPage {                                   // 72 bytes
    const uint8_t* src;
    uint8_t* dst;
    double inv_x, inv_y;
    int64_t tile_begin;                            // the page's first tile in the launch's flat list of tiles
    int32_t h, w, ho, wo, c;
    int32_t path;                                  // RSZ_PATH_*
    int32_t tiles_x, pad_;                         // tiles across a destination row of wo * c bytes
};
static_assert(sizeof(RszPage) == 72, "resize table layout");

struct RszTaps {                                   // one destination index of one axis
    int32_t idx[4];                                // the clipped source indices
    int32_t coef[4];                               // the fixed-point coefficients (each fits a short)
};

// ---- the coefficients ----------------------------------------------------------------------------------------------------------------
__host__ __device__ inline int32_t rsz_fixed(float c) {         // saturate_cast<short>(c * 2048): the product is exact
    const float p = c * (float)RSZ_COEF_ONE;
    const float r = rintf(p);
    return r < -32768.0f ? -32768 : (r > 32767.0f ? 32767 : (int32_t)r);
}

__host__ __device__ inline void rsz_coeffs(float x, int32_t* coef) {
    const float A = -0.75f;
    const float x1 = x + 1.0f;
    float t = A * x1;                                            // ((A (x+1) - 5A) (x+1) + 8A) (x+1) - 4A
    t = t - 5.0f * A;
    t = t * x1;
    t = t + 8.0f * A;
    t = t * x1;
    const float c0 = t - 4.0f * A;
    t = (A + 2.0f) * x;                                          // ((A+2) x - (A+3)) x x + 1
    t = t - (A + 3.0f);
    t = t * x;
    t = t * x;
    const float c1 = t + 1.0f;
    const float y = 1.0f - x;
    t = (A + 2.0f) * y;                                          // the same in 1 - x
    t = t - (A + 3.0f);
    t = t * y;
    t = t * y;
    const float c2 = t + 1.0f;
    t = 1.0f - c0;
    t = t - c1;
    const float c3 = t - c2;
    coef[0] = rsz_fixed(c0);
    coef[1] = rsz_fixed(c1);
    coef[2] = rsz_fixed(c2);
    coef[3] = rsz_fixed(c3);
}

// the taps of destination index d on an axis of n source samples
__host__ __device__ inline void rsz_taps(int d, double inv, int n, RszTaps* t) {
    const double a = (double)d + 0.5;
    const double b = a * inv;
    const double f = b - 0.5;
    const double fl = floor(f);
    rsz_coeffs((float)(f - fl), t->coef);
    // every tap of a position left of -2 clips to 0 and every tap of one right of n clips to n - 1: clamped before it becomes an int
    const int s = fl < -3.0 ? -3 : (fl > (double)n + 1.0 ? n + 1 : (int)fl);
    for (int k = 0; k < 4; ++k) {
        const int i = s - 1 + k;
        t->idx[k] = i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
    }
}

__host__ __device__ inline uint8_t rsz_output(int32_t v) {
    const int32_t r = (v + (1 << (2 * RSZ_COEF_BITS - 1))) >> (2 * RSZ_COEF_BITS);      // arithmetic shift
    return (uint8_t)(r < 0 ? 0 : (r > 255 ? 255 : r));
}

// ---- the tile walk ----------------------------------------------------------------------------------------------------------------------
// In LDS a tile row of horizontal sums is not in column order: a lane of the vertical pass owns RSZ_CHUNK consecutive columns and
// reads them four at a time (16 bytes), so the four columns 16 l + 4 q .. + 3 of lane l lie at dwords 64 q + 4 l .. + 3: a group of
// lanes reads consecutive dwords, free of bank conflicts.  Thread t of the horizontal pass owns slot t, so its writes are consecutive
// across lanes too.
__host__ __device__ inline int rsz_slot_column(int slot) { return 16 * ((slot & 63) >> 2) + 4 * (slot >> 6) + (slot & 3); }
__host__ __device__ inline int rsz_column_slot(int col) { return 64 * ((col >> 2) & 3) + 4 * (col >> 4) + (col & 3); }

struct RszColumn {                                 // one destination byte column of a tile
    int32_t off[4];                                // byte offsets of its taps in a source row (sample index * c + channel)
    int32_t coef[4];                               // all 0 for a column past the end of the row
};

__host__ __device__ inline void rsz_column(const RszPage& p, int64_t bx, RszColumn* col) {
    const bool inside = bx < (int64_t)p.wo * p.c;
    const int64_t b = inside ? bx : 0;
    const int dx = (int)(b / p.c), ch = (int)(b - (int64_t)dx * p.c);
    RszTaps t;
    rsz_taps(dx, p.inv_x, p.w, &t);
    for (int k = 0; k < 4; ++k) {
        col->off[k] = inside ? t.idx[k] * p.c + ch : 0;
        col->coef[k] = inside ? t.coef[k] : 0;
    }
}

// a product of two factors of at most 24 signed bits (a byte, a coefficient, a horizontal sum) that fits int32
__host__ __device__ inline int32_t rsz_mul(int32_t a, int32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __mul24(a, b);
#else
    return a * b;
#endif
}

template <class Row>                               // const uint8_t*, or the kernel's pointer into global memory
__host__ __device__ inline int32_t rsz_horizontal(Row row, const RszColumn& col) {
    int32_t h = rsz_mul((int32_t)row[col.off[0]], col.coef[0]);
    h += rsz_mul((int32_t)row[col.off[1]], col.coef[1]);
    h += rsz_mul((int32_t)row[col.off[2]], col.coef[2]);
    h += rsz_mul((int32_t)row[col.off[3]], col.coef[3]);
    return h;
}

// the source rows a tile of rows [y0, y0 + rows) reads: the taps of a later row are never above those of an earlier one
__host__ __device__ inline void rsz_tile_span(const RszTaps* first_row, const RszTaps* last_row, int* first, int* count) {
    *first = first_row->idx[0];
    *count = last_row->idx[3] - first_row->idx[0] + 1;
}

// ---- argument checks and the page table the device entry and the twin share -------------------------------------------------------------
inline int rsz_choose_path(int forced, double inv_y) {
    if (forced == RSZ_PATH_DIRECT) return RSZ_PATH_DIRECT;
    return inv_y <= 1.0 ? RSZ_PATH_TILED : RSZ_PATH_DIRECT;      // forced tiled: only where the tile's source rows fit
}

inline const char* rsz_plan(int n, const uint8_t* const* pages, const int32_t* heights, const int32_t* widths, const int32_t* channels,
                            const int32_t* out_heights, const int32_t* out_widths, const double* inv_x, const double* inv_y,
                            uint8_t* const* outs, int forced_path, RszPage* table, int64_t* tiles) {
    if (n < 0 || n > RSZ_MAX_PAGES) return "0 .. 65535 pages expected";
    if (n && (!pages || !heights || !widths || !channels || !out_heights || !out_widths || !inv_x || !inv_y || !outs))
        return "the pages, their sizes, channels, output sizes, inverse scales and outputs expected";
    int64_t pos = 0;
    for (int i = 0; i < n; ++i) {
        RszPage& e = table[i];
        memset(&e, 0, sizeof(e));
        if (!pages[i] || !outs[i]) return "a page or its output is missing";
        if (heights[i] < 1 || widths[i] < 1 || heights[i] > RSZ_MAX_SIDE || widths[i] > RSZ_MAX_SIDE || out_heights[i] < 1 ||
            out_widths[i] < 1 || out_heights[i] > RSZ_MAX_SIDE || out_widths[i] > RSZ_MAX_SIDE)
            return "a page or an output has a side outside 1 .. 65500";
        if (channels[i] != 1 && channels[i] != 3) return "a page has a channel count other than 1 or 3";
        for (const double v : {inv_x[i], inv_y[i]})
            if (!(v - v == 0.0) || !(v > 0.0) || v > RSZ_MAX_INV) return "an inverse scale is not a positive finite number of at most 2^31";
        const uint64_t sb = (uint64_t)heights[i] * (uint64_t)widths[i] * (uint64_t)channels[i];
        const uint64_t db = (uint64_t)out_heights[i] * (uint64_t)out_widths[i] * (uint64_t)channels[i];
        const uintptr_t s = (uintptr_t)pages[i], d = (uintptr_t)outs[i];
        if (s < d + db && d < s + sb) return "an output overlaps its page";
        e.src = pages[i];
        e.dst = outs[i];
        e.inv_x = inv_x[i];
        e.inv_y = inv_y[i];
        e.h = heights[i];
        e.w = widths[i];
        e.ho = out_heights[i];
        e.wo = out_widths[i];
        e.c = channels[i];
        e.path = rsz_choose_path(forced_path, inv_y[i]);
        e.tiles_x = (int32_t)(((int64_t)e.wo * e.c + RSZ_TILE_BYTES - 1) / RSZ_TILE_BYTES);
        e.tile_begin = pos;
        pos += (int64_t)e.tiles_x * ((e.ho + RSZ_TILE_ROWS - 1) / RSZ_TILE_ROWS);
    }
    if (pos > RSZ_MAX_TILES) return "more than 2^24 - 1 tiles (128 GiB of output) in one call";
    *tiles = pos;
    return nullptr;
}

// the page of a tile of the flat list: the last page whose tile_begin is not above it
__host__ __device__ inline int rsz_page_of_tile(const RszPage* table, int n, int64_t tile) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].tile_begin <= tile) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// ---- the CPU twin: the walk of resize_u8_kernel, tile by tile and thread by thread ----------------------------------------------------
// hbuf: RSZ_LDS_ROWS * RSZ_TILE_BYTES sums, the kernel's LDS image with its slot order
inline void rsz_host_tile(const RszPage& p, int64_t local, int32_t* hbuf) {
    const int ty = (int)(local / p.tiles_x), tx = (int)(local - (int64_t)ty * p.tiles_x);
    const int y0 = ty * RSZ_TILE_ROWS;
    const int rows = p.ho - y0 < RSZ_TILE_ROWS ? p.ho - y0 : RSZ_TILE_ROWS;
    const int64_t x0 = (int64_t)tx * RSZ_TILE_BYTES;
    const int64_t row_bytes = (int64_t)p.wo * p.c, src_row_bytes = (int64_t)p.w * p.c;
    RszTaps rt[RSZ_TILE_ROWS];
    RszColumn col[RSZ_THREADS];
    for (int r = 0; r < rows; ++r) rsz_taps(y0 + r, p.inv_y, p.h, &rt[r]);
    for (int t = 0; t < RSZ_THREADS; ++t) rsz_column(p, x0 + rsz_slot_column(t), &col[t]);
    int first, count;
    rsz_tile_span(&rt[0], &rt[rows - 1], &first, &count);
    const bool tiled = p.path == RSZ_PATH_TILED && count <= RSZ_LDS_ROWS;
    if (tiled)
        for (int r = 0; r < count; ++r)
            for (int t = 0; t < RSZ_THREADS; ++t)
                hbuf[(size_t)r * RSZ_TILE_BYTES + t] = rsz_horizontal(p.src + (int64_t)(first + r) * src_row_bytes, col[t]);
    for (int r = 0; r < rows; ++r) {
        uint8_t* drow = p.dst + (int64_t)(y0 + r) * row_bytes;
        for (int c = 0; c < RSZ_TILE_BYTES && x0 + c < row_bytes; ++c) {
            const int slot = rsz_column_slot(c);
            int32_t v = 0;
            for (int k = 0; k < 4; ++k) {
                const int32_t hv = tiled ? hbuf[(size_t)(rt[r].idx[k] - first) * RSZ_TILE_BYTES + slot]
                                         : rsz_horizontal(p.src + (int64_t)rt[r].idx[k] * src_row_bytes, col[slot]);
                v += rsz_mul(hv, rt[r].coef[k]);
            }
            drow[x0 + c] = rsz_output(v);
        }
    }
}

// the body of rtn_resize_u8_host; forced_path: 0, or RSZ_PATH_* (RTN_RESIZE_U8_PATH)
inline const char* rsz_host(int n, const uint8_t* const* pages, const int32_t* heights, const int32_t* widths, const int32_t* channels,
                            const int32_t* out_heights, const int32_t* out_widths, const double* inv_x, const double* inv_y,
                            uint8_t* const* outs, int forced_path) {
    std::vector<RszPage> table((size_t)(n > 0 && n <= RSZ_MAX_PAGES ? n : 0));
    int64_t tiles = 0;
    if (const char* why = rsz_plan(n, pages, heights, widths, channels, out_heights, out_widths, inv_x, inv_y, outs, forced_path, table.data(), &tiles))
        return why;
    std::vector<int32_t> hbuf((size_t)RSZ_LDS_ROWS * RSZ_TILE_BYTES);
    for (int64_t tile = 0; tile < tiles; ++tile) {
        const RszPage& p = table[(size_t)rsz_page_of_tile(table.data(), n, tile)];
        rsz_host_tile(p, tile - p.tile_begin, hbuf.data());
    }
    return nullptr;
}
