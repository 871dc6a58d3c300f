// rtn_compose.h — the text that the page composer (csrc/rtn_compose.hip) and its CPU twin share: where a pixel of a
// decoded image lands on its page, the argument checks and the tables of a batch.  A plain C++17 compiler compiles this header (no
// HIP); tools/compose_fuzz.cpp does.
//
// An item is a decoded image S of (h, w, 3) B,G,R bytes, an orientation code 1 .. 8 (TIFF / EXIF: where row 0 and column 0 of S lie
// on the page) and a rectangle.  The oriented image O has oh x ow pixels, (h, w) for codes 1 .. 4 and (w, h) for 5 .. 8:
//   O[y][x] = S[fy ? h - 1 - u : u][fx ? w - 1 - v : v],  (u, v) = (y, x) for 1 .. 4 and (x, y) for 5 .. 8,
//   fy for 3, 4, 6, 7 and fx for 2, 3, 7, 8
// (1 as stored, 2 mirrored, 3 half turn, 4 upside down, 5 transposed, 6 quarter turn clockwise, 7 transverse, 8 quarter turn counter-
// clockwise).  The pixels crop_y .. crop_y + crop_h - 1, crop_x .. crop_x + crop_w - 1 of O go to the page rectangle whose top-left
// is (x, y), each byte v as it is or as 255 - v (invert).  The rectangles of a page's items are apart; what no item covers is 255.
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "rtn.h"
#if !defined(__HIPCC__) && !defined(__host__)      // a plain C++ compiler (host-only sanitizer builds)
#define __host__
#define __device__
#endif

constexpr int CMP_MAX_SIDE = 65535;                // of a page and of an image
constexpr int CMP_MAX_ITEMS = 1 << 20;
constexpr int CMP_MAX_PAGES = 1 << 20;
constexpr int CMP_THREADS = 256;
constexpr int CMP_TILE = 64;                       // a workgroup of the compose kernel owns 64 x 64 destination pixels
constexpr int CMP_PITCH = CMP_TILE * 3 + 4;        // bytes of an LDS tile row: 49 dwords, odd, so the rows a wave reads lie in different banks
constexpr int CMP_FILL_ROWS = 16;                  // rows of a page a workgroup of the fill kernel owns

struct CmpItem {                                   // 72 bytes
    const uint8_t* src;
    uint8_t* dst;                                  // the page
    int64_t tile_begin;                            // the item's first tile in the flat list of tiles
    int32_t h, w;                                  // of the decoded image
    int32_t page_w;                                // pixels of a page row
    int32_t orientation, invert;
    int32_t x, y;                                  // top-left of the destination rectangle
    int32_t cx, cy, cw, ch;                        // the rectangle of the oriented image that goes there
    int32_t tiles_x;
};
static_assert(sizeof(CmpItem) == 72, "compose item table layout");

struct CmpFill {                                   // 32 bytes: a page that its items do not cover
    uint8_t* dst;
    int64_t tile_begin;                            // the page's first tile in the flat list of row tiles
    int32_t h, w;
    int32_t item_first, item_count;                // its items in the table, which is in page order
};
static_assert(sizeof(CmpFill) == 32, "compose fill table layout");

// ---- per-pixel rules ----------------------------------------------------------------------------------------------------------------------
__host__ __device__ inline bool cmp_transposed(int o) { return o >= 5; }
__host__ __device__ inline bool cmp_flip_y(int o) { return o == 3 || o == 4 || o == 6 || o == 7; }
__host__ __device__ inline bool cmp_flip_x(int o) { return o == 2 || o == 3 || o == 7 || o == 8; }

// the pixel of S that O[oy][ox] shows, as a pixel index into S
__host__ __device__ inline int64_t cmp_source_pixel(int h, int w, int o, int oy, int ox) {
    const int u = cmp_transposed(o) ? ox : oy, v = cmp_transposed(o) ? oy : ox;
    const int sy = cmp_flip_y(o) ? h - 1 - u : u, sx = cmp_flip_x(o) ? w - 1 - v : v;
    return (int64_t)sy * w + sx;
}

template <class T>
__host__ __device__ inline int cmp_of_tile(const T* table, int n, int64_t tile) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].tile_begin <= tile) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// ---- argument checks and the tables the device entry and the twin share -------------------------------------------------------------------
// items_out: the items in page order (stable); fills_out: the pages with uncovered pixels; *tiles, *fill_tiles: the lengths of the two
// flat tile lists.  Null, or why the batch is refused; nothing is launched or written then.
inline const char* cmp_plan(int n_items, const rtn_compose_item_t* items, int n_pages, uint8_t* const* pages, const int32_t* widths,
                            const int32_t* heights, std::vector<CmpItem>* items_out, std::vector<CmpFill>* fills_out, int64_t* tiles,
                            int64_t* fill_tiles) {
    if (n_items < 0 || n_items > CMP_MAX_ITEMS) return "0 .. 1048576 items expected";
    if (n_pages < 0 || n_pages > CMP_MAX_PAGES) return "0 .. 1048576 pages expected";
    if (n_items && !items) return "the items expected";
    if (n_pages && (!pages || !widths || !heights)) return "the pages and their sizes expected";
    for (int p = 0; p < n_pages; ++p) {
        if (!pages[p]) return "a page is missing";
        if (widths[p] < 1 || heights[p] < 1 || widths[p] > CMP_MAX_SIDE || heights[p] > CMP_MAX_SIDE) return "a page has a side outside 1 .. 65535";
    }
    std::vector<int32_t> order((size_t)n_items);
    for (int i = 0; i < n_items; ++i) {
        const rtn_compose_item_t& it = items[i];
        order[(size_t)i] = i;
        if (!it.src) return "an item has no image";
        if (it.h < 1 || it.w < 1 || it.h > CMP_MAX_SIDE || it.w > CMP_MAX_SIDE) return "an image has a side outside 1 .. 65535";
        if (it.orientation < 1 || it.orientation > 8) return "an orientation code outside 1 .. 8";
        if (it.invert != 0 && it.invert != 1) return "invert must be 0 or 1";
        if (it.page < 0 || it.page >= n_pages) return "an item names a page outside the batch";
        const int oh = cmp_transposed(it.orientation) ? it.w : it.h, ow = cmp_transposed(it.orientation) ? it.h : it.w;
        if (it.crop_w < 1 || it.crop_h < 1 || it.crop_x < 0 || it.crop_y < 0 || it.crop_x > ow - it.crop_w || it.crop_y > oh - it.crop_h)
            return "a rectangle is outside its image as the orientation turns it";
        if (it.x < 0 || it.y < 0 || it.x > widths[it.page] - it.crop_w || it.y > heights[it.page] - it.crop_h)
            return "a rectangle is outside its page";
    }
    // page order, then top to bottom: two rectangles of a page overlap only if the later one starts above the earlier one's end
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
        return items[a].page != items[b].page ? items[a].page < items[b].page : items[a].y < items[b].y;
    });
    for (size_t a = 0; a < order.size(); ++a) {
        const rtn_compose_item_t& p = items[order[a]];
        for (size_t b = a + 1; b < order.size(); ++b) {
            const rtn_compose_item_t& q = items[order[b]];
            if (q.page != p.page || q.y >= p.y + p.crop_h) break;
            if (q.x < p.x + p.crop_w && p.x < q.x + q.crop_w) return "two items of a page overlap";
        }
    }
    items_out->assign((size_t)n_items, CmpItem());
    fills_out->clear();
    int64_t tile = 0, fill_tile = 0;
    size_t k = 0;
    for (int p = 0; p < n_pages; ++p) {
        const size_t first = k;
        int64_t covered = 0;
        for (; k < order.size() && items[order[k]].page == p; ++k) {
            const rtn_compose_item_t& it = items[order[k]];
            CmpItem& e = (*items_out)[k];
            memset(&e, 0, sizeof(e));
            e.src = it.src;
            e.dst = pages[p];
            e.tile_begin = tile;
            e.h = it.h;
            e.w = it.w;
            e.page_w = widths[p];
            e.orientation = it.orientation;
            e.invert = it.invert;
            e.x = it.x;
            e.y = it.y;
            e.cx = it.crop_x;
            e.cy = it.crop_y;
            e.cw = it.crop_w;
            e.ch = it.crop_h;
            e.tiles_x = (it.crop_w + CMP_TILE - 1) / CMP_TILE;
            tile += (int64_t)e.tiles_x * ((it.crop_h + CMP_TILE - 1) / CMP_TILE);
            covered += (int64_t)it.crop_w * it.crop_h;
        }
        if (covered == (int64_t)widths[p] * heights[p]) continue;
        CmpFill f;
        memset(&f, 0, sizeof(f));
        f.dst = pages[p];
        f.tile_begin = fill_tile;
        f.h = heights[p];
        f.w = widths[p];
        f.item_first = (int32_t)first;
        f.item_count = (int32_t)(k - first);
        fills_out->push_back(f);
        fill_tile += (heights[p] + CMP_FILL_ROWS - 1) / CMP_FILL_ROWS;
    }
    if (tile > 0x7fffffff || fill_tile > 0x7fffffff) return "more tiles than one launch takes";
    *tiles = tile;
    *fill_tiles = fill_tile;
    return nullptr;
}

// ---- the CPU twin: per destination pixel, no tiles ------------------------------------------------------------------------------------------
inline const char* cmp_host(int n_items, const rtn_compose_item_t* items, int n_pages, uint8_t* const* pages, const int32_t* widths,
                            const int32_t* heights) {
    std::vector<CmpItem> table;
    std::vector<CmpFill> fills;
    int64_t tiles = 0, fill_tiles = 0;
    if (const char* why = cmp_plan(n_items, items, n_pages, pages, widths, heights, &table, &fills, &tiles, &fill_tiles)) return why;
    for (const CmpFill& f : fills) memset(f.dst, 255, (size_t)f.h * (size_t)f.w * 3);
    for (const CmpItem& e : table) {
        const uint8_t flip = e.invert ? 255 : 0;
        for (int y = 0; y < e.ch; ++y) {
            uint8_t* out = e.dst + ((size_t)(e.y + y) * (size_t)e.page_w + (size_t)e.x) * 3;
            for (int x = 0; x < e.cw; ++x, out += 3) {
                const uint8_t* px = e.src + (size_t)cmp_source_pixel(e.h, e.w, e.orientation, e.cy + y, e.cx + x) * 3;
                out[0] = px[0] ^ flip;
                out[1] = px[1] ^ flip;
                out[2] = px[2] ^ flip;
            }
        }
    }
    return nullptr;
}
