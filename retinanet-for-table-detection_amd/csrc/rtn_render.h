// rtn_render.h — the text that the detection renderer (csrc/rtn_render.hip) and its CPU twins share: the tables, the
// argument checks that build them, the per-pixel rule, the tile's operation test and the 16-byte unit of the tile walk, as
// __host__ __device__ functions.  A plain C++17 compiler compiles this header (no HIP), so that csrc/rtn_render.hip and a
// stand-alone sanitizer build (tools/render_fuzz.cpp) compile the same text.
//
// The rule (model/utils.py render_detections: for each kept detection j, outline j, crop j, caption j): an output image shows the
// outlines 0 .. n_outline - 1 and the captions 0 .. n_caption - 1 of its page, and a pixel takes the value of the last operation
// that covers it.  Scanning j from high to low: caption j (if j < n_caption and the pixel's mask bit is set) gives 0,0,255;
// otherwise outline j (if j < n_outline and the pixel lies in one of draw_box's four bands) gives 0,0,0; otherwise j - 1; at the
// end the source pixel.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "rtn.h"
#if !defined(__HIPCC__) && !defined(__host__)      // a plain C++ compiler (host-only fuzzing builds)
#define __host__
#define __device__
#endif

constexpr int RND_TILE_W = 256;                // pixels of an output row a workgroup owns
constexpr int RND_TILE_H = 16;                 // rows
constexpr int RND_THREADS = 256;
constexpr int RND_UNITS = RND_TILE_W * 3 / 16 + 2;      // 16-byte destination units a tile row can touch, whatever its alignment
constexpr int RND_MAX_SIDE = 65500;            // the image writers' limit
constexpr int RND_MAX_COORD = 1 << 30;
constexpr int RND_MAX_THICKNESS = 1 << 16;

struct RPage {                                 // 24 bytes
    const uint8_t* src;
    int32_t H, W, op_begin, op_count;
};
struct ROp {                                   // 48 bytes
    int32_t x1, y1, x2, y2;                    // sorted corners (draw_box)
    int32_t cx, cy, cw, ch;                    // caption: the mask's first pixel on the page, its width and height
    int64_t mask_bit;
    int32_t pitch, pad_;
};
struct ROut {                                  // 40 bytes
    int64_t off;
    int32_t page, x0, y0, w, h, n_outline, n_caption, tiles_x;
};
static_assert(sizeof(RPage) == 24 && sizeof(ROp) == 48 && sizeof(ROut) == 40, "render table layout");

struct RTables {
    const RPage* pages;
    const ROp* ops;
    const ROut* outs;
    const int32_t* tile_begin;                 // n_out + 1: first tile of every output image, then the total
    const uint8_t* masks;
    uint8_t* out;
    int32_t n_out, lo, hi;                     // lo = t / 2, hi = t - t / 2
};

// ---- the rule ---------------------------------------------------------------------------------------------------------------------
// what operation `o` makes of page pixel (x, y): 2 = caption colour, 1 = outline colour, 0 = nothing
__host__ __device__ inline int render_op_code(const ROp& o, bool outline, bool caption, int x, int y, int lo, int hi,
                                              const uint8_t* masks) {
    if (caption) {
        const int dx = x - o.cx, dy = y - o.cy;
        if (dx >= 0 && dx < o.cw && dy >= 0 && dy < o.ch) {
            const int64_t bit = o.mask_bit + (int64_t)dy * o.pitch + dx;
            if ((masks[bit >> 3] >> (bit & 7)) & 1) return 2;
        }
    }
    if (outline && x >= o.x1 - lo && x < o.x2 + hi && y >= o.y1 - lo && y < o.y2 + hi &&
        (y < o.y1 + hi || y >= o.y2 - lo || x < o.x1 + hi || x >= o.x2 - lo))
        return 1;
    return 0;
}

// the whole scan for one pixel of output image `o` (ops: the page's first operation)
__host__ __device__ inline int render_pixel_code(const ROp* ops, const ROut& o, int x, int y, int lo, int hi, const uint8_t* masks) {
    for (int j = (o.n_outline > o.n_caption ? o.n_outline : o.n_caption) - 1; j >= 0; --j) {
        const int c = render_op_code(ops[j], j < o.n_outline, j < o.n_caption, x, y, lo, hi, masks);
        if (c) return c;
    }
    return 0;
}

// can operation `o` change a pixel of the page rectangle [X0, X1) x [Y0, Y1)?  (An outline does not when the rectangle lies in
// its hole.)
__host__ __device__ inline bool render_op_hits(const ROp& o, bool outline, bool caption, int X0, int Y0, int X1, int Y1, int lo,
                                               int hi) {
    if (caption && o.cw > 0 && o.ch > 0 && o.cx < X1 && o.cx + o.cw > X0 && o.cy < Y1 && o.cy + o.ch > Y0) return true;
    return outline && lo + hi > 0 && o.x1 - lo < X1 && o.x2 + hi > X0 && o.y1 - lo < Y1 && o.y2 + hi > Y0 &&
           !(X0 >= o.x1 + hi && X1 <= o.x2 - lo && Y0 >= o.y1 + hi && Y1 <= o.y2 - lo);
}

// ---- the tile walk's unit ---------------------------------------------------------------------------------------------------------
// Unit u of row y of an output image's tile: the tile owns bytes [b0, b1) of the (3 w)-byte row, and unit u is what of them lies in
// the u-th 16-byte-aligned chunk of destination memory from the row's first byte on.  A whole chunk is loaded as aligned 4-byte
// source words (shifted into place) where those words lie inside the page, and stored as one 16-byte word; everything else moves
// byte by byte, so nothing outside the page is read and nothing outside [b0, b1) is written.  hits[0 .. nhit): the page's
// operations that can change the tile, in drawing order.
__host__ __device__ inline void render_unit(const RTables& t, const RPage& pg, const ROut& o, const uint16_t* hits, int nhit, int y,
                                            int b0, int b1, int u) {
    uint8_t* drow = t.out + o.off + (int64_t)y * o.w * 3;
    const int mis = (int)((uintptr_t)(drow + b0) & 15);
    const int cb = b0 - mis + 16 * u;                          // the chunk's first byte, as a byte of the row (may lie before b0)
    const int lo_b = cb > b0 ? cb : b0, hi_b = cb + 16 < b1 ? cb + 16 : b1;
    if (lo_b >= hi_b) return;
    const int k0 = lo_b - cb, k1 = hi_b - cb;                   // the chunk's bytes [k0, k1) are the tile's
    const uint8_t* S = pg.src + ((int64_t)(o.y0 + y) * pg.W + o.x0) * 3 + lo_b;
    uint32_t v[4] = {0u, 0u, 0u, 0u};
    const bool whole = k1 - k0 == 16;
    bool words = false;
    if (whole) {
        const int sh = (int)((uintptr_t)S & 3);
        const uint8_t* sa = S - sh;
        const uint8_t* end = pg.src + (int64_t)pg.H * pg.W * 3;
        if (sa >= pg.src && sa + (sh ? 20 : 16) <= end) {
            const uint32_t* w = reinterpret_cast<const uint32_t*>(sa);
            words = true;
            if (sh == 0) {
                v[0] = w[0]; v[1] = w[1]; v[2] = w[2]; v[3] = w[3];
            } else {
                const uint32_t a0 = w[0], a1 = w[1], a2 = w[2], a3 = w[3], a4 = w[4];
                const int r = 8 * sh, l = 32 - r;
                v[0] = (a0 >> r) | (a1 << l); v[1] = (a1 >> r) | (a2 << l); v[2] = (a2 >> r) | (a3 << l); v[3] = (a3 >> r) | (a4 << l);
            }
        }
    }
    if (!words) {
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (k >= k0 && k < k1) v[k >> 2] |= (uint32_t)S[k - k0] << (8 * (k & 3));
    }
    if (nhit > 0) {
        const int p0 = lo_b / 3, c0 = lo_b - 3 * p0;
        const int npx = (c0 + (k1 - k0) + 2) / 3;              // <= 6 pixels
        const ROp* ops = t.ops + pg.op_begin;
        uint32_t codes = 0;
        for (int i = 0; i < npx; ++i) {
            int c = 0;
            for (int q = nhit - 1; q >= 0 && !c; --q) {
                const int j = hits[q];
                c = render_op_code(ops[j], j < o.n_outline, j < o.n_caption, o.x0 + p0 + i, o.y0 + y, t.lo, t.hi, t.masks);
            }
            codes |= (uint32_t)c << (2 * i);
        }
        if (codes) {
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                if (k < k0 || k >= k1) continue;
                const int q = c0 + k - k0, i = q / 3, ch = q - 3 * i;
                const uint32_t c = (codes >> (2 * i)) & 3u;
                if (c) {
                    const uint32_t byte = (c == 2 && ch == 2) ? 255u : 0u;
                    v[k >> 2] = (v[k >> 2] & ~(0xffu << (8 * (k & 3)))) | (byte << (8 * (k & 3)));
                }
            }
        }
    }
    uint8_t* D = drow + cb;                                     // 16-byte aligned
    if (whole) {
#if defined(__HIP_DEVICE_COMPILE__)
        *reinterpret_cast<uint4*>(D) = make_uint4(v[0], v[1], v[2], v[3]);
#else
        uint32_t* d = reinterpret_cast<uint32_t*>(D);
        d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3];
#endif
    } else {
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (k >= k0 && k < k1) D[k] = (uint8_t)(v[k >> 2] >> (8 * (k & 3)));
    }
}

// the tile `lt` of output image o: rows [r0, r1), row bytes [b0, b1), and its rectangle on the page
struct RTile { int r0, r1, b0, b1, X0, Y0, X1, Y1; };
__host__ __device__ inline RTile render_tile(const ROut& o, int lt) {
    const int ty = lt / o.tiles_x, tx = lt - ty * o.tiles_x;
    RTile r;
    r.r0 = ty * RND_TILE_H;
    r.r1 = r.r0 + RND_TILE_H < o.h ? r.r0 + RND_TILE_H : o.h;
    const int p0 = tx * RND_TILE_W, p1 = p0 + RND_TILE_W < o.w ? p0 + RND_TILE_W : o.w;
    r.b0 = 3 * p0; r.b1 = 3 * p1;
    r.X0 = o.x0 + p0; r.X1 = o.x0 + p1; r.Y0 = o.y0 + r.r0; r.Y1 = o.y0 + r.r1;
    return r;
}

// ---- host: argument checks and tables ------------------------------------------------------------------------------------------------
struct RArgs {                                 // the arguments rtn_render_pages, rtn_render_host and rtn_render_tiles_host share
    int n_pages; const uint8_t* const* pages; const int32_t *heights, *widths, *op_begin;
    int n_ops; const int32_t *boxes, *captions; const int64_t* mask_bits; const int32_t* mask_pitch;
    const uint8_t* masks; size_t mask_bytes;
    int n_out; const int32_t *out_page, *out_rects, *out_outlines, *out_captions; const int64_t* out_offsets;
    int thickness; uint8_t* out; size_t out_bytes;
};
struct RPlan {
    std::vector<RPage> pages;
    std::vector<ROp> ops;
    std::vector<ROut> outs;
    std::vector<int32_t> tile_begin;
    int lo, hi;
};

#define RND_FAIL(...) do { snprintf(why, why_n, __VA_ARGS__); return RTN_EINVAL; } while (0)
inline int render_plan(const RArgs& a, RPlan* pl, char* why, size_t why_n) {
    if (a.n_pages < 0 || a.n_ops < 0 || a.n_out < 0) RND_FAIL("a negative count");
    if (a.thickness < 0 || a.thickness > RND_MAX_THICKNESS) RND_FAIL("thickness %d outside 0..%d", a.thickness, RND_MAX_THICKNESS);
    if (a.n_out == 0) return RTN_OK;
    if (a.n_pages == 0 || !a.pages || !a.heights || !a.widths || !a.op_begin || !a.out_page || !a.out_rects || !a.out_outlines ||
        !a.out_captions || !a.out_offsets || !a.out)
        RND_FAIL("NULL argument");
    if (a.n_ops && (!a.boxes || !a.captions || !a.mask_bits || !a.mask_pitch)) RND_FAIL("NULL operation table");
    if (a.mask_bytes && !a.masks) RND_FAIL("NULL masks");
    pl->lo = a.thickness / 2;
    pl->hi = a.thickness - a.thickness / 2;
    pl->pages.resize(a.n_pages);
    const uint8_t* out_end = a.out + a.out_bytes;
    for (int p = 0; p < a.n_pages; ++p) {
        const int H = a.heights[p], W = a.widths[p], b = a.op_begin[p], e = a.op_begin[p + 1];
        if (!a.pages[p]) RND_FAIL("page %d is NULL", p);
        if (H < 1 || H > RND_MAX_SIDE || W < 1 || W > RND_MAX_SIDE) RND_FAIL("page %d: %dx%d: sides must be 1..%d", p, H, W, RND_MAX_SIDE);
        if (b < 0 || e < b || e > a.n_ops) RND_FAIL("page %d: operations [%d, %d) of %d", p, b, e, a.n_ops);
        if (e - b > RTN_RENDER_MAX_OPS) RND_FAIL("page %d: %d operations, at most %d", p, e - b, RTN_RENDER_MAX_OPS);
        if (a.pages[p] < out_end && a.out < a.pages[p] + (int64_t)H * W * 3) RND_FAIL("page %d overlaps the output buffer", p);
        pl->pages[p] = RPage{a.pages[p], H, W, b, e - b};
    }
    pl->ops.resize(a.n_ops);
    for (int j = 0; j < a.n_ops; ++j) {
        const int32_t* b = a.boxes + 4 * j;
        const int32_t* c = a.captions + 4 * j;
        for (int k = 0; k < 4; ++k)
            if (b[k] < -RND_MAX_COORD || b[k] > RND_MAX_COORD) RND_FAIL("operation %d: box coordinate %d", j, b[k]);
        if (c[0] < -RND_MAX_COORD || c[0] > RND_MAX_COORD || c[1] < -RND_MAX_COORD || c[1] > RND_MAX_COORD)
            RND_FAIL("operation %d: caption origin (%d, %d)", j, c[0], c[1]);
        if (c[2] < 0 || c[2] > RND_MAX_SIDE || c[3] < 0 || c[3] > RND_MAX_SIDE) RND_FAIL("operation %d: caption mask %dx%d", j, c[3], c[2]);
        ROp& o = pl->ops[j];
        o.x1 = b[0] < b[2] ? b[0] : b[2]; o.x2 = b[0] < b[2] ? b[2] : b[0];
        o.y1 = b[1] < b[3] ? b[1] : b[3]; o.y2 = b[1] < b[3] ? b[3] : b[1];
        o.cx = c[0]; o.cy = c[1]; o.cw = c[2]; o.ch = c[3];
        o.mask_bit = 0; o.pitch = 0; o.pad_ = 0;
        if (c[2] > 0 && c[3] > 0) {
            const int64_t bit = a.mask_bits[j];
            const int pitch = a.mask_pitch[j];
            if (pitch < c[2] || pitch > (1 << 20)) RND_FAIL("operation %d: mask pitch %d for %d columns", j, pitch, c[2]);
            if (bit < 0 || (uint64_t)bit > 8 * (uint64_t)a.mask_bytes ||
                (uint64_t)(c[3] - 1) * pitch + c[2] > 8 * (uint64_t)a.mask_bytes - (uint64_t)bit)
                RND_FAIL("operation %d: mask bits leave the %zu mask bytes", j, a.mask_bytes);
            o.mask_bit = bit; o.pitch = pitch;
        } else {
            o.cw = o.ch = 0;
        }
    }
    pl->outs.resize(a.n_out);
    pl->tile_begin.resize(a.n_out + 1);
    int64_t tiles = 0;
    std::vector<std::pair<int64_t, int64_t>> spans(a.n_out);
    for (int i = 0; i < a.n_out; ++i) {
        const int p = a.out_page[i];
        const int32_t* r = a.out_rects + 4 * i;
        if (p < 0 || p >= a.n_pages) RND_FAIL("output %d: page %d of %d", i, p, a.n_pages);
        const RPage& pg = pl->pages[p];
        if (r[0] < 0 || r[1] < 0 || r[2] < 1 || r[3] < 1 || r[0] > pg.W - r[2] || r[1] > pg.H - r[3])
            RND_FAIL("output %d: rectangle x %d y %d w %d h %d on a %dx%d page", i, r[0], r[1], r[2], r[3], pg.H, pg.W);
        if (a.out_outlines[i] < 0 || a.out_outlines[i] > pg.op_count || a.out_captions[i] < 0 || a.out_captions[i] > pg.op_count)
            RND_FAIL("output %d: %d outlines, %d captions of %d operations", i, a.out_outlines[i], a.out_captions[i], pg.op_count);
        const int64_t bytes = (int64_t)r[2] * r[3] * 3, off = a.out_offsets[i];
        if (off < 0 || (uint64_t)off > a.out_bytes || (uint64_t)bytes > a.out_bytes - (uint64_t)off)
            RND_FAIL("output %d: bytes [%lld, %lld) of %zu", i, (long long)off, (long long)(off + bytes), a.out_bytes);
        spans[i] = {off, off + bytes};
        ROut& o = pl->outs[i];
        o.off = off; o.page = p; o.x0 = r[0]; o.y0 = r[1]; o.w = r[2]; o.h = r[3];
        o.n_outline = a.out_outlines[i]; o.n_caption = a.out_captions[i];
        o.tiles_x = (r[2] + RND_TILE_W - 1) / RND_TILE_W;
        pl->tile_begin[i] = (int32_t)tiles;
        tiles += (int64_t)o.tiles_x * ((r[3] + RND_TILE_H - 1) / RND_TILE_H);
        if (tiles > 0x7fffffff) RND_FAIL("more than 2^31 - 1 tiles");
    }
    pl->tile_begin[a.n_out] = (int32_t)tiles;
    std::sort(spans.begin(), spans.end());
    for (int i = 1; i < a.n_out; ++i)
        if (spans[i].first < spans[i - 1].second) RND_FAIL("two output images overlap at byte %lld", (long long)spans[i].first);
    return RTN_OK;
}
#undef RND_FAIL

inline RTables render_tables(const RPlan& pl, const RArgs& a) {
    return RTables{pl.pages.data(), pl.ops.data(), pl.outs.data(), pl.tile_begin.data(), a.masks, a.out, a.n_out, pl.lo, pl.hi};
}

// the twin: the rule for every pixel of every output image
inline void render_pixels_host(const RTables& t) {
    for (int i = 0; i < t.n_out; ++i) {
        const ROut& o = t.outs[i];
        const RPage& pg = t.pages[o.page];
        for (int y = 0; y < o.h; ++y) {
            const uint8_t* s = pg.src + ((int64_t)(o.y0 + y) * pg.W + o.x0) * 3;
            uint8_t* d = t.out + o.off + (int64_t)y * o.w * 3;
            for (int x = 0; x < o.w; ++x) {
                const int c = render_pixel_code(t.ops + pg.op_begin, o, o.x0 + x, o.y0 + y, t.lo, t.hi, t.masks);
                d[3 * x] = c ? 0 : s[3 * x];
                d[3 * x + 1] = c ? 0 : s[3 * x + 1];
                d[3 * x + 2] = c == 2 ? 255 : c ? 0 : s[3 * x + 2];
            }
        }
    }
}

// the kernel's walk, one tile after another: collect the operations that meet the tile, then its rows unit by unit
inline void render_tiles_host(const RTables& t) {
    std::vector<uint16_t> hits(RTN_RENDER_MAX_OPS);
    for (int i = 0; i < t.n_out; ++i) {
        const ROut& o = t.outs[i];
        const RPage& pg = t.pages[o.page];
        const int nmax = o.n_outline > o.n_caption ? o.n_outline : o.n_caption;
        for (int lt = 0; lt < t.tile_begin[i + 1] - t.tile_begin[i]; ++lt) {
            const RTile r = render_tile(o, lt);
            int nhit = 0;
            for (int j = 0; j < nmax; ++j)
                if (render_op_hits(t.ops[pg.op_begin + j], j < o.n_outline, j < o.n_caption, r.X0, r.Y0, r.X1, r.Y1, t.lo, t.hi))
                    hits[nhit++] = (uint16_t)j;
            for (int y = r.r0; y < r.r1; ++y)
                for (int u = 0; u < RND_UNITS; ++u) render_unit(t, pg, o, hits.data(), nhit, y, r.b0, r.b1, u);
        }
    }
}
