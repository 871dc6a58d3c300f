// rtn_png_layout.h — the pixel layouts of PNG beyond whole 8-bit gray and R,G,B samples ("Pixel layouts"): sub-byte gray, palette,
// alpha, 16-bit samples and the seven Adam7 passes.  The geometry of a page's filtered stream, the filter arithmetic and the
// expansion of one output pixel, as __host__ __device__ functions: csrc/rtn_png_stream.hip calls them from its kernels,
// pl_pixels_host (below) runs the same functions on a CPU, and tools/png_layout_fuzz.cpp compiles this text on its own.
#pragma once
#include <stdint.h>
#include <string.h>
#include <vector>
#include "rtn_png_inflate.h"

constexpr uint32_t PL_MAGIC = 0x4c4e5052u;     // "RPNL"

// The format word of a page: depth | colour type << 8 | interlace << 16 | palette entries << 20.
__host__ __device__ inline uint32_t pl_fmt(int depth, int ctype, int interlace, int npal) {
    return (uint32_t)depth | (uint32_t)ctype << 8 | (uint32_t)interlace << 16 | (uint32_t)npal << 20;
}
__host__ __device__ inline int pl_depth(uint32_t fmt) { return (int)(fmt & 255u); }
__host__ __device__ inline int pl_ctype(uint32_t fmt) { return (int)((fmt >> 8) & 255u); }
__host__ __device__ inline int pl_interlace(uint32_t fmt) { return (int)((fmt >> 16) & 15u); }
__host__ __device__ inline int pl_npal(uint32_t fmt) { return (int)((fmt >> 20) & 511u); }

// Samples per pixel of a colour type; 0: no such type.
__host__ __device__ inline int pl_samples(int ctype) { return ctype == 0 ? 1 : ctype == 2 ? 3 : ctype == 3 ? 1 : ctype == 4 ? 2 : ctype == 6 ? 4 : 0; }

// The (type, depth) pairs the layout decoder takes: every legal pair but 16-bit gray (Pillow clips it; it stays on the host).
__host__ __device__ inline bool pl_accepts(int ctype, int depth) {
    if (ctype == 0) return depth == 1 || depth == 2 || depth == 4 || depth == 8;
    if (ctype == 3) return depth == 1 || depth == 2 || depth == 4 || depth == 8;
    if (ctype == 2 || ctype == 4 || ctype == 6) return depth == 8 || depth == 16;
    return false;
}

// A whole format word: an accepted pair, interlace 0 or 1, 1 .. 2^depth palette entries for a palette page and none otherwise.
__host__ __device__ inline bool pl_fmt_ok(uint32_t fmt) {
    if ((fmt >> 29) || !pl_accepts(pl_ctype(fmt), pl_depth(fmt)) || pl_interlace(fmt) > 1) return false;
    if (pl_ctype(fmt) == 3) return pl_npal(fmt) >= 1 && pl_npal(fmt) <= (1 << pl_depth(fmt));
    return pl_npal(fmt) == 0;
}

struct PLPass {                                // one sub-image: pixel (r, c) of the pass is pixel (y0 + r dy, x0 + c dx) of the page
    int32_t x0, y0, dx, dy, cols, rows;        // rows == 0: the pass is empty and takes no byte of the stream
    uint32_t rb;                               // bytes of one row behind its filter byte: ceil(cols * bits / 8)
    uint32_t off;                              // the filter byte of the pass's first row, in the filtered stream
};
struct PLGeom {
    PLPass p[7];
    int32_t npass;                             // 1 or 7
    int32_t bits, bpp;                         // bits per pixel; the filter distance max(1, bits / 8)
    long long stream;                          // the filtered stream's length: sum over passes of rows * (1 + rb); >= 2^31: too large
};

// The geometry of a W x H page (both >= 1) of format fmt.  stream >= 2^31 (and nothing else valid) if a row or the sum is too long.
__host__ __device__ inline void pl_geometry(int W, int H, uint32_t fmt, PLGeom* g) {
    const int X0[7] = {0, 4, 0, 2, 0, 1, 0}, Y0[7] = {0, 0, 4, 0, 2, 0, 1}, DX[7] = {8, 8, 4, 4, 2, 2, 1}, DY[7] = {8, 8, 8, 4, 4, 2, 2};
    const bool lace = pl_interlace(fmt) != 0;
    g->npass = lace ? 7 : 1;
    g->bits = pl_depth(fmt) * pl_samples(pl_ctype(fmt));
    g->bpp = g->bits >= 8 ? g->bits / 8 : 1;
    unsigned long long at = 0;
    bool big = false;
    for (int q = 0; q < 7; ++q) {
        PLPass& ps = g->p[q];
        ps.x0 = lace ? X0[q] : 0; ps.y0 = lace ? Y0[q] : 0; ps.dx = lace ? DX[q] : 1; ps.dy = lace ? DY[q] : 1;
        ps.cols = q < g->npass && W > ps.x0 ? (int32_t)(((long long)W - ps.x0 + ps.dx - 1) / ps.dx) : 0;
        ps.rows = q < g->npass && H > ps.y0 ? (int32_t)(((long long)H - ps.y0 + ps.dy - 1) / ps.dy) : 0;
        if (ps.cols == 0 || ps.rows == 0) ps.cols = ps.rows = 0;
        const unsigned long long rb = ((unsigned long long)ps.cols * (unsigned)g->bits + 7u) >> 3;
        if (rb + 1 >= (1ull << 31)) big = true;
        ps.rb = (uint32_t)rb;
        ps.off = (uint32_t)at;
        at += (unsigned long long)ps.rows * (1ull + rb);
        if (at >= (1ull << 31)) big = true;
    }
    g->stream = big ? (1ll << 62) : (long long)at;
}

// The Adam7 pass (0 .. 6) that holds pixel (y, x).
__host__ __device__ inline int pl_pass_of(int y, int x) {
    if ((y & 7) == 0 && (x & 7) == 0) return 0;
    if ((y & 7) == 0 && (x & 7) == 4) return 1;
    if ((y & 7) == 4 && (x & 3) == 0) return 2;
    if ((y & 3) == 0 && (x & 3) == 2) return 3;
    if ((y & 3) == 2 && (x & 1) == 0) return 4;
    if ((y & 1) == 0) return 5;
    return 6;
}

__host__ __device__ inline uint32_t pl_paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return (uint32_t)((pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c));
}

// One byte of a row reconstructed: a the byte bpp to the left, b the byte above, c the byte above a (0 outside the pass).
__host__ __device__ inline uint32_t pl_unfilter_byte(uint32_t type, uint32_t raw, uint32_t a, uint32_t b, uint32_t c) {
    uint32_t v = raw;
    if (type == 1u) v += a;
    else if (type == 2u) v += b;
    else if (type == 3u) v += (a + b) >> 1;
    else if (type == 4u) v += pl_paeth((int)a, (int)b, (int)c);
    return v & 255u;
}

// Pixel (y, x) of the page as B,G,R from the reconstructed stream `rec`: sub-byte samples are read MSB first (the padding bits of a
// row's last byte are never reached, c < cols), gray of depth d is scaled by 255 / (2^d - 1), a 16-bit sample gives its high byte,
// alpha is dropped, a palette index past the last entry gives (0,0,0).  pal: 3 pl_npal(fmt) bytes, R,G,B.
__host__ __device__ inline void pl_pixel(const PLGeom& g, uint32_t fmt, const uint8_t* rec, const uint8_t* pal, int y, int x,
                                         uint32_t* B, uint32_t* G, uint32_t* R) {
    const int depth = pl_depth(fmt), ctype = pl_ctype(fmt);
    const PLPass& ps = g.p[pl_interlace(fmt) ? pl_pass_of(y, x) : 0];
    const long long r = (y - ps.y0) / ps.dy, c = (x - ps.x0) / ps.dx;
    const uint8_t* row = rec + ps.off + r * (1ll + ps.rb) + 1;
    uint32_t v0, v1 = 0, v2 = 0;
    if (depth < 8) {
        const long long bit = c * depth;
        v0 = ((uint32_t)row[bit >> 3] >> (8 - depth - (int)(bit & 7))) & ((1u << depth) - 1u);
        if (ctype == 0) v0 *= 255u / ((1u << depth) - 1u);
    } else {
        const int sb = depth >> 3;
        const uint8_t* px = row + c * g.bpp;
        v0 = px[0];
        if (ctype == 2 || ctype == 6) { v1 = px[sb]; v2 = px[2 * sb]; }
    }
    if (ctype == 3) {
        const bool in = v0 < (uint32_t)pl_npal(fmt);
        *R = in ? pal[3 * v0] : 0u; *G = in ? pal[3 * v0 + 1] : 0u; *B = in ? pal[3 * v0 + 2] : 0u;
    } else if (ctype == 2 || ctype == 6) {
        *R = v0; *G = v1; *B = v2;
    } else {
        *R = *G = *B = v0;
    }
}

// The last stage on the CPU: `rec` (g.stream bytes, the filtered stream) is reconstructed in place pass by pass, then every pixel of
// the W x H page is written to out (H W 3 bytes, B,G,R).  Returns PI_FILTER, with nothing written, if a row's filter type is above 4.
inline uint32_t pl_pixels(const PLGeom& g, uint32_t fmt, int W, int H, uint8_t* rec, const uint8_t* pal, uint8_t* out) {
    for (int q = 0; q < g.npass; ++q)
        for (long long r = 0; r < g.p[q].rows; ++r)
            if (rec[g.p[q].off + r * (1ll + g.p[q].rb)] > 4) return (uint32_t)PI_FILTER;
    for (int q = 0; q < g.npass; ++q) {
        const PLPass& ps = g.p[q];
        for (long long r = 0; r < ps.rows; ++r) {
            uint8_t* row = rec + ps.off + r * (1ll + ps.rb);
            const uint8_t* up = r ? row - (1ll + ps.rb) + 1 : nullptr;
            const uint32_t type = row[0];
            ++row;
            for (uint32_t i = 0; i < ps.rb; ++i) {
                const bool left = i >= (uint32_t)g.bpp;
                row[i] = (uint8_t)pl_unfilter_byte(type, row[i], left ? row[i - g.bpp] : 0u, up ? up[i] : 0u, up && left ? up[i - g.bpp] : 0u);
            }
        }
    }
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            uint32_t b, gg, r;
            pl_pixel(g, fmt, rec, pal, y, x, &b, &gg, &r);
            uint8_t* o = out + ((long long)y * W + x) * 3;
            o[0] = (uint8_t)b; o[1] = (uint8_t)gg; o[2] = (uint8_t)r;
        }
    return 0u;
}
