// rtn_skew.h — the text that the skew estimator (csrc/rtn_skew.hip) and its CPU twin share: a Postl / Bloomberg
// profile sweep in integers, as __host__ __device__ functions.  A plain C++17 compiler compiles this header (no HIP).  Its users are
// compiled with -ffp-contract=off: the four double operations of an Otsu candidate are one rounding each.  The kernels, the twin and
// the NumPy oracle (tests/skew_ref.py) give the same bits.
//
// Per page (uint8 (H, W) gray or (H, W, 3) B,G,R, sides 1 .. 32767, rows without padding):
//   gray      cca_gray's rule (rtn_cca.h): (1868 B + 9617 G + 4899 R + 8192) >> 14; a gray page as it is
//   t         the caller's threshold 1 .. 255, or for 0 Otsu's on the 256-bin histogram: for t = 1 .. 255 with w0 = sum_{g<t} h[g],
//             m0 = sum_{g<t} g h[g], w1 = N - w0, m1 = M - m0 (int64), skipping w0 == 0 and w1 == 0, d = m0/w0 - m1/w1 and
//             v = w0 * w1 * d * d in double, left to right; the smallest t of the largest v.  No candidate (a constant page): t = 0,
//             which makes no pixel ink
//   ink       gray < t
//   C[y][b]   the ink pixels of row y in columns [b band, min(W, (b + 1) band)), band in {8, 16, 32, 64}, NB = ceil(W / band) bands
//   shift     of band b at shear factor T (tan(angle) * 65536, |T| <= 17561): floor(((b band + band/2 - W/2) T + 32768) / 65536)
//   P_k[r]    sum_b C[r + shift][b] over the bands whose r + shift lies in [0, H)
//   S_k       sum_{r=0}^{H-2} (P_k[r+1] - P_k[r])^2 in uint64
//   best      the k of the largest S_k; ties go to the smallest |k - n_steps| (K = 2 n_steps + 1), then to the smaller k
// In memory the counts are band-major, Ct[b * H + y] (one byte each): the sweep reads a band's column at consecutive rows.
#pragma once
#include <stdint.h>
#include <string.h>
#include <vector>
#include "rtn.h"
#if !defined(__HIPCC__) && !defined(__host__)      // a plain C++ compiler (host-only sanitizer builds)
#define __host__
#define __device__
#endif

constexpr int SKW_MAX_SIDE = 32767;                // rtn_warp_affine_u8's limit; a profile entry (<= W) fits uint16
constexpr int SKW_MAX_PAGES = 65535;
constexpr int SKW_MAX_ANGLES = 401;
constexpr int SKW_MAX_SHEAR = 17561;               // rint(tan(15 degrees) * 65536)
constexpr int SKW_THREADS = 256;
constexpr int SKW_TILE_ROWS = 16;                  // rows of a page a workgroup of the pixel passes owns: four per wave
constexpr int SKW_CHUNK = 256;                     // pixels of a row a wave takes per step: four per lane; every band width divides it

struct SkwPage {                                   // 40 bytes
    const uint8_t* src;
    int64_t counts_off;                            // byte offset of the page's band-major counts in the counts block
    int64_t tile_begin;                            // the page's first tile in the flat list of row tiles
    int32_t h, w, c, nb;
};
static_assert(sizeof(SkwPage) == 40, "skew table layout");

// ---- per-pixel and per-candidate rules --------------------------------------------------------------------------------------------------
__host__ __device__ inline int skw_gray3(int b, int g, int r) { return (1868 * b + 9617 * g + 4899 * r + 8192) >> 14; }

// the between-class term of candidate t, or -1 where one class is empty (a valid term is positive: m0/w0 < t <= m1/w1)
__host__ __device__ inline double skw_otsu_term(int64_t w0, int64_t m0, int64_t N, int64_t M) {
    const int64_t w1 = N - w0, m1 = M - m0;
    if (w0 == 0 || w1 == 0) return -1.0;
    const double a = (double)m0 / (double)w0;
    const double b = (double)m1 / (double)w1;
    const double d = a - b;
    double v = (double)w0 * (double)w1;
    v = v * d;
    v = v * d;
    return v;
}

// candidate (v, t) beats (bv, bt): larger term, then smaller t
__host__ __device__ inline bool skw_otsu_better(double v, int t, double bv, int bt) { return v > bv || (v == bv && t < bt); }

__host__ __device__ inline int32_t skw_shift(int b, int band, int w, int32_t shear) {
    const int64_t dx = (int64_t)b * band + band / 2 - w / 2;
    return (int32_t)((dx * shear + 32768) >> 16);                // arithmetic shift: floor
}

// angle (s, k) beats (bs, bk)
__host__ __device__ inline bool skw_pick_better(uint64_t s, int k, uint64_t bs, int bk, int n_steps) {
    if (s != bs) return s > bs;
    const int a = k < n_steps ? n_steps - k : k - n_steps, b = bk < n_steps ? n_steps - bk : bk - n_steps;
    return a != b ? a < b : k < bk;
}

__host__ __device__ inline int skw_page_of_tile(const SkwPage* table, int n, int64_t tile) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].tile_begin <= tile) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// ---- argument checks and the page table the device entry and the twin share -------------------------------------------------------------
inline int64_t skw_align(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

inline const char* skw_check_sizes(int n, const int32_t* heights, const int32_t* widths, int band, int K) {
    if (n < 0 || n > SKW_MAX_PAGES) return "0 .. 65535 pages expected";
    if (band != 8 && band != 16 && band != 32 && band != 64) return "the band width must be 8, 16, 32 or 64";
    if (K < 1 || K > SKW_MAX_ANGLES || !(K & 1)) return "an odd number of 1 .. 401 shear factors expected";
    if (n && (!heights || !widths)) return "the pages' sizes expected";
    for (int i = 0; i < n; ++i)
        if (heights[i] < 1 || widths[i] < 1 || heights[i] > SKW_MAX_SIDE || widths[i] > SKW_MAX_SIDE) return "a page has a side outside 1 .. 32767";
    return nullptr;
}

// table: n entries (may be null: sizes only); counts_bytes: the size of the counts block; tiles: the flat list's length
inline const char* skw_plan(int n, const uint8_t* const* pages, const int32_t* heights, const int32_t* widths, const int32_t* channels,
                            int threshold, int band, int K, const int32_t* shear_q16, SkwPage* table, int64_t* counts_bytes, int64_t* tiles,
                            int* max_h, int* max_nb) {
    if (const char* why = skw_check_sizes(n, heights, widths, band, K)) return why;
    if (threshold < 0 || threshold > 255) return "the threshold must be 0 (Otsu) or 1 .. 255";
    if (!shear_q16) return "the shear factors expected";
    for (int k = 0; k < K; ++k)
        if (shear_q16[k] < -SKW_MAX_SHEAR || shear_q16[k] > SKW_MAX_SHEAR) return "a shear factor is beyond 15 degrees (17561)";
    if (n && (!pages || !channels)) return "the pages and their channel counts expected";
    int64_t pos = 0, tile = 0;
    int mh = 0, mnb = 0;
    for (int i = 0; i < n; ++i) {
        if (!pages[i]) return "a page is missing";
        if (channels[i] != 1 && channels[i] != 3) return "a page has a channel count other than 1 or 3";
        SkwPage& e = table[i];
        memset(&e, 0, sizeof(e));
        e.src = pages[i];
        e.h = heights[i];
        e.w = widths[i];
        e.c = channels[i];
        e.nb = (widths[i] + band - 1) / band;
        e.counts_off = pos;
        e.tile_begin = tile;
        pos += skw_align((int64_t)e.h * e.nb, 16);
        tile += (e.h + SKW_TILE_ROWS - 1) / SKW_TILE_ROWS;
        mh = e.h > mh ? e.h : mh;
        mnb = e.nb > mnb ? e.nb : mnb;
    }
    *counts_bytes = pos;
    *tiles = tile;
    *max_h = mh;
    *max_nb = mnb;
    return nullptr;
}

// ---- the CPU twin ---------------------------------------------------------------------------------------------------------------------
inline int skw_host_gray(const SkwPage& p, int y, int x) {
    const uint8_t* q = p.src + ((size_t)y * p.w + x) * p.c;
    return p.c == 3 ? skw_gray3(q[0], q[1], q[2]) : q[0];
}

inline int skw_host_otsu(const SkwPage& p) {
    std::vector<int64_t> hist(256, 0);
    for (int y = 0; y < p.h; ++y)
        for (int x = 0; x < p.w; ++x) ++hist[(size_t)skw_host_gray(p, y, x)];
    int64_t N = 0, M = 0;
    for (int g = 0; g < 256; ++g) {
        N += hist[g];
        M += g * hist[g];
    }
    int64_t w0 = 0, m0 = 0;
    double bv = -1.0;
    int bt = 0;
    for (int t = 1; t < 256; ++t) {
        w0 += hist[t - 1];
        m0 += (t - 1) * hist[t - 1];
        const double v = skw_otsu_term(w0, m0, N, M);
        if (v >= 0.0 && skw_otsu_better(v, t, bv, bt)) {
            bv = v;
            bt = t;
        }
    }
    return bt;
}

// counts: h * nb bytes, band-major; profile: h entries
inline void skw_host_page(const SkwPage& p, int threshold, int band, int K, const int32_t* shear_q16, int32_t* t_out, int64_t* ink_out,
                          int32_t* best_out, uint64_t* scores, uint8_t* counts, uint16_t* profile) {
    const int t = threshold ? threshold : skw_host_otsu(p);
    int64_t ink = 0;
    memset(counts, 0, (size_t)p.h * p.nb);
    for (int y = 0; y < p.h; ++y)
        for (int x = 0; x < p.w; ++x)
            if (skw_host_gray(p, y, x) < t) {
                ++counts[(size_t)(x / band) * p.h + y];
                ++ink;
            }
    const int n_steps = K / 2;
    int best = n_steps;
    uint64_t best_s = 0;
    for (int k = 0; k < K; ++k) {
        for (int r = 0; r < p.h; ++r) profile[r] = 0;
        for (int b = 0; b < p.nb; ++b) {
            const int32_t s = skw_shift(b, band, p.w, shear_q16[k]);
            const uint8_t* col = counts + (size_t)b * p.h;
            const int r0 = s < 0 ? -s : 0, r1 = s > 0 ? p.h - s : p.h;      // r + s in [0, h)
            for (int r = r0; r < r1; ++r) profile[r] = (uint16_t)(profile[r] + col[r + s]);
        }
        uint64_t S = 0;
        for (int r = 0; r + 1 < p.h; ++r) {
            const int64_t d = (int64_t)profile[r + 1] - (int64_t)profile[r];
            S += (uint64_t)(d * d);
        }
        scores[k] = S;
        if (k == 0 || skw_pick_better(S, k, best_s, best, n_steps)) {
            best_s = S;
            best = k;
        }
    }
    *t_out = t;
    *ink_out = ink;
    *best_out = best;
}

// the body of rtn_skew_estimate_host
inline const char* skw_host(int n, const uint8_t* const* pages, const int32_t* heights, const int32_t* widths, const int32_t* channels,
                            int threshold, int band, int K, const int32_t* shear_q16, int32_t* thresholds, int64_t* ink, int32_t* best,
                            uint64_t* scores) {
    std::vector<SkwPage> table((size_t)(n > 0 && n <= SKW_MAX_PAGES ? n : 0));
    int64_t counts_bytes = 0, tiles = 0;
    int max_h = 0, max_nb = 0;
    if (const char* why = skw_plan(n, pages, heights, widths, channels, threshold, band, K, shear_q16, table.data(), &counts_bytes, &tiles, &max_h, &max_nb))
        return why;
    if (n && (!thresholds || !ink || !best || !scores)) return "the four result arrays expected";
    std::vector<uint8_t> counts((size_t)max_h * (size_t)max_nb);
    std::vector<uint16_t> profile((size_t)max_h);
    for (int i = 0; i < n; ++i)
        skw_host_page(table[(size_t)i], threshold, band, K, shear_q16, thresholds + i, ink + i, best + i, scores + (size_t)i * K, counts.data(), profile.data());
    return nullptr;
}
