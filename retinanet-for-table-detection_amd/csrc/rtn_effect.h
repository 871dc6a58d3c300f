// rtn_effect.h — the text that the colour effects (csrc/rtn_effect.hip) and their CPU twin share: the per-element
// rules of VisualEffect (model/transform.py:397-512) as __host__ __device__ functions.  A plain C++17 compiler compiles this header
// (no HIP).  Every float expression is float64, written one operation per statement in the order NumPy evaluates the reference's
// array text, and the file is compiled with -ffp-contract=off: the kernels, the twin and the NumPy oracle (tests/effect_ref.py) give
// the same bits.  The two colour rules are rtn_header.h's.
//
// The four steps after the mean are functions of one byte, so each is a 256-entry table: contrast then brightness composed into one
// table per channel, one table for H, one for S, applied around the two colour conversions.
#pragma once
#include "rtn_header.h"

constexpr int EFX_MAX_SIDE = HDR_MAX_SIDE;         // a column sum stays below 2^24: 65500 * 255
constexpr int EFX_MAX_PAGES = 65535;
constexpr int EFX_THREADS = 256;
constexpr int EFX_STRIP = 32;                      // rows of a page one column-sum workgroup adds
constexpr int EFX_CHUNK = 512;                     // column means the tables kernel holds in LDS at a time
constexpr int EFX_GROUP = 16;                      // pixels of one vector access: 48 bytes, three 16-byte words
constexpr int EFX_BLOCK_PIXELS = EFX_THREADS * EFX_GROUP * 4;
constexpr int EFX_TABLE_BYTES = 5 * 256;           // per page: B, G, R (contrast, then brightness), H, S

// EfxPage::mode: which steps run (a parameter that is not 0, or its RTN_EFFECT_FORCE_* flag) and how the pixels are read
constexpr uint32_t EFX_CONTRAST = 1, EFX_BRIGHTNESS = 2, EFX_HUE = 4, EFX_SATURATION = 8;
constexpr uint32_t EFX_RAW_HSV = 16;               // RTN_EFFECT_RAW_HSV: the page holds H,S,V already, no conversion
constexpr uint32_t EFX_VECTOR = 32;                // src and dst are 16-byte aligned: whole groups move as 16-byte words

struct EfxPage {                                   // 72 bytes
    const uint8_t* src;
    uint8_t* dst;
    double p[4];                                   // contrast factor, brightness delta, hue delta, saturation factor
    int64_t sum_off;                               // the page's first column sum, in sums (3 * w of them, index 3 * x + channel)
    int32_t h, w;
    uint32_t mode, pad_;
};
static_assert(sizeof(EfxPage) == 72, "effect table layout");
static_assert(RTN_EFFECT_FORCE_BRIGHTNESS == RTN_EFFECT_FORCE_CONTRAST << 1 && RTN_EFFECT_FORCE_HUE == RTN_EFFECT_FORCE_CONTRAST << 2 &&
              RTN_EFFECT_FORCE_SATURATION == RTN_EFFECT_FORCE_CONTRAST << 3, "the force flags follow the order of the parameters");

// ---- the mean of a channel: image.mean(axis=0).mean(axis=0) --------------------------------------------------------------------------
// a column's mean is its exact integer sum over the height; the columns' means are then added from x = 0 upwards (NumPy reduces the
// outer axis in order, without pairwise summation) and the sum divided by the width
__host__ __device__ inline double efx_column_mean(uint32_t sum, int h) { return (double)sum / (double)h; }

// ---- the steps, each a function of one byte ------------------------------------------------------------------------------------------
__host__ __device__ inline uint8_t efx_clip_u8(double v) {      // np.clip(v, 0, 255).astype(np.uint8): truncation
    const double c = v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v);
    return (uint8_t)c;
}

__host__ __device__ inline uint8_t efx_contrast(int x, double mean, double factor) {     // (x - mean) * factor + mean
    const double d = (double)x - mean;
    const double s = d * factor;
    const double v = s + mean;
    return efx_clip_u8(v);
}

__host__ __device__ inline uint8_t efx_brightness(int x, double delta) {                 // x + delta * 255
    const double o = delta * 255.0;
    const double v = (double)x + o;
    return efx_clip_u8(v);
}

__host__ __device__ inline uint8_t efx_hue(int x, double delta) {                        // np.mod(x + delta * 180, 180)
    const double o = delta * 180.0;
    const double a = (double)x + o;
    double m = fmod(a, 180.0);                     // exact; NumPy then moves a negative remainder into [0, 180]
    if (m != 0.0) {
        if (m < 0.0) m = m + 180.0;                // 180.0 itself for a tiny negative remainder: the byte 180 reaches HSV2BGR
    } else {
        m = 0.0;
    }
    return (uint8_t)m;
}

__host__ __device__ inline uint8_t efx_saturation(int x, double factor) {                // clip(x * factor)
    const double v = (double)x * factor;
    return efx_clip_u8(v);
}

// entry x of a page's tables; the tables of steps that do not run are not written
__host__ __device__ inline void efx_table_entry(const double* p, uint32_t mode, const double* mean, int x, uint8_t* tab) {
    if (mode & (EFX_CONTRAST | EFX_BRIGHTNESS)) {
        for (int c = 0; c < 3; ++c) {
            int v = x;
            if (mode & EFX_CONTRAST) v = efx_contrast(v, mean[c], p[0]);
            if (mode & EFX_BRIGHTNESS) v = efx_brightness(v, p[1]);
            tab[256 * c + x] = (uint8_t)v;
        }
    }
    if (mode & EFX_HUE) tab[768 + x] = efx_hue(x, p[2]);
    if (mode & EFX_SATURATION) tab[1024 + x] = efx_saturation(x, p[3]);
}

// one pixel through the tables; sdiv[v] = hdr_sdiv(v) and hdiv[d] = hdr_hdiv(d) for every byte
__host__ __device__ inline void efx_pixel(uint32_t mode, const uint8_t* tab, const int32_t* sdiv, const int32_t* hdiv, int* b, int* g,
                                          int* r) {
    if (mode & (EFX_CONTRAST | EFX_BRIGHTNESS)) {
        *b = tab[*b];
        *g = tab[256 + *g];
        *r = tab[512 + *r];
    }
    if (!(mode & (EFX_HUE | EFX_SATURATION))) return;
    uint8_t px[3] = {(uint8_t)*b, (uint8_t)*g, (uint8_t)*r};
    if (!(mode & EFX_RAW_HSV)) {
        int v, diff;
        hdr_value_range(*b, *g, *r, &v, &diff);
        hdr_bgr2hsv_div(*b, *g, *r, v, diff, sdiv[v], hdiv[diff], px);
    }
    if (mode & EFX_HUE) px[0] = tab[768 + px[0]];
    if (mode & EFX_SATURATION) px[1] = tab[1024 + px[1]];
    if (!(mode & EFX_RAW_HSV)) hdr_hsv2bgr(px[0], px[1], px[2], px);
    *b = px[0];
    *g = px[1];
    *r = px[2];
}

// ---- argument checks the device entry and the twin share ---------------------------------------------------------------------------------
inline const char* efx_check_sizes(int n, const int32_t* heights, const int32_t* widths) {
    if (n < 0 || n > EFX_MAX_PAGES || (n && (!heights || !widths))) return "0 .. 65535 pages with their heights and widths expected";
    for (int i = 0; i < n; ++i)
        if (heights[i] < 1 || widths[i] < 1 || heights[i] > EFX_MAX_SIDE || widths[i] > EFX_MAX_SIDE) return "a page has a side outside 1 .. 65500";
    return nullptr;
}

// the page table of a batch; `device`: the kernels' alignment rule decides EFX_VECTOR (the twin reads bytes)
inline const char* efx_plan(int n, const uint8_t* const* pages, const int32_t* heights, const int32_t* widths, const double* params,
                            const uint32_t* flags, uint8_t* const* outs, bool device, EfxPage* table) {
    if (const char* why = efx_check_sizes(n, heights, widths)) return why;
    if (n && (!pages || !params || !outs)) return "the pages, their parameters and their outputs expected";
    int64_t pos = 0;
    for (int i = 0; i < n; ++i) {
        EfxPage& e = table[i];
        memset(&e, 0, sizeof(e));
        if (!pages[i] || !outs[i]) return "a page or its output is missing";
        const uint32_t f = flags ? flags[i] : 0u;
        if (f & ~(uint32_t)(RTN_EFFECT_RAW_HSV | RTN_EFFECT_FORCE_CONTRAST | RTN_EFFECT_FORCE_BRIGHTNESS | RTN_EFFECT_FORCE_HUE |
                            RTN_EFFECT_FORCE_SATURATION))
            return "unknown flag bits";
        const uint64_t bytes = 3ull * (uint64_t)heights[i] * (uint64_t)widths[i];
        const uintptr_t s = (uintptr_t)pages[i], d = (uintptr_t)outs[i];
        if (s != d && s < d + bytes && d < s + bytes) return "an output overlaps its page without being the page itself";
        e.src = pages[i];
        e.dst = outs[i];
        e.h = heights[i];
        e.w = widths[i];
        e.sum_off = pos;
        pos += 3 * (int64_t)widths[i];
        for (int k = 0; k < 4; ++k) {
            const double v = params[4 * i + k];
            if (!(v - v == 0.0)) return "a parameter is not finite";
            e.p[k] = v;
            if (v != 0.0 || (f & (RTN_EFFECT_FORCE_CONTRAST << k))) e.mode |= EFX_CONTRAST << k;
        }
        if (f & RTN_EFFECT_RAW_HSV) e.mode |= EFX_RAW_HSV;
        if (device && ((s | d) & 15) == 0) e.mode |= EFX_VECTOR;
    }
    return nullptr;
}
