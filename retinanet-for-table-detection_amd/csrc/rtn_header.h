// rtn_header.h — the text that header detection (csrc/rtn_header.hip) and its CPU twins share: the per-element rules
// of the four stages as __host__ __device__ functions.  A plain C++17 compiler compiles this header (no HIP).  Every float
// expression below is written one operation per statement in a fixed order and the file is compiled with -ffp-contract=off: the
// kernels, the twins and the NumPy oracle (tests/header_ref.py) give the same bits.
//
// Stages (HeaderDetect.py main()): sample (imutils.resize(width=500) as an exact box filter, then cv2's 8-bit BGR2HSV), cluster
// (k-means for k = 1 .. 9 in a chain, integer accumulators), stats (per cluster and channel histograms of the chosen k) and
// patches (inRange by Q1 / Q3, the 3x3 non-zero mask of GaussianBlur, cv2's 8-bit HSV2BGR).
// The two colour rules restate OpenCV's published color_hsv source (RGB2HSV_b, HSV2RGB_b / HSV2RGB_native) from memory:
// recalled, not verifiable offline (OpenCV is not a dependency and was not available when this was written).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "rtn.h"
#if !defined(__HIPCC__) && !defined(__host__)      // a plain C++ compiler (host-only sanitizer builds)
#define __host__
#define __device__
#endif

constexpr int HDR_W = RTN_HEADER_WIDTH;            // imutils.resize(width=500)
constexpr int HDR_K = RTN_HEADER_MAX_K;
constexpr int HDR_MAX_POINTS = RTN_HEADER_MAX_POINTS;
constexpr int HDR_MAX_SIDE = 65500;                // the image readers' limit
constexpr int HDR_THREADS = 512;                   // cluster and stats kernels: one workgroup per crop (cluster: 222 VGPRs, no scratch; 1024 threads spill)
constexpr int HDR_PIX_THREADS = 256;               // sample and patches kernels: one thread per destination pixel

struct HCrop {                                     // 32 bytes
    const uint8_t* src;                            // (h, w, 3) B,G,R; sample only
    int64_t off;                                   // first point of the crop in the packed H,S,V buffer (a multiple of 4: 500 * dh is)
    int32_t h, w, dh, k;                           // k: the chosen k (stats only)
};
struct HPatch {                                    // 24 bytes
    int64_t out_off;                               // byte offset of the (dh, 500, 3) B,G,R patch
    int32_t crop;
    uint8_t lo[3], hi[3], pad_[6];
};
static_assert(sizeof(HCrop) == 32 && sizeof(HPatch) == 24, "header table layout");

// one pass's sums of a crop: integers, so no sum depends on the order it was added in
struct HAcc {
    uint64_t q[HDR_K][3];                          // sum of squares per cluster and channel
    uint32_t s[HDR_K][3];                          // sum per cluster and channel (<= 2^21 * 255)
    uint32_t n[HDR_K];
};

// ---- stage 1: sample ------------------------------------------------------------------------------------------------------------
// cv2 BGR2HSV, 8 bit, H in [0, 180): sdiv = cvRound((255 << 12) / v), hdiv = cvRound((180 << 12) / (6 * diff)), both 0 at 0
__host__ __device__ inline int hdr_sdiv(int v) { return v ? (int)rint(1044480.0 / (double)v) : 0; }
__host__ __device__ inline int hdr_hdiv(int diff) { return diff ? (int)rint(737280.0 / (6.0 * (double)diff)) : 0; }

__host__ __device__ inline void hdr_value_range(int b, int g, int r, int* v_out, int* diff_out) {
    int v = b > g ? b : g;
    v = v > r ? v : r;
    int vmin = b < g ? b : g;
    vmin = vmin < r ? vmin : r;
    *v_out = v;
    *diff_out = v - vmin;
}

// the integer half of the rule: sdiv = hdr_sdiv(v) and hdiv = hdr_hdiv(diff), computed or read from a table of them
__host__ __device__ inline void hdr_bgr2hsv_div(int b, int g, int r, int v, int diff, int sdiv, int hdiv, uint8_t* out) {
    const int s = (diff * sdiv + 2048) >> 12;
    int h = v == r ? g - b : (v == g ? b - r + 2 * diff : r - g + 4 * diff);
    h = (h * hdiv + 2048) >> 12;                   // arithmetic shift of a negative h, as in OpenCV
    if (h < 0) h += 180;
    out[0] = (uint8_t)(h > 255 ? 255 : h);
    out[1] = (uint8_t)s;
    out[2] = (uint8_t)v;
}

__host__ __device__ inline void hdr_bgr2hsv(int b, int g, int r, uint8_t* out) {
    int v, diff;
    hdr_value_range(b, g, r, &v, &diff);
    hdr_bgr2hsv_div(b, g, r, v, diff, hdr_sdiv(v), hdr_hdiv(diff), out);
}

// destination pixel (Y, X) of the dh x 500 box resample of an (h, w, 3) image: source pixel i covers [500 i, 500 (i + 1)) of the
// x axis scaled by 500 w and destination pixel X covers [w X, w (X + 1)); the same along y with dh and h; weights are overlaps
__host__ __device__ inline void hdr_sample_bgr(const uint8_t* src, int h, int w, int dh, int Y, int X, int* bgr) {
    const int64_t x0 = (int64_t)w * X, x1 = x0 + w, y0 = (int64_t)h * Y, y1 = y0 + h;
    const int i0 = (int)(x0 / HDR_W), i1 = (int)((x1 - 1) / HDR_W), j0 = (int)(y0 / dh), j1 = (int)((y1 - 1) / dh);
    int64_t sum[3] = {0, 0, 0};
    for (int j = j0; j <= j1; ++j) {
        const int64_t ya = (int64_t)dh * j, yb = ya + dh;
        const int64_t wy = (yb < y1 ? yb : y1) - (ya > y0 ? ya : y0);
        const uint8_t* row = src + (size_t)j * w * 3;
        for (int i = i0; i <= i1; ++i) {
            const int64_t xa = (int64_t)HDR_W * i, xb = xa + HDR_W;
            const int64_t wgt = wy * ((xb < x1 ? xb : x1) - (xa > x0 ? xa : x0));
            sum[0] += wgt * row[3 * i];
            sum[1] += wgt * row[3 * i + 1];
            sum[2] += wgt * row[3 * i + 2];
        }
    }
    const int64_t area = (int64_t)w * h;
    for (int c = 0; c < 3; ++c) bgr[c] = (int)((2 * sum[c] + area) / (2 * area));
}

__host__ __device__ inline void hdr_sample_point(const HCrop& c, int64_t i, uint8_t* hsv) {
    int bgr[3];
    hdr_sample_bgr(c.src, c.h, c.w, c.dh, (int)(i / HDR_W), (int)(i % HDR_W), bgr);
    hdr_bgr2hsv(bgr[0], bgr[1], bgr[2], hsv + 3 * (c.off + i));
}

// ---- stage 2: cluster -----------------------------------------------------------------------------------------------------------
// d(p, c) = ((H - c0)^2 + (S - c1)^2) + (V - c2)^2 in float32
__host__ __device__ inline float hdr_dist(float H, float S, float V, const float* c) {
    const float a = H - c[0], b = S - c[1], e = V - c[2];
    const float aa = a * a, bb = b * b, ee = e * e;
    const float ab = aa + bb;
    return ab + ee;
}

// the nearest of the first K centres (cen: [K][3]); ties go to the lowest index
template <int K>
__host__ __device__ inline int hdr_nearest(int H, int S, int V, const float* cen, float* dmin) {
    const float fh = (float)H, fs = (float)S, fv = (float)V;
    int best = 0;
    float bd = hdr_dist(fh, fs, fv, cen);
    for (int c = 1; c < K; ++c) {
        const float d = hdr_dist(fh, fs, fv, cen + 3 * c);
        if (d < bd) { bd = d; best = c; }
    }
    *dmin = bd;
    return best;
}

// one point's share of distortion_fx
__host__ __device__ inline uint64_t hdr_distortion_fx(float d) {
    const float r = sqrtf(d);                      // correctly rounded on both compilers
    const float x = r * 65536.0f;
    return (uint64_t)(int64_t)rintf(x);            // < 2^25: to nearest, ties to even
}

// after an assignment pass: the centres of the non-empty clusters from the pass's sums; an empty cluster keeps its centre
__host__ __device__ inline void hdr_update_centres(const HAcc& a, int k, float* cen) {
    for (int c = 0; c < k; ++c) {
        if (!a.n[c]) continue;
        for (int j = 0; j < 3; ++j) cen[3 * c + j] = (float)((double)a.s[c][j] / (double)a.n[c]);
    }
}

// k -> k + 1: the cluster of the largest SSE is split along its channel of the largest variance (lowest index on ties)
__host__ __device__ inline void hdr_split(const HAcc& a, int k, float* cen) {
    int js = 0;
    double best = -1.0;
    for (int c = 0; c < k; ++c) {
        double sse = 0.0;
        if (a.n[c]) {
            const double q = (double)(a.q[c][0] + a.q[c][1] + a.q[c][2]);
            const double s0 = (double)a.s[c][0], s1 = (double)a.s[c][1], s2 = (double)a.s[c][2];
            const double p0 = s0 * s0, p1 = s1 * s1, p2 = s2 * s2;
            const double p01 = p0 + p1;
            const double p = p01 + p2;
            const double m = p / (double)a.n[c];
            sse = q - m;
        }
        if (c == 0 || sse > best) { best = sse; js = c; }
    }
    int cs = 0;
    double vbest = 0.0;
    for (int j = 0; j < 3; ++j) {
        double var = 0.0;
        if (a.n[js]) {
            const double n = (double)a.n[js];
            const double m2 = (double)a.q[js][j] / n;
            const double m = (double)a.s[js][j] / n;
            const double mm = m * m;
            var = m2 - mm;
        }
        if (j == 0 || var > vbest) { vbest = var; cs = j; }
    }
    const float e = (float)sqrt(vbest > 0.0 ? vbest : 0.0);
    for (int j = 0; j < 3; ++j) cen[3 * k + j] = cen[3 * js + j];
    cen[3 * k + cs] = cen[3 * js + cs] + e;
    cen[3 * js + cs] = cen[3 * js + cs] - e;
}

#define HDR_DISPATCH_K(k, call)                                                                                                     \
    switch (k) {                                                                                                                    \
        case 1: call(1); break; case 2: call(2); break; case 3: call(3); break; case 4: call(4); break; case 5: call(5); break;    \
        case 6: call(6); break; case 7: call(7); break; case 8: call(8); break; default: call(9); break;                            \
    }

// ---- stage 2 on the CPU: the twins' loops -------------------------------------------------------------------------------------------------------
template <int K>
inline void assign_pass_host(const uint8_t* pts, uint8_t* lab, int N, bool first, const float* cen, HAcc* acc, int* changed) {
    for (int i = 0; i < N; ++i) {
        float d;
        const uint32_t H = pts[3 * i], S = pts[3 * i + 1], V = pts[3 * i + 2];
        const int best = hdr_nearest<K>((int)H, (int)S, (int)V, cen, &d);
        if (first || lab[i] != best) { *changed = 1; lab[i] = (uint8_t)best; }
        acc->n[best] += 1;
        acc->s[best][0] += H; acc->s[best][1] += S; acc->s[best][2] += V;
        acc->q[best][0] += H * H; acc->q[best][1] += S * S; acc->q[best][2] += V * V;
    }
}

template <int K>
inline void distortion_pass_host(const uint8_t* pts, int N, const float* cen, uint64_t* dsum) {
    for (int i = 0; i < N; ++i) {
        float d;
        hdr_nearest<K>(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], cen, &d);
        *dsum += hdr_distortion_fx(d);
    }
}

// the pass structure of cluster_kernel for one crop, one statement per barrier interval
inline void cluster_crop_host(const uint8_t* pts, int N, int max_iter, float* centres, uint32_t* counts, int32_t* passes,
                       uint64_t* distortion, uint8_t* labels) {
    HAcc acc;
    float cen[3 * HDR_K];
    memset(&acc, 0, sizeof(acc));
    for (int k = 1; k <= HDR_K; ++k) {
        uint8_t* lab = labels + (size_t)(k - 1) * N;
        if (k == 1) cen[0] = cen[1] = cen[2] = 0.0f;
        else hdr_split(acc, k - 1, cen);
        uint64_t dsum = 0;
        int used = 0;
        for (int pass = 1; pass <= max_iter; ++pass) {
            int changed = 0;
            memset(&acc, 0, sizeof(acc));
#define HDR_ASSIGN(K) assign_pass_host<K>(pts, lab, N, pass == 1, cen, &acc, &changed)
            HDR_DISPATCH_K(k, HDR_ASSIGN)
#undef HDR_ASSIGN
            hdr_update_centres(acc, k, cen);
            used = pass;
            if (!changed) break;
        }
#define HDR_DISTORTION(K) distortion_pass_host<K>(pts, N, cen, &dsum)
        HDR_DISPATCH_K(k, HDR_DISTORTION)
#undef HDR_DISTORTION
        for (int i = 0; i < 3 * HDR_K; ++i) centres[(k - 1) * 3 * HDR_K + i] = i < 3 * k ? cen[i] : 0.0f;
        for (int i = 0; i < HDR_K; ++i) counts[(k - 1) * HDR_K + i] = i < k ? acc.n[i] : 0u;
        passes[k - 1] = used;
        distortion[k - 1] = dsum;
    }
}

// ---- stage 5: patches -----------------------------------------------------------------------------------------------------------
// cv2 HSV2BGR, 8 bit (HSV2RGB_b over HSV2RGB_native, hrange 180), float32, one operation per statement
__host__ __device__ inline uint8_t hdr_sat_u8(float x) {
    const float r = rintf(x);                      // cvRound: to nearest, ties to even
    return (uint8_t)(r < 0.0f ? 0 : (r > 255.0f ? 255 : (int)r));
}

__host__ __device__ inline void hdr_hsv2bgr(int H, int S, int V, uint8_t* out) {
    float h = (float)H;
    const float s = (float)S * (1.0f / 255.0f), v = (float)V * (1.0f / 255.0f);
    float b = v, g = v, r = v;
    if (S != 0) {
        h = h * (6.0f / 180.0f);
        if (h >= 6.0f) h = h - 6.0f;               // fmod(h, 6) for h < 12: exact
        int sector = (int)floorf(h);
        h = h - (float)sector;
        if ((unsigned)sector >= 6u) { sector = 0; h = 0.0f; }
        float tab[4];
        tab[0] = v;
        const float t1 = 1.0f - s;
        tab[1] = v * t1;
        const float sh = s * h;
        const float t2 = 1.0f - sh;
        tab[2] = v * t2;
        const float h1 = 1.0f - h;
        const float sh1 = s * h1;
        const float t3 = 1.0f - sh1;
        tab[3] = v * t3;
        switch (sector) {                          // sector_data, as (b, g, r)
            case 0: b = tab[1]; g = tab[3]; r = tab[0]; break;
            case 1: b = tab[1]; g = tab[0]; r = tab[2]; break;
            case 2: b = tab[3]; g = tab[0]; r = tab[1]; break;
            case 3: b = tab[0]; g = tab[2]; r = tab[1]; break;
            case 4: b = tab[0]; g = tab[1]; r = tab[3]; break;
            default: b = tab[2]; g = tab[1]; r = tab[0]; break;
        }
    }
    out[0] = hdr_sat_u8(b * 255.0f);
    out[1] = hdr_sat_u8(g * 255.0f);
    out[2] = hdr_sat_u8(r * 255.0f);
}

__host__ __device__ inline bool hdr_in_range(const uint8_t* p, const uint8_t* lo, const uint8_t* hi) {
    return p[0] >= lo[0] && p[0] <= hi[0] && p[1] >= lo[1] && p[1] <= hi[1] && p[2] >= lo[2] && p[2] <= hi[2];
}

// pixel (Y, X) of a patch: the point's H,S,V where any pixel of its 3x3 neighbourhood, clipped to the image, is in range (the
// non-zero set of GaussianBlur(3x3, sigma 0, reflect-101) over the inRange mask), else 0,0,0; then HSV2BGR
__host__ __device__ inline void hdr_patch_pixel(const uint8_t* hsv, int dh, int Y, int X, const uint8_t* lo, const uint8_t* hi,
                                                uint8_t* out) {
    bool keep = false;
    const int ya = Y > 0 ? Y - 1 : 0, yb = Y + 1 < dh ? Y + 1 : dh - 1;
    const int xa = X > 0 ? X - 1 : 0, xb = X + 1 < HDR_W ? X + 1 : HDR_W - 1;
    for (int y = ya; y <= yb; ++y)
        for (int x = xa; x <= xb; ++x) keep = keep || hdr_in_range(hsv + 3 * ((size_t)y * HDR_W + x), lo, hi);
    const uint8_t* p = hsv + 3 * ((size_t)Y * HDR_W + X);
    if (keep) hdr_hsv2bgr(p[0], p[1], p[2], out);
    else out[0] = out[1] = out[2] = 0;
}

// ---- argument checks the device entries and the twins share ---------------------------------------------------------------------
// the crops' destination heights and packed offsets: dh >= 1, 500 * dh <= RTN_HEADER_MAX_POINTS, offsets[i + 1] = offsets[i] + 500 * dh
inline const char* hdr_check_layout(int n, const int32_t* dst_heights, const int64_t* offsets, size_t hsv_bytes) {
    if (n < 0 || (n && (!dst_heights || !offsets))) return "n crops with their dst_heights and offsets expected";
    int64_t pos = 0;
    for (int i = 0; i < n; ++i) {
        if (dst_heights[i] < 1 || (int64_t)dst_heights[i] * HDR_W > HDR_MAX_POINTS) return "a destination height is outside 1 .. RTN_HEADER_MAX_POINTS / 500";
        if (offsets[i] != pos) return "offsets must be the running sum of 500 * dst_heights";
        pos += (int64_t)dst_heights[i] * HDR_W;
    }
    if ((uint64_t)pos * 3 > hsv_bytes) return "the H,S,V buffer is smaller than 3 bytes per point";
    return nullptr;
}
