// rtn_cca.h — the text that scan analysis (csrc/rtn_cca.hip; connectedComponentAnalysis.py) and its CPU twins share:
// the per-element rules as __host__ __device__ functions and the twins themselves, which a plain C++17 compiler compiles (no HIP;
// tools/cca_fuzz.cpp builds them under the sanitizers).  Everything is integer arithmetic: kernels, twins and the NumPy / scipy
// oracle (tests/cca_ref.py) give the same bytes.
//
// The rules restate OpenCV's published behaviour (BGR2GRAY, adaptiveThreshold's mean, the morphology border, GaussianBlur's 8-bit
// fixed point, findContours(RETR_EXTERNAL) + boundingRect) from memory: recalled, not verifiable offline.
#pragma once
#include <stdint.h>
#include <string.h>
#include <vector>
#include "rtn.h"
#if !defined(__HIPCC__) && !defined(__host__)      // a plain C++ compiler (host-only sanitizer builds)
#define __host__
#define __device__
#endif

constexpr int CCA_MIN_SIDE = RTN_CCA_MIN_SIDE;     // below 30 the reference's structuring element has length 0
constexpr int CCA_MAX_SIDE = RTN_CCA_MAX_SIDE;     // a row's prefix counts fit 16 bits, a raster index 28
constexpr int CCA_MAX_IMAGES = 65535;              // one grid row per image
constexpr int CCA_ROW_THREADS = 256;               // row kernels: one workgroup per row, <= 64 pixels of the row per thread
constexpr int CCA_TILE_W = 32, CCA_TILE_H = 16;    // labelling tile: one thread per pixel
constexpr int CCA_PIX_THREADS = 256;               // per-pixel kernels
constexpr int CCA_RANK_PIXELS = 4;                 // rank kernels: consecutive pixels per thread (1024 per workgroup)
constexpr int CCA_BW_TW = 64, CCA_BW_TH = 32;      // box-mean threshold tile

struct CPage {                                     // 32 bytes: one page of a mask entry
    const uint8_t* src;                            // (h, w, ch) B,G,R or gray
    int64_t off;                                   // first byte of the page in every packed mask buffer
    int32_t h, w, ch, pad_;
};
struct CRows {                                     // 32 bytes: one image of the row-opening launch
    const uint8_t* src;
    uint8_t* dst;
    int32_t rows, cols, L, pad_;
};
struct CLab {                                      // 48 bytes: one image of the labelling launches
    const uint8_t* img;                            // (h, w), non-zero is foreground
    int64_t pix_off;                               // first pixel in the per-pixel workspace arrays
    int64_t box_off;                               // first box (4 int32) in the boxes buffer
    int64_t blk_off;                               // first entry in the per-workgroup root counts
    int32_t h, w, cap, pad_;
};
struct CPaintPage { uint8_t* dst; int32_t h, w, ch, pad_; };             // 24 bytes
struct CRect { int32_t page, x0, y0, x1, y1, pad_; };                    // 24 bytes: [y0, y1) x [x0, x1), inside the page
static_assert(sizeof(CPage) == 32 && sizeof(CRows) == 32 && sizeof(CLab) == 48 && sizeof(CPaintPage) == 24 && sizeof(CRect) == 24, "cca table layout");

// ---- per-element rules ----------------------------------------------------------------------------------------------------------
// cv2 BGR2GRAY, 8 bit (the rule of csrc/rtn_preprocess.hip); a gray page is taken as it is
__host__ __device__ inline int cca_gray(const uint8_t* p, int ch) {
    return ch == 3 ? ((1868 * p[0] + 9617 * p[1] + 4899 * p[2] + 8192) >> 14) : p[0];
}
__host__ __device__ inline int cca_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// bitwise_not(gray) at (y, x) with replicated borders
__host__ __device__ inline int cca_ginv(const CPage& p, int y, int x) {
    y = cca_clamp(y, 0, p.h - 1);
    x = cca_clamp(x, 0, p.w - 1);
    return 255 - cca_gray(p.src + ((size_t)y * p.w + x) * p.ch, p.ch);
}
// adaptiveThreshold(MEAN_C, BINARY, 15, -2): S the 15x15 box sum; the mean rounds to nearest (225 is odd: no exact half)
__host__ __device__ inline uint8_t cca_bw(int g, int S) {
    const int mean = (2 * S + 225) / 450;
    return g - mean > 2 ? 255 : 0;
}
// BORDER_REFLECT_101 for a tap one pixel outside
__host__ __device__ inline int cca_reflect(int v, int n) { return v < 0 ? -v : (v >= n ? 2 * n - 2 - v : v); }
// GaussianBlur((5,5), 0.5) in 8-bit fixed point: taps (0, 27, 202, 27, 0) / 256, the row pass keeps 16 bits
__host__ __device__ inline int cca_blur_row(const CPage& p, int y, int x) {
    const uint8_t* row = p.src + (size_t)y * p.w * p.ch;
    return 27 * cca_gray(row + (size_t)cca_reflect(x - 1, p.w) * p.ch, p.ch) + 202 * cca_gray(row + (size_t)x * p.ch, p.ch) +
           27 * cca_gray(row + (size_t)cca_reflect(x + 1, p.w) * p.ch, p.ch);
}
__host__ __device__ inline uint8_t cca_blur(const CPage& p, int y, int x) {
    const int s = 27 * cca_blur_row(p, cca_reflect(y - 1, p.h), x) + 202 * cca_blur_row(p, y, x) + 27 * cca_blur_row(p, cca_reflect(y + 1, p.h), x);
    return (uint8_t)((s + 32768) >> 16);
}
// the window of position x on a line of n: [x - anchor, x - anchor + L - 1] cut to the line (never empty: anchor < L)
__host__ __device__ inline void cca_window(int x, int L, int anchor, int n, int* lo, int* hi) {
    const int a = x - anchor, b = a + L - 1;
    *lo = a < 0 ? 0 : a;
    *hi = b > n - 1 ? n - 1 : b;
}
// erode (is_min) / dilate of a binary line from the number of ones in the window
__host__ __device__ inline bool cca_win_bit(int ones, int lo, int hi, bool is_min) { return is_min ? ones == hi - lo + 1 : ones > 0; }
constexpr int CCA_STEPS = 5;                       // the binary steps of process_image after the threshold
__host__ __device__ inline void cca_text_step(int s, int* L, int* anchor, bool* is_min) {
    *L = s == 0 ? 28 : 10;                         // 9 iterations of the all-ones 1x4 element = one 1x28 element anchored at 18
    *anchor = s == 0 ? 18 : 5;
    *is_min = s == 2 || s == 4;                    // dilate 28, then close 10 twice
}
// the rectangles a box paints: mode 0 the box itself (white), mode 1 the outline of thickness 2 from (x, y) to (x + w, y + h)
// (draw_box of model/utils.py: bands centred on the edges); clipped to the page, empty ones dropped.  Returns their number.
__host__ __device__ inline int cca_box_rects(int mode, const int32_t* box, int page, int H, int W, CRect* out) {
    const int x = box[0], y = box[1], x2 = box[0] + box[2], y2 = box[1] + box[3];
    int r[4][4], n = 1;
    if (mode == 0) {
        r[0][0] = x; r[0][1] = y; r[0][2] = x2; r[0][3] = y2;
    } else {
        const int lo = 1, hi = 1;
        n = 4;
        r[0][0] = x - lo; r[0][1] = y - lo; r[0][2] = x2 + hi; r[0][3] = y + hi;
        r[1][0] = x - lo; r[1][1] = y2 - lo; r[1][2] = x2 + hi; r[1][3] = y2 + hi;
        r[2][0] = x - lo; r[2][1] = y - lo; r[2][2] = x + hi; r[2][3] = y2 + hi;
        r[3][0] = x2 - lo; r[3][1] = y - lo; r[3][2] = x2 + hi; r[3][3] = y2 + hi;
    }
    int m = 0;
    for (int i = 0; i < n; ++i) {
        const int x0 = r[i][0] < 0 ? 0 : r[i][0], y0 = r[i][1] < 0 ? 0 : r[i][1];
        const int x1 = r[i][2] > W ? W : r[i][2], y1 = r[i][3] > H ? H : r[i][3];
        if (x0 < x1 && y0 < y1) out[m++] = CRect{page, x0, y0, x1, y1, 0};
    }
    return m;
}
// the value a painted pixel's channel takes: white boxes, green (0, 255, 0) outlines, 255 on a gray page
__host__ __device__ inline uint8_t cca_paint_value(int mode, int ch, int c) { return mode == 0 || ch == 1 || c == 1 ? 255 : 0; }
__host__ __device__ inline void cca_paint_pixel(const CPaintPage& p, int mode, int y, int x) {
    uint8_t* d = p.dst + ((size_t)y * p.w + x) * p.ch;
    for (int c = 0; c < p.ch; ++c) d[c] = cca_paint_value(mode, p.ch, c);
}

// ---- argument checks shared by the device entries and the twins -------------------------------------------------------------------
inline const char* cca_check_sizes(int n, const int32_t* heights, const int32_t* widths) {
    if (n < 0 || n > CCA_MAX_IMAGES) return "0 .. 65535 images expected";
    if (n && (!heights || !widths)) return "the heights and widths expected";
    for (int i = 0; i < n; ++i)
        if (heights[i] < CCA_MIN_SIDE || widths[i] < CCA_MIN_SIDE || heights[i] > CCA_MAX_SIDE || widths[i] > CCA_MAX_SIDE)
            return "an image has a side outside 30 .. 16384";
    return nullptr;
}
inline const char* cca_plan_pages(int n, const uint8_t* const* pages, const int32_t* heights, const int32_t* widths, const int32_t* channels,
                                  const int64_t* offsets, size_t mask_bytes, std::vector<CPage>* out) {
    if (const char* why = cca_check_sizes(n, heights, widths)) return why;
    if (n && (!pages || !channels || !offsets)) return "the pages with their channels and offsets expected";
    int64_t pos = 0;
    out->resize((size_t)n);
    for (int i = 0; i < n; ++i) {
        if (!pages[i] || (channels[i] != 1 && channels[i] != 3)) return "a page is missing or has neither 1 nor 3 channels";
        if (offsets[i] < pos) return "mask offsets must increase without overlap";
        pos = offsets[i] + (int64_t)heights[i] * widths[i];
        if ((uint64_t)pos > mask_bytes) return "a page's mask ends past the mask buffer";
        (*out)[i] = CPage{pages[i], offsets[i], heights[i], widths[i], channels[i], 0};
    }
    return nullptr;
}
inline const char* cca_plan_label(int n, const uint8_t* const* images, const int32_t* heights, const int32_t* widths, const int32_t* capacity,
                                  const int64_t* box_offsets, const void* counts, const void* boxes, size_t boxes_bytes,
                                  std::vector<CLab>* out) {
    if (const char* why = cca_check_sizes(n, heights, widths)) return why;
    if (n && (!images || !capacity || !box_offsets || !counts)) return "the images, capacities, box offsets and counts expected";
    int64_t pos = 0, pix = 0, blk = 0;
    out->resize((size_t)n);
    for (int i = 0; i < n; ++i) {
        if (!images[i] || capacity[i] < 0) return "an image is missing or has a negative capacity";
        if (box_offsets[i] < pos) return "box offsets must increase without overlap";
        pos = box_offsets[i] + capacity[i];
        if ((uint64_t)pos * 16 > boxes_bytes || (pos && !boxes)) return "an image's boxes end past the boxes buffer";
        (*out)[i] = CLab{images[i], pix, box_offsets[i], blk, heights[i], widths[i], capacity[i], 0};
        const int64_t px = (int64_t)heights[i] * widths[i];
        pix += px;
        blk += (px + CCA_PIX_THREADS * CCA_RANK_PIXELS - 1) / (CCA_PIX_THREADS * CCA_RANK_PIXELS);
    }
    return nullptr;
}
inline const char* cca_plan_paint(int n, uint8_t* const* pages, const int32_t* heights, const int32_t* widths, const int32_t* channels,
                                  int n_boxes, const int32_t* box_page, const int32_t* boxes, int mode, std::vector<CPaintPage>* pp,
                                  std::vector<CRect>* rects) {
    if (const char* why = cca_check_sizes(n, heights, widths)) return why;
    if (mode != 0 && mode != 1) return "mode 0 (white boxes) or 1 (outlines) expected";
    if (n_boxes < 0 || (n_boxes && (!box_page || !boxes)) || (n && (!pages || !channels))) return "the pages and n_boxes boxes with their pages expected";
    pp->resize((size_t)n);
    for (int i = 0; i < n; ++i) {
        if (!pages[i] || (channels[i] != 1 && channels[i] != 3)) return "a page is missing or has neither 1 nor 3 channels";
        (*pp)[i] = CPaintPage{pages[i], heights[i], widths[i], channels[i], 0};
    }
    rects->clear();
    rects->reserve((size_t)n_boxes * (mode ? 4 : 1));
    for (int j = 0; j < n_boxes; ++j) {
        const int32_t* b = boxes + 4 * (size_t)j;
        if (box_page[j] < 0 || box_page[j] >= n) return "a box names a page outside the batch";
        if (b[0] < 0 || b[1] < 0 || b[2] < 0 || b[3] < 0 || b[0] > CCA_MAX_SIDE || b[1] > CCA_MAX_SIDE || b[2] > CCA_MAX_SIDE || b[3] > CCA_MAX_SIDE)
            return "a box has a coordinate outside 0 .. 16384";
        CRect r[4];
        const int m = cca_box_rects(mode, b, box_page[j], heights[box_page[j]], widths[box_page[j]], r);
        rects->insert(rects->end(), r, r + m);
    }
    return nullptr;
}

// ---- the CPU twins' bodies ---------------------------------------------------------------------------------------------------------
// one binary window step along a line of n with stride `st`: prefix counts, no loop over the window
inline void cca_line_step(const uint8_t* in, uint8_t* out, int n, ptrdiff_t st, int L, int anchor, bool is_min, std::vector<int32_t>* P) {
    P->resize((size_t)n + 1);
    (*P)[0] = 0;
    for (int x = 0; x < n; ++x) (*P)[x + 1] = (*P)[x] + (in[x * st] != 0);
    for (int x = 0; x < n; ++x) {
        int lo, hi;
        cca_window(x, L, anchor, n, &lo, &hi);
        out[x * st] = cca_win_bit((*P)[hi + 1] - (*P)[lo], lo, hi, is_min) ? 255 : 0;
    }
}

// process_graphical_lines up to the two opened masks; bw (optional) receives the thresholded image
inline void cca_lines_mask_page(const CPage& p, uint8_t* horizontal, uint8_t* vertical, uint8_t* bw_out) {
    const int h = p.h, w = p.w;
    std::vector<uint8_t> g((size_t)h * w), bw((size_t)h * w), tmp((size_t)h * w);
    std::vector<int32_t> rs((size_t)h * w), P;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) g[(size_t)y * w + x] = (uint8_t)cca_ginv(p, y, x);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            int s = 0;
            for (int d = -7; d <= 7; ++d) s += g[(size_t)y * w + cca_clamp(x + d, 0, w - 1)];
            rs[(size_t)y * w + x] = s;
        }
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            int S = 0;
            for (int d = -7; d <= 7; ++d) S += rs[(size_t)cca_clamp(y + d, 0, h - 1) * w + x];
            bw[(size_t)y * w + x] = cca_bw(g[(size_t)y * w + x], S);
        }
    if (bw_out) memcpy(bw_out, bw.data(), bw.size());
    const int Lh = w / 30, Lv = h / 30;
    for (int y = 0; y < h; ++y) {
        cca_line_step(&bw[(size_t)y * w], &tmp[(size_t)y * w], w, 1, Lh, Lh / 2, true, &P);
        cca_line_step(&tmp[(size_t)y * w], horizontal + (size_t)y * w, w, 1, Lh, Lh / 2, false, &P);
    }
    for (int x = 0; x < w; ++x) {
        cca_line_step(&bw[x], &tmp[x], h, w, Lv, Lv / 2, true, &P);
        cca_line_step(&tmp[x], vertical + x, h, w, Lv, Lv / 2, false, &P);
    }
}

// process_image up to the closed mask; stages (optional) receives four planes of h * w: blurred, blackhat, thresholded, dilated
inline void cca_text_mask_page(const CPage& p, uint8_t* closed, uint8_t* stages) {
    const int h = p.h, w = p.w;
    const size_t px = (size_t)h * w;
    std::vector<uint8_t> blur(w), dil(w), a(w), b(w);
    std::vector<int32_t> P;
    for (int y = 0; y < h; ++y) {
        for (int x = 0; x < w; ++x) blur[x] = cca_blur(p, y, x);
        for (int x = 0; x < w; ++x) {
            int lo, hi, m = 0;
            cca_window(x, 4, 2, w, &lo, &hi);
            for (int i = lo; i <= hi; ++i) m = blur[i] > m ? blur[i] : m;
            dil[x] = (uint8_t)m;
        }
        for (int x = 0; x < w; ++x) {
            int lo, hi, m = 255;
            cca_window(x, 4, 2, w, &lo, &hi);
            for (int i = lo; i <= hi; ++i) m = dil[i] < m ? dil[i] : m;
            const int bh = m - blur[x] > 0 ? m - blur[x] : 0;
            a[x] = bh > 10 ? 255 : 0;
            if (stages) {
                stages[(size_t)y * w + x] = blur[x];
                stages[px + (size_t)y * w + x] = (uint8_t)bh;
                stages[2 * px + (size_t)y * w + x] = a[x];
            }
        }
        for (int s = 0; s < CCA_STEPS; ++s) {
            int L, anchor;
            bool is_min;
            cca_text_step(s, &L, &anchor, &is_min);
            cca_line_step(a.data(), b.data(), w, 1, L, anchor, is_min, &P);
            a.swap(b);
            if (s == 0 && stages) memcpy(stages + 3 * px + (size_t)y * w, a.data(), (size_t)w);
        }
        memcpy(closed + (size_t)y * w, a.data(), (size_t)w);
    }
}

// labelling by flood fill in raster order: the components come out in the order of their first pixels.  Writes the true count and
// the first `cap` boxes (x, y, w, h); returns the count.
inline int64_t cca_label_image(const uint8_t* img, int h, int w, int external_only, int cap, int32_t* boxes) {
    const size_t px = (size_t)h * w;
    std::vector<uint8_t> outer(px, 0), seen(px, 0);
    std::vector<int32_t> stack;
    auto push_outer = [&](int y, int x) {
        const size_t i = (size_t)y * w + x;
        if (!img[i] && !outer[i]) { outer[i] = 1; stack.push_back((int32_t)i); }
    };
    if (external_only) {                                           // the background region that contains the frame, 4-connected
        for (int x = 0; x < w; ++x) { push_outer(0, x); push_outer(h - 1, x); }
        for (int y = 0; y < h; ++y) { push_outer(y, 0); push_outer(y, w - 1); }
        while (!stack.empty()) {
            const int32_t i = stack.back();
            stack.pop_back();
            const int y = i / w, x = i % w;
            if (x > 0) push_outer(y, x - 1);
            if (x < w - 1) push_outer(y, x + 1);
            if (y > 0) push_outer(y - 1, x);
            if (y < h - 1) push_outer(y + 1, x);
        }
    }
    int64_t count = 0;
    for (size_t s = 0; s < px; ++s) {
        if (!img[s] || seen[s]) continue;
        int x0 = w, y0 = h, x1 = -1, y1 = -1;
        bool ext = false;
        seen[s] = 1;
        stack.push_back((int32_t)s);
        while (!stack.empty()) {
            const int32_t i = stack.back();
            stack.pop_back();
            const int y = i / w, x = i % w;
            x0 = x < x0 ? x : x0; x1 = x > x1 ? x : x1; y0 = y < y0 ? y : y0; y1 = y > y1 ? y : y1;
            if (external_only)
                ext = ext || x == 0 || y == 0 || x == w - 1 || y == h - 1 || outer[i - 1] || outer[i + 1] || outer[i - w] || outer[i + w];
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const int ny = y + dy, nx = x + dx;
                    if (ny < 0 || nx < 0 || ny >= h || nx >= w) continue;
                    const size_t j = (size_t)ny * w + nx;
                    if (img[j] && !seen[j]) { seen[j] = 1; stack.push_back((int32_t)j); }
                }
        }
        if (external_only && !ext) continue;
        if (count < cap) {
            int32_t* b = boxes + 4 * count;
            b[0] = x0; b[1] = y0; b[2] = x1 - x0 + 1; b[3] = y1 - y0 + 1;
        }
        ++count;
    }
    return count;
}
