// rtn_lattice.h — the text that table structure (csrc/rtn_lattice.hip; model/structure.py) and its CPU twins share:
// the tables, the per-element rules as __host__ __device__ functions, the argument checks and the twins' bodies, which a plain
// C++17 compiler compiles (no HIP; tools/lattice_fuzz.cpp builds them under the sanitizers).  Everything is integer arithmetic:
// kernels, twins and the NumPy oracle (tests/lattice_ref.py) give the same bytes.
//
// A crop is a box of a page grown by the margin and cut to the page: (x0, y0, w, h), w and h at least 30.  Its masks (bw, hm, vm,
// ink: uint8, 0 or 255, (h, w)) lie at the crop's offset in every packed mask buffer.  Separator runs are pairs (lo, hi), inclusive,
// in crop coordinates; a box's R row runs come first, its C column runs after them.  A run may be empty (hi = lo - 1) only as the
// first or the last of its axis (the stream flavour's leading and trailing runs).
#pragma once
#include <stdint.h>
#include <string.h>
#include <vector>
#include "rtn.h"
#include "rtn_cca.h"

constexpr int LAT_THREADS = 256;                   // every kernel: four waves
constexpr int LAT_MAX_BOXES = 32767;               // the opening launch has two grid rows per box
constexpr int LAT_ROWS_PER_GROUP = 4;              // profile launch: a wave per row
constexpr int LAT_COLS_PER_GROUP = 64;             // profile launch: a lane per column, the four waves share the rows
constexpr int LAT_EDGES_PER_GROUP = 4;             // edge launch: a wave per edge

struct LCrop {                                     // 56 bytes: one box of a launch
    const uint8_t* src;                            // its page
    int64_t off;                                   // first byte of the crop in every packed mask buffer
    int64_t toff;                                  // the same in the workspace's transposed planes (device entries)
    int32_t ph, pw, ch;                            // the page
    int32_t x0, y0, w, h;                          // the crop inside it
    int32_t pad_;
};
struct LProf {                                     // 32 bytes: one box of the profile launch
    int64_t off, prof_off;                         // prof_off: the box's first int32 in the profiles: rowH[h], rowInk[h], colV[w], colInk[w]
    int32_t w, h, row_groups, pad_;
};
struct LEdge {                                     // 48 bytes: pixel (s, b) of span and band is mask[off + (span_lo + s) * ss + (band_lo + b) * sb]
    int64_t off;
    int64_t out;                                   // the edge's byte in the edges buffer
    int32_t ss, sb, span_lo, span_n, band_lo, band_n;
    int32_t vertical, pad_;                        // vertical edges read vm, horizontal ones hm
};
struct LCell {                                     // 48 bytes: the cell [y0, y1) x [x0, x1) of a crop, possibly empty
    int64_t off;
    int64_t out;                                   // the cell's index in cell_ink; 4 * out in cell_box
    int32_t w, x0, y0, x1, y1;
    int32_t px, py, pad_;                          // the crop's origin in the page
};
static_assert(sizeof(LCrop) == 56 && sizeof(LProf) == 32 && sizeof(LEdge) == 48 && sizeof(LCell) == 48, "lattice table layout");

// ---- per-element rules ----------------------------------------------------------------------------------------------------------
// the thresholded image at page pixel (y, x): rtn_cca_lines_mask's, from the whole page (S: the 15x15 box sum of 255 - gray with
// replicated page borders), so that a crop's border never acts as an image border
__host__ __device__ inline CPage lat_page(const LCrop& c) { return CPage{c.src, 0, c.ph, c.pw, c.ch, 0}; }
// the window length of an opening along a side of n pixels
__host__ __device__ inline int lat_window(int n, int line_scale) { return n / line_scale; }
__host__ __device__ inline uint8_t lat_ink(uint8_t bw, uint8_t hm, uint8_t vm) { return (uint8_t)(bw & ~hm & ~vm); }
// is an edge present: `covered` of the `len` positions of its span hold a line pixel within the band; an empty span is present
__host__ __device__ inline uint8_t lat_edge_present(int covered, int len, int cover) { return 100 * covered >= cover * len ? 1 : 0; }
// a band around a run, cut to a side of n
__host__ __device__ inline void lat_band(int lo, int hi, int tol, int n, int* b0, int* bn) {
    const int a = lo - tol < 0 ? 0 : lo - tol, b = hi + tol > n - 1 ? n - 1 : hi + tol;
    *b0 = a;
    *bn = b - a + 1;
}
// a cell's count and box to its outputs: page coordinates, 0,0,0,0 without ink
__host__ __device__ inline void lat_cell_store(const LCell& c, int cnt, int xa, int ya, int xb, int yb, int32_t* cell_ink, int32_t* cell_box) {
    cell_ink[c.out] = cnt;
    int32_t* b = cell_box + 4 * c.out;
    b[0] = cnt ? c.px + xa : 0;
    b[1] = cnt ? c.py + ya : 0;
    b[2] = cnt ? xb - xa + 1 : 0;
    b[3] = cnt ? yb - ya + 1 : 0;
}

// ---- separators: profiles to runs (host; the device path and the twins both call it) --------------------------------
// mode 0 (lattice): the maximal runs of profile > 0, two runs with at most `param` zeros between them being one.
// mode 1 (stream): the leading zero run (possibly empty), every inner zero run of at least `param`, the trailing zero run (possibly
// empty); no run at all where the profile is zero everywhere.  Writes the first `cap` runs (lo, hi); returns the true count.
inline int64_t lat_runs(const int32_t* prof, int n, int mode, int param, int64_t cap, int32_t* runs) {
    int64_t count = 0;
    auto emit = [&](int lo, int hi) {
        if (count < cap) { runs[2 * count] = lo; runs[2 * count + 1] = hi; }
        ++count;
    };
    if (mode == 0) {
        int lo = -1, hi = -1;                                                  // the run being grown
        for (int i = 0; i < n; ++i) {
            if (prof[i] <= 0) continue;
            if (lo >= 0 && i - hi - 1 > param) { emit(lo, hi); lo = -1; }
            if (lo < 0) lo = i;
            hi = i;
        }
        if (lo >= 0) emit(lo, hi);
        return count;
    }
    int first = 0, last = n - 1;
    while (first < n && prof[first] <= 0) ++first;
    if (first == n) return 0;
    while (prof[last] <= 0) --last;
    emit(0, first - 1);
    for (int i = first; i <= last;) {
        if (prof[i] > 0) { ++i; continue; }
        int j = i;
        while (prof[j] <= 0) ++j;                                               // ends at or before `last`
        if (j - i >= param) emit(i, j - 1);
        i = j;
    }
    emit(last + 1, n - 1);
    return count;
}

// ---- argument checks shared by the device entries and the twins -------------------------------------------------------------------
inline const char* lat_plan_crops(int n_boxes, const int32_t* crops, const int64_t* offsets, size_t mask_bytes, std::vector<LCrop>* out) {
    if (n_boxes < 0 || n_boxes > LAT_MAX_BOXES) return "0 .. 32767 boxes expected";
    if (n_boxes && (!crops || !offsets)) return "the crops and their offsets expected";
    int64_t pos = 0;
    out->resize((size_t)n_boxes);
    for (int j = 0; j < n_boxes; ++j) {
        const int32_t* c = crops + 4 * (size_t)j;
        if (c[0] < 0 || c[1] < 0 || c[2] < CCA_MIN_SIDE || c[3] < CCA_MIN_SIDE || c[2] > CCA_MAX_SIDE || c[3] > CCA_MAX_SIDE ||
            c[0] > CCA_MAX_SIDE || c[1] > CCA_MAX_SIDE)
            return "a crop has a side outside 30 .. 16384 or a negative origin";
        if (offsets[j] < pos) return "mask offsets must increase without overlap";
        pos = offsets[j] + (int64_t)c[2] * c[3];
        if ((uint64_t)pos > mask_bytes) return "a crop's mask ends past the mask buffer";
        (*out)[j] = LCrop{nullptr, offsets[j], 0, 0, 0, 0, c[0], c[1], c[2], c[3], 0};
    }
    return nullptr;
}
inline const char* lat_plan_pages(int n, const uint8_t* const* pages, const int32_t* heights, const int32_t* widths, const int32_t* channels,
                                  int n_boxes, const int32_t* box_page, int line_scale, std::vector<LCrop>* crops) {
    if (const char* why = cca_check_sizes(n, heights, widths)) return why;
    if (line_scale < 1 || line_scale > CCA_MIN_SIDE) return "line_scale within 1 .. 30 expected";
    if ((n && (!pages || !channels)) || (n_boxes && !box_page)) return "the pages with their channels and the boxes' pages expected";
    for (int i = 0; i < n; ++i)
        if (!pages[i] || (channels[i] != 1 && channels[i] != 3)) return "a page is missing or has neither 1 nor 3 channels";
    for (int j = 0; j < n_boxes; ++j) {
        LCrop& c = (*crops)[j];
        const int p = box_page[j];
        if (p < 0 || p >= n) return "a box names a page outside the batch";
        if (c.x0 + c.w > widths[p] || c.y0 + c.h > heights[p]) return "a crop reaches outside its page";
        c.src = pages[p]; c.ph = heights[p]; c.pw = widths[p]; c.ch = channels[p];
    }
    return nullptr;
}
// the runs of box j along a side of n: in order, apart, inside; empty only at the ends
inline const char* lat_check_runs(const int32_t* r, int count, int n) {
    int prev = -1;                                                              // the last position taken
    for (int k = 0; k < count; ++k) {
        const int lo = r[2 * k], hi = r[2 * k + 1];
        const bool empty = hi == lo - 1;
        if (empty && k != 0 && k != count - 1) return "an empty separator run that is neither the first nor the last";
        if (lo < 0 || hi >= n || hi < lo - 1 || lo < prev + (k ? 1 : 0)) return "separator runs must lie inside the crop, in order and apart";
        prev = hi > prev ? hi : prev;
    }
    return nullptr;
}
struct LGrid { const int32_t* rows; const int32_t* cols; int R, C; };
inline const char* lat_plan_grids(const std::vector<LCrop>& crops, const int32_t* R, const int32_t* C, const int64_t* sep_offsets,
                                  const int32_t* runs, size_t runs_count, std::vector<LGrid>* out) {
    const size_t n = crops.size();
    if (n && (!R || !C || !sep_offsets)) return "the run counts and offsets expected";
    out->resize(n);
    for (size_t j = 0; j < n; ++j) {
        if (R[j] < 0 || C[j] < 0 || R[j] > crops[j].h + 1 || C[j] > crops[j].w + 1) return "a run count outside 0 .. side + 1";
        if (sep_offsets[j] < 0 || (uint64_t)(sep_offsets[j] + R[j] + C[j]) > runs_count || ((R[j] || C[j]) && !runs))
            return "a box's runs end past the runs";
        const int32_t* r = runs ? runs + 2 * sep_offsets[j] : nullptr;
        (*out)[j] = LGrid{r, r ? r + 2 * R[j] : nullptr, R[j], C[j]};
        if (const char* why = lat_check_runs((*out)[j].rows, R[j], crops[j].h)) return why;
        if (const char* why = lat_check_runs((*out)[j].cols, C[j], crops[j].w)) return why;
    }
    return nullptr;
}
inline int64_t lat_edge_count(int R, int C) { return R >= 1 && C >= 1 ? (int64_t)R * (C - 1) + (int64_t)(R - 1) * C : 0; }
inline int64_t lat_cell_count(int R, int C) { return R >= 1 && C >= 1 ? (int64_t)(R - 1) * (C - 1) : 0; }
// the edges of every box: box j's R (C - 1) horizontal ones from edge_offsets[j], row by row, then its (R - 1) C vertical ones.
// *need receives the bytes the edges buffer must hold.
inline const char* lat_plan_edges(const std::vector<LCrop>& crops, const std::vector<LGrid>& grids, const int64_t* edge_offsets, int line_tol,
                                  int cover, int64_t* need, std::vector<LEdge>* out) {
    if (line_tol < 0 || line_tol > CCA_MAX_SIDE || cover < 0 || cover > 100) return "line_tol within 0 .. 16384 and cover within 0 .. 100 expected";
    if (!crops.empty() && !edge_offsets) return "the edge offsets expected";
    out->clear();
    int64_t pos = 0;
    for (size_t j = 0; j < crops.size(); ++j) {
        const LCrop& c = crops[j];
        const LGrid& g = grids[j];
        if (edge_offsets[j] < pos) return "edge offsets must increase without overlap";
        int64_t o = edge_offsets[j];
        pos = o + lat_edge_count(g.R, g.C);
        for (int r = 0; r < g.R; ++r)
            for (int k = 0; k + 1 < g.C; ++k) {
                LEdge e{c.off, o++, 1, c.w, g.cols[2 * k + 1] + 1, g.cols[2 * k + 2] - g.cols[2 * k + 1] - 1, 0, 0, 0, 0};
                lat_band(g.rows[2 * r], g.rows[2 * r + 1], line_tol, c.h, &e.band_lo, &e.band_n);
                out->push_back(e);
            }
        for (int r = 0; r + 1 < g.R; ++r)
            for (int k = 0; k < g.C; ++k) {
                LEdge e{c.off, o++, c.w, 1, g.rows[2 * r + 1] + 1, g.rows[2 * r + 2] - g.rows[2 * r + 1] - 1, 0, 0, 1, 0};
                lat_band(g.cols[2 * k], g.cols[2 * k + 1], line_tol, c.w, &e.band_lo, &e.band_n);
                out->push_back(e);
            }
    }
    *need = pos;
    return nullptr;
}
// the cells of every box, row by row from cell_offsets[j]; *need receives the cells the outputs must hold
inline const char* lat_plan_cells(const std::vector<LCrop>& crops, const std::vector<LGrid>& grids, const int64_t* cell_offsets, int64_t* need,
                                  std::vector<LCell>* out) {
    if (!crops.empty() && !cell_offsets) return "the cell offsets expected";
    out->clear();
    int64_t pos = 0;
    for (size_t j = 0; j < crops.size(); ++j) {
        const LCrop& c = crops[j];
        const LGrid& g = grids[j];
        if (cell_offsets[j] < pos) return "cell offsets must increase without overlap";
        int64_t o = cell_offsets[j];
        pos = o + lat_cell_count(g.R, g.C);
        for (int r = 0; r + 1 < g.R; ++r)
            for (int k = 0; k + 1 < g.C; ++k)
                out->push_back(LCell{c.off, o++, c.w, g.cols[2 * k + 1] + 1, g.rows[2 * r + 1] + 1, g.cols[2 * k + 2], g.rows[2 * r + 2], c.x0, c.y0, 0});
    }
    *need = pos;
    return nullptr;
}
inline const char* lat_plan_profiles(const std::vector<LCrop>& crops, const int64_t* prof_offsets, size_t profiles_count, std::vector<LProf>* out) {
    if (!crops.empty() && !prof_offsets) return "the profile offsets expected";
    out->resize(crops.size());
    int64_t pos = 0;
    for (size_t j = 0; j < crops.size(); ++j) {
        const LCrop& c = crops[j];
        if (prof_offsets[j] < pos) return "profile offsets must increase without overlap";
        pos = prof_offsets[j] + 2 * ((int64_t)c.w + c.h);
        if ((uint64_t)pos > profiles_count) return "a box's profiles end past the profiles buffer";
        (*out)[j] = LProf{c.off, prof_offsets[j], c.w, c.h, (c.h + LAT_ROWS_PER_GROUP - 1) / LAT_ROWS_PER_GROUP, 0};
    }
    return nullptr;
}

// ---- the CPU twins' bodies ---------------------------------------------------------------------------------------------------------
// the thresholded image of a whole page, by separable sums
inline void lat_bw_page(const CPage& p, std::vector<uint8_t>* bw) {
    const int h = p.h, w = p.w;
    std::vector<uint8_t> g((size_t)h * w);
    std::vector<int32_t> rs((size_t)h * w);
    bw->resize((size_t)h * w);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) g[(size_t)y * w + x] = (uint8_t)cca_ginv(p, y, x);
    for (int y = 0; y < h; ++y) {
        int s = 0;                                                              // a sliding sum along the row
        for (int d = -7; d <= 7; ++d) s += g[(size_t)y * w + cca_clamp(d, 0, w - 1)];
        for (int x = 0; x < w; ++x) {
            rs[(size_t)y * w + x] = s;
            s += g[(size_t)y * w + cca_clamp(x + 8, 0, w - 1)] - g[(size_t)y * w + cca_clamp(x - 7, 0, w - 1)];
        }
    }
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            int S = 0;
            for (int d = -7; d <= 7; ++d) S += rs[(size_t)cca_clamp(y + d, 0, h - 1) * w + x];
            (*bw)[(size_t)y * w + x] = cca_bw(g[(size_t)y * w + x], S);
        }
}
// the four masks of one crop from its page's thresholded image
inline void lat_masks_crop(const LCrop& c, const uint8_t* page_bw, int line_scale, uint8_t* bw, uint8_t* hm, uint8_t* vm, uint8_t* ink) {
    const int w = c.w, h = c.h;
    std::vector<uint8_t> tmp((size_t)w * h);
    std::vector<int32_t> P;
    for (int y = 0; y < h; ++y) memcpy(bw + (size_t)y * w, page_bw + (size_t)(c.y0 + y) * c.pw + c.x0, (size_t)w);
    const int Lh = lat_window(w, line_scale), Lv = lat_window(h, line_scale);
    for (int y = 0; y < h; ++y) {
        cca_line_step(bw + (size_t)y * w, &tmp[(size_t)y * w], w, 1, Lh, Lh / 2, true, &P);
        cca_line_step(&tmp[(size_t)y * w], hm + (size_t)y * w, w, 1, Lh, Lh / 2, false, &P);
    }
    for (int x = 0; x < w; ++x) {
        cca_line_step(bw + x, &tmp[x], h, w, Lv, Lv / 2, true, &P);
        cca_line_step(&tmp[x], vm + x, h, w, Lv, Lv / 2, false, &P);
    }
    for (size_t i = 0; i < (size_t)w * h; ++i) ink[i] = lat_ink(bw[i], hm[i], vm[i]);
}
inline void lat_profiles_crop(const LProf& p, const uint8_t* hm, const uint8_t* vm, const uint8_t* ink, int32_t* profiles) {
    int32_t* rowH = profiles + p.prof_off;
    int32_t* rowInk = rowH + p.h;
    int32_t* colV = rowInk + p.h;
    int32_t* colInk = colV + p.w;
    memset(rowH, 0, sizeof(int32_t) * 2 * ((size_t)p.w + p.h));
    for (int y = 0; y < p.h; ++y)
        for (int x = 0; x < p.w; ++x) {
            const size_t i = (size_t)p.off + (size_t)y * p.w + x;
            rowH[y] += hm[i] != 0;
            rowInk[y] += ink[i] != 0;
            colV[x] += vm[i] != 0;
            colInk[x] += ink[i] != 0;
        }
}
inline uint8_t lat_edge(const LEdge& e, const uint8_t* hm, const uint8_t* vm, int cover) {
    const uint8_t* m = (e.vertical ? vm : hm) + e.off;
    int covered = 0;
    for (int s = 0; s < e.span_n; ++s) {
        bool any = false;
        for (int b = 0; b < e.band_n && !any; ++b) any = m[(size_t)(e.span_lo + s) * e.ss + (size_t)(e.band_lo + b) * e.sb] != 0;
        covered += any;
    }
    return lat_edge_present(covered, e.span_n, cover);
}
inline void lat_cell(const LCell& c, const uint8_t* ink, int32_t* cell_ink, int32_t* cell_box) {
    int cnt = 0, xa = c.w, ya = 1 << 30, xb = -1, yb = -1;
    for (int y = c.y0; y < c.y1; ++y)
        for (int x = c.x0; x < c.x1; ++x) {
            if (!ink[c.off + (int64_t)y * c.w + x]) continue;
            ++cnt;
            xa = x < xa ? x : xa; xb = x > xb ? x : xb;
            ya = y < ya ? y : ya; yb = y > yb ? y : yb;
        }
    lat_cell_store(c, cnt, xa, ya, xb, yb, cell_ink, cell_box);
}
