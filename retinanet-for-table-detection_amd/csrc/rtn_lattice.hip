// rtn_lattice.hip — table structure on the device (model/structure.py): the ruling-line masks of every detected box,
// their projections, the edges between the separators and the ink of every cell.  Integers only; no kernel waits on another
// workgroup, no atomics: every output element is written by one thread, so a second call gives the same bytes.
//
//   crop_bw_kernel     64x32 tiles of every crop through bw_tile (rtn_cca_rows.h), the tile of rtn_cca_lines_mask's threshold: the
//                      page around the tile with the PAGE's replicated borders.  The whole-page threshold taken only where a crop
//                      needs it: the gather and the threshold are one launch.
//   transpose_kernel, open_rows_kernel (rtn_cca_rows.h)   the two openings of crops of mixed sizes in one launch: 64-bit masks per
//                      thread, prefix counts, the column pass as a row pass of the transpose.
//   finish_kernel      32x32 tiles: the opened transpose back into vm, and ink = bw & ~hm & ~vm on the way.
//   profile_kernel     one launch for the four profiles: row groups (a wave per row: ballot and popcount over 64 pixels a step) and
//                      column groups (a lane per column, the four waves share the rows, a tree in LDS) side by side.
//   edge_kernel        a wave per edge: OR over the band, ballot and popcount over the span.
//   cell_kernel        a workgroup per cell: count and bounding box by wave shuffles and a tree over the four waves.
// The per-element rules, the argument checks and the CPU twins' bodies are in rtn_lattice.h.
#include <algorithm>
#include <vector>
#include "rtn_page_launch.h"
#include "rtn_lattice.h"
#include "rtn_cca_rows.h"

namespace {

__global__ __launch_bounds__(LAT_THREADS) void crop_bw_kernel(const LCrop* crops, uint8_t* bw) {
    const LCrop c = crops[blockIdx.y];
    bw_tile(lat_page(c), c.y0, c.x0, c.h, c.w, bw + c.off);                     // clamped to the page, never to the crop
}

// vm (h, w) = transpose of vT (w, h); ink beside it
__global__ __launch_bounds__(LAT_THREADS) void finish_kernel(const LCrop* crops, const uint8_t* vT, const uint8_t* bw, const uint8_t* hm,
                                                             uint8_t* vm, uint8_t* ink) {
    __shared__ uint8_t t[32][33];
    const LCrop c = crops[blockIdx.y];
    const int tiles_x = (c.w + 31) / 32, tiles_y = (c.h + 31) / 32;
    if ((int)blockIdx.x >= tiles_x * tiles_y) return;                          // uniform
    const int x0 = ((int)blockIdx.x % tiles_x) * 32, y0 = ((int)blockIdx.x / tiles_x) * 32;
    const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
    for (int j = ly; j < 32; j += 8)
        if (x0 + j < c.w && y0 + lx < c.h) t[j][lx] = vT[c.toff + (int64_t)(x0 + j) * c.h + y0 + lx];
    __syncthreads();
    for (int j = ly; j < 32; j += 8)
        if (y0 + j < c.h && x0 + lx < c.w) {
            const int64_t i = c.off + (int64_t)(y0 + j) * c.w + x0 + lx;
            const uint8_t v = t[lx][j];
            vm[i] = v;
            ink[i] = lat_ink(bw[i], hm[i], v);
        }
}

__global__ __launch_bounds__(LAT_THREADS) void profile_kernel(const LProf* boxes, const uint8_t* hm, const uint8_t* vm, const uint8_t* ink,
                                                              int32_t* profiles) {
    __shared__ int part[LAT_THREADS / 64][LAT_COLS_PER_GROUP][2];
    const LProf p = boxes[blockIdx.y];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col_groups = (p.w + LAT_COLS_PER_GROUP - 1) / LAT_COLS_PER_GROUP;
    int32_t* rowH = profiles + p.prof_off;
    int32_t* rowInk = rowH + p.h;
    int32_t* colV = rowInk + p.h;
    int32_t* colInk = colV + p.w;
    if ((int)blockIdx.x < p.row_groups) {                                       // uniform: a wave per row
        const int y = (int)blockIdx.x * LAT_ROWS_PER_GROUP + wave;
        if (y >= p.h) return;                                                   // uniform in the wave; no barrier follows
        const int64_t row = p.off + (int64_t)y * p.w;
        int a = 0, b = 0;
        for (int x0 = 0; x0 < p.w; x0 += 64) {
            const int x = x0 + lane;
            a += __popcll(__ballot(x < p.w && hm[row + x] != 0));
            b += __popcll(__ballot(x < p.w && ink[row + x] != 0));
        }
        if (lane == 0) { rowH[y] = a; rowInk[y] = b; }
        return;
    }
    const int cg = (int)blockIdx.x - p.row_groups;
    if (cg >= col_groups) return;                                               // uniform
    const int x = cg * LAT_COLS_PER_GROUP + lane;
    int a = 0, b = 0;
    if (x < p.w)
        for (int y = wave; y < p.h; y += LAT_THREADS / 64) {                    // a wave reads 64 consecutive bytes of a row
            const int64_t i = p.off + (int64_t)y * p.w + x;
            a += vm[i] != 0;
            b += ink[i] != 0;
        }
    part[wave][lane][0] = a;
    part[wave][lane][1] = b;
    __syncthreads();
    if (wave == 0 && x < p.w) {
        colV[x] = part[0][lane][0] + part[1][lane][0] + part[2][lane][0] + part[3][lane][0];
        colInk[x] = part[0][lane][1] + part[1][lane][1] + part[2][lane][1] + part[3][lane][1];
    }
}

__global__ __launch_bounds__(LAT_THREADS) void edge_kernel(const LEdge* edges, int64_t n_edges, const uint8_t* hm, const uint8_t* vm, int cover,
                                                           uint8_t* out) {
    const int lane = threadIdx.x & 63;
    const int64_t k = (int64_t)blockIdx.x * LAT_EDGES_PER_GROUP + (threadIdx.x >> 6);
    if (k >= n_edges) return;                                                   // uniform in the wave
    const LEdge e = edges[k];
    const uint8_t* m = (e.vertical ? vm : hm) + e.off;
    int covered = 0;
    for (int s0 = 0; s0 < e.span_n; s0 += 64) {
        const int s = s0 + lane;
        bool any = false;
        if (s < e.span_n)
            for (int b = 0; b < e.band_n; ++b) any = any || m[(int64_t)(e.span_lo + s) * e.ss + (int64_t)(e.band_lo + b) * e.sb] != 0;
        covered += __popcll(__ballot(any));
    }
    if (lane == 0) out[e.out] = lat_edge_present(covered, e.span_n, cover);
}

__device__ inline int wave_sum(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ inline int wave_min(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = min(v, __shfl_xor(v, d));
    return v;
}
__device__ inline int wave_max(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d));
    return v;
}

__global__ __launch_bounds__(LAT_THREADS) void cell_kernel(const LCell* cells, const uint8_t* ink, int32_t* cell_ink, int32_t* cell_box) {
    __shared__ int part[LAT_THREADS / 64][5];
    const LCell c = cells[blockIdx.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int cnt = 0, xa = c.w, ya = 1 << 30, xb = -1, yb = -1;
    for (int y = c.y0 + wave; y < c.y1; y += LAT_THREADS / 64)
        for (int x = c.x0 + lane; x < c.x1; x += 64) {
            if (!ink[c.off + (int64_t)y * c.w + x]) continue;
            ++cnt;
            xa = min(xa, x); xb = max(xb, x);
            ya = min(ya, y); yb = max(yb, y);
        }
    cnt = wave_sum(cnt);
    xa = wave_min(xa); ya = wave_min(ya);
    xb = wave_max(xb); yb = wave_max(yb);
    if (lane == 0) { part[wave][0] = cnt; part[wave][1] = xa; part[wave][2] = ya; part[wave][3] = xb; part[wave][4] = yb; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int i = 1; i < LAT_THREADS / 64; ++i) {
        cnt += part[i][0];
        xa = min(xa, part[i][1]); ya = min(ya, part[i][2]);
        xb = max(xb, part[i][3]); yb = max(yb, part[i][4]);
    }
    lat_cell_store(c, cnt, xa, ya, xb, yb, cell_ink, cell_box);
}

// ---- workspace: the tables first, then (rtn_lattice_masks only) two planes of the crops' pixels ---------------------------------------
struct Sizes { int64_t pixels = 0; int max_w = 0, max_h = 0; };
Sizes sizes_of(int n_boxes, const int32_t* crops) {
    Sizes s;
    for (int j = 0; j < n_boxes; ++j) {
        s.pixels += (int64_t)crops[4 * j + 2] * crops[4 * j + 3];
        s.max_w = std::max(s.max_w, crops[4 * j + 2]);
        s.max_h = std::max(s.max_h, crops[4 * j + 3]);
    }
    return s;
}
struct MaskLayout { size_t crops, rows, bwT, vT; };
MaskLayout mask_layout(rtn_stage& st, int n_boxes, int64_t pixels) {
    MaskLayout l;
    l.crops = st.reserve((int64_t)n_boxes * sizeof(LCrop));
    l.rows = st.reserve((int64_t)n_boxes * 3 * sizeof(CRows));
    l.bwT = st.reserve(pixels);
    l.vT = st.reserve(pixels);
    return l;
}
// the one table of the profile, edge and cell entries lies in room for n_boxes LProf or n_items LEdge (an LCell is as large) -> its offset
size_t items_room(rtn_stage& st, int n_boxes, int64_t n_items) {
    return st.reserve(std::max<int64_t>((int64_t)n_boxes * sizeof(LProf), n_items * (int64_t)sizeof(LEdge)));
}

}  // namespace

// rtn_lattice_*: see include/rtn.h
extern "C" size_t rtn_lattice_workspace_bytes(int n_boxes, const int32_t* crops, int64_t n_items) {
    if (n_boxes < 0 || n_boxes > LAT_MAX_BOXES || n_items < 0 || (n_boxes && !crops)) return 0;
    rtn_stage masks, items;
    mask_layout(masks, n_boxes, sizes_of(n_boxes, crops).pixels);
    items_room(items, n_boxes, n_items);
    return std::max(masks.bytes(), items.bytes());
}

extern "C" int rtn_lattice_masks(rtn_handle_t h, int n, const uint8_t* const* pages, const int32_t* heights, const int32_t* widths,
                                 const int32_t* channels, int n_boxes, const int32_t* box_page, const int32_t* crops, int line_scale,
                                 const int64_t* offsets, uint8_t* bw, uint8_t* hm, uint8_t* vm, uint8_t* ink, size_t mask_bytes,
                                 void* workspace, size_t workspace_bytes) {
    if (!h) return RTN_EINVAL;
    std::vector<LCrop> cr;
    RTN_PLAN(h, "rtn_lattice_masks", lat_plan_crops(n_boxes, crops, offsets, mask_bytes, &cr));
    RTN_PLAN(h, "rtn_lattice_masks", lat_plan_pages(n, pages, heights, widths, channels, n_boxes, box_page, line_scale, &cr));
    if (n_boxes && (!bw || !hm || !vm || !ink)) return rtn_fail(h, RTN_EINVAL, "rtn_lattice_masks: the four mask buffers expected");
    if (n_boxes == 0) return RTN_OK;
    const Sizes s = sizes_of(n_boxes, crops);
    rtn_stage st;
    const MaskLayout l = mask_layout(st, n_boxes, s.pixels);
    if (const int rc = st.check(h, "rtn_lattice_masks", workspace, workspace_bytes)) return rc;
    // two planes beside the outputs: bw's transpose and its opening; the planes are packed, the crops keep the caller's offsets
    uint8_t* bwT = st.at<uint8_t>(l.bwT);
    uint8_t* vT = st.at<uint8_t>(l.vT);
    std::vector<CRows> rows((size_t)3 * n_boxes);
    int64_t pos = 0;
    for (int j = 0; j < n_boxes; ++j) {
        LCrop& c = cr[j];
        c.toff = pos;
        rows[j] = CRows{bw + c.off, bwT + pos, c.h, c.w, 0, 0};                                    // transpose bw
        rows[n_boxes + j] = CRows{bw + c.off, hm + c.off, c.h, c.w, lat_window(c.w, line_scale), 0};        // open the rows
        rows[2 * n_boxes + j] = CRows{bwT + pos, vT + pos, c.w, c.h, lat_window(c.h, line_scale), 0};       // open the columns
        pos += (int64_t)c.w * c.h;
    }
    st.put(l.crops, cr);
    st.put(l.rows, rows);
    if (const int rc = st.upload(h)) return rc;
    const LCrop* tc = st.at<const LCrop>(l.crops);
    unsigned t_tiles;
    crop_bw_kernel<<<dim3(rtn_blocks_for(s.max_w, CCA_BW_TW) * rtn_blocks_for(s.max_h, CCA_BW_TH), (unsigned)n_boxes), dim3(LAT_THREADS), 0, h->stream>>>(tc, bw);
    RTN_CHECK_LAUNCH(h, "crop_bw_kernel");
    if (const int rc = launch_transpose_open(h, st.at<const CRows>(l.rows), n_boxes, s.max_h, s.max_w, &t_tiles)) return rc;
    finish_kernel<<<dim3(t_tiles, (unsigned)n_boxes), dim3(LAT_THREADS), 0, h->stream>>>(tc, vT, bw, hm, vm, ink);
    RTN_CHECK_LAUNCH(h, "finish_kernel");
    return RTN_OK;
}

extern "C" int rtn_lattice_profiles(rtn_handle_t h, int n_boxes, const int32_t* crops, const int64_t* offsets, const uint8_t* hm,
                                    const uint8_t* vm, const uint8_t* ink, size_t mask_bytes, const int64_t* prof_offsets,
                                    int32_t* profiles, size_t profiles_count, void* workspace, size_t workspace_bytes) {
    if (!h) return RTN_EINVAL;
    std::vector<LCrop> cr;
    std::vector<LProf> pr;
    RTN_PLAN(h, "rtn_lattice_profiles", lat_plan_crops(n_boxes, crops, offsets, mask_bytes, &cr));
    RTN_PLAN(h, "rtn_lattice_profiles", lat_plan_profiles(cr, prof_offsets, profiles_count, &pr));
    if (n_boxes && (!hm || !vm || !ink || !profiles)) return rtn_fail(h, RTN_EINVAL, "rtn_lattice_profiles: the three masks and the profiles expected");
    if (n_boxes == 0) return RTN_OK;
    rtn_stage st;
    st.put(items_room(st, n_boxes, 0), pr);
    if (const int rc = st.commit(h, "rtn_lattice_profiles", workspace, workspace_bytes)) return rc;
    unsigned groups = 1;
    for (const LProf& p : pr) groups = std::max(groups, (unsigned)p.row_groups + rtn_blocks_for(p.w, LAT_COLS_PER_GROUP));
    profile_kernel<<<dim3(groups, (unsigned)n_boxes), dim3(LAT_THREADS), 0, h->stream>>>(st.at<const LProf>(0), hm, vm, ink, profiles);
    RTN_CHECK_LAUNCH(h, "profile_kernel");
    return RTN_OK;
}

extern "C" int rtn_lattice_edges(rtn_handle_t h, int n_boxes, const int32_t* crops, const int64_t* offsets, const int32_t* R, const int32_t* C,
                                 const int64_t* sep_offsets, const int32_t* runs, size_t runs_count, int line_tol, int cover,
                                 const int64_t* edge_offsets, const uint8_t* hm, const uint8_t* vm, size_t mask_bytes, uint8_t* edges,
                                 size_t edges_bytes, void* workspace, size_t workspace_bytes) {
    if (!h) return RTN_EINVAL;
    std::vector<LCrop> cr;
    std::vector<LGrid> gr;
    std::vector<LEdge> ed;
    int64_t need = 0;
    RTN_PLAN(h, "rtn_lattice_edges", lat_plan_crops(n_boxes, crops, offsets, mask_bytes, &cr));
    RTN_PLAN(h, "rtn_lattice_edges", lat_plan_grids(cr, R, C, sep_offsets, runs, runs_count, &gr));
    RTN_PLAN(h, "rtn_lattice_edges", lat_plan_edges(cr, gr, edge_offsets, line_tol, cover, &need, &ed));
    if ((uint64_t)need > edges_bytes) return rtn_fail(h, RTN_EINVAL, "rtn_lattice_edges: %lld edges, room for %zu", (long long)need, edges_bytes);
    if (ed.empty()) return RTN_OK;
    if (!hm || !vm || !edges) return rtn_fail(h, RTN_EINVAL, "rtn_lattice_edges: the two masks and the edges expected");
    rtn_stage st;
    st.put(items_room(st, n_boxes, (int64_t)ed.size()), ed);
    if (const int rc = st.commit(h, "rtn_lattice_edges", workspace, workspace_bytes)) return rc;
    edge_kernel<<<dim3(rtn_blocks_for((int64_t)ed.size(), LAT_EDGES_PER_GROUP)), dim3(LAT_THREADS), 0, h->stream>>>(st.at<const LEdge>(0), (int64_t)ed.size(), hm, vm, cover, edges);
    RTN_CHECK_LAUNCH(h, "edge_kernel");
    return RTN_OK;
}

extern "C" int rtn_lattice_cells(rtn_handle_t h, int n_boxes, const int32_t* crops, const int64_t* offsets, const int32_t* R, const int32_t* C,
                                 const int64_t* sep_offsets, const int32_t* runs, size_t runs_count, const int64_t* cell_offsets,
                                 const uint8_t* ink, size_t mask_bytes, int32_t* cell_ink, int32_t* cell_box, size_t cells_count,
                                 void* workspace, size_t workspace_bytes) {
    if (!h) return RTN_EINVAL;
    std::vector<LCrop> cr;
    std::vector<LGrid> gr;
    std::vector<LCell> ce;
    int64_t need = 0;
    RTN_PLAN(h, "rtn_lattice_cells", lat_plan_crops(n_boxes, crops, offsets, mask_bytes, &cr));
    RTN_PLAN(h, "rtn_lattice_cells", lat_plan_grids(cr, R, C, sep_offsets, runs, runs_count, &gr));
    RTN_PLAN(h, "rtn_lattice_cells", lat_plan_cells(cr, gr, cell_offsets, &need, &ce));
    if ((uint64_t)need > cells_count) return rtn_fail(h, RTN_EINVAL, "rtn_lattice_cells: %lld cells, room for %zu", (long long)need, cells_count);
    if (ce.empty()) return RTN_OK;
    if (ce.size() > 0x7fffffffull) return rtn_fail(h, RTN_EINVAL, "rtn_lattice_cells: %zu cells are more than one launch takes", ce.size());
    if (!ink || !cell_ink || !cell_box) return rtn_fail(h, RTN_EINVAL, "rtn_lattice_cells: the ink mask and the two cell tables expected");
    rtn_stage st;
    st.put(items_room(st, n_boxes, (int64_t)ce.size()), ce);
    if (const int rc = st.commit(h, "rtn_lattice_cells", workspace, workspace_bytes)) return rc;
    cell_kernel<<<dim3((unsigned)ce.size()), dim3(LAT_THREADS), 0, h->stream>>>(st.at<const LCell>(0), ink, cell_ink, cell_box);
    RTN_CHECK_LAUNCH(h, "cell_kernel");
    return RTN_OK;
}

// ---- host only: the separators (both paths call it) and the CPU twins, through the bodies of rtn_lattice.h ----------------------------
extern "C" int rtn_lattice_separators_host(const int32_t* profile, int n, int mode, int param, int capacity, int32_t* runs, int32_t* count) {
    if (!profile || !count || n < 1 || n > CCA_MAX_SIDE || (mode != 0 && mode != 1) || param < 0 || capacity < 0 || (capacity && !runs))
        return rtn_fail_host(nullptr, RTN_EINVAL, "rtn_lattice_separators_host: a profile of 1 .. 16384, mode 0 or 1, param >= 0 and room for the runs expected");
    const int64_t got = lat_runs(profile, n, mode, param, capacity, runs);
    *count = (int32_t)got;
    if (got > capacity) return rtn_fail_host(nullptr, RTN_EINVAL, "rtn_lattice_separators_host: %lld runs, room for %d (count holds the true number)", (long long)got, capacity);
    return RTN_OK;
}

extern "C" int rtn_lattice_masks_host(int n, const uint8_t* const* pages, const int32_t* heights, const int32_t* widths, const int32_t* channels,
                                      int n_boxes, const int32_t* box_page, const int32_t* crops, int line_scale, const int64_t* offsets,
                                      uint8_t* bw, uint8_t* hm, uint8_t* vm, uint8_t* ink, size_t mask_bytes) {
    std::vector<LCrop> cr;
    RTN_PLAN(nullptr, "rtn_lattice_masks_host", lat_plan_crops(n_boxes, crops, offsets, mask_bytes, &cr));
    RTN_PLAN(nullptr, "rtn_lattice_masks_host", lat_plan_pages(n, pages, heights, widths, channels, n_boxes, box_page, line_scale, &cr));
    if (n_boxes && (!bw || !hm || !vm || !ink)) return rtn_fail_host(nullptr, RTN_EINVAL, "rtn_lattice_masks_host: the four mask buffers expected");
    std::vector<uint8_t> page_bw;
    for (int i = 0; i < n; ++i) {                                               // a page's threshold once, whatever the number of its boxes
        bool done = false;
        for (int j = 0; j < n_boxes; ++j) {
            if (box_page[j] != i) continue;
            if (!done) lat_bw_page(lat_page(cr[j]), &page_bw);
            done = true;
            lat_masks_crop(cr[j], page_bw.data(), line_scale, bw + cr[j].off, hm + cr[j].off, vm + cr[j].off, ink + cr[j].off);
        }
    }
    return RTN_OK;
}

extern "C" int rtn_lattice_profiles_host(int n_boxes, const int32_t* crops, const int64_t* offsets, const uint8_t* hm, const uint8_t* vm,
                                         const uint8_t* ink, size_t mask_bytes, const int64_t* prof_offsets, int32_t* profiles,
                                         size_t profiles_count) {
    std::vector<LCrop> cr;
    std::vector<LProf> pr;
    RTN_PLAN(nullptr, "rtn_lattice_profiles_host", lat_plan_crops(n_boxes, crops, offsets, mask_bytes, &cr));
    RTN_PLAN(nullptr, "rtn_lattice_profiles_host", lat_plan_profiles(cr, prof_offsets, profiles_count, &pr));
    if (n_boxes && (!hm || !vm || !ink || !profiles)) return rtn_fail_host(nullptr, RTN_EINVAL, "rtn_lattice_profiles_host: the three masks and the profiles expected");
    for (const LProf& p : pr) lat_profiles_crop(p, hm, vm, ink, profiles);
    return RTN_OK;
}

extern "C" int rtn_lattice_edges_host(int n_boxes, const int32_t* crops, const int64_t* offsets, const int32_t* R, const int32_t* C,
                                      const int64_t* sep_offsets, const int32_t* runs, size_t runs_count, int line_tol, int cover,
                                      const int64_t* edge_offsets, const uint8_t* hm, const uint8_t* vm, size_t mask_bytes, uint8_t* edges,
                                      size_t edges_bytes) {
    std::vector<LCrop> cr;
    std::vector<LGrid> gr;
    std::vector<LEdge> ed;
    int64_t need = 0;
    RTN_PLAN(nullptr, "rtn_lattice_edges_host", lat_plan_crops(n_boxes, crops, offsets, mask_bytes, &cr));
    RTN_PLAN(nullptr, "rtn_lattice_edges_host", lat_plan_grids(cr, R, C, sep_offsets, runs, runs_count, &gr));
    RTN_PLAN(nullptr, "rtn_lattice_edges_host", lat_plan_edges(cr, gr, edge_offsets, line_tol, cover, &need, &ed));
    if ((uint64_t)need > edges_bytes) return rtn_fail_host(nullptr, RTN_EINVAL, "rtn_lattice_edges_host: %lld edges, room for %zu", (long long)need, edges_bytes);
    if (!ed.empty() && (!hm || !vm || !edges)) return rtn_fail_host(nullptr, RTN_EINVAL, "rtn_lattice_edges_host: the two masks and the edges expected");
    for (const LEdge& e : ed) edges[e.out] = lat_edge(e, hm, vm, cover);
    return RTN_OK;
}

extern "C" int rtn_lattice_cells_host(int n_boxes, const int32_t* crops, const int64_t* offsets, const int32_t* R, const int32_t* C,
                                      const int64_t* sep_offsets, const int32_t* runs, size_t runs_count, const int64_t* cell_offsets,
                                      const uint8_t* ink, size_t mask_bytes, int32_t* cell_ink, int32_t* cell_box, size_t cells_count) {
    std::vector<LCrop> cr;
    std::vector<LGrid> gr;
    std::vector<LCell> ce;
    int64_t need = 0;
    RTN_PLAN(nullptr, "rtn_lattice_cells_host", lat_plan_crops(n_boxes, crops, offsets, mask_bytes, &cr));
    RTN_PLAN(nullptr, "rtn_lattice_cells_host", lat_plan_grids(cr, R, C, sep_offsets, runs, runs_count, &gr));
    RTN_PLAN(nullptr, "rtn_lattice_cells_host", lat_plan_cells(cr, gr, cell_offsets, &need, &ce));
    if ((uint64_t)need > cells_count) return rtn_fail_host(nullptr, RTN_EINVAL, "rtn_lattice_cells_host: %lld cells, room for %zu", (long long)need, cells_count);
    if (!ce.empty() && (!ink || !cell_ink || !cell_box)) return rtn_fail_host(nullptr, RTN_EINVAL, "rtn_lattice_cells_host: the ink mask and the two cell tables expected");
    for (const LCell& c : ce) lat_cell(c, ink, cell_ink, cell_box);
    return RTN_OK;
}
