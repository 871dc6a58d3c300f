// rtn_cca.hip — scan analysis on the device (connectedComponentAnalysis.py): ruling-line masks, the text-line mask,
// connected-component labelling and painting.  Integers only; no kernel waits on another workgroup, every step that needs the
// whole image finished is a launch of its own on the handle's stream.
//
//   bw_kernel          64x32 tiles: bitwise_not(gray), the 15x15 box sum (row sums, then column sums, in LDS), the mean threshold.
//   transpose_kernel   32x32 tiles through LDS: the column opening runs as a row opening of the transposed image.
//   open_rows_kernel   one workgroup per row.  A thread owns <= 64 consecutive pixels as a bit mask; a window step is a workgroup
//                      prefix count of the ones into LDS (16 bits per pixel) and two reads per pixel, whatever the window length.
//   text_rows_kernel   one workgroup per row: blur, the gray close of 4, black-hat and threshold into the bit masks, then the five
//                      binary steps (dilate 28, close 10 twice) as window steps; the row goes out through LDS.
//   label_*            tiles in LDS (horizontal runs by a wave ballot, union-find between rows, label = smallest raster index), merge across tile borders (atomicMin union-find in
//                      global memory: a loop repeats only after another thread lowered a label, labels are bounded below), flatten,
//                      the flags of external components from the joint labelling of foreground (8-connected) and background
//                      (4-connected), ranks by a prefix sum over root pixels in raster order, boxes by integer atomicMin / atomicMax.
//   paint_kernel       rectangles: white boxes, green outlines.
// The per-element rules and the CPU twins' bodies are in rtn_cca.h; bw_kernel's tile, transpose_kernel, open_rows_kernel and the
// window step, which csrc/rtn_lattice.hip uses too, are in rtn_cca_rows.h.
#include <algorithm>
#include <vector>
#include "rtn_page_launch.h"
#include "rtn_cca.h"
#include "rtn_cca_rows.h"

namespace {

// ---- masks ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CCA_PIX_THREADS) void bw_kernel(const CPage* pages, uint8_t* bw) {
    const CPage p = pages[blockIdx.y];
    bw_tile(p, 0, 0, p.h, p.w, bw + p.off);
}

__global__ __launch_bounds__(CCA_ROW_THREADS) void text_rows_kernel(const CPage* pages, uint8_t* closed) {
    extern __shared__ uint16_t P[];                                             // first the blurred and the dilated row (bytes), then the counts
    __shared__ int wave_sums[CCA_ROW_THREADS / 64];
    const CPage p = pages[blockIdx.y];
    if ((int)blockIdx.x >= p.h) return;                                         // uniform
    const int n = p.w, y = blockIdx.x, tid = threadIdx.x;
    uint8_t* blur = reinterpret_cast<uint8_t*>(P);
    uint8_t* dil = blur + n;
    for (int x = tid; x < n; x += CCA_ROW_THREADS) blur[x] = cca_blur(p, y, x);
    __syncthreads();
    for (int x = tid; x < n; x += CCA_ROW_THREADS) {
        int lo, hi, mx = 0;
        cca_window(x, 4, 2, n, &lo, &hi);
        for (int i = lo; i <= hi; ++i) mx = max(mx, (int)blur[i]);
        dil[x] = (uint8_t)mx;
    }
    __syncthreads();
    const int per = (n + CCA_ROW_THREADS - 1) / CCA_ROW_THREADS;
    const int x0 = tid * per, cnt = max(0, min(per, n - x0));
    uint64_t bits = 0;
    for (int i = 0; i < cnt; ++i) {
        int lo, hi, mn = 255;
        cca_window(x0 + i, 4, 2, n, &lo, &hi);
        for (int j = lo; j <= hi; ++j) mn = min(mn, (int)dil[j]);
        if (mn - (int)blur[x0 + i] > 10) bits |= 1ull << i;
    }
    __syncthreads();                                                            // blur and dil are read: P takes the counts
    for (int s = 0; s < CCA_STEPS; ++s) {
        int L, anchor;
        bool is_min;
        cca_text_step(s, &L, &anchor, &is_min);
        bits = window_step(bits, x0, cnt, n, L, anchor, is_min, P, wave_sums);
    }
    for (int i = 0; i < cnt; ++i) blur[x0 + i] = (bits >> i) & 1 ? 255 : 0;
    __syncthreads();
    uint8_t* dst = closed + p.off + (int64_t)y * n;
    for (int x = tid; x < n; x += CCA_ROW_THREADS) dst[x] = blur[x];
}

// ---- labelling ------------------------------------------------------------------------------------------------------------------
// Union-find over labels that only ever decrease.  find: follow the links to a root.  unite: link the larger root to the smaller
// with atomicMin; when the word held something else, another thread linked it first: go on with that value.  An iteration repeats
// only after some label decreased, and labels are bounded below by 0.
template <class T>
__device__ inline int uf_find(const T* lab, int a) {
    int p = lab[a];
    while (p != a) {
        a = p;
        p = lab[a];
    }
    return a;
}
__device__ inline void uf_unite(int* lab, int a, int b) {
    for (;;) {
        a = uf_find(const_cast<const volatile int*>(lab), a);
        b = uf_find(const_cast<const volatile int*>(lab), b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }                          // a > b: a goes under b
        const int old = atomicMin(&lab[a], b);
        if (old == a) return;
        a = old;
    }
}

// find with path compression for the merge across tiles, where chains of tile roots grow long: every node on the way is pointed at
// the root found (smaller, same component) with atomicMin, so labels still only decrease.  The walk ends at the first node <= root
// (another thread may have pointed a node past it meanwhile); nodes above the root have lab[a] < a, so it moves on strictly.
__device__ inline int uf_find_compress(int* lab, int a) {
    const int root = uf_find(const_cast<const volatile int*>(lab), a);
    while (a > root) {
        const int next = *const_cast<const volatile int*>(&lab[a]);
        if (next > root) atomicMin(&lab[a], root);
        a = next;
    }
    return root;
}

constexpr int CCA_TILE = CCA_TILE_W * CCA_TILE_H;

__global__ __launch_bounds__(CCA_TILE) void label_tiles_kernel(const CLab* imgs, int32_t* labels) {
    __shared__ int lab[CCA_TILE];
    __shared__ int8_t val[CCA_TILE];
    const CLab m = imgs[blockIdx.y];
    const int tiles_x = (m.w + CCA_TILE_W - 1) / CCA_TILE_W, tiles_y = (m.h + CCA_TILE_H - 1) / CCA_TILE_H;
    if ((int)blockIdx.x >= tiles_x * tiles_y) return;                          // uniform
    const int tx0 = ((int)blockIdx.x % tiles_x) * CCA_TILE_W, ty0 = ((int)blockIdx.x / tiles_x) * CCA_TILE_H;
    const int tid = threadIdx.x, lx = tid % CCA_TILE_W, ly = tid / CCA_TILE_W, x = tx0 + lx, y = ty0 + ly;
    const bool in = x < m.w && y < m.h;
    const int v = in ? (m.img[(size_t)y * m.w + x] != 0) : -1;
    val[tid] = (int8_t)v;
    __syncthreads();
    // a row of the tile is half a wave: a pixel starts at the first pixel of its horizontal run (joined along x whatever the value)
    const bool join_left = in && lx > 0 && val[tid - 1] == v;
    const uint32_t joined = (uint32_t)(__ballot(join_left) >> (tid & 32));
    const int start = 31 - __clz((int)(~joined & (uint32_t)((2ull << lx) - 1)));                  // bit 0 is never set
    lab[tid] = ly * CCA_TILE_W + start;
    __syncthreads();
    if (in && ly > 0) {
        const int up = tid - CCA_TILE_W;
        if (val[up] == v) {                                                      // one union per pair of overlapping runs: where either starts
            if (lx == 0 || start == lx || val[up - 1] != v) uf_unite(lab, tid, up);
        } else if (v == 1) {                                                     // the pixel above is background: the diagonals
            if (lx > 0 && val[up - 1] == 1) uf_unite(lab, tid, up - 1);
            if (lx < CCA_TILE_W - 1 && val[up + 1] == 1) uf_unite(lab, tid, up + 1);
        }
    }
    __syncthreads();
    if (in) {
        const int r = uf_find(const_cast<const volatile int*>(lab), tid);
        labels[m.pix_off + (int64_t)y * m.w + x] = (ty0 + r / CCA_TILE_W) * m.w + tx0 + r % CCA_TILE_W;
    }
}

// the pixel a thread of a per-pixel launch owns
__device__ inline bool pixel_of(const CLab& m, int64_t* i, int* y, int* x) {
    *i = (int64_t)blockIdx.x * CCA_PIX_THREADS + threadIdx.x;
    if (*i >= (int64_t)m.h * m.w) return false;
    *y = (int)(*i / m.w);
    *x = (int)(*i % m.w);
    return true;
}

// The links across tile borders.  One union per pair of overlapping runs along a border: a pixel on a tile's top row unites with the
// pixel above unless both have equal-valued left neighbours in their own tiles (those two made the link); the same for the left
// column with the pixels above.  A diagonal is needed only for a foreground pixel whose upper neighbour is background (and, for the
// upper left one, whose left neighbour is background too): otherwise the two are joined through that neighbour.
__global__ __launch_bounds__(CCA_PIX_THREADS) void label_merge_kernel(const CLab* imgs, int32_t* labels) {
    const CLab m = imgs[blockIdx.y];
    int64_t i;
    int y, x;
    if (!pixel_of(m, &i, &y, &x)) return;
    const int lx = x % CCA_TILE_W, ly = y % CCA_TILE_H;
    if (lx != 0 && ly != 0 && lx != CCA_TILE_W - 1) return;
    const uint8_t* p = m.img + i;
    const int w = m.w, v = p[0] != 0;
    const int up = y > 0 ? (p[-w] != 0) : -1, left = x > 0 ? (p[-1] != 0) : -1;
    const int up_left = y > 0 && x > 0 ? (p[-w - 1] != 0) : -1;
    int* lab = labels + m.pix_off;
    const int me = (int)i;
    if (ly == 0 && up == v && (lx == 0 || left != v || up_left != v)) uf_unite(lab, uf_find_compress(lab, me), uf_find_compress(lab, me - w));
    if (lx == 0 && left == v && (ly == 0 || up != v || up_left != v)) uf_unite(lab, uf_find_compress(lab, me), uf_find_compress(lab, me - 1));
    if (v == 1 && up == 0) {
        if (left == 0 && up_left == 1 && (lx == 0 || ly == 0)) uf_unite(lab, uf_find_compress(lab, me), uf_find_compress(lab, me - w - 1));
        if (x < w - 1 && p[-w + 1] != 0 && (ly == 0 || lx == CCA_TILE_W - 1)) uf_unite(lab, uf_find_compress(lab, me), uf_find_compress(lab, me - w + 1));
    }
}

// every pixel takes its root; the flags start at 0
__global__ __launch_bounds__(CCA_PIX_THREADS) void label_flatten_kernel(const CLab* imgs, int32_t* labels, uint8_t* flags) {
    const CLab m = imgs[blockIdx.y];
    int64_t i;
    int y, x;
    if (!pixel_of(m, &i, &y, &x)) return;
    int* lab = labels + m.pix_off;
    lab[i] = uf_find(const_cast<const volatile int*>(lab), (int)i);
    flags[m.pix_off + i] = 0;
}

// a background component that touches the page's edge belongs to the region of the frame: flag its root
__global__ __launch_bounds__(CCA_PIX_THREADS) void label_frame_kernel(const CLab* imgs, const int32_t* labels, uint8_t* flags) {
    const CLab m = imgs[blockIdx.y];
    int64_t i;
    int y, x;
    if (!pixel_of(m, &i, &y, &x)) return;
    if (m.img[i] != 0 || (x != 0 && y != 0 && x != m.w - 1 && y != m.h - 1)) return;
    flags[m.pix_off + labels[m.pix_off + i]] = 1;
}

// a foreground component with a pixel on the page's edge or 4-adjacent to the frame's region is external: flag its root
__global__ __launch_bounds__(CCA_PIX_THREADS) void label_external_kernel(const CLab* imgs, const int32_t* labels, uint8_t* flags) {
    const CLab m = imgs[blockIdx.y];
    int64_t i;
    int y, x;
    if (!pixel_of(m, &i, &y, &x)) return;
    if (m.img[i] == 0) return;
    const int32_t* lab = labels + m.pix_off;
    const uint8_t* fl = flags + m.pix_off;
    bool ext = x == 0 || y == 0 || x == m.w - 1 || y == m.h - 1;
    if (!ext) {
        const int64_t nb[4] = {i - 1, i + 1, i - m.w, i + m.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) ext = ext || (m.img[nb[k]] == 0 && fl[lab[nb[k]]] != 0);
    }
    if (ext) flags[m.pix_off + lab[i]] = 1;
}

// is pixel i the root of a component that is counted
__device__ inline bool counted_root(const CLab& m, const int32_t* lab, const uint8_t* fl, int64_t i, int external_only) {
    return m.img[i] != 0 && lab[i] == (int32_t)i && (!external_only || fl[i] != 0);
}

__global__ __launch_bounds__(CCA_PIX_THREADS) void label_count_kernel(const CLab* imgs, const int32_t* labels, const uint8_t* flags,
                                                                       int external_only, int32_t* block_counts) {
    __shared__ int wave_sums[CCA_PIX_THREADS / 64];
    const CLab m = imgs[blockIdx.y];
    const int64_t px = (int64_t)m.h * m.w, first = ((int64_t)blockIdx.x * CCA_PIX_THREADS + threadIdx.x) * CCA_RANK_PIXELS;
    if ((int64_t)blockIdx.x * CCA_PIX_THREADS * CCA_RANK_PIXELS >= px) return;                     // uniform
    int c = 0;
    for (int j = 0; j < CCA_RANK_PIXELS; ++j)
        if (first + j < px) c += counted_root(m, labels + m.pix_off, flags + m.pix_off, first + j, external_only);
    int total;
    block_scan(c, wave_sums, &total);
    if (threadIdx.x == 0) block_counts[m.blk_off + blockIdx.x] = total;
}

// one workgroup per image: the counts of its workgroups become their exclusive prefix sums; the total is the image's count
__global__ __launch_bounds__(CCA_PIX_THREADS) void label_scan_kernel(const CLab* imgs, int32_t* block_counts, int32_t* counts) {
    __shared__ int wave_sums[CCA_PIX_THREADS / 64];
    const CLab m = imgs[blockIdx.x];
    const int64_t px = (int64_t)m.h * m.w;
    const int nb = (int)((px + CCA_PIX_THREADS * CCA_RANK_PIXELS - 1) / (CCA_PIX_THREADS * CCA_RANK_PIXELS));
    int32_t* bc = block_counts + m.blk_off;
    int base = 0;
    for (int b0 = 0; b0 < nb; b0 += CCA_PIX_THREADS) {                          // nb is uniform: every thread scans every round
        const int b = b0 + threadIdx.x;
        const int v = b < nb ? bc[b] : 0;
        int total;
        const int ex = block_scan(v, wave_sums, &total);
        if (b < nb) bc[b] = base + ex;
        base += total;
    }
    if (threadIdx.x == 0) counts[blockIdx.x] = base;
}

// the rank of every counted root in raster order; a root within the capacity starts its box at itself (x0, y0, x1, y1)
__global__ __launch_bounds__(CCA_PIX_THREADS) void label_rank_kernel(const CLab* imgs, const int32_t* labels, const uint8_t* flags,
                                                                      int external_only, const int32_t* block_counts, int32_t* ranks,
                                                                      int32_t* boxes) {
    __shared__ int wave_sums[CCA_PIX_THREADS / 64];
    const CLab m = imgs[blockIdx.y];
    const int64_t px = (int64_t)m.h * m.w, first = ((int64_t)blockIdx.x * CCA_PIX_THREADS + threadIdx.x) * CCA_RANK_PIXELS;
    if ((int64_t)blockIdx.x * CCA_PIX_THREADS * CCA_RANK_PIXELS >= px) return;                     // uniform
    bool root[CCA_RANK_PIXELS];
    int c = 0;
    for (int j = 0; j < CCA_RANK_PIXELS; ++j) {
        root[j] = first + j < px && counted_root(m, labels + m.pix_off, flags + m.pix_off, first + j, external_only);
        c += root[j];
    }
    int total;
    int k = block_counts[m.blk_off + blockIdx.x] + block_scan(c, wave_sums, &total);
    for (int j = 0; j < CCA_RANK_PIXELS; ++j) {
        if (!root[j]) continue;
        const int64_t i = first + j;
        ranks[m.pix_off + i] = k;
        if (k < m.cap) {
            const int x = (int)(i % m.w), y = (int)(i / m.w);
            int32_t* b = boxes + 4 * (m.box_off + k);
            b[0] = x; b[1] = y; b[2] = x; b[3] = y;
        }
        ++k;
    }
}

// every foreground pixel of a counted component widens the component's box; the read before an atomic only saves atomics (a stale
// value is never smaller than the minimum so far, nor larger than the maximum)
__global__ __launch_bounds__(CCA_PIX_THREADS) void label_boxes_kernel(const CLab* imgs, const int32_t* labels, const uint8_t* flags,
                                                                       int external_only, const int32_t* ranks, int32_t* boxes) {
    const CLab m = imgs[blockIdx.y];
    int64_t i;
    int y, x;
    if (!pixel_of(m, &i, &y, &x)) return;
    if (m.img[i] == 0) return;
    // a box's left, right and bottom are reached at pixels without a foreground neighbour on that side
    if (x > 0 && x < m.w - 1 && y < m.h - 1 && m.img[i - 1] != 0 && m.img[i + 1] != 0 && m.img[i + m.w] != 0) return;
    const int r = labels[m.pix_off + i];
    if (external_only && flags[m.pix_off + r] == 0) return;
    const int k = ranks[m.pix_off + r];
    if (k >= m.cap) return;
    int32_t* b = boxes + 4 * (m.box_off + k);
    if (x < *(volatile int32_t*)&b[0]) atomicMin(&b[0], x);
    if (x > *(volatile int32_t*)&b[2]) atomicMax(&b[2], x);
    if (y > *(volatile int32_t*)&b[3]) atomicMax(&b[3], y);                    // y0 is the root's row: the root is the first pixel
}

// (x0, y0, x1, y1) -> (x, y, w, h)
__global__ __launch_bounds__(CCA_PIX_THREADS) void label_finish_kernel(const CLab* imgs, const int32_t* counts, int32_t* boxes) {
    const CLab m = imgs[blockIdx.y];
    const int k = blockIdx.x * CCA_PIX_THREADS + threadIdx.x;
    if (k >= m.cap || k >= counts[blockIdx.y]) return;
    int32_t* b = boxes + 4 * (m.box_off + k);
    b[2] = b[2] - b[0] + 1;
    b[3] = b[3] - b[1] + 1;
}

// ---- painting -------------------------------------------------------------------------------------------------------------------
// rectangle blockIdx.x, slice blockIdx.y of its pixels; overlapping rectangles write the same value
__global__ __launch_bounds__(CCA_PIX_THREADS) void paint_kernel(const CPaintPage* pages, const CRect* rects, int mode) {
    const CRect r = rects[blockIdx.x];
    const CPaintPage p = pages[r.page];
    const int rw = r.x1 - r.x0;
    const int64_t area = (int64_t)rw * (r.y1 - r.y0);
    for (int64_t i = (int64_t)blockIdx.y * CCA_PIX_THREADS + threadIdx.x; i < area; i += (int64_t)gridDim.y * CCA_PIX_THREADS)
        cca_paint_pixel(p, mode, r.y0 + (int)(i / rw), r.x0 + (int)(i % rw));
}

// ---- workspace ------------------------------------------------------------------------------------------------------------------
struct Sizes { int64_t pixels = 0, blocks = 0; int max_h = 0, max_w = 0; int64_t max_px = 0; };
Sizes sizes_of(int n, const int32_t* heights, const int32_t* widths) {
    Sizes s;
    for (int i = 0; i < n; ++i) {
        const int64_t px = (int64_t)heights[i] * widths[i];
        s.pixels += px;
        s.blocks += (px + CCA_PIX_THREADS * CCA_RANK_PIXELS - 1) / (CCA_PIX_THREADS * CCA_RANK_PIXELS);
        s.max_h = std::max(s.max_h, heights[i]);
        s.max_w = std::max(s.max_w, widths[i]);
        s.max_px = std::max(s.max_px, px);
    }
    return s;
}
// tables first (the largest any entry uploads: 4 n CRows, n CLab or n pages and 4 n_boxes rectangles), then the per-pixel arrays:
// labels and ranks (4 bytes each) and flags (1) for labelling; three byte planes for the line masks fit in the same room
struct Layout { size_t rows, lab, rects, labels, ranks, flags, block_counts; };
Layout layout_of(rtn_stage& st, int n, int n_boxes, const Sizes& s) {
    Layout l;
    l.rows = st.reserve((int64_t)n * 4 * sizeof(CRows));
    l.lab = st.reserve((int64_t)n * sizeof(CLab));
    l.rects = st.reserve((int64_t)n_boxes * 4 * sizeof(CRect));
    l.labels = st.reserve(s.pixels * 4);
    l.ranks = st.reserve(s.pixels * 4);
    l.flags = st.reserve(s.pixels);
    l.block_counts = st.reserve(s.blocks * 4);
    return l;
}

}  // namespace

// rtn_cca_*: see include/rtn.h
extern "C" size_t rtn_cca_workspace_bytes(int n, const int32_t* heights, const int32_t* widths, int n_boxes) {
    if (n_boxes < 0 || cca_check_sizes(n, heights, widths)) return 0;
    rtn_stage st;
    layout_of(st, n, n_boxes, sizes_of(n, heights, widths));
    return st.bytes();
}

extern "C" int rtn_cca_lines_mask(rtn_handle_t h, int n, const uint8_t* const* pages, const int32_t* heights, const int32_t* widths,
                                  const int32_t* channels, const int64_t* offsets, uint8_t* horizontal, uint8_t* vertical,
                                  size_t mask_bytes, void* workspace, size_t workspace_bytes) {
    if (!h) return RTN_EINVAL;
    std::vector<CPage> pg;
    RTN_PLAN(h, "rtn_cca_lines_mask", cca_plan_pages(n, pages, heights, widths, channels, offsets, mask_bytes, &pg));
    if (n && (!horizontal || !vertical)) return rtn_fail(h, RTN_EINVAL, "rtn_cca_lines_mask: the two mask buffers expected");
    if (n == 0) return RTN_OK;
    const Sizes s = sizes_of(n, heights, widths);
    rtn_stage st;
    const Layout l = layout_of(st, n, 0, s);
    if (const int rc = st.check(h, "rtn_cca_lines_mask", workspace, workspace_bytes)) return rc;
    // three planes of the pages' pixels in the room of the labels: bw, its transpose, the opened transpose
    uint8_t* bw = st.at<uint8_t>(l.labels);
    uint8_t* bwT = bw + rtn_a256(s.pixels);
    uint8_t* vT = bwT + rtn_a256(s.pixels);
    std::vector<CPage> pbw(pg);
    std::vector<CRows> rows((size_t)4 * n);
    int64_t pos = 0;
    for (int i = 0; i < n; ++i) {
        const CPage& p = pg[i];
        pbw[i].off = pos;
        rows[i] = CRows{bw + pos, bwT + pos, p.h, p.w, 0, 0};                                     // transpose bw
        rows[n + i] = CRows{bw + pos, horizontal + p.off, p.h, p.w, p.w / 30, 0};                 // open the rows
        rows[2 * n + i] = CRows{bwT + pos, vT + pos, p.w, p.h, p.h / 30, 0};                      // open the columns
        rows[3 * n + i] = CRows{vT + pos, vertical + p.off, p.w, p.h, 0, 0};                      // transpose back
        pos += (int64_t)p.h * p.w;
    }
    st.put(l.rows, rows);
    st.put(l.lab, pbw);
    if (const int rc = st.upload(h)) return rc;
    const CRows* tr = st.at<const CRows>(l.rows);
    unsigned t_tiles;
    bw_kernel<<<dim3(rtn_blocks_for(s.max_w, CCA_BW_TW) * rtn_blocks_for(s.max_h, CCA_BW_TH), (unsigned)n), dim3(CCA_PIX_THREADS), 0, h->stream>>>(st.at<const CPage>(l.lab), bw);
    RTN_CHECK_LAUNCH(h, "bw_kernel");
    if (const int rc = launch_transpose_open(h, tr, n, s.max_h, s.max_w, &t_tiles)) return rc;
    transpose_kernel<<<dim3(t_tiles, (unsigned)n), dim3(CCA_PIX_THREADS), 0, h->stream>>>(tr + 3 * n);
    RTN_CHECK_LAUNCH(h, "transpose_kernel");
    return RTN_OK;
}

extern "C" int rtn_cca_text_mask(rtn_handle_t h, int n, const uint8_t* const* pages, const int32_t* heights, const int32_t* widths,
                                 const int32_t* channels, const int64_t* offsets, uint8_t* closed, size_t mask_bytes, void* workspace,
                                 size_t workspace_bytes) {
    if (!h) return RTN_EINVAL;
    std::vector<CPage> pg;
    RTN_PLAN(h, "rtn_cca_text_mask", cca_plan_pages(n, pages, heights, widths, channels, offsets, mask_bytes, &pg));
    if (n && !closed) return rtn_fail(h, RTN_EINVAL, "rtn_cca_text_mask: the mask buffer expected");
    if (n == 0) return RTN_OK;
    const Sizes s = sizes_of(n, heights, widths);
    rtn_stage st;
    const Layout l = layout_of(st, n, 0, s);
    st.put(l.rows, pg);
    if (const int rc = st.commit(h, "rtn_cca_text_mask", workspace, workspace_bytes)) return rc;
    text_rows_kernel<<<dim3((unsigned)s.max_h, (unsigned)n), dim3(CCA_ROW_THREADS), row_lds_bytes(s.max_w), h->stream>>>(st.at<const CPage>(l.rows), closed);
    RTN_CHECK_LAUNCH(h, "text_rows_kernel");
    return RTN_OK;
}

extern "C" int rtn_cca_label(rtn_handle_t h, int n, const uint8_t* const* images, const int32_t* heights, const int32_t* widths,
                             int external_only, const int32_t* capacity, const int64_t* box_offsets, int32_t* counts, int32_t* boxes,
                             size_t boxes_bytes, void* workspace, size_t workspace_bytes) {
    if (!h) return RTN_EINVAL;
    std::vector<CLab> im;
    RTN_PLAN(h, "rtn_cca_label", cca_plan_label(n, images, heights, widths, capacity, box_offsets, counts, boxes, boxes_bytes, &im));
    if (n == 0) return RTN_OK;
    const Sizes s = sizes_of(n, heights, widths);
    rtn_stage st;
    const Layout l = layout_of(st, n, 0, s);
    st.put(l.rows, im);
    if (const int rc = st.commit(h, "rtn_cca_label", workspace, workspace_bytes)) return rc;
    const CLab* t = st.at<const CLab>(l.rows);
    int32_t* labels = st.at<int32_t>(l.labels);
    int32_t* ranks = st.at<int32_t>(l.ranks);
    uint8_t* flags = st.at<uint8_t>(l.flags);
    int32_t* block_counts = st.at<int32_t>(l.block_counts);
    const dim3 tiles(rtn_blocks_for(s.max_w, CCA_TILE_W) * rtn_blocks_for(s.max_h, CCA_TILE_H), (unsigned)n);
    const dim3 pixels(rtn_blocks_for(s.max_px, CCA_PIX_THREADS), (unsigned)n);
    const dim3 groups(rtn_blocks_for(s.max_px, CCA_PIX_THREADS * CCA_RANK_PIXELS), (unsigned)n);
    int max_cap = 0;
    for (const CLab& m : im) max_cap = std::max(max_cap, m.cap);
    label_tiles_kernel<<<tiles, dim3(CCA_TILE), 0, h->stream>>>(t, labels);
    RTN_CHECK_LAUNCH(h, "label_tiles_kernel");
    label_merge_kernel<<<pixels, dim3(CCA_PIX_THREADS), 0, h->stream>>>(t, labels);
    RTN_CHECK_LAUNCH(h, "label_merge_kernel");
    label_flatten_kernel<<<pixels, dim3(CCA_PIX_THREADS), 0, h->stream>>>(t, labels, flags);
    RTN_CHECK_LAUNCH(h, "label_flatten_kernel");
    if (external_only) {
        label_frame_kernel<<<pixels, dim3(CCA_PIX_THREADS), 0, h->stream>>>(t, labels, flags);
        RTN_CHECK_LAUNCH(h, "label_frame_kernel");
        label_external_kernel<<<pixels, dim3(CCA_PIX_THREADS), 0, h->stream>>>(t, labels, flags);
        RTN_CHECK_LAUNCH(h, "label_external_kernel");
    }
    label_count_kernel<<<groups, dim3(CCA_PIX_THREADS), 0, h->stream>>>(t, labels, flags, external_only, block_counts);
    RTN_CHECK_LAUNCH(h, "label_count_kernel");
    label_scan_kernel<<<dim3((unsigned)n), dim3(CCA_PIX_THREADS), 0, h->stream>>>(t, block_counts, counts);
    RTN_CHECK_LAUNCH(h, "label_scan_kernel");
    label_rank_kernel<<<groups, dim3(CCA_PIX_THREADS), 0, h->stream>>>(t, labels, flags, external_only, block_counts, ranks, boxes);
    RTN_CHECK_LAUNCH(h, "label_rank_kernel");
    if (max_cap > 0) {
        label_boxes_kernel<<<pixels, dim3(CCA_PIX_THREADS), 0, h->stream>>>(t, labels, flags, external_only, ranks, boxes);
        RTN_CHECK_LAUNCH(h, "label_boxes_kernel");
        label_finish_kernel<<<dim3(rtn_blocks_for(max_cap, CCA_PIX_THREADS), (unsigned)n), dim3(CCA_PIX_THREADS), 0, h->stream>>>(t, counts, boxes);
        RTN_CHECK_LAUNCH(h, "label_finish_kernel");
    }
    // the counts come back: an image with more components than its capacity is an error, never a silent cut
    std::vector<int32_t> got((size_t)n);
    RTN_HIP(h, hipMemcpyAsync(got.data(), counts, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    RTN_HIP(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < n; ++i)
        if (got[i] > capacity[i])
            return rtn_fail(h, RTN_EINVAL, "rtn_cca_label: image %d has %d components, capacity %d (counts holds the true numbers)", i, got[i], capacity[i]);
    return RTN_OK;
}

extern "C" int rtn_cca_paint(rtn_handle_t h, int n, uint8_t* const* pages, const int32_t* heights, const int32_t* widths,
                             const int32_t* channels, int n_boxes, const int32_t* box_page, const int32_t* boxes, int mode,
                             void* workspace, size_t workspace_bytes) {
    if (!h) return RTN_EINVAL;
    std::vector<CPaintPage> pp;
    std::vector<CRect> rects;
    RTN_PLAN(h, "rtn_cca_paint", cca_plan_paint(n, pages, heights, widths, channels, n_boxes, box_page, boxes, mode, &pp, &rects));
    if (rects.empty()) return RTN_OK;
    rtn_stage st;
    const Layout l = layout_of(st, n, n_boxes, Sizes{});                       // the tables alone
    st.put(l.rows, pp);
    st.put(l.rects, rects);
    if (const int rc = st.commit(h, "rtn_cca_paint", workspace, workspace_bytes)) return rc;
    int64_t max_area = 1;
    for (const CRect& r : rects) max_area = std::max(max_area, (int64_t)(r.x1 - r.x0) * (r.y1 - r.y0));
    const unsigned slices = std::min(rtn_blocks_for(max_area, CCA_PIX_THREADS), 1024u);
    paint_kernel<<<dim3((unsigned)rects.size(), slices), dim3(CCA_PIX_THREADS), 0, h->stream>>>(st.at<const CPaintPage>(l.rows), st.at<const CRect>(l.rects), mode);
    RTN_CHECK_LAUNCH(h, "paint_kernel");
    return RTN_OK;
}

// ---- the CPU twins: host pointers, no handle, the bodies of rtn_cca.h --------------------------------------------------------------
extern "C" int rtn_cca_lines_mask_host(int n, const uint8_t* const* pages, const int32_t* heights, const int32_t* widths,
                                       const int32_t* channels, const int64_t* offsets, uint8_t* horizontal, uint8_t* vertical,
                                       size_t mask_bytes, uint8_t* bw) {
    std::vector<CPage> pg;
    RTN_PLAN(nullptr, "rtn_cca_lines_mask_host", cca_plan_pages(n, pages, heights, widths, channels, offsets, mask_bytes, &pg));
    if (n && (!horizontal || !vertical)) return rtn_fail_host(nullptr, RTN_EINVAL, "rtn_cca_lines_mask_host: the two mask buffers expected");
    for (const CPage& p : pg) cca_lines_mask_page(p, horizontal + p.off, vertical + p.off, bw ? bw + p.off : nullptr);
    return RTN_OK;
}

extern "C" int rtn_cca_text_mask_host(int n, const uint8_t* const* pages, const int32_t* heights, const int32_t* widths,
                                      const int32_t* channels, const int64_t* offsets, uint8_t* closed, size_t mask_bytes,
                                      uint8_t* stages) {
    std::vector<CPage> pg;
    RTN_PLAN(nullptr, "rtn_cca_text_mask_host", cca_plan_pages(n, pages, heights, widths, channels, offsets, mask_bytes, &pg));
    if (n && !closed) return rtn_fail_host(nullptr, RTN_EINVAL, "rtn_cca_text_mask_host: the mask buffer expected");
    for (const CPage& p : pg) cca_text_mask_page(p, closed + p.off, stages ? stages + 4 * p.off : nullptr);
    return RTN_OK;
}

extern "C" int rtn_cca_label_host(int n, const uint8_t* const* images, const int32_t* heights, const int32_t* widths, int external_only,
                                  const int32_t* capacity, const int64_t* box_offsets, int32_t* counts, int32_t* boxes,
                                  size_t boxes_bytes) {
    std::vector<CLab> im;
    RTN_PLAN(nullptr, "rtn_cca_label_host", cca_plan_label(n, images, heights, widths, capacity, box_offsets, counts, boxes, boxes_bytes, &im));
    int over = -1;
    for (int i = 0; i < n; ++i) {
        counts[i] = (int32_t)cca_label_image(im[i].img, im[i].h, im[i].w, external_only, im[i].cap, boxes + 4 * im[i].box_off);
        if (counts[i] > im[i].cap && over < 0) over = i;
    }
    if (over >= 0)
        return rtn_fail_host(nullptr, RTN_EINVAL, "rtn_cca_label_host: image %d has %d components, capacity %d (counts holds the true numbers)",
                             over, counts[over], capacity[over]);
    return RTN_OK;
}

extern "C" int rtn_cca_paint_host(int n, uint8_t* const* pages, const int32_t* heights, const int32_t* widths, const int32_t* channels,
                                  int n_boxes, const int32_t* box_page, const int32_t* boxes, int mode) {
    std::vector<CPaintPage> pp;
    std::vector<CRect> rects;
    RTN_PLAN(nullptr, "rtn_cca_paint_host", cca_plan_paint(n, pages, heights, widths, channels, n_boxes, box_page, boxes, mode, &pp, &rects));
    for (const CRect& r : rects)
        for (int y = r.y0; y < r.y1; ++y)
            for (int x = r.x0; x < r.x1; ++x) cca_paint_pixel(pp[r.page], mode, y, x);
    return RTN_OK;
}
