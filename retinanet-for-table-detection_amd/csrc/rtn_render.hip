// rtn_render.hip — detection rendering on the device: every crop and annotated page of a batch in one launch.
//
// A workgroup of 256 threads owns one tile (RND_TILE_H rows x RND_TILE_W pixels) of one output image.  It finds its image by a binary
// search over the images' first tiles, collects into LDS, in drawing order, the page's operations whose outline bands or caption
// rectangle meet the tile (one operation per thread and pass, positions from wave ballots: no atomics), and then moves the tile in
// 16-byte destination units (render_unit of rtn_render.h): most tiles collect nothing and are a copy.  The rule, the operation test
// and the unit are the text the CPU twins run (rtn_render_host, rtn_render_tiles_host).
#include "rtn_page_launch.h"
#include "rtn_render.h"

namespace {

__global__ __launch_bounds__(RND_THREADS) void render_kernel(RTables t) {
    __shared__ uint16_t hits[RTN_RENDER_MAX_OPS];
    __shared__ int wave_hits[RND_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = blockIdx.x;
    int i = 0, last = t.n_out - 1;
    while (i < last) {                                          // the last image whose first tile is <= tile
        const int mid = (i + last + 1) >> 1;
        if (t.tile_begin[mid] <= tile) i = mid; else last = mid - 1;
    }
    const ROut o = t.outs[i];
    const RPage pg = t.pages[o.page];
    const RTile r = render_tile(o, tile - t.tile_begin[i]);

    const int nmax = o.n_outline > o.n_caption ? o.n_outline : o.n_caption;
    int nhit = 0;
    for (int base = 0; base < nmax; base += RND_THREADS) {
        const int j = base + tid;
        const bool hit = j < nmax && render_op_hits(t.ops[pg.op_begin + j], j < o.n_outline, j < o.n_caption, r.X0, r.Y0, r.X1, r.Y1,
                                                    t.lo, t.hi);
        const unsigned long long b = __ballot(hit);
        if (lane == 0) wave_hits[wave] = __popcll(b);
        __syncthreads();
        int pos = nhit, all = 0;
        for (int w = 0; w < RND_THREADS / 64; ++w) {
            if (w < wave) pos += wave_hits[w];
            all += wave_hits[w];
        }
        if (hit) hits[pos + __popcll(b & ((1ull << lane) - 1ull))] = (uint16_t)j;
        nhit += all;
        __syncthreads();
    }

    const int units = (r.r1 - r.r0) * RND_UNITS;
    for (int k = tid; k < units; k += RND_THREADS) {
        const int row = k / RND_UNITS;
        render_unit(t, pg, o, hits, nhit, r.r0 + row, r.b0, r.b1, k - row * RND_UNITS);
    }
}

// the workspace: the page, operation and output tables, then the first tile of every output
struct Layout { size_t pages, ops, outs, tiles; };
Layout render_ws_layout(rtn_stage& st, int n_pages, int n_ops, int n_out) {
    Layout l;
    l.pages = st.reserve((int64_t)n_pages * sizeof(RPage));
    l.ops = st.reserve((int64_t)n_ops * sizeof(ROp));
    l.outs = st.reserve((int64_t)n_out * sizeof(ROut));
    l.tiles = st.reserve(((int64_t)n_out + 1) * 4);
    return l;
}

int render_host_call(const RArgs& a, bool tiles, const char* name) {
    RPlan pl;
    char why[200];
    const int rc = render_plan(a, &pl, why, sizeof(why));
    if (rc) return rtn_fail_host(nullptr, rc, "%s: %s", name, why);
    if (a.n_out == 0) return RTN_OK;
    const RTables t = render_tables(pl, a);
    if (tiles) render_tiles_host(t); else render_pixels_host(t);
    return RTN_OK;
}

}  // namespace

// rtn_render_workspace_bytes / rtn_render_pages / rtn_render_host / rtn_render_tiles_host: see include/rtn.h
extern "C" size_t rtn_render_workspace_bytes(int n_pages, int n_ops, int n_out) {
    if (n_pages < 0 || n_ops < 0 || n_out < 0) return 0;
    rtn_stage st;
    render_ws_layout(st, n_pages, n_ops, n_out);
    return st.bytes();
}

extern "C" int rtn_render_pages(rtn_handle_t h, int n_pages, const uint8_t* const* pages, const int32_t* heights,
                                const int32_t* widths, const int32_t* op_begin, int n_ops, const int32_t* boxes,
                                const int32_t* captions, const int64_t* mask_bits, const int32_t* mask_pitch, const uint8_t* masks,
                                size_t mask_bytes, int n_out, const int32_t* out_page, const int32_t* out_rects,
                                const int32_t* out_outlines, const int32_t* out_captions, const int64_t* out_offsets, int thickness,
                                uint8_t* out, size_t out_bytes, void* workspace, size_t workspace_bytes) {
    if (!h) return RTN_EINVAL;
    const RArgs a{n_pages, pages, heights, widths, op_begin, n_ops, boxes, captions, mask_bits, mask_pitch, masks, mask_bytes,
                  n_out, out_page, out_rects, out_outlines, out_captions, out_offsets, thickness, out, out_bytes};
    RPlan pl;
    char why[200];
    const int rc = render_plan(a, &pl, why, sizeof(why));
    if (rc) return rtn_fail(h, rc, "rtn_render_pages: %s", why);
    if (n_out == 0) return RTN_OK;
    rtn_stage st;
    const Layout l = render_ws_layout(st, n_pages, n_ops, n_out);
    st.put(l.pages, pl.pages);
    st.put(l.ops, pl.ops);
    st.put(l.outs, pl.outs);
    st.put(l.tiles, pl.tile_begin);
    if (const int rc2 = st.commit(h, "rtn_render_pages", workspace, workspace_bytes)) return rc2;
    RTables t;
    t.pages = st.at<const RPage>(l.pages);
    t.ops = st.at<const ROp>(l.ops);
    t.outs = st.at<const ROut>(l.outs);
    t.tile_begin = st.at<const int32_t>(l.tiles);
    t.masks = masks;
    t.out = out;
    t.n_out = n_out; t.lo = pl.lo; t.hi = pl.hi;
    render_kernel<<<dim3((unsigned)pl.tile_begin[n_out]), dim3(RND_THREADS), 0, h->stream>>>(t);
    RTN_CHECK_LAUNCH(h, "render_kernel");
    return RTN_OK;
}

extern "C" int rtn_render_host(int n_pages, const uint8_t* const* pages, const int32_t* heights, const int32_t* widths,
                               const int32_t* op_begin, int n_ops, const int32_t* boxes, const int32_t* captions,
                               const int64_t* mask_bits, const int32_t* mask_pitch, const uint8_t* masks, size_t mask_bytes, int n_out,
                               const int32_t* out_page, const int32_t* out_rects, const int32_t* out_outlines,
                               const int32_t* out_captions, const int64_t* out_offsets, int thickness, uint8_t* out, size_t out_bytes) {
    return render_host_call(RArgs{n_pages, pages, heights, widths, op_begin, n_ops, boxes, captions, mask_bits, mask_pitch, masks,
                                  mask_bytes, n_out, out_page, out_rects, out_outlines, out_captions, out_offsets, thickness, out,
                                  out_bytes}, false, "rtn_render_host");
}

extern "C" int rtn_render_tiles_host(int n_pages, const uint8_t* const* pages, const int32_t* heights, const int32_t* widths,
                                     const int32_t* op_begin, int n_ops, const int32_t* boxes, const int32_t* captions,
                                     const int64_t* mask_bits, const int32_t* mask_pitch, const uint8_t* masks, size_t mask_bytes,
                                     int n_out, const int32_t* out_page, const int32_t* out_rects, const int32_t* out_outlines,
                                     const int32_t* out_captions, const int64_t* out_offsets, int thickness, uint8_t* out,
                                     size_t out_bytes) {
    return render_host_call(RArgs{n_pages, pages, heights, widths, op_begin, n_ops, boxes, captions, mask_bits, mask_pitch, masks,
                                  mask_bytes, n_out, out_page, out_rects, out_outlines, out_captions, out_offsets, thickness, out,
                                  out_bytes}, true, "rtn_render_tiles_host");
}
