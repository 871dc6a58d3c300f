// rtn_compose.hip — decoded images onto their pages on the device: the strips, turned and mirrored images of scanned
// PDF pages, for a whole batch of pages of different sizes.  The per-pixel rule, the argument checks and the tables are the text the
// CPU twin runs (rtn_compose.h).  One call queues, on the handle's stream and with no host round trip between them:
//   compose_fill     over the pages their items leave uncovered: a workgroup owns CMP_FILL_ROWS rows of a page, a lane a byte of a
//                    row at a step; a byte of a pixel that no item of the page covers becomes 255, every other byte is left alone
//   compose          over the 64 x 64 pixel tiles of all items: codes 1 .. 4 copy runs of a source row to runs of a page row (a
//                    mirrored one pixel by pixel backwards); codes 5 .. 8 read the tile's source rows, runs of up to 192 consecutive
//                    bytes, into LDS and write the page rows out of its columns, so neither side walks a column of HBM
// A lane moves one byte at a step and the lanes of a wave take consecutive bytes: a wave reads and writes 64 consecutive bytes at
// any alignment (a pixel is 3 bytes, a page rectangle starts anywhere).  Every byte of a page has one writer in one of the two
// launches and nothing is accumulated: a second call on the same buffers gives the same bytes.
#include <vector>
#include "rtn_page_launch.h"
#include "rtn_compose.h"

namespace {

constexpr int WAVES = CMP_THREADS / 64;

__global__ __launch_bounds__(CMP_THREADS) void compose_fill_kernel(const CmpFill* fills, int n_fills, const CmpItem* items) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t tile = blockIdx.x;
    const CmpFill f = fills[cmp_of_tile(fills, n_fills, tile)];
    const CmpItem* mine = items + f.item_first;
    const int y0 = (int)(tile - f.tile_begin) * CMP_FILL_ROWS;
    const int y1 = y0 + CMP_FILL_ROWS < f.h ? y0 + CMP_FILL_ROWS : f.h;
    const int row_bytes = f.w * 3;
    for (int y = y0 + wave; y < y1; y += WAVES) {
        uint8_t* row = f.dst + (int64_t)y * row_bytes;
        for (int j = lane; j < row_bytes; j += 64) {
            const int x = j / 3;
            bool covered = false;
            for (int k = 0; k < f.item_count; ++k) {
                const CmpItem& e = mine[k];
                covered = covered || (y >= e.y && y < e.y + e.ch && x >= e.x && x < e.x + e.cw);
            }
            if (!covered) row[j] = 255;
        }
    }
}

__global__ __launch_bounds__(CMP_THREADS) void compose_kernel(const CmpItem* items, int n_items) {
    __shared__ uint8_t lds[CMP_TILE * CMP_PITCH];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t tile = blockIdx.x;
    const CmpItem e = items[cmp_of_tile(items, n_items, tile)];
    const int t = (int)(tile - e.tile_begin);
    const int y0 = t / e.tiles_x * CMP_TILE, x0 = t % e.tiles_x * CMP_TILE;          // of the tile in the destination rectangle
    const int th = e.ch - y0 < CMP_TILE ? e.ch - y0 : CMP_TILE, tw = e.cw - x0 < CMP_TILE ? e.cw - x0 : CMP_TILE;
    const int oy0 = e.cy + y0, ox0 = e.cx + x0;                                     // of the tile in the oriented image
    const uint8_t flip = e.invert ? 255 : 0;
    const bool fy = cmp_flip_y(e.orientation), fx = cmp_flip_x(e.orientation);
    uint8_t* dst = e.dst + ((int64_t)(e.y + y0) * e.page_w + e.x + x0) * 3;
    const int64_t dst_pitch = (int64_t)e.page_w * 3, src_pitch = (int64_t)e.w * 3;
    if (!cmp_transposed(e.orientation)) {
        for (int yy = wave; yy < th; yy += WAVES) {
            const int sy = fy ? e.h - 1 - (oy0 + yy) : oy0 + yy;
            const uint8_t* srow = e.src + sy * src_pitch;
            uint8_t* drow = dst + yy * dst_pitch;
            for (int j = lane; j < tw * 3; j += 64) {
                const int px = j / 3, c = j - 3 * px;
                const int sx = fx ? e.w - 1 - (ox0 + px) : ox0 + px;
                drow[j] = srow[sx * 3 + c] ^ flip;
            }
        }
        return;
    }
    // transposed: page column xx of the tile is a source row, page rows oy0 .. oy0 + th - 1 are th consecutive source columns from lo
    const int lo = fx ? e.w - 1 - (oy0 + th - 1) : oy0;
    for (int xx = wave; xx < tw; xx += WAVES) {
        const int sy = fy ? e.h - 1 - (ox0 + xx) : ox0 + xx;
        const uint8_t* srow = e.src + sy * src_pitch + (int64_t)lo * 3;
        for (int j = lane; j < th * 3; j += 64) lds[xx * CMP_PITCH + j] = srow[j];
    }
    __syncthreads();
    for (int yy = wave; yy < th; yy += WAVES) {
        const int k = fx ? th - 1 - yy : yy;
        uint8_t* drow = dst + yy * dst_pitch;
        for (int j = lane; j < tw * 3; j += 64) {
            const int px = j / 3, c = j - 3 * px;
            drow[j] = lds[px * CMP_PITCH + k * 3 + c] ^ flip;
        }
    }
}

// the workspace: the item table, the fill table
struct Layout { size_t items, fills; };

Layout layout_of(rtn_stage& st, int n_items, int n_pages) {
    Layout l;
    l.items = st.reserve((int64_t)n_items * sizeof(CmpItem));
    l.fills = st.reserve((int64_t)n_pages * sizeof(CmpFill));
    return l;
}

}  // namespace

// rtn_page_compose*: see include/rtn.h
extern "C" size_t rtn_page_compose_workspace_bytes(int n_items, int n_pages) {
    if (n_items < 0 || n_items > CMP_MAX_ITEMS || n_pages < 0 || n_pages > CMP_MAX_PAGES) return 0;
    rtn_stage st;
    layout_of(st, n_items, n_pages);
    return st.bytes();
}

extern "C" int rtn_page_compose(rtn_handle_t h, int n_items, const rtn_compose_item_t* items, int n_pages, uint8_t* const* pages,
                                const int32_t* widths, const int32_t* heights, void* workspace, size_t workspace_bytes) {
    if (!h) return RTN_EINVAL;
    std::vector<CmpItem> table;
    std::vector<CmpFill> fills;
    int64_t tiles = 0, fill_tiles = 0;
    RTN_PLAN(h, "rtn_page_compose", cmp_plan(n_items, items, n_pages, pages, widths, heights, &table, &fills, &tiles, &fill_tiles));
    if (n_pages == 0) return RTN_OK;
    rtn_stage st;
    const Layout l = layout_of(st, n_items, n_pages);
    st.put(l.items, table);
    st.put(l.fills, fills);
    if (const int rc = st.commit(h, "rtn_page_compose", workspace, workspace_bytes)) return rc;
    const CmpItem* d_items = st.at<const CmpItem>(l.items);
    if (fill_tiles) {
        compose_fill_kernel<<<dim3((unsigned)fill_tiles), dim3(CMP_THREADS), 0, h->stream>>>(st.at<const CmpFill>(l.fills), (int)fills.size(), d_items);
        RTN_CHECK_LAUNCH(h, "compose_fill_kernel");
    }
    if (tiles) {
        compose_kernel<<<dim3((unsigned)tiles), dim3(CMP_THREADS), 0, h->stream>>>(d_items, n_items);
        RTN_CHECK_LAUNCH(h, "compose_kernel");
    }
    return RTN_OK;
}

// ---- the CPU twin: host pointers, no handle (rtn_compose.h) -----------------------------------------------------------------------------
extern "C" int rtn_page_compose_host(int n_items, const rtn_compose_item_t* items, int n_pages, uint8_t* const* pages, const int32_t* widths,
                                     const int32_t* heights) {
    RTN_PLAN(nullptr, "rtn_page_compose_host", cmp_host(n_items, items, n_pages, pages, widths, heights));
    return RTN_OK;
}
