// rtn_resize_u8.hip — cv2.resize(INTER_CUBIC) of 8-bit pages on the device (interpolateImages,
// DetectTablesUtils.py:296-316): one launch for a whole batch of pages of different sizes, factors and channel counts.
//
// A workgroup of 256 threads owns a tile of RSZ_TILE_ROWS destination rows by RSZ_TILE_BYTES destination bytes; the flat list of
// the tiles of all pages is the grid, a workgroup finds its page by bisection of the page table.  Threads 0 .. 31 put the taps of
// the tile's rows into LDS; thread t keeps the taps of tile column rsz_slot_column(t) in registers.
//   tiled path   (inv_y <= 1) the horizontal sums of the source rows the tile reads go into LDS once, int32, a row of 256 slots
//                per source row; then a lane of the vertical pass takes 16 consecutive destination bytes of one row: four 16-byte
//                LDS reads per tap (consecutive dwords across a group of lanes: no bank conflict), 64 multiply-adds, one store.
//   direct path  (a tile would need more source rows than the LDS image holds) thread t computes the samples of its column from
//                their 16 taps, row by row, into a byte image of the tile in LDS, which the same store walk then writes.
// The store walk: a lane's 16 bytes go as one 16-byte store where their address is 16-byte aligned and the row holds all of them,
// else as 8-byte, 4-byte or single-byte stores, each guarded by the end of the row.  A page has no row padding, so the alignment
// changes from row to row.  The per-sample rules are the text the CPU twin runs (rtn_resize_u8.h).
#include <algorithm>
#include <vector>
#include "rtn_page_launch.h"
#include "rtn_resize_u8.h"

namespace {

// the pages are global memory: said in the pointer's type, so that the loads and stores are not the slower generic ones
typedef __attribute__((address_space(1))) const uint8_t* SrcPtr;
typedef __attribute__((address_space(1))) uint8_t* DstPtr;
typedef uint32_t U32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t U32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(1))) U32x4 G16;
typedef __attribute__((address_space(1))) U32x2 G8;
typedef __attribute__((address_space(1))) uint32_t G4;

// 16 bytes of a destination row at byte `bx` of `row_bytes`: the widest stores the address allows, nothing past the end of the row
__device__ inline void store_chunk(DstPtr row, int64_t bx, int64_t row_bytes, const uint32_t* w) {
    DstPtr q = row + bx;
    const int64_t left = row_bytes - bx;
    if (left <= 0) return;
    const uintptr_t a = (uintptr_t)q;
    if (left >= RSZ_CHUNK && (a & 15) == 0) {
        *reinterpret_cast<G16*>(q) = U32x4{w[0], w[1], w[2], w[3]};
    } else if (left >= RSZ_CHUNK && (a & 7) == 0) {
        reinterpret_cast<G8*>(q)[0] = U32x2{w[0], w[1]};
        reinterpret_cast<G8*>(q)[1] = U32x2{w[2], w[3]};
    } else if (left >= RSZ_CHUNK && (a & 3) == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) reinterpret_cast<G4*>(q)[k] = w[k];
    } else {
        const int m = left < RSZ_CHUNK ? (int)left : RSZ_CHUNK;
#pragma unroll
        for (int k = 0; k < RSZ_CHUNK; ++k)
            if (k < m) q[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
    }
}

// One sample as a dword for packing.  The empty asm keeps the compiler from fusing the shift-and-clip of two neighbouring samples into
// v_ashr_pk_u8_i32: it takes the upper half of that instruction's result for zero, while gfx950 leaves the upper half of the
// destination register as it was, so bytes 2 and 3 of a packed word came out or-ed with bits of a vertical sum.
__device__ inline uint32_t sample_word(int32_t v) {
    uint32_t b = rsz_output(v);
    asm volatile("" : "+v"(b));
    return b;
}

constexpr int LANES_PER_ROW = RSZ_TILE_BYTES / RSZ_CHUNK;       // 16
constexpr int ROWS_PER_PASS = RSZ_THREADS / LANES_PER_ROW;      // 16

__global__ __launch_bounds__(RSZ_THREADS) void resize_u8_kernel(const RszPage* pages, int n) {
    __shared__ __attribute__((aligned(16))) int32_t hbuf[RSZ_LDS_ROWS * RSZ_TILE_BYTES];
    __shared__ int32_t ridx[RSZ_TILE_ROWS][4], rcoef[RSZ_TILE_ROWS][4];
    const int tid = threadIdx.x;
    const int64_t tile = blockIdx.x;
    const RszPage p = pages[rsz_page_of_tile(pages, n, tile)];
    const int64_t local = tile - p.tile_begin;
    const int ty = (int)(local / p.tiles_x), tx = (int)(local - (int64_t)ty * p.tiles_x);
    const int y0 = ty * RSZ_TILE_ROWS;
    const int rows = p.ho - y0 < RSZ_TILE_ROWS ? p.ho - y0 : RSZ_TILE_ROWS;          // >= 1: the tile exists
    const int64_t x0 = (int64_t)tx * RSZ_TILE_BYTES;
    const int64_t row_bytes = (int64_t)p.wo * p.c, src_row_bytes = (int64_t)p.w * p.c;
    const SrcPtr src = (SrcPtr)p.src;
    const DstPtr dst = (DstPtr)p.dst;
    if (tid < rows) {
        RszTaps t;
        rsz_taps(y0 + tid, p.inv_y, p.h, &t);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            ridx[tid][k] = t.idx[k];
            rcoef[tid][k] = t.coef[k];
        }
    }
    RszColumn col;
    rsz_column(p, x0 + rsz_slot_column(tid), &col);
    __syncthreads();
    const int first = ridx[0][0];
    const int count = ridx[rows - 1][3] - first + 1;
    const bool tiled = p.path == RSZ_PATH_TILED && count <= RSZ_LDS_ROWS;             // uniform: the barriers below are reached by all
    if (tiled) {
        SrcPtr srow = src + (int64_t)first * src_row_bytes;
#pragma unroll 4
        for (int r = 0; r < count; ++r, srow += src_row_bytes) hbuf[r * RSZ_TILE_BYTES + tid] = rsz_horizontal(srow, col);
    } else {
        uint8_t* obuf = reinterpret_cast<uint8_t*>(hbuf);
        const int c = rsz_slot_column(tid);
        for (int r = 0; r < rows; ++r) {
            int32_t v = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) v += rsz_mul(rsz_horizontal(src + (int64_t)ridx[r][k] * src_row_bytes, col), rcoef[r][k]);
            obuf[r * RSZ_TILE_BYTES + c] = rsz_output(v);
        }
    }
    __syncthreads();
    const int l = tid % LANES_PER_ROW;
    for (int r = tid / LANES_PER_ROW; r < rows; r += ROWS_PER_PASS) {
        uint32_t w[4];
        if (tiled) {
            int32_t acc[RSZ_CHUNK];
#pragma unroll
            for (int e = 0; e < RSZ_CHUNK; ++e) acc[e] = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int32_t* hrow = hbuf + (ridx[r][k] - first) * RSZ_TILE_BYTES + 4 * l;
                const int32_t b = rcoef[r][k];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int4 hv = *reinterpret_cast<const int4*>(hrow + 64 * q);
                    acc[4 * q] += rsz_mul(hv.x, b);
                    acc[4 * q + 1] += rsz_mul(hv.y, b);
                    acc[4 * q + 2] += rsz_mul(hv.z, b);
                    acc[4 * q + 3] += rsz_mul(hv.w, b);
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
                w[q] = sample_word(acc[4 * q]) | sample_word(acc[4 * q + 1]) << 8 | sample_word(acc[4 * q + 2]) << 16 | sample_word(acc[4 * q + 3]) << 24;
        } else {
            const uint4 v = *reinterpret_cast<const uint4*>(reinterpret_cast<const uint8_t*>(hbuf) + r * RSZ_TILE_BYTES + RSZ_CHUNK * l);
            w[0] = v.x;
            w[1] = v.y;
            w[2] = v.z;
            w[3] = v.w;
        }
        store_chunk(dst + (int64_t)(y0 + r) * row_bytes, x0 + RSZ_CHUNK * l, row_bytes, w);
    }
}

int forced_path() {
    rtn_env_sync();
    const int v = rtn_env_int("RTN_RESIZE_U8_PATH", 0);          // 0: by the factor, 1: tiled wherever it fits, 2: direct
    return v == RSZ_PATH_TILED || v == RSZ_PATH_DIRECT ? v : 0;
}

// the workspace: the page table alone -> its offset
size_t page_table_room(rtn_stage& st, int n) { return st.reserve((int64_t)n * sizeof(RszPage)); }

}  // namespace

// rtn_resize_u8_*: see include/rtn.h
extern "C" int rtn_resize_u8_tile(int32_t* rows, int32_t* bytes) {
    if (!rows || !bytes) return RTN_EINVAL;
    *rows = RSZ_TILE_ROWS;
    *bytes = RSZ_TILE_BYTES;
    return RTN_OK;
}

extern "C" int rtn_resize_u8_path(double inv_y) {
    if (!(inv_y - inv_y == 0.0) || !(inv_y > 0.0)) return RTN_EINVAL;
    return rsz_choose_path(forced_path(), inv_y);
}

extern "C" size_t rtn_resize_u8_workspace_bytes(int n) {
    if (n < 1 || n > RSZ_MAX_PAGES) return 0;
    rtn_stage st;
    page_table_room(st, n);
    return st.bytes();
}

extern "C" int rtn_resize_u8(rtn_handle_t h, int n, const uint8_t* const* pages, const int32_t* heights, const int32_t* widths,
                             const int32_t* channels, const int32_t* out_heights, const int32_t* out_widths, const double* inv_x,
                             const double* inv_y, uint8_t* const* outs, void* workspace, size_t workspace_bytes) {
    if (!h) return RTN_EINVAL;
    std::vector<RszPage> table((size_t)(n > 0 && n <= RSZ_MAX_PAGES ? n : 0));
    int64_t tiles = 0;
    RTN_PLAN(h, "rtn_resize_u8", rsz_plan(n, pages, heights, widths, channels, out_heights, out_widths, inv_x, inv_y, outs, forced_path(), table.data(), &tiles));
    if (n == 0) return RTN_OK;
    rtn_stage st;
    const size_t off = page_table_room(st, n);
    st.put(off, table);
    if (const int rc = st.commit(h, "rtn_resize_u8", workspace, workspace_bytes)) return rc;
    resize_u8_kernel<<<dim3((unsigned)tiles), dim3(RSZ_THREADS), 0, h->stream>>>(st.at<const RszPage>(off), n);
    RTN_CHECK_LAUNCH(h, "resize_u8_kernel");
    return RTN_OK;
}

// ---- the CPU twin: host pointers, no handle; the walk is rsz_host (rtn_resize_u8.h) -------------------------------------------------
extern "C" int rtn_resize_u8_host(int n, const uint8_t* const* pages, const int32_t* heights, const int32_t* widths, const int32_t* channels,
                                  const int32_t* out_heights, const int32_t* out_widths, const double* inv_x, const double* inv_y,
                                  uint8_t* const* outs) {
    RTN_PLAN(nullptr, "rtn_resize_u8_host", rsz_host(n, pages, heights, widths, channels, out_heights, out_widths, inv_x, inv_y, outs, forced_path()));
    return RTN_OK;
}
