// rtn_jpeg.hip — baseline JPEG pages decoded on the device, bit-identical to libjpeg-turbo's default decode (what Pillow's
// read_image_bgr gives): ISLOW IDCT, "fancy" upsampling, ycc_rgb_convert.
//
// Host: rtn_jpeg_inspect parses one file (every read bounds-checked) into a packed blob: header, Huffman lookup tables, quantisation
// tables, restart-segment bit offsets and the entropy-coded bytes with 0xFF00 stuffing and the RST markers removed.
// Device, three kernels per batch (each page's work stays inside its own workgroups; no workgroup waits on another):
//   1. jpeg_huffman_kernel: one workgroup per page.  Thread t owns bits [t L, (t+1) L) of the stream.  Self-synchronising decode:
//      pass 0 starts every thread from a guessed state (its first bit, block 0 of an MCU, DC next); pass k starts thread t from
//      thread t-1's exit state of pass k-1, until no exit state changes (a workgroup-uniform flag after a barrier; at most T + 1
//      passes).  Restart segments start from a known state.  A segmented scan over the threads gives each one its first block
//      ordinal in its segment and its DC predictors; a last pass writes the de-zigzagged coefficients with absolute DC values.
//   2. jpeg_idct_kernel: one thread per 8x8 block, dequantisation + jpeg_idct_islow into component planes.
//   3. jpeg_color_kernel: one thread per pixel, h2v1 / h2v2 fancy (or box) upsampling + ycc_rgb_convert into the B,G,R page.
// A page whose stream breaks JPEG's rules, or whose IDCT leaves the range where libjpeg-turbo's C and SIMD IDCTs agree, gets a
// non-zero status word: the caller decodes that page on the host.
// The blob layout, the inspector and every decode function live in rtn_jpeg_decode.h, which a plain C++ compiler also compiles:
// rtn_jpeg_decode_host runs the same functions for any number of virtual threads on the CPU, behind a bounds-checking context.
#include "rtn_codec_launch.h"
#include "rtn_jpeg_decode.h"

namespace {

struct JBatch {
    int n, maxblocks, maxpix, pad_;
    long long blob_off[RTN_CODEC_BATCH];
    long long ws_off[RTN_CODEC_BATCH];
    unsigned char* out[RTN_CODEC_BATCH];
};

// the kernels' memory context (rtn_jpeg_decode.h): plain loads and stores on the blob and on the page's workspace
struct JDevMem {
    const uint32_t* w;                         // the entropy-coded bytes
    const int32_t* sg;                         // nseg + 1 bit offsets
    uint8_t* base;                             // the page's workspace: coefficients, then the planes at hd->plane_off
    const JHdr* hd;
    __device__ inline uint32_t word(int i) const { return w[i]; }
    __device__ inline int seg(int i) const { return sg[i]; }
    __device__ inline void zero(long long b) const {
        int4* z = reinterpret_cast<int4*>(reinterpret_cast<int16_t*>(base) + b * 64);
        for (int i = 0; i < 8; ++i) z[i] = make_int4(0, 0, 0, 0);
    }
    __device__ inline void coef(long long b, int i, int v) const { reinterpret_cast<int16_t*>(base)[b * 64 + i] = (int16_t)v; }
    __device__ inline const int16_t* block(long long b) const { return reinterpret_cast<const int16_t*>(base) + b * 64; }
    __device__ inline void row8(int c, long long off, uint32_t lo, uint32_t hi) const {
        *reinterpret_cast<uint2*>(base + hd->plane_off[c] + off) = make_uint2(lo, hi);
    }
    __device__ inline int px(int c, long long off) const { return base[hd->plane_off[c] + off]; }
};

__device__ inline JDevMem dev_mem(const uint8_t* blob, const uint8_t* ws_page) {
    const JHdr* hd = reinterpret_cast<const JHdr*>(blob);
    return JDevMem{reinterpret_cast<const uint32_t*>(blob + hd->off_data), reinterpret_cast<const int32_t*>(blob + hd->off_seg),
                   const_cast<uint8_t*>(ws_page), hd};
}

// ---- kernels --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(JPG_THREADS) void jpeg_huffman_kernel(const uint8_t* __restrict__ blobs, uint8_t* __restrict__ ws,
                                                                   int32_t* __restrict__ status, JBatch bt) {
    __shared__ JHuff tabs[8];
    __shared__ int ex_p[JPG_THREADS], ex_bk[JPG_THREADS];
    __shared__ int sc[5][JPG_THREADS];
    __shared__ int chg[2], bad;
    const int page = blockIdx.x, t = threadIdx.x;
    if (page >= bt.n) return;
    const uint8_t* blob = blobs + bt.blob_off[page];
    {
        const int4* src = reinterpret_cast<const int4*>(blob + JB_HUFF);
        int4* dst = reinterpret_cast<int4*>(tabs);
        for (int i = t; i < (int)(sizeof(tabs) / 16); i += JPG_THREADS) dst[i] = src[i];
    }
    if (t == 0) { chg[0] = 0; chg[1] = 0; bad = 0; }
    __syncthreads();
    JDevMem m = dev_mem(blob, ws + bt.ws_off[page]);
    const JPage pg = make_page(m.hd, blob + m.hd->off_data, m.sg, tabs);
    const int total = pg.hd->total_bits;
    const int L = jpeg_range_bits(total, JPG_THREADS);
    const int rstart = min(t * L, total), rend = min(rstart + L, total);

    JState entry = {rstart, 0, 0};
    JSync res;
    for (int pass = 0; pass <= JPG_THREADS; ++pass) {
        if (pass > 0 && t > 0) { entry.p = ex_p[t - 1]; entry.b = ex_bk[t - 1] >> 8; entry.k = ex_bk[t - 1] & 255; }
        __syncthreads();
        if (t == 0) chg[(pass + 1) & 1] = 0;
        res = jpeg_sync_range(pg, m, entry, rend);
        const int bk = (res.exit.b << 8) | res.exit.k;
        if (pass > 0 && (res.exit.p != ex_p[t] || bk != ex_bk[t])) chg[pass & 1] = 1;
        ex_p[t] = res.exit.p;
        ex_bk[t] = bk;
        __syncthreads();
        if (pass > 0 && chg[pass & 1] == 0) break;
    }
    // segmented inclusive scan over threads of (reset, blocks, DC sums)
    int f = res.reset, v0 = res.cnt, v1 = res.dc[0], v2 = res.dc[1], v3 = res.dc[2];
    for (int d = 1; d < JPG_THREADS; d <<= 1) {
        sc[0][t] = f; sc[1][t] = v0; sc[2][t] = v1; sc[3][t] = v2; sc[4][t] = v3;
        __syncthreads();
        if (t >= d && !f) {
            f = sc[0][t - d]; v0 += sc[1][t - d]; v1 += sc[2][t - d]; v2 += sc[3][t - d]; v3 += sc[4][t - d];
        }
        __syncthreads();
    }
    sc[0][t] = f; sc[1][t] = v0; sc[2][t] = v1; sc[3][t] = v2; sc[4][t] = v3;
    __syncthreads();
    int ord = 0, p0 = 0, p1 = 0, p2 = 0;
    if (t > 0) { ord = sc[1][t - 1]; p0 = sc[2][t - 1]; p1 = sc[3][t - 1]; p2 = sc[4][t - 1]; }
    const int err = jpeg_write_range(pg, m, entry, rend, ord, p0, p1, p2);
    if (err) bad = err;
    __syncthreads();
    if (t == 0) status[page] = bad;
}

__global__ __launch_bounds__(256) void jpeg_idct_kernel(const uint8_t* __restrict__ blobs, uint8_t* __restrict__ ws,
                                                        int32_t* __restrict__ status, JBatch bt) {
    const int page = blockIdx.y;
    if (page >= bt.n) return;
    const uint8_t* blob = blobs + bt.blob_off[page];
    const JHdr* hd = reinterpret_cast<const JHdr*>(blob);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= hd->total_blocks || status[page] != 0) return;
    int c, ld;
    long long off;
    jpeg_block_place(hd, i, &c, &off, &ld);
    JDevMem m = dev_mem(blob, ws + bt.ws_off[page]);
    const uint16_t* q = reinterpret_cast<const uint16_t*>(blob + hd->off_quant) + 64 * (hd->tq[c] & 3);
    if (!idct_islow(m, i, q, c, off, ld)) status[page] = 2;
}

__global__ __launch_bounds__(256) void jpeg_color_kernel(const uint8_t* __restrict__ blobs, const uint8_t* __restrict__ ws,
                                                         const int32_t* __restrict__ status, JBatch bt) {
    const int page = blockIdx.y;
    if (page >= bt.n) return;
    const uint8_t* blob = blobs + bt.blob_off[page];
    const JHdr* hd = reinterpret_cast<const JHdr*>(blob);
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int W = hd->W, H = hd->H;
    if (i >= (long long)W * H || status[page] != 0) return;
    const int y = (int)(i / W), x = (int)(i - (long long)y * W);
    const JDevMem m = dev_mem(blob, ws + bt.ws_off[page]);
    jpeg_pixel(hd, m, x, y, bt.out[page] + i * 3);
}

thread_local JHostStats g_host_stats = {0, 0};

// off >= 0: the callers (rtn_codec_blobs, and the walk behind it) have looked at the sign
const JHdr* jd_blob(const void* host_blobs, int64_t off) {
    const uint8_t* b = static_cast<const uint8_t*>(host_blobs) + off;
    return jpeg_blob_ok(b) ? reinterpret_cast<const JHdr*>(b) : nullptr;
}

}  // namespace

// rtn_jpeg_inspect: see include/rtn.h
extern "C" int rtn_jpeg_inspect(rtn_handle_t h, const void* file, size_t file_bytes, rtn_jpeg_info_t* info, void* blob_out,
                                size_t blob_capacity) {
    return rtn_codec_inspect(h, "rtn_jpeg_inspect", file, info, false, [&](char* why, size_t bytes) {
        return jpeg_inspect(static_cast<const uint8_t*>(file), file_bytes, info, blob_out, blob_capacity, why, bytes);
    });
}

// rtn_jpeg_decode_host, rtn_jpeg_decode_host_counters: see include/rtn.h
extern "C" int rtn_jpeg_decode_host(const void* blob, int threads, uint8_t* out_bgr, size_t out_bytes, int32_t* status) {
    if (!blob || !out_bgr || !status) { rtn_set_host_error("rtn_jpeg_decode_host: NULL argument"); return RTN_EINVAL; }
    const char* why = "";
    g_host_stats = JHostStats{0, 0};
    const int rc = jpeg_decode_host(blob, threads, out_bgr, out_bytes, status, &why, &g_host_stats);
    if (rc != RTN_OK) rtn_set_host_error(why);
    return rc;
}

extern "C" void rtn_jpeg_decode_host_counters(int32_t* passes, int32_t* busy_threads) {
    if (passes) *passes = g_host_stats.passes;
    if (busy_threads) *busy_threads = g_host_stats.busy;
}

extern "C" size_t rtn_jpeg_workspace_bytes(int n, const void* host_blobs, const int64_t* offsets) {
    return rtn_codec_blob_bytes(n, host_blobs, offsets, jd_blob);
}

extern "C" int rtn_jpeg_decode(rtn_handle_t h, int n, const void* host_blobs, const void* dev_blobs, const int64_t* offsets,
                               uint8_t* const* pages, int32_t* status, void* workspace, size_t workspace_bytes) {
    const int rc = rtn_decode_check(h, "rtn_jpeg_decode", "rtn_jpeg_inspect", n, host_blobs, dev_blobs, offsets, pages, status, workspace,
                                    workspace_bytes, jd_blob, rtn_codec_no_extra);
    if (rc != RTN_CODEC_GO) return rc;
    const uint8_t* db = static_cast<const uint8_t*>(dev_blobs);
    uint8_t* wsp = static_cast<uint8_t*>(workspace);
    long long maxpix = 0;
    int maxblocks = 0;
    return rtn_codec_walk<JBatch>(n,
        [&](JBatch& bt, int k, int i, long long ws) {
            const JHdr* hd = jd_blob(host_blobs, offsets[i]);
            if (k == 0) maxpix = 0, maxblocks = 0;
            bt.blob_off[k] = offsets[i];
            bt.ws_off[k] = ws;
            bt.out[k] = pages[i];
            maxblocks = hd->total_blocks > maxblocks ? hd->total_blocks : maxblocks;
            maxpix = (long long)hd->W * hd->H > maxpix ? (long long)hd->W * hd->H : maxpix;
            return (long long)hd->ws_bytes;
        },
        [&](const JBatch& bt, int i0) {
            jpeg_huffman_kernel<<<bt.n, JPG_THREADS, 0, h->stream>>>(db, wsp, status + i0, bt);
            RTN_CHECK_LAUNCH(h, "jpeg_huffman_kernel");
            jpeg_idct_kernel<<<dim3((maxblocks + 255) / 256, bt.n), 256, 0, h->stream>>>(db, wsp, status + i0, bt);
            RTN_CHECK_LAUNCH(h, "jpeg_idct_kernel");
            jpeg_color_kernel<<<dim3((unsigned)((maxpix + 255) / 256), bt.n), 256, 0, h->stream>>>(db, wsp, status + i0, bt);
            RTN_CHECK_LAUNCH(h, "jpeg_color_kernel");
            return RTN_OK;
        });
}
