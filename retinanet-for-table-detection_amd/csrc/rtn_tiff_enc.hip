// rtn_tiff_enc.hip — bilevel pages encoded as CCITT Group 4 (T.6) strip TIFFs on the device: the strips' bytes are those
// libtiff (Pillow's compression="group4") writes for the same bits, the file is what csrc/rtn_tiff.hip decodes with one wave per
// strip.  Decoding a row needs the decoded row above it; encoding has every row and its reference row in memory from the start, so
// every row of every page is coded on its own and only the bit positions need a prefix sum.  The row encoder, the size rules and the
// container writer are the text of csrc/rtn_tiff_encode.h, which the CPU twin (rtn_tiff_encode_host) runs as well.
//
//   1. tfe_pack_kernel     a wave per 64 pixels of a row: gray (skw_gray3), ink = gray < t, one ballot -> one 64-bit word of the page's
//                          bitmap in the workspace (te_bitmap_row: its layout goes with the row kernels')
//   2. tfe_rows_kernel<0>  a lane per row: te_row with the counting sink -> the row's bit length
//   3. tfe_scan_kernel     a workgroup per page: exclusive scan of the row lengths (64-bit), the strips' byte lengths
//                          ceil((row bits + 24) / 8) from it, their exclusive scan, the file's length -> out_bytes and status
//   4. tfe_zero_kernel     zeroes the file's words (its length is known now; the slot is not touched behind it)
//   5. tfe_rows_kernel<1>  the same row function with the word sink, at the row's final bit offset: the first and the last word of a
//                          row, which the rows before and behind it may share, are merged with atomicOr into the zeroed file (an OR
//                          does not depend on the order: the file is deterministic), the whole words between them are plain stores
//   6. tfe_finish_kernel   a workgroup per page: the 8-byte header and the IFD, then per strip its EOFB and its entries of the two arrays
// RTN_TIFF_ENC_WAVE_ROW=1 runs kernels 2 and 5 with a wave per row (lane 0 codes, as the Group 4 decoder does) instead of a lane per
// row: the variant tools/bench_encode_tiff.py measures against the default.  No workgroup waits on another.
#include "rtn_codec_launch.h"
#include "rtn_tiff_encode.h"

namespace {

constexpr int TE_THREADS = 256;
constexpr int TE_MAX_GRID = 4096;              // workgroups along x of the pack and zero launches: the rest is looped over

struct TEPage {
    const uint8_t* src;
    uint8_t* out;
    long long ws_off;
    long long bound;                           // te_bound of the page (<= its slot): a longer file is flagged, not written
    int32_t W, H, nc, t, rps, photometric, nstrips, pad_;
};
struct TEBatch {
    int n, row_major;                          // row_major: the bitmap's layout (te_bitmap_row)
    TEPage p[RTN_CODEC_BATCH];
};
static_assert(sizeof(TEBatch) <= 3072, "kernel arguments");

struct TEMeta {                                // written by the scan kernel
    unsigned long long file_bytes, data_bytes;
    uint32_t ok, pad_;
};

// The page's part of the workspace: the bitmap, a uint32 bit length per row, the H + 1 prefix sums, the nstrips + 1 strip offsets
// (behind byte 8 of the file), TEMeta.  Every part is 256-byte aligned.
struct TELayout { long long rowbits, prefix, strips, meta, total; };
__host__ __device__ inline long long te_align(long long v) { return (v + 255) & ~255ll; }
__host__ __device__ inline TELayout te_layout(int W, int H, int nstrips) {
    TELayout L;
    L.rowbits = te_align(8ll * te_words(W) * H);
    L.prefix = L.rowbits + te_align(4ll * H);
    L.strips = L.prefix + te_align(8ll * (H + 1));
    L.meta = L.strips + te_align(8ll * (nstrips + 1));
    L.total = L.meta + 256;
    return L;
}

// Row y of a page's bitmap (H rows of wpr words).  With a lane per row the lanes of a wave read the same word of 64 neighbouring rows
// at a time, so word k of row y lies at [k * H + y]; with a wave per row one lane walks along a row, so the rows are whole.
__device__ inline long long te_bitmap_at(int y, int k, int H, int wpr, bool row_major) {
    return row_major ? (long long)y * wpr + k : (long long)k * H + y;
}
__device__ inline TERow te_bitmap_row(const uint64_t* bm, int y, int H, int wpr, bool row_major) {
    return TERow{bm + te_bitmap_at(y, 0, H, wpr, row_major), row_major ? 1ll : (long long)H, false};
}

// ---- kernel 1: pixels -> bitmap ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TE_THREADS) void tfe_pack_kernel(uint8_t* ws, TEBatch bt) {
    const int page = blockIdx.y;
    if (page >= bt.n) return;
    const TEPage& pg = bt.p[page];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, W = pg.W, H = pg.H, nc = pg.nc, wpr = te_words(W);
    uint64_t* bm = reinterpret_cast<uint64_t*>(ws + pg.ws_off);
    const long long items = (long long)H * wpr;                        // the same trip count in every lane of a wave
    for (long long it = (long long)blockIdx.x * (TE_THREADS / 64) + wave; it < items; it += (long long)gridDim.x * (TE_THREADS / 64)) {
        const int y = (int)(it / wpr), k = (int)(it % wpr), x = 64 * k + lane;
        uint32_t bit = 0u;
        if (x < W) bit = te_bit(te_gray(pg.src + ((long long)y * W + x) * nc, nc), pg.t, pg.photometric);
        const unsigned long long w = __ballot((int)bit);
        if (lane == 0) bm[te_bitmap_at(y, k, H, wpr, bt.row_major != 0)] = w;
    }
}

// ---- kernels 2 and 5: rows ---------------------------------------------------------------------------------------------------------------------
struct TEWordSink {                            // MSB first into 32-bit words of the zeroed file (big-endian inside a word)
    uint32_t* words;
    long long w;                               // the word under construction
    uint64_t acc;                              // its n bits so far, in the low bits
    int n;
    bool first;                                // no word stored yet: the next one may be shared with the row before
    __device__ inline void put(uint32_t code, int len) {              // len <= 13, n < 32
        acc = acc << len | code;
        n += len;
        if (n >= 32) {
            n -= 32;
            const uint32_t v = __builtin_bswap32((uint32_t)(acc >> n));
            if (first) { atomicOr(words + w, v); first = false; }
            else words[w] = v;
            ++w;
            acc &= (1ull << n) - 1u;
        }
    }
    __device__ inline void flush() {                                   // the last word may be shared with what follows the row
        if (n) atomicOr(words + w, __builtin_bswap32((uint32_t)(acc << (32 - n))));
    }
};

template <bool EMIT, bool WAVE_ROW>
__global__ __launch_bounds__(WAVE_ROW ? TE_THREADS : 64) void tfe_rows_kernel(uint8_t* ws, TEBatch bt) {
    const int page = blockIdx.y;
    if (page >= bt.n) return;
    const TEPage& pg = bt.p[page];
    if (WAVE_ROW && (threadIdx.x & 63)) return;
    const int y = WAVE_ROW ? (int)(blockIdx.x * (TE_THREADS / 64) + (threadIdx.x >> 6)) : (int)(blockIdx.x * 64 + threadIdx.x);
    const int W = pg.W, H = pg.H;
    if (y >= H) return;
    uint8_t* base = ws + pg.ws_off;
    const TELayout L = te_layout(W, H, pg.nstrips);
    const uint64_t* bm = reinterpret_cast<const uint64_t*>(base);
    const int sr = te_strip_rows(H, pg.rps), s = y / sr;
    const TERow cur = te_bitmap_row(bm, y, H, te_words(W), WAVE_ROW);
    const TERow ref = y > s * sr ? te_bitmap_row(bm, y - 1, H, te_words(W), WAVE_ROW) : TERow{bm, 0ll, true};
    if (!EMIT) {
        TECount c = {0ull};
        te_row(cur, ref, W, c);
        reinterpret_cast<uint32_t*>(base + L.rowbits)[y] = (uint32_t)c.bits;
    } else {
        if (!reinterpret_cast<const TEMeta*>(base + L.meta)->ok) return;
        const unsigned long long* prefix = reinterpret_cast<const unsigned long long*>(base + L.prefix);
        const unsigned long long* strips = reinterpret_cast<const unsigned long long*>(base + L.strips);
        const unsigned long long bit = 8ull * (8ull + strips[s]) + (prefix[y] - prefix[s * sr]);
        TEWordSink k = {reinterpret_cast<uint32_t*>(pg.out), (long long)(bit >> 5), 0ull, (int)(bit & 31u), true};
        te_row(cur, ref, W, k);
        k.flush();
    }
}

// ---- kernel 3: offsets ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TE_THREADS) void tfe_scan_kernel(uint8_t* ws, long long* out_bytes, int32_t* status, TEBatch bt) {
    __shared__ unsigned long long sh[TE_THREADS];
    const int page = blockIdx.x, tid = threadIdx.x;
    const TEPage& pg = bt.p[page];
    const int H = pg.H, ns = pg.nstrips, sr = te_strip_rows(H, pg.rps);
    uint8_t* base = ws + pg.ws_off;
    const TELayout L = te_layout(pg.W, H, ns);
    const uint32_t* rowbits = reinterpret_cast<const uint32_t*>(base + L.rowbits);
    unsigned long long* prefix = reinterpret_cast<unsigned long long*>(base + L.prefix);
    unsigned long long* strips = reinterpret_cast<unsigned long long*>(base + L.strips);
    unsigned long long sum = 0;
    for (int y0 = 0; y0 < H; y0 += TE_THREADS) {
        const int y = y0 + tid;
        unsigned long long v = y < H ? rowbits[y] : 0ull;
        const unsigned long long tot = rtn_wg_exclusive_scan<TE_THREADS>(sh, v);
        if (y < H) prefix[y] = sum + v;
        sum += tot;
    }
    if (tid == 0) prefix[H] = sum;
    __syncthreads();                                                   // the prefix sums, written by other threads, are read below
    sum = 0;
    for (int s0 = 0; s0 < ns; s0 += TE_THREADS) {
        const int s = s0 + tid;
        unsigned long long v = 0;
        if (s < ns) {
            const int r0 = s * sr, r1 = r0 + sr < H ? r0 + sr : H;
            v = te_strip_bytes(prefix[r1] - prefix[r0]);
        }
        const unsigned long long tot = rtn_wg_exclusive_scan<TE_THREADS>(sh, v);
        if (s < ns) strips[s] = sum + v;
        sum += tot;
    }
    if (tid == 0) {
        strips[ns] = sum;
        const unsigned long long file = te_file_bytes(sum, ns);
        const bool ok = file <= (unsigned long long)pg.bound;         // always, by the bound's derivation; checked because the file is written
        TEMeta* meta = reinterpret_cast<TEMeta*>(base + L.meta);
        meta->file_bytes = ok ? file : 0ull;
        meta->data_bytes = sum;
        meta->ok = ok ? 1u : 0u;
        out_bytes[page] = ok ? (long long)file : 0ll;
        status[page] = ok ? 0 : 1;
    }
}

// ---- kernel 4: zero the file ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TE_THREADS) void tfe_zero_kernel(const uint8_t* ws, TEBatch bt) {
    const int page = blockIdx.y;
    if (page >= bt.n) return;
    const TEPage& pg = bt.p[page];
    const TEMeta* meta = reinterpret_cast<const TEMeta*>(ws + pg.ws_off + te_layout(pg.W, pg.H, pg.nstrips).meta);
    const long long words = (long long)((meta->file_bytes + 3u) >> 2);  // <= bound / 4: the bound is a multiple of 4
    uint32_t* o = reinterpret_cast<uint32_t*>(pg.out);
    for (long long i = (long long)blockIdx.x * TE_THREADS + threadIdx.x; i < words; i += (long long)gridDim.x * TE_THREADS) o[i] = 0u;
}

// ---- kernel 6: EOFBs, header, IFD, strip arrays ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TE_THREADS) void tfe_finish_kernel(const uint8_t* ws, TEBatch bt) {
    const int page = blockIdx.x, tid = threadIdx.x;
    const TEPage& pg = bt.p[page];
    const int H = pg.H, ns = pg.nstrips, sr = te_strip_rows(H, pg.rps);
    const uint8_t* base = ws + pg.ws_off;
    const TELayout L = te_layout(pg.W, H, ns);
    const TEMeta* meta = reinterpret_cast<const TEMeta*>(base + L.meta);
    if (!meta->ok) return;
    const unsigned long long* prefix = reinterpret_cast<const unsigned long long*>(base + L.prefix);
    const unsigned long long* strips = reinterpret_cast<const unsigned long long*>(base + L.strips);
    const uint64_t ifd = te_ifd_offset(meta->data_bytes);
    if (tid == 0) te_header_ifd(pg.out, ifd, pg.W, H, pg.rps, pg.photometric, ns);
    __syncthreads();                                                   // a page of one strip: its entries lie inside the IFD
    for (int s = tid; s < ns; s += TE_THREADS) {                       // a strip's EOFB lies in bytes of its own
        const int r0 = s * sr, r1 = r0 + sr < H ? r0 + sr : H;
        te_eofb(pg.out, 8ull * (8ull + strips[s]) + (prefix[r1] - prefix[r0]));
        te_strip_entry(pg.out, ifd, ns, s, (uint32_t)(8ull + strips[s]), (uint32_t)(strips[s + 1] - strips[s]));
    }
}

int te_check(rtn_handle_t h, int W, int H, int nc, int rps, const char* who) {
    if (te_valid(W, H, nc, rps) && te_bound(W, H, rps)) return RTN_OK;
    if (nc != 1 && nc != 3) return rtn_fail_host(h, RTN_EINVAL, "%s: %d components (1 or 3)", who, nc);
    if (rps < 1 || rps > TE_MAX_RPS) return rtn_fail_host(h, RTN_EINVAL, "%s: %d rows per strip (1 .. %d)", who, rps, TE_MAX_RPS);
    return rtn_fail_host(h, RTN_EINVAL, "%s: %d x %d page: sides must be 1 .. %d and the largest file below 4 GiB", who, W, H, TE_MAX_SIDE);
}

template <bool WAVE_ROW>
int te_launch(rtn_handle_t h, uint8_t* ws, long long* out_bytes, int32_t* status, const TEBatch& bt, int maxrows, long long maxitems,
              long long maxwords) {
    const dim3 rows(WAVE_ROW ? (maxrows + TE_THREADS / 64 - 1) / (TE_THREADS / 64) : (maxrows + 63) / 64, bt.n);
    const int row_threads = WAVE_ROW ? TE_THREADS : 64;
    const long long pack = (maxitems + TE_THREADS / 64 - 1) / (TE_THREADS / 64);
    // the bitmap's layout goes with the row kernels' (te_bitmap_row)
    tfe_pack_kernel<<<dim3(rtn_min_grid(pack, TE_MAX_GRID), bt.n), TE_THREADS, 0, h->stream>>>(ws, bt);
    RTN_CHECK_LAUNCH(h, "tfe_pack_kernel");
    tfe_rows_kernel<false, WAVE_ROW><<<rows, row_threads, 0, h->stream>>>(ws, bt);
    RTN_CHECK_LAUNCH(h, "tfe_rows_kernel (lengths)");
    tfe_scan_kernel<<<bt.n, TE_THREADS, 0, h->stream>>>(ws, out_bytes, status, bt);
    RTN_CHECK_LAUNCH(h, "tfe_scan_kernel");
    tfe_zero_kernel<<<dim3(rtn_grid_for(maxwords, TE_MAX_GRID), bt.n), TE_THREADS, 0, h->stream>>>(ws, bt);
    RTN_CHECK_LAUNCH(h, "tfe_zero_kernel");
    tfe_rows_kernel<true, WAVE_ROW><<<rows, row_threads, 0, h->stream>>>(ws, bt);
    RTN_CHECK_LAUNCH(h, "tfe_rows_kernel (emit)");
    tfe_finish_kernel<<<bt.n, TE_THREADS, 0, h->stream>>>(ws, bt);
    RTN_CHECK_LAUNCH(h, "tfe_finish_kernel");
    return RTN_OK;
}

}  // namespace

// rtn_tiff_encode_*: see include/rtn.h
extern "C" size_t rtn_tiff_encode_bound(int width, int height, int rows_per_strip) {
    if (te_check(nullptr, width, height, 1, rows_per_strip, "rtn_tiff_encode_bound")) return 0;
    return (size_t)te_bound(width, height, rows_per_strip);
}

extern "C" size_t rtn_tiff_encode_workspace_bytes(int n, const int32_t* widths, const int32_t* heights, const int32_t* components,
                                                  const int32_t* rows_per_strip) {
    if (n <= 0 || !widths || !heights || !components || !rows_per_strip) return 0;
    return rtn_codec_page_bytes(
        n, [&](int i) { return te_check(nullptr, widths[i], heights[i], components[i], rows_per_strip[i], "rtn_tiff_encode_workspace_bytes"); },
        [&](int i) { return te_layout(widths[i], heights[i], te_strips(heights[i], rows_per_strip[i])).total; });
}

extern "C" int rtn_tiff_encode_host(int width, int height, int components, const uint8_t* page, int threshold, int rows_per_strip,
                                    int photometric, uint8_t* out, size_t capacity, size_t* out_bytes) {
    if (!page || !out || !out_bytes) { rtn_set_host_error("rtn_tiff_encode_host: NULL argument"); return RTN_EINVAL; }
    const char* why = "";
    const int rc = te_encode_host(width, height, components, page, threshold, rows_per_strip, photometric, out, capacity, out_bytes, &why);
    if (rc != RTN_OK) rtn_fail_host(nullptr, rc, "rtn_tiff_encode_host: %s", why);
    return rc;
}

extern "C" int rtn_tiff_encode(rtn_handle_t h, int n, const uint8_t* const* pages, const int32_t* widths, const int32_t* heights,
                               const int32_t* components, const int32_t* thresholds, const int32_t* rows_per_strip,
                               const int32_t* photometric, uint8_t* out, const int64_t* out_offsets, int64_t* out_bytes, int32_t* status,
                               void* workspace, size_t workspace_bytes) {
    const char* name = "rtn_tiff_encode";
    const int rc = rtn_encode_check(
        h, name, n, {pages, widths, heights, components, thresholds, rows_per_strip, photometric, out, out_offsets, out_bytes, status, workspace}, pages,
        workspace, workspace_bytes, [&](int i) { return te_check(h, widths[i], heights[i], components[i], rows_per_strip[i], name); },
        [&](int i) {
            if (thresholds[i] < 1 || thresholds[i] > 255) return rtn_fail(h, RTN_EINVAL, "%s: page %d: threshold %d (1 .. 255)", name, i, thresholds[i]);
            if (photometric[i] != 0 && photometric[i] != 1) return rtn_fail(h, RTN_EINVAL, "%s: page %d: photometric %d (0 or 1)", name, i, photometric[i]);
            const long long bound = (long long)te_bound(widths[i], heights[i], rows_per_strip[i]);
            if (out_offsets[i] < 0 || out_offsets[i + 1] - out_offsets[i] < bound)
                return rtn_fail(h, RTN_EINVAL, "%s: output slot %d is [%lld, %lld), rtn_tiff_encode_bound asks for %lld bytes", name, i,
                                (long long)out_offsets[i], (long long)out_offsets[i + 1], bound);
            if (((uintptr_t)out + (uintptr_t)out_offsets[i]) & 3) return rtn_fail(h, RTN_EINVAL, "%s: output slot %d is not 4-byte aligned", name, i);
            return RTN_OK;
        },
        [&](int i) { return te_layout(widths[i], heights[i], te_strips(heights[i], rows_per_strip[i])).total; });
    if (rc != RTN_CODEC_GO) return rc;
    rtn_env_sync();                                                    // only a call that launches reads the knob
    const bool wave_row = rtn_env_int("RTN_TIFF_ENC_WAVE_ROW", 0) != 0;
    uint8_t* wsp = static_cast<uint8_t*>(workspace);
    int maxrows = 1;
    long long maxitems = 1, maxwords = 1;
    return rtn_codec_walk<TEBatch>(n,
        [&](TEBatch& bt, int k, int i, long long ws) {
            if (k == 0) bt.row_major = wave_row ? 1 : 0, maxrows = 1, maxitems = 1, maxwords = 1;
            TEPage& p = bt.p[k];
            p.src = pages[i];
            p.out = out + out_offsets[i];
            p.ws_off = ws;
            p.bound = (long long)te_bound(widths[i], heights[i], rows_per_strip[i]);
            p.W = widths[i]; p.H = heights[i]; p.nc = components[i]; p.t = thresholds[i]; p.rps = rows_per_strip[i];
            p.photometric = photometric[i];
            p.nstrips = te_strips(p.H, p.rps);
            maxrows = p.H > maxrows ? p.H : maxrows;
            const long long items = (long long)p.H * te_words(p.W);
            maxitems = items > maxitems ? items : maxitems;
            maxwords = p.bound / 4 > maxwords ? p.bound / 4 : maxwords;
            return te_layout(p.W, p.H, p.nstrips).total;
        },
        [&](const TEBatch& bt, int i0) {
            long long* lengths = reinterpret_cast<long long*>(out_bytes + i0);
            return wave_row ? te_launch<true>(h, wsp, lengths, status + i0, bt, maxrows, maxitems, maxwords)
                            : te_launch<false>(h, wsp, lengths, status + i0, bt, maxrows, maxitems, maxwords);
        });
}
