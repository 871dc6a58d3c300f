// rtn_tiff.hip — strip TIFF pages (uncompressed, PackBits, LZW, Deflate, CCITT Group 4; bilevel, gray, palette, R,G,B) decoded on the
// device, bit-identical to Pillow's decode.  The host side (tf_inspect, csrc/rtn_tiff_decode.h) walks the first IFD and
// copies the strips into a blob; it decodes nothing.  Strips are independent, so the parallelism is strip x page:
//
//   1. tfd_strip_kernel   one wave per strip: the strip's bytes -> its rows of the page's packed rows in the workspace, one status word
//                         per strip.  LZW keeps its 4096 (offset, length) pairs in LDS and copies every string from the output already
//                         written, all lanes sharing the copy; Deflate is pi_run over the strip's zlib stream, then its Adler-32;
//                         PackBits splits its copies over the lanes; a stored strip is only checked (kernel 2 reads it in the blob); Group 4 keeps both run lookups (13 bits in,
//                         run and code length out) and the row under construction and the one before it in LDS: one lane decodes
//                         a row, finding the reference row's changes by scanning its bytes, all lanes clear and store it.
//   2. tfd_pixel_kernel   one workgroup per row (grid-strided): packed row -> B,G,R: bit unpack, predictor 2 as a prefix sum over
//                         the row (per thread a segment's sum, a workgroup scan, then the segment again), inversion, palette.  The
//                         workgroup of row 0 also ORs the page's strip words into its status word.
// No workgroup waits on another and there are no atomics.  Every loop of a decoder consumes input bits or produces output bytes and is
// bounded by the strip's byte count and its rows; every position is checked against those before use (csrc/rtn_tiff_decode.h).  Any
// non-zero status word sends the page to the host decoder.
#include "rtn_codec_launch.h"
#include "rtn_tiff_decode.h"

namespace {

constexpr int TF_WAVE = 64;
constexpr int TF_THREADS = 256;                // the pixel kernel's workgroup
constexpr int TF_MAX_GRID = 4096;              // workgroups along x of either launch: strips and rows past it are looped over
constexpr int TF_LDS_WORDS = 8192;             // 32 KiB: the LZW table, or both run lookups, or Deflate's tables
constexpr uint32_t TF_ROW_BYTES = 8192;        // behind them, Group 4's two rows: ceil(65535 / 8) bytes each at most (the inspector's limit)

struct TFPage {
    long long blob_off, ws_off;
    uint8_t* out;
    int32_t W, H;
    uint32_t compression, layout, invert, predictor, nstrips, rowbytes, off_table, off_pal, off_data, pad_;
};
struct TFBatch {
    int n, pad_;
    TFPage p[RTN_CODEC_BATCH];
};
static_assert(sizeof(TFBatch) <= 3072, "kernel arguments");

struct TFDevMem {                              // one wave, one strip; the positions were checked by the caller (csrc/rtn_tiff_decode.h)
    const uint8_t* src;
    uint32_t in_bytes, lead;
    uint8_t* out;
    uint32_t* lds;
    int ln;
    __device__ inline uint32_t in(uint32_t i) const { return i < in_bytes ? src[i] : 0u; }
    __device__ inline uint32_t word(uint32_t i) const {                // src + lead is word aligned; the blob is padded behind the last strip
        const uint32_t left = in_bytes - lead - 4u * i;                // > 0: i < ceil((in_bytes - lead) / 4)
        const uint32_t w = reinterpret_cast<const uint32_t*>(src + lead)[i];
        return left >= 4u ? w : w & (0xffffffffu >> (8u * (4u - left)));
    }
    __device__ inline uint32_t get(uint32_t pos) const { return out[pos]; }
    __device__ inline void put(uint32_t pos, uint32_t b) { if (ln == 0) out[pos] = (uint8_t)b; }
    __device__ inline uint32_t in32(uint32_t i) const {               // src is word aligned; the blob is padded behind the last strip
        if (i >= in_bytes) return 0u;
        const uint32_t w = __builtin_bswap32(*reinterpret_cast<const uint32_t*>(src + i)), left = in_bytes - i;
        return left >= 4u ? w : w & (0xffffffffu << (8u * (4u - left)));
    }
    // Group 4: rows y and y - 1 live in LDS behind the lookups (rowbytes <= TF_ROW_BYTES); lane 0 decodes, all lanes clear and store
    __device__ inline void row_begin(uint32_t y, uint32_t rowbytes, uint32_t* cur, uint32_t* ref) {
        *cur = (y & 1u) * TF_ROW_BYTES; *ref = ((y & 1u) ^ 1u) * TF_ROW_BYTES;
        uint32_t* row = lds + TF_LDS_WORDS + *cur / 4u;
        for (uint32_t i = (uint32_t)ln; i < (rowbytes + 3u) / 4u; i += TF_WAVE) row[i] = 0u;
        __syncthreads();
    }
    __device__ inline void row_end(uint32_t y, uint32_t rowbytes, uint32_t cur) {
        __syncthreads();
        const uint8_t* row = reinterpret_cast<const uint8_t*>(lds + TF_LDS_WORDS) + cur;
        for (uint32_t i = (uint32_t)ln; i < rowbytes; i += TF_WAVE) out[y * rowbytes + i] = row[i];
    }
    __device__ inline uint32_t rget(uint32_t pos) const { return reinterpret_cast<const uint8_t*>(lds + TF_LDS_WORDS)[pos]; }
    __device__ inline void ror(uint32_t pos, uint32_t mask) { reinterpret_cast<uint8_t*>(lds + TF_LDS_WORDS)[pos] |= (uint8_t)mask; }
    __device__ inline void fill(uint32_t pos, uint32_t n, uint32_t b) {
        for (uint32_t i = (uint32_t)ln; i < n; i += TF_WAVE) out[pos + i] = (uint8_t)b;
    }
    __device__ inline void stored(uint32_t pos, uint32_t at, uint32_t n) {
        for (uint32_t i = (uint32_t)ln; i < n; i += TF_WAVE) out[pos + i] = src[lead + at + i];
    }
    // all lanes copy; the barrier orders the copy behind the writes before it (one wave: no other wave is waited for)
    __device__ inline void match(uint32_t pos, uint32_t d, uint32_t n) {
        __syncthreads();
        if (d >= (uint32_t)TF_WAVE) {                                  // a step of 64 bytes reads nothing the same step writes
            for (uint32_t b = 0; b < n; b += TF_WAVE) {
                const uint32_t i = b + (uint32_t)ln;
                if (i < n) out[pos + i] = out[pos + i - d];
                __syncthreads();
            }
        } else {                                                       // the d bytes before pos, repeated
            for (uint32_t b = 0; b < n; b += TF_WAVE) {
                const uint32_t i = b + (uint32_t)ln;
                if (i < n) out[pos + i] = out[pos - d + (d == 1u ? 0u : i % d)];
            }
        }
    }
    __device__ inline void copy(uint32_t pos, uint32_t from, uint32_t n, bool kwk) {   // every source byte lies before pos
        __syncthreads();
        for (uint32_t i = (uint32_t)ln; i < n; i += TF_WAVE) out[pos + i] = out[kwk && i == n - 1u ? from : from + i];
    }
    // every lane writes the same pair and reads its own write back: no barrier between tab() and tab_off()
    __device__ inline void tab(uint32_t code, uint32_t off, uint32_t len) { lds[2u * code] = off; lds[2u * code + 1u] = len; }
    __device__ inline uint32_t tab_off(uint32_t code) const { return lds[2u * code]; }
    __device__ inline uint32_t tab_len(uint32_t code) const { return lds[2u * code + 1u]; }
    __device__ inline void run_set(int colour, uint32_t i, uint32_t v) { reinterpret_cast<uint16_t*>(lds)[colour * 8192 + (int)i] = (uint16_t)v; }
    __device__ inline uint32_t run(int colour, uint32_t i) const { return reinterpret_cast<const uint16_t*>(lds)[colour * 8192 + (int)i]; }
    __device__ inline int lane() const { return ln; }
    __device__ inline int lanes() const { return TF_WAVE; }
    __device__ inline void sync() { __syncthreads(); }
    __device__ inline uint32_t uni(uint32_t v) const { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
    __device__ inline bool boundary(uint64_t) const { return false; }
    __device__ inline uint32_t adler_join(uint32_t a, uint32_t b, uint32_t n) const {
        for (int o = 32; o > 0; o >>= 1) { a += (uint32_t)__shfl_xor((int)a, o); b += (uint32_t)__shfl_xor((int)b, o); }
        return ((b % 65521u + n % 65521u) % 65521u) << 16 | (a + 1u) % 65521u;
    }
};

// ---- kernel 1: strips -> packed rows --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TF_WAVE) void tfd_strip_kernel(const uint8_t* blobs, uint8_t* ws, TFBatch bt) {
    __shared__ uint32_t lds[TF_LDS_WORDS + 2 * TF_ROW_BYTES / 4];
    static_assert(sizeof(PiTables) <= sizeof(uint32_t) * TF_LDS_WORDS, "Deflate's tables fit");
    const int page = blockIdx.y;
    if (page >= bt.n) return;
    const TFPage& pg = bt.p[page];
    const int ln = threadIdx.x;
    const uint8_t* blob = blobs + pg.blob_off;
    uint32_t* words = reinterpret_cast<uint32_t*>(ws + pg.ws_off + tf_ws_status(pg.H, pg.rowbytes));
    for (uint32_t s = blockIdx.x; s < pg.nstrips; s += gridDim.x) {    // the same trip count in every lane
        const TFStrip sp = reinterpret_cast<const TFStrip*>(blob + pg.off_table)[s];
        TFDevMem m{blob + pg.off_data + sp.off, sp.bytes, pg.compression == TF_DEFLATE ? 2u : 0u,
                   ws + pg.ws_off + (long long)sp.row0 * pg.rowbytes, lds, ln};
        __syncthreads();                                               // the last strip's readers of the tables are done
        // a stored strip is not copied: the pixel kernel reads it where it lies
        const uint32_t st = pg.compression == TF_NONE ? (sp.bytes < sp.rows * pg.rowbytes ? (uint32_t)TF_SHORT : 0u)
                                                      : tf_strip(m, *reinterpret_cast<PiTables*>(lds), pg.compression, sp.bytes, pg.W, sp.rows, pg.rowbytes);
        if (ln == 0) words[s] = st;
    }
}

// ---- kernel 2: packed rows -> the B,G,R page, and the page's status word -----------------------------------------------------------------------
__global__ __launch_bounds__(TF_THREADS) void tfd_pixel_kernel(const uint8_t* blobs, const uint8_t* ws, int32_t* status, TFBatch bt) {
    __shared__ uint32_t sh[TF_THREADS];
    __shared__ uint8_t pal[768];
    const int page = blockIdx.y, tid = threadIdx.x;
    if (page >= bt.n) return;
    const TFPage& pg = bt.p[page];
    const int W = pg.W, H = pg.H;
    const uint32_t layout = pg.layout, invert = pg.invert;
    if (blockIdx.x == 0) {
        const uint32_t* words = reinterpret_cast<const uint32_t*>(ws + pg.ws_off + tf_ws_status(H, pg.rowbytes));
        uint32_t st = 0;
        for (uint32_t s = (uint32_t)tid; s < pg.nstrips; s += TF_THREADS) st |= words[s];
        sh[tid] = st;
        __syncthreads();
        for (int d = TF_THREADS / 2; d > 0; d >>= 1) {
            if (tid < d) sh[tid] |= sh[tid + d];
            __syncthreads();
        }
        if (tid == 0) status[page] = (int32_t)sh[0];
        __syncthreads();
    }
    if (layout == TF_PALETTE)
        for (int i = tid; i < 768; i += TF_THREADS) pal[i] = blobs[pg.blob_off + pg.off_pal + i];
    __syncthreads();
    const int ns = (int)tf_samples(layout);
    for (int y = blockIdx.x; y < H; y += gridDim.x) {
        const uint8_t* row = ws + pg.ws_off + (long long)y * pg.rowbytes;
        if (pg.compression == TF_NONE) {                               // the strip's bytes in the blob; every strip but the last has strip 0's rows
            const TFStrip* table = reinterpret_cast<const TFStrip*>(blobs + pg.blob_off + pg.off_table);
            const TFStrip sp = table[(uint32_t)y / table[0].rows < pg.nstrips ? (uint32_t)y / table[0].rows : 0u];
            if ((uint32_t)y < sp.row0 || (uint32_t)y - sp.row0 >= sp.rows || sp.bytes < sp.rows * pg.rowbytes) continue;   // the page is flagged
            row = blobs + pg.blob_off + pg.off_data + sp.off + (long long)((uint32_t)y - sp.row0) * pg.rowbytes;
        }
        uint8_t* o = pg.out + (long long)y * W * 3;
        if (pg.predictor == 2u) {                                      // 8-bit samples: sample = sum of the row's differences up to it
            const int seg = (W + TF_THREADS - 1) / TF_THREADS, x0 = tid * seg < W ? tid * seg : W, x1 = x0 + seg < W ? x0 + seg : W;
            uint32_t acc[3] = {0u, 0u, 0u};
            for (int x = x0; x < x1; ++x)
                for (int k = 0; k < ns; ++k) acc[k] += tf_raw(row, layout, x, k);
            for (int k = 0; k < ns; ++k) rtn_wg_exclusive_scan<TF_THREADS, uint32_t>(sh, acc[k]);
            for (int x = x0; x < x1; ++x) {
                for (int k = 0; k < ns; ++k) acc[k] = (acc[k] + tf_raw(row, layout, x, k)) & 255u;
                tf_pixel(layout, invert, pal, acc[0], acc[1], acc[2], o + 3ll * x);
            }
        } else {
            for (int x = tid; x < W; x += TF_THREADS)
                tf_pixel(layout, invert, pal, tf_raw(row, layout, x, 0), ns == 3 ? tf_raw(row, layout, x, 1) : 0u, ns == 3 ? tf_raw(row, layout, x, 2) : 0u,
                         o + 3ll * x);
        }
    }
}

// off >= 0: the callers (rtn_codec_blobs, and the walk behind it) have looked at the sign
const TFHdr* tfd_blob(const void* host_blobs, int64_t off) {
    const TFHdr* hd = reinterpret_cast<const TFHdr*>(static_cast<const uint8_t*>(host_blobs) + off);
    if (hd->magic != TF_MAGIC || hd->blob_bytes < (int64_t)sizeof(TFHdr)) return nullptr;
    return tf_blob_ok(hd, (size_t)hd->blob_bytes) ? hd : nullptr;
}

}  // namespace

// rtn_tiff_*: see include/rtn.h
extern "C" size_t rtn_tiff_blob_bound(size_t file_bytes) {
    const size_t strips = file_bytes / 2 + 2 < 65535 ? file_bytes / 2 + 2 : 65535;   // two arrays of at least SHORTs; ImageLength <= 65535
    return 1024 + file_bytes + 21 * strips;
}

extern "C" int rtn_tiff_inspect_flags(rtn_handle_t h, const void* file, size_t file_bytes, int flags, rtn_tiff_info_t* info, void* blob_out,
                                      size_t blob_capacity) {
    return rtn_codec_inspect(h, "rtn_tiff_inspect", file, info, true, [&](char* why, size_t bytes) {
        if (flags & ~RTN_TIFF_ALLOW_G4_ONE_STRIP) {
            snprintf(why, bytes, "rtn_tiff_inspect_flags: unknown flag bits %d", flags);
            return (int)RTN_EINVAL;
        }
        rtn_env_sync();
        const bool one_strip = (flags & RTN_TIFF_ALLOW_G4_ONE_STRIP) || rtn_env_int("RTN_TIFF_G4_ONE_STRIP", 0) != 0;
        return tf_inspect(static_cast<const uint8_t*>(file), file_bytes, one_strip, info, blob_out, blob_capacity, why, bytes);
    });
}

extern "C" int rtn_tiff_inspect(rtn_handle_t h, const void* file, size_t file_bytes, rtn_tiff_info_t* info, void* blob_out, size_t blob_capacity) {
    return rtn_tiff_inspect_flags(h, file, file_bytes, 0, info, blob_out, blob_capacity);
}

extern "C" size_t rtn_tiff_decode_workspace_bytes(int n, const void* host_blobs, const int64_t* offsets) {
    return rtn_codec_blob_bytes(n, host_blobs, offsets, tfd_blob);
}

extern "C" int rtn_tiff_decode_host(const void* blob, uint8_t* out_bgr, size_t out_bytes, int32_t* status) {
    if (!blob || !out_bgr || !status) { rtn_set_host_error("rtn_tiff_decode_host: NULL argument"); return RTN_EINVAL; }
    const TFHdr* hd = static_cast<const TFHdr*>(blob);
    if (hd->magic != TF_MAGIC || hd->blob_bytes < (int64_t)sizeof(TFHdr)) {
        rtn_set_host_error("rtn_tiff_decode_host: not an rtn_tiff_inspect blob");
        return RTN_EINVAL;
    }
    const char* why = "";
    const int rc = tf_decode_host(blob, (size_t)hd->blob_bytes, out_bgr, out_bytes, status, &why);
    if (rc != RTN_OK) rtn_set_host_error(why);
    return rc;
}

extern "C" int rtn_tiff_decode(rtn_handle_t h, int n, const void* host_blobs, const void* dev_blobs, const int64_t* offsets, uint8_t* const* pages,
                               int32_t* status, void* workspace, size_t workspace_bytes) {
    const int rc = rtn_decode_check(h, "rtn_tiff_decode", "rtn_tiff_inspect", n, host_blobs, dev_blobs, offsets, pages, status, workspace,
                                    workspace_bytes, tfd_blob, rtn_codec_no_extra);
    if (rc != RTN_CODEC_GO) return rc;
    const uint8_t* db = static_cast<const uint8_t*>(dev_blobs);
    uint8_t* wsp = static_cast<uint8_t*>(workspace);
    unsigned maxstrips = 1, maxrows = 1;
    return rtn_codec_walk<TFBatch>(n,
        [&](TFBatch& bt, int k, int i, long long ws) {
            const TFHdr* hd = tfd_blob(host_blobs, offsets[i]);
            if (k == 0) maxstrips = 1, maxrows = 1;
            TFPage& p = bt.p[k];
            p.blob_off = offsets[i];
            p.ws_off = ws;
            p.out = pages[i];
            p.W = hd->W; p.H = hd->H;
            p.compression = hd->compression; p.layout = hd->layout; p.invert = hd->invert; p.predictor = hd->predictor;
            p.nstrips = hd->nstrips; p.rowbytes = hd->rowbytes;
            p.off_table = hd->off_table; p.off_pal = hd->off_pal; p.off_data = hd->off_data;
            maxstrips = p.nstrips > maxstrips ? p.nstrips : maxstrips;
            maxrows = (unsigned)p.H > maxrows ? (unsigned)p.H : maxrows;
            return (long long)hd->ws_bytes;
        },
        [&](const TFBatch& bt, int i0) {
            tfd_strip_kernel<<<dim3(rtn_min_grid(maxstrips, TF_MAX_GRID), bt.n), TF_WAVE, 0, h->stream>>>(db, wsp, bt);
            RTN_CHECK_LAUNCH(h, "tfd_strip_kernel");
            tfd_pixel_kernel<<<dim3(rtn_min_grid(maxrows, TF_MAX_GRID), bt.n), TF_THREADS, 0, h->stream>>>(db, wsp, status + i0, bt);
            RTN_CHECK_LAUNCH(h, "tfd_pixel_kernel");
            return RTN_OK;
        });
}
