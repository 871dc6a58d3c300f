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
#include "rtn_internal.h"
#include "rtn_codec.h"

namespace {

constexpr int JPG_MAGIC = 0x47504a52;          // "RJPG"
constexpr int JPG_THREADS = 1024;              // huffman kernel workgroup: one page
constexpr int JPG_MAX_PIXELS = 1 << 28;

struct JHuff {                                 // 1440 bytes
    uint16_t fast[512];                        // 9-bit lookahead: (length << 8) | symbol; 0 = longer code (or none)
    int32_t maxcode[18];                       // [l], l = 1..16: largest code of length l, -1 if none
    int32_t valoff[18];                        // symbol index of code c of length l: c + valoff[l]
    uint8_t val[256];
    uint8_t pad_[16];
};
static_assert(sizeof(JHuff) == 1440, "JHuff layout");

struct JHdr {                                  // 512 bytes at the start of every blob
    int32_t magic, blob_bytes, W, H, ncomp, hmax, vmax;
    int32_t mcux, mcuy, bpm, restart, nseg, total_bits, total_blocks, data_bytes;
    int32_t ch[3], cv[3], tq[3], td[3], ta[3], bw[3], bh[3], blk_off[3], cw[3], chh[3];
    int32_t mcu_c[10], mcu_dy[10], mcu_dx[10];
    int32_t off_huff, off_quant, off_seg, off_data;
    int64_t plane_off[3], ws_bytes;            // per-page workspace: coefficients [total_blocks][64] int16, then the planes
    int32_t reserved_[40];
};
static_assert(sizeof(JHdr) == 512, "JHdr layout");

constexpr int JB_HUFF = 512;                   // 8 tables: DC 0..3, AC 0..3
constexpr int JB_QUANT = JB_HUFF + 8 * (int)sizeof(JHuff);
constexpr int JB_SEG = JB_QUANT + 4 * 64 * 2;

struct JBatch {
    int n, maxblocks, maxpix, pad_;
    long long blob_off[RTN_CODEC_BATCH];
    long long ws_off[RTN_CODEC_BATCH];
    unsigned char* out[RTN_CODEC_BATCH];
};

__host__ __device__ constexpr int zz_natural(int k) {
    constexpr unsigned char nat[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20,
                                       13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59,
                                       52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return nat[k & 63];
}

// ---- bitstream ------------------------------------------------------------------------------------------------------------
__host__ __device__ inline uint32_t bswap32(uint32_t v) {
    return (v >> 24) | ((v >> 8) & 0xff00u) | ((v << 8) & 0xff0000u) | (v << 24);
}

// 32 bits starting at bit p of the segment ending at bit `end`, bits at or past `end` reading as 0, from a cached 64-bit window
// (a thread reads forward: one 32-bit load per 32 bits consumed).  The data is padded by >= 8 bytes behind the last word that
// holds a bit, so every load stays inside the blob whenever p < end.
struct JWin {
    int wbase;
    uint64_t v;
    __host__ __device__ inline uint32_t peek(const uint8_t* data, int p, int end) {
        if (p >= end) return 0u;
        const int wi = p >> 5;
        const uint32_t* w = reinterpret_cast<const uint32_t*>(data);
        if (wi == wbase + 1) { v = (v << 32) | (uint64_t)bswap32(w[wi + 1]); wbase = wi; }
        else if (wi != wbase) { v = ((uint64_t)bswap32(w[wi]) << 32) | (uint64_t)bswap32(w[wi + 1]); wbase = wi; }
        uint32_t r = (uint32_t)(v >> (32 - (p & 31)));
        const int valid = end - p;
        if (valid < 32) r &= ~(0xffffffffu >> valid);
        return r;
    }
};

__host__ __device__ inline int huff_decode(const JHuff* t, uint32_t w, int* len) {
    const int e = t->fast[w >> 23];
    if (e) { *len = e >> 8; return e & 255; }
    for (int l = 10; l <= 16; ++l) {
        const int code = (int)(w >> (32 - l));
        if (code <= t->maxcode[l]) { *len = l; return t->val[(code + t->valoff[l]) & 255]; }
    }
    *len = 0;
    return -1;
}

__host__ __device__ inline int huff_extend(uint32_t v, int s) {
    return v < (1u << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v;
}

// decoder state at a codeword boundary
struct JState { int p, b, k; };

struct JPage {
    const JHdr* hd;
    const uint8_t* data;
    const int32_t* seg;                        // nseg + 1 bit offsets
    const JHuff* dc[10];
    const JHuff* ac[10];
    int comp[10];
};

// largest s with seg[s] <= p (p < seg[nseg]); segments are contiguous in the unstuffed stream
__host__ __device__ inline int find_seg(const int32_t* seg, int nseg, int p) {
    int lo = 0, hi = nseg - 1;
    for (int it = 0; it < 32 && lo < hi; ++it) {
        const int mid = (lo + hi + 1) >> 1;
        if (seg[mid] <= p) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// One decode step from state s inside segment [.., end): returns false on a rule violation (invalid code, coefficient index past
// 63, bits read past the segment end).  What the step produced: *dcdiff for a DC code, else *acpos = natural index of an AC
// coefficient with value *acval (-1 for a run, ZRL or EOB).
__host__ __device__ inline bool jpeg_step(const JPage& pg, JWin& win, JState& s, int end, int* dcdiff, int* acpos, int* acval) {
    const uint32_t w = win.peek(pg.data, s.p, end);
    int len;
    *acpos = -1;
    if (s.k == 0) {
        const int sym = huff_decode(pg.dc[s.b], w, &len);
        if (sym < 0 || sym > 15) return false;
        *dcdiff = sym ? huff_extend((w << len) >> (32 - sym), sym) : 0;
        s.p += len + sym;
        s.k = 1;
    } else {
        const int sym = huff_decode(pg.ac[s.b], w, &len);
        if (sym < 0) return false;
        const int r = sym >> 4, sz = sym & 15;
        if (sz) {
            s.k += r;
            if (s.k > 63) return false;
            *acpos = zz_natural(s.k);
            *acval = huff_extend((w << len) >> (32 - sz), sz);
            s.p += len + sz;
            s.k += 1;
        } else if (r == 15) {
            s.k += 16;
            if (s.k > 64) return false;
            s.p += len;
        } else {
            s.k = 64;
            s.p += len;
        }
        if (s.k == 64) {
            s.k = 0;
            s.b = (s.b + 1 == pg.hd->bpm) ? 0 : s.b + 1;
        }
    }
    return s.p <= end;
}

// what a synchronisation pass leaves per thread: its exit state and, since the last segment start it crossed (reset = 1) or since
// its entry, the blocks it started and the sum of its DC differences per component
struct JSync { JState exit; int reset, cnt, dc[3]; };

__host__ __device__ inline JSync jpeg_sync_range(const JPage& pg, JState s, int rend) {
    JSync o;
    o.reset = 0; o.cnt = 0; o.dc[0] = o.dc[1] = o.dc[2] = 0;
    const int nseg = pg.hd->nseg, total = pg.hd->total_bits;
    if (s.p >= rend || s.p >= total) { o.exit = s; return o; }
    int sg = find_seg(pg.seg, nseg, s.p);
    if (s.p == pg.seg[sg]) { s.b = 0; s.k = 0; o.reset = 1; }
    const int cap = (rend - s.p) + nseg + 2;
    JWin win = {-2, 0};
    for (int it = 0; it < cap && s.p < rend; ++it) {
        const int end = pg.seg[sg + 1];
        if (s.p >= end) {
            if (++sg >= nseg) break;
            s.p = pg.seg[sg]; s.b = 0; s.k = 0;
            o.reset = 1; o.cnt = 0; o.dc[0] = o.dc[1] = o.dc[2] = 0;
            continue;
        }
        const int b = s.b, k = s.k;
        int dcd = 0, ap, av;
        const int p0 = s.p;
        if (!jpeg_step(pg, win, s, end, &dcd, &ap, &av)) {          // a guessed state (or padding, or a corrupt stream): guess again one
            s.p = p0 + 1; s.b = 0; s.k = 0;                     // bit further on; the writing pass decides what an error means
            continue;
        }
        if (k == 0) { o.cnt += 1; o.dc[pg.comp[b]] += dcd; }
    }
    o.exit = s;
    return o;
}

// The writing pass from an exact entry state: blocks started at p < rend are written whole (the thread runs past rend to finish
// its last block); a block in progress at entry belongs to the previous thread and is only parsed.  ord / pred: the first block
// ordinal in the entry segment and the DC predictors there (from the scan).  Returns 0 or a status code.
__host__ __device__ inline int jpeg_write_range(const JPage& pg, JState s, int rend, int ord, int pred0, int pred1, int pred2,
                                                int16_t* coef) {
    const JHdr* hd = pg.hd;
    const int nseg = hd->nseg, total = hd->total_bits;
    if (s.p >= rend || s.p >= total) return 0;
    int pred[3] = {pred0, pred1, pred2};
    int sg = find_seg(pg.seg, nseg, s.p);
    if (s.p == pg.seg[sg]) { s.b = 0; s.k = 0; ord = 0; pred[0] = pred[1] = pred[2] = 0; }
    const int seg_mcus = hd->restart;
    const int total_mcus = hd->mcux * hd->mcuy;
    bool own = s.k == 0;                        // writing the current block (false: finishing the previous thread's block)
    int16_t* blk = nullptr;
    const int cap = (rend - s.p) + nseg + 256;
    JWin win = {-2, 0};
    for (int it = 0; it < cap; ++it) {
        const int end = pg.seg[sg + 1];
        const int mcus = (sg == nseg - 1) ? total_mcus - seg_mcus * (nseg - 1) : seg_mcus;
        const int E = mcus * hd->bpm;
        if (s.k != 0 && !own && ord > E) { s.k = 0; s.p = end; }       // a block past the segment's last: padding, not data
        if (s.k == 0 && (s.p >= rend || s.p >= end || ord >= E)) {
            if (s.p >= rend && ord < E && s.p < end) return 0;         // the next thread continues this segment
            if (ord < E) return 1;                                      // segment ended before its last block
            // this segment is complete: its remaining bits are padding
            if (++sg >= nseg) return 0;
            if (pg.seg[sg] >= rend) return 0;
            s.p = pg.seg[sg]; s.b = 0; s.k = 0; ord = 0; pred[0] = pred[1] = pred[2] = 0; own = true;
            continue;
        }
        if (s.p >= end) return 1;                                       // block cut off by the segment end
        if (s.k == 0) {
            own = true;
            if (ord % hd->bpm != s.b) return 1;
            const int m = sg * seg_mcus + ord / hd->bpm;
            const int c = hd->mcu_c[s.b];
            int by, bx;
            if (hd->ncomp == 1) { by = m / hd->mcux; bx = m - by * hd->mcux; }
            else {
                const int my = m / hd->mcux, mx = m - my * hd->mcux;
                by = my * hd->cv[c] + hd->mcu_dy[s.b];
                bx = mx * hd->ch[c] + hd->mcu_dx[s.b];
            }
            blk = coef + ((long long)hd->blk_off[c] + (long long)by * hd->bw[c] + bx) * 64;
            int4* z = reinterpret_cast<int4*>(blk);
            for (int i = 0; i < 8; ++i) z[i] = make_int4(0, 0, 0, 0);
            ord += 1;
        }
        const int b = s.b, k = s.k;
        int dcd = 0, ap, av;
        if (!jpeg_step(pg, win, s, end, &dcd, &ap, &av)) return 1;
        if (own) {
            if (k == 0) {
                const int c = pg.comp[b];
                pred[c] += dcd;
                blk[0] = (int16_t)pred[c];
            } else if (ap >= 0) {
                blk[ap] = (int16_t)av;
            }
        }
    }
    return 1;
}

// ---- IDCT (jidctint.c jpeg_idct_islow) ---------------------------------------------------------------------------------------
// Returns false where libjpeg-turbo's C code and its 16-bit SIMD code could differ (a dequantised coefficient or a pass-1 value
// too large for 16-bit lanes, an output outside [-512, 511] where the C range-limit table wraps): the host decodes that page.
__host__ __device__ inline int range_limit_idct(int x) {
    const int i = x & 0x3ff;
    return i < 128 ? i + 128 : (i < 512 ? 255 : (i < 896 ? 0 : i - 896));
}

#define JFIX_0_298631336 2446
#define JFIX_0_390180644 3196
#define JFIX_0_541196100 4433
#define JFIX_0_765366865 6270
#define JFIX_0_899976223 7373
#define JFIX_1_175875602 9633
#define JFIX_1_501321110 12299
#define JFIX_1_847759065 15137
#define JFIX_1_961570560 16069
#define JFIX_2_053119869 16819
#define JFIX_2_562915447 20995
#define JFIX_3_072711026 25172

template <typename T>
__host__ __device__ inline void idct_1d(T in0, T in1, T in2, T in3, T in4, T in5, T in6, T in7, T out[8], int shift) {
    T z2 = in2, z3 = in6;
    T z1 = (z2 + z3) * JFIX_0_541196100;
    T tmp2 = z1 + z3 * (-JFIX_1_847759065);
    T tmp3 = z1 + z2 * JFIX_0_765366865;
    z2 = in0; z3 = in4;
    T tmp0 = (z2 + z3) * 8192;
    T tmp1 = (z2 - z3) * 8192;
    const T tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = in7; tmp1 = in5; tmp2 = in3; tmp3 = in1;
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    T z4 = tmp1 + tmp3;
    const T z5 = (z3 + z4) * JFIX_1_175875602;
    tmp0 = tmp0 * JFIX_0_298631336; tmp1 = tmp1 * JFIX_2_053119869;
    tmp2 = tmp2 * JFIX_3_072711026; tmp3 = tmp3 * JFIX_1_501321110;
    z1 = z1 * (-JFIX_0_899976223); z2 = z2 * (-JFIX_2_562915447);
    z3 = z3 * (-JFIX_1_961570560); z4 = z4 * (-JFIX_0_390180644);
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    const T r = (T)1 << (shift - 1);
    out[0] = (tmp10 + tmp3 + r) >> shift; out[7] = (tmp10 - tmp3 + r) >> shift;
    out[1] = (tmp11 + tmp2 + r) >> shift; out[6] = (tmp11 - tmp2 + r) >> shift;
    out[2] = (tmp12 + tmp1 + r) >> shift; out[5] = (tmp12 - tmp1 + r) >> shift;
    out[3] = (tmp13 + tmp0 + r) >> shift; out[4] = (tmp13 - tmp0 + r) >> shift;
}

// coefficients in natural order, quant table in natural order; writes 8 rows of 8 samples at out (row stride ld)
__host__ __device__ inline bool idct_islow(const int16_t* cf, const uint16_t* q, uint8_t* out, int ld) {
    int ws[64];
    bool ok = true;
    for (int c = 0; c < 8; ++c) {
        int d[8];
        for (int r = 0; r < 8; ++r) {
            d[r] = (int)cf[r * 8 + c] * (int)(int16_t)q[r * 8 + c];
            ok &= d[r] > -8192 && d[r] < 8192;
        }
        int o[8];
        idct_1d<int>(d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], o, 11);
        for (int r = 0; r < 8; ++r) {
            ws[r * 8 + c] = o[r];
            ok &= o[r] > -16384 && o[r] < 16384;
        }
    }
    for (int r = 0; r < 8; ++r) {
        const int* w = ws + r * 8;
        long long o[8];
        idct_1d<long long>(w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], o, 18);
        unsigned int lo = 0, hi = 0;
        for (int i = 0; i < 8; ++i) {
            ok &= o[i] >= -512 && o[i] <= 511;
            const unsigned int v = (unsigned int)range_limit_idct((int)o[i]);
            if (i < 4) lo |= v << (8 * i); else hi |= v << (8 * (i - 4));
        }
        uint2* dst = reinterpret_cast<uint2*>(out + (long long)r * ld);
        *dst = make_uint2(lo, hi);
    }
    return ok;
}

// ---- colour (jdcolor.c ycc_rgb_convert, SCALEBITS 16) and upsampling (jdsample.c) -------------------------------------------
__host__ __device__ inline int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__host__ __device__ inline void ycc_to_bgr(int y, int cb, int cr, uint8_t* o) {
    const int x_cr = cr - 128, x_cb = cb - 128;
    const int crr = (91881 * x_cr + 32768) >> 16;                  // FIX(1.40200)
    const int cbb = (116130 * x_cb + 32768) >> 16;                 // FIX(1.77200)
    const int crg = -46802 * x_cr;                                 // -FIX(0.71414)
    const int cbg = -22554 * x_cb + 32768;                         // -FIX(0.34414), ONE_HALF folded in
    o[2] = (uint8_t)clamp255(y + crr);
    o[1] = (uint8_t)clamp255(y + ((cbg + crg) >> 16));
    o[0] = (uint8_t)clamp255(y + cbb);
}

// upsampled chroma sample at output (x, y) from a plane of real size cw x chh (row stride ld)
__host__ __device__ inline int chroma_at(const uint8_t* pl, int ld, int cw, int chh, int hs, int vs, int x, int y) {
    if (hs == 1) return pl[(long long)y * ld + x];                 // 4:4:4
    const int i = x >> 1;
    if (cw <= 2) return pl[(long long)(vs == 2 ? y >> 1 : y) * ld + i];      // libjpeg's box upsampler for narrow planes
    const int in = (x & 1) ? (i + 1 < cw ? i + 1 : cw - 1) : (i > 0 ? i - 1 : 0);
    if (vs == 1) {                                                 // h2v1_fancy_upsample
        const uint8_t* row = pl + (long long)y * ld;
        return (3 * row[i] + row[in] + ((x & 1) ? 2 : 1)) >> 2;
    }
    const int r = y >> 1;                                          // h2v2_fancy_upsample
    const int rf = (y & 1) ? (r + 1 < chh ? r + 1 : chh - 1) : (r > 0 ? r - 1 : 0);
    const uint8_t* near = pl + (long long)r * ld;
    const uint8_t* far = pl + (long long)rf * ld;
    const int cs = 3 * near[i] + far[i];
    const int cn = 3 * near[in] + far[in];
    return (3 * cs + cn + ((x & 1) ? 7 : 8)) >> 4;
}

__host__ __device__ inline JPage make_page(const uint8_t* blob, const JHuff* tables) {
    JPage pg;
    pg.hd = reinterpret_cast<const JHdr*>(blob);
    pg.data = blob + pg.hd->off_data;
    pg.seg = reinterpret_cast<const int32_t*>(blob + pg.hd->off_seg);
    for (int i = 0; i < 10; ++i) {
        const int c = i < pg.hd->bpm ? pg.hd->mcu_c[i] : 0;
        pg.comp[i] = c;
        pg.dc[i] = tables + (pg.hd->td[c] & 3);
        pg.ac[i] = tables + 4 + (pg.hd->ta[c] & 3);
    }
    return pg;
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
    const JPage pg = make_page(blob, tabs);
    const int total = pg.hd->total_bits;
    const int L = ((total + JPG_THREADS - 1) / JPG_THREADS + 31) & ~31;
    const int rstart = min(t * L, total), rend = min(rstart + L, total);

    JState entry = {rstart, 0, 0};
    JSync res;
    for (int pass = 0; pass <= JPG_THREADS; ++pass) {
        if (pass > 0 && t > 0) { entry.p = ex_p[t - 1]; entry.b = ex_bk[t - 1] >> 8; entry.k = ex_bk[t - 1] & 255; }
        __syncthreads();
        if (t == 0) chg[(pass + 1) & 1] = 0;
        res = jpeg_sync_range(pg, entry, rend);
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
    int16_t* coef = reinterpret_cast<int16_t*>(ws + bt.ws_off[page]);
    const int err = jpeg_write_range(pg, entry, rend, ord, p0, p1, p2, coef);
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
    int c = 0;
    if (hd->ncomp == 3) c = i >= hd->blk_off[2] ? 2 : (i >= hd->blk_off[1] ? 1 : 0);
    const int j = i - hd->blk_off[c];
    const int by = j / hd->bw[c], bx = j - by * hd->bw[c];
    uint8_t* base = ws + bt.ws_off[page];
    const int16_t* cf = reinterpret_cast<const int16_t*>(base) + (long long)i * 64;
    const uint16_t* q = reinterpret_cast<const uint16_t*>(blob + hd->off_quant) + 64 * (hd->tq[c] & 3);
    const int ld = hd->bw[c] * 8;
    uint8_t* out = base + hd->plane_off[c] + (long long)by * 8 * ld + bx * 8;
    if (!idct_islow(cf, q, out, ld)) status[page] = 2;
}

__global__ __launch_bounds__(256) void jpeg_color_kernel(const uint8_t* __restrict__ blobs, const uint8_t* __restrict__ ws,
                                                         const int32_t* __restrict__ status, JBatch bt) {
    const int page = blockIdx.y;
    if (page >= bt.n) return;
    const JHdr* hd = reinterpret_cast<const JHdr*>(blobs + bt.blob_off[page]);
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int W = hd->W, H = hd->H;
    if (i >= (long long)W * H || status[page] != 0) return;
    const int y = (int)(i / W), x = (int)(i - (long long)y * W);
    const uint8_t* base = ws + bt.ws_off[page];
    const uint8_t* py = base + hd->plane_off[0];
    const int Y = py[(long long)y * hd->bw[0] * 8 + x];
    uint8_t* o = bt.out[page] + i * 3;
    if (hd->ncomp == 1) { o[0] = o[1] = o[2] = (uint8_t)Y; return; }
    const int hs = hd->hmax, vs = hd->vmax;
    const int cb = chroma_at(base + hd->plane_off[1], hd->bw[1] * 8, hd->cw[1], hd->chh[1], hs, vs, x, y);
    const int cr = chroma_at(base + hd->plane_off[2], hd->bw[2] * 8, hd->cw[2], hd->chh[2], hs, vs, x, y);
    ycc_to_bgr(Y, cb, cr, o);
}

// ---- host parser ------------------------------------------------------------------------------------------------------------
struct RawHuff { bool defined; uint8_t bits[17]; uint8_t val[256]; int count; };

#define jfail(h, ...) rtn_fail_host((h), RTN_EINVAL, __VA_ARGS__)      // a macro, so every message is format-checked

inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// jdhuff.c jpeg_make_d_derived_tbl, as lookup tables; false for a table libjpeg rejects
bool build_huff(const RawHuff& r, bool dc, JHuff* t) {
    memset(t, 0, sizeof(*t));
    int code = 0, p = 0;
    int codes[256], sizes[256];
    for (int l = 1; l <= 16; ++l) {
        for (int i = 0; i < r.bits[l]; ++i) { codes[p] = code++; sizes[p] = l; ++p; }
        if (code >= (1 << l)) return false;                         // no code may be all ones
        code <<= 1;
    }
    p = 0;
    for (int l = 1; l <= 16; ++l) {
        if (r.bits[l]) {
            t->valoff[l] = p - codes[p];
            p += r.bits[l];
            t->maxcode[l] = codes[p - 1];
        } else {
            t->maxcode[l] = -1;
        }
    }
    t->maxcode[0] = -1; t->maxcode[17] = 0x7fffffff;
    for (int i = 0; i < r.count; ++i) {
        t->val[i] = r.val[i];
        if (dc && r.val[i] > 15) return false;
    }
    for (int i = 0; i < r.count; ++i) {
        if (sizes[i] > 9) continue;
        const int shift = 9 - sizes[i];
        const int lo = codes[i] << shift;
        for (int j = 0; j < (1 << shift); ++j) t->fast[lo + j] = (uint16_t)((sizes[i] << 8) | r.val[i]);
    }
    return true;
}

}  // namespace

// rtn_jpeg_inspect: see include/rtn.h
extern "C" int rtn_jpeg_inspect(rtn_handle_t h, const void* file, size_t file_bytes, rtn_jpeg_info_t* info, void* blob_out,
                                size_t blob_capacity) {
    if (!info) return jfail(h, "rtn_jpeg_inspect: info is NULL");
    memset(info, 0, sizeof(*info));
    if (!file) return jfail(h, "rtn_jpeg_inspect: file is NULL");
    const uint8_t* f = static_cast<const uint8_t*>(file);
    const size_t n = file_bytes;
    if (n < 4 || f[0] != 0xFF || f[1] != 0xD8) return jfail(h, "not a JPEG file (no SOI marker)");
    if (n >= ((size_t)1 << 28)) return jfail(h, "file larger than 256 MiB");

    RawHuff rh[8];
    for (auto& r : rh) r.defined = false;
    uint16_t qt[4][64];
    bool qdef[4] = {false, false, false, false};
    bool sof = false, jfif = false, adobe = false;
    int adobe_transform = -1, restart = 0;
    int W = 0, H = 0, nf = 0, cid[3] = {0, 0, 0}, chs[3] = {0, 0, 0}, cvs[3] = {0, 0, 0}, ctq[3] = {0, 0, 0};
    int td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};
    size_t pos = 2;
    size_t scan_begin = 0;
    for (;;) {
        // next marker: 0xFF, any fill 0xFF bytes, a code
        if (pos >= n || f[pos] != 0xFF) return jfail(h, "corrupt JPEG: expected a marker at byte %zu", pos);
        while (pos < n && f[pos] == 0xFF) ++pos;
        if (pos >= n) return jfail(h, "truncated JPEG header");
        const int m = f[pos++];
        if (m == 0xD8) return jfail(h, "corrupt JPEG: second SOI marker");
        if (m == 0xD9) return jfail(h, "JPEG has no scan (EOI before SOS)");
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) return jfail(h, "unexpected marker 0x%02X before the scan", m);
        if (pos + 2 > n) return jfail(h, "truncated JPEG header");
        const int len = be16(f + pos);
        if (len < 2 || pos + (size_t)len > n) return jfail(h, "truncated JPEG header (marker 0x%02X)", m);
        const uint8_t* s = f + pos + 2;
        const int sl = len - 2;
        pos += len;
        switch (m) {
        case 0xC0:
            if (sof) return jfail(h, "more than one frame header");
            if (sl < 6) return jfail(h, "corrupt SOF0 segment");
            if (s[0] != 8) return jfail(h, "%d-bit JPEG (only 8-bit is decoded on the device)", s[0]);
            H = be16(s + 1); W = be16(s + 3); nf = s[5];
            if (H == 0) return jfail(h, "JPEG height defined by a DNL marker");
            if (W == 0) return jfail(h, "JPEG width is 0");
            if (nf != 1 && nf != 3) return jfail(h, "%d-component JPEG (CMYK/YCCK or other; only 1 or 3 components)", nf);
            if (sl < 6 + 3 * nf) return jfail(h, "corrupt SOF0 segment");
            for (int c = 0; c < nf; ++c) {
                cid[c] = s[6 + 3 * c]; chs[c] = s[7 + 3 * c] >> 4; cvs[c] = s[7 + 3 * c] & 15; ctq[c] = s[8 + 3 * c];
                if (ctq[c] > 3) return jfail(h, "corrupt SOF0: quantisation table %d", ctq[c]);
                if (chs[c] < 1 || chs[c] > 4 || cvs[c] < 1 || cvs[c] > 4) return jfail(h, "corrupt SOF0: sampling factors");
            }
            sof = true;
            break;
        case 0xC1: return jfail(h, "extended sequential JPEG (SOF1)");
        case 0xC2: return jfail(h, "progressive JPEG (SOF2)");
        case 0xC3: return jfail(h, "lossless JPEG (SOF3)");
        case 0xC5: case 0xC6: case 0xC7: return jfail(h, "hierarchical JPEG (SOF%d)", m - 0xC0);
        case 0xC9: case 0xCA: case 0xCB: case 0xCD: case 0xCE: case 0xCF:
            return jfail(h, "arithmetic-coded JPEG (SOF%d)", m - 0xC0);
        case 0xCC: return jfail(h, "arithmetic-coded JPEG (DAC)");
        case 0xDC: return jfail(h, "JPEG with a DNL marker");
        case 0xC4: {
            int q = 0;
            while (q < sl) {
                if (q + 17 > sl) return jfail(h, "corrupt DHT segment");
                const int tc = s[q] >> 4, th = s[q] & 15;
                if (tc > 1 || th > 3) return jfail(h, "corrupt DHT segment (table 0x%02X)", s[q]);
                RawHuff& r = rh[tc * 4 + th];
                int count = 0;
                r.bits[0] = 0;
                for (int l = 1; l <= 16; ++l) { r.bits[l] = s[q + l]; count += s[q + l]; }
                if (count > 256 || q + 17 + count > sl) return jfail(h, "corrupt DHT segment");
                memcpy(r.val, s + q + 17, count);
                r.count = count;
                r.defined = true;
                q += 17 + count;
            }
            break;
        }
        case 0xDB: {
            int q = 0;
            while (q < sl) {
                const int pq = s[q] >> 4, tq = s[q] & 15;
                if (pq > 1 || tq > 3) return jfail(h, "corrupt DQT segment");
                const int need = 1 + 64 * (pq ? 2 : 1);
                if (q + need > sl) return jfail(h, "corrupt DQT segment");
                for (int k = 0; k < 64; ++k)
                    qt[tq][zz_natural(k)] = (uint16_t)(pq ? be16(s + q + 1 + 2 * k) : s[q + 1 + k]);
                qdef[tq] = true;
                q += need;
            }
            break;
        }
        case 0xDD:
            if (sl < 2) return jfail(h, "corrupt DRI segment");
            restart = be16(s);
            break;
        case 0xE0:
            if (sl >= 14 && s[0] == 'J' && s[1] == 'F' && s[2] == 'I' && s[3] == 'F' && s[4] == 0) jfif = true;
            break;
        case 0xEE:
            if (sl >= 12 && s[0] == 'A' && s[1] == 'd' && s[2] == 'o' && s[3] == 'b' && s[4] == 'e') {
                adobe = true;
                adobe_transform = s[11];
            }
            break;
        case 0xDA: {
            if (!sof) return jfail(h, "corrupt JPEG: scan before the frame header");
            if (sl < 1) return jfail(h, "corrupt SOS segment");
            const int ns = s[0];
            if (sl < 1 + 2 * ns + 3) return jfail(h, "corrupt SOS segment");
            if (ns != nf) return jfail(h, "multi-scan JPEG (a scan with %d of %d components)", ns, nf);
            for (int c = 0; c < ns; ++c) {
                if (s[1 + 2 * c] != cid[c]) return jfail(h, "scan components out of frame order");
                td[c] = s[2 + 2 * c] >> 4; ta[c] = s[2 + 2 * c] & 15;
                if (td[c] > 3 || ta[c] > 3) return jfail(h, "corrupt SOS: Huffman table index");
            }
            const uint8_t* e = s + 1 + 2 * ns;
            if (e[0] != 0 || e[1] != 63 || e[2] != 0) return jfail(h, "JPEG scan is not a baseline sequential scan");
            scan_begin = pos;
            break;
        }
        default:
            break;                                                  // APPn, COM, ... skipped
        }
        if (scan_begin) break;
    }

    // colour space (jdapimin.c default_decompress_parms) and sampling
    if (nf == 3) {
        if (!jfif && adobe && adobe_transform == 0) return jfail(h, "Adobe RGB JPEG (transform 0)");
        if (!jfif && !adobe && cid[0] == 82 && cid[1] == 71 && cid[2] == 66) return jfail(h, "RGB JPEG (component ids R, G, B)");
        if (chs[1] != 1 || cvs[1] != 1 || chs[2] != 1 || cvs[2] != 1 ||
            !((chs[0] == 1 && cvs[0] == 1) || (chs[0] == 2 && cvs[0] == 1) || (chs[0] == 2 && cvs[0] == 2)))
            return jfail(h, "unsupported sampling factors %dx%d,%dx%d,%dx%d", chs[0], cvs[0], chs[1], cvs[1], chs[2], cvs[2]);
    }
    if ((long long)W * H > JPG_MAX_PIXELS) return jfail(h, "image too large for the device decoder");
    for (int c = 0; c < nf; ++c) {
        if (!qdef[ctq[c]]) return jfail(h, "quantisation table %d not defined", ctq[c]);
        if (!rh[td[c]].defined || !rh[4 + ta[c]].defined) return jfail(h, "Huffman table not defined (standard tables are not assumed)");
    }

    // geometry
    JHdr hd;
    memset(&hd, 0, sizeof(hd));
    hd.magic = JPG_MAGIC;
    hd.W = W; hd.H = H; hd.ncomp = nf;
    if (nf == 1) {
        hd.hmax = hd.vmax = 1;
        hd.mcux = (W + 7) / 8; hd.mcuy = (H + 7) / 8; hd.bpm = 1;
        hd.ch[0] = hd.cv[0] = 1;
        hd.bw[0] = hd.mcux; hd.bh[0] = hd.mcuy;
        hd.cw[0] = W; hd.chh[0] = H;
        hd.mcu_c[0] = 0;
    } else {
        hd.hmax = chs[0]; hd.vmax = cvs[0];
        hd.mcux = (W + 8 * hd.hmax - 1) / (8 * hd.hmax);
        hd.mcuy = (H + 8 * hd.vmax - 1) / (8 * hd.vmax);
        int b = 0;
        for (int c = 0; c < 3; ++c) {
            hd.ch[c] = chs[c]; hd.cv[c] = cvs[c];
            hd.bw[c] = hd.mcux * chs[c]; hd.bh[c] = hd.mcuy * cvs[c];
            hd.cw[c] = (W * chs[c] + hd.hmax - 1) / hd.hmax;
            hd.chh[c] = (H * cvs[c] + hd.vmax - 1) / hd.vmax;
            for (int dy = 0; dy < cvs[c]; ++dy)
                for (int dx = 0; dx < chs[c]; ++dx) { hd.mcu_c[b] = c; hd.mcu_dy[b] = dy; hd.mcu_dx[b] = dx; ++b; }
        }
        hd.bpm = b;
    }
    for (int c = 0; c < nf; ++c) { hd.tq[c] = ctq[c]; hd.td[c] = td[c]; hd.ta[c] = ta[c]; }
    int blocks = 0;
    for (int c = 0; c < nf; ++c) { hd.blk_off[c] = blocks; blocks += hd.bw[c] * hd.bh[c]; }
    hd.total_blocks = blocks;
    long long wsb = ((long long)blocks * 128 + 255) & ~255LL;
    for (int c = 0; c < nf; ++c) {
        hd.plane_off[c] = wsb;
        wsb += ((long long)hd.bw[c] * 8 * hd.bh[c] * 8 + 255) & ~255LL;
    }
    hd.ws_bytes = wsb;
    const long long total_mcus = (long long)hd.mcux * hd.mcuy;
    hd.restart = restart > 0 ? restart : (int)total_mcus;
    const long long nseg = (total_mcus + hd.restart - 1) / hd.restart;
    hd.nseg = (int)nseg;
    if (nseg - 1 > (long long)(n - scan_begin) / 2) return jfail(h, "corrupt JPEG: more restart segments than the file holds");

    // the entropy-coded segment: unstuff, drop RST markers, record segment starts; the scan must end at EOI
    hd.off_seg = JB_SEG;
    hd.off_data = (int)((JB_SEG + 4 * (nseg + 1) + 15) & ~15LL);
    const size_t data_cap = n - scan_begin;
    const size_t bound = (size_t)hd.off_data + ((data_cap + 15) & ~(size_t)15) + 32;
    info->width = W; info->height = H; info->components = nf;
    info->h_samp = hd.hmax; info->v_samp = hd.vmax; info->restart_interval = restart;
    int ntab = 0;
    for (auto& r : rh) ntab += r.defined;
    info->huffman_tables = ntab;
    int nq = 0;
    for (bool q : qdef) nq += q;
    info->quant_tables = nq;
    info->blob_bytes = (int64_t)bound;
    info->workspace_bytes = hd.ws_bytes;
    if (!blob_out) return RTN_OK;                                   // geometry only
    if (blob_capacity < bound) return jfail(h, "blob buffer too small: %zu < %zu bytes", blob_capacity, bound);
    uint8_t* bl = static_cast<uint8_t*>(blob_out);
    uint8_t* d = bl + hd.off_data;
    int32_t* segs = reinterpret_cast<int32_t*>(bl + JB_SEG);
    size_t dn = 0, q = scan_begin;
    long long nrst = 0;
    segs[0] = 0;
    bool eoi = false;
    while (q < n) {
        const uint8_t* ff = static_cast<const uint8_t*>(memchr(f + q, 0xFF, n - q));
        const size_t stop = ff ? (size_t)(ff - f) : n;
        memcpy(d + dn, f + q, stop - q);
        dn += stop - q;
        q = stop;
        if (!ff) break;
        if (q + 1 >= n) break;
        const int m = f[q + 1];
        if (m == 0x00) { d[dn++] = 0xFF; q += 2; continue; }
        if (m == 0xFF) { q += 1; continue; }                        // fill byte before a marker
        if (m >= 0xD0 && m <= 0xD7) {
            if ((m & 7) != (int)(nrst & 7) || ++nrst >= nseg) return jfail(h, "corrupt JPEG: restart markers out of sequence");
            segs[nrst] = (int32_t)(dn * 8);
            q += 2;
            continue;
        }
        eoi = m == 0xD9;
        if (!eoi) return jfail(h, "JPEG continues after the scan with marker 0x%02X (multi-scan or DNL)", m);
        break;
    }
    if (!eoi) return jfail(h, "truncated JPEG (no EOI after the scan)");
    if (nrst != nseg - 1) return jfail(h, "corrupt JPEG: %lld restart markers, %lld expected", nrst, nseg - 1);
    if (dn == 0) return jfail(h, "corrupt JPEG: empty scan");
    if (dn * 8 >= ((size_t)1 << 31)) return jfail(h, "scan too long");
    for (long long i = 1; i < nseg; ++i)
        if (segs[i] <= segs[i - 1]) return jfail(h, "corrupt JPEG: empty restart segment %lld", i - 1);
    hd.data_bytes = (int)dn;
    hd.total_bits = (int)(dn * 8);
    segs[nseg] = hd.total_bits;
    memset(d + dn, 0, bound - hd.off_data - dn);
    if (segs[nseg] <= segs[nseg - 1]) return jfail(h, "corrupt JPEG: empty restart segment %lld", nseg - 1);
    hd.blob_bytes = (int)((size_t)hd.off_data + ((dn + 15) & ~(size_t)15) + 16);
    if ((size_t)hd.blob_bytes > bound) return jfail(h, "internal: blob bound");
    for (int i = 0; i < 8; ++i) {
        JHuff* t = reinterpret_cast<JHuff*>(bl + JB_HUFF) + i;
        if (!rh[i].defined) { memset(t, 0, sizeof(*t)); continue; }
        if (!build_huff(rh[i], i < 4, t)) return jfail(h, "corrupt JPEG: bad Huffman table 0x%02X", (i >> 2) * 16 + (i & 3));
    }
    uint16_t* qd = reinterpret_cast<uint16_t*>(bl + JB_QUANT);
    for (int t = 0; t < 4; ++t)
        for (int k = 0; k < 64; ++k) qd[t * 64 + k] = qdef[t] ? qt[t][k] : 0;
    hd.off_huff = JB_HUFF;
    hd.off_quant = JB_QUANT;
    memcpy(bl, &hd, sizeof(hd));
    info->blob_bytes = hd.blob_bytes;
    info->scan_bytes = (int64_t)dn;
    return RTN_OK;
}

static bool jpeg_blob_ok(const uint8_t* b) {
    const JHdr* hd = reinterpret_cast<const JHdr*>(b);
    return hd->magic == JPG_MAGIC && hd->ws_bytes > 0 && hd->nseg > 0;
}

extern "C" size_t rtn_jpeg_workspace_bytes(int n, const void* host_blobs, const int64_t* offsets) {
    if (n <= 0 || !host_blobs || !offsets) return 0;
    size_t tot = 0;
    for (int i = 0; i < n; ++i) {
        const uint8_t* b = static_cast<const uint8_t*>(host_blobs) + offsets[i];
        if (!jpeg_blob_ok(b)) return 0;
        tot += (size_t)reinterpret_cast<const JHdr*>(b)->ws_bytes;
    }
    return tot;
}

extern "C" int rtn_jpeg_decode(rtn_handle_t h, int n, const void* host_blobs, const void* dev_blobs, const int64_t* offsets,
                               uint8_t* const* pages, int32_t* status, void* workspace, size_t workspace_bytes) {
    if (!h) return RTN_EINVAL;
    if (n < 0) return rtn_fail(h, RTN_EINVAL, "rtn_jpeg_decode: n < 0");
    if (n == 0) return RTN_OK;
    if (!host_blobs || !dev_blobs || !offsets || !pages || !status || !workspace)
        return rtn_fail(h, RTN_EINVAL, "rtn_jpeg_decode: NULL argument");
    if (((uintptr_t)dev_blobs & 15) || ((uintptr_t)workspace & 255))
        return rtn_fail(h, RTN_EINVAL, "rtn_jpeg_decode: blobs must be 16-byte aligned, the workspace 256-byte aligned");
    size_t need = 0;
    for (int i = 0; i < n; ++i) {
        if (offsets[i] < 0 || (offsets[i] & 15)) return rtn_fail(h, RTN_EINVAL, "rtn_jpeg_decode: blob %d offset not 16-byte aligned", i);
        const uint8_t* b = static_cast<const uint8_t*>(host_blobs) + offsets[i];
        if (!jpeg_blob_ok(b)) return rtn_fail(h, RTN_EINVAL, "rtn_jpeg_decode: blob %d is not an rtn_jpeg_inspect blob", i);
        if (!pages[i]) return rtn_fail(h, RTN_EINVAL, "rtn_jpeg_decode: page %d is NULL", i);
        need += (size_t)reinterpret_cast<const JHdr*>(b)->ws_bytes;
    }
    if (workspace_bytes < need)
        return rtn_fail(h, RTN_ENOMEM, "rtn_jpeg_decode: workspace %zu < %zu bytes", workspace_bytes, need);
    long long ws = 0;
    for (int i0 = 0; i0 < n; i0 += RTN_CODEC_BATCH) {
        JBatch bt;
        memset(&bt, 0, sizeof(bt));
        bt.n = n - i0 < RTN_CODEC_BATCH ? n - i0 : RTN_CODEC_BATCH;
        long long maxpix = 0;
        int maxblocks = 0;
        for (int j = 0; j < bt.n; ++j) {
            const JHdr* hd = reinterpret_cast<const JHdr*>(static_cast<const uint8_t*>(host_blobs) + offsets[i0 + j]);
            bt.blob_off[j] = offsets[i0 + j];
            bt.ws_off[j] = ws;
            bt.out[j] = pages[i0 + j];
            ws += hd->ws_bytes;
            maxblocks = hd->total_blocks > maxblocks ? hd->total_blocks : maxblocks;
            maxpix = (long long)hd->W * hd->H > maxpix ? (long long)hd->W * hd->H : maxpix;
        }
        const uint8_t* db = static_cast<const uint8_t*>(dev_blobs);
        uint8_t* wsp = static_cast<uint8_t*>(workspace);
        jpeg_huffman_kernel<<<bt.n, JPG_THREADS, 0, h->stream>>>(db, wsp, status + i0, bt);
        RTN_CHECK_LAUNCH(h, "jpeg_huffman_kernel");
        jpeg_idct_kernel<<<dim3((maxblocks + 255) / 256, bt.n), 256, 0, h->stream>>>(db, wsp, status + i0, bt);
        RTN_CHECK_LAUNCH(h, "jpeg_idct_kernel");
        jpeg_color_kernel<<<dim3((unsigned)((maxpix + 255) / 256), bt.n), 256, 0, h->stream>>>(db, wsp, status + i0, bt);
        RTN_CHECK_LAUNCH(h, "jpeg_color_kernel");
    }
    return RTN_OK;
}
