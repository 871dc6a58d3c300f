// rtn_jpeg_decode.h — the text that the device JPEG decoder (csrc/rtn_jpeg.hip) and its CPU twin share: the blob
// layout, the file inspector, and the decode functions (bit window, Huffman decode, the synchronisation and writing passes over a
// bit range, ISLOW IDCT, upsampling, colour) as __host__ __device__ functions.  A plain C++17 compiler compiles this header (no
// HIP), so that csrc/rtn_jpeg.hip and a stand-alone sanitizer build (tools/jpeg_decode_fuzz.cpp) compile the same text.
//
// Every access to memory whose position comes from file bytes goes through a memory context `M`:
//   uint32_t word(int i)                      32-bit word i of the entropy-coded bytes, as stored (big-endian bit order)
//   int seg(int i)                            bit offset at which restart segment i starts, i = 0 .. nseg (nseg: the total)
//   void zero(long long b)                    the 64 coefficients of block b = 0
//   void coef(long long b, int i, int v)      coefficient i (natural order) of block b = v
//   const int16_t* block(long long b)         the 64 coefficients of block b
//   void row8(int c, long long off, uint32_t lo, uint32_t hi)     8 samples at byte `off` of component c's plane (off % 8 == 0)
//   int px(int c, long long off)              the sample at byte `off` of component c's plane
// The kernels' context (JDevMem in rtn_jpeg.hip) does the plain loads and stores; the twin's (JHostMem below) checks every position
// against the sizes it was given and aborts on one outside them.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "rtn.h"
#if !defined(__HIPCC__) && !defined(__host__)      // a plain C++ compiler (host-only fuzzing builds)
#define __host__
#define __device__
#endif

constexpr int JPG_MAGIC = 0x47504a52;          // "RJPG"
constexpr int JPG_THREADS = 1024;              // huffman kernel workgroup: one page
constexpr int JPG_MAX_PIXELS = 1 << 28;
constexpr int JPG_HOST_THREADS_MAX = 1 << 16;  // the twin's virtual threads

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
    template <class M>
    __host__ __device__ inline uint32_t peek(const M& m, int p, int end) {
        if (p >= end) return 0u;
        const int wi = p >> 5;
        if (wi == wbase + 1) { v = (v << 32) | (uint64_t)bswap32(m.word(wi + 1)); wbase = wi; }
        else if (wi != wbase) { v = ((uint64_t)bswap32(m.word(wi)) << 32) | (uint64_t)bswap32(m.word(wi + 1)); wbase = wi; }
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

// largest s with seg(s) <= p (p < seg(nseg)); segments are contiguous in the unstuffed stream
template <class M>
__host__ __device__ inline int find_seg(const M& m, int nseg, int p) {
    int lo = 0, hi = nseg - 1;
    for (int it = 0; it < 32 && lo < hi; ++it) {
        const int mid = (lo + hi + 1) >> 1;
        if (m.seg(mid) <= p) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// One decode step from state s inside segment [.., end): returns false on a rule violation (invalid code, coefficient index past
// 63, bits read past the segment end).  What the step produced: *dcdiff for a DC code, else *acpos = natural index of an AC
// coefficient with value *acval (-1 for a run, ZRL or EOB).
template <class M>
__host__ __device__ inline bool jpeg_step(const JPage& pg, const M& m, JWin& win, JState& s, int end, int* dcdiff, int* acpos,
                                          int* acval) {
    const uint32_t w = win.peek(m, s.p, end);
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

template <class M>
__host__ __device__ inline JSync jpeg_sync_range(const JPage& pg, const M& m, JState s, int rend) {
    JSync o;
    o.reset = 0; o.cnt = 0; o.dc[0] = o.dc[1] = o.dc[2] = 0;
    const int nseg = pg.hd->nseg, total = pg.hd->total_bits;
    if (s.p >= rend || s.p >= total) { o.exit = s; return o; }
    int sg = find_seg(m, nseg, s.p);
    if (s.p == m.seg(sg)) { s.b = 0; s.k = 0; o.reset = 1; }
    const int cap = (rend - s.p) + nseg + 2;
    JWin win = {-2, 0};
    for (int it = 0; it < cap && s.p < rend; ++it) {
        const int end = m.seg(sg + 1);
        if (s.p >= end) {
            if (++sg >= nseg) break;
            s.p = m.seg(sg); s.b = 0; s.k = 0;
            o.reset = 1; o.cnt = 0; o.dc[0] = o.dc[1] = o.dc[2] = 0;
            continue;
        }
        const int b = s.b, k = s.k;
        int dcd = 0, ap, av;
        const int p0 = s.p;
        if (!jpeg_step(pg, m, win, s, end, &dcd, &ap, &av)) {       // a guessed state (or padding, or a corrupt stream): guess again one
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
template <class M>
__host__ __device__ inline int jpeg_write_range(const JPage& pg, M& m, JState s, int rend, int ord, int pred0, int pred1, int pred2) {
    const JHdr* hd = pg.hd;
    const int nseg = hd->nseg, total = hd->total_bits;
    if (s.p >= rend || s.p >= total) return 0;
    int pred[3] = {pred0, pred1, pred2};
    int sg = find_seg(m, nseg, s.p);
    if (s.p == m.seg(sg)) { s.b = 0; s.k = 0; ord = 0; pred[0] = pred[1] = pred[2] = 0; }
    const int seg_mcus = hd->restart;
    const int total_mcus = hd->mcux * hd->mcuy;
    bool own = s.k == 0;                        // writing the current block (false: finishing the previous thread's block)
    long long blk = -1;
    const int cap = (rend - s.p) + nseg + 256;
    JWin win = {-2, 0};
    for (int it = 0; it < cap; ++it) {
        const int end = m.seg(sg + 1);
        const int mcus = (sg == nseg - 1) ? total_mcus - seg_mcus * (nseg - 1) : seg_mcus;
        const int E = mcus * hd->bpm;
        if (s.k != 0 && !own && ord > E) { s.k = 0; s.p = end; }       // a block past the segment's last: padding, not data
        if (s.k == 0 && (s.p >= rend || s.p >= end || ord >= E)) {
            if (s.p >= rend && ord < E && s.p < end) return 0;         // the next thread continues this segment
            if (ord < E) return 1;                                      // segment ended before its last block
            // this segment is complete: its remaining bits are padding
            if (++sg >= nseg) return 0;
            if (m.seg(sg) >= rend) return 0;
            s.p = m.seg(sg); s.b = 0; s.k = 0; ord = 0; pred[0] = pred[1] = pred[2] = 0; own = true;
            continue;
        }
        if (s.p >= end) return 1;                                       // block cut off by the segment end
        if (s.k == 0) {
            own = true;
            if (ord % hd->bpm != s.b) return 1;
            const int mi = sg * seg_mcus + ord / hd->bpm;
            const int c = hd->mcu_c[s.b];
            int by, bx;
            if (hd->ncomp == 1) { by = mi / hd->mcux; bx = mi - by * hd->mcux; }
            else {
                const int my = mi / hd->mcux, mx = mi - my * hd->mcux;
                by = my * hd->cv[c] + hd->mcu_dy[s.b];
                bx = mx * hd->ch[c] + hd->mcu_dx[s.b];
            }
            blk = (long long)hd->blk_off[c] + (long long)by * hd->bw[c] + bx;
            m.zero(blk);
            ord += 1;
        }
        const int b = s.b, k = s.k;
        int dcd = 0, ap, av;
        if (!jpeg_step(pg, m, win, s, end, &dcd, &ap, &av)) return 1;
        if (own) {
            if (k == 0) {
                const int c = pg.comp[b];
                pred[c] += dcd;
                m.coef(blk, 0, pred[c]);
            } else if (ap >= 0) {
                m.coef(blk, ap, av);
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

// block b's coefficients in natural order, quant table in natural order; writes 8 rows of 8 samples of component c's plane from
// byte `off` (row stride ld).  P1: the type pass 1 computes in.  int (libjpeg's, the kernel's) is exact for every block this
// function accepts; the twin passes long long, so that the arithmetic of a block it refuses cannot overflow on a CPU.
template <typename P1 = int, class M>
__host__ __device__ inline bool idct_islow(M& m, long long b, const uint16_t* q, int c, long long off, int ld) {
    const int16_t* cf = m.block(b);
    int ws[64];
    bool ok = true;
    for (int col = 0; col < 8; ++col) {
        int d[8];
        for (int r = 0; r < 8; ++r) {
            d[r] = (int)cf[r * 8 + col] * (int)(int16_t)q[r * 8 + col];
            ok &= d[r] > -8192 && d[r] < 8192;
        }
        P1 o[8];
        idct_1d<P1>(d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], o, 11);
        for (int r = 0; r < 8; ++r) {
            ws[r * 8 + col] = (int)o[r];
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
        m.row8(c, off + (long long)r * ld, lo, hi);
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

// upsampled chroma sample at output (x, y) from component c's plane of real size cw x chh (row stride ld)
template <class M>
__host__ __device__ inline int chroma_at(const M& m, int c, int ld, int cw, int chh, int hs, int vs, int x, int y) {
    if (hs == 1) return m.px(c, (long long)y * ld + x);            // 4:4:4
    const int i = x >> 1;
    if (cw <= 2) return m.px(c, (long long)(vs == 2 ? y >> 1 : y) * ld + i);     // libjpeg's box upsampler for narrow planes
    const int in = (x & 1) ? (i + 1 < cw ? i + 1 : cw - 1) : (i > 0 ? i - 1 : 0);
    if (vs == 1) {                                                 // h2v1_fancy_upsample
        const long long row = (long long)y * ld;
        return (3 * m.px(c, row + i) + m.px(c, row + in) + ((x & 1) ? 2 : 1)) >> 2;
    }
    const int r = y >> 1;                                          // h2v2_fancy_upsample
    const int rf = (y & 1) ? (r + 1 < chh ? r + 1 : chh - 1) : (r > 0 ? r - 1 : 0);
    const long long near = (long long)r * ld, far = (long long)rf * ld;
    const int cs = 3 * m.px(c, near + i) + m.px(c, far + i);
    const int cn = 3 * m.px(c, near + in) + m.px(c, far + in);
    return (3 * cs + cn + ((x & 1) ? 7 : 8)) >> 4;
}

// the B,G,R bytes of pixel (x, y)
template <class M>
__host__ __device__ inline void jpeg_pixel(const JHdr* hd, const M& m, int x, int y, uint8_t* o) {
    const int Y = m.px(0, (long long)y * hd->bw[0] * 8 + x);
    if (hd->ncomp == 1) { o[0] = o[1] = o[2] = (uint8_t)Y; return; }
    const int hs = hd->hmax, vs = hd->vmax;
    const int cb = chroma_at(m, 1, hd->bw[1] * 8, hd->cw[1], hd->chh[1], hs, vs, x, y);
    const int cr = chroma_at(m, 2, hd->bw[2] * 8, hd->cw[2], hd->chh[2], hs, vs, x, y);
    ycc_to_bgr(Y, cb, cr, o);
}

// the component and plane position of block i (of total_blocks)
__host__ __device__ inline void jpeg_block_place(const JHdr* hd, int i, int* c, long long* off, int* ld) {
    int cc = 0;
    if (hd->ncomp == 3) cc = i >= hd->blk_off[2] ? 2 : (i >= hd->blk_off[1] ? 1 : 0);
    const int j = i - hd->blk_off[cc];
    const int by = j / hd->bw[cc], bx = j - by * hd->bw[cc];
    *c = cc;
    *ld = hd->bw[cc] * 8;
    *off = (long long)by * 8 * *ld + bx * 8;
}

__host__ __device__ inline JPage make_page(const JHdr* hd, const uint8_t* data, const int32_t* seg, const JHuff* tables) {
    JPage pg;
    pg.hd = hd;
    pg.data = data;
    pg.seg = seg;
    for (int i = 0; i < 10; ++i) {
        const int c = i < pg.hd->bpm ? pg.hd->mcu_c[i] : 0;
        pg.comp[i] = c;
        pg.dc[i] = tables + (pg.hd->td[c] & 3);
        pg.ac[i] = tables + 4 + (pg.hd->ta[c] & 3);
    }
    return pg;
}

// the bits per thread when `threads` threads share a stream of `total` bits: whole 32-bit words
__host__ __device__ inline int jpeg_range_bits(int total, int threads) {
    return (int)((((long long)total + threads - 1) / threads + 31) & ~31LL);
}

// ---- host parser ------------------------------------------------------------------------------------------------------------
struct RawHuff { bool defined; uint8_t bits[17]; uint8_t val[256]; int count; };

inline int jpeg_be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// jdhuff.c jpeg_make_d_derived_tbl, as lookup tables; false for a table libjpeg rejects
inline bool build_huff(const RawHuff& r, bool dc, JHuff* t) {
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

// Everything in a blob's header that follows from the frame (size, components, luma sampling), the restart interval (0: none) and
// the table selectors; the scan's fields (data_bytes, total_bits, blob_bytes) stay 0.  The inspector writes this header, and
// jpeg_blob_ok accepts no other.
inline void jpeg_geometry(JHdr* out, int W, int H, int nf, int hmax, int vmax, int restart, const int* tq, const int* td, const int* ta) {
    JHdr& hd = *out;
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
        const int chs[3] = {hmax, 1, 1}, cvs[3] = {vmax, 1, 1};
        hd.hmax = hmax; hd.vmax = vmax;
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
    for (int c = 0; c < nf; ++c) { hd.tq[c] = tq[c]; hd.td[c] = td[c]; hd.ta[c] = ta[c]; }
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
    hd.nseg = (int)((total_mcus + hd.restart - 1) / hd.restart);
    hd.off_huff = JB_HUFF;
    hd.off_quant = JB_QUANT;
    hd.off_seg = JB_SEG;
    hd.off_data = (int)((JB_SEG + 4 * ((long long)hd.nseg + 1) + 15) & ~15LL);
}

// rtn_jpeg_inspect without the handle: RTN_OK, or RTN_EINVAL with the reason in why
inline int jpeg_inspect(const uint8_t* f, size_t n, rtn_jpeg_info_t* info, void* blob_out, size_t blob_capacity, char* why,
                        size_t whylen) {
#define JFAIL(...) do { snprintf(why, whylen, __VA_ARGS__); return RTN_EINVAL; } while (0)
    memset(info, 0, sizeof(*info));
    if (n < 4 || f[0] != 0xFF || f[1] != 0xD8) JFAIL("not a JPEG file (no SOI marker)");
    if (n >= ((size_t)1 << 28)) JFAIL("file larger than 256 MiB");

    std::vector<RawHuff> rh(8);
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
        if (pos >= n || f[pos] != 0xFF) JFAIL("corrupt JPEG: expected a marker at byte %zu", pos);
        while (pos < n && f[pos] == 0xFF) ++pos;
        if (pos >= n) JFAIL("truncated JPEG header");
        const int m = f[pos++];
        if (m == 0xD8) JFAIL("corrupt JPEG: second SOI marker");
        if (m == 0xD9) JFAIL("JPEG has no scan (EOI before SOS)");
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) JFAIL("unexpected marker 0x%02X before the scan", m);
        if (pos + 2 > n) JFAIL("truncated JPEG header");
        const int len = jpeg_be16(f + pos);
        if (len < 2 || pos + (size_t)len > n) JFAIL("truncated JPEG header (marker 0x%02X)", m);
        const uint8_t* s = f + pos + 2;
        const int sl = len - 2;
        pos += len;
        switch (m) {
        case 0xC0:
            if (sof) JFAIL("more than one frame header");
            if (sl < 6) JFAIL("corrupt SOF0 segment");
            if (s[0] != 8) JFAIL("%d-bit JPEG (only 8-bit is decoded on the device)", s[0]);
            H = jpeg_be16(s + 1); W = jpeg_be16(s + 3); nf = s[5];
            if (H == 0) JFAIL("JPEG height defined by a DNL marker");
            if (W == 0) JFAIL("JPEG width is 0");
            if (nf != 1 && nf != 3) JFAIL("%d-component JPEG (CMYK/YCCK or other; only 1 or 3 components)", nf);
            if (sl < 6 + 3 * nf) JFAIL("corrupt SOF0 segment");
            for (int c = 0; c < nf; ++c) {
                cid[c] = s[6 + 3 * c]; chs[c] = s[7 + 3 * c] >> 4; cvs[c] = s[7 + 3 * c] & 15; ctq[c] = s[8 + 3 * c];
                if (ctq[c] > 3) JFAIL("corrupt SOF0: quantisation table %d", ctq[c]);
                if (chs[c] < 1 || chs[c] > 4 || cvs[c] < 1 || cvs[c] > 4) JFAIL("corrupt SOF0: sampling factors");
            }
            sof = true;
            break;
        case 0xC1: JFAIL("extended sequential JPEG (SOF1)");
        case 0xC2: JFAIL("progressive JPEG (SOF2)");
        case 0xC3: JFAIL("lossless JPEG (SOF3)");
        case 0xC5: case 0xC6: case 0xC7: JFAIL("hierarchical JPEG (SOF%d)", m - 0xC0);
        case 0xC9: case 0xCA: case 0xCB: case 0xCD: case 0xCE: case 0xCF:
            JFAIL("arithmetic-coded JPEG (SOF%d)", m - 0xC0);
        case 0xCC: JFAIL("arithmetic-coded JPEG (DAC)");
        case 0xDC: JFAIL("JPEG with a DNL marker");
        case 0xC4: {
            int q = 0;
            while (q < sl) {
                if (q + 17 > sl) JFAIL("corrupt DHT segment");
                const int tc = s[q] >> 4, th = s[q] & 15;
                if (tc > 1 || th > 3) JFAIL("corrupt DHT segment (table 0x%02X)", s[q]);
                RawHuff& r = rh[tc * 4 + th];
                int count = 0;
                r.bits[0] = 0;
                for (int l = 1; l <= 16; ++l) { r.bits[l] = s[q + l]; count += s[q + l]; }
                if (count > 256 || q + 17 + count > sl) JFAIL("corrupt DHT segment");
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
                if (pq > 1 || tq > 3) JFAIL("corrupt DQT segment");
                const int need = 1 + 64 * (pq ? 2 : 1);
                if (q + need > sl) JFAIL("corrupt DQT segment");
                for (int k = 0; k < 64; ++k)
                    qt[tq][zz_natural(k)] = (uint16_t)(pq ? jpeg_be16(s + q + 1 + 2 * k) : s[q + 1 + k]);
                qdef[tq] = true;
                q += need;
            }
            break;
        }
        case 0xDD:
            if (sl < 2) JFAIL("corrupt DRI segment");
            restart = jpeg_be16(s);
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
            if (!sof) JFAIL("corrupt JPEG: scan before the frame header");
            if (sl < 1) JFAIL("corrupt SOS segment");
            const int ns = s[0];
            if (sl < 1 + 2 * ns + 3) JFAIL("corrupt SOS segment");
            if (ns != nf) JFAIL("multi-scan JPEG (a scan with %d of %d components)", ns, nf);
            for (int c = 0; c < ns; ++c) {
                if (s[1 + 2 * c] != cid[c]) JFAIL("scan components out of frame order");
                td[c] = s[2 + 2 * c] >> 4; ta[c] = s[2 + 2 * c] & 15;
                if (td[c] > 3 || ta[c] > 3) JFAIL("corrupt SOS: Huffman table index");
            }
            const uint8_t* e = s + 1 + 2 * ns;
            if (e[0] != 0 || e[1] != 63 || e[2] != 0) JFAIL("JPEG scan is not a baseline sequential scan");
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
        if (!jfif && adobe && adobe_transform == 0) JFAIL("Adobe RGB JPEG (transform 0)");
        if (!jfif && !adobe && cid[0] == 82 && cid[1] == 71 && cid[2] == 66) JFAIL("RGB JPEG (component ids R, G, B)");
        if (chs[1] != 1 || cvs[1] != 1 || chs[2] != 1 || cvs[2] != 1 ||
            !((chs[0] == 1 && cvs[0] == 1) || (chs[0] == 2 && cvs[0] == 1) || (chs[0] == 2 && cvs[0] == 2)))
            JFAIL("unsupported sampling factors %dx%d,%dx%d,%dx%d", chs[0], cvs[0], chs[1], cvs[1], chs[2], cvs[2]);
    }
    if ((long long)W * H > JPG_MAX_PIXELS) JFAIL("image too large for the device decoder");
    for (int c = 0; c < nf; ++c) {
        if (!qdef[ctq[c]]) JFAIL("quantisation table %d not defined", ctq[c]);
        if (!rh[td[c]].defined || !rh[4 + ta[c]].defined) JFAIL("Huffman table not defined (standard tables are not assumed)");
    }

    JHdr hd;
    jpeg_geometry(&hd, W, H, nf, chs[0], cvs[0], restart, ctq, td, ta);
    const long long nseg = hd.nseg;
    if (nseg - 1 > (long long)(n - scan_begin) / 2) JFAIL("corrupt JPEG: more restart segments than the file holds");

    // the entropy-coded segment: unstuff, drop RST markers, record segment starts; the scan must end at EOI
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
    if (blob_capacity < bound) JFAIL("blob buffer too small: %zu < %zu bytes", blob_capacity, bound);
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
            if ((m & 7) != (int)(nrst & 7) || ++nrst >= nseg) JFAIL("corrupt JPEG: restart markers out of sequence");
            segs[nrst] = (int32_t)(dn * 8);
            q += 2;
            continue;
        }
        eoi = m == 0xD9;
        if (!eoi) JFAIL("JPEG continues after the scan with marker 0x%02X (multi-scan or DNL)", m);
        break;
    }
    if (!eoi) JFAIL("truncated JPEG (no EOI after the scan)");
    if (nrst != nseg - 1) JFAIL("corrupt JPEG: %lld restart markers, %lld expected", nrst, nseg - 1);
    if (dn == 0) JFAIL("corrupt JPEG: empty scan");
    if (dn * 8 >= ((size_t)1 << 31)) JFAIL("scan too long");
    for (long long i = 1; i < nseg; ++i)
        if (segs[i] <= segs[i - 1]) JFAIL("corrupt JPEG: empty restart segment %lld", i - 1);
    hd.data_bytes = (int)dn;
    hd.total_bits = (int)(dn * 8);
    segs[nseg] = hd.total_bits;
    memset(d + dn, 0, bound - hd.off_data - dn);
    if (segs[nseg] <= segs[nseg - 1]) JFAIL("corrupt JPEG: empty restart segment %lld", nseg - 1);
    hd.blob_bytes = (int)((size_t)hd.off_data + ((dn + 15) & ~(size_t)15) + 16);
    if ((size_t)hd.blob_bytes > bound) JFAIL("internal: blob bound");
    for (int i = 0; i < 8; ++i) {
        JHuff* t = reinterpret_cast<JHuff*>(bl + JB_HUFF) + i;
        if (!rh[i].defined) { memset(t, 0, sizeof(*t)); continue; }
        if (!build_huff(rh[i], i < 4, t)) JFAIL("corrupt JPEG: bad Huffman table 0x%02X", (i >> 2) * 16 + (i & 3));
    }
    uint16_t* qd = reinterpret_cast<uint16_t*>(bl + JB_QUANT);
    for (int t = 0; t < 4; ++t)
        for (int k = 0; k < 64; ++k) qd[t * 64 + k] = qdef[t] ? qt[t][k] : 0;
    memcpy(bl, &hd, sizeof(hd));
    info->blob_bytes = hd.blob_bytes;
    info->scan_bytes = (int64_t)dn;
    return RTN_OK;
#undef JFAIL
}

// Whether b starts a blob that rtn_jpeg_inspect can have written: the header is the one jpeg_geometry gives for its frame, the
// scan's sizes agree with each other, the restart segments are non-empty, in order and end at the stream's last bit, and every
// Huffman table entry keeps a code's length and symbol index in range.  After this check no position that the decode functions
// derive from the header, the tables or the segment offsets leaves the blob's blob_bytes or the page's ws_bytes.
inline bool jpeg_blob_ok(const uint8_t* b) {
    JHdr hd;
    memcpy(&hd, b, sizeof(hd));
    if (hd.magic != JPG_MAGIC || hd.ws_bytes <= 0 || hd.nseg <= 0) return false;
    if (hd.W < 1 || hd.W > 65535 || hd.H < 1 || hd.H > 65535 || (long long)hd.W * hd.H > JPG_MAX_PIXELS) return false;
    if (hd.ncomp != 1 && hd.ncomp != 3) return false;
    if (!((hd.hmax == 1 && hd.vmax == 1) || (hd.ncomp == 3 && hd.hmax == 2 && (hd.vmax == 1 || hd.vmax == 2)))) return false;
    for (int c = 0; c < hd.ncomp; ++c)
        if ((hd.tq[c] | hd.td[c] | hd.ta[c]) & ~3) return false;
    if (hd.restart < 1 || hd.data_bytes < 1 || hd.data_bytes >= (1 << 28)) return false;
    JHdr want;
    jpeg_geometry(&want, hd.W, hd.H, hd.ncomp, hd.hmax, hd.vmax, hd.restart, hd.tq, hd.td, hd.ta);
    want.data_bytes = hd.data_bytes;
    want.total_bits = hd.data_bytes * 8;
    want.blob_bytes = (int)((size_t)want.off_data + (((size_t)hd.data_bytes + 15) & ~(size_t)15) + 16);
    if (memcmp(&want, &hd, sizeof(hd)) != 0) return false;
    const uint8_t* sp = b + hd.off_seg;
    int32_t prev = -1;
    for (int i = 0; i <= hd.nseg; ++i) {
        int32_t v;
        memcpy(&v, sp + 4 * (size_t)i, 4);
        if (v <= prev || (i == 0 && v != 0)) return false;
        prev = v;
    }
    if (prev != hd.total_bits) return false;
    for (int t = 0; t < 8; ++t) {
        JHuff h;
        memcpy(&h, b + JB_HUFF + (size_t)t * sizeof(JHuff), sizeof(h));
        for (int i = 0; i < 512; ++i)
            if ((h.fast[i] >> 8) > 9 || (h.fast[i] != 0 && (h.fast[i] >> 8) == 0)) return false;
        for (int l = 0; l < 18; ++l)
            if (h.valoff[l] < -65536 || h.valoff[l] > 256) return false;
    }
    return true;
}

// ---- the CPU twin -----------------------------------------------------------------------------------------------------------
struct JHostMem {                              // every position is checked against the sizes given; one outside them aborts
    const uint8_t* data; long long data_bytes; // the entropy-coded bytes and their padding: blob_bytes - off_data
    const uint8_t* segs; int nseg;
    int16_t* cf; long long nblocks;
    uint8_t* plane[3]; long long plane_bytes[3];
    [[noreturn]] static void out_of_range(const char* what, long long pos, long long n) {
        fprintf(stderr, "JHostMem: %s %lld outside %lld\n", what, pos, n);
        abort();
    }
    inline uint32_t word(int i) const {
        if (i < 0 || 4 * ((long long)i + 1) > data_bytes) out_of_range("data word", i, data_bytes / 4);
        uint32_t w;
        memcpy(&w, data + 4 * (size_t)i, 4);
        return w;
    }
    inline int seg(int i) const {
        if (i < 0 || i > nseg) out_of_range("segment", i, nseg + 1);
        int32_t v;
        memcpy(&v, segs + 4 * (size_t)i, 4);
        return v;
    }
    inline void zero(long long b) {
        if (b < 0 || b >= nblocks) out_of_range("block", b, nblocks);
        memset(cf + b * 64, 0, 128);
    }
    inline void coef(long long b, int i, int v) {
        if (b < 0 || b >= nblocks || i < 0 || i > 63) out_of_range("coefficient", b * 64 + i, nblocks * 64);
        cf[b * 64 + i] = (int16_t)v;
    }
    inline const int16_t* block(long long b) const {
        if (b < 0 || b >= nblocks) out_of_range("block", b, nblocks);
        return cf + b * 64;
    }
    inline void row8(int c, long long off, uint32_t lo, uint32_t hi) {
        if (c < 0 || c > 2 || off < 0 || off + 8 > plane_bytes[c]) out_of_range("plane row", off, c < 0 || c > 2 ? 0 : plane_bytes[c]);
        for (int i = 0; i < 4; ++i) { plane[c][off + i] = (uint8_t)(lo >> (8 * i)); plane[c][off + 4 + i] = (uint8_t)(hi >> (8 * i)); }
    }
    inline int px(int c, long long off) const {
        if (c < 0 || c > 2 || off < 0 || off >= plane_bytes[c]) out_of_range("plane sample", off, c < 0 || c > 2 ? 0 : plane_bytes[c]);
        return plane[c][off];
    }
};

struct JHostStats { int passes, busy; };       // synchronisation passes run; threads whose bit range was not empty

// rtn_jpeg_decode_host without the error text: jpeg_huffman_kernel's algorithm for `threads` virtual threads, one after another
// (the same range rule, pass loop, segmented scan and writing pass), then the IDCT per block and the colour step per pixel.
// RTN_OK with *status = 0 and the page in out, or *status = 1 or 2 and out not written; RTN_EINVAL (*why: the reason) otherwise.
inline int jpeg_decode_host(const void* blob, int threads, uint8_t* out, size_t out_bytes, int32_t* status, const char** why,
                            JHostStats* stats = nullptr) {
    const uint8_t* bl = static_cast<const uint8_t*>(blob);
    if (!jpeg_blob_ok(bl)) { *why = "not an rtn_jpeg_inspect blob"; return RTN_EINVAL; }
    if (threads < 1 || threads > JPG_HOST_THREADS_MAX) { *why = "threads outside 1 .. 65536"; return RTN_EINVAL; }
    JHdr hd;
    memcpy(&hd, bl, sizeof(hd));
    if (out_bytes != (size_t)hd.W * hd.H * 3) { *why = "out_bytes is not height * width * 3"; return RTN_EINVAL; }
    std::vector<JHuff> tabs(8);
    memcpy(tabs.data(), bl + JB_HUFF, 8 * sizeof(JHuff));
    const JPage pg = make_page(&hd, nullptr, nullptr, tabs.data());     // the twin reads data and segments through its context only
    std::vector<int16_t> coef((size_t)hd.total_blocks * 64, 0);
    std::vector<uint8_t> planes[3];
    JHostMem m;
    m.data = bl + hd.off_data; m.data_bytes = (long long)hd.blob_bytes - hd.off_data;
    m.segs = bl + hd.off_seg; m.nseg = hd.nseg;
    m.cf = coef.data(); m.nblocks = hd.total_blocks;
    for (int c = 0; c < 3; ++c) {
        m.plane_bytes[c] = c < hd.ncomp ? (long long)hd.bw[c] * 8 * hd.bh[c] * 8 : 0;
        planes[c].assign((size_t)m.plane_bytes[c], 0);
        m.plane[c] = planes[c].data();
    }
    const int T = threads, total = hd.total_bits;
    const int L = jpeg_range_bits(total, T);
    auto rstart_of = [&](int t) { const long long s = (long long)t * L; return (int)(s < total ? s : total); };
    auto rend_of = [&](int t) { const long long e = (long long)rstart_of(t) + L; return (int)(e < total ? e : total); };
    std::vector<JState> entry(T), ex(T), ex_prev(T);
    std::vector<JSync> res(T);
    int busy = 0;
    for (int t = 0; t < T; ++t) { entry[t] = JState{rstart_of(t), 0, 0}; busy += rend_of(t) > rstart_of(t); }
    int passes = 0;
    for (int pass = 0; pass <= T; ++pass) {
        ++passes;
        bool changed = false;
        for (int t = 0; t < T; ++t) {
            bool same = pass > 0;                                   // a range's result depends on its entry state alone: a thread
            if (pass > 0 && t > 0) {                                // that enters where it did in the last pass leaves where it did
                const JState e = ex_prev[t - 1];
                same = e.p == entry[t].p && e.b == entry[t].b && e.k == entry[t].k;
                entry[t] = e;
            }
            if (!same) res[t] = jpeg_sync_range(pg, m, entry[t], rend_of(t));
            const JState e = res[t].exit;
            if (pass > 0 && (e.p != ex_prev[t].p || e.b != ex_prev[t].b || e.k != ex_prev[t].k)) changed = true;
            ex[t] = e;
        }
        ex_prev = ex;
        if (pass > 0 && !changed) break;
    }
    if (stats) { stats->passes = passes; stats->busy = busy; }
    // segmented inclusive scan over threads of (reset, blocks, DC sums)
    struct Sc { int f, v[4]; };
    std::vector<Sc> cur(T), nxt(T);
    for (int t = 0; t < T; ++t) cur[t] = Sc{res[t].reset, {res[t].cnt, res[t].dc[0], res[t].dc[1], res[t].dc[2]}};
    for (long long d = 1; d < T; d <<= 1) {
        for (int t = 0; t < T; ++t) {
            nxt[t] = cur[t];
            if (t >= d && !cur[t].f) {
                nxt[t].f = cur[t - d].f;
                for (int j = 0; j < 4; ++j) nxt[t].v[j] += cur[t - d].v[j];
            }
        }
        cur.swap(nxt);
    }
    int bad = 0;
    for (int t = 0; t < T; ++t) {
        int ord = 0, p0 = 0, p1 = 0, p2 = 0;
        if (t > 0) { ord = cur[t - 1].v[0]; p0 = cur[t - 1].v[1]; p1 = cur[t - 1].v[2]; p2 = cur[t - 1].v[3]; }
        const int err = jpeg_write_range(pg, m, entry[t], rend_of(t), ord, p0, p1, p2);
        if (err) bad = err;
    }
    if (bad == 0) {
        for (int i = 0; i < hd.total_blocks; ++i) {
            int c, ld;
            long long off;
            jpeg_block_place(&hd, i, &c, &off, &ld);
            uint16_t q[64];
            memcpy(q, bl + hd.off_quant + 128 * (size_t)(hd.tq[c] & 3), sizeof(q));
            if (!idct_islow<long long>(m, i, q, c, off, ld)) bad = 2;
        }
    }
    *status = bad;
    if (bad) return RTN_OK;
    for (int y = 0; y < hd.H; ++y)
        for (int x = 0; x < hd.W; ++x) {
            const size_t i = (size_t)y * hd.W + x;
            if (3 * i + 3 > out_bytes) JHostMem::out_of_range("output pixel", (long long)i, (long long)(out_bytes / 3));
            jpeg_pixel(&hd, m, x, y, out + 3 * i);
        }
    return RTN_OK;
}
