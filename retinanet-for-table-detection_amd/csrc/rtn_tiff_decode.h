// rtn_tiff_decode.h — the text that the device TIFF decoder (csrc/rtn_tiff.hip) and its CPU twin share: the blob layout,
// the file inspector, and the decode functions (PackBits, TIFF-LZW, CCITT T.6 / Group 4, the Deflate call into pi_run, the pixel
// stage) as __host__ __device__ functions.  A plain C++17 compiler compiles this header (no HIP), so that csrc/rtn_tiff.hip and a
// stand-alone sanitizer build (tools/tiff_fuzz.cpp) compile the same text.
//
// Every access to memory whose position comes from file bytes goes through a memory context `M` that stands for ONE strip: its
// compressed bytes (`in`), its part of the page's packed rows (`out`, rows * rowbytes bytes) and the decoder's tables:
//   uint32_t in(uint32_t i)                          compressed byte i; 0 at or past the strip's last byte
//   uint32_t in32(uint32_t i)                        bytes i .. i + 3 (i a multiple of 4) as one big-endian number, zeros past the last byte
//   uint32_t word(uint32_t i)                        little-endian word i of the bytes behind the 2-byte zlib header, zero padded
//   uint32_t get(uint32_t pos)                       out[pos]
//   void put(uint32_t pos, uint32_t byte)            out[pos] = byte
//   void fill(uint32_t pos, uint32_t n, uint32_t b)  out[pos + i] = b, i < n
//   void stored(uint32_t pos, uint32_t at, uint32_t n)   out[pos + i] = compressed byte at + i (for Deflate: at counts behind the header)
//   void match(uint32_t pos, uint32_t d, uint32_t n) out[pos + i] = out[pos + i - d], i = 0 .. n-1 in order (d <= pos)
//   void copy(uint32_t pos, uint32_t src, uint32_t n, bool kwk)   out[pos + i] = out[src + i]; kwk: the last byte is out[src] instead
//   void tab(uint32_t code, uint32_t off, uint32_t len), uint32_t tab_off(code), tab_len(code)     the LZW string table, code < 4096
//   void run_set(int colour, uint32_t i, uint32_t v), uint32_t run(int colour, uint32_t i)         the T.4 run lookup, i < 8192
//   void row_begin(y, rowbytes, &cur, &ref), uint32_t rget(pos), void ror(pos, mask), void row_end(y, rowbytes, cur)
//                                                    Group 4's row under construction and the row before it: see tf_g4_strip
//   int lane(), int lanes(), void sync(), uint32_t uni(uint32_t), bool boundary(uint64_t)          as in csrc/rtn_png_inflate.h
//   uint32_t adler_join(uint32_t a, uint32_t b, uint32_t n)   the Adler-32 of n bytes from the lanes' sums of d[i] and (n - i) d[i]
// The decoders hand a position to the context only after checking it against the strip's sizes; the kernels' context (TFDevMem in
// rtn_tiff.hip) does the plain loads and stores, the twin's (TFHostMem below) checks every position again and aborts on one outside.
// tf_packbits, tf_lzw, tf_none and tf_deflate are uniform across the lanes of a wave (every lane computes the same values, only the
// memory operations are split); tf_g4_row reads the row written before it and is run by one lane.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "rtn.h"
#include "rtn_png_inflate.h"

constexpr uint32_t TF_MAGIC = 0x46495452u;     // "RTIF"

enum {                                         // status bits above those of csrc/rtn_png_inflate.h (a Deflate strip sets PI_* bits)
    TF_CODE = 1 << 16,     // an invalid code: LZW code above the next free one or a full table, no T.4 / T.6 code, a misplaced empty run
    TF_RUN = 1 << 17,      // a run past the row's end, or a vertical mode that does not move forward
    TF_SHORT = 1 << 18,    // the strip ended (EOI, EOFB, its last byte) before its rows were full
    TF_OVER = 1 << 19,     // a string, run or block past the strip's last row
    TF_CLEAR = 1 << 20,    // an LZW code before the first Clear
    TF_EXT = 1 << 21,      // Group 4's extension (uncompressed mode)
    TF_ZLIB = 1 << 22,     // no zlib header, or no Adler-32 behind the final block
};

enum { TF_BILEVEL = 0, TF_GRAY = 1, TF_PALETTE = 2, TF_RGB = 3 };
enum { TF_NONE = 1, TF_G4 = 4, TF_LZW = 5, TF_DEFLATE = 8, TF_PACKBITS = 32773 };

struct TFHdr {                                 // 64 bytes at the start of every blob
    uint32_t magic;
    int32_t W, H;
    uint32_t compression;                      // TF_NONE .. TF_PACKBITS (32946 is stored as 8)
    uint32_t layout;                           // TF_BILEVEL .. TF_RGB
    uint32_t invert;                           // 1: PhotometricInterpretation 0
    uint32_t predictor;                        // 1 or 2
    uint32_t nstrips;
    uint32_t rowbytes;                         // bytes of one packed row: ceil(W / 8), W or 3 W
    uint32_t off_table, off_pal, off_data;     // TFStrip[nstrips]; 768 bytes B,G,R (palette pages, else off_pal = 0); the strips' bytes
    int64_t blob_bytes, ws_bytes;
};
static_assert(sizeof(TFHdr) == 64, "TFHdr layout");

struct TFStrip {
    uint32_t off;                              // behind off_data; a multiple of 4 (Deflate: 2 more, so that the words behind the zlib header are aligned)
    uint32_t bytes;
    uint32_t row0, rows;                       // rows row0 .. row0 + rows - 1 of the page; the strips follow one another
};

__host__ __device__ inline uint32_t tf_samples(uint32_t layout) { return layout == TF_RGB ? 3u : 1u; }

// The per-page workspace: the packed rows (H * rowbytes), then one status word per strip.
__host__ __device__ inline long long tf_ws_status(long long H, long long rowbytes) { return (H * rowbytes + 255) & ~255ll; }
__host__ __device__ inline long long tf_ws_bytes(long long H, long long rowbytes, long long nstrips) {
    return tf_ws_status(H, rowbytes) + ((4 * nstrips + 255) & ~255ll);
}

// A blob that every later step may follow without another check: sizes, table, strips inside the data, rows that tile the page.
inline bool tf_blob_ok(const void* blob, size_t bytes) {
    if (!blob || bytes < sizeof(TFHdr)) return false;
    TFHdr hd;
    memcpy(&hd, blob, sizeof(hd));
    if (hd.magic != TF_MAGIC || hd.blob_bytes < (int64_t)sizeof(TFHdr) || (uint64_t)hd.blob_bytes > bytes || (hd.blob_bytes & 15)) return false;
    if (hd.W < 1 || hd.H < 1 || hd.W > 65535 || hd.H > 65535 || hd.layout > TF_RGB || hd.invert > 1u) return false;
    const uint32_t c = hd.compression;
    if (c != TF_NONE && c != TF_G4 && c != TF_LZW && c != TF_DEFLATE && c != TF_PACKBITS) return false;
    if (c == TF_G4 && hd.layout != TF_BILEVEL) return false;
    if (hd.predictor != 1u && !(hd.predictor == 2u && hd.layout != TF_BILEVEL && (c == TF_LZW || c == TF_DEFLATE))) return false;
    if (hd.invert && (hd.layout == TF_PALETTE || hd.layout == TF_RGB)) return false;
    const unsigned long long rb = hd.layout == TF_BILEVEL ? ((unsigned long long)hd.W + 7u) >> 3 : (unsigned long long)hd.W * tf_samples(hd.layout);
    if (rb != hd.rowbytes || rb * (unsigned long long)hd.H >= (1ull << 31)) return false;
    if (hd.nstrips < 1u || hd.nstrips > (uint32_t)hd.H) return false;
    const uint64_t size = (uint64_t)hd.blob_bytes;
    if (hd.off_table != sizeof(TFHdr) || (uint64_t)hd.off_table + (uint64_t)hd.nstrips * sizeof(TFStrip) > size) return false;
    uint64_t at = (uint64_t)hd.off_table + (uint64_t)hd.nstrips * sizeof(TFStrip);
    if (hd.layout == TF_PALETTE) {
        if (hd.off_pal != at) return false;
        at += 768;
    } else if (hd.off_pal != 0) return false;
    if (hd.off_data != ((at + 15u) & ~15ull) || hd.off_data + 16ull > size) return false;
    if (hd.ws_bytes != tf_ws_bytes(hd.H, hd.rowbytes, hd.nstrips)) return false;
    const uint64_t data = size - hd.off_data - 8u;                     // 8 bytes of padding behind the last strip
    const uint8_t* tb = static_cast<const uint8_t*>(blob) + hd.off_table;
    uint64_t row = 0;
    for (uint32_t s = 0; s < hd.nstrips; ++s) {
        TFStrip st;
        memcpy(&st, tb + (size_t)s * sizeof(TFStrip), sizeof(st));
        if ((st.off & 3u) != (c == TF_DEFLATE ? 2u : 0u)) return false;
        if ((uint64_t)st.off + st.bytes > data) return false;
        if (st.row0 != row || st.rows < 1u || st.rows > (uint32_t)hd.H - st.row0) return false;
        row += st.rows;
    }
    return row == (uint64_t)hd.H;
}

// ---- PackBits ------------------------------------------------------------------------------------------------------------------------------
// Literal and repeat runs may cross row boundaries (the strip is one buffer); a run past the strip's last byte, or input that ends
// before the strip is full, is flagged.  Bytes behind a full strip are not looked at.
template <class M>
__host__ __device__ inline uint32_t tf_packbits(M& m, uint32_t in_bytes, uint32_t want) {
    uint32_t at = 0, pos = 0;
    while (pos < want) {                                               // every turn consumes at least one byte
        if (at >= in_bytes) return TF_SHORT;
        const uint32_t n = m.uni(m.in(at++));
        if (n == 128u) continue;
        if (n > 128u) {
            const uint32_t len = 257u - n;
            if (at >= in_bytes) return TF_SHORT;
            if (len > want - pos) return TF_OVER;
            m.fill(pos, len, m.uni(m.in(at++)));
            pos += len;
        } else {
            const uint32_t len = n + 1u;
            if (len > in_bytes - at) return TF_SHORT;
            if (len > want - pos) return TF_OVER;
            m.stored(pos, at, len);
            at += len;
            pos += len;
        }
    }
    return 0u;
}

// ---- no compression ------------------------------------------------------------------------------------------------------------------------
template <class M>
__host__ __device__ inline uint32_t tf_none(M& m, uint32_t in_bytes, uint32_t want) {
    if (in_bytes < want) return TF_SHORT;
    m.stored(0u, 0u, want);
    return 0u;
}

// ---- TIFF-LZW (MSB first, early change) ------------------------------------------------------------------------------------------------------
// The string of code c >= 258 is out[tab_off(c) .. + tab_len(c)): every string the table holds has been written once, in full, when
// its entry was made (the entry of the code after string P is P + the next string's first byte, which is what follows P in out).
// Strict where libtiff only warns: the first code must be Clear, the code after a Clear a byte, the table must not fill up, the last
// string must end with the strip, and EOI or the end of the bytes before that is flagged.  Bytes behind a full strip are not looked at.
template <class M>
__host__ __device__ inline uint32_t tf_lzw(M& m, uint32_t in_bytes, uint32_t want) {
    const uint64_t nbits = (uint64_t)in_bytes * 8u;
    uint64_t bit = 0;
    uint32_t width = 9, free_code = 258, pos = 0, prev_off = 0, prev_len = 0;
    bool cleared = false;
    while (pos < want) {                                               // every turn consumes at least 9 bits
        if (bit + width > nbits) return TF_SHORT;
        const uint32_t at = (uint32_t)(bit >> 3);
        const uint32_t w24 = m.in(at) << 16 | m.in(at + 1u) << 8 | m.in(at + 2u);
        const uint32_t code = m.uni((w24 >> (24u - width - (uint32_t)(bit & 7u))) & ((1u << width) - 1u));
        bit += width;
        if (code == 257u) return TF_SHORT;
        if (code == 256u) {
            width = 9; free_code = 258; prev_len = 0; cleared = true;
            continue;
        }
        if (!cleared) return TF_CLEAR;
        if (prev_len == 0u) {                                          // the first code behind a Clear
            if (code > 255u) return TF_CODE;
            m.put(pos, code);
            prev_off = pos; prev_len = 1u;
            ++pos;
            continue;
        }
        uint32_t len;
        if (code < 256u) {
            len = 1u;
            m.put(pos, code);
        } else if (code < free_code) {
            const uint32_t off = m.uni(m.tab_off(code));
            len = m.uni(m.tab_len(code));
            if (len > want - pos) return TF_OVER;
            if ((uint64_t)off + len > pos) return TF_CODE;             // cannot happen: an entry ends where it was made
            m.copy(pos, off, len, false);
        } else if (code == free_code) {                                // the string being defined: the last string and its first byte
            len = prev_len + 1u;
            if (len > want - pos) return TF_OVER;
            m.copy(pos, prev_off, len, true);
        } else {
            return TF_CODE;
        }
        if (free_code >= 4096u) return TF_CODE;
        m.tab(free_code, prev_off, prev_len + 1u);
        ++free_code;
        if (free_code > (1u << width) - 2u && width < 12u) ++width;
        prev_off = pos; prev_len = len;
        pos += len;
    }
    return 0u;
}

// ---- Deflate: one zlib stream per strip --------------------------------------------------------------------------------------------------------
// Adler-32 of out[0 .. n), each lane summing every lanes()-th byte.
template <class M>
__host__ __device__ inline uint32_t tf_adler(M& m, uint32_t n) {
    m.sync();
    uint32_t a = 0;
    unsigned long long b = 0;
    for (uint32_t i = (uint32_t)m.lane(); i < n; i += (uint32_t)m.lanes()) {
        const uint32_t d = m.get(i);
        a += d;
        b += (unsigned long long)(n - i) * d;
        if ((i & 0xffffu) < (uint32_t)m.lanes()) { a %= 65521u; b %= 65521u; }   // once per 65536 bytes: neither sum overflows
    }
    return m.adler_join(a % 65521u, (uint32_t)(b % 65521u), n);
}

template <class M>
__host__ __device__ inline uint32_t tf_deflate(M& m, PiTables& T, uint32_t in_bytes, uint32_t want) {
    if (in_bytes < 6u) return TF_ZLIB;
    const uint32_t cmf = m.in(0), flg = m.in(1);
    if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || (flg & 32u) || ((cmf << 8 | flg) % 31u) != 0u) return TF_ZLIB;
    const uint32_t payload = in_bytes - 2u;
    PiRun run = {0ull, 0u, 0u};
    const int rc = pi_run(m, T, payload, 0ull, 0u, want, &run);
    if (rc) return (uint32_t)rc;
    if (!run.final) return (uint32_t)PI_CHAIN;
    if (run.out != want) return (uint32_t)PI_LENGTH;
    const uint64_t end = (run.end_bit + 7u) >> 3;
    if (end + 4u > payload) return TF_ZLIB;
    const uint32_t e = 2u + (uint32_t)end;
    const uint32_t stored = m.in(e) << 24 | m.in(e + 1u) << 16 | m.in(e + 2u) << 8 | m.in(e + 3u);
    return tf_adler(m, want) == stored ? 0u : (uint32_t)PI_ADLER;
}

// ---- CCITT T.6 (Group 4) ---------------------------------------------------------------------------------------------------------------------
// The T.4 run codes, as code << 4 | length; entry i < 64 is the terminating code of run i, entry 64 + k the make-up code of run 64 (k + 1).
__host__ __device__ inline uint32_t tf_white_code(int i) {
    constexpr uint32_t t[91] = {
        0x35 << 4 | 8, 0x07 << 4 | 6, 0x07 << 4 | 4, 0x08 << 4 | 4, 0x0b << 4 | 4, 0x0c << 4 | 4, 0x0e << 4 | 4, 0x0f << 4 | 4,
        0x13 << 4 | 5, 0x14 << 4 | 5, 0x07 << 4 | 5, 0x08 << 4 | 5, 0x08 << 4 | 6, 0x03 << 4 | 6, 0x34 << 4 | 6, 0x35 << 4 | 6,
        0x2a << 4 | 6, 0x2b << 4 | 6, 0x27 << 4 | 7, 0x0c << 4 | 7, 0x08 << 4 | 7, 0x17 << 4 | 7, 0x03 << 4 | 7, 0x04 << 4 | 7,
        0x28 << 4 | 7, 0x2b << 4 | 7, 0x13 << 4 | 7, 0x24 << 4 | 7, 0x18 << 4 | 7, 0x02 << 4 | 8, 0x03 << 4 | 8, 0x1a << 4 | 8,
        0x1b << 4 | 8, 0x12 << 4 | 8, 0x13 << 4 | 8, 0x14 << 4 | 8, 0x15 << 4 | 8, 0x16 << 4 | 8, 0x17 << 4 | 8, 0x28 << 4 | 8,
        0x29 << 4 | 8, 0x2a << 4 | 8, 0x2b << 4 | 8, 0x2c << 4 | 8, 0x2d << 4 | 8, 0x04 << 4 | 8, 0x05 << 4 | 8, 0x0a << 4 | 8,
        0x0b << 4 | 8, 0x52 << 4 | 8, 0x53 << 4 | 8, 0x54 << 4 | 8, 0x55 << 4 | 8, 0x24 << 4 | 8, 0x25 << 4 | 8, 0x58 << 4 | 8,
        0x59 << 4 | 8, 0x5a << 4 | 8, 0x5b << 4 | 8, 0x4a << 4 | 8, 0x4b << 4 | 8, 0x32 << 4 | 8, 0x33 << 4 | 8, 0x34 << 4 | 8,
        // make-up 64 .. 1728
        0x1b << 4 | 5, 0x12 << 4 | 5, 0x17 << 4 | 6, 0x37 << 4 | 7, 0x36 << 4 | 8, 0x37 << 4 | 8, 0x64 << 4 | 8, 0x65 << 4 | 8,
        0x68 << 4 | 8, 0x67 << 4 | 8, 0xcc << 4 | 9, 0xcd << 4 | 9, 0xd2 << 4 | 9, 0xd3 << 4 | 9, 0xd4 << 4 | 9, 0xd5 << 4 | 9,
        0xd6 << 4 | 9, 0xd7 << 4 | 9, 0xd8 << 4 | 9, 0xd9 << 4 | 9, 0xda << 4 | 9, 0xdb << 4 | 9, 0x98 << 4 | 9, 0x99 << 4 | 9,
        0x9a << 4 | 9, 0x18 << 4 | 6, 0x9b << 4 | 9};
    return t[i];
}
__host__ __device__ inline uint32_t tf_black_code(int i) {
    constexpr uint32_t t[91] = {
        0x37 << 4 | 10, 0x02 << 4 | 3, 0x03 << 4 | 2, 0x02 << 4 | 2, 0x03 << 4 | 3, 0x03 << 4 | 4, 0x02 << 4 | 4, 0x03 << 4 | 5,
        0x05 << 4 | 6, 0x04 << 4 | 6, 0x04 << 4 | 7, 0x05 << 4 | 7, 0x07 << 4 | 7, 0x04 << 4 | 8, 0x07 << 4 | 8, 0x18 << 4 | 9,
        0x17 << 4 | 10, 0x18 << 4 | 10, 0x08 << 4 | 10, 0x67 << 4 | 11, 0x68 << 4 | 11, 0x6c << 4 | 11, 0x37 << 4 | 11, 0x28 << 4 | 11,
        0x17 << 4 | 11, 0x18 << 4 | 11, 0xca << 4 | 12, 0xcb << 4 | 12, 0xcc << 4 | 12, 0xcd << 4 | 12, 0x68 << 4 | 12, 0x69 << 4 | 12,
        0x6a << 4 | 12, 0x6b << 4 | 12, 0xd2 << 4 | 12, 0xd3 << 4 | 12, 0xd4 << 4 | 12, 0xd5 << 4 | 12, 0xd6 << 4 | 12, 0xd7 << 4 | 12,
        0x6c << 4 | 12, 0x6d << 4 | 12, 0xda << 4 | 12, 0xdb << 4 | 12, 0x54 << 4 | 12, 0x55 << 4 | 12, 0x56 << 4 | 12, 0x57 << 4 | 12,
        0x64 << 4 | 12, 0x65 << 4 | 12, 0x52 << 4 | 12, 0x53 << 4 | 12, 0x24 << 4 | 12, 0x37 << 4 | 12, 0x38 << 4 | 12, 0x27 << 4 | 12,
        0x28 << 4 | 12, 0x58 << 4 | 12, 0x59 << 4 | 12, 0x2b << 4 | 12, 0x2c << 4 | 12, 0x5a << 4 | 12, 0x66 << 4 | 12, 0x67 << 4 | 12,
        // make-up 64 .. 1728
        0x0f << 4 | 10, 0xc8 << 4 | 12, 0xc9 << 4 | 12, 0x5b << 4 | 12, 0x33 << 4 | 12, 0x34 << 4 | 12, 0x35 << 4 | 12, 0x6c << 4 | 13,
        0x6d << 4 | 13, 0x4a << 4 | 13, 0x4b << 4 | 13, 0x4c << 4 | 13, 0x4d << 4 | 13, 0x72 << 4 | 13, 0x73 << 4 | 13, 0x74 << 4 | 13,
        0x75 << 4 | 13, 0x76 << 4 | 13, 0x77 << 4 | 13, 0x52 << 4 | 13, 0x53 << 4 | 13, 0x54 << 4 | 13, 0x55 << 4 | 13, 0x5a << 4 | 13,
        0x5b << 4 | 13, 0x64 << 4 | 13, 0x65 << 4 | 13};
    return t[i];
}
// The make-up codes of runs 1792 + 64 k, k = 0 .. 12, of either colour.
__host__ __device__ inline uint32_t tf_long_code(int k) {
    constexpr uint32_t t[13] = {0x08 << 4 | 11, 0x0c << 4 | 11, 0x0d << 4 | 11, 0x12 << 4 | 12, 0x13 << 4 | 12, 0x14 << 4 | 12, 0x15 << 4 | 12,
                                0x16 << 4 | 12, 0x17 << 4 | 12, 0x1c << 4 | 12, 0x1d << 4 | 12, 0x1e << 4 | 12, 0x1f << 4 | 12};
    return t[k];
}
constexpr int TF_RUN_CODES = 91 + 13;          // per colour
constexpr int TF_RUN_BITS = 13;                // the lookup is indexed by the next 13 bits: run << 4 | code length, 0 = no code

// Fill this lane's share of both lookups (they must be zero before; m.sync() behind the call makes them readable).
template <class M>
__host__ __device__ inline void tf_run_tables(M& m) {
    for (int j = m.lane(); j < 2 * TF_RUN_CODES; j += m.lanes()) {
        const int colour = j / TF_RUN_CODES, i = j % TF_RUN_CODES;
        const uint32_t e = i < 91 ? (colour ? tf_black_code(i) : tf_white_code(i)) : tf_long_code(i - 91);
        const uint32_t run = i < 64 ? (uint32_t)i : i < 91 ? 64u * (uint32_t)(i - 63) : 1792u + 64u * (uint32_t)(i - 91);
        const uint32_t len = e & 15u, first = (e >> 4) << (TF_RUN_BITS - len);
        for (uint32_t k = 0; k < (1u << (TF_RUN_BITS - len)); ++k) m.run_set(colour, first + k, run << 4 | len);
    }
}

struct TFBits {                                // MSB-first reader over in32(); zeros behind the last byte, consumed() tells the caller
    uint64_t acc;
    int cnt;
    uint32_t next;                             // the next byte to load, a multiple of 4
    template <class M>
    __host__ __device__ inline uint32_t peek(M& m, int k) {           // k <= 16
        if (cnt <= 32) { acc |= (uint64_t)m.in32(next) << (32 - cnt); cnt += 32; next += 4u; }
        return (uint32_t)(acc >> (64 - k));
    }
    __host__ __device__ inline void drop(int k) { acc <<= k; cnt -= k; }
    __host__ __device__ inline uint64_t consumed() const { return (uint64_t)next * 8u - (uint64_t)cnt; }
};

// First x' >= x (x >= 0) of the row at `base` whose pixel is v, or W.
template <class M>
__host__ __device__ inline int tf_find(M& m, uint32_t base, int x, int W, uint32_t v) {
    while (x < W) {
        uint32_t b = m.rget(base + (uint32_t)(x >> 3));
        if (!v) b = ~b;
        b &= 0xffu >> (x & 7);
        if (b) {
            const int p = (x & ~7) + (__builtin_clz(b) - 24);
            return p < W ? p : W;
        }
        x = (x & ~7) + 8;
    }
    return W;
}

// black pixels [x0, x1) of the (zeroed) row at base; 0 <= x0 <= x1 <= W
template <class M>
__host__ __device__ inline void tf_black(M& m, uint32_t base, int x0, int x1) {
    if (x0 >= x1) return;
    const int b0 = x0 >> 3, b1 = (x1 - 1) >> 3;
    const uint32_t head = 0xffu >> (x0 & 7), tail = (0xff00u >> (((x1 - 1) & 7) + 1)) & 0xffu;
    if (b0 == b1) { m.ror(base + (uint32_t)b0, head & tail); return; }
    m.ror(base + (uint32_t)b0, head);
    for (int b = b0 + 1; b < b1; ++b) m.ror(base + (uint32_t)b, 0xffu);
    m.ror(base + (uint32_t)b1, tail);
}

// One run length of `colour`: make-up codes, then a terminating code.  Returns TF_* bits; *len <= W.
template <class M>
__host__ __device__ inline uint32_t tf_g4_run(M& m, TFBits& r, uint64_t nbits, int colour, int W, int* len) {
    int total = 0;
    for (;;) {                                                         // every code consumes at least 2 bits
        const uint32_t e = m.run(colour, r.peek(m, TF_RUN_BITS));
        if (!e) return TF_CODE;
        r.drop((int)(e & 15u));
        if (r.consumed() > nbits) return TF_SHORT;
        total += (int)(e >> 4);
        if (total > W) return TF_RUN;
        if ((e >> 4) < 64u) break;
    }
    *len = total;
    return 0u;
}

// One row into the zeroed row at `cur`, coded against the row at `ref` (has_ref false: an all-white row).  a0 = -1 stands for the
// imaginary white pixel before the row.  Strict where libtiff goes on: every vertical mode must move forward, and an empty run is
// accepted only where an encoder writes one (the white run of a row that starts black, the second run where the row ends).
template <class M>
__host__ __device__ inline uint32_t tf_g4_row(M& m, TFBits& r, uint64_t nbits, uint32_t cur, uint32_t ref, bool has_ref, int W) {
    int a0 = -1;
    uint32_t colour = 0;
    while (a0 < W) {                                                   // every mode consumes at least 1 bit
        const uint32_t p = r.peek(m, 7);
        int mode, d = 0, bits;                                         // 0 pass, 1 horizontal, 2 vertical
        if (p & 64u) { mode = 2; bits = 1; }
        else if ((p >> 4) == 3u) { mode = 2; d = 1; bits = 3; }
        else if ((p >> 4) == 2u) { mode = 2; d = -1; bits = 3; }
        else if ((p >> 4) == 1u) { mode = 1; bits = 3; }
        else if ((p >> 3) == 1u) { mode = 0; bits = 4; }
        else if ((p >> 1) == 3u) { mode = 2; d = 2; bits = 6; }
        else if ((p >> 1) == 2u) { mode = 2; d = -2; bits = 6; }
        else if (p == 3u) { mode = 2; d = 3; bits = 7; }
        else if (p == 2u) { mode = 2; d = -3; bits = 7; }
        else if (p == 1u) return TF_EXT;
        else return r.consumed() + 7u > nbits ? TF_SHORT : TF_CODE;    // EOFB (or nothing) where a row should start
        r.drop(bits);
        if (r.consumed() > nbits) return TF_SHORT;
        const int start = a0 < 0 ? 0 : a0;
        if (mode == 1) {
            int r1, r2;
            if (const uint32_t rc = tf_g4_run(m, r, nbits, (int)colour, W, &r1)) return rc;
            if (const uint32_t rc = tf_g4_run(m, r, nbits, (int)(colour ^ 1u), W, &r2)) return rc;
            if ((long long)start + r1 + r2 > W) return TF_RUN;
            if ((r1 == 0 && a0 >= 0) || (r2 == 0 && start + r1 + r2 != W)) return TF_CODE;
            if (colour) tf_black(m, cur, start, start + r1);
            else tf_black(m, cur, start + r1, start + r1 + r2);
            a0 = start + r1 + r2;
            continue;
        }
        int b1 = W, b2 = W;                                            // the reference row's next change to the other colour, and back
        if (has_ref) {
            const int j = a0 < 0 ? (colour ? tf_find(m, ref, 0, W, 1u) : -1) : tf_find(m, ref, a0, W, colour);
            b1 = j >= W ? W : tf_find(m, ref, j + 1, W, colour ^ 1u);
            b2 = b1 >= W ? W : tf_find(m, ref, b1 + 1, W, colour);
        }
        if (mode == 0) {
            if (colour) tf_black(m, cur, start, b2);
            a0 = b2;
        } else {
            const int a1 = b1 + d;
            if (a1 <= a0 || a1 > W) return TF_RUN;
            if (colour) tf_black(m, cur, start, a1);
            a0 = a1;
            colour ^= 1u;
        }
    }
    return 0u;
}

// The rows of one strip (lookups filled); the first row's reference is white.  Every lane walks the rows: row_begin gives the
// position of a zeroed row y and of the row before it (the twin: in the strip's rows; the kernel: in two rows of LDS), lane 0 decodes
// the row, row_end puts it into the strip's rows.  The bytes behind the last row (EOFB, padding) are not looked at.
template <class M>
__host__ __device__ inline uint32_t tf_g4_strip(M& m, uint32_t in_bytes, int W, uint32_t rows, uint32_t rowbytes) {
    TFBits r = {0ull, 0, 0u};
    const uint64_t nbits = (uint64_t)in_bytes * 8u;
    for (uint32_t y = 0; y < rows; ++y) {
        uint32_t cur, ref;
        m.row_begin(y, rowbytes, &cur, &ref);
        uint32_t rc = 0;
        if (m.lane() == 0) rc = tf_g4_row(m, r, nbits, cur, ref, y > 0u, W);
        rc = m.uni(rc);
        if (rc) return rc;
        m.row_end(y, rowbytes, cur);
    }
    return 0u;
}

// One strip, whatever its compression.  T: Deflate's tables.
template <class M>
__host__ __device__ inline uint32_t tf_strip(M& m, PiTables& T, uint32_t compression, uint32_t in_bytes, int W, uint32_t rows,
                                             uint32_t rowbytes) {
    const uint32_t want = rows * rowbytes;
    if (compression == TF_NONE) return tf_none(m, in_bytes, want);
    if (compression == TF_PACKBITS) return tf_packbits(m, in_bytes, want);
    if (compression == TF_LZW) return tf_lzw(m, in_bytes, want);
    if (compression == TF_DEFLATE) return tf_deflate(m, T, in_bytes, want);
    for (uint32_t i = (uint32_t)m.lane(); i < 2u << TF_RUN_BITS; i += (uint32_t)m.lanes()) m.run_set((int)(i >> TF_RUN_BITS), i & ((1u << TF_RUN_BITS) - 1u), 0u);
    m.sync();
    tf_run_tables(m);
    m.sync();
    return tf_g4_strip(m, in_bytes, W, rows, rowbytes);
}

// ---- the pixel stage --------------------------------------------------------------------------------------------------------------------------
// Sample k (0 .. samples - 1) of pixel x of a packed row, before predictor and inversion: a bit (MSB first) or a byte.
__host__ __device__ inline uint32_t tf_raw(const uint8_t* row, uint32_t layout, int x, int k) {
    if (layout == TF_BILEVEL) return ((uint32_t)row[x >> 3] >> (7 - (x & 7))) & 1u;
    return layout == TF_RGB ? row[3ll * x + k] : row[x];
}
// B,G,R of a pixel from its samples (predictor undone): bilevel 0 / 255, inversion for PhotometricInterpretation 0, palette B,G,R bytes.
__host__ __device__ inline void tf_pixel(uint32_t layout, uint32_t invert, const uint8_t* pal, uint32_t v0, uint32_t v1, uint32_t v2, uint8_t* o) {
    if (layout == TF_RGB) { o[0] = (uint8_t)v2; o[1] = (uint8_t)v1; o[2] = (uint8_t)v0; return; }
    if (layout == TF_PALETTE) { o[0] = pal[3u * (v0 & 255u)]; o[1] = pal[3u * (v0 & 255u) + 1u]; o[2] = pal[3u * (v0 & 255u) + 2u]; return; }
    uint32_t v = layout == TF_BILEVEL ? (v0 ? 255u : 0u) : (v0 & 255u);
    if (invert) v = 255u - v;
    o[0] = o[1] = o[2] = (uint8_t)v;
}

// ---- the inspector (host) ---------------------------------------------------------------------------------------------------------------------
struct TFReader {
    const uint8_t* p;
    size_t n;
    bool be;
    bool ok(uint64_t off, uint64_t len) const { return off <= n && len <= n - off; }
    uint32_t u16(size_t off) const { return be ? (uint32_t)p[off] << 8 | p[off + 1] : (uint32_t)p[off + 1] << 8 | p[off]; }
    uint32_t u32(size_t off) const { return be ? u16(off) << 16 | u16(off + 2) : u16(off + 2) << 16 | u16(off); }
};

struct TFField {                               // one IFD entry: its values are read on demand, each position checked
    uint32_t tag = 0, type = 0, count = 0;
    size_t at = 0;                             // where the values start (inside the entry or at its offset)
    bool present = false;
};

inline uint8_t tf_bitrev(uint8_t b) {
    b = (uint8_t)((b >> 4) | (b << 4));
    b = (uint8_t)(((b & 0xcc) >> 2) | ((b & 0x33) << 2));
    return (uint8_t)(((b & 0xaa) >> 1) | ((b & 0x55) << 1));
}

#define TF_REFUSE(...) do { snprintf(why, why_bytes, __VA_ARGS__); return RTN_EINVAL; } while (0)

// RTN_OK and *info (and the blob, if blob_out is not NULL) for a file the device decodes; RTN_EINVAL and a reason in `why` otherwise.
// g4_one_strip: take Group 4 pages of a single strip as well (one serial decoder per page).
inline int tf_inspect(const uint8_t* file, size_t n, bool g4_one_strip, rtn_tiff_info_t* info, void* blob_out, size_t capacity, char* why, size_t why_bytes) {
    memset(info, 0, sizeof(*info));
    if (n < 8) TF_REFUSE("not a TIFF: %zu bytes", n);
    TFReader r{file, n, false};
    if (file[0] == 'I' && file[1] == 'I') r.be = false;
    else if (file[0] == 'M' && file[1] == 'M') r.be = true;
    else TF_REFUSE("not a TIFF: no II or MM byte-order mark");
    const uint32_t version = r.u16(2);
    if (version == 43u) TF_REFUSE("BigTIFF");
    if (version != 42u) TF_REFUSE("not a TIFF: version %u", version);
    const uint64_t ifd = r.u32(4);
    if (!r.ok(ifd, 2)) TF_REFUSE("the IFD lies outside the file");
    const uint32_t nent = r.u16((size_t)ifd);
    if (!r.ok(ifd + 2, (uint64_t)nent * 12u + 4u)) TF_REFUSE("the IFD lies outside the file");
    enum { F_W, F_H, F_BITS, F_COMP, F_PHOTO, F_FILL, F_OFFS, F_ORIENT, F_SPP, F_RPS, F_COUNTS, F_PLANAR, F_T6, F_PRED, F_CMAP, F_EXTRA, F_TILEW,
           F_TILEO, F_SUBFMT, F_N };
    static const uint32_t tags[F_N] = {256, 257, 258, 259, 262, 266, 273, 274, 277, 278, 279, 284, 293, 317, 320, 338, 322, 324, 339};
    static const uint32_t type_bytes[14] = {0, 1, 1, 2, 4, 8, 1, 1, 2, 4, 8, 4, 8, 4};
    TFField f[F_N];
    for (uint32_t e = 0; e < nent; ++e) {
        const size_t at = (size_t)ifd + 2 + 12 * (size_t)e;
        const uint32_t tag = r.u16(at), type = r.u16(at + 2), count = r.u32(at + 4);
        for (int k = 0; k < F_N; ++k) {
            if (tags[k] != tag) continue;
            if (f[k].present) TF_REFUSE("tag %u twice", tag);
            if (type != 1u && type != 3u && type != 4u) TF_REFUSE("tag %u: type %u is not BYTE, SHORT or LONG", tag, type);
            const uint64_t bytes = (uint64_t)count * type_bytes[type];
            size_t where = at + 8;
            if (bytes > 4u) {
                const uint64_t off = r.u32(at + 8);
                if (!r.ok(off, bytes)) TF_REFUSE("tag %u: its %u values lie outside the file", tag, count);
                where = (size_t)off;
            }
            f[k].tag = tag; f[k].type = type; f[k].count = count; f[k].at = where; f[k].present = true;
        }
    }
    auto value = [&](const TFField& fd, uint32_t i) -> uint32_t {
        return fd.type == 1u ? file[fd.at + i] : fd.type == 3u ? r.u16(fd.at + 2 * (size_t)i) : r.u32(fd.at + 4 * (size_t)i);
    };
    auto one = [&](int k, uint32_t absent) -> uint32_t { return f[k].present && f[k].count >= 1u ? value(f[k], 0) : absent; };
    if (f[F_TILEW].present || f[F_TILEO].present) TF_REFUSE("tiles");
    if (!f[F_W].present || !f[F_H].present || f[F_W].count != 1u || f[F_H].count != 1u) TF_REFUSE("no ImageWidth or ImageLength");
    const uint32_t W = one(F_W, 0), H = one(F_H, 0);
    if (W < 1u || H < 1u || W > 65535u || H > 65535u) TF_REFUSE("%u x %u: sides must be 1 .. 65535", W, H);
    const uint32_t spp = one(F_SPP, 1), comp = one(F_COMP, 1), fill = one(F_FILL, 1), planar = one(F_PLANAR, 1), pred = one(F_PRED, 1);
    if (!f[F_PHOTO].present) TF_REFUSE("no PhotometricInterpretation");
    const uint32_t photo = one(F_PHOTO, 0);
    if (photo > 3u) TF_REFUSE("PhotometricInterpretation %u (CMYK, YCbCr, Lab, ...)", photo);
    if (one(F_ORIENT, 1) != 1u) TF_REFUSE("Orientation %u", one(F_ORIENT, 1));
    if (f[F_EXTRA].present && f[F_EXTRA].count) TF_REFUSE("ExtraSamples (alpha)");
    if (spp != 1u && spp != 3u) TF_REFUSE("%u samples per pixel", spp);
    if (planar != 1u && spp > 1u) TF_REFUSE("PlanarConfiguration %u", planar);
    uint32_t bits = 1;
    if (f[F_BITS].present) {
        if (f[F_BITS].count != spp) TF_REFUSE("BitsPerSample has %u values for %u samples", f[F_BITS].count, spp);
        bits = value(f[F_BITS], 0);
        for (uint32_t i = 1; i < spp; ++i)
            if (value(f[F_BITS], i) != bits) TF_REFUSE("samples of different depths");
    }
    if (f[F_SUBFMT].present)
        for (uint32_t i = 0; i < f[F_SUBFMT].count; ++i)
            if (value(f[F_SUBFMT], i) != 1u) TF_REFUSE("SampleFormat %u", value(f[F_SUBFMT], i));
    if (bits != 1u && bits != 8u) TF_REFUSE("%u-bit samples", bits);
    uint32_t layout;
    if (bits == 1u) {
        if (spp != 1u || photo > 1u) TF_REFUSE("1-bit samples that are not bilevel");
        layout = TF_BILEVEL;
    } else if (photo <= 1u) {
        if (spp != 1u) TF_REFUSE("gray with %u samples", spp);
        layout = TF_GRAY;
    } else if (photo == 2u) {
        if (spp != 3u) TF_REFUSE("R,G,B with %u samples", spp);
        layout = TF_RGB;
    } else {
        if (spp != 1u) TF_REFUSE("palette with %u samples", spp);
        if (!f[F_CMAP].present || f[F_CMAP].type != 3u || f[F_CMAP].count != 768u) TF_REFUSE("palette without a ColorMap of 768 SHORTs");
        layout = TF_PALETTE;
    }
    if (fill != 1u && !(fill == 2u && layout == TF_BILEVEL)) TF_REFUSE("FillOrder %u on %u-bit samples", fill, bits);
    uint32_t compression = comp == 32946u ? (uint32_t)TF_DEFLATE : comp;
    if (comp == 2u || comp == 3u) TF_REFUSE("Compression %u (Group 3)", comp);
    if (comp == 6u || comp == 7u) TF_REFUSE("Compression %u (JPEG)", comp);
    if (compression != TF_NONE && compression != TF_G4 && compression != TF_LZW && compression != TF_DEFLATE && compression != TF_PACKBITS)
        TF_REFUSE("Compression %u", comp);
    if (compression == TF_G4) {
        if (layout != TF_BILEVEL) TF_REFUSE("Group 4 on %u-bit samples", bits);
        if (one(F_T6, 0) != 0u) TF_REFUSE("T6Options %u (uncompressed mode)", one(F_T6, 0));
    }
    if (pred != 1u) {
        if (pred != 2u) TF_REFUSE("Predictor %u", pred);
        if (compression == TF_LZW || compression == TF_DEFLATE) {
            if (layout == TF_BILEVEL) TF_REFUSE("Predictor 2 on 1-bit samples");
        } else TF_REFUSE("Predictor 2 without LZW or Deflate");
    }
    const uint64_t rowbytes = layout == TF_BILEVEL ? ((uint64_t)W + 7u) >> 3 : (uint64_t)W * spp;
    if (rowbytes * H >= (1ull << 31)) TF_REFUSE("%u x %u: the page's rows take 2^31 bytes or more", W, H);
    uint32_t rps = one(F_RPS, 0xffffffffu);
    if (rps < 1u) TF_REFUSE("RowsPerStrip 0");
    if (rps > H) rps = H;
    const uint32_t nstrips = (H + rps - 1u) / rps;
    if (!f[F_OFFS].present || !f[F_COUNTS].present) TF_REFUSE("no StripOffsets or StripByteCounts");
    if (f[F_OFFS].type == 1u || f[F_COUNTS].type == 1u) TF_REFUSE("StripOffsets or StripByteCounts of type BYTE");
    if (f[F_OFFS].count != nstrips || f[F_COUNTS].count != nstrips)
        TF_REFUSE("%u strip offsets and %u byte counts for %u strips", f[F_OFFS].count, f[F_COUNTS].count, nstrips);
    if (compression == TF_G4 && nstrips == 1u && H > 64u && !g4_one_strip)
        TF_REFUSE("Group 4 in a single strip of %u rows: one serial decoder per page (RTN_TIFF_G4_ONE_STRIP=1 takes it)", H);
    uint64_t total = 0;
    for (uint32_t s = 0; s < nstrips; ++s) {
        const uint64_t off = value(f[F_OFFS], s), cnt = value(f[F_COUNTS], s);
        if (!r.ok(off, cnt)) TF_REFUSE("strip %u lies outside the file", s);
        const uint32_t rows = s + 1u < nstrips ? rps : H - s * rps;
        if (compression == TF_NONE && cnt < rows * rowbytes) TF_REFUSE("strip %u: %llu bytes for %u rows", s, (unsigned long long)cnt, rows);
        if (compression == TF_LZW && cnt >= 2u && file[off] == 0 && (file[off + 1] & 1)) TF_REFUSE("old-style LZW");
        total += cnt;
        if (total > n) TF_REFUSE("the strips overlap: more strip bytes than the file has");
    }
    // the blob
    uint64_t at = sizeof(TFHdr) + (uint64_t)nstrips * sizeof(TFStrip);
    const uint64_t off_pal = layout == TF_PALETTE ? at : 0;
    if (layout == TF_PALETTE) at += 768;
    const uint64_t off_data = (at + 15u) & ~15ull;
    const uint32_t lead = compression == TF_DEFLATE ? 2u : 0u;
    uint64_t data = 0;
    for (uint32_t s = 0; s < nstrips; ++s) data = ((data + 3u) & ~3ull) + lead + value(f[F_COUNTS], s);
    const uint64_t blob_bytes = (off_data + data + 8u + 15u) & ~15ull;
    info->width = (int32_t)W; info->height = (int32_t)H; info->components = (int32_t)spp; info->strips = (int32_t)nstrips;
    info->compression = (int32_t)compression; info->bits = (int32_t)bits; info->photometric = (int32_t)photo; info->predictor = (int32_t)pred;
    info->blob_bytes = (int64_t)blob_bytes;
    info->workspace_bytes = tf_ws_bytes(H, (long long)rowbytes, nstrips);
    info->payload_bytes = (int64_t)total;
    if (!blob_out) return RTN_OK;
    if (capacity < blob_bytes) {
        memset(info, 0, sizeof(*info));
        TF_REFUSE("blob_capacity %zu < %llu bytes", capacity, (unsigned long long)blob_bytes);
    }
    uint8_t* b = static_cast<uint8_t*>(blob_out);
    memset(b, 0, (size_t)blob_bytes);
    TFHdr hd;
    memset(&hd, 0, sizeof(hd));
    hd.magic = TF_MAGIC; hd.W = (int32_t)W; hd.H = (int32_t)H; hd.compression = compression; hd.layout = layout;
    hd.invert = (layout == TF_BILEVEL || layout == TF_GRAY) && photo == 0u ? 1u : 0u;
    hd.predictor = pred; hd.nstrips = nstrips; hd.rowbytes = (uint32_t)rowbytes;
    hd.off_table = (uint32_t)sizeof(TFHdr); hd.off_pal = (uint32_t)off_pal; hd.off_data = (uint32_t)off_data;
    hd.blob_bytes = (int64_t)blob_bytes; hd.ws_bytes = info->workspace_bytes;
    memcpy(b, &hd, sizeof(hd));
    if (layout == TF_PALETTE)
        for (uint32_t i = 0; i < 256u; ++i)                            // Pillow takes the high byte of every 16-bit entry
            for (uint32_t c = 0; c < 3u; ++c) b[off_pal + 3u * i + (2u - c)] = (uint8_t)(value(f[F_CMAP], c * 256u + i) >> 8);
    data = 0;
    for (uint32_t s = 0; s < nstrips; ++s) {
        const uint64_t off = value(f[F_OFFS], s), cnt = value(f[F_COUNTS], s);
        data = ((data + 3u) & ~3ull) + lead;
        TFStrip st;
        st.off = (uint32_t)data; st.bytes = (uint32_t)cnt; st.row0 = s * rps; st.rows = s + 1u < nstrips ? rps : H - s * rps;
        memcpy(b + hd.off_table + (size_t)s * sizeof(TFStrip), &st, sizeof(st));
        uint8_t* dst = b + off_data + data;
        if (fill == 2u) for (uint64_t i = 0; i < cnt; ++i) dst[i] = tf_bitrev(file[off + i]);   // FillOrder 2: the strip's bytes, bit-reversed
        else if (cnt) memcpy(dst, file + off, (size_t)cnt);
        data += cnt;
    }
    return RTN_OK;
}
#undef TF_REFUSE

// ---- the CPU twin -----------------------------------------------------------------------------------------------------------------------------
struct TFHostMem {                             // every position is checked against the sizes given; one outside them aborts
    const uint8_t* src; uint32_t in_bytes, lead;   // lead: 2 for Deflate (word and stored count behind the zlib header)
    uint8_t* out; uint32_t out_bytes;
    uint32_t* lzw;                             // 2 * 4096
    uint16_t* runs;                            // 2 * 8192
    [[noreturn]] static void out_of_range(const char* what, long long pos, long long n) {
        fprintf(stderr, "TFHostMem: %s %lld outside %lld\n", what, pos, n);
        abort();
    }
    inline void chk(const char* what, uint64_t pos, uint64_t n, uint64_t size) const {
        if (pos > size || n > size - pos) out_of_range(what, (long long)pos, (long long)size);
    }
    inline uint32_t in(uint32_t i) const { return i < in_bytes ? src[i] : 0u; }
    inline uint32_t word(uint32_t i) const {
        uint32_t w = 0;
        for (uint32_t k = 0; k < 4u; ++k) w |= in(lead + 4u * i + k) << (8u * k);
        if ((uint64_t)lead + 4ull * i >= in_bytes) out_of_range("word", i, in_bytes / 4);
        return w;
    }
    inline uint32_t get(uint32_t pos) const { chk("get", pos, 1, out_bytes); return out[pos]; }
    inline void put(uint32_t pos, uint32_t b) { chk("put", pos, 1, out_bytes); out[pos] = (uint8_t)b; }
    inline uint32_t in32(uint32_t i) const { return in(i) << 24 | in(i + 1u) << 16 | in(i + 2u) << 8 | in(i + 3u); }
    inline void row_begin(uint32_t y, uint32_t rowbytes, uint32_t* cur, uint32_t* ref) {   // the rows decode in place
        chk("row", (uint64_t)y * rowbytes, rowbytes, out_bytes);
        memset(out + (size_t)y * rowbytes, 0, rowbytes);
        *cur = y * rowbytes; *ref = y ? (y - 1u) * rowbytes : 0u;
    }
    inline void row_end(uint32_t, uint32_t, uint32_t) {}
    inline uint32_t rget(uint32_t pos) const { return get(pos); }
    inline void ror(uint32_t pos, uint32_t mask) { chk("ror", pos, 1, out_bytes); out[pos] |= (uint8_t)mask; }
    inline void fill(uint32_t pos, uint32_t n, uint32_t b) { chk("fill", pos, n, out_bytes); memset(out + pos, (int)b, n); }
    inline void stored(uint32_t pos, uint32_t at, uint32_t n) {
        chk("stored", pos, n, out_bytes); chk("stored from", (uint64_t)lead + at, n, in_bytes);
        memcpy(out + pos, src + lead + at, n);
    }
    inline void match(uint32_t pos, uint32_t d, uint32_t n) {
        chk("match", pos, n, out_bytes);
        if (d < 1u || d > pos) out_of_range("match distance", d, pos);
        for (uint32_t i = 0; i < n; ++i) out[pos + i] = out[pos + i - d];
    }
    inline void copy(uint32_t pos, uint32_t from, uint32_t n, bool kwk) {
        chk("copy", pos, n, out_bytes);
        if (n < 1u || (uint64_t)from + n - (kwk ? 1u : 0u) > pos) out_of_range("copy source", from, pos);
        for (uint32_t i = 0; i < n; ++i) out[pos + i] = out[kwk && i == n - 1u ? from : from + i];
    }
    inline void tab(uint32_t code, uint32_t off, uint32_t len) { chk("tab", code, 1, 4096); lzw[2 * code] = off; lzw[2 * code + 1] = len; }
    inline uint32_t tab_off(uint32_t code) const { chk("tab_off", code, 1, 4096); return lzw[2 * code]; }
    inline uint32_t tab_len(uint32_t code) const { chk("tab_len", code, 1, 4096); return lzw[2 * code + 1]; }
    inline void run_set(int colour, uint32_t i, uint32_t v) { chk("run_set", (uint64_t)colour * 8192u + i, 1, 16384); runs[colour * 8192 + i] = (uint16_t)v; }
    inline uint32_t run(int colour, uint32_t i) const { chk("run", (uint64_t)colour * 8192u + i, 1, 16384); return runs[colour * 8192 + i]; }
    inline int lane() const { return 0; }
    inline int lanes() const { return 1; }
    inline void sync() {}
    inline uint32_t uni(uint32_t v) const { return v; }
    inline bool boundary(uint64_t) const { return false; }
    inline uint32_t adler_join(uint32_t a, uint32_t b, uint32_t n) const { return ((b + n) % 65521u) << 16 | (a + 1u) % 65521u; }
};

// rtn_tiff_decode_host without the error text: every strip through tf_strip, then the pixel stage.  RTN_OK with *status = 0 and the
// page in out, or *status != 0 (the OR of the strips' words) and out not written; RTN_EINVAL (*why: the reason) otherwise.
inline int tf_decode_host(const void* blob, size_t blob_bytes, uint8_t* out, size_t out_bytes, int32_t* status, const char** why) {
    if (!tf_blob_ok(blob, blob_bytes)) { *why = "not an rtn_tiff_inspect blob"; return RTN_EINVAL; }
    const uint8_t* bl = static_cast<const uint8_t*>(blob);
    TFHdr hd;
    memcpy(&hd, bl, sizeof(hd));
    if (out_bytes != (size_t)hd.W * hd.H * 3) { *why = "out_bytes is not height * width * 3"; return RTN_EINVAL; }
    std::vector<uint8_t> rows((size_t)hd.H * hd.rowbytes, 0);
    std::vector<uint32_t> lzw(2 * 4096, 0);
    std::vector<uint16_t> runs(2 * 8192, 0);
    PiTables T;
    uint32_t st = 0;
    for (uint32_t s = 0; s < hd.nstrips; ++s) {
        TFStrip sp;
        memcpy(&sp, bl + hd.off_table + (size_t)s * sizeof(TFStrip), sizeof(sp));
        TFHostMem m;
        m.src = bl + hd.off_data + sp.off; m.in_bytes = sp.bytes; m.lead = hd.compression == TF_DEFLATE ? 2u : 0u;
        m.out = rows.data() + (size_t)sp.row0 * hd.rowbytes; m.out_bytes = sp.rows * hd.rowbytes;
        m.lzw = lzw.data(); m.runs = runs.data();
        st |= tf_strip(m, T, hd.compression, sp.bytes, hd.W, sp.rows, hd.rowbytes);
    }
    *status = (int32_t)st;
    if (st) return RTN_OK;
    const uint8_t* pal = hd.layout == TF_PALETTE ? bl + hd.off_pal : nullptr;
    const int ns = (int)tf_samples(hd.layout);
    for (int y = 0; y < hd.H; ++y) {
        const uint8_t* row = rows.data() + (size_t)y * hd.rowbytes;
        uint32_t acc[3] = {0u, 0u, 0u};
        for (int x = 0; x < hd.W; ++x) {
            uint32_t v[3] = {0u, 0u, 0u};
            for (int k = 0; k < ns; ++k) {
                v[k] = tf_raw(row, hd.layout, x, k);
                if (hd.predictor == 2u) { acc[k] = (acc[k] + v[k]) & 255u; v[k] = acc[k]; }
            }
            tf_pixel(hd.layout, hd.invert, pal, v[0], v[1], v[2], out + ((size_t)y * hd.W + x) * 3);
        }
    }
    return RTN_OK;
}
