// rtn_tiff_encode.h — the text that the device Group 4 TIFF encoder (csrc/rtn_tiff_enc.hip) and its CPU twin share: the
// bilevel bitmap, the T.6 row encoder as a __host__ __device__ function templated on a bit sink, the size rules, the container writer
// and the twin itself.  A plain C++17 compiler compiles this header (no HIP), so that csrc/rtn_tiff_enc.hip and a stand-alone
// sanitizer build (tools/tiff_encode_fuzz.cpp) compile the same text.  The run-length codes are those of rtn_tiff_decode.h
// (tf_white_code, tf_black_code, tf_long_code): there is one copy of the tables.
//
// The bitmap of a page is 64-bit words, bit i of word k of a row = pixel 64 k + i (what one ballot over 64 pixels gives), the bits
// past the row's end 0.  A set bit is the coder's "black".  A row is read through a view (TERow: first word, distance between the
// row's words) so that the kernels may keep the words of neighbouring rows next to each other and the twin keeps rows whole.
//
// The row rule is libtiff's (Fax3Encode2DRow with putspan), which is what the parity tests compare with, byte for byte:
//   pass when b2 < a1; vertical when |a1 - b1| <= 3; otherwise horizontal, white first exactly when a0 + a1 == 0 or pixel a0 is 0;
//   a run of 2624 or more emits the 2560 make-up code repeatedly; a strip ends with EOFB (000000000001 twice) and zero bits up to
//   the next byte.  Rows are not byte aligned, and the first row of a strip is coded against an all-white row.
// A sink offers put(code, length): TECount only adds the lengths, the writing sinks (TEByteSink here, the kernel's word sink) place
// the bits MSB first, so the length pass and the emit pass share te_row.
#pragma once
#include "rtn_tiff_decode.h"
#include "rtn_skew.h"

constexpr int TE_MAX_SIDE = 65500;             // the page writers' limit (JPEG's), as page_io._check_page
constexpr int TE_MAX_RPS = 65535;              // RowsPerStrip is written as a SHORT
constexpr uint32_t TE_IFD_BYTES = 2 + 9 * 12 + 4;

// ---- the size rules ---------------------------------------------------------------------------------------------------------------------------
__host__ __device__ inline bool te_valid(int W, int H, int nc, int rps) {
    return W >= 1 && H >= 1 && W <= TE_MAX_SIDE && H <= TE_MAX_SIDE && (nc == 1 || nc == 3) && rps >= 1 && rps <= TE_MAX_RPS;
}
__host__ __device__ inline int te_words(int W) { return (W + 63) >> 6; }
__host__ __device__ inline int te_strip_rows(int H, int rps) { return rps < H ? rps : H; }            // a value above H gives one strip
__host__ __device__ inline int te_strips(int H, int rps) { const int r = te_strip_rows(H, rps); return (H + r - 1) / r; }
__host__ __device__ inline uint64_t te_strip_bytes(uint64_t row_bits) { return (row_bits + 24u + 7u) >> 3; }   // the rows, EOFB, padding
__host__ __device__ inline uint64_t te_ifd_offset(uint64_t data_bytes) { return (8u + data_bytes + 1u) & ~1ull; }
__host__ __device__ inline uint64_t te_file_bytes(uint64_t data_bytes, int nstrips) {
    return te_ifd_offset(data_bytes) + TE_IFD_BYTES + (nstrips > 1 ? 8ull * (uint64_t)nstrips : 0ull);
}
// The most bits one row can take (see rtn_tiff_encode_bound in include/rtn.h for the derivation): 7 per pixel and 24 per row.
__host__ __device__ inline uint64_t te_row_bound_bits(int W) { return 7ull * (uint64_t)W + 24u; }
// The largest file of a valid page, a multiple of 4 (the kernels write whole 32-bit words); 0 for 4 GiB or more.
inline uint64_t te_bound(int W, int H, int rps) {
    const uint64_t r = (uint64_t)te_strip_rows(H, rps), ns = (uint64_t)te_strips(H, rps), last = (uint64_t)H - (ns - 1u) * r;
    const uint64_t data = (ns - 1u) * te_strip_bytes(r * te_row_bound_bits(W)) + te_strip_bytes(last * te_row_bound_bits(W));
    const uint64_t file = (te_file_bytes(data, (int)ns) + 3u) & ~3ull;
    return file >= (1ull << 32) ? 0ull : file;
}

// ---- the bitmap ---------------------------------------------------------------------------------------------------------------------------------
__host__ __device__ inline int te_gray(const uint8_t* px, int nc) { return nc == 3 ? skw_gray3(px[0], px[1], px[2]) : px[0]; }
// the coder's bit of a pixel: ink (gray < t) under photometric 0 (WhiteIsZero), non-ink under photometric 1
__host__ __device__ inline uint32_t te_bit(int gray, int t, int photometric) { return (uint32_t)((gray < t) != (photometric != 0)); }

struct TERow {                                 // one row of a bitmap; white: the all-white row above a strip's first row
    const uint64_t* p;
    long long stride;
    bool white;
    __host__ __device__ inline uint64_t word(int k) const { return white ? 0ull : p[(long long)k * stride]; }
};

__host__ __device__ inline int te_ctz(uint64_t w) {                    // w != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return __ffsll((unsigned long long)w) - 1;
#else
    return __builtin_ctzll(w);
#endif
}
__host__ __device__ inline uint32_t te_pixel(const TERow& r, int x) { return (uint32_t)(r.word(x >> 6) >> (x & 63)) & 1u; }   // x < W
// First x' >= x whose pixel is v, or W (0 <= x <= W).  The bits past W are 0 and the result is clamped.
__host__ __device__ inline int te_find(const TERow& r, int x, int W, uint32_t v) {
    if (x >= W) return W;
    const int nk = te_words(W);
    int k = x >> 6;
    uint64_t w = (v ? r.word(k) : ~r.word(k)) & (~0ull << (x & 63));
    while (!w) {
        if (++k >= nk) return W;
        w = v ? r.word(k) : ~r.word(k);
    }
    const int p = (k << 6) + te_ctz(w);
    return p < W ? p : W;
}

// ---- the row encoder ------------------------------------------------------------------------------------------------------------------------------
struct TECount {
    uint64_t bits;
    __host__ __device__ inline void put(uint32_t, int len) { bits += (uint64_t)len; }
};

template <class S>
__host__ __device__ inline void te_code(S& s, uint32_t e) { s.put(e >> 4, (int)(e & 15u)); }   // an entry of the run tables: code << 4 | length

template <class S>
__host__ __device__ inline void te_span(S& s, int span, uint32_t black) {
    while (span >= 2624) { te_code(s, tf_long_code(12)); span -= 2560; }
    if (span >= 64) {
        const int k = span >> 6;                                       // 1 .. 40
        te_code(s, k > 27 ? tf_long_code(k - 28) : black ? tf_black_code(63 + k) : tf_white_code(63 + k));
        span -= k << 6;
    }
    te_code(s, black ? tf_black_code(span) : tf_white_code(span));
}

template <class S>
__host__ __device__ inline void te_row(const TERow& cur, const TERow& ref, int W, S& s) {
    int a0 = 0;
    int a1 = te_find(cur, 0, W, 1u);                                   // the first black pixel of either row, or W
    int b1 = te_find(ref, 0, W, 1u);
    for (;;) {                                                         // every turn but the first moves a0 forward
        const int b2 = b1 < W ? te_find(ref, b1, W, te_pixel(ref, b1) ^ 1u) : W;
        if (b2 < a1) {                                                 // pass
            s.put(1u, 4);
            a0 = b2;
        } else {
            const int d = b1 - a1;
            if (d >= -3 && d <= 3) {                                   // vertical: V0 1, VR1 011, VL1 010, VR2 000011, VL2 000010, VR3 0000011, VL3 0000010
                if (d == 0) s.put(1u, 1);
                else s.put(d < 0 ? 3u : 2u, d == 1 || d == -1 ? 3 : d == 2 || d == -2 ? 6 : 7);
                a0 = a1;
            } else {                                                   // horizontal: 001 and the two runs a0 .. a1, a1 .. a2
                const int a2 = a1 < W ? te_find(cur, a1, W, te_pixel(cur, a1) ^ 1u) : W;
                s.put(1u, 3);
                const uint32_t black = (a0 + a1 == 0 || te_pixel(cur, a0) == 0u) ? 0u : 1u;
                te_span(s, a1 - a0, black);
                te_span(s, a2 - a1, black ^ 1u);
                a0 = a2;
            }
        }
        if (a0 >= W) break;
        const uint32_t c = te_pixel(cur, a0);
        a1 = te_find(cur, a0, W, c ^ 1u);
        b1 = te_find(ref, te_find(ref, a0, W, c), W, c ^ 1u);
    }
}

// ---- the container ----------------------------------------------------------------------------------------------------------------------------------
__host__ __device__ inline void te_put16(uint8_t* o, uint32_t v) { o[0] = (uint8_t)v; o[1] = (uint8_t)(v >> 8); }
__host__ __device__ inline void te_put32(uint8_t* o, uint32_t v) { te_put16(o, v); te_put16(o + 2, v >> 16); }
__host__ __device__ inline void te_field(uint8_t* e, uint32_t tag, uint32_t type, uint32_t count, uint32_t value) {
    te_put16(e, tag); te_put16(e + 2, type); te_put32(e + 4, count); te_put32(e + 8, value);           // a SHORT sits in the low half
}
// EOFB behind a strip's rows: bits [bit, bit + 24) of the zeroed file are 000000000001 000000000001
__host__ __device__ inline void te_eofb(uint8_t* out, uint64_t bit) {
    out[(bit + 11u) >> 3] |= (uint8_t)(0x80u >> ((bit + 11u) & 7u));
    out[(bit + 23u) >> 3] |= (uint8_t)(0x80u >> ((bit + 23u) & 7u));
}
// Strip s (at file offset `off`, `bytes` long) in the two arrays behind the IFD; a page of one strip holds both values inline.
__host__ __device__ inline void te_strip_entry(uint8_t* out, uint64_t ifd, int nstrips, int s, uint32_t off, uint32_t bytes) {
    if (nstrips == 1) { te_put32(out + ifd + 2 + 5 * 12 + 8, off); te_put32(out + ifd + 2 + 7 * 12 + 8, bytes); return; }
    te_put32(out + ifd + TE_IFD_BYTES + 4ull * (uint64_t)s, off);
    te_put32(out + ifd + TE_IFD_BYTES + 4ull * (uint64_t)(nstrips + s), bytes);
}
// The 8-byte header and the IFD at `ifd` (te_ifd_offset of the strips' bytes): the nine fields Pillow writes for such a page.
__host__ __device__ inline void te_header_ifd(uint8_t* out, uint64_t ifd, int W, int H, int rps, int photometric, int nstrips) {
    out[0] = 'I'; out[1] = 'I';
    te_put16(out + 2, 42u);
    te_put32(out + 4, (uint32_t)ifd);
    uint8_t* e = out + ifd;
    const uint32_t n = (uint32_t)nstrips, arrays = (uint32_t)ifd + TE_IFD_BYTES;
    te_put16(e, 9u);
    te_field(e + 2 + 0 * 12, 256u, 3u, 1u, (uint32_t)W);
    te_field(e + 2 + 1 * 12, 257u, 3u, 1u, (uint32_t)H);
    te_field(e + 2 + 2 * 12, 258u, 3u, 1u, 1u);
    te_field(e + 2 + 3 * 12, 259u, 3u, 1u, 4u);
    te_field(e + 2 + 4 * 12, 262u, 3u, 1u, (uint32_t)photometric);
    te_field(e + 2 + 5 * 12, 273u, 4u, n, n > 1u ? arrays : 0u);      // one strip: te_strip_entry writes the values
    te_field(e + 2 + 6 * 12, 278u, 3u, 1u, (uint32_t)rps);
    te_field(e + 2 + 7 * 12, 279u, 4u, n, n > 1u ? arrays + 4u * n : 0u);
    te_field(e + 2 + 8 * 12, 284u, 3u, 1u, 1u);
    te_put32(e + 2 + 9 * 12, 0u);
}

// ---- the CPU twin ---------------------------------------------------------------------------------------------------------------------------------
struct TEByteSink {                            // bit `bit` of the zeroed file, MSB first; every position checked (one outside aborts)
    uint8_t* out;
    uint64_t bit, capacity_bits;
    inline void put(uint32_t code, int len) {
        if (bit + (uint64_t)len > capacity_bits) { fprintf(stderr, "TEByteSink: bit %llu outside %llu\n", (unsigned long long)bit, (unsigned long long)capacity_bits); abort(); }
        for (int i = len - 1; i >= 0; --i, ++bit)
            if ((code >> i) & 1u) out[bit >> 3] |= (uint8_t)(0x80u >> (bit & 7u));
    }
};

// rtn_tiff_encode_host without the error text: RTN_OK and the file in out[0 .. *out_bytes), or RTN_EINVAL / RTN_ENOMEM and *why.
inline int te_encode_host(int W, int H, int nc, const uint8_t* page, int t, int rps, int photometric, uint8_t* out, size_t capacity,
                          size_t* out_bytes, const char** why) {
    if (!te_valid(W, H, nc, rps)) { *why = "invalid page: sides 1 .. 65500, 1 or 3 components, rows per strip 1 .. 65535"; return RTN_EINVAL; }
    if (t < 1 || t > 255 || (photometric != 0 && photometric != 1)) { *why = "threshold must be 1 .. 255 and photometric 0 or 1"; return RTN_EINVAL; }
    if (te_bound(W, H, rps) == 0) { *why = "the page can give a file of 4 GiB or more"; return RTN_EINVAL; }
    const int wpr = te_words(W), sr = te_strip_rows(H, rps), ns = te_strips(H, rps);
    std::vector<uint64_t> bm((size_t)wpr * H, 0ull);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
            bm[(size_t)y * wpr + (x >> 6)] |= (uint64_t)te_bit(te_gray(page + ((size_t)y * W + x) * nc, nc), t, photometric) << (x & 63);
    auto row = [&](int y) { return TERow{bm.data() + (size_t)y * wpr, 1, false}; };
    auto above = [&](int y) { return y % sr ? row(y - 1) : TERow{nullptr, 0, true}; };
    std::vector<uint64_t> bits((size_t)H), strip_off((size_t)ns + 1, 0ull);
    for (int y = 0; y < H; ++y) {                                      // the length pass
        TECount c = {0ull};
        te_row(row(y), above(y), W, c);
        if (c.bits > te_row_bound_bits(W)) { fprintf(stderr, "te_encode_host: a row of %llu bits\n", (unsigned long long)c.bits); abort(); }
        bits[(size_t)y] = c.bits;
    }
    for (int s = 0; s < ns; ++s) {
        uint64_t b = 0;
        for (int y = s * sr; y < H && y < (s + 1) * sr; ++y) b += bits[(size_t)y];
        strip_off[(size_t)s + 1] = strip_off[(size_t)s] + te_strip_bytes(b);
    }
    const uint64_t data = strip_off[(size_t)ns], file = te_file_bytes(data, ns), ifd = te_ifd_offset(data);
    if (file > capacity) { *why = "capacity is below the file's length (rtn_tiff_encode_bound bytes always suffice)"; return RTN_ENOMEM; }
    memset(out, 0, (size_t)file);
    te_header_ifd(out, ifd, W, H, rps, photometric, ns);
    for (int s = 0; s < ns; ++s) {                                     // the emit pass
        TEByteSink k = {out, 8u * (8u + strip_off[(size_t)s]), 8u * (8u + strip_off[(size_t)s + 1])};
        for (int y = s * sr; y < H && y < (s + 1) * sr; ++y) te_row(row(y), above(y), W, k);
        te_eofb(out, k.bit);
        te_strip_entry(out, ifd, ns, s, (uint32_t)(8u + strip_off[(size_t)s]), (uint32_t)(strip_off[(size_t)s + 1] - strip_off[(size_t)s]));
    }
    *out_bytes = (size_t)file;
    return RTN_OK;
}
