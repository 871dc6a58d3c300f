// rtn_png_inflate.h — raw-deflate decode of ONE chunk of the DESIGN §3.4d PNG layout: the code that turns untrusted bytes into
// indices (bit reader, Huffman table builder, token decoder), as __host__ __device__ functions.  csrc/rtn_png_dec.hip calls them
// from its inflate kernel (one wave per chunk) and from rtn_png_inflate_chunk_host, which runs the same functions on a CPU so
// they can be fuzzed there.  Everything here is uniform across the lanes of a wave: every lane computes the same values and takes
// the same branches; only the memory operations behind the context `C` are split between lanes.
//
// The context supplies:
//   uint32_t word(uint32_t i)                        little-endian word i of the payload (i < ceil(in_bytes / 4), zero padded)
//   void put(uint32_t pos, uint32_t byte)            out[pos] = byte
//   void match(uint32_t pos, uint32_t d, uint32_t n) out[pos + i] = out[pos + i - d], i = 0 .. n-1 in order (d <= pos)
//   void stored(uint32_t pos, uint32_t at, uint32_t n)  out[pos + i] = payload byte at + i
//   int lane(), int lanes()                          this caller's share of a table fill
//   void sync()                                      makes table fills by other lanes visible
//   uint32_t uni(uint32_t v)                         v, which is the same in every lane (lets a wave keep it in a scalar register)
// pi_inflate checks every position before it hands it to the context: pos + n <= want, at + n <= in_bytes, d <= pos.
//
// A chunk is accepted (status 0) only if it is a sequence of non-final blocks that ends, exactly at the payload's last byte, with
// an empty stored block, and gives exactly `want` bytes without a match reaching before the chunk's first byte.  The code sets
// that zlib's inflate refuses are refused: over-subscribed, incomplete (but for a single code of one bit), no end-of-block code,
// more than 286 literal/length or 30 distance codes, a repeat with no previous length or past the end.
#pragma once
#include <stdint.h>
#if !defined(__HIPCC__) && !defined(__host__)      // a plain C++ compiler (host-only fuzzing builds)
#define __host__
#define __device__
#endif

enum {
    PI_TRUNC = 1,      // the blocks need more bits than the payload has
    PI_BLOCK = 2,      // block type 3, or a stored block whose length words disagree
    PI_CODE = 4,       // an invalid code set, or a code / symbol that no table holds
    PI_OVER = 8,       // more output than the chunk's slice
    PI_DIST = 16,      // a match starts before the chunk's first byte
    PI_FINAL = 32,     // a final block inside a chunk
    PI_SHORT = 64,     // the payload ended with fewer bytes than the slice
    PI_FILTER = 128,   // a row filter other than None, Sub, Up (set by the kernel)
    PI_ADLER = 256,    // the joined Adler-32 is not the stored one (set by the page kernel)
    PI_CRC = 512,      // a chunk's CRC-32 is not the stored one (set by the kernel)
    // stream PNG (csrc/rtn_png_stream.hip) only:
    PI_CHAIN = 1024,   // the chain of segments from the stream's first bit never decodes the final block
    PI_LEFT = 2048,    // bytes between the final block and the Adler-32
    PI_LENGTH = 4096,  // the stream holds fewer or more bytes than the page's filtered rows
};

constexpr int PI_LROOT = 10, PI_DROOT = 8;     // bits of the first-level lookup; longer codes are decoded canonically, bit by bit
constexpr int PI_NLL = 288, PI_ND = 32;

struct PiTables {
    uint16_t lfast[1 << PI_LROOT];             // symbol << 4 | code length; 0 = not in the table
    uint16_t dfast[1 << PI_DROOT];
    uint16_t lsym[PI_NLL], dsym[PI_ND];        // symbols in canonical order (by length, then value)
    uint16_t lcount[16], dcount[16];           // codes per length
    uint16_t first[16], start[16];             // builder scratch: first code and first canonical index of every length
    uint8_t lens[PI_NLL + PI_ND];              // code lengths of the block being set up
};

enum { PI_KIND_CODES = 0, PI_KIND_LENS = 1, PI_KIND_DISTS = 2 };

// LSB-first bit reader over the payload's words.  Past the end it reads zeros; consumed() tells the caller, who compares with the
// payload's length after every token.
template <class C>
struct PiReader {
    C& c;
    uint32_t nwords, next;
    uint64_t acc;
    int cnt;
    __host__ __device__ inline void refill() {
        if (cnt <= 32) {
            const uint32_t w = next < nwords ? c.word(next) : 0u;
            ++next;
            acc |= (uint64_t)w << cnt;
            cnt += 32;
        }
    }
    __host__ __device__ inline uint32_t peek(int k) {                  // k <= 16
        refill();
        return (uint32_t)acc & ((1u << k) - 1u);
    }
    __host__ __device__ inline void drop(int k) { acc >>= k; cnt -= k; }
    __host__ __device__ inline uint32_t bits(int k) {
        const uint32_t v = peek(k);
        drop(k);
        return v;
    }
    __host__ __device__ inline uint64_t consumed() const { return (uint64_t)next * 32u - (uint64_t)cnt; }
    __host__ __device__ inline void seek(uint32_t byte) {              // continue at a byte position
        next = byte >> 2;
        acc = 0;
        cnt = 0;
        refill();
        drop(8 * (int)(byte & 3u));
    }
    __host__ __device__ inline void seekbit(uint64_t bit) {            // continue at a bit position
        next = (uint32_t)(bit >> 5);
        acc = 0;
        cnt = 0;
        refill();
        drop((int)(bit & 31u));
    }
};

__host__ __device__ inline uint32_t pi_bitrev(uint32_t v, int n) {
    uint32_t r = 0;
    for (int i = 0; i < n; ++i) r |= ((v >> i) & 1u) << (n - 1 - i);
    return r;
}

// Decode tables of the n code lengths T.lens[at .. at + n): counts, canonical symbol order, first-level lookup.  false = a set
// inflate refuses.  An empty distance set is allowed (a block of literals only); using it is an invalid code.
template <class C>
__host__ __device__ inline bool pi_build(C& c, PiTables& T, int at, int n, int kind, int root, uint16_t* fast, uint16_t* count,
                                         uint16_t* sym) {
    const uint8_t* lens = T.lens + at;
    c.sync();                                                          // readers of the previous block's tables are done
    for (int l = 0; l < 16; ++l) count[l] = 0;
    for (int s = 0; s < n; ++s) count[lens[s]]++;
    for (int i = c.lane(); i < (1 << root); i += c.lanes()) fast[i] = 0;
    const int used = n - count[0];
    if (used == 0) {
        c.sync();
        return kind == PI_KIND_DISTS;
    }
    int left = 1;
    for (int l = 1; l < 16; ++l) {
        left = (left << 1) - count[l];
        if (left < 0) return false;                                    // over-subscribed
    }
    if (left > 0 && (kind == PI_KIND_CODES || !(used == 1 && count[1] == 1))) return false;       // incomplete
    uint32_t code = 0, idx = 0;
    for (int l = 1; l < 16; ++l) {
        T.first[l] = (uint16_t)code;
        T.start[l] = (uint16_t)idx;
        code = (code + count[l]) << 1;
        idx += count[l];
    }
    uint32_t off[16];
    for (int l = 1; l < 16; ++l) off[l] = T.start[l];
    for (int s = 0; s < n; ++s) {
        const int l = lens[s];
        if (!l) continue;
        uint32_t o = 0;
        for (int k = 1; k < 16; ++k) {                                 // off[l]++ without indexing registers by a variable
            if (k == l) { o = off[k]; off[k] = o + 1; }
        }
        sym[o] = (uint16_t)s;
    }
    c.sync();
    for (int i = c.lane(); i < used; i += c.lanes()) {
        const int s = sym[i], l = lens[s];
        if (l > root) continue;
        const uint32_t r = pi_bitrev((uint32_t)T.first[l] + (uint32_t)(i - T.start[l]), l);
        for (uint32_t k = r; k < (1u << root); k += 1u << l) fast[k] = (uint16_t)((s << 4) | l);
    }
    c.sync();
    return true;
}

// one symbol; -1 = the bits are no code of the set.  Consumes at least one bit otherwise.
template <class C>
__host__ __device__ inline int pi_decode(PiReader<C>& r, const uint16_t* fast, int root, const uint16_t* count, const uint16_t* sym) {
    const uint32_t peek = r.peek(15);
    const uint32_t e = r.c.uni(fast[peek & ((1u << root) - 1u)]);
    if (e & 15u) {
        r.drop((int)(e & 15u));
        return (int)(e >> 4);
    }
    int code = 0, first = 0, index = 0;
    for (int l = 1; l < 16; ++l) {
        code |= (int)((peek >> (l - 1)) & 1u);
        const int n = count[l];
        if (code - n < first) {
            r.drop(l);
            return sym[index + (code - first)];
        }
        index += n;
        first = (first + n) << 1;
        code <<= 1;
    }
    return -1;
}

// the code lengths of a dynamic block's header into T.lens: literal/length codes at 0, distance codes at hlit
template <class C>
__host__ __device__ inline int pi_dynamic_header(C& c, PiTables& T, PiReader<C>& r, int* hlit_out, int* hdist_out) {
    const int hlit = (int)r.bits(5) + 257, hdist = (int)r.bits(5) + 1, hclen = (int)r.bits(4) + 4;
    if (hlit > 286 || hdist > 30) return PI_CODE;
    // the order of the code-length code's lengths: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, five bits each
    const uint64_t order_lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 |
                              10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
    const uint64_t order_hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    for (int i = 0; i < 19; ++i) T.lens[i] = 0;
    for (int i = 0; i < hclen; ++i) {
        const int o = (int)((i < 12 ? order_lo >> (5 * i) : order_hi >> (5 * (i - 12))) & 31u);
        T.lens[o] = (uint8_t)r.bits(3);
    }
    if (!pi_build(c, T, 0, 19, PI_KIND_CODES, 7, T.dfast, T.dcount, T.dsym)) return PI_CODE;
    // the code-length tables are complete now, so T.lens is overwritten from 0
    const int total = hlit + hdist;
    int have = 0, prev = 0;
    while (have < total) {
        const int s = pi_decode(r, T.dfast, 7, T.dcount, T.dsym);
        if (s < 0) return PI_CODE;
        if (s < 16) {
            T.lens[have++] = (uint8_t)s;
            prev = s;
            continue;
        }
        int rep, v = 0;
        if (s == 16) {
            if (have == 0) return PI_CODE;                             // nothing to repeat
            v = prev;
            rep = 3 + (int)r.bits(2);
        } else if (s == 17) {
            rep = 3 + (int)r.bits(3);
        } else {
            rep = 11 + (int)r.bits(7);
        }
        if (have + rep > total) return PI_CODE;
        for (int i = 0; i < rep; ++i) T.lens[have++] = (uint8_t)v;
        prev = v;
    }
    if (T.lens[256] == 0) return PI_CODE;                              // no end-of-block code
    *hlit_out = hlit;
    *hdist_out = hdist;
    return 0;
}

// The decode tables of a fixed (type 1) or dynamic (type 2) block whose 3 header bits have been read.  Returns 0 or PI_* bits.
template <class C>
__host__ __device__ inline int pi_block_tables(C& c, PiTables& T, PiReader<C>& r, uint32_t type, uint64_t nbits) {
    int hlit = 288, hdist = 32;
    if (type == 1) {
        for (int s = 0; s < 288; ++s) T.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
        for (int s = 0; s < 32; ++s) T.lens[288 + s] = 5;
    } else {
        const int rc = pi_dynamic_header(c, T, r, &hlit, &hdist);
        if (r.consumed() > nbits) return PI_TRUNC;
        if (rc) return rc;
    }
    // the distance lengths sit behind the literal/length ones; build the distance tables first: they do not read T.dfast's
    // former content (the code-length code), and the literal/length build leaves T.lens alone
    if (!pi_build(c, T, hlit, hdist, PI_KIND_DISTS, PI_DROOT, T.dfast, T.dcount, T.dsym)) return PI_CODE;
    if (!pi_build(c, T, 0, hlit, PI_KIND_LENS, PI_LROOT, T.lfast, T.lcount, T.lsym)) return PI_CODE;
    return 0;
}

// The tokens of one block up to its end-of-block code; `out` advances.  A match may start up to `back` bytes before position 0
// (the context sees d > pos then).  Returns 0 or PI_* bits.
template <class C>
__host__ __device__ inline int pi_block_tokens(C& c, PiTables& T, PiReader<C>& r, uint64_t nbits, uint32_t& out, uint32_t want,
                                               uint32_t back) {
    for (;;) {                                                         // every token consumes at least 1 bit
        const int s = pi_decode(r, T.lfast, PI_LROOT, T.lcount, T.lsym);
        if (r.consumed() > nbits) return PI_TRUNC;
        if (s < 0) return PI_CODE;
        if (s < 256) {
            if (out >= want) return PI_OVER;
            c.put(out++, (uint32_t)s);
            continue;
        }
        if (s == 256) return 0;
        if (s > 285) return PI_CODE;
        const int i = s - 257;
        uint32_t len;
        if (i < 8) len = 3u + (uint32_t)i;
        else if (i == 28) len = 258u;
        else {
            const int eb = (i >> 2) - 1;
            len = 3u + ((4u + (uint32_t)(i & 3)) << eb) + r.bits(eb);
        }
        const int j = pi_decode(r, T.dfast, PI_DROOT, T.dcount, T.dsym);
        if (r.consumed() > nbits) return PI_TRUNC;
        if (j < 0 || j > 29) return PI_CODE;
        uint32_t dist;
        if (j < 4) dist = 1u + (uint32_t)j;
        else {
            const int eb = (j >> 1) - 1;
            dist = 1u + ((2u + (uint32_t)(j & 1)) << eb) + r.bits(eb);
        }
        if (r.consumed() > nbits) return PI_TRUNC;
        if ((uint64_t)dist > (uint64_t)out + back) return PI_DIST;
        if (len > want - out) return PI_OVER;
        c.match(out, dist, len);
        out += len;
    }
}

// Inflate the payload (in_bytes bytes behind c.word) into exactly `want` bytes.  Returns 0 or PI_* bits.
template <class C>
__host__ __device__ inline int pi_inflate(C& c, PiTables& T, uint32_t in_bytes, uint32_t want) {
    PiReader<C> r{c, (in_bytes + 3u) >> 2, 0u, 0ull, 0};
    const uint64_t nbits = (uint64_t)in_bytes * 8u;
    uint32_t out = 0;
    for (;;) {                                                         // every block consumes at least 3 bits
        const uint32_t hdr = r.bits(3);
        if (r.consumed() > nbits) return PI_TRUNC;
        if (hdr & 1u) return PI_FINAL;
        const uint32_t type = hdr >> 1;
        if (type == 3) return PI_BLOCK;
        if (type == 0) {
            uint32_t at = (uint32_t)((r.consumed() + 7u) >> 3);
            if (at + 4u > in_bytes) return PI_TRUNC;
            r.seek(at);
            const uint32_t len = r.bits(16), nlen = r.bits(16);
            if ((len ^ 0xffffu) != nlen) return PI_BLOCK;
            at += 4u;
            if (len > in_bytes - at) return PI_TRUNC;
            if (len > want - out) return PI_OVER;
            if (len) c.stored(out, at, len);
            out += len;
            at += len;
            if (len == 0 && at == in_bytes) return out == want ? 0 : PI_SHORT;
            r.seek(at);
            continue;
        }
        if (const int rc = pi_block_tables(c, T, r, type, nbits)) return rc;
        if (const int rc = pi_block_tokens(c, T, r, nbits, out, want, 0u)) return rc;
    }
}

// ---- one zlib stream cut into segments ------------------------------------------------------------------------------------
// The functions below serve csrc/rtn_png_stream.hip (one wave per call) and its CPU twin.  Beyond the members above the context has
//   uint64_t quick(uint64_t bit, uint64_t end)   bit j set: pi_quick_dynamic holds at bit offset bit + j (< end), j = 0 .. 63
//   bool boundary(uint64_t bit)                  a later segment's candidate sits at this bit offset
constexpr uint64_t PI_NONE = ~0ull;
constexpr uint32_t PI_WINDOW = 32768u;         // deflate's largest distance
constexpr uint32_t PI_MARK = 0x8000u;          // symbol PI_MARK | i: byte i of the PI_WINDOW bytes before the segment's first byte

// `n` <= 32 bits at bit offset `bit` of the bytes p[0 .. nbytes), zeros past the end.  Not uniform: every lane reads its own offset.
__host__ __device__ inline uint32_t pi_bits_at(const uint8_t* p, uint64_t nbytes, uint64_t bit, int n) {
    uint64_t v = 0;
    const uint64_t b0 = bit >> 3;
    for (int k = 0; k < 5; ++k) v |= (uint64_t)(b0 + k < nbytes ? p[b0 + k] : 0u) << (8 * k);
    return (uint32_t)((v >> (bit & 7u)) & ((1ull << n) - 1ull));
}

// The cheap part of the candidate test, from 74 bits: block type 2, at most 286 literal/length and 30 distance codes, a complete
// code-length code (Kraft sum of its 4 .. 19 three-bit lengths exactly 1).
__host__ __device__ inline bool pi_quick_dynamic(const uint8_t* p, uint64_t nbytes, uint64_t bit) {
    const uint32_t h = pi_bits_at(p, nbytes, bit, 17);
    if (((h >> 1) & 3u) != 2u) return false;
    if (((h >> 3) & 31u) > 29u || ((h >> 8) & 31u) > 29u) return false;
    const int hclen = (int)((h >> 13) & 15u) + 4;
    uint32_t kraft = 0;                                                // in units of 2^-7
    for (int i = 0; i < 19; i += 10) {
        const uint32_t v = pi_bits_at(p, nbytes, bit + 17u + 3u * (uint32_t)i, 30);
        for (int k = 0; k < 10 && i + k < hclen; ++k) {
            const uint32_t l = (v >> (3 * k)) & 7u;
            if (l) kraft += 128u >> l;
        }
    }
    return kraft == 128u;
}

// The full candidate test at one bit offset: a dynamic block header whose three code sets inflate would accept (pi_build's rules).
template <class C>
__host__ __device__ inline bool pi_is_dynamic_header(C& c, PiTables& T, uint32_t in_bytes, uint64_t bit) {
    PiReader<C> r{c, (in_bytes + 3u) >> 2, 0u, 0ull, 0};
    r.seekbit(bit);
    const uint32_t hdr = r.bits(3);
    if ((hdr >> 1) != 2u) return false;
    return pi_block_tables(c, T, r, 2u, (uint64_t)in_bytes * 8u) == 0;
}

// The first candidate in bit offsets [lo, hi), or PI_NONE.  The loop runs over the offsets, whatever the bytes hold.
template <class C>
__host__ __device__ inline uint64_t pi_find(C& c, PiTables& T, uint32_t in_bytes, uint64_t lo, uint64_t hi) {
    for (uint64_t b = lo; b < hi; b += 64u) {
        uint64_t mask = c.quick(b, hi);
        while (mask) {
            int j = 0;
            while (!((mask >> j) & 1u)) ++j;
            mask &= mask - 1u;
            if (pi_is_dynamic_header(c, T, in_bytes, b + (uint64_t)j)) return b + (uint64_t)j;
        }
    }
    return PI_NONE;
}

struct PiRun {
    uint64_t end_bit;                          // the bit after the last block decoded
    uint32_t out;                              // bytes produced
    uint32_t final;                            // 1: the last block decoded was the stream's final block
};

// Decode blocks from bit offset `start` until a block boundary that c.boundary() accepts, or through the final block, giving at
// most `want` bytes through the context.  A match may reach `back` bytes before the run's first byte.  Returns 0 or PI_* bits.
template <class C>
__host__ __device__ inline int pi_run(C& c, PiTables& T, uint32_t in_bytes, uint64_t start, uint32_t back, uint32_t want, PiRun* run) {
    PiReader<C> r{c, (in_bytes + 3u) >> 2, 0u, 0ull, 0};
    const uint64_t nbits = (uint64_t)in_bytes * 8u;
    r.seekbit(start);
    uint32_t out = 0;
    for (bool first = true;; first = false) {                          // every block consumes at least 3 bits
        const uint64_t at_bit = r.consumed();
        if (!first && c.boundary(at_bit)) {
            run->end_bit = at_bit; run->out = out; run->final = 0u;
            return 0;
        }
        const uint32_t hdr = r.bits(3);
        if (r.consumed() > nbits) return PI_TRUNC;
        const uint32_t type = hdr >> 1;
        if (type == 3) return PI_BLOCK;
        if (type == 0) {
            uint32_t at = (uint32_t)((r.consumed() + 7u) >> 3);
            if ((uint64_t)at + 4u > in_bytes) return PI_TRUNC;
            r.seek(at);
            const uint32_t len = r.bits(16), nlen = r.bits(16);
            if ((len ^ 0xffffu) != nlen) return PI_BLOCK;
            at += 4u;
            if (len > in_bytes - at) return PI_TRUNC;
            if (len > want - out) return PI_OVER;
            if (len) c.stored(out, at, len);
            out += len;
            r.seek(at + len);
        } else {
            if (const int rc = pi_block_tables(c, T, r, type, nbits)) return rc;
            if (const int rc = pi_block_tokens(c, T, r, nbits, out, want, back)) return rc;
        }
        if (hdr & 1u) {
            run->end_bit = r.consumed(); run->out = out; run->final = 1u;
            return 0;
        }
    }
}

// One entry of the window walk: byte i of the PI_WINDOW bytes that end where a segment ends (its bytes are [off, off + n) of the
// stream, as symbols in sym[off ..)), from the window `prev` that ends where the segment starts.  Positions before the stream's
// first byte give 0.
__host__ __device__ inline uint8_t pi_window_entry(const uint16_t* sym, const uint8_t* prev, uint32_t off, uint32_t n, uint32_t i) {
    const long long p = (long long)off + n - PI_WINDOW + i;
    if (p < 0) return 0;
    if (p >= (long long)off) {
        const uint16_t s = sym[p];
        return (s & PI_MARK) ? prev[s & (PI_WINDOW - 1u)] : (uint8_t)s;
    }
    return prev[p - ((long long)off - PI_WINDOW)];
}

// Symbol -> byte for stream position off + i of a segment whose preceding window is `prev`; *bad is set where a marker points
// before the stream's first byte.
__host__ __device__ inline uint8_t pi_resolve(uint16_t s, const uint8_t* prev, uint32_t off, int* bad) {
    if (!(s & PI_MARK)) return (uint8_t)s;
    const uint32_t m = s & (PI_WINDOW - 1u);
    if ((long long)off - PI_WINDOW + m < 0) *bad = 1;
    return prev[m];
}
