// rtn_png_stream.h — the host side of the stream PNG decoder: the blob and workspace layouts, the file inspector and
// the CPU twin of the device's inflate, for both of its entry points (rtn_png_stream_* and rtn_png_layout_*).  Plain C++ (no HIP), so that csrc/rtn_png_stream.hip and a stand-alone sanitizer build
// (tools/png_stream_fuzz.cpp) compile the same text.  Everything that reads file bytes checks each position against the length
// it was given before it uses it.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "rtn.h"
#include "rtn_png_inflate.h"
#include "rtn_png_crc.h"
#include "rtn_png_layout.h"

constexpr uint32_t PS_MAGIC = 0x534e5052u;     // "RPNS"
constexpr int PS_CHUNK = 32768;                // bytes of the filtered stream per Adler pair (and per resolve workgroup)
constexpr uint32_t PS_SEGMENT_MIN = 256, PS_SEGMENT_MAX = 1u << 24, PS_SEGMENT_DEFAULT = 16384;

struct PSHdr {                                 // start of a blob; 64 bytes
    uint32_t magic;
    int32_t W, H, nc;
    uint32_t nsegs, nidat;
    uint32_t seg_bytes;                        // S: compressed bytes per segment
    uint32_t in_bytes;                         // deflate bytes: the zlib stream without its 2-byte header and its Adler-32
    uint32_t adler;                            // the stream's last four bytes
    uint32_t off_table;                        // PSIdat[nidat], from the blob's start
    uint32_t off_data;                         // the deflate bytes, from the blob's start (a multiple of 4; the zlib header sits 2 before)
    uint32_t fmt;                              // PS_MAGIC: 0; PL_MAGIC: the page's format word (pl_fmt), its palette behind the table
    int64_t blob_bytes, ws_bytes;
};
static_assert(sizeof(PSHdr) == 64, "blob header");
struct PSIdat { uint32_t off, len, crc; };     // [off, off + len) of the zlib stream (which starts at off_data - 2), the chunk's stored CRC

struct PSSeg {                                 // per segment, in the workspace
    uint64_t cand;                             // bit offset of its candidate block start in the deflate bytes, or PI_NONE
    uint64_t end_bit;                          // where the run from cand landed
    uint32_t out, final, status, pad_;         // bytes the run produced; 1 = it decoded the final block; PI_* bits
};
struct PSLink { uint32_t seg, off; };          // one link of the chain: segment, offset of its first byte in the filtered stream
struct PSHead { uint32_t nlinks, status, pad_[2]; };
struct PSMeta { uint32_t a, b, status, pad_; };     // per PS_CHUNK bytes of the filtered stream: Adler pair, PI_* bits

struct PSLayout { long long meta, sym, seg, chain, win, total, nchunks; };
__host__ __device__ inline long long ps_al(long long v) { return (v + 255) & ~255LL; }
// The workspace of one page from what the host knows: the filtered stream's length and the number of segments.  The chain can have
// a link in every segment, so every segment gets a window: 32 KiB per S compressed bytes.  At the default S = 16384 that is twice
// the file's size; at the smallest S = 256 (tests) it is 128 times the file's size, 128 MB for a 1 MB stream.
__host__ __device__ inline PSLayout ps_layout(long long stream, long long nsegs) {
    PSLayout l;
    l.nchunks = (stream + PS_CHUNK - 1) / PS_CHUNK;
    l.meta = l.nchunks * PS_CHUNK;                                     // the filtered stream comes first
    l.sym = l.meta + ps_al(l.nchunks * (long long)sizeof(PSMeta));
    l.seg = l.sym + ps_al(2 * stream);
    l.chain = l.seg + ps_al(nsegs * (long long)sizeof(PSSeg));
    l.win = l.chain + ps_al((long long)sizeof(PSHead) + nsegs * (long long)sizeof(PSLink));
    l.total = l.win + nsegs * (long long)PI_WINDOW;                    // one window per link
    return l;
}

// Follow the landings from segment 0.  Every link lies in a later segment than the one before, so the walk ends within nsegs
// steps.  Returns PI_* bits (0: the chain decoded the final block, which ended in the deflate data's last byte, after exactly
// `want` bytes) and the links walked before any fault.
__host__ __device__ inline uint32_t ps_chain(const PSSeg* segs, uint32_t nsegs, uint32_t S, uint32_t in_bytes, uint32_t want,
                                             PSLink* links, uint32_t* nlinks) {
    uint32_t st = 0, k = 0, off = 0, n = 0;
    for (uint32_t step = 0; step < nsegs; ++step) {
        const PSSeg s = segs[k];
        if (s.cand == PI_NONE || s.status) { st |= PI_CHAIN | s.status; break; }
        if (s.out > want - off) { st |= PI_LENGTH; break; }
        links[n].seg = k;
        links[n].off = off;
        ++n;
        off += s.out;
        if (s.final) {
            if (((s.end_bit + 7u) >> 3) != in_bytes) st |= PI_LEFT;
            if (off != want) st |= PI_LENGTH;
            *nlinks = n;
            return st;
        }
        const uint64_t nk = (s.end_bit >> 3) / S;
        if (nk <= k || nk >= nsegs) { st |= PI_CHAIN; break; }
        k = (uint32_t)nk;
    }
    *nlinks = n;
    return st ? st : (uint32_t)PI_CHAIN;
}

// The link that holds stream position p (the last one that starts at or before it), by bisection; nlinks >= 1, links[0].off == 0.
__host__ __device__ inline uint32_t ps_link_of(const PSLink* links, uint32_t nlinks, uint32_t p) {
    uint32_t lo = 0, hi = nlinks;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (links[mid].off <= p) lo = mid; else hi = mid;
    }
    return lo;
}

inline uint32_t ps_be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

inline uint32_t ps_crc(uint32_t c, const uint8_t* p, size_t n) {
    for (size_t i = 0; i < n; ++i) c = pe_crc_byte(c, p[i]);
    return c;
}

// rtn_png_stream_inspect (layout false) and rtn_png_layout_inspect (layout true: every pixel layout of pl_accepts, Adam7, PLTE and
// tRNS) without the handle: RTN_OK, or RTN_EINVAL and a reason in why[whylen].  S: the segment size.
inline int ps_inspect_any(const uint8_t* f, size_t n, uint32_t S, rtn_png_info_t* info, void* blob_out, size_t blob_capacity, char* why,
                          size_t whylen, bool layout) {
#define PS_FAIL(...) do { snprintf(why, whylen, __VA_ARGS__); return RTN_EINVAL; } while (0)
    memset(info, 0, sizeof(*info));
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    if (n < 8 || memcmp(f, sig, 8) != 0) PS_FAIL("not a PNG file (no signature)");
    if (n >= ((size_t)1 << 30)) PS_FAIL("file larger than 1 GiB");
    if (n < 8 + 25) PS_FAIL("truncated PNG (no IHDR)");
    if (ps_be32(f + 8) != 13 || memcmp(f + 12, "IHDR", 4) != 0) PS_FAIL("the first chunk is not a 13-byte IHDR");
    if (~ps_crc(0xffffffffu, f + 12, 17) != ps_be32(f + 29)) PS_FAIL("CRC of IHDR");
    const uint32_t W = ps_be32(f + 16), H = ps_be32(f + 20);
    const int depth = f[24], ctype = f[25];
    if (!layout) {
        if (depth != 8) PS_FAIL("bit depth %d (only 8-bit PNG is decoded on the device)", depth);
        if (ctype != 0 && ctype != 2) PS_FAIL("colour type %d (only gray and R,G,B are decoded on the device)", ctype);
    } else if (!pl_accepts(ctype, depth)) {
        if (ctype == 0 && depth == 16) PS_FAIL("16-bit gray PNG (left to the host decoder)");
        PS_FAIL("colour type %d at bit depth %d", ctype, depth);
    }
    if (f[26] != 0 || f[27] != 0) PS_FAIL("compression method %d, filter method %d", f[26], f[27]);
    if (f[28] != 0 && !layout) PS_FAIL("interlaced PNG");
    if (f[28] > 1) PS_FAIL("interlace method %d", f[28]);
    const int nc = pl_samples(ctype);
    if (W < 1 || H < 1 || W > 0x7fffffffu || H > 0x7fffffffu) PS_FAIL("PNG sides %u x %u", W, H);
    PLGeom geom;
    pl_geometry((int)W, (int)H, pl_fmt(depth, ctype, f[28], 0), &geom);
    if (geom.stream >= (1ll << 31)) {
        if (!layout) PS_FAIL("%u x %u page: height * (1 + width * components) must be < 2^31", W, H);
        PS_FAIL("%u x %u page: the filtered rows of all passes must take < 2^31 bytes", W, H);
    }
    const long long stream = geom.stream;

    // ancillary chunks that cannot change what Image.open(f).convert("RGB") returns
    static const char* const harmless[] = {"pHYs", "tEXt", "zTXt", "iTXt", "tIME", "gAMA", "cHRM", "sRGB", "iCCP", "eXIf"};
    struct Part { size_t at; uint32_t len, crc; };
    std::vector<Part> parts;
    size_t pos = 8 + 25, zbytes = 0, pal_at = 0;
    int npal = 0;
    int state = 0;                                                     // 0 before the IDATs, 1 among them, 2 behind them
    for (;;) {                                                         // every chunk takes at least 12 bytes
        if (n - pos < 12) PS_FAIL("truncated PNG (chunk header at byte %zu)", pos);
        const uint32_t len = ps_be32(f + pos);
        const uint8_t* type = f + pos + 4;
        if ((size_t)len > n - pos - 12) PS_FAIL("truncated PNG (the chunk at byte %zu runs past the file)", pos);
        if (memcmp(type, "IEND", 4) == 0) {
            if (state == 0) PS_FAIL("no IDAT");
            if (ctype == 3 && !npal) PS_FAIL("palette PNG without a PLTE chunk before the first IDAT");
            if (len != 0 || ps_be32(f + pos + 8) != 0xae426082u) PS_FAIL("IEND is not empty or its CRC is wrong");
            if (pos + 12 != n) PS_FAIL("%zu bytes after IEND", n - pos - 12);
            break;
        }
        if (memcmp(type, "IDAT", 4) == 0) {
            if (state == 2) PS_FAIL("an IDAT after another chunk");
            state = 1;
            parts.push_back({pos + 8, len, ps_be32(f + pos + 8 + len)});
            zbytes += len;
        } else {
            bool ok = false;
            for (const char* t : harmless) ok = ok || memcmp(type, t, 4) == 0;
            if (layout && memcmp(type, "tRNS", 4) == 0) ok = true;     // the conversion to R,G,B ignores it
            if (layout && memcmp(type, "PLTE", 4) == 0 && (ctype == 2 || ctype == 6)) ok = true;     // a suggested palette: unused
            if (layout && memcmp(type, "PLTE", 4) == 0 && ctype == 3) {
                if (state != 0) PS_FAIL("PLTE after the first IDAT");
                if (npal) PS_FAIL("a second PLTE chunk");
                if (len % 3u != 0 || len < 3u || len / 3u > (1u << depth)) PS_FAIL("PLTE of %u bytes at bit depth %d", len, depth);
                npal = (int)(len / 3u);
                pal_at = pos + 8;
                ok = true;
            }
            if (!ok) PS_FAIL("chunk %02x %02x %02x %02x (not one the device decoder passes over)", type[0], type[1], type[2], type[3]);
            if (~ps_crc(0xffffffffu, type, 4 + (size_t)len) != ps_be32(f + pos + 8 + len)) PS_FAIL("CRC of the chunk at byte %zu", pos);
            if (state == 1) state = 2;
        }
        pos += 12 + (size_t)len;
    }
    if (zbytes < 7) PS_FAIL("%zu bytes of IDAT data: no room for a zlib header, a block and the Adler-32", zbytes);
    if (parts.size() >= ((size_t)1 << 28)) PS_FAIL("too many IDAT chunks");
    std::vector<uint8_t> z(zbytes);
    {
        size_t at = 0;
        for (const Part& p : parts) {
            if (p.len) memcpy(z.data() + at, f + p.at, p.len);
            at += p.len;
        }
    }
    const int cmf = z[0], flg = z[1];
    if ((cmf & 15) != 8 || (cmf >> 4) > 7 || (flg & 0x20) || (cmf * 256 + flg) % 31 != 0) PS_FAIL("bad zlib header %02x %02x", cmf, flg);
    const size_t in_bytes = zbytes - 6;
    if (S < PS_SEGMENT_MIN) S = PS_SEGMENT_MIN;
    if (S > PS_SEGMENT_MAX) S = PS_SEGMENT_MAX;
    const size_t nsegs = (in_bytes + S - 1) / S;
    const size_t nidat = parts.size();
    const size_t off_table = sizeof(PSHdr);
    const size_t off_pal = off_table + nidat * sizeof(PSIdat);         // 3 npal bytes; none in a stream blob
    const size_t off_data = ((off_pal + 3 * (size_t)npal + 15) & ~(size_t)15) + 4;
    const size_t total = (off_data - 2 + zbytes + 4 + 15) & ~(size_t)15;      // at least one zero word behind the stream
    info->width = (int32_t)W; info->height = (int32_t)H; info->components = nc; info->chunks = (int32_t)nsegs;
    info->blob_bytes = (int64_t)total;
    info->workspace_bytes = ps_layout(stream, (long long)nsegs).total;
    info->payload_bytes = (int64_t)zbytes;
    if (!blob_out) return RTN_OK;
    if (total > 128 + 2 * n) PS_FAIL("internal: blob bound");
    if (blob_capacity < total) PS_FAIL("rtn_png_%s_inspect: blob capacity %zu < %zu bytes", layout ? "layout" : "stream", blob_capacity, total);
    uint8_t* bl = static_cast<uint8_t*>(blob_out);
    memset(bl, 0, total);
    PSHdr hd;
    memset(&hd, 0, sizeof(hd));
    hd.magic = layout ? PL_MAGIC : PS_MAGIC;
    hd.fmt = layout ? pl_fmt(depth, ctype, f[28], npal) : 0u;
    hd.W = (int32_t)W; hd.H = (int32_t)H; hd.nc = nc;
    hd.nsegs = (uint32_t)nsegs; hd.nidat = (uint32_t)nidat; hd.seg_bytes = S; hd.in_bytes = (uint32_t)in_bytes;
    hd.adler = ps_be32(z.data() + zbytes - 4);
    hd.off_table = (uint32_t)off_table; hd.off_data = (uint32_t)off_data;
    hd.blob_bytes = (int64_t)total; hd.ws_bytes = info->workspace_bytes;
    memcpy(bl, &hd, sizeof(hd));
    uint32_t at = 0;
    for (size_t k = 0; k < nidat; ++k) {
        const PSIdat e = {at, parts[k].len, parts[k].crc};
        memcpy(bl + off_table + k * sizeof(PSIdat), &e, sizeof(e));
        at += parts[k].len;
    }
    if (npal) memcpy(bl + off_pal, f + pal_at, 3 * (size_t)npal);
    memcpy(bl + off_data - 2, z.data(), zbytes);
    return RTN_OK;
#undef PS_FAIL
}

inline int ps_inspect(const uint8_t* f, size_t n, uint32_t S, rtn_png_info_t* info, void* blob_out, size_t blob_capacity, char* why,
                      size_t whylen) {
    return ps_inspect_any(f, n, S, info, blob_out, blob_capacity, why, whylen, false);
}
inline int pl_inspect(const uint8_t* f, size_t n, uint32_t S, rtn_png_info_t* info, void* blob_out, size_t blob_capacity, char* why,
                      size_t whylen) {
    return ps_inspect_any(f, n, S, info, blob_out, blob_capacity, why, whylen, true);
}

// The format word of a blob's page: a layout blob carries it, a stream blob is 8-bit gray or R,G,B without interlace.
inline uint32_t ps_fmt(const PSHdr* hd) { return hd->magic == PL_MAGIC ? hd->fmt : pl_fmt(8, hd->nc == 3 ? 2 : 0, 0, 0); }
// The length of a blob's filtered stream (< 2^31 for a blob ps_blob_any passed).
inline long long ps_want(const PSHdr* hd) {
    PLGeom g;
    pl_geometry(hd->W, hd->H, ps_fmt(hd), &g);
    return g.stream;
}

// A blob's header (of either inspector) if [blob, blob + avail) can hold what it describes, else null.
inline const PSHdr* ps_blob_any(const void* blob, size_t avail) {
    if (avail < sizeof(PSHdr)) return nullptr;
    const PSHdr* hd = static_cast<const PSHdr*>(blob);
    if ((hd->magic != PS_MAGIC && hd->magic != PL_MAGIC) || hd->W < 1 || hd->H < 1 || hd->nsegs < 1 || hd->nidat < 1) return nullptr;
    if (hd->magic == PS_MAGIC ? (hd->nc != 1 && hd->nc != 3) || hd->fmt != 0 : !pl_fmt_ok(hd->fmt) || hd->nc != pl_samples(pl_ctype(hd->fmt)))
        return nullptr;
    if (hd->seg_bytes < PS_SEGMENT_MIN || hd->seg_bytes > PS_SEGMENT_MAX || hd->in_bytes < 1 || hd->in_bytes >= (1u << 30)) return nullptr;
    if (ps_want(hd) >= (1ll << 31)) return nullptr;
    if (hd->nsegs != (hd->in_bytes + hd->seg_bytes - 1) / hd->seg_bytes) return nullptr;
    if (hd->blob_bytes < 0 || (size_t)hd->blob_bytes > avail || hd->off_table != sizeof(PSHdr) || (hd->off_data & 3)) return nullptr;
    if ((size_t)hd->off_data < hd->off_table + (size_t)hd->nidat * sizeof(PSIdat) + 3 * (size_t)pl_npal(ps_fmt(hd)) + 2) return nullptr;
    if ((size_t)hd->off_data + hd->in_bytes + 8 > (size_t)hd->blob_bytes) return nullptr;
    return hd;
}
// The same for one inspector's blobs alone.
inline const PSHdr* ps_blob(const void* blob, size_t avail, uint32_t magic = PS_MAGIC) {
    const PSHdr* hd = ps_blob_any(blob, avail);
    return hd && hd->magic == magic ? hd : nullptr;
}
// The palette of a layout blob: 3 pl_npal(fmt) bytes behind the IDAT table.
inline const uint8_t* pl_palette(const PSHdr* hd) {
    return reinterpret_cast<const uint8_t*>(hd) + hd->off_table + (size_t)hd->nidat * sizeof(PSIdat);
}

struct PSHostCtx {                             // the CPU twin: one caller does everything
    const uint8_t* in;                         // the deflate bytes, zero padded to a whole word and one more
    uint32_t in_bytes;
    const PSSeg* segs;
    uint32_t nsegs, S, self;
    uint16_t* sym;                             // null: count only
    uint32_t want;                             // symbols behind sym (every write is checked against it: the sanitizer build's context)
    bool fault = false;
    inline uint32_t word(uint32_t i) const {
        uint32_t w;
        memcpy(&w, in + 4 * (size_t)i, 4);
        return w;
    }
    inline void check(uint32_t pos, uint32_t n) {
        if ((uint64_t)pos + n > want) { fault = true; fprintf(stderr, "PSHostCtx: write [%u, +%u) outside %u\n", pos, n, want); abort(); }
    }
    inline void put(uint32_t pos, uint32_t b) {
        if (!sym) return;
        check(pos, 1);
        sym[pos] = (uint16_t)b;
    }
    inline void match(uint32_t pos, uint32_t d, uint32_t n) {
        if (!sym) return;
        check(pos, n);
        for (uint32_t i = 0; i < n; ++i) {
            const long long p = (long long)pos + i - d;
            if (p < -(long long)PI_WINDOW) { fprintf(stderr, "PSHostCtx: match source %lld\n", p); abort(); }
            sym[pos + i] = p < 0 ? (uint16_t)(PI_MARK | (uint32_t)(PI_WINDOW + p)) : sym[p];
        }
    }
    inline void stored(uint32_t pos, uint32_t at, uint32_t n) {
        if ((uint64_t)at + n > in_bytes) { fprintf(stderr, "PSHostCtx: stored source [%u, +%u) outside %u\n", at, n, in_bytes); abort(); }
        if (!sym) return;
        check(pos, n);
        for (uint32_t i = 0; i < n; ++i) sym[pos + i] = in[at + i];
    }
    inline int lane() const { return 0; }
    inline int lanes() const { return 1; }
    inline void sync() {}
    inline uint32_t uni(uint32_t v) const { return v; }
    inline uint64_t quick(uint64_t bit, uint64_t end) const {
        uint64_t m = 0;
        for (int j = 0; j < 64; ++j)
            if (bit + j < end && pi_quick_dynamic(in, in_bytes, bit + j)) m |= 1ull << j;
        return m;
    }
    inline bool boundary(uint64_t bit) const {
        const uint64_t k = (bit >> 3) / S;
        return k > self && k < nsegs && segs[k].cand == bit;
    }
};

// rtn_png_stream_inflate_host without the error text: the device's find, count, chain, marker decode, window walk and resolve, one
// after the other on the CPU.  segment_bytes 0: the blob's own.  Returns RTN_OK with *status set, or RTN_EINVAL (*why: the reason).
inline int ps_inflate_host(const void* blob, size_t blob_bytes, uint32_t segment_bytes, uint8_t* out, size_t want_bytes, int32_t* status,
                           const char** why, uint32_t* links_out = nullptr) {
    const PSHdr* hd = ps_blob_any(blob, blob_bytes);
    if (!hd) { *why = "not an rtn_png_stream_inspect or rtn_png_layout_inspect blob"; return RTN_EINVAL; }
    const uint32_t want = (uint32_t)ps_want(hd);
    if (want_bytes != want) { *why = "want_bytes is not the length of the page's filtered stream"; return RTN_EINVAL; }
    uint32_t S = segment_bytes ? segment_bytes : hd->seg_bytes;
    if (S < PS_SEGMENT_MIN || S > PS_SEGMENT_MAX) { *why = "segment_bytes outside 256 .. 2^24"; return RTN_EINVAL; }
    const uint8_t* bl = static_cast<const uint8_t*>(blob);
    const uint32_t in_bytes = hd->in_bytes, nsegs = (in_bytes + S - 1) / S;
    const uint64_t nbits = (uint64_t)in_bytes * 8u;
    std::vector<uint8_t> padded((((size_t)in_bytes + 3) & ~(size_t)3) + 8, 0);
    memcpy(padded.data(), bl + hd->off_data, in_bytes);
    std::vector<PSSeg> segs(nsegs);
    PiTables T;
    memset(&T, 0, sizeof(T));
    uint32_t st = 0;
    // find
    for (uint32_t k = 0; k < nsegs; ++k) {
        PSHostCtx c{padded.data(), in_bytes, segs.data(), nsegs, S, k, nullptr, 0u};
        const uint64_t lo = (uint64_t)k * S * 8u, hi = lo + (uint64_t)S * 8u < nbits ? lo + (uint64_t)S * 8u : nbits;
        segs[k] = PSSeg{k == 0 ? 0ull : pi_find(c, T, in_bytes, lo, hi), 0ull, 0u, 0u, 0u, 0u};
    }
    // count
    for (uint32_t k = 0; k < nsegs; ++k) {
        if (segs[k].cand == PI_NONE) continue;
        PSHostCtx c{padded.data(), in_bytes, segs.data(), nsegs, S, k, nullptr, 0u};
        PiRun run = {0ull, 0u, 0u};
        segs[k].status = (uint32_t)pi_run(c, T, in_bytes, segs[k].cand, k ? PI_WINDOW : 0u, want, &run);
        segs[k].end_bit = run.end_bit; segs[k].out = run.out; segs[k].final = run.final;
    }
    // chain
    std::vector<PSLink> links(nsegs);
    uint32_t nlinks = 0;
    st |= ps_chain(segs.data(), nsegs, S, in_bytes, want, links.data(), &nlinks);
    if (links_out) *links_out = nlinks;
    // decode with markers
    std::vector<uint16_t> sym(want, 0);
    for (uint32_t l = 0; l < nlinks; ++l) {
        const uint32_t k = links[l].seg;
        PSHostCtx c{padded.data(), in_bytes, segs.data(), nsegs, S, k, sym.data() + links[l].off, segs[k].out};
        PiRun run = {0ull, 0u, 0u};
        const int rc = pi_run(c, T, in_bytes, segs[k].cand, k ? PI_WINDOW : 0u, segs[k].out, &run);
        if (rc || run.out != segs[k].out || run.end_bit != segs[k].end_bit) st |= (uint32_t)rc | PI_CHAIN;
    }
    // windows: win[l] ends where link l starts
    std::vector<uint8_t> win((size_t)(nlinks ? nlinks : 1) * PI_WINDOW, 0);
    for (uint32_t l = 0; l + 1 < nlinks; ++l)
        for (uint32_t i = 0; i < PI_WINDOW; ++i)
            win[(size_t)(l + 1) * PI_WINDOW + i] = pi_window_entry(sym.data(), win.data() + (size_t)l * PI_WINDOW, links[l].off,
                                                                   segs[links[l].seg].out, i);
    // resolve, Adler-32
    std::vector<uint8_t> bytes(want, 0);
    uint32_t a = 1, b = 0;
    int bad = 0;
    const uint32_t have = nlinks ? links[nlinks - 1].off + segs[links[nlinks - 1].seg].out : 0u;
    for (uint32_t p = 0; p < have; ++p) {
        const uint32_t l = ps_link_of(links.data(), nlinks, p);
        bytes[p] = pi_resolve(sym[p], win.data() + (size_t)l * PI_WINDOW, links[l].off, &bad);
    }
    for (uint32_t p = 0; p < want; ++p) {
        a = (a + bytes[p]) % PE_ADLER;
        b = (b + a) % PE_ADLER;
    }
    if (bad) st |= PI_DIST;
    if ((b << 16 | a) != hd->adler) st |= PI_ADLER;
    // the IDAT CRCs
    for (uint32_t k = 0; k < hd->nidat; ++k) {
        PSIdat e;
        memcpy(&e, bl + hd->off_table + (size_t)k * sizeof(PSIdat), sizeof(e));
        if ((uint64_t)e.off + e.len > (uint64_t)in_bytes + 6) { st |= PI_CRC; break; }
        uint32_t c = ps_crc(0xffffffffu, reinterpret_cast<const uint8_t*>("IDAT"), 4);
        c = ps_crc(c, bl + hd->off_data - 2 + e.off, e.len);
        if (~c != e.crc) st |= PI_CRC;
    }
    *status = (int32_t)st;
    if (st == 0) memcpy(out, bytes.data(), want);
    return RTN_OK;
}

// rtn_png_layout_pixels_host without the error text: the device's last stage (reconstruct every pass, expand every pixel) on the CPU
// over the filtered stream of a layout blob's page.  Returns RTN_OK with *status set (out written only if it is 0), or RTN_EINVAL.
inline int pl_pixels_host(const void* blob, size_t blob_bytes, const uint8_t* stream, size_t bytes, uint8_t* out, int32_t* status,
                          const char** why) {
    const PSHdr* hd = ps_blob(blob, blob_bytes, PL_MAGIC);
    if (!hd) { *why = "not an rtn_png_layout_inspect blob"; return RTN_EINVAL; }
    PLGeom g;
    pl_geometry(hd->W, hd->H, hd->fmt, &g);
    if ((long long)bytes != g.stream) { *why = "bytes is not the length of the page's filtered stream"; return RTN_EINVAL; }
    std::vector<uint8_t> rec(stream, stream + bytes);
    *status = (int32_t)pl_pixels(g, hd->fmt, hd->W, hd->H, rec.data(), pl_palette(hd), out);
    return RTN_OK;
}
