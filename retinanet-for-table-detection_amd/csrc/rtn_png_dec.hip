// rtn_png_dec.hip — PNG pages of the chunked layout (what csrc/rtn_png_enc.hip writes) decoded on the device, bit-identical
// to Pillow's decode.  The host side (rtn_png_inspect) only takes the file apart: signature, IHDR, one IDAT per chunk of
// RTN_PNG_CHUNK filtered bytes, IEND, nothing else; it copies every IDAT's deflate payload into a blob behind a table of (offset,
// length, stored CRC).  It does not look into the deflate data beyond the bytes the layout fixes: the device vouches for the rest,
// and a page whose status is not 0 is decoded by the caller on the host.
//
// Four kernels per batch of up to RTN_CODEC_BATCH pages; no workgroup waits on another:
//   1. pdec_inflate_kernel: one workgroup of one wave per chunk.  Window (32 KiB) and decode tables in LDS; block loop, table build
//      and symbol decode (csrc/rtn_png_inflate.h) uniform across the wave, payload words fetched 64 at a time into one register per
//      lane, matches copied by all lanes.  Then the chunk's CRC-32 (slices per lane, joined like the encoder's), its Adler pair, the
//      filter-type bytes that fall into it, and the window stored to the page's filtered stream with 16-byte lane stores.
//   2. pdec_page_kernel: one wave per page: joins the Adler pairs (A = A1 + A2 - 1, B = B1 + B2 + len2 (A1 - 1) mod 65521), compares
//      with the stored Adler-32, ORs the chunk status words into the page's.
//   3. pdec_sub_kernel: one workgroup per row: a Sub row becomes its per-channel prefix sum mod 256, in place.
//   4. pdec_up_kernel: one thread per byte column walks down the rows, adds the reconstructed row above on Up rows and writes the
//      (H, W, 3) B,G,R page (R and B swapped, gray replicated).
//
// Why status 0 is enough: every chunk inflated alone, from a byte boundary, through non-final blocks to an empty stored block that
// ends at the payload's last byte, with no match before its first byte.  An inflater reading the concatenated IDATs is therefore at
// a block boundary on a byte boundary wherever a payload ends, decodes the same blocks, and finds every match source inside the
// same chunk: it produces the same bytes, and after the last payload the final block and the Adler-32 the page kernel compared.
#include "rtn_codec_launch.h"
#include "rtn_png_crc.h"
#include "rtn_png_inflate.h"
#include <vector>

namespace {

constexpr int PD_CHUNK = RTN_PNG_CHUNK;
constexpr int PD_WAVE = 64;                    // workgroup of kernels 1 and 2: one wave
constexpr int PD_THREADS = 256;                // workgroup of kernels 3 and 4
constexpr int PD_MAX_GRID = 1 << 20;           // workgroups along x of the Sub launch: rows past it are looped over
constexpr uint32_t PD_MAGIC = 0x444e5052u;     // "RPND"
static_assert(PD_CHUNK == 32768 && PD_CHUNK % (16 * PD_WAVE) == 0, "chunk size");

struct PDHdr {                                 // start of a blob; 64 bytes
    uint32_t magic;
    int32_t W, H, nc, nchunks;
    uint32_t adler;                            // the stream's stored Adler-32
    uint32_t zhdr;                             // the two bytes of the zlib header (CRC of IDAT 0)
    uint32_t off_table;                        // PDEntry[nchunks], from the blob's start
    int64_t blob_bytes, ws_bytes, payload_bytes;
    uint32_t pad_[2];
};
static_assert(sizeof(PDHdr) == 64, "blob header");
struct PDEntry { uint32_t off, len, crc, pad_; };   // payload of chunk k: [off, off + len) from the blob's start, off % 4 == 0, zero padded to a word

struct PDMeta { uint32_t a, b, status, pad_; };     // per chunk: Adler pair of its bytes, PI_* bits

struct PDPage {
    long long blob_off, ws_off, off_meta, stream;
    uint8_t* out;
    int W, H, nc, nchunks;
    uint32_t adler, zhdr, off_table, pad_;
};
struct PDBatch {
    int n, maxchunks, maxrows, maxcols;
    PDPage p[RTN_CODEC_BATCH];
};

inline long long pd_ws_bytes(long long nchunks) { return nchunks * PD_CHUNK + rtn_align256(nchunks * (long long)sizeof(PDMeta)); }

#define pfail(h, ...) rtn_fail_host((h), RTN_EINVAL, __VA_ARGS__)      // a macro, so every message is format-checked

inline uint32_t be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

// ---- the inflate contexts ---------------------------------------------------------------------------------------------------------------
struct PDHostCtx {                             // rtn_png_inflate_chunk_host: one caller does everything
    const uint8_t* in;                         // zero padded to a whole word
    uint8_t* out;
    inline uint32_t word(uint32_t i) const {
        uint32_t w;
        memcpy(&w, in + 4 * (size_t)i, 4);
        return w;
    }
    inline void put(uint32_t pos, uint32_t b) { out[pos] = (uint8_t)b; }
    inline void match(uint32_t pos, uint32_t d, uint32_t n) {
        for (uint32_t i = 0; i < n; ++i) out[pos + i] = out[pos + i - d];
    }
    inline void stored(uint32_t pos, uint32_t at, uint32_t n) { memcpy(out + pos, in + at, n); }
    inline int lane() const { return 0; }
    inline int lanes() const { return 1; }
    inline void sync() {}
    inline uint32_t uni(uint32_t v) const { return v; }
};

struct PDDevCtx {                              // one wave; win and the tables are in LDS
    const uint32_t* w;                         // the payload, word aligned
    uint32_t nwords;
    uint8_t* win;
    int ln;
    uint32_t cache, cbase;                     // words [64 cbase, 64 cbase + 64) of the payload, one per lane
    __device__ inline uint32_t word(uint32_t i) {
        if ((i >> 6) != cbase) {
            cbase = i >> 6;
            const uint32_t j = cbase * 64u + (uint32_t)ln;
            cache = j < nwords ? w[j] : 0u;
        }
        return (uint32_t)__builtin_amdgcn_readlane((int)cache, __builtin_amdgcn_readfirstlane((int)(i & 63u)));
    }
    __device__ inline uint32_t uni(uint32_t v) const { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
    __device__ inline void put(uint32_t pos, uint32_t b) {
        if (ln == 0) win[pos] = (uint8_t)b;
    }
    // all lanes copy; the barrier orders the copy behind the writes before it (one wave: it costs a wait, no other wave is waited for)
    __device__ inline void match(uint32_t pos, uint32_t d, uint32_t n) {
        __syncthreads();
        if (d >= (uint32_t)PD_WAVE) {                                  // a step of 64 bytes reads nothing the same step writes
            for (uint32_t b = 0; b < n; b += PD_WAVE) {
                const uint32_t i = b + (uint32_t)ln;
                if (i < n) win[pos + i] = win[pos + i - d];
                __syncthreads();
            }
        } else {                                                       // the d bytes before pos, repeated
            for (uint32_t b = 0; b < n; b += PD_WAVE) {
                const uint32_t i = b + (uint32_t)ln;
                if (i < n) win[pos + i] = win[pos - d + (d == 1u ? 0u : i % d)];
            }
        }
    }
    __device__ inline void stored(uint32_t pos, uint32_t at, uint32_t n) {
        const uint8_t* in = reinterpret_cast<const uint8_t*>(w);
        for (uint32_t i = (uint32_t)ln; i < n; i += PD_WAVE) win[pos + i] = in[at + i];
    }
    __device__ inline int lane() const { return ln; }
    __device__ inline int lanes() const { return PD_WAVE; }
    __device__ inline void sync() { __syncthreads(); }
};

__device__ inline uint32_t pd_wave_sum(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
    return v;
}
__device__ inline uint32_t pd_wave_xor(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v ^= (uint32_t)__shfl_xor((int)v, o);
    return v;
}
__device__ inline uint32_t pd_wave_or(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v |= (uint32_t)__shfl_xor((int)v, o);
    return v;
}

// ---- kernel 1: one chunk -> its slice of the page's filtered stream ------------------------------------------------------------------------
__global__ __launch_bounds__(PD_WAVE) void pdec_inflate_kernel(const uint8_t* blobs, uint8_t* ws, PDBatch bt) {
    __shared__ __align__(16) uint8_t win[PD_CHUNK];
    __shared__ PiTables T;
    __shared__ uint32_t crctab[256];
    const int page = blockIdx.y;
    if (page >= bt.n) return;
    const PDPage& pg = bt.p[page];
    const int k = blockIdx.x;
    if (k >= pg.nchunks) return;
    const int ln = threadIdx.x;
    const uint8_t* blob = blobs + pg.blob_off;
    const PDEntry e = reinterpret_cast<const PDEntry*>(blob + pg.off_table)[k];
    const long long c0 = (long long)k * PD_CHUNK;
    const uint32_t want = (uint32_t)(pg.stream - c0 < PD_CHUNK ? pg.stream - c0 : PD_CHUNK);    // 1..PD_CHUNK
    const uint32_t* payw = reinterpret_cast<const uint32_t*>(blob + e.off);
    const uint32_t nwords = (e.len + 3u) >> 2;

    for (int i = ln; i < PD_CHUNK / 16; i += PD_WAVE) reinterpret_cast<uint4*>(win)[i] = make_uint4(0u, 0u, 0u, 0u);
    for (int i = ln; i < 256; i += PD_WAVE) {
        uint32_t c = (uint32_t)i;
        for (int j = 0; j < 8; ++j) c = (c & 1u) ? (c >> 1) ^ PE_POLY : c >> 1;
        crctab[i] = c;
    }
    __syncthreads();

    PDDevCtx ctx{payw, nwords, win, ln, 0u, 0xffffffffu};
    uint32_t st = (uint32_t)pi_inflate(ctx, T, e.len, want);
    __syncthreads();

    // ---- CRC-32 of "IDAT" (+ the zlib header in front of chunk 0) + payload (+ final block and Adler-32 behind the last chunk)
    {
        uint32_t crc0 = 0xffffffffu;
        crc0 = pe_crc_byte(crc0, 'I'); crc0 = pe_crc_byte(crc0, 'D'); crc0 = pe_crc_byte(crc0, 'A'); crc0 = pe_crc_byte(crc0, 'T');
        if (k == 0) { crc0 = pe_crc_byte(crc0, pg.zhdr & 255u); crc0 = pe_crc_byte(crc0, (pg.zhdr >> 8) & 255u); }
        const uint32_t clen = e.len;
        const uint32_t per = 4u * ((clen + 4u * PD_WAVE - 1) / (4u * PD_WAVE));             // bytes per lane, whole words
        const uint32_t b0 = (uint32_t)ln * per < clen ? (uint32_t)ln * per : clen;
        const uint32_t b1 = b0 + per < clen ? b0 + per : clen;
        uint32_t r = 0;
        for (uint32_t b = b0; b < b1; b += 4) {
            const uint32_t wv = payw[b >> 2];
            for (uint32_t q = 0; q < 4 && b + q < b1; ++q) r = crctab[(r ^ (wv >> (8 * q))) & 255u] ^ (r >> 8);
        }
        uint32_t part = b1 > b0 ? pe_mulmod(r, pe_xpow8(clen - b1)) : 0u;
        if (ln == 0) part ^= pe_mulmod(crc0, pe_xpow8(clen));
        uint32_t crc = pd_wave_xor(part);
        if (k == pg.nchunks - 1) {
            crc = pe_crc_byte(crc, 1u); crc = pe_crc_byte(crc, 0u); crc = pe_crc_byte(crc, 0u);
            crc = pe_crc_byte(crc, 0xffu); crc = pe_crc_byte(crc, 0xffu);
            for (int s = 24; s >= 0; s -= 8) crc = pe_crc_byte(crc, (pg.adler >> s) & 255u);
        }
        if (~crc != e.crc) st |= PI_CRC;
    }

    // ---- Adler-32 pair of the chunk's bytes: A = 1 + sum d_i, B = n + sum (n - i) d_i; the window past `want` is zero
    uint32_t sa = 0;
    unsigned long long sb = 0;
    for (int i = ln; i < PD_CHUNK / 4; i += PD_WAVE) {
        const uint32_t wv = reinterpret_cast<const uint32_t*>(win)[i];
        for (int q = 0; q < 4; ++q) {
            const uint32_t p = 4u * (uint32_t)i + (uint32_t)q, d = p < want ? (wv >> (8 * q)) & 255u : 0u;
            sa += d;
            sb += (unsigned long long)(want - (p < want ? p : want)) * d;
        }
    }
    const uint32_t A = (1u + pd_wave_sum(sa)) % PE_ADLER;
    const uint32_t B = (want + pd_wave_sum((uint32_t)(sb % PE_ADLER))) % PE_ADLER;

    // ---- the filter-type bytes of the rows that start in this chunk
    {
        const long long rb1 = 1 + (long long)pg.W * pg.nc;
        int bad = 0;
        for (long long r = (c0 + rb1 - 1) / rb1 + ln; r * rb1 < c0 + (long long)want; r += PD_WAVE)
            if (win[r * rb1 - c0] > 2) bad = 1;
        if (__any(bad)) st |= PI_FILTER;
    }

    uint8_t* dst = ws + pg.ws_off + c0;                                // 256-byte aligned; the page's stream region holds whole chunks
    for (uint32_t i = 16u * (uint32_t)ln; i < want; i += 16u * PD_WAVE)
        *reinterpret_cast<uint4*>(dst + i) = *reinterpret_cast<const uint4*>(win + i);
    if (ln == 0) {
        PDMeta m;
        m.a = A; m.b = B; m.status = st; m.pad_ = 0;
        reinterpret_cast<PDMeta*>(ws + pg.ws_off + pg.off_meta)[k] = m;
    }
}

// ---- kernel 2: one page's Adler-32 and status -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PD_WAVE) void pdec_page_kernel(uint8_t* ws, int32_t* status, PDBatch bt) {
    const int page = blockIdx.x;
    if (page >= bt.n) return;
    const PDPage& pg = bt.p[page];
    const int ln = threadIdx.x;
    const PDMeta* meta = reinterpret_cast<const PDMeta*>(ws + pg.ws_off + pg.off_meta);
    uint32_t st = 0, carry = 0, bsum = 0;                               // carry: sum of (A_j - 1) over the chunks before this tile
    for (int k0 = 0; k0 < pg.nchunks; k0 += PD_WAVE) {
        const int k = k0 + ln;
        PDMeta m = {1u, 0u, 0u, 0u};
        if (k < pg.nchunks) m = meta[k];
        st |= m.status;
        const uint32_t a1 = (m.a % PE_ADLER + PE_ADLER - 1u) % PE_ADLER;
        uint32_t incl = a1;
        for (int o = 1; o < PD_WAVE; o <<= 1) {
            const uint32_t v = (uint32_t)__shfl_up((int)incl, o);
            if (ln >= o) incl += v;                                    // < 64 * 65521
        }
        const long long len = k < pg.nchunks ? (pg.stream - (long long)k * PD_CHUNK < PD_CHUNK ? pg.stream - (long long)k * PD_CHUNK : PD_CHUNK) : 0;
        const unsigned long long before = (carry + incl - a1) % PE_ADLER;
        const uint32_t term = k < pg.nchunks ? (uint32_t)((m.b % PE_ADLER + (unsigned long long)len * before) % PE_ADLER) : 0u;
        bsum = (bsum + pd_wave_sum(term)) % PE_ADLER;
        carry = (carry + (uint32_t)__shfl((int)incl, PD_WAVE - 1)) % PE_ADLER;
    }
    st = pd_wave_or(st);
    const uint32_t adler = bsum << 16 | (1u + carry) % PE_ADLER;
    if (adler != pg.adler) st |= PI_ADLER;
    if (ln == 0) status[page] = (int32_t)st;
}

// ---- kernel 3: Sub rows ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PD_THREADS) void pdec_sub_kernel(uint8_t* ws, PDBatch bt) {
    __shared__ uint32_t tot[3][PD_THREADS / 64];
    const int page = blockIdx.y;
    if (page >= bt.n) return;
    const PDPage& pg = bt.p[page];
    const int nc = pg.nc, W = pg.W, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long long rb1 = 1 + (long long)W * nc;
    const int per = (W + PD_THREADS - 1) / PD_THREADS;                 // pixels per thread
    const long long x0 = (long long)tid * per < W ? (long long)tid * per : W, x1 = x0 + per < W ? x0 + per : W;
    for (int y = blockIdx.x; y < pg.H; y += gridDim.x) {
        uint8_t* row = ws + pg.ws_off + (long long)y * rb1;
        if (row[0] != 1) continue;                                     // the same for the whole workgroup
        uint32_t s[3] = {0u, 0u, 0u};
        for (long long x = x0; x < x1; ++x)
            for (int c = 0; c < nc; ++c) s[c] += row[1 + x * nc + c];
        uint32_t excl[3] = {0u, 0u, 0u};
        for (int c = 0; c < nc; ++c) {                                 // exclusive scan of the threads' sums (mod 2^32, used mod 256)
            uint32_t incl = s[c];
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t v = (uint32_t)__shfl_up((int)incl, o);
                if (lane >= o) incl += v;
            }
            if (lane == 63) tot[c][wv] = incl;
            excl[c] = incl - s[c];
        }
        __syncthreads();
        for (int c = 0; c < nc; ++c)
            for (int w = 0; w < wv; ++w) excl[c] += tot[c][w];
        for (long long x = x0; x < x1; ++x)
            for (int c = 0; c < nc; ++c) {
                excl[c] += row[1 + x * nc + c];
                row[1 + x * nc + c] = (uint8_t)excl[c];
            }
        __syncthreads();                                               // tot[] is reused by the next row
    }
}

// ---- kernel 4: Up rows and the page -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PD_THREADS) void pdec_up_kernel(const uint8_t* ws, PDBatch bt) {
    const int page = blockIdx.y;
    if (page >= bt.n) return;
    const PDPage& pg = bt.p[page];
    const long long rb = (long long)pg.W * pg.nc, rb1 = rb + 1;
    const long long col = (long long)blockIdx.x * PD_THREADS + threadIdx.x;
    if (col >= rb) return;
    const uint8_t* src = ws + pg.ws_off;
    const int nc = pg.nc;
    const long long px = nc == 3 ? col / 3 : col;
    const int ch = nc == 3 ? 2 - (int)(col - px * 3) : 0;              // R,G,B in the file -> B,G,R in the page
    uint8_t* out = pg.out + px * 3 + ch;
    const long long orow = (long long)pg.W * 3;
    constexpr int U = 8;
    uint32_t prev = 0;
    for (int y0 = 0; y0 < pg.H; y0 += U) {
        uint32_t v[U], t[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool in = y0 + u < pg.H;
            const uint8_t* row = src + (long long)(y0 + u) * rb1;
            t[u] = in ? row[0] : 0u;
            v[u] = in ? row[1 + col] : 0u;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (y0 + u >= pg.H) break;
            prev = t[u] == 2u ? (v[u] + prev) & 255u : v[u];
            uint8_t* o = out + (long long)(y0 + u) * orow;
            o[0] = (uint8_t)prev;
            if (nc == 1) { o[1] = (uint8_t)prev; o[2] = (uint8_t)prev; }
        }
    }
}

// off >= 0: the callers (rtn_codec_blobs, and the walk behind it) have looked at the sign
const PDHdr* pd_blob(const void* host_blobs, int64_t off) {
    const PDHdr* hd = reinterpret_cast<const PDHdr*>(static_cast<const uint8_t*>(host_blobs) + off);
    return (hd->magic == PD_MAGIC && hd->nchunks > 0 && hd->ws_bytes > 0) ? hd : nullptr;
}

}  // namespace

// rtn_png_inspect / rtn_png_decode_workspace_bytes / rtn_png_decode / rtn_png_inflate_chunk_host: see include/rtn.h
extern "C" int rtn_png_inspect(rtn_handle_t h, const void* file, size_t file_bytes, rtn_png_info_t* info, void* blob_out,
                               size_t blob_capacity) {
    if (!info) return pfail(h, "rtn_png_inspect: info is NULL");
    memset(info, 0, sizeof(*info));
    if (!file) return pfail(h, "rtn_png_inspect: file is NULL");
    const uint8_t* f = static_cast<const uint8_t*>(file);
    const size_t n = file_bytes;
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    if (n < 8 || memcmp(f, sig, 8) != 0) return pfail(h, "not a PNG file (no signature)");
    if (n >= ((size_t)1 << 30)) return pfail(h, "file larger than 1 GiB");
    if (n < 8 + 25) return pfail(h, "truncated PNG (no IHDR)");
    if (be32(f + 8) != 13 || memcmp(f + 12, "IHDR", 4) != 0) return pfail(h, "the first chunk is not a 13-byte IHDR");
    {
        uint32_t c = 0xffffffffu;
        for (int i = 12; i < 29; ++i) c = pe_crc_byte(c, f[i]);
        if (~c != be32(f + 29)) return pfail(h, "CRC of IHDR");
    }
    const uint32_t W = be32(f + 16), H = be32(f + 20);
    const int depth = f[24], ctype = f[25];
    if (depth != 8) return pfail(h, "bit depth %d (only 8-bit PNG is decoded on the device)", depth);
    if (ctype != 0 && ctype != 2) return pfail(h, "colour type %d (only gray and R,G,B are decoded on the device)", ctype);
    if (f[26] != 0 || f[27] != 0) return pfail(h, "compression method %d, filter method %d", f[26], f[27]);
    if (f[28] != 0) return pfail(h, "interlaced PNG");
    const int nc = ctype == 2 ? 3 : 1;
    if (W < 1 || H < 1 || W > 0x7fffffffu || H > 0x7fffffffu) return pfail(h, "PNG sides %u x %u", W, H);
    const unsigned long long rb1 = 1ull + (unsigned long long)W * nc;
    if (rb1 >= (1ull << 31) || (unsigned long long)H * rb1 >= (1ull << 31))
        return pfail(h, "%u x %u page: height * (1 + width * components) must be < 2^31", W, H);
    const long long stream = (long long)((unsigned long long)H * rb1);
    const long long nchunks = (stream + PD_CHUNK - 1) / PD_CHUNK;

    struct Part { size_t at; uint32_t len, crc; };
    std::vector<Part> parts;
    parts.reserve((size_t)nchunks);
    size_t pos = 8 + 25;
    uint32_t adler = 0, zhdr = 0;
    long long payload = 0;
    for (long long k = 0; k < nchunks; ++k) {
        if (n - pos < 12) return pfail(h, "truncated PNG (IDAT %lld of %lld)", k, nchunks);
        const uint32_t len = be32(f + pos);
        if (memcmp(f + pos + 4, "IDAT", 4) != 0) {
            if (memcmp(f + pos + 4, "IEND", 4) == 0) return pfail(h, "%lld IDAT chunks, the chunked layout has %lld", k, nchunks);
            return pfail(h, "chunk %02x %02x %02x %02x (the chunked layout has IHDR, IDAT and IEND only)", f[pos + 4], f[pos + 5], f[pos + 6],
                         f[pos + 7]);
        }
        if ((size_t)len > n - pos - 12) return pfail(h, "truncated PNG (IDAT %lld runs past the file)", k);
        size_t a = pos + 8, b = a + len;                               // the deflate payload is [a, b)
        if (k == 0) {
            if (b - a < 2) return pfail(h, "IDAT 0 has no zlib header");
            const int cmf = f[a], flg = f[a + 1];
            if ((cmf & 15) != 8 || (cmf >> 4) > 7 || (flg & 0x20) || (cmf * 256 + flg) % 31 != 0)
                return pfail(h, "bad zlib header %02x %02x", cmf, flg);
            zhdr = (uint32_t)cmf | (uint32_t)flg << 8;
            a += 2;
        }
        if (k == nchunks - 1) {
            static const uint8_t fin[5] = {1, 0, 0, 0xff, 0xff};
            if (b - a < 9 || memcmp(f + b - 9, fin, 5) != 0)
                return pfail(h, "the last IDAT does not end with a final empty stored block and the Adler-32");
            adler = be32(f + b - 4);
            b -= 9;
        }
        static const uint8_t sync[4] = {0, 0, 0xff, 0xff};
        if (b - a < 5 || memcmp(f + b - 4, sync, 4) != 0) return pfail(h, "IDAT %lld does not end with an empty stored block", k);
        parts.push_back({a, (uint32_t)(b - a), be32(f + pos + 8 + len)});
        payload += (long long)(b - a);
        pos += 12 + (size_t)len;
    }
    if (n - pos < 12) return pfail(h, "truncated PNG (no IEND)");
    if (memcmp(f + pos + 4, "IDAT", 4) == 0) return pfail(h, "more than %lld IDAT chunks", nchunks);
    if (memcmp(f + pos + 4, "IEND", 4) != 0)
        return pfail(h, "chunk %02x %02x %02x %02x (the chunked layout has IHDR, IDAT and IEND only)", f[pos + 4], f[pos + 5], f[pos + 6],
                     f[pos + 7]);
    if (be32(f + pos) != 0 || be32(f + pos + 8) != 0xae426082u) return pfail(h, "IEND is not empty or its CRC is wrong");
    if (pos + 12 != n) return pfail(h, "%zu bytes after IEND", n - pos - 12);

    size_t total = sizeof(PDHdr) + (size_t)nchunks * sizeof(PDEntry);
    for (const Part& p : parts) total += ((size_t)p.len + 3) & ~(size_t)3;
    total = (total + 15) & ~(size_t)15;
    info->width = (int32_t)W; info->height = (int32_t)H; info->components = nc; info->chunks = (int32_t)nchunks;
    info->blob_bytes = (int64_t)total;
    info->workspace_bytes = pd_ws_bytes(nchunks);
    info->payload_bytes = payload;
    if (!blob_out) return RTN_OK;
    if (total > RTN_PNG_BLOB_BOUND(n)) return pfail(h, "internal: blob bound");
    if (blob_capacity < total) return pfail(h, "rtn_png_inspect: blob capacity %zu < %zu bytes", blob_capacity, total);
    uint8_t* bl = static_cast<uint8_t*>(blob_out);
    PDHdr hd;
    memset(&hd, 0, sizeof(hd));
    hd.magic = PD_MAGIC;
    hd.W = (int32_t)W; hd.H = (int32_t)H; hd.nc = nc; hd.nchunks = (int32_t)nchunks;
    hd.adler = adler; hd.zhdr = zhdr;
    hd.off_table = (uint32_t)sizeof(PDHdr);
    hd.blob_bytes = (int64_t)total; hd.ws_bytes = info->workspace_bytes; hd.payload_bytes = payload;
    memcpy(bl, &hd, sizeof(hd));
    size_t at = sizeof(PDHdr) + (size_t)nchunks * sizeof(PDEntry);
    for (long long k = 0; k < nchunks; ++k) {
        const Part& p = parts[(size_t)k];
        const PDEntry e = {(uint32_t)at, p.len, p.crc, 0u};
        memcpy(bl + sizeof(PDHdr) + (size_t)k * sizeof(PDEntry), &e, sizeof(e));
        memcpy(bl + at, f + p.at, p.len);
        const size_t padded = ((size_t)p.len + 3) & ~(size_t)3;
        memset(bl + at + p.len, 0, padded - p.len);
        at += padded;
    }
    memset(bl + at, 0, total - at);
    return RTN_OK;
}

extern "C" int rtn_png_inflate_chunk_host(const void* in, size_t in_bytes, void* out, size_t want_bytes, int32_t* status) {
    if (!in || !out || !status) { rtn_set_host_error("rtn_png_inflate_chunk_host: NULL argument"); return RTN_EINVAL; }
    if (want_bytes < 1 || want_bytes > (size_t)PD_CHUNK || in_bytes >= ((size_t)1 << 30)) {
        rtn_set_host_error("rtn_png_inflate_chunk_host: want_bytes must be 1..RTN_PNG_CHUNK, in_bytes < 2^30");
        return RTN_EINVAL;
    }
    std::vector<uint8_t> padded(((in_bytes + 3) & ~(size_t)3) + 4, 0);
    memcpy(padded.data(), in, in_bytes);
    std::vector<uint8_t> win(want_bytes, 0);
    PiTables T;
    memset(&T, 0, sizeof(T));
    PDHostCtx ctx{padded.data(), win.data()};
    int st = PI_TRUNC;
    static const uint8_t sync[4] = {0, 0, 0xff, 0xff};
    if (in_bytes >= 5 && memcmp(padded.data() + in_bytes - 4, sync, 4) == 0) st = pi_inflate(ctx, T, (uint32_t)in_bytes, (uint32_t)want_bytes);
    *status = st;
    if (st == 0) memcpy(out, win.data(), want_bytes);
    return RTN_OK;
}

extern "C" size_t rtn_png_decode_workspace_bytes(int n, const void* host_blobs, const int64_t* offsets) {
    return rtn_codec_blob_bytes(n, host_blobs, offsets, pd_blob);
}

extern "C" int rtn_png_decode(rtn_handle_t h, int n, const void* host_blobs, const void* dev_blobs, const int64_t* offsets,
                              uint8_t* const* pages, int32_t* status, void* workspace, size_t workspace_bytes) {
    const int rc = rtn_decode_check(h, "rtn_png_decode", "rtn_png_inspect", n, host_blobs, dev_blobs, offsets, pages, status, workspace,
                                    workspace_bytes, pd_blob, rtn_codec_no_extra);
    if (rc != RTN_CODEC_GO) return rc;
    const uint8_t* db = static_cast<const uint8_t*>(dev_blobs);
    uint8_t* wsp = static_cast<uint8_t*>(workspace);
    long long maxcols = 0;
    return rtn_codec_walk<PDBatch>(n,
        [&](PDBatch& bt, int k, int i, long long ws) {
            const PDHdr* hd = pd_blob(host_blobs, offsets[i]);
            if (k == 0) maxcols = 0;
            PDPage& p = bt.p[k];
            p.blob_off = offsets[i];
            p.ws_off = ws;
            p.off_meta = (long long)hd->nchunks * PD_CHUNK;
            p.stream = (long long)hd->H * (1 + (long long)hd->W * hd->nc);
            p.out = pages[i];
            p.W = hd->W; p.H = hd->H; p.nc = hd->nc; p.nchunks = hd->nchunks;
            p.adler = hd->adler; p.zhdr = hd->zhdr; p.off_table = hd->off_table;
            bt.maxchunks = p.nchunks > bt.maxchunks ? p.nchunks : bt.maxchunks;
            bt.maxrows = p.H > bt.maxrows ? p.H : bt.maxrows;
            maxcols = (long long)p.W * p.nc > maxcols ? (long long)p.W * p.nc : maxcols;
            return (long long)hd->ws_bytes;
        },
        [&](const PDBatch& bt, int i0) {
            pdec_inflate_kernel<<<dim3(bt.maxchunks, bt.n), PD_WAVE, 0, h->stream>>>(db, wsp, bt);
            RTN_CHECK_LAUNCH(h, "pdec_inflate_kernel");
            pdec_page_kernel<<<bt.n, PD_WAVE, 0, h->stream>>>(wsp, status + i0, bt);
            RTN_CHECK_LAUNCH(h, "pdec_page_kernel");
            pdec_sub_kernel<<<dim3(rtn_min_grid(bt.maxrows, PD_MAX_GRID), bt.n), PD_THREADS, 0, h->stream>>>(wsp, bt);
            RTN_CHECK_LAUNCH(h, "pdec_sub_kernel");
            pdec_up_kernel<<<dim3((unsigned)((maxcols + PD_THREADS - 1) / PD_THREADS), bt.n), PD_THREADS, 0, h->stream>>>(wsp, bt);
            RTN_CHECK_LAUNCH(h, "pdec_up_kernel");
            return RTN_OK;
        });
}
