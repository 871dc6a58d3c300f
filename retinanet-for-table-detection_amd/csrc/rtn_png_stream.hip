// rtn_png_stream.hip — ordinary PNG pages (one zlib stream over any number of IDATs, all five row filters) decoded on the device,
// bit-identical to Pillow's decode.  The host side (csrc/rtn_png_stream.h) takes the file apart and cuts the deflate
// bytes into segments of S compressed bytes; it does not inflate.  Deflate blocks are independent but for the 32 KiB window, so
// the page is inflated by as many waves as it has segments that hold a block start:
//
//   1. psd_find_kernel     one wave per segment: the first bit offset in the segment that passes the dynamic-block-header test
//                          (segment 0: the stream's first bit).  A false candidate costs time, never correctness (see 3).
//   2. psd_count_kernel    one wave per candidate: decodes tokens without writing until it lands, at a block boundary, on a later
//                          segment's candidate, or has decoded the final block; records the landing and the bytes produced.
//   3. psd_crc_kernel      one wave per IDAT: CRC-32 in slices, joined (csrc/rtn_png_crc.h).
//      psd_chain_kernel    one lane per page: follows the landings from segment 0 (ps_chain) and turns byte counts into offsets.
//                          Only what the true decode from the stream's first bit reaches is on the chain.
//   4. psd_decode_kernel   one wave per link: decodes again, writing 16-bit symbols at the link's offset: a byte, or PI_MARK | i for
//                          "byte i of the 32 KiB before this link's first byte".  The window is a ring of 32 Ki symbols in LDS.
//   5. psd_window_kernel   one workgroup per page walks the links in order: the 32 KiB that end where link l ends, from the window
//                          that ends where it starts (parallel over the 32 Ki entries, serial over the links).
//   6. psd_resolve_kernel  one workgroup per 32 KiB of the filtered stream: symbols -> bytes, Adler pair, filter-type check.
//   7. psd_page_kernel     one lane per page: joins the Adler pairs, ORs the status words.
//   8. psd_unfilter_kernel one workgroup per page: thread t of a band of 1024 rows computes pixel s - t of its row at step s, so
//                          the row above is always one pixel ahead (what Average and Paeth need); writes the B,G,R page.
// rtn_png_layout_decode (pages of the other pixel layouts: sub-byte gray, palette, alpha, 16-bit samples, Adam7; csrc/rtn_png_layout.h)
// runs stages 1 - 7 unchanged (the page record carries the stream's length and the format word) and then, instead of 8:
//   8a. pld_unfilter_kernel one workgroup per page and pass: the same schedule over filter units of 1 .. 8 bytes, in place.
//   8b. pld_expand_kernel   one thread per four pixels of the page: sample -> B,G,R, every pass gathered into the page.
// No workgroup waits on another, no loop's end depends on file bytes alone, and every position derived from them is checked before
// use.  Any non-zero status word sends the page to the host decoder.
#include "rtn_codec_launch.h"
#include "rtn_png_stream.h"

namespace {

constexpr int PS_WAVE = 64;
constexpr int PS_THREADS = 256;                // resolve
constexpr int PS_BAND = 1024;                  // rows per band of the unfilter kernel = its workgroup; window kernel too
constexpr int PS_MAX_GRID = 4096;              // workgroups along x of the CRC launch: IDATs past it are looped over

struct PSPage {
    long long blob_off, ws_off;
    uint8_t* out;
    int32_t W, H, nc;
    uint32_t nsegs, nidat, S, in_bytes, adler, off_table, off_data;
    uint32_t stream, fmt;                      // the filtered stream's length (ps_want) and the page's format word (ps_fmt)
};
struct PSBatch {
    int n, pad_;
    PSPage p[RTN_CODEC_BATCH];
};
static_assert(sizeof(PSBatch) <= 3072, "kernel arguments");

__device__ inline long long ps_stream(const PSPage& pg) { return (long long)pg.stream; }

template <bool WRITE>
struct PSDevCtx {                              // one wave; the tables (and the ring) are in LDS
    const uint32_t* w;                         // the deflate bytes, word aligned, a zero word behind them
    uint32_t in_bytes, nwords;
    const PSSeg* segs;
    uint32_t nsegs, S, self;
    uint16_t* ring;                            // PI_WINDOW symbols
    uint16_t* g;                               // the link's symbols in the workspace
    int ln;
    uint32_t cache, cbase;                     // words [64 cbase, 64 cbase + 64), one per lane
    __device__ inline uint32_t word(uint32_t i) {
        if ((i >> 6) != cbase) {
            cbase = i >> 6;
            const uint32_t j = cbase * 64u + (uint32_t)ln;
            cache = j < nwords ? w[j] : 0u;
        }
        return (uint32_t)__builtin_amdgcn_readlane((int)cache, __builtin_amdgcn_readfirstlane((int)(i & 63u)));
    }
    __device__ inline uint32_t uni(uint32_t v) const { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
    __device__ inline int lane() const { return ln; }
    __device__ inline int lanes() const { return PS_WAVE; }
    __device__ inline void sync() { __syncthreads(); }
    __device__ inline uint64_t quick(uint64_t bit, uint64_t end) const {
        const uint64_t b = bit + (uint64_t)ln;
        return __ballot(b < end && pi_quick_dynamic(reinterpret_cast<const uint8_t*>(w), in_bytes, b));
    }
    __device__ inline bool boundary(uint64_t bit) const {
        const uint64_t k = (bit >> 3) / S;
        return k > self && k < nsegs && segs[k].cand == bit;
    }
    __device__ inline uint16_t src(int p) const {                      // symbol at position p of the link; p >= -PI_WINDOW
        return p < 0 ? (uint16_t)(PI_MARK | (uint32_t)((int)PI_WINDOW + p)) : ring[(uint32_t)p & (PI_WINDOW - 1u)];
    }
    __device__ inline void put(uint32_t pos, uint32_t b) {
        if (!WRITE) return;
        if (ln == 0) {
            ring[pos & (PI_WINDOW - 1u)] = (uint16_t)b;
            g[pos] = (uint16_t)b;
        }
    }
    // all lanes copy; the barrier orders the copy behind the writes before it (one wave: no other wave is waited for)
    __device__ inline void match(uint32_t pos, uint32_t d, uint32_t n) {
        if (!WRITE) return;
        __syncthreads();
        if (d >= (uint32_t)PS_WAVE) {                                  // a step of 64 symbols reads nothing the same step writes
            for (uint32_t b = 0; b < n; b += PS_WAVE) {
                const uint32_t i = b + (uint32_t)ln;
                if (i < n) {
                    const uint16_t v = src((int)(pos + i) - (int)d);
                    ring[(pos + i) & (PI_WINDOW - 1u)] = v;
                    g[pos + i] = v;
                }
                __syncthreads();
            }
        } else {                                                       // the d symbols before pos, repeated
            for (uint32_t b = 0; b < n; b += PS_WAVE) {
                const uint32_t i = b + (uint32_t)ln;
                if (i < n) {
                    const uint16_t v = src((int)pos - (int)d + (int)(d == 1u ? 0u : i % d));
                    ring[(pos + i) & (PI_WINDOW - 1u)] = v;
                    g[pos + i] = v;
                }
            }
        }
    }
    __device__ inline void stored(uint32_t pos, uint32_t at, uint32_t n) {
        if (!WRITE) return;
        const uint8_t* in = reinterpret_cast<const uint8_t*>(w);
        for (uint32_t i = (uint32_t)ln; i < n; i += PS_WAVE) {         // positions PI_WINDOW apart belong to the same lane, in order
            ring[(pos + i) & (PI_WINDOW - 1u)] = in[at + i];
            g[pos + i] = in[at + i];
        }
    }
};

__device__ inline uint32_t ps_wave_sum(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
    return v;
}
__device__ inline uint32_t ps_wave_xor(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v ^= (uint32_t)__shfl_xor((int)v, o);
    return v;
}

// ---- kernel 1: candidates --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PS_WAVE) void psd_find_kernel(const uint8_t* blobs, uint8_t* ws, PSBatch bt) {
    __shared__ PiTables T;
    const int page = blockIdx.y;
    if (page >= bt.n) return;
    const PSPage& pg = bt.p[page];
    const uint32_t k = blockIdx.x;
    if (k >= pg.nsegs) return;
    const int ln = threadIdx.x;
    const PSLayout lay = ps_layout(ps_stream(pg), pg.nsegs);
    PSSeg* segs = reinterpret_cast<PSSeg*>(ws + pg.ws_off + lay.seg);
    uint64_t cand = 0;
    if (k > 0) {
        PSDevCtx<false> ctx{reinterpret_cast<const uint32_t*>(blobs + pg.blob_off + pg.off_data), pg.in_bytes, (pg.in_bytes + 3u) >> 2,
                            segs, pg.nsegs, pg.S, k, nullptr, nullptr, ln, 0u, 0xffffffffu};
        const uint64_t nbits = (uint64_t)pg.in_bytes * 8u, lo = (uint64_t)k * pg.S * 8u;
        const uint64_t hi = lo + (uint64_t)pg.S * 8u < nbits ? lo + (uint64_t)pg.S * 8u : nbits;
        cand = pi_find(ctx, T, pg.in_bytes, lo, hi);
    }
    if (ln == 0) {
        PSSeg s;
        s.cand = cand; s.end_bit = 0; s.out = 0; s.final = 0; s.status = 0; s.pad_ = 0;
        segs[k] = s;
        if (k == 0) {
            PSHead hd = {0u, 0u, {0u, 0u}};
            *reinterpret_cast<PSHead*>(ws + pg.ws_off + lay.chain) = hd;
        }
    }
}

// ---- kernel 2: where every candidate lands, and after how many bytes ---------------------------------------------------------------------
__global__ __launch_bounds__(PS_WAVE) void psd_count_kernel(const uint8_t* blobs, uint8_t* ws, PSBatch bt) {
    __shared__ PiTables T;
    const int page = blockIdx.y;
    if (page >= bt.n) return;
    const PSPage& pg = bt.p[page];
    const uint32_t k = blockIdx.x;
    if (k >= pg.nsegs) return;
    const int ln = threadIdx.x;
    const long long stream = ps_stream(pg);
    const PSLayout lay = ps_layout(stream, pg.nsegs);
    PSSeg* segs = reinterpret_cast<PSSeg*>(ws + pg.ws_off + lay.seg);
    const uint64_t cand = segs[k].cand;
    if (cand == PI_NONE) return;
    PSDevCtx<false> ctx{reinterpret_cast<const uint32_t*>(blobs + pg.blob_off + pg.off_data), pg.in_bytes, (pg.in_bytes + 3u) >> 2,
                        segs, pg.nsegs, pg.S, k, nullptr, nullptr, ln, 0u, 0xffffffffu};
    PiRun run = {0ull, 0u, 0u};
    const int rc = pi_run(ctx, T, pg.in_bytes, cand, k ? PI_WINDOW : 0u, (uint32_t)stream, &run);
    if (ln == 0) {
        segs[k].end_bit = run.end_bit;
        segs[k].out = run.out;
        segs[k].final = run.final;
        segs[k].status = (uint32_t)rc;
    }
}

// ---- kernel 3a: the IDATs' CRC-32 ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PS_WAVE) void psd_crc_kernel(const uint8_t* blobs, uint8_t* ws, PSBatch bt) {
    __shared__ uint32_t crctab[256];
    const int page = blockIdx.y;
    if (page >= bt.n) return;
    const PSPage& pg = bt.p[page];
    const int ln = threadIdx.x;
    for (int i = ln; i < 256; i += PS_WAVE) {
        uint32_t c = (uint32_t)i;
        for (int j = 0; j < 8; ++j) c = (c & 1u) ? (c >> 1) ^ PE_POLY : c >> 1;
        crctab[i] = c;
    }
    __syncthreads();
    const uint8_t* blob = blobs + pg.blob_off;
    const uint8_t* z = blob + pg.off_data - 2;                         // the zlib stream: in_bytes + 6 bytes
    const PSLayout lay = ps_layout(ps_stream(pg), pg.nsegs);
    int bad = 0;
    for (uint32_t k = blockIdx.x; k < pg.nidat; k += gridDim.x) {
        const PSIdat e = reinterpret_cast<const PSIdat*>(blob + pg.off_table)[k];
        if ((uint64_t)e.off + e.len > (uint64_t)pg.in_bytes + 6u) { bad = 1; continue; }
        uint32_t crc0 = 0xffffffffu;
        crc0 = pe_crc_byte(crc0, 'I'); crc0 = pe_crc_byte(crc0, 'D'); crc0 = pe_crc_byte(crc0, 'A'); crc0 = pe_crc_byte(crc0, 'T');
        const uint32_t clen = e.len;
        const uint32_t per = (clen + PS_WAVE - 1) / PS_WAVE;           // bytes per lane
        const uint32_t b0 = (uint32_t)ln * per < clen ? (uint32_t)ln * per : clen;
        const uint32_t b1 = b0 + per < clen ? b0 + per : clen;
        uint32_t r = 0;
        for (uint32_t b = b0; b < b1; ++b) r = crctab[(r ^ z[e.off + b]) & 255u] ^ (r >> 8);
        uint32_t part = b1 > b0 ? pe_mulmod(r, pe_xpow8(clen - b1)) : 0u;
        if (ln == 0) part ^= pe_mulmod(crc0, pe_xpow8(clen));
        if (~ps_wave_xor(part) != e.crc) bad = 1;
    }
    if (bad && ln == 0) atomicOr(&reinterpret_cast<PSHead*>(ws + pg.ws_off + lay.chain)->status, (uint32_t)PI_CRC);
}

// ---- kernel 3b: the chain --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PS_WAVE) void psd_chain_kernel(uint8_t* ws, PSBatch bt) {
    const int page = blockIdx.x;
    if (page >= bt.n || threadIdx.x != 0) return;
    const PSPage& pg = bt.p[page];
    const long long stream = ps_stream(pg);
    const PSLayout lay = ps_layout(stream, pg.nsegs);
    const PSSeg* segs = reinterpret_cast<const PSSeg*>(ws + pg.ws_off + lay.seg);
    PSHead* hd = reinterpret_cast<PSHead*>(ws + pg.ws_off + lay.chain);
    uint32_t nlinks = 0;
    const uint32_t st = ps_chain(segs, pg.nsegs, pg.S, pg.in_bytes, (uint32_t)stream, reinterpret_cast<PSLink*>(hd + 1), &nlinks);
    hd->nlinks = nlinks;
    if (st) atomicOr(&hd->status, st);
}

// ---- kernel 4: symbols -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PS_WAVE) void psd_decode_kernel(const uint8_t* blobs, uint8_t* ws, PSBatch bt) {
    __shared__ uint16_t ring[PI_WINDOW];
    __shared__ PiTables T;
    const int page = blockIdx.y;
    if (page >= bt.n) return;
    const PSPage& pg = bt.p[page];
    const uint32_t l = blockIdx.x;
    const long long stream = ps_stream(pg);
    const PSLayout lay = ps_layout(stream, pg.nsegs);
    PSHead* hd = reinterpret_cast<PSHead*>(ws + pg.ws_off + lay.chain);
    if (l >= hd->nlinks || l >= pg.nsegs) return;
    const PSLink link = reinterpret_cast<const PSLink*>(hd + 1)[l];
    if (link.seg >= pg.nsegs) return;
    const PSSeg* segs = reinterpret_cast<const PSSeg*>(ws + pg.ws_off + lay.seg);
    const PSSeg seg = segs[link.seg];
    if ((long long)link.off + seg.out > stream) return;                // ps_chain checked it
    const int ln = threadIdx.x;
    PSDevCtx<true> ctx{reinterpret_cast<const uint32_t*>(blobs + pg.blob_off + pg.off_data), pg.in_bytes, (pg.in_bytes + 3u) >> 2,
                       segs, pg.nsegs, pg.S, link.seg, ring, reinterpret_cast<uint16_t*>(ws + pg.ws_off + lay.sym) + link.off, ln, 0u,
                       0xffffffffu};
    PiRun run = {0ull, 0u, 0u};
    const int rc = pi_run(ctx, T, pg.in_bytes, seg.cand, link.seg ? PI_WINDOW : 0u, seg.out, &run);
    if (ln == 0 && (rc || run.out != seg.out || run.end_bit != seg.end_bit)) atomicOr(&hd->status, (uint32_t)rc | (uint32_t)PI_CHAIN);
}

// ---- kernel 5: the window before every link ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PS_BAND) void psd_window_kernel(uint8_t* ws, PSBatch bt) {
    const int page = blockIdx.x;
    if (page >= bt.n) return;
    const PSPage& pg = bt.p[page];
    const PSLayout lay = ps_layout(ps_stream(pg), pg.nsegs);
    const PSHead* hd = reinterpret_cast<const PSHead*>(ws + pg.ws_off + lay.chain);
    const PSLink* links = reinterpret_cast<const PSLink*>(hd + 1);
    const PSSeg* segs = reinterpret_cast<const PSSeg*>(ws + pg.ws_off + lay.seg);
    const uint16_t* sym = reinterpret_cast<const uint16_t*>(ws + pg.ws_off + lay.sym);
    uint8_t* win = ws + pg.ws_off + lay.win;
    const uint32_t nlinks = hd->nlinks < pg.nsegs ? hd->nlinks : pg.nsegs;
    for (uint32_t i = threadIdx.x; i < PI_WINDOW; i += PS_BAND) win[i] = 0;
    for (uint32_t l = 0; l + 1 < nlinks; ++l) {
        __syncthreads();                                               // the window before link l is complete
        const PSLink link = links[l];
        const uint32_t n = segs[link.seg < pg.nsegs ? link.seg : 0u].out;
        const uint8_t* prev = win + (size_t)l * PI_WINDOW;
        for (uint32_t i = threadIdx.x; i < PI_WINDOW; i += PS_BAND) win[(size_t)(l + 1) * PI_WINDOW + i] = pi_window_entry(sym, prev, link.off, n, i);
    }
}

// ---- kernel 6: bytes ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PS_THREADS) void psd_resolve_kernel(uint8_t* ws, PSBatch bt) {
    __shared__ uint32_t red[2][PS_THREADS / 64];
    __shared__ PLGeom geom;
    const int page = blockIdx.y;
    if (page >= bt.n) return;
    const PSPage& pg = bt.p[page];
    const long long stream = ps_stream(pg);
    const PSLayout lay = ps_layout(stream, pg.nsegs);
    const long long j = blockIdx.x;
    if (j >= lay.nchunks) return;
    const PSHead* hd = reinterpret_cast<const PSHead*>(ws + pg.ws_off + lay.chain);
    const PSLink* links = reinterpret_cast<const PSLink*>(hd + 1);
    const PSSeg* segs = reinterpret_cast<const PSSeg*>(ws + pg.ws_off + lay.seg);
    const uint16_t* sym = reinterpret_cast<const uint16_t*>(ws + pg.ws_off + lay.sym);
    const uint8_t* win = ws + pg.ws_off + lay.win;
    uint8_t* dst = ws + pg.ws_off + j * PS_CHUNK;
    const uint32_t nlinks = hd->nlinks < pg.nsegs ? hd->nlinks : pg.nsegs;
    uint32_t have = 0;                                                 // bytes the chain covers
    if (nlinks) {
        const PSLink last = links[nlinks - 1];
        have = last.off + segs[last.seg < pg.nsegs ? last.seg : 0u].out;
    }
    const uint32_t c0 = (uint32_t)(j * PS_CHUNK);
    const uint32_t want = (uint32_t)(stream - c0 < PS_CHUNK ? stream - c0 : PS_CHUNK);
    const int tid = threadIdx.x;
    if (tid == 0) pl_geometry(pg.W, pg.H, pg.fmt, &geom);
    uint32_t sa = 0, l = 0, loff = 0, lend = 0;
    unsigned long long sb = 0;
    int bad = 0;
    for (uint32_t i = (uint32_t)tid; i < want; i += PS_THREADS) {
        const uint32_t p = c0 + i;
        uint32_t d = 0;
        if (p < have) {
            if (p < loff || p >= lend) {
                l = ps_link_of(links, nlinks, p);
                loff = links[l].off;
                lend = l + 1 < nlinks ? links[l + 1].off : have;
            }
            d = pi_resolve(sym[p], win + (size_t)l * PI_WINDOW, loff, &bad);
        }
        dst[i] = (uint8_t)d;
        sa += d;
        sb += (unsigned long long)(want - i) * d;
    }
    __syncthreads();                                                   // this chunk's bytes are written, the geometry is known
    int badf = 0;
    for (int q = 0; q < geom.npass; ++q) {                             // the filter bytes of every pass's rows that start in this chunk
        const long long rb1 = 1 + (long long)geom.p[q].rb, lo = geom.p[q].off, hi = lo + geom.p[q].rows * rb1;
        const long long a = lo > (long long)c0 ? lo : (long long)c0, b = hi < (long long)c0 + want ? hi : (long long)c0 + want;
        for (long long r = (a - lo + rb1 - 1) / rb1 + tid; lo + r * rb1 < b; r += PS_THREADS)
            if (dst[lo + r * rb1 - c0] > 4) badf = 1;
    }
    const uint32_t wa = ps_wave_sum(sa), wb = ps_wave_sum((uint32_t)(sb % PE_ADLER));
    if ((tid & 63) == 0) { red[0][tid >> 6] = wa; red[1][tid >> 6] = wb; }
    const int anybad = __syncthreads_or(bad), anyf = __syncthreads_or(badf);
    if (tid == 0) {
        uint32_t A = 1, B = want % PE_ADLER;
        for (int w = 0; w < PS_THREADS / 64; ++w) { A = (A + red[0][w]) % PE_ADLER; B = (B + red[1][w]) % PE_ADLER; }
        PSMeta m;
        m.a = A; m.b = B; m.pad_ = 0;
        m.status = (anybad ? (uint32_t)PI_DIST : 0u) | (anyf ? (uint32_t)PI_FILTER : 0u) | (j == 0 ? hd->status : 0u);
        reinterpret_cast<PSMeta*>(ws + pg.ws_off + lay.meta)[j] = m;
    }
}

// ---- kernel 7: one page's Adler-32 and status -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PS_WAVE) void psd_page_kernel(const uint8_t* ws, int32_t* status, PSBatch bt) {
    const int page = blockIdx.x;
    if (page >= bt.n || threadIdx.x != 0) return;
    const PSPage& pg = bt.p[page];
    const long long stream = ps_stream(pg);
    const PSLayout lay = ps_layout(stream, pg.nsegs);
    const PSMeta* meta = reinterpret_cast<const PSMeta*>(ws + pg.ws_off + lay.meta);
    uint32_t st = 0, A = 1, B = 0;                                     // A = A1 + A2 - 1, B = B1 + B2 + len2 (A1 - 1) mod 65521
    for (long long k = 0; k < lay.nchunks; ++k) {
        const PSMeta m = meta[k];
        const long long len = stream - k * PS_CHUNK < PS_CHUNK ? stream - k * PS_CHUNK : PS_CHUNK;
        st |= m.status;
        B = (uint32_t)((B + m.b % PE_ADLER + (unsigned long long)len * ((A + PE_ADLER - 1u) % PE_ADLER)) % PE_ADLER);
        A = (A + m.a % PE_ADLER + PE_ADLER - 1u) % PE_ADLER;
    }
    if ((B << 16 | A) != pg.adler) st |= PI_ADLER;
    status[page] = (int32_t)st;
}

// ---- kernel 8: the five filters undone, the B,G,R page written ----------------------------------------------------------------------------------
__device__ inline uint32_t ps_paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return (uint32_t)((pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c));
}

__global__ __launch_bounds__(PS_BAND) void psd_unfilter_kernel(const uint8_t* ws, PSBatch bt) {
    __shared__ uint32_t pub[2][PS_BAND];                               // the pixel every thread computed in the last two steps, channels packed
    const int page = blockIdx.x;
    if (page >= bt.n) return;
    const PSPage& pg = bt.p[page];
    const int W = pg.W, H = pg.H, nc = pg.nc, tid = threadIdx.x;
    const long long rb1 = 1 + (long long)W * nc;
    const uint8_t* src = ws + pg.ws_off;
    uint8_t* out = pg.out;
    for (int y0 = 0; y0 < H; y0 += PS_BAND) {
        const int y = y0 + tid;
        const bool live = y < H;
        const uint8_t* row = src + (long long)(live ? y : 0) * rb1;
        uint32_t type = live ? row[0] : 0u;
        if (type > 4u) type = 0u;                                      // the page is flagged (PI_FILTER)
        const int rows = H - y0 < PS_BAND ? H - y0 : PS_BAND;
        const long long steps = (long long)W + rows - 1;
        uint32_t a = 0, c = 0;                                         // the pixel to the left, the pixel above it
        for (long long s = 0; s < steps; ++s) {
            const long long x = s - tid;
            uint32_t cur = 0;
            if (live && x >= 0 && x < W) {
                uint32_t b = 0;                                        // the pixel above
                if (tid > 0) b = pub[(s - 1) & 1][tid - 1];
                else if (y > 0) {
                    const uint8_t* o = out + ((long long)(y - 1) * W + x) * 3;
                    b = nc == 3 ? ((uint32_t)o[2] | (uint32_t)o[1] << 8 | (uint32_t)o[0] << 16) : (uint32_t)o[0];
                }
                uint8_t* o = out + ((long long)y * W + x) * 3;
                for (int ch = 0; ch < nc; ++ch) {
                    const uint32_t raw = row[1 + x * nc + ch];
                    const uint32_t av = (a >> (8 * ch)) & 255u, bv = (b >> (8 * ch)) & 255u, cv = (c >> (8 * ch)) & 255u;
                    uint32_t v = raw;
                    if (type == 1u) v += av;
                    else if (type == 2u) v += bv;
                    else if (type == 3u) v += (av + bv) >> 1;
                    else if (type == 4u) v += ps_paeth((int)av, (int)bv, (int)cv);
                    v &= 255u;
                    cur |= v << (8 * ch);
                    if (nc == 3) o[2 - ch] = (uint8_t)v;               // R,G,B in the file -> B,G,R in the page
                    else { o[0] = (uint8_t)v; o[1] = (uint8_t)v; o[2] = (uint8_t)v; }
                }
                c = b;
                a = cur;
            }
            pub[s & 1][tid] = cur;
            __syncthreads();
        }
        __syncthreads();                                               // the band's last row is in the page before the next band reads it
    }
}

// ---- kernel 8a (layout pages): the five filters undone in place, one workgroup per page and pass ------------------------------------------------
// The schedule of psd_unfilter_kernel over filter units of bpp bytes: thread t of a band computes unit s - t of its row at step s.
// Every pass has a zero row above its first, so the passes do not wait for each other.
__global__ __launch_bounds__(PS_BAND) void pld_unfilter_kernel(uint8_t* ws, PSBatch bt) {
    __shared__ unsigned long long pub[2][PS_BAND];                     // the unit every thread computed in the last two steps, bytes packed
    __shared__ PLGeom geom;
    const int page = blockIdx.y, q = blockIdx.x, tid = threadIdx.x;
    if (page >= bt.n) return;
    const PSPage& pg = bt.p[page];
    if (tid == 0) pl_geometry(pg.W, pg.H, pg.fmt, &geom);
    __syncthreads();
    if (q >= geom.npass || geom.p[q].rows == 0) return;                // the whole workgroup leaves
    const PLPass ps = geom.p[q];
    const int bpp = geom.bpp, rows = ps.rows;
    const long long rb1 = 1 + (long long)ps.rb, units = ((long long)ps.rb + bpp - 1) / bpp;     // rb is a multiple of bpp when bpp > 1
    uint8_t* base = ws + pg.ws_off + ps.off;                           // [off, off + rows * rb1) lies inside the stream: pl_geometry
    for (int y0 = 0; y0 < rows; y0 += PS_BAND) {
        const int y = y0 + tid;
        const bool live = y < rows;
        uint8_t* row = base + (long long)(live ? y : 0) * rb1;
        uint32_t type = live ? row[0] : 0u;
        if (type > 4u) type = 0u;                                      // the page is flagged (PI_FILTER)
        const int band = rows - y0 < PS_BAND ? rows - y0 : PS_BAND;
        const long long steps = units + band - 1;
        unsigned long long a = 0, c = 0;                               // the unit to the left, the unit above it
        for (long long s = 0; s < steps; ++s) {
            const long long x = s - tid;
            unsigned long long cur = 0;
            if (live && x >= 0 && x < units) {
                unsigned long long b = 0;                              // the unit above
                if (tid > 0) b = pub[(s - 1) & 1][tid - 1];
                else if (y > 0)
                    for (int ch = 0; ch < bpp; ++ch) b |= (unsigned long long)row[1 - rb1 + x * bpp + ch] << (8 * ch);
                for (int ch = 0; ch < bpp; ++ch) {
                    uint8_t* at = row + 1 + x * bpp + ch;
                    const uint32_t v = pl_unfilter_byte(type, *at, (uint32_t)(a >> (8 * ch)) & 255u, (uint32_t)(b >> (8 * ch)) & 255u,
                                                        (uint32_t)(c >> (8 * ch)) & 255u);
                    *at = (uint8_t)v;
                    cur |= (unsigned long long)v << (8 * ch);
                }
                c = b;
                a = cur;
            }
            pub[s & 1][tid] = cur;
            __syncthreads();
        }
        __syncthreads();                                               // the band's last row is reconstructed before the next band reads it
    }
}

// ---- kernel 8b (layout pages): samples -> B,G,R, every pass gathered into the page -----------------------------------------------------------
// One thread per four consecutive pixels of the page (12 bytes, three aligned words when the page starts on a word), so the stores of a
// workgroup are contiguous whatever the interlace; the palette is read from LDS.
constexpr int PL_THREADS = 256, PL_MAX_GRID = 8192;
__global__ __launch_bounds__(PL_THREADS) void pld_expand_kernel(const uint8_t* blobs, const uint8_t* ws, PSBatch bt) {
    __shared__ uint8_t pal[768];
    __shared__ PLGeom geom;
    const int page = blockIdx.y, tid = threadIdx.x;
    if (page >= bt.n) return;
    const PSPage& pg = bt.p[page];
    const uint32_t fmt = pg.fmt;
    const int npal = pl_npal(fmt) <= 256 ? pl_npal(fmt) : 256;
    const uint8_t* src = blobs + pg.blob_off + pg.off_table + (size_t)pg.nidat * sizeof(PSIdat);
    for (int i = tid; i < 3 * npal; i += PL_THREADS) pal[i] = src[i];
    if (tid == 0) pl_geometry(pg.W, pg.H, fmt, &geom);
    __syncthreads();
    const int W = pg.W;
    const long long npix = (long long)W * pg.H, groups = (npix + 3) >> 2;
    const uint8_t* rec = ws + pg.ws_off;
    uint8_t* out = pg.out;
    const bool words = ((uintptr_t)out & 3) == 0;
    for (long long u = (long long)blockIdx.x * PL_THREADS + tid; u < groups; u += (long long)gridDim.x * PL_THREADS) {
        const long long i0 = u << 2;
        int y = (int)(i0 / W), x = (int)(i0 - (long long)y * W);
        const int n = npix - i0 < 4 ? (int)(npix - i0) : 4;
        uint32_t w[3] = {0u, 0u, 0u};
        for (int k = 0; k < n; ++k) {
            uint32_t b, g, r;
            pl_pixel(geom, fmt, rec, pal, y, x, &b, &g, &r);
            const uint32_t v[3] = {b, g, r};
            for (int ch = 0; ch < 3; ++ch) {
                const int at = 3 * k + ch;
                w[at >> 2] |= v[ch] << (8 * (at & 3));
            }
            if (++x == W) { x = 0; ++y; }
        }
        if (n == 4 && words) {
            uint32_t* o = reinterpret_cast<uint32_t*>(out + 3 * i0);
            o[0] = w[0]; o[1] = w[1]; o[2] = w[2];
        } else {
            for (int at = 0; at < 3 * n; ++at) out[3 * i0 + at] = (uint8_t)(w[at >> 2] >> (8 * (at & 3)));
        }
    }
}

// off >= 0: the callers (rtn_codec_blobs, and the walk behind it) have looked at the sign
const PSHdr* psd_blob(const void* host_blobs, int64_t off, uint32_t magic) {
    const PSHdr* hd = reinterpret_cast<const PSHdr*>(static_cast<const uint8_t*>(host_blobs) + off);
    if (hd->magic != magic || hd->blob_bytes < (int64_t)sizeof(PSHdr)) return nullptr;
    return ps_blob(hd, (size_t)hd->blob_bytes, magic);
}

uint32_t psd_segment_bytes() {
    rtn_env_sync();
    const int v = rtn_env_int("RTN_PNG_SEGMENT", (int)PS_SEGMENT_DEFAULT);
    return v < (int)PS_SEGMENT_MIN ? PS_SEGMENT_MIN : v > (int)PS_SEGMENT_MAX ? PS_SEGMENT_MAX : (uint32_t)v;
}

int psd_inspect(const char* name, bool layout, rtn_handle_t h, const void* file, size_t file_bytes, rtn_png_info_t* info, void* blob_out,
                size_t blob_capacity) {
    return rtn_codec_inspect(h, name, file, info, true, [&](char* why, size_t bytes) {
        return ps_inspect_any(static_cast<const uint8_t*>(file), file_bytes, psd_segment_bytes(), info, blob_out, blob_capacity, why, bytes, layout);
    });
}

size_t psd_workspace_bytes(uint32_t magic, int n, const void* host_blobs, const int64_t* offsets) {
    return rtn_codec_blob_bytes(n, host_blobs, offsets, [=](const void* blobs, int64_t off) { return psd_blob(blobs, off, magic); });
}

// rtn_png_stream_decode (magic PS_MAGIC) and rtn_png_layout_decode (PL_MAGIC): stages 1 - 7 are the same launches, the last stage is
// psd_unfilter_kernel for the one and pld_unfilter_kernel + pld_expand_kernel for the other.
int psd_decode(const char* name, uint32_t magic, rtn_handle_t h, int n, const void* host_blobs, const void* dev_blobs, const int64_t* offsets,
               uint8_t* const* pages, int32_t* status, void* workspace, size_t workspace_bytes) {
    const auto header_at = [=](const void* blobs, int64_t off) { return psd_blob(blobs, off, magic); };
    const int rc = rtn_decode_check(h, name, magic == PL_MAGIC ? "rtn_png_layout_inspect" : "rtn_png_stream_inspect", n, host_blobs, dev_blobs,
                                    offsets, pages, status, workspace, workspace_bytes, header_at, [](const PSHdr* hd) {
                                        return hd->ws_bytes != ps_layout(ps_want(hd), hd->nsegs).total ? "workspace size does not match its header" : nullptr;
                                    });
    if (rc != RTN_CODEC_GO) return rc;
    const uint8_t* db = static_cast<const uint8_t*>(dev_blobs);
    uint8_t* wsp = static_cast<uint8_t*>(workspace);
    struct { unsigned segs = 1, idat = 1, pass = 1; long long chunks = 1, groups = 1; } most;      // of the table being filled
    return rtn_codec_walk<PSBatch>(n,
        [&](PSBatch& bt, int k, int i, long long ws) {
            const PSHdr* hd = header_at(host_blobs, offsets[i]);
            if (k == 0) most = {};
            PSPage& p = bt.p[k];
            p.blob_off = offsets[i];
            p.ws_off = ws;
            p.out = pages[i];
            p.W = hd->W; p.H = hd->H; p.nc = hd->nc;
            p.nsegs = hd->nsegs; p.nidat = hd->nidat; p.S = hd->seg_bytes; p.in_bytes = hd->in_bytes; p.adler = hd->adler;
            p.off_table = hd->off_table; p.off_data = hd->off_data;
            p.stream = (uint32_t)ps_want(hd); p.fmt = ps_fmt(hd);
            const long long nchunks = ps_layout(ps_want(hd), hd->nsegs).nchunks, groups = ((long long)hd->W * hd->H + 3) / 4;
            most.segs = p.nsegs > most.segs ? p.nsegs : most.segs;
            most.idat = p.nidat > most.idat ? p.nidat : most.idat;
            most.chunks = nchunks > most.chunks ? nchunks : most.chunks;
            most.groups = groups > most.groups ? groups : most.groups;
            if (pl_interlace(p.fmt)) most.pass = 7;
            return (long long)hd->ws_bytes;
        },
        [&](const PSBatch& bt, int i0) {
            const dim3 per_seg(most.segs, bt.n);
            psd_find_kernel<<<per_seg, PS_WAVE, 0, h->stream>>>(db, wsp, bt);
            RTN_CHECK_LAUNCH(h, "psd_find_kernel");
            psd_count_kernel<<<per_seg, PS_WAVE, 0, h->stream>>>(db, wsp, bt);
            RTN_CHECK_LAUNCH(h, "psd_count_kernel");
            psd_crc_kernel<<<dim3(rtn_min_grid(most.idat, PS_MAX_GRID), bt.n), PS_WAVE, 0, h->stream>>>(db, wsp, bt);
            RTN_CHECK_LAUNCH(h, "psd_crc_kernel");
            psd_chain_kernel<<<bt.n, PS_WAVE, 0, h->stream>>>(wsp, bt);
            RTN_CHECK_LAUNCH(h, "psd_chain_kernel");
            psd_decode_kernel<<<per_seg, PS_WAVE, 0, h->stream>>>(db, wsp, bt);
            RTN_CHECK_LAUNCH(h, "psd_decode_kernel");
            psd_window_kernel<<<bt.n, PS_BAND, 0, h->stream>>>(wsp, bt);
            RTN_CHECK_LAUNCH(h, "psd_window_kernel");
            psd_resolve_kernel<<<dim3((unsigned)most.chunks, bt.n), PS_THREADS, 0, h->stream>>>(wsp, bt);
            RTN_CHECK_LAUNCH(h, "psd_resolve_kernel");
            psd_page_kernel<<<bt.n, PS_WAVE, 0, h->stream>>>(wsp, status + i0, bt);
            RTN_CHECK_LAUNCH(h, "psd_page_kernel");
            if (magic == PS_MAGIC) {
                psd_unfilter_kernel<<<bt.n, PS_BAND, 0, h->stream>>>(wsp, bt);
                RTN_CHECK_LAUNCH(h, "psd_unfilter_kernel");
            } else {
                pld_unfilter_kernel<<<dim3(most.pass, bt.n), PS_BAND, 0, h->stream>>>(wsp, bt);
                RTN_CHECK_LAUNCH(h, "pld_unfilter_kernel");
                const long long blocks = (most.groups + PL_THREADS - 1) / PL_THREADS;
                pld_expand_kernel<<<dim3(rtn_min_grid(blocks, PL_MAX_GRID), bt.n), PL_THREADS, 0, h->stream>>>(db, wsp, bt);
                RTN_CHECK_LAUNCH(h, "pld_expand_kernel");
            }
            return RTN_OK;
        });
}

}  // namespace

// rtn_png_stream_*, rtn_png_layout_*: see include/rtn.h
extern "C" size_t rtn_png_stream_blob_bound(size_t file_bytes) { return RTN_PNG_BLOB_BOUND(file_bytes); }
// the table, the palette and the stream are disjoint parts of the file, so the bound of the stream blob holds
extern "C" size_t rtn_png_layout_blob_bound(size_t file_bytes) { return RTN_PNG_BLOB_BOUND(file_bytes); }

extern "C" int rtn_png_stream_inspect(rtn_handle_t h, const void* file, size_t file_bytes, rtn_png_info_t* info, void* blob_out,
                                      size_t blob_capacity) {
    return psd_inspect("rtn_png_stream_inspect", false, h, file, file_bytes, info, blob_out, blob_capacity);
}

extern "C" int rtn_png_layout_inspect(rtn_handle_t h, const void* file, size_t file_bytes, rtn_png_info_t* info, void* blob_out,
                                      size_t blob_capacity) {
    return psd_inspect("rtn_png_layout_inspect", true, h, file, file_bytes, info, blob_out, blob_capacity);
}

extern "C" int rtn_png_stream_inflate_host(const void* blob, size_t segment_bytes, void* out, size_t want_bytes, int32_t* status) {
    if (!blob || !out || !status) { rtn_set_host_error("rtn_png_stream_inflate_host: NULL argument"); return RTN_EINVAL; }
    const PSHdr* hd = static_cast<const PSHdr*>(blob);
    if ((hd->magic != PS_MAGIC && hd->magic != PL_MAGIC) || hd->blob_bytes < (int64_t)sizeof(PSHdr)) {
        rtn_set_host_error("rtn_png_stream_inflate_host: not an rtn_png_stream_inspect or rtn_png_layout_inspect blob");
        return RTN_EINVAL;
    }
    if (segment_bytes > PS_SEGMENT_MAX) { rtn_set_host_error("rtn_png_stream_inflate_host: segment_bytes outside 256 .. 2^24"); return RTN_EINVAL; }
    const char* why = "";
    const int rc = ps_inflate_host(blob, (size_t)hd->blob_bytes, (uint32_t)segment_bytes, static_cast<uint8_t*>(out), want_bytes, status, &why);
    if (rc != RTN_OK) rtn_set_host_error(why);
    return rc;
}

extern "C" int rtn_png_layout_pixels_host(const void* blob, const void* filtered_stream, size_t bytes, void* out_bgr, int32_t* status) {
    if (!blob || !filtered_stream || !out_bgr || !status) { rtn_set_host_error("rtn_png_layout_pixels_host: NULL argument"); return RTN_EINVAL; }
    const PSHdr* hd = static_cast<const PSHdr*>(blob);
    if (hd->magic != PL_MAGIC || hd->blob_bytes < (int64_t)sizeof(PSHdr)) {
        rtn_set_host_error("rtn_png_layout_pixels_host: not an rtn_png_layout_inspect blob");
        return RTN_EINVAL;
    }
    const char* why = "";
    const int rc = pl_pixels_host(blob, (size_t)hd->blob_bytes, static_cast<const uint8_t*>(filtered_stream), bytes, static_cast<uint8_t*>(out_bgr),
                                  status, &why);
    if (rc != RTN_OK) rtn_set_host_error(why);
    return rc;
}

extern "C" size_t rtn_png_stream_decode_workspace_bytes(int n, const void* host_blobs, const int64_t* offsets) {
    return psd_workspace_bytes(PS_MAGIC, n, host_blobs, offsets);
}

extern "C" size_t rtn_png_layout_decode_workspace_bytes(int n, const void* host_blobs, const int64_t* offsets) {
    return psd_workspace_bytes(PL_MAGIC, n, host_blobs, offsets);
}

extern "C" int rtn_png_stream_decode(rtn_handle_t h, int n, const void* host_blobs, const void* dev_blobs, const int64_t* offsets,
                                     uint8_t* const* pages, int32_t* status, void* workspace, size_t workspace_bytes) {
    return psd_decode("rtn_png_stream_decode", PS_MAGIC, h, n, host_blobs, dev_blobs, offsets, pages, status, workspace, workspace_bytes);
}

extern "C" int rtn_png_layout_decode(rtn_handle_t h, int n, const void* host_blobs, const void* dev_blobs, const int64_t* offsets,
                                     uint8_t* const* pages, int32_t* status, void* workspace, size_t workspace_bytes) {
    return psd_decode("rtn_png_layout_decode", PL_MAGIC, h, n, host_blobs, dev_blobs, offsets, pages, status, workspace, workspace_bytes);
}
