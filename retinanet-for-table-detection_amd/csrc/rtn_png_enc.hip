// rtn_png_enc.hip — PNG pages encoded on the device: 8-bit R,G,B (colour type 2) or gray (colour type 0), non-interlaced, row
// filters None / Sub / Up, and a zlib stream cut into independently deflated chunks of RTN_PNG_CHUNK raw bytes, one IDAT each
// (DESIGN §3.4d).  Every chunk starts a fresh deflate block, matches nothing before its first byte and ends byte-aligned on an
// empty stored block, so IDAT k inflated alone gives raw bytes [k CHUNK, (k + 1) CHUNK): the chunks compress in parallel now and
// can be inflated in parallel later.
//
// Four kernels per batch of up to RTN_CODEC_BATCH pages; no workgroup waits on another:
//   1. penc_filter_kernel: one workgroup per row (rows past PE_MAX_GRID are looped over).  Counts, for None, Sub and Up, the
//      bytes of the filtered row that differ from the byte before them, keeps the filter with the fewest (ties: the lower type) and writes type byte + filtered row into the
//      page's filtered stream.
//   2. penc_deflate_kernel: one workgroup per chunk, the chunk in LDS.  Sub-block by sub-block of PE_THREADS positions: every
//      thread finds the longest match of its position among four candidates (distance 1, distance of one pixel, the earliest
//      position of the same sub-block with the same 3-byte hash, the latest position of earlier sub-blocks with that hash: all
//      independent of thread order), then wave 0 walks the greedy parse through the sub-block with the step table in registers.
//      Then: histograms, two length-limited Huffman codes and the code-length code, the dynamic block header, the tokens packed
//      at their prefix-summed bit offsets into the chunk's own workspace slot, the sync flush.  A chunk whose dynamic block
//      would be longer than its stored form is written as one stored block.  Last: the slot's CRC-32 state (slices per thread,
//      joined by multiplying with x^(8 n) mod P) and the chunk's Adler-32 pair.
//   3. penc_scan_kernel: one workgroup per page: scans the IDAT lengths into file offsets, joins the Adler pairs, writes the
//      signature, IHDR, IEND and the file length.
//   4. penc_copy_kernel: one workgroup per chunk: length, "IDAT", (zlib header,) the slot's bytes, (final block, Adler-32,) CRC.
//
// Size bound (pe_bound): a chunk of r raw bytes is never longer than its stored form, 5 (stored-block header) + r + 5 (sync
// flush), and its IDAT adds 12 bytes of framing; the file adds the signature (8), IHDR (25), IEND (12), the zlib header (2), the
// final empty stored block (5) and the Adler-32 (4).  So a file is at most 56 + stream + 22 * chunks bytes, and the host path
// has nothing to catch.
#include "rtn_codec_launch.h"
#include "rtn_png_crc.h"

namespace {

constexpr int PE_CHUNK = RTN_PNG_CHUNK;        // raw bytes per deflate chunk; <= 32768, so every match distance is legal
constexpr int PE_THREADS = 256;                // workgroup of kernels 1, 2, 4; positions per sub-block of the matcher
constexpr int PE_SCAN_THREADS = 1024;          // workgroup of kernel 3: one page
constexpr int PE_SLOT = PE_CHUNK + 256;        // bytes of one chunk's workspace slot (>= stored form, a multiple of 256)
constexpr int PE_HASH_BITS = 12;
constexpr int PE_HASH = 1 << PE_HASH_BITS;
constexpr int PE_MIN_MATCH = 3, PE_MAX_MATCH = 258;
constexpr int PE_MAX_GRID = 1 << 20;           // workgroups along x of the filter launch: rows past it are looped over
constexpr int PE_FAR = 4096;                   // a 3-byte match further back than this costs more than three literals
static_assert(PE_CHUNK <= 32768 && PE_CHUNK % PE_THREADS == 0 && PE_CHUNK % 64 == 0, "chunk size");

struct PEPage {
    const uint8_t* src;                        // (H, W, 3) B,G,R or (H, W) gray
    uint8_t* out;                              // the page's output slot (>= pe_bound bytes)
    long long ws_off;                          // start of the page's workspace
    long long off_meta, off_file, off_slots;   // workspace sections, relative to ws_off (the filtered stream is at 0)
    long long stream;                          // bytes of the filtered stream: H * (1 + W * nc)
    int W, H, nc, nchunks;
};

struct PEBatch {
    uint8_t* ws;
    long long* out_bytes;
    int32_t* status;
    int n, maxrows, maxchunks, pad_;
    PEPage p[RTN_CODEC_BATCH];
};

struct PEMeta { uint32_t len, crc, a, b; };    // per chunk: slot bytes used, CRC state over "IDAT" (+ zlib header) + slot, Adler pair

// ---- geometry, bound, workspace ---------------------------------------------------------------------------------------------------
inline bool pe_valid(int W, int H, int nc) {
    return W >= 1 && H >= 1 && (nc == 1 || nc == 3) && (long long)H * (1 + (long long)W * nc) < (1LL << 31);
}
inline long long pe_stream(int W, int H, int nc) { return (long long)H * (1 + (long long)W * nc); }
inline long long pe_chunks(long long stream) { return (stream + PE_CHUNK - 1) / PE_CHUNK; }

// the derivation is in the file comment
inline long long pe_bound(int W, int H, int nc) {
    const long long s = pe_stream(W, H, nc);
    return 8 + 25 + 12 + s + pe_chunks(s) * (5 + 5 + 12) + 2 + 5 + 4;
}

struct PELayout { long long meta, file, slots, total; };
inline PELayout pe_layout(int W, int H, int nc) {
    const long long s = pe_stream(W, H, nc), nk = pe_chunks(s);
    PELayout L;
    L.meta = rtn_align256(s + 8);                                      // filtered stream, padded for word reads
    L.file = L.meta + rtn_align256(nk * (long long)sizeof(PEMeta));    // PEMeta per chunk
    L.slots = L.file + rtn_align256((nk + 1) * 8 + 8);                 // file offset of every IDAT (int64), then the page's Adler-32
    L.total = L.slots + nk * PE_SLOT;
    return L;
}

// ---- deflate symbol tables ----------------------------------------------------------------------------------------------------------
__device__ inline void pe_len_code(int len, int* code, int* nb, int* extra) {       // len 3..258 -> 0..28 (symbol 257 + code)
    const int l = len - 3;
    if (l < 8) { *code = l; *nb = 0; *extra = 0; return; }
    if (len == 258) { *code = 28; *nb = 0; *extra = 0; return; }
    const int b = 31 - __builtin_clz((unsigned)l) - 2;
    *code = 4 * b + 4 + ((l >> b) & 3); *nb = b; *extra = l & ((1 << b) - 1);
}
__device__ inline void pe_dist_code(int dist, int* code, int* nb, int* extra) {     // dist 1..32768 -> 0..29
    const int d = dist - 1;
    if (d < 4) { *code = d; *nb = 0; *extra = 0; return; }
    const int b = 31 - __builtin_clz((unsigned)d) - 1;
    *code = 2 * b + 2 + ((d >> b) & 1); *nb = b; *extra = d & ((1 << b) - 1);
}

// ---- LDS of the deflate kernel ------------------------------------------------------------------------------------------------------
constexpr int PE_NLL = 288, PE_ND = 32, PE_NCL = 19;
struct PELds {
    uint32_t data[PE_CHUNK / 4 + 4];           // the chunk, zero padded
    uint8_t tok[PE_CHUNK];                     // at a match's first position: length - 3, then distance - 1 (16 bits, little endian)
    uint32_t head[PE_HASH];                    // 1 + latest position of earlier sub-blocks with this hash; 0 = none
    uint32_t lmin[PE_HASH];                    // earliest position of this sub-block with this hash; ~0 = none
    unsigned long long start[PE_CHUNK / 64];   // bit p: a token starts at position p
    unsigned long long match[PE_CHUNK / 64];   // bit p: that token is a match
    uint32_t minfo[PE_THREADS];                // per position of the sub-block: match length (0 = none) | distance << 16
    uint32_t freq_ll[PE_NLL], freq_d[PE_ND], freq_cl[32];
    uint16_t code_ll[PE_NLL], code_d[PE_ND], code_cl[32];
    uint8_t len_ll[PE_NLL], len_d[PE_ND], len_cl[32];
    uint16_t sorted[PE_NLL];                   // Huffman scratch: symbols by (frequency, symbol)
    uint32_t nodef[2 * PE_NLL];
    uint16_t parent[2 * PE_NLL];
    uint8_t depth[PE_NLL];
    uint16_t clseq[PE_NLL + PE_ND];            // code-length symbols of the header: symbol | extra << 8
    uint32_t scan[PE_THREADS];
    uint32_t crctab[256];
    int cur, hm, ncl, hlit, hdist, hclen;
    uint32_t red[8];
};

__device__ inline uint32_t pe_load4(const uint32_t* data, int p) {                 // 4 bytes at byte position p (any alignment)
    const uint32_t a = data[p >> 2], b = data[(p >> 2) + 1];
    return (uint32_t)((((unsigned long long)b << 32) | a) >> (8 * (p & 3)));
}
__device__ inline int pe_byte(const uint32_t* data, int p) { return (int)((data[p >> 2] >> (8 * (p & 3))) & 255u); }

__device__ inline int pe_match_len(const uint32_t* data, int p, int c, int maxlen) {
    int l = 0;
    while (l < maxlen) {
        const uint32_t x = pe_load4(data, p + l) ^ pe_load4(data, c + l);
        if (x) { l += __builtin_ctz(x) >> 3; break; }
        l += 4;
    }
    return l < maxlen ? l : maxlen;
}

__device__ inline uint32_t pe_bitrev(uint32_t code, int len) { return __brev(code) >> (32 - len); }

// Code lengths (<= maxbits) and canonical codes, bit-reversed for LSB-first packing, of the n symbols with frequencies freq[]:
// Huffman's algorithm on the symbols sorted by (frequency, symbol), lengths over maxbits folded back by moving codes between
// lengths until Kraft's sum is exactly 1.  At least two symbols get a code (inflate wants complete codes).  All threads call it.
__device__ void pe_huffman(PELds& S, uint32_t* freq, int n, int maxbits, uint8_t* lens, uint16_t* codes) {
    const int tid = threadIdx.x;
    if (tid == 0) {
        int m = 0;
        for (int s = 0; s < n; ++s) m += freq[s] != 0;
        for (int s = 0; m < 2 && s < n; ++s)
            if (!freq[s]) { freq[s] = 1; ++m; }
        S.hm = m;
    }
    __syncthreads();
    const int m = S.hm;
    for (int s = tid; s < n; s += PE_THREADS) {
        const uint32_t f = freq[s];
        lens[s] = 0;
        codes[s] = 0;
        if (!f) continue;
        int r = 0;
        for (int j = 0; j < n; ++j) {
            const uint32_t fj = freq[j];
            r += (fj != 0 && (fj < f || (fj == f && j < s))) ? 1 : 0;
        }
        S.sorted[r] = (uint16_t)s;
        S.nodef[r] = f;
    }
    __syncthreads();
    if (tid == 0) {                            // two queues: leaves in order, internal nodes in order of creation
        int i = 0, j = m, next = m;
        for (int k = 0; k < m - 1; ++k) {
            int pick[2];
            for (int q = 0; q < 2; ++q) pick[q] = (i < m && (j >= next || S.nodef[i] <= S.nodef[j])) ? i++ : j++;
            S.nodef[next] = S.nodef[pick[0]] + S.nodef[pick[1]];
            S.parent[pick[0]] = S.parent[pick[1]] = (uint16_t)next;
            ++next;
        }
    }
    __syncthreads();
    for (int r = tid; r < m; r += PE_THREADS) {
        int d = 0;
        for (int x = r; x != 2 * m - 2; x = S.parent[x]) ++d;
        S.depth[r] = (uint8_t)(d < maxbits ? d : maxbits);
    }
    __syncthreads();
    if (tid == 0) {
        int count[16];
        for (int l = 0; l < 16; ++l) count[l] = 0;
        for (int r = 0; r < m; ++r) count[S.depth[r]]++;
        uint32_t total = 0;
        for (int l = maxbits; l > 0; --l) total += (uint32_t)count[l] << (maxbits - l);
        while (total != (1u << maxbits)) {
            count[maxbits]--;
            for (int l = maxbits - 1; l > 0; --l)
                if (count[l]) { count[l]--; count[l + 1] += 2; break; }
            total--;
        }
        int r = m;                             // the most frequent symbols take the shortest codes
        for (int l = 1; l <= maxbits; ++l)
            for (int c = count[l]; c > 0; --c) lens[S.sorted[--r]] = (uint8_t)l;
        uint32_t nextc[17];
        uint32_t code = 0;
        count[0] = 0;
        for (int l = 1; l <= maxbits; ++l) { code = (code + (uint32_t)count[l - 1]) << 1; nextc[l] = code; }
        for (int s = 0; s < n; ++s)
            if (lens[s]) codes[s] = (uint16_t)pe_bitrev(nextc[lens[s]]++, lens[s]);
    }
    __syncthreads();
}

// LSB-first bit writer over the chunk's slot: words only this thread owns are stored, the (at most two) words it shares with
// its neighbours are ORed atomically (order-independent); the slot is zeroed first.
struct PEWriter {
    uint32_t* w;
    unsigned long long acc;
    int fill;
    bool first;
    __device__ inline void operator()(uint32_t bits, int len) {
        acc |= (unsigned long long)bits << fill;
        fill += len;
        if (fill >= 32) {
            if (first) atomicOr(w, (uint32_t)acc);
            else *w = (uint32_t)acc;
            ++w; acc >>= 32; fill -= 32; first = false;
        }
    }
    __device__ inline void finish() {
        if (fill > 0) atomicOr(w, (uint32_t)acc);
    }
};
struct PECounter {
    int bits;
    __device__ inline void operator()(uint32_t, int len) { bits += len; }
};

// the dynamic block's header: BFINAL 0, BTYPE 2, HLIT, HDIST, HCLEN, the code-length code, the run-length coded lengths
template <class Emit>
__device__ inline void pe_block_header(const PELds& S, Emit& emit) {
    constexpr unsigned char order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    emit(4u, 3);
    emit((uint32_t)(S.hlit - 257), 5);
    emit((uint32_t)(S.hdist - 1), 5);
    emit((uint32_t)(S.hclen - 4), 4);
    for (int i = 0; i < S.hclen; ++i) emit(S.len_cl[order[i]], 3);
    for (int i = 0; i < S.ncl; ++i) {
        const int sym = S.clseq[i] & 255, extra = S.clseq[i] >> 8;
        emit(S.code_cl[sym], S.len_cl[sym]);
        if (sym == 16) emit((uint32_t)extra, 2);
        else if (sym == 17) emit((uint32_t)extra, 3);
        else if (sym == 18) emit((uint32_t)extra, 7);
    }
}

// the tokens that start in positions [p0, p1)
template <class Emit>
__device__ inline void pe_tokens(const PELds& S, int p0, int p1, Emit& emit) {
    for (int wq = p0 >> 6; wq < (p1 + 63) >> 6; ++wq) {
        unsigned long long m = S.start[wq];
        const unsigned long long mm = S.match[wq];
        while (m) {
            const int b = __builtin_ctzll(m);
            m &= m - 1;
            const int p = wq * 64 + b;
            if (p < p0 || p >= p1) continue;
            if ((mm >> b) & 1ull) {
                const int len = S.tok[p] + 3, dist = (S.tok[p + 1] | (S.tok[p + 2] << 8)) + 1;
                int c, nb, ex;
                pe_len_code(len, &c, &nb, &ex);
                emit((uint32_t)S.code_ll[257 + c] | ((uint32_t)ex << S.len_ll[257 + c]), S.len_ll[257 + c] + nb);
                pe_dist_code(dist, &c, &nb, &ex);
                emit((uint32_t)S.code_d[c] | ((uint32_t)ex << S.len_d[c]), S.len_d[c] + nb);
            } else {
                const int v = pe_byte(S.data, p);
                emit(S.code_ll[v], S.len_ll[v]);
            }
        }
    }
}

// sum over the workgroup (PE_THREADS); every thread gets the total
__device__ inline uint32_t pe_wg_sum(PELds& S, uint32_t v, bool is_xor) {
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t a = (uint32_t)__shfl_xor((int)v, o);
        v = is_xor ? v ^ a : v + a;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) S.red[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t t = 0;
    for (int w = 0; w < PE_THREADS / 64; ++w) t = is_xor ? t ^ S.red[w] : t + S.red[w];
    return t;
}

// ---- kernel 1: row filters ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PE_THREADS) void penc_filter_kernel(PEBatch bt) {
    __shared__ int cost[3][PE_THREADS / 64];
    const int page = blockIdx.y;
    if (page >= bt.n) return;
    const PEPage& pg = bt.p[page];
    const int nc = pg.nc, rb = pg.W * nc;
    for (int y = blockIdx.x; y < pg.H; y += gridDim.x) {                // the grid is capped at PE_MAX_GRID rows
        const uint8_t* row = pg.src + (long long)y * rb;
        // byte i of the row in file order (R,G,B) and its None / Sub / Up residuals
        auto val = [&](const uint8_t* r, int i) -> int {
            if (nc == 1) return r[i];
            const int px = i / 3, c = i - px * 3;
            return r[px * 3 + 2 - c];
        };
        auto filt = [&](int i, int f[3]) {
            const int v = val(row, i);
            f[0] = v;
            f[1] = (v - (i >= nc ? val(row, i - nc) : 0)) & 255;
            f[2] = (v - (y > 0 ? val(row - rb, i) : 0)) & 255;
        };
        int c3[3] = {0, 0, 0};
        for (int i = 1 + threadIdx.x; i < rb; i += PE_THREADS) {
            int a[3], b[3];
            filt(i, a);
            filt(i - 1, b);
            for (int t = 0; t < 3; ++t) c3[t] += a[t] != b[t];
        }
        for (int t = 0; t < 3; ++t) {
            int s = c3[t];
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
            if ((threadIdx.x & 63) == 0) cost[t][threadIdx.x >> 6] = s;
        }
        __syncthreads();
        int best = 0, bestc = 0;
        for (int t = 0; t < 3; ++t) {
            int s = 0;
            for (int w = 0; w < PE_THREADS / 64; ++w) s += cost[t][w];
            if (t == 0 || s < bestc) { best = t; bestc = s; }
        }
        uint8_t* dst = bt.ws + pg.ws_off + (long long)y * (rb + 1);
        if (threadIdx.x == 0) dst[0] = (uint8_t)best;
        for (int i = threadIdx.x; i < rb; i += PE_THREADS) {
            int f[3];
            filt(i, f);
            dst[1 + i] = (uint8_t)f[best];
        }
        __syncthreads();                                                // cost[] is reused by the next row
    }
}

// ---- kernel 2: one chunk -> its slot ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PE_THREADS) void penc_deflate_kernel(PEBatch bt) {
    extern __shared__ __align__(16) uint8_t pe_lds_raw[];
    PELds& S = *reinterpret_cast<PELds*>(pe_lds_raw);
    const int page = blockIdx.y;
    if (page >= bt.n) return;
    const PEPage& pg = bt.p[page];
    const int k = blockIdx.x;
    if (k >= pg.nchunks) return;
    const int tid = threadIdx.x, lane = tid & 63;
    uint8_t* base = bt.ws + pg.ws_off;
    const long long c0 = (long long)k * PE_CHUNK;
    const int n = (int)(pg.stream - c0 < PE_CHUNK ? pg.stream - c0 : PE_CHUNK);        // 1..PE_CHUNK raw bytes
    uint8_t* slot = base + pg.off_slots + (long long)k * PE_SLOT;
    uint32_t* slotw = reinterpret_cast<uint32_t*>(slot);

    // load the chunk (its start is a multiple of PE_CHUNK past a 256-byte aligned base: word loads), clear the tables
    {
        const uint32_t* srcw = reinterpret_cast<const uint32_t*>(base + c0);
        const int nw = (n + 3) >> 2;
        for (int i = tid; i < PE_CHUNK / 4 + 4; i += PE_THREADS) {
            uint32_t v = i < nw ? srcw[i] : 0u;                                         // the stream is padded by 8 readable bytes
            if (i == nw - 1 && (n & 3)) v &= (1u << (8 * (n & 3))) - 1u;
            S.data[i] = v;
        }
        for (int i = tid; i < PE_HASH; i += PE_THREADS) { S.head[i] = 0u; S.lmin[i] = 0xffffffffu; }
        for (int i = tid; i < PE_CHUNK / 64; i += PE_THREADS) { S.start[i] = 0ull; S.match[i] = 0ull; }
        for (int i = tid; i < PE_NLL; i += PE_THREADS) S.freq_ll[i] = 0u;
        if (tid < 32) { S.freq_d[tid] = 0u; S.freq_cl[tid] = 0u; }
        uint32_t c = (uint32_t)tid;
        for (int j = 0; j < 8; ++j) c = (c & 1u) ? (c >> 1) ^ PE_POLY : c >> 1;
        S.crctab[tid] = c;
        if (tid == 0) S.cur = 0;
    }
    __syncthreads();

    // ---- matches and the greedy parse, sub-block by sub-block
    for (int sb = 0; sb < n; sb += PE_THREADS) {
        const int p = sb + tid;
        const bool canhash = p + PE_MIN_MATCH <= n;
        uint32_t hsh = 0;
        if (canhash) {
            hsh = ((pe_load4(S.data, p) & 0xffffffu) * 0x9E3779B1u) >> (32 - PE_HASH_BITS);
            atomicMin(&S.lmin[hsh], (uint32_t)p);
        }
        __syncthreads();
        const int cur0 = S.cur;
        uint32_t info = 0;
        if (canhash && p >= cur0) {                                    // positions a chosen match already covers need none
            const int maxlen = n - p < PE_MAX_MATCH ? n - p : PE_MAX_MATCH;
            int blen = 0, bdist = 0;
            auto consider = [&](int c) {
                if (c < 0 || c >= p) return;
                const int l = pe_match_len(S.data, p, c, maxlen), d = p - c;
                if (l > blen || (l == blen && d < bdist)) { blen = l; bdist = d; }
            };
            consider(p - 1);
            if (pg.nc == 3) consider(p - 3);
            const uint32_t e = S.lmin[hsh];
            if (e < (uint32_t)p) consider((int)e);
            consider((int)S.head[hsh] - 1);
            if (blen >= PE_MIN_MATCH && !(blen == PE_MIN_MATCH && bdist > PE_FAR)) info = (uint32_t)blen | ((uint32_t)bdist << 16);
        }
        S.minfo[tid] = info;
        __syncthreads();
        if (canhash) {
            S.lmin[hsh] = 0xffffffffu;
            atomicMax(&S.head[hsh], (uint32_t)p + 1u);
        }
        if (tid < 64) {                                                // wave 0: the parse, one window of 64 positions at a time
            int cur = __builtin_amdgcn_readfirstlane(cur0);
            for (int w = 0; w < PE_THREADS / 64; ++w) {
                const int wbase = sb + w * 64;
                const uint32_t mi = S.minfo[w * 64 + lane];
                const int len = (int)(mi & 0xffffu);
                const int step = len >= PE_MIN_MATCH ? len : 1;
                unsigned long long mask = 0ull;
                while (cur < wbase + 64 && cur < n) {
                    const int at = cur - wbase;                        // 0..63: cur never falls behind the window
                    mask |= 1ull << at;
                    cur += __builtin_amdgcn_readlane(step, at);
                }
                const bool mine = (mask >> lane) & 1ull;
                const bool ism = mine && len >= PE_MIN_MATCH;
                const unsigned long long mm = __ballot(ism);
                if (lane == 0) { S.start[wbase >> 6] = mask; S.match[wbase >> 6] = mm; }
                const int q = wbase + lane;
                if (ism) {
                    const int dist = (int)(mi >> 16);
                    S.tok[q] = (uint8_t)(len - 3);
                    S.tok[q + 1] = (uint8_t)((dist - 1) & 255);
                    S.tok[q + 2] = (uint8_t)((dist - 1) >> 8);
                    int c, nb, ex;
                    pe_len_code(len, &c, &nb, &ex);
                    atomicAdd(&S.freq_ll[257 + c], 1u);
                    pe_dist_code(dist, &c, &nb, &ex);
                    atomicAdd(&S.freq_d[c], 1u);
                } else if (mine) {
                    atomicAdd(&S.freq_ll[pe_byte(S.data, q)], 1u);
                }
            }
            if (lane == 0) S.cur = cur;
        }
        __syncthreads();
    }
    if (tid == 0) S.freq_ll[256] = 1u;
    __syncthreads();

    // ---- the three codes
    pe_huffman(S, S.freq_ll, 286, 15, S.len_ll, S.code_ll);
    pe_huffman(S, S.freq_d, 30, 15, S.len_d, S.code_d);
    if (tid == 0) {                            // run-length code the two length tables as one sequence
        int hlit = 286, hdist = 30;
        while (hlit > 257 && S.len_ll[hlit - 1] == 0) --hlit;
        while (hdist > 1 && S.len_d[hdist - 1] == 0) --hdist;
        const int total = hlit + hdist;
        auto at = [&](int i) -> int { return i < hlit ? S.len_ll[i] : S.len_d[i - hlit]; };
        int ncl = 0;
        auto push = [&](int sym, int extra) { S.clseq[ncl++] = (uint16_t)(sym | (extra << 8)); S.freq_cl[sym]++; };
        for (int i = 0; i < total;) {
            const int v = at(i);
            int run = 1;
            while (i + run < total && at(i + run) == v) ++run;
            i += run;
            if (v == 0) {
                while (run >= 3) {
                    const int r = run >= 11 ? (run < 138 ? run : 138) : run;
                    if (run >= 11) push(18, r - 11);
                    else push(17, r - 3);
                    run -= r;
                }
            } else {
                push(v, 0);
                --run;
                while (run >= 3) {
                    const int r = run < 6 ? run : 6;
                    push(16, r - 3);
                    run -= r;
                }
            }
            while (run-- > 0) push(v, 0);
        }
        S.ncl = ncl; S.hlit = hlit; S.hdist = hdist;
    }
    __syncthreads();
    pe_huffman(S, S.freq_cl, PE_NCL, 7, S.len_cl, S.code_cl);
    if (tid == 0) {
        constexpr unsigned char order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        int hclen = 19;
        while (hclen > 4 && S.len_cl[order[hclen - 1]] == 0) --hclen;
        S.hclen = hclen;
    }
    __syncthreads();

    // ---- bit offsets: thread t packs the tokens that start in its PE_CHUNK / PE_THREADS positions; thread 0 the header before
    // them, the last thread the end-of-block code and the sync flush's three header bits after them
    constexpr int PER = PE_CHUNK / PE_THREADS;
    const int p0 = tid * PER, p1 = p0 + PER;
    PECounter cnt{0};
    if (tid == 0) pe_block_header(S, cnt);
    pe_tokens(S, p0, p1, cnt);
    if (tid == PE_THREADS - 1) cnt.bits += S.len_ll[256] + 3;
    uint32_t incl = (uint32_t)cnt.bits;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t a = (uint32_t)__shfl_up((int)incl, o);
        if (lane >= o) incl += a;
    }
    if (lane == 63) S.scan[tid >> 6] = incl;
    __syncthreads();
    uint32_t pos = incl - (uint32_t)cnt.bits, total_bits = 0;
    for (int w = 0; w < PE_THREADS / 64; ++w) {
        if (w < (tid >> 6)) pos += S.scan[w];
        total_bits += S.scan[w];
    }
    const uint32_t body = (total_bits + 7) >> 3;                       // the dynamic block and the flush's header bits, padded
    const bool stored = body + 4 > (uint32_t)n + 10u;
    const uint32_t clen = stored ? (uint32_t)n + 10u : body + 4;
    if (!stored) {
        const uint32_t nw = (clen + 3) >> 2;
        for (uint32_t i = tid; i < nw; i += PE_THREADS) slotw[i] = 0u;
        __threadfence();
        __syncthreads();
        PEWriter wr;
        wr.w = slotw + (pos >> 5);
        wr.acc = 0ull;
        wr.fill = (int)(pos & 31u);
        wr.first = true;
        if (tid == 0) pe_block_header(S, wr);
        pe_tokens(S, p0, p1, wr);
        if (tid == PE_THREADS - 1) {
            wr(S.code_ll[256], S.len_ll[256]);
            wr(0u, 3);
        }
        wr.finish();
        if (tid == 0) {                                                // LEN 0000, NLEN ffff of the empty stored block
            const uint32_t b2 = body + 2, b3 = body + 3;
            atomicOr(slotw + (b2 >> 2), 0xffu << (8 * (b2 & 3)));
            atomicOr(slotw + (b3 >> 2), 0xffu << (8 * (b3 & 3)));
        }
    } else {                                                           // one stored block, then the sync flush
        if (tid == 0) {
            slot[0] = 0;
            slot[1] = (uint8_t)(n & 255); slot[2] = (uint8_t)(n >> 8);
            slot[3] = (uint8_t)(~n & 255); slot[4] = (uint8_t)((~n >> 8) & 255);
            uint8_t* e = slot + 5 + n;
            e[0] = 0; e[1] = 0; e[2] = 0; e[3] = 0xff; e[4] = 0xff;
        }
        for (int i = tid; i < n; i += PE_THREADS) slot[5 + i] = (uint8_t)pe_byte(S.data, i);
    }
    __threadfence();
    __syncthreads();

    // ---- CRC-32 state over "IDAT" (+ the zlib header in front of chunk 0) + the slot's bytes
    uint32_t crc0 = 0xffffffffu;
    crc0 = pe_crc_byte(crc0, 'I'); crc0 = pe_crc_byte(crc0, 'D'); crc0 = pe_crc_byte(crc0, 'A'); crc0 = pe_crc_byte(crc0, 'T');
    if (k == 0) { crc0 = pe_crc_byte(crc0, 0x78); crc0 = pe_crc_byte(crc0, 0x01); }
    const uint32_t per = 4u * ((clen + 4u * PE_THREADS - 1) / (4u * PE_THREADS));     // bytes per thread, whole words
    const uint32_t b0 = (uint32_t)tid * per < clen ? (uint32_t)tid * per : clen;
    const uint32_t b1 = b0 + per < clen ? b0 + per : clen;
    uint32_t r = 0;
    for (uint32_t b = b0; b < b1; b += 4) {
        const uint32_t wv = __builtin_nontemporal_load(slotw + (b >> 2));
        for (uint32_t q = 0; q < 4 && b + q < b1; ++q) r = S.crctab[(r ^ (wv >> (8 * q))) & 255u] ^ (r >> 8);
    }
    uint32_t part = b1 > b0 ? pe_mulmod(r, pe_xpow8(clen - b1)) : 0u;
    if (tid == 0) part ^= pe_mulmod(crc0, pe_xpow8(clen));
    const uint32_t crc = pe_wg_sum(S, part, true);

    // ---- Adler-32 pair of the chunk's raw bytes: A = 1 + sum d_i, B = n + sum (n - i) d_i
    constexpr int APER = PE_CHUNK / PE_THREADS;
    uint32_t sa = 0, sb2 = 0;
    for (int i = tid * APER; i < (tid + 1) * APER && i < n; ++i) {
        const uint32_t d = (uint32_t)pe_byte(S.data, i);
        sa += d;
        sb2 += (uint32_t)(n - i) * d;
    }
    const uint32_t A = (1u + pe_wg_sum(S, sa, false)) % PE_ADLER;
    const uint32_t B = ((uint32_t)n + pe_wg_sum(S, sb2 % PE_ADLER, false)) % PE_ADLER;
    if (tid == 0) {
        PEMeta m;
        m.len = clen; m.crc = crc; m.a = A; m.b = B;
        reinterpret_cast<PEMeta*>(base + pg.off_meta)[k] = m;
    }
}

// ---- kernel 3: one page's offsets, Adler-32 and fixed chunks ------------------------------------------------------------------------------
__device__ inline void pe_put32(uint8_t* o, uint32_t v) { o[0] = (uint8_t)(v >> 24); o[1] = (uint8_t)(v >> 16); o[2] = (uint8_t)(v >> 8); o[3] = (uint8_t)v; }

__global__ __launch_bounds__(PE_SCAN_THREADS) void penc_scan_kernel(PEBatch bt) {
    __shared__ long long sh[PE_SCAN_THREADS];
    const int page = blockIdx.x;
    if (page >= bt.n) return;
    const PEPage& pg = bt.p[page];
    uint8_t* base = bt.ws + pg.ws_off;
    const PEMeta* meta = reinterpret_cast<const PEMeta*>(base + pg.off_meta);
    long long* off = reinterpret_cast<long long*>(base + pg.off_file);
    const int nk = pg.nchunks;
    long long fpos = 8 + 25, asum = 0, bsum = 0;                       // file position of the next IDAT; sum (A_k - 1); B
    for (int i0 = 0; i0 < nk; i0 += PE_SCAN_THREADS) {
        const int i = i0 + (int)threadIdx.x;
        PEMeta m = {0, 0, 1, 0};
        if (i < nk) m = meta[i];
        long long v = i < nk ? 12 + (long long)m.len + (i == 0 ? 2 : 0) + (i == nk - 1 ? 9 : 0) : 0;
        const long long tot = rtn_wg_exclusive_scan<PE_SCAN_THREADS>(sh, v);
        if (i < nk) off[i] = fpos + v;
        fpos += tot;
        long long a = i < nk ? ((long long)m.a + PE_ADLER - 1) % PE_ADLER : 0;
        const long long atot = rtn_wg_exclusive_scan<PE_SCAN_THREADS>(sh, a);
        // joining (A1, B1) with (A2, B2) over len2 bytes: A = A1 + A2 - 1, B = B1 + B2 + len2 (A1 - 1)
        const long long raw = i < nk ? (pg.stream - (long long)i * PE_CHUNK < PE_CHUNK ? pg.stream - (long long)i * PE_CHUNK : PE_CHUNK) : 0;
        long long b = i < nk ? ((long long)m.b + raw * ((asum + a) % PE_ADLER)) % PE_ADLER : 0;
        bsum += rtn_wg_exclusive_scan<PE_SCAN_THREADS>(sh, b);
        asum += atot;
    }
    if (threadIdx.x == 0) {
        off[nk] = fpos;
        const uint32_t adler = (uint32_t)(bsum % PE_ADLER) << 16 | (uint32_t)((1 + asum) % PE_ADLER);
        *reinterpret_cast<uint32_t*>(base + pg.off_file + (long long)(nk + 1) * 8) = adler;
        uint8_t* o = pg.out;
        const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
        for (int i = 0; i < 8; ++i) o[i] = sig[i];
        pe_put32(o + 8, 13);
        o[12] = 'I'; o[13] = 'H'; o[14] = 'D'; o[15] = 'R';
        pe_put32(o + 16, (uint32_t)pg.W);
        pe_put32(o + 20, (uint32_t)pg.H);
        o[24] = 8; o[25] = pg.nc == 3 ? 2 : 0; o[26] = 0; o[27] = 0; o[28] = 0;
        uint32_t c = 0xffffffffu;
        for (int i = 12; i < 29; ++i) c = pe_crc_byte(c, o[i]);
        pe_put32(o + 29, ~c);
        uint8_t* e = o + fpos;
        pe_put32(e, 0);
        e[4] = 'I'; e[5] = 'E'; e[6] = 'N'; e[7] = 'D';
        pe_put32(e + 8, 0xae426082u);
        bt.out_bytes[page] = fpos + 12;
        bt.status[page] = 0;
    }
}

// ---- kernel 4: one IDAT -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PE_THREADS) void penc_copy_kernel(PEBatch bt) {
    const int page = blockIdx.y;
    if (page >= bt.n) return;
    const PEPage& pg = bt.p[page];
    const int k = blockIdx.x, nk = pg.nchunks;
    if (k >= nk) return;
    uint8_t* base = bt.ws + pg.ws_off;
    const PEMeta m = reinterpret_cast<const PEMeta*>(base + pg.off_meta)[k];
    const long long* off = reinterpret_cast<const long long*>(base + pg.off_file);
    const uint32_t* slotw = reinterpret_cast<const uint32_t*>(base + pg.off_slots + (long long)k * PE_SLOT);
    uint8_t* o = pg.out + off[k];
    const bool first = k == 0, last = k == nk - 1;
    uint8_t* body = o + 8 + (first ? 2 : 0);
    for (uint32_t b = 4u * threadIdx.x; b < m.len; b += 4u * PE_THREADS) {
        const uint32_t wv = slotw[b >> 2];
        for (uint32_t q = 0; q < 4 && b + q < m.len; ++q) body[b + q] = (uint8_t)(wv >> (8 * q));
    }
    if (threadIdx.x == 0) {
        pe_put32(o, m.len + (first ? 2u : 0u) + (last ? 9u : 0u));
        o[4] = 'I'; o[5] = 'D'; o[6] = 'A'; o[7] = 'T';
        if (first) { o[8] = 0x78; o[9] = 0x01; }
        uint8_t* e = body + m.len;
        uint32_t c = m.crc;
        if (last) {                                                    // the final empty stored block and the stream's Adler-32
            const uint32_t adler = *reinterpret_cast<const uint32_t*>(base + pg.off_file + (long long)(nk + 1) * 8);
            e[0] = 1; e[1] = 0; e[2] = 0; e[3] = 0xff; e[4] = 0xff;
            pe_put32(e + 5, adler);
            for (int i = 0; i < 9; ++i) c = pe_crc_byte(c, e[i]);
            e += 9;
        }
        pe_put32(e, ~c);
    }
}

int pe_check(rtn_handle_t h, int W, int H, int nc, const char* who) {
    if (pe_valid(W, H, nc)) return RTN_OK;
    if (nc != 1 && nc != 3) return rtn_fail_host(h, RTN_EINVAL, "%s: %d components (1 or 3)", who, nc);
    return rtn_fail_host(h, RTN_EINVAL, "%s: %d x %d page: sides must be >= 1 and height * (1 + width * components) < 2^31", who, W, H);
}

}  // namespace

// rtn_png_encode_bound / rtn_png_encode_workspace_bytes / rtn_png_encode: see include/rtn.h
extern "C" size_t rtn_png_encode_bound(int width, int height, int components) {
    if (pe_check(nullptr, width, height, components, "rtn_png_encode_bound")) return 0;
    return (size_t)pe_bound(width, height, components);
}

extern "C" size_t rtn_png_encode_workspace_bytes(int n, const int32_t* widths, const int32_t* heights, const int32_t* components) {
    if (n <= 0 || !widths || !heights || !components) return 0;
    return rtn_codec_page_bytes(n, [&](int i) { return pe_check(nullptr, widths[i], heights[i], components[i], "rtn_png_encode_workspace_bytes"); },
                                [&](int i) { return pe_layout(widths[i], heights[i], components[i]).total; });
}

extern "C" int rtn_png_encode(rtn_handle_t h, int n, const uint8_t* const* pages, const int32_t* widths, const int32_t* heights,
                              const int32_t* components, uint8_t* out, const int64_t* out_offsets, int64_t* out_bytes,
                              int32_t* status, void* workspace, size_t workspace_bytes) {
    const char* name = "rtn_png_encode";
    const int rc = rtn_encode_check(
        h, name, n, {pages, widths, heights, components, out, out_offsets, out_bytes, status, workspace}, pages, workspace, workspace_bytes,
        [&](int i) { return pe_check(h, widths[i], heights[i], components[i], name); },
        [&](int i) {
            const long long bound = pe_bound(widths[i], heights[i], components[i]);
            if (out_offsets[i] < 0 || out_offsets[i + 1] - out_offsets[i] < bound)
                return rtn_fail(h, RTN_EINVAL, "%s: output slot %d is [%lld, %lld), rtn_png_encode_bound asks for %lld bytes", name, i,
                                (long long)out_offsets[i], (long long)out_offsets[i + 1], bound);
            return RTN_OK;
        },
        [&](int i) { return pe_layout(widths[i], heights[i], components[i]).total; });
    if (rc != RTN_CODEC_GO) return rc;
    return rtn_codec_walk<PEBatch>(n,
        [&](PEBatch& bt, int k, int i, long long ws) {
            if (k == 0) {
                bt.ws = static_cast<uint8_t*>(workspace);
                bt.out_bytes = reinterpret_cast<long long*>(out_bytes + i);
                bt.status = status + i;
            }
            const PELayout L = pe_layout(widths[i], heights[i], components[i]);
            PEPage& p = bt.p[k];
            p.src = pages[i];
            p.out = out + out_offsets[i];
            p.ws_off = ws;
            p.off_meta = L.meta; p.off_file = L.file; p.off_slots = L.slots;
            p.stream = pe_stream(widths[i], heights[i], components[i]);
            p.W = widths[i]; p.H = heights[i]; p.nc = components[i];
            p.nchunks = (int)pe_chunks(p.stream);
            bt.maxrows = p.H > bt.maxrows ? p.H : bt.maxrows;
            bt.maxchunks = p.nchunks > bt.maxchunks ? p.nchunks : bt.maxchunks;
            return L.total;
        },
        [&](const PEBatch& bt, int) {
            penc_filter_kernel<<<dim3(rtn_min_grid(bt.maxrows, PE_MAX_GRID), bt.n), PE_THREADS, 0, h->stream>>>(bt);
            RTN_CHECK_LAUNCH(h, "penc_filter_kernel");
            const int rc = rtn_launch_lds<penc_deflate_kernel>(h, dim3(bt.maxchunks, bt.n), dim3(PE_THREADS), (unsigned)sizeof(PELds),
                                                               (int)sizeof(PELds), bt);
            if (rc) return rc;
            RTN_CHECK_LAUNCH(h, "penc_deflate_kernel");
            penc_scan_kernel<<<bt.n, PE_SCAN_THREADS, 0, h->stream>>>(bt);
            RTN_CHECK_LAUNCH(h, "penc_scan_kernel");
            penc_copy_kernel<<<dim3(bt.maxchunks, bt.n), PE_THREADS, 0, h->stream>>>(bt);
            RTN_CHECK_LAUNCH(h, "penc_copy_kernel");
            return RTN_OK;
        });
}
