// rtn_jpeg_enc.hip — baseline JPEG pages encoded on the device, byte-identical to what Pillow (libjpeg-turbo) writes for
// Image.save(f, "JPEG", quality=q, subsampling=s): JFIF 1.01 header, the Annex K quantisation tables scaled by q, the standard
// Huffman tables, one interleaved scan, no restart markers, no optimisation pass.
//
// Host: the header (SOI .. SOS) is one __host__ __device__ function, so rtn_jpeg_encode_header and the device write the same bytes.
// Device, five kernels per batch of up to RTN_CODEC_BATCH pages (each page's work stays inside its own workgroups; no workgroup
// waits on another):
//   1. jenc_transform_kernel: one thread per 8x8 block in scan order (MCU order, dummy blocks included): rgb_ycc_convert, edge
//      replication, h2v1 / h2v2 downsampling, jpeg_fdct_islow, quantisation; writes the zig-zagged int16 coefficients.
//   2. jenc_bits_kernel: the Huffman bit length of every block (its DC difference reads the predecessor's DC in scan order) and
//      the sum over each 256-block tile.
//   3. jenc_scan_kernel: one workgroup per page: exclusive scan of the tile sums (64-bit bit offsets), the status word, and the
//      zeroing of the packed stream the next kernel ORs into.
//   4. jenc_pack_kernel: one thread per block writes its codes at its bit offset into a big-endian word stream: full words with
//      plain stores, the (at most two) words it shares with its neighbours with a vector atomic OR (order-independent).
//   5. jenc_assemble_kernel: one workgroup per page: pads the last byte with 1-bits, counts the 0xFF bytes per thread chunk,
//      scans, and writes header + stuffed stream + EOI into the page's output slot, and the file length.
// A page whose file would not fit its slot gets a non-zero status word and a length of 0: the caller encodes it on the host.
#include "rtn_codec_launch.h"

namespace {

constexpr int JE_TILE = 256;                   // blocks per tile of the bit-offset scan (= workgroup of kernels 1, 2, 4)
constexpr int JE_SCAN_THREADS = 1024;          // workgroup of kernels 3 and 5: one page
constexpr int JE_BLOCK_BITS = 16 + 11 + 63 * (16 + 10);   // most bits one block can take: DC code + value, 63 x (AC code + value)
constexpr int JE_HDR_MAX = 640;                // header bytes: 623 for three components, 328 for one
constexpr int JE_MAX_DIM = 65500;              // libjpeg's JPEG_MAX_DIMENSION

struct JEPage {
    const uint8_t* src;                        // (H, W, 3) B,G,R or (H, W) gray
    uint8_t* out;                              // the page's output slot
    long long cap;                             // slot bytes
    long long ws_off;                          // start of the page's workspace
    long long off_bits, off_tiles, off_stream; // workspace sections, relative to ws_off
    long long stream_words;                    // capacity of the packed stream
    int W, H, nc, ss, q, nblocks, ntiles, pad_;
};

struct JEBatch {
    int n, maxblocks, pad_[2];
    JEPage p[RTN_CODEC_BATCH];
};

__host__ __device__ constexpr int je_natural(int k) {
    constexpr unsigned char nat[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20,
                                       13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59,
                                       52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return nat[k & 63];
}

// Annex K.1 quantisation tables in zig-zag order (t = 0 luminance, 1 chrominance)
__host__ __device__ inline int je_base_quant(int t, int k) {
    constexpr unsigned char q[128] = {
        16, 11, 12, 14, 12, 10, 16, 14, 13, 14, 18, 17, 16, 19, 24, 40, 26, 24, 22, 22, 24, 49, 35, 37, 29, 40, 58, 51, 61, 60, 57, 51,
        56, 55, 64, 72, 92, 78, 64, 68, 87, 69, 55, 56, 80, 109, 81, 87, 95, 98, 103, 104, 103, 62, 77, 113, 121, 112, 100, 120, 92,
        101, 103, 99,
        17, 18, 18, 24, 21, 24, 47, 26, 26, 47, 99, 66, 56, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
        99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
    return q[(t & 1) * 64 + (k & 63)];
}

// jcparam.c jpeg_quality_scaling + jpeg_add_quant_table with force_baseline
__host__ __device__ inline int je_quant(int t, int k, int quality) {
    const int scale = quality < 50 ? 5000 / quality : 200 - quality * 2;
    int v = (je_base_quant(t, k) * scale + 50) / 100;
    return v < 1 ? 1 : (v > 255 ? 255 : v);
}

// Annex K.3 Huffman tables: t = 0 DC luminance, 1 AC luminance, 2 DC chrominance, 3 AC chrominance
__host__ __device__ inline int je_huff_bits(int t, int l) {          // codes of length l + 1, l = 0..15
    constexpr unsigned char b[64] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0,
                                     0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125,
                                     0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0,
                                     0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119};
    return b[(t & 3) * 16 + (l & 15)];
}
__host__ __device__ inline int je_huff_count(int t) { return (t & 1) ? 162 : 12; }
__host__ __device__ inline int je_huff_val(int t, int i) {
    constexpr unsigned char ac_l[162] = {
        0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
        0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
        0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
        0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
        0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
        0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
        0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
        0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
    constexpr unsigned char ac_c[162] = {
        0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
        0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
        0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
        0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
        0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
        0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
        0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
        0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
    if (!(t & 1)) return i;                                        // DC: categories 0..11 in order
    return (t & 2) ? ac_c[i % 162] : ac_l[i % 162];
}

// ---- geometry (jcmaster.c initial_setup / per_scan_setup for one interleaved scan) ------------------------------------------
struct JEGeom {
    int nc, hmax, vmax, mcux, mcuy, bpm, nblocks;
    int wib[3], hib[3];                        // width_in_blocks / height_in_blocks of each component
};

__host__ __device__ inline JEGeom je_geom(int W, int H, int nc, int ss) {
    JEGeom g;
    g.nc = nc;
    if (nc == 1) {                             // one component, non-interleaved: MCU = one block, no dummy blocks
        g.hmax = g.vmax = 1;
        g.mcux = (W + 7) / 8; g.mcuy = (H + 7) / 8; g.bpm = 1;
        g.wib[0] = g.mcux; g.hib[0] = g.mcuy;
        g.wib[1] = g.wib[2] = g.hib[1] = g.hib[2] = 0;
    } else {
        g.hmax = ss >= 1 ? 2 : 1;
        g.vmax = ss == 2 ? 2 : 1;
        g.mcux = (W + 8 * g.hmax - 1) / (8 * g.hmax);
        g.mcuy = (H + 8 * g.vmax - 1) / (8 * g.vmax);
        g.bpm = g.hmax * g.vmax + 2;
        g.wib[0] = (W + 7) / 8; g.hib[0] = (H + 7) / 8;
        g.wib[1] = g.wib[2] = (W + 8 * g.hmax - 1) / (8 * g.hmax);
        g.hib[1] = g.hib[2] = (H + 8 * g.vmax - 1) / (8 * g.vmax);
    }
    g.nblocks = g.mcux * g.mcuy * g.bpm;
    return g;
}

// ---- header ---------------------------------------------------------------------------------------------------------------
__host__ __device__ inline int je_header_bytes(int nc) {
    const int ntab = nc == 1 ? 1 : 2;
    return 2 + 18 + ntab * 69 + (10 + 3 * nc) + ntab * ((2 + 2 + 17 + 12) + (2 + 2 + 17 + 162)) + (8 + 2 * nc);
}

// SOI, APP0 (JFIF 1.01, density 1:1, no unit), DQT per table, SOF0, DHT per table (DC then AC of each table set), SOS: the markers
// and grouping libjpeg's jcmarker.c writes with Pillow's settings.  Returns the bytes written (je_header_bytes(nc)).
__host__ __device__ inline int je_write_header(uint8_t* o, int W, int H, int nc, int ss, int quality) {
    int p = 0;
    auto b = [&](int v) { o[p++] = (uint8_t)v; };
    auto w16 = [&](int v) { b(v >> 8); b(v & 255); };
    w16(0xFFD8);
    w16(0xFFE0); w16(16); b('J'); b('F'); b('I'); b('F'); b(0); b(1); b(1); b(0); w16(1); w16(1); b(0); b(0);
    const int ntab = nc == 1 ? 1 : 2;
    for (int t = 0; t < ntab; ++t) {
        w16(0xFFDB); w16(67); b(t);
        for (int k = 0; k < 64; ++k) b(je_quant(t, k, quality));
    }
    const int samp0 = ss == 0 ? 0x11 : (ss == 1 ? 0x21 : 0x22);  // Pillow sets the first component's factors for gray pages too
    w16(0xFFC0); w16(8 + 3 * nc); b(8); w16(H); w16(W); b(nc);
    for (int c = 0; c < nc; ++c) { b(c + 1); b(c == 0 ? samp0 : 0x11); b(c == 0 ? 0 : 1); }
    for (int t = 0; t < 2 * ntab; ++t) {
        const int cnt = je_huff_count(t);
        w16(0xFFC4); w16(2 + 1 + 16 + cnt); b(((t & 1) << 4) | (t >> 1));
        for (int l = 0; l < 16; ++l) b(je_huff_bits(t, l));
        for (int i = 0; i < cnt; ++i) b(je_huff_val(t, i));
    }
    w16(0xFFDA); w16(6 + 2 * nc); b(nc);
    for (int c = 0; c < nc; ++c) { b(c + 1); b(c == 0 ? 0x00 : 0x11); }
    b(0); b(63); b(0);
    return p;
}

// ---- per-page workspace ---------------------------------------------------------------------------------------------------
struct JELayout { long long bits, tiles, stream, total, stream_words; int ntiles; };

inline JELayout je_layout(const JEGeom& g) {
    JELayout L;
    L.ntiles = (g.nblocks + JE_TILE - 1) / JE_TILE;
    L.stream_words = ((long long)g.nblocks * JE_BLOCK_BITS + 31) / 32 + 1;
    L.bits = rtn_align256((long long)g.nblocks * 128);                 // coefficients: [nblocks][64] int16, zig-zag order
    L.tiles = L.bits + rtn_align256((long long)g.nblocks * 4);         // bits per block (int32)
    // tile bit offsets (int64, ntiles + 1, the last one the page's total), tile sums (int32), the page's no-code flag (int32)
    L.stream = L.tiles + rtn_align256((long long)(L.ntiles + 1) * 8 + (long long)L.ntiles * 4 + 4);
    L.total = L.stream + rtn_align256((long long)L.stream_words * 4);
    return L;
}

// the largest file: header + every block at JE_BLOCK_BITS, every stream byte stuffed, the pad byte, EOI
inline long long je_bound(const JEGeom& g) {
    return je_header_bytes(g.nc) + 2 * (((long long)g.nblocks * JE_BLOCK_BITS + 7) / 8 + 1) + 2;
}

// ---- per-block helpers (host and device) ----------------------------------------------------------------------------------
__host__ __device__ inline void je_block_coords(const JEGeom& g, int j, int* c, int* by, int* bx, int* mx) {
    if (g.nc == 1) {
        *c = 0; *by = j / g.mcux; *bx = j - *by * g.mcux; *mx = *bx;
        return;
    }
    const int m = j / g.bpm, b = j - m * g.bpm;
    const int my = m / g.mcux;
    *mx = m - my * g.mcux;
    const int nY = g.hmax * g.vmax;
    if (b < nY) {
        const int dy = b / g.hmax, dx = b - dy * g.hmax;
        *c = 0; *by = my * g.vmax + dy; *bx = *mx * g.hmax + dx;
    } else {
        *c = b - nY + 1; *by = my; *bx = *mx;
    }
}

// jccolor.c rgb_ycc_convert, SCALEBITS 16
__host__ __device__ inline int je_ycc(const uint8_t* px, int c) {
    const int B = px[0], G = px[1], R = px[2];
    if (c == 0) return (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
    if (c == 1) return (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
    return (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
}

// sample (x, y) of component c's (edge-replicated, downsampled) plane
__host__ __device__ inline int je_sample(const JEPage& pg, const JEGeom& g, int c, int x, int y) {
    const int W = pg.W, H = pg.H;
    if (g.nc == 1) return pg.src[(long long)min(y, H - 1) * W + min(x, W - 1)];
    auto px = [&](int xx, int yy) { return pg.src + ((long long)min(yy, H - 1) * W + min(xx, W - 1)) * 3; };
    if (c == 0 || g.hmax == 1) return je_ycc(px(x, y), c);                          // full size
    if (g.vmax == 1) {                                                              // h2v1_downsample
        return (je_ycc(px(2 * x, y), c) + je_ycc(px(2 * x + 1, y), c) + (x & 1)) >> 1;
    }
    // h2v2_downsample of input rows replicated to a multiple of 2; then the last downsampled row repeats to the iMCU height
    const int yd = min(y, (H + 1) / 2 - 1);
    return (je_ycc(px(2 * x, 2 * yd), c) + je_ycc(px(2 * x + 1, 2 * yd), c) + je_ycc(px(2 * x, 2 * yd + 1), c) +
            je_ycc(px(2 * x + 1, 2 * yd + 1), c) + 1 + (x & 1)) >> 2;
}

#define JE_FIX_0_298631336 2446
#define JE_FIX_0_390180644 3196
#define JE_FIX_0_541196100 4433
#define JE_FIX_0_765366865 6270
#define JE_FIX_0_899976223 7373
#define JE_FIX_1_175875602 9633
#define JE_FIX_1_501321110 12299
#define JE_FIX_1_847759065 15137
#define JE_FIX_1_961570560 16069
#define JE_FIX_2_053119869 16819
#define JE_FIX_2_562915447 20995
#define JE_FIX_3_072711026 25172

// one 1-D pass of jfdctint.c jpeg_fdct_islow over d[0], d[s], ..., d[7 s]: pass 1 (rows) shifts the even part left by PASS1_BITS
// and descales the odd part by CONST_BITS - PASS1_BITS; pass 2 (columns) descales by PASS1_BITS and CONST_BITS + PASS1_BITS
__host__ __device__ inline void je_fdct_1d(int* d, int s, bool pass1) {
    const int tmp0 = d[0] + d[7 * s], tmp7 = d[0] - d[7 * s];
    const int tmp1 = d[s] + d[6 * s], tmp6 = d[s] - d[6 * s];
    const int tmp2 = d[2 * s] + d[5 * s], tmp5 = d[2 * s] - d[5 * s];
    const int tmp3 = d[3 * s] + d[4 * s], tmp4 = d[3 * s] - d[4 * s];
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    const int sh = pass1 ? 13 - 2 : 13 + 2;
    const int r = 1 << (sh - 1);
    if (pass1) { d[0] = (tmp10 + tmp11) * 4; d[4 * s] = (tmp10 - tmp11) * 4; }
    else { d[0] = (tmp10 + tmp11 + 2) >> 2; d[4 * s] = (tmp10 - tmp11 + 2) >> 2; }
    int z1 = (tmp12 + tmp13) * JE_FIX_0_541196100;
    d[2 * s] = (z1 + tmp13 * JE_FIX_0_765366865 + r) >> sh;
    d[6 * s] = (z1 - tmp12 * JE_FIX_1_847759065 + r) >> sh;
    z1 = tmp4 + tmp7;
    int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int z5 = (z3 + z4) * JE_FIX_1_175875602;
    const int t4 = tmp4 * JE_FIX_0_298631336, t5 = tmp5 * JE_FIX_2_053119869;
    const int t6 = tmp6 * JE_FIX_3_072711026, t7 = tmp7 * JE_FIX_1_501321110;
    z1 *= -JE_FIX_0_899976223; z2 *= -JE_FIX_2_562915447;
    z3 = z3 * -JE_FIX_1_961570560 + z5; z4 = z4 * -JE_FIX_0_390180644 + z5;
    d[7 * s] = (t4 + z1 + z3 + r) >> sh;
    d[5 * s] = (t5 + z2 + z4 + r) >> sh;
    d[3 * s] = (t6 + z2 + z3 + r) >> sh;
    d[s] = (t7 + z1 + z4 + r) >> sh;
}

// Huffman code tables in LDS: code | (length << 16) per symbol, 0 = no code (t as in je_huff_bits)
__device__ inline void je_build_codes(uint32_t (*codes)[256]) {
    const int t = threadIdx.x;
    if (t < 4) {
        for (int s = 0; s < 256; ++s) codes[t][s] = 0;
        int code = 0, k = 0;
        for (int l = 0; l < 16; ++l) {
            for (int i = 0; i < je_huff_bits(t, l); ++i) codes[t][je_huff_val(t, k++)] = (uint32_t)code++ | ((uint32_t)(l + 1) << 16);
            code <<= 1;
        }
    }
    __syncthreads();
}

__host__ __device__ inline int je_nbits(int v) { return v ? 32 - __builtin_clz((unsigned)v) : 0; }

// Entropy-code one block (jchuff.c encode_one_block): emit(bits, length) per DC / AC field, code and value bits joined (<= 27 bits).
// Returns false where a symbol has no code (cannot happen for 8-bit samples; the caller then flags the page).
template <class Emit>
__host__ __device__ inline bool je_code_block(const int* zz, int pred, const uint32_t* dct, const uint32_t* act, Emit& emit) {
    bool ok = true;
    int v = zz[0] - pred;
    int v2 = v;
    if (v < 0) { v = -v; v2 -= 1; }
    int nb = je_nbits(v);
    uint32_t e = dct[nb & 255];
    ok &= e != 0 && nb <= 11;
    int len = (int)(e >> 16);
    emit(((e & 0xffffu) << nb) | ((uint32_t)v2 & ((1u << nb) - 1)), len + nb);
    int r = 0;
#pragma unroll
    for (int k = 1; k < 64; ++k) {
        v = zz[k];
        if (v == 0) { ++r; continue; }
        while (r > 15) { const uint32_t z = act[0xF0]; emit(z & 0xffffu, (int)(z >> 16)); r -= 16; }
        v2 = v;
        if (v < 0) { v = -v; v2 -= 1; }
        nb = je_nbits(v);
        e = act[((r << 4) + nb) & 255];
        ok &= e != 0 && nb <= 10;
        len = (int)(e >> 16);
        emit(((e & 0xffffu) << nb) | ((uint32_t)v2 & ((1u << nb) - 1)), len + nb);
        r = 0;
    }
    if (r > 0) { const uint32_t z = act[0]; emit(z & 0xffffu, (int)(z >> 16)); }
    return ok;
}

// the 64 zig-zagged coefficients of block j and the DC of its predecessor in scan order (same component; 0 for the first)
__host__ __device__ inline int je_load_block(const int16_t* coef, const JEGeom& g, int j, int* zz) {
    const int4* s = reinterpret_cast<const int4*>(coef + (long long)j * 64);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int4 v = s[i];
        const int w[4] = {v.x, v.y, v.z, v.w};
        for (int h = 0; h < 4; ++h) { zz[i * 8 + 2 * h] = (int)(int16_t)(w[h] & 0xffff); zz[i * 8 + 2 * h + 1] = w[h] >> 16; }
    }
    int pj = -1;
    if (g.nc == 1) pj = j - 1;
    else {
        const int m = j / g.bpm, b = j - m * g.bpm, nY = g.hmax * g.vmax;
        if (b > 0 && b < nY) pj = j - 1;                               // luma blocks inside one MCU
        else if (m > 0) pj = b == 0 ? j - g.bpm + nY - 1 : j - g.bpm; // last luma block / same chroma block of the previous MCU
    }
    return pj >= 0 ? (int)coef[(long long)pj * 64] : 0;
}

// block j of the page in scan order: colour conversion, edge replication, downsampling, FDCT, quantisation -> 32 words of
// zig-zagged int16 pairs.  qt: the two quantisation tables in zig-zag order, times 8 (the FDCT's scale)
__host__ __device__ inline void je_transform_block(const JEPage& pg, const int* qt, int j, int out[32]) {
    const JEGeom g = je_geom(pg.W, pg.H, pg.nc, pg.ss);
    int c, by, bx, mx;
    je_block_coords(g, j, &c, &by, &bx, &mx);
    // dummy blocks (jccoefct.c compress_data): AC 0, DC of the block libjpeg copies it from
    bool dummy = false;
    if (c == 0 && g.nc == 3) {
        if (by >= g.hib[0]) { dummy = true; by -= 1; bx = min(mx * g.hmax + g.hmax - 1, g.wib[0] - 1); }
        else if (bx >= g.wib[0]) { dummy = true; bx = g.wib[0] - 1; }
    }
    int d[64];
    for (int y = 0; y < 8; ++y)
        for (int x = 0; x < 8; ++x) d[y * 8 + x] = je_sample(pg, g, c, bx * 8 + x, by * 8 + y) - 128;
    for (int y = 0; y < 8; ++y) je_fdct_1d(d + y * 8, 1, true);
    for (int x = 0; x < 8; ++x) je_fdct_1d(d + x, 8, false);
    const int* q = qt + (c > 0 ? 64 : 0);
    for (int k = 0; k < 64; k += 2) {
        int pair[2];
        for (int h = 0; h < 2; ++h) {
            const int x = d[je_natural(k + h)], qd = q[k + h];
            int v = x < 0 ? -((-x + (qd >> 1)) / qd) : (x + (qd >> 1)) / qd;
            if (dummy && k + h > 0) v = 0;
            pair[h] = v;
        }
        out[k >> 1] = (int)(((uint32_t)pair[0] & 0xffffu) | ((uint32_t)pair[1] << 16));
    }
}

// ---- kernels --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(JE_TILE) void jenc_transform_kernel(uint8_t* __restrict__ ws, JEBatch bt) {
    __shared__ int qt[2][64];
    const int page = blockIdx.y;
    if (page >= bt.n) return;
    const JEPage& pg = bt.p[page];
    if (threadIdx.x < 128) qt[threadIdx.x >> 6][threadIdx.x & 63] = 8 * je_quant(threadIdx.x >> 6, threadIdx.x & 63, pg.q);
    __syncthreads();
    const int j = blockIdx.x * JE_TILE + threadIdx.x;
    if (j >= pg.nblocks) return;
    if (j == 0) *reinterpret_cast<int*>(ws + pg.ws_off + pg.off_tiles + (long long)(pg.ntiles + 1) * 8 + (long long)pg.ntiles * 4) = 0;
    int out[32];
    je_transform_block(pg, &qt[0][0], j, out);
    int4* dst = reinterpret_cast<int4*>(ws + pg.ws_off + (long long)j * 128);
    for (int i = 0; i < 8; ++i) dst[i] = make_int4(out[4 * i], out[4 * i + 1], out[4 * i + 2], out[4 * i + 3]);
}

__global__ __launch_bounds__(JE_TILE) void jenc_bits_kernel(uint8_t* __restrict__ ws, JEBatch bt) {
    __shared__ uint32_t codes[4][256];
    __shared__ int part[JE_TILE / 64];
    const int page = blockIdx.y;
    if (page >= bt.n) return;
    const JEPage& pg = bt.p[page];
    const int tile = blockIdx.x;
    if (tile >= pg.ntiles) return;
    je_build_codes(codes);
    const int j = tile * JE_TILE + threadIdx.x;
    uint8_t* base = ws + pg.ws_off;
    int bits = 0;
    if (j < pg.nblocks) {
        const JEGeom g = je_geom(pg.W, pg.H, pg.nc, pg.ss);
        int zz[64];
        const int pred = je_load_block(reinterpret_cast<const int16_t*>(base), g, j, zz);
        int c, by, bx, mx;
        je_block_coords(g, j, &c, &by, &bx, &mx);
        const int t = c > 0 ? 2 : 0;
        auto count = [&](uint32_t, int len) { bits += len; };
        if (!je_code_block(zz, pred, codes[t], codes[t + 1], count))                   // flags the page
            *reinterpret_cast<int*>(base + pg.off_tiles + (long long)(pg.ntiles + 1) * 8 + (long long)pg.ntiles * 4) = 1;
        reinterpret_cast<int*>(base + pg.off_bits)[j] = bits;
    }
    int s = bits;
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot = 0;
        for (int w = 0; w < JE_TILE / 64; ++w) tot += part[w];
        reinterpret_cast<int*>(base + pg.off_tiles + (long long)(pg.ntiles + 1) * 8)[tile] = tot;
    }
}

__global__ __launch_bounds__(JE_SCAN_THREADS) void jenc_scan_kernel(uint8_t* __restrict__ ws, int32_t* __restrict__ status,
                                                                    long long* __restrict__ out_bytes, JEBatch bt) {
    __shared__ long long sh[JE_SCAN_THREADS];
    const int page = blockIdx.x;
    if (page >= bt.n) return;
    const JEPage& pg = bt.p[page];
    uint8_t* base = ws + pg.ws_off;
    long long* off = reinterpret_cast<long long*>(base + pg.off_tiles);
    const int* sums = reinterpret_cast<const int*>(base + pg.off_tiles + (long long)(pg.ntiles + 1) * 8);
    long long carry = 0;
    for (int i0 = 0; i0 < pg.ntiles; i0 += JE_SCAN_THREADS) {
        const int i = i0 + threadIdx.x;
        long long v = i < pg.ntiles ? sums[i] : 0;
        const long long tot = rtn_wg_exclusive_scan<JE_SCAN_THREADS>(sh, v);
        if (i < pg.ntiles) off[i] = carry + v;
        carry += tot;
    }
    const long long total_bits = carry;
    const int nocode = *reinterpret_cast<const int*>(base + pg.off_tiles + (long long)(pg.ntiles + 1) * 8 + (long long)pg.ntiles * 4);
    const bool fits = nocode == 0 && total_bits <= (pg.stream_words - 1) * 32;
    if (threadIdx.x == 0) {
        off[pg.ntiles] = total_bits;
        status[page] = fits ? 0 : 1;
        out_bytes[page] = 0;
    }
    if (!fits) return;
    uint32_t* words = reinterpret_cast<uint32_t*>(base + pg.off_stream);
    const long long nw = (total_bits + 31) / 32;
    for (long long i = threadIdx.x; i < nw; i += JE_SCAN_THREADS) words[i] = 0u;
}

// big-endian bit writer over the page's word stream: words only this block owns are stored, shared ones ORed atomically
struct JEWriter {
    uint32_t* w;
    uint64_t acc;                              // pending bits, left-aligned: bit 63 = bit `base` of word *w
    int fill;                                  // valid bits in acc (counting from bit 63)
    bool first;                                // *w is the block's first word (shared with the previous block)
    __device__ inline void flush_word() {
        const uint32_t v = __builtin_bswap32((uint32_t)(acc >> 32));
        if (first) atomicOr(w, v);
        else *w = v;
        ++w; acc <<= 32; fill -= 32; first = false;
    }
    __device__ inline void operator()(uint32_t bits, int len) {
        acc |= (uint64_t)bits << (64 - fill - len);
        fill += len;
        if (fill >= 32) flush_word();
    }
    __device__ inline void finish() {
        if (fill > 0) atomicOr(w, __builtin_bswap32((uint32_t)(acc >> 32)));   // shared with the next block
    }
};

__global__ __launch_bounds__(JE_TILE) void jenc_pack_kernel(uint8_t* __restrict__ ws, const int32_t* __restrict__ status, JEBatch bt) {
    __shared__ uint32_t codes[4][256];
    __shared__ int part[JE_TILE / 64];
    const int page = blockIdx.y;
    if (page >= bt.n) return;
    const JEPage& pg = bt.p[page];
    const int tile = blockIdx.x;
    if (tile >= pg.ntiles || status[page] != 0) return;
    je_build_codes(codes);
    const int j = tile * JE_TILE + threadIdx.x;
    uint8_t* base = ws + pg.ws_off;
    const int bits = j < pg.nblocks ? reinterpret_cast<const int*>(base + pg.off_bits)[j] : 0;
    // exclusive scan of the tile's bit lengths: inside each wave, then across the four waves
    int s = bits;
    const int lane = threadIdx.x & 63;
    for (int o = 1; o < 64; o <<= 1) {
        const int a = __shfl_up(s, o);
        if (lane >= o) s += a;
    }
    if (lane == 63) part[threadIdx.x >> 6] = s;
    __syncthreads();
    long long pos = reinterpret_cast<const long long*>(base + pg.off_tiles)[tile] + (s - bits);
    for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) pos += part[w];
    if (j >= pg.nblocks) return;
    const JEGeom g = je_geom(pg.W, pg.H, pg.nc, pg.ss);
    int zz[64];
    const int pred = je_load_block(reinterpret_cast<const int16_t*>(base), g, j, zz);
    int c, by, bx, mx;
    je_block_coords(g, j, &c, &by, &bx, &mx);
    const int t = c > 0 ? 2 : 0;
    JEWriter wr;
    wr.w = reinterpret_cast<uint32_t*>(base + pg.off_stream) + (pos >> 5);
    wr.fill = (int)(pos & 31);
    wr.acc = 0;
    wr.first = true;
    je_code_block(zz, pred, codes[t], codes[t + 1], wr);
    wr.finish();
}

__global__ __launch_bounds__(JE_SCAN_THREADS) void jenc_assemble_kernel(uint8_t* __restrict__ ws, int32_t* __restrict__ status,
                                                                        long long* __restrict__ out_bytes, JEBatch bt) {
    __shared__ long long sh[JE_SCAN_THREADS];
    __shared__ uint8_t hdr[JE_HDR_MAX];
    const int page = blockIdx.x;
    if (page >= bt.n) return;
    const JEPage& pg = bt.p[page];
    if (status[page] != 0) return;
    uint8_t* base = ws + pg.ws_off;
    const long long total_bits = reinterpret_cast<const long long*>(base + pg.off_tiles)[pg.ntiles];
    const uint32_t* words = reinterpret_cast<const uint32_t*>(base + pg.off_stream);
    const long long nbytes = (total_bits + 7) / 8;
    const long long nwords = (nbytes + 3) / 4;
    const long long per = (nwords + JE_SCAN_THREADS - 1) / JE_SCAN_THREADS;
    const long long w0 = min((long long)threadIdx.x * per, nwords), w1 = min(w0 + per, nwords);
    const int pad_byte = (int)(total_bits & 7) ? (int)(nbytes - 1) : -1;     // jchuff.c flush_bits: fill with 1-bits
    const uint32_t pad = 0xFFu >> (total_bits & 7);
    auto byte_at = [&](long long wi, int k, uint32_t wv) -> uint32_t {
        const long long bi = wi * 4 + k;
        uint32_t v = (wv >> (8 * k)) & 0xFFu;
        if (bi == pad_byte) v |= pad;
        return v;
    };
    long long ff = 0;
    for (long long wi = w0; wi < w1; ++wi) {
        const uint32_t wv = words[wi];
        for (int k = 0; k < 4; ++k)
            if (wi * 4 + k < nbytes && byte_at(wi, k, wv) == 0xFFu) ++ff;
    }
    const long long total_ff = rtn_wg_exclusive_scan<JE_SCAN_THREADS>(sh, ff);
    const int hb = je_header_bytes(pg.nc);
    const long long len = hb + nbytes + total_ff + 2;
    if (len > pg.cap) {
        if (threadIdx.x == 0) status[page] = 2;
        return;
    }
    if (threadIdx.x == 0) je_write_header(hdr, pg.W, pg.H, pg.nc, pg.ss, pg.q);
    __syncthreads();
    uint8_t* out = pg.out;
    for (int i = threadIdx.x; i < hb; i += JE_SCAN_THREADS) out[i] = hdr[i];
    long long p = hb + w0 * 4 + ff;
    for (long long wi = w0; wi < w1; ++wi) {
        const uint32_t wv = words[wi];
        for (int k = 0; k < 4; ++k) {
            if (wi * 4 + k >= nbytes) break;
            const uint32_t v = byte_at(wi, k, wv);
            out[p++] = (uint8_t)v;
            if (v == 0xFFu) out[p++] = 0;
        }
    }
    if (threadIdx.x == 0) {
        out[len - 2] = 0xFF;
        out[len - 1] = 0xD9;
        out_bytes[page] = len;
    }
}

int je_check(rtn_handle_t h, int W, int H, int nc, int ss, int q, const char* who) {
    if (q < 1 || q > 100) return rtn_fail_host(h, RTN_EINVAL, "%s: quality %d outside 1..100", who, q);
    if (W < 1 || W > JE_MAX_DIM || H < 1 || H > JE_MAX_DIM)
        return rtn_fail_host(h, RTN_EINVAL, "%s: %d x %d page: width and height must be 1..%d", who, W, H, JE_MAX_DIM);
    if (nc != 1 && nc != 3) return rtn_fail_host(h, RTN_EINVAL, "%s: %d components (1 or 3)", who, nc);
    if (ss < 0 || ss > 2) return rtn_fail_host(h, RTN_EINVAL, "%s: subsampling %d (0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0)", who, ss);
    return RTN_OK;
}

}  // namespace

// rtn_jpeg_encode_header / rtn_jpeg_encode_bound / rtn_jpeg_encode_workspace_bytes / rtn_jpeg_encode: see include/rtn.h
extern "C" int rtn_jpeg_encode_header(int width, int height, int components, int subsampling, int quality, uint8_t* out,
                                      size_t capacity, size_t* written) {
    if (written) *written = 0;
    const int rc = je_check(nullptr, width, height, components, subsampling, quality, "rtn_jpeg_encode_header");
    if (rc) return rc;
    const int n = je_header_bytes(components);
    if (!out || (size_t)n > capacity)
        return rtn_fail_host(nullptr, RTN_EINVAL, "rtn_jpeg_encode_header: %zu-byte buffer, %d bytes needed", out ? capacity : (size_t)0, n);
    const int got = je_write_header(out, width, height, components, subsampling, quality);
    if (got != n) return RTN_EINVAL;
    if (written) *written = (size_t)n;
    return RTN_OK;
}

extern "C" size_t rtn_jpeg_encode_bound(int width, int height, int components, int subsampling) {
    if (je_check(nullptr, width, height, components, subsampling, 75, "rtn_jpeg_encode_bound")) return 0;
    return (size_t)je_bound(je_geom(width, height, components, subsampling));
}

extern "C" size_t rtn_jpeg_encode_workspace_bytes(int n, const int32_t* widths, const int32_t* heights, const int32_t* components,
                                                  const int32_t* subsampling) {
    if (n <= 0 || !widths || !heights || !components || !subsampling) return 0;
    return rtn_codec_page_bytes(
        n, [&](int i) { return je_check(nullptr, widths[i], heights[i], components[i], subsampling[i], 75, "rtn_jpeg_encode_workspace_bytes"); },
        [&](int i) { return je_layout(je_geom(widths[i], heights[i], components[i], subsampling[i])).total; });
}

extern "C" int rtn_jpeg_encode(rtn_handle_t h, int n, const uint8_t* const* pages, const int32_t* widths, const int32_t* heights,
                               const int32_t* components, const int32_t* subsampling, const int32_t* quality, uint8_t* out,
                               const int64_t* out_offsets, int64_t* out_bytes, int32_t* status, void* workspace,
                               size_t workspace_bytes) {
    const char* name = "rtn_jpeg_encode";
    const int rc = rtn_encode_check(
        h, name, n, {pages, widths, heights, components, subsampling, quality, out, out_offsets, out_bytes, status, workspace}, pages, workspace,
        workspace_bytes, [&](int i) { return je_check(h, widths[i], heights[i], components[i], subsampling[i], quality[i], name); },
        [&](int i) {
            if (out_offsets[i] < 0 || out_offsets[i + 1] < out_offsets[i])
                return rtn_fail(h, RTN_EINVAL, "%s: output slot %d is [%lld, %lld)", name, i, (long long)out_offsets[i], (long long)out_offsets[i + 1]);
            return RTN_OK;
        },
        [&](int i) { return je_layout(je_geom(widths[i], heights[i], components[i], subsampling[i])).total; });
    if (rc != RTN_CODEC_GO) return rc;
    uint8_t* wsp = static_cast<uint8_t*>(workspace);
    return rtn_codec_walk<JEBatch>(n,
        [&](JEBatch& bt, int k, int i, long long ws) {
            const JEGeom g = je_geom(widths[i], heights[i], components[i], subsampling[i]);
            const JELayout L = je_layout(g);
            JEPage& p = bt.p[k];
            p.src = pages[i];
            p.out = out + out_offsets[i];
            p.cap = out_offsets[i + 1] - out_offsets[i];
            p.ws_off = ws;
            p.off_bits = L.bits; p.off_tiles = L.tiles; p.off_stream = L.stream;
            p.W = widths[i]; p.H = heights[i]; p.nc = components[i]; p.ss = subsampling[i]; p.q = quality[i];
            p.nblocks = g.nblocks; p.ntiles = L.ntiles; p.stream_words = L.stream_words;
            bt.maxblocks = g.nblocks > bt.maxblocks ? g.nblocks : bt.maxblocks;
            return L.total;
        },
        [&](const JEBatch& bt, int i0) {
            const dim3 grid((bt.maxblocks + JE_TILE - 1) / JE_TILE, bt.n);
            long long* lengths = reinterpret_cast<long long*>(out_bytes + i0);
            jenc_transform_kernel<<<grid, JE_TILE, 0, h->stream>>>(wsp, bt);
            RTN_CHECK_LAUNCH(h, "jenc_transform_kernel");
            jenc_bits_kernel<<<grid, JE_TILE, 0, h->stream>>>(wsp, bt);
            RTN_CHECK_LAUNCH(h, "jenc_bits_kernel");
            jenc_scan_kernel<<<bt.n, JE_SCAN_THREADS, 0, h->stream>>>(wsp, status + i0, lengths, bt);
            RTN_CHECK_LAUNCH(h, "jenc_scan_kernel");
            jenc_pack_kernel<<<grid, JE_TILE, 0, h->stream>>>(wsp, status + i0, bt);
            RTN_CHECK_LAUNCH(h, "jenc_pack_kernel");
            jenc_assemble_kernel<<<bt.n, JE_SCAN_THREADS, 0, h->stream>>>(wsp, status + i0, lengths, bt);
            RTN_CHECK_LAUNCH(h, "jenc_assemble_kernel");
            return RTN_OK;
        });
}
