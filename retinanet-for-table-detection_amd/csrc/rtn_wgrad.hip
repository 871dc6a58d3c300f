// rtn_wgrad.hip — the general weight gradient of the training step (RetinaNet.py:125-131,280: Keras compile + fit_generator =>
// TF autodiff of every conv):
//
//   rtn_conv2d_wgrad[_bias | _rowinfo | _prepared]   dW[n][(kh,kw,c)] += sum_pixels dY[pix][n] * X[tap(pix,kh,kw)][c]   (Conv2DBackpropFilter)
//   rtn_wgrad_finish                                 the ordered reduction of the pixel splits (also of rtn_wgrad_win.hip)
//
// wgrad on MFMA: the reduction runs over PIXELS, so both operands are needed pixel-major per lane while memory is
// channel-major.  Tiles [64 pixels][16 x 16-byte chunks] are staged as they lie in memory (range-checked buffer loads:
// padding taps and tail pixels read zeros) and the fragments are read TRANSPOSED with ds_read_b64_tr_b16 (gfx950): one
// read hands a lane 4 consecutive pixels of its channel.  Rows are padded to 288 B and rows 8..15 of every 16 swap
// their 128-byte halves, which makes the transposed reads of a 32-lane half conflict-free.  The pixel range is split
// over gridDim.y; partial tiles are added into the f32 gradient with global_atomic_add_f32.
#include "rtn_internal.h"
#include "rtn_device.h"
#include <algorithm>

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;

constexpr unsigned OOB_OFFSET = 0xFFFFFF00u;
constexpr int WG_ROWB = 288;                 // LDS bytes per pixel row (256 B of channels + 32 B pad)
constexpr int WG_TILE_B = 64 * WG_ROWB;      // one operand tile

struct WGroup {
    const char* x;
    const char* dy;
    unsigned x_bytes, dy_bytes;
    long long x_img_stride_b, dy_img_stride_b, dy_off_b;
    int x_row_stride_b;
    int Hin, Win, Hout, Wout;
    int M;
    int tile_begin;      // first 64-pixel tile of the group
};

struct WParams {
    WGroup g[RTN_MAX_GROUPS];
    float* dW;
    float* db;           // optional bias gradient (BiasAddGrad fused: column sums of dY), accumulated by the tile_k == 0 blocks
    float* slab;         // not null: every pixel split stores its tile into slab[split][N][Ktot] (plain stores) and wgrad_finish adds the
    float* bslab;        // splits in order into dW / db - no atomics, the same bits on every run; bslab[split][N] for the bias sums
    int db_n;            // valid bias entries
    const uint4* rowinfo;
    int ngroups, total_tiles, tiles_per_split, ntiles_k;
    int out_tiles, xcd_map;   // xcd_map: 1-D grid, the output tiles of one pixel split share an XCD (its L2)
    int N, Ktot;
    int cshift, crun_mask, kw_inv, KW;
    int pix_stride_b, sy, sx, pad_t, pad_l, dy_ld_b;
};

// per output pixel: {byte offset of tap (0,0) in X (mod 2^32), byte offset of the dY row, iy0 | ix0 << 16, -}
template <int ES>
__global__ __launch_bounds__(256) void wgrad_rowinfo_kernel(const WParams p, uint4* __restrict__ info) {
    const long long total = (long long)p.total_tiles * 64;
    for (long long R = (long long)blockIdx.x * blockDim.x + threadIdx.x; R < total; R += (long long)gridDim.x * blockDim.x) {
        const int tile = (int)(R >> 6);
        int gi = 0;
        for (int i = 1; i < RTN_MAX_GROUPS; ++i)
            if (i < p.ngroups && tile >= p.g[i].tile_begin) gi = i;
        const WGroup& G = p.g[gi];
        const int m = (int)(R - (long long)G.tile_begin * 64);
        uint4 o = make_uint4(0u, OOB_OFFSET, 0x00008000u, 0u);          // iy0 = -32768: every tap out of range
        if (m < G.M) {
            const int cells = G.Hout * G.Wout;
            const int b = m / cells;
            const int cell = m - b * cells;
            const int oy = cell / G.Wout, ox = cell - oy * G.Wout;
            const int iy0 = oy * p.sy - p.pad_t, ix0 = ox * p.sx - p.pad_l;
            o.x = (unsigned)((long long)b * G.x_img_stride_b + (long long)iy0 * G.x_row_stride_b + (long long)ix0 * p.pix_stride_b);
            o.y = (unsigned)((long long)b * G.dy_img_stride_b + G.dy_off_b + (long long)cell * p.dy_ld_b);
            o.z = ((unsigned)iy0 & 0xffffu) | ((unsigned)ix0 << 16);
        }
        info[R] = o;
    }
}

// One 64-pixel step of the MFMA loop: transposed fragment reads of the dY tile (A) and the X tile (B) of one LDS buffer.
template <int ES, int FI, int WT>
__device__ __forceinline__ void wgrad_step(const char* A, const char* B, int lane, int wm, int wn, f32x4 (&acc)[FI][FI]) {
    if constexpr (ES == 2) {
        const int g = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3;
        const int swz = (g & 1) << 3;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int row = 32 * s + 8 * g + q;
            s16x8 af[FI], bf[FI];
#pragma unroll
            for (int i = 0; i < FI; ++i) {
                const int ca = (wm * WT + 16 * i + 4 * pp) * 2;       // byte column inside the 256-byte row
                const int aoff = row * WG_ROWB + ((((ca >> 4) ^ swz)) << 4) + (ca & 15);
                const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(A + aoff));
                const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(A + aoff + 4 * WG_ROWB));
                af[i] = (s16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                const int cb = (wn * WT + 16 * i + 4 * pp) * 2;
                const int boff = row * WG_ROWB + ((((cb >> 4) ^ swz)) << 4) + (cb & 15);
                const s16x4 lo2 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(B + boff));
                const s16x4 hi2 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(B + boff + 4 * WG_ROWB));
                bf[i] = (s16x8){lo2[0], lo2[1], lo2[2], lo2[3], hi2[0], hi2[1], hi2[2], hi2[3]};
            }
#pragma unroll
            for (int i = 0; i < FI; ++i)
#pragma unroll
                for (int j = 0; j < FI; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[i]),
                                                                        __builtin_bit_cast(bf16x8, bf[j]), acc[i][j], 0, 0, 0);
        }
    } else {
        const int li = lane & 15, kq = lane >> 4;
#pragma unroll 4
        for (int s = 0; s < 16; ++s) {
            const int row = 4 * s + kq;
            const int swz = ((row >> 3) & 1) << 3;
            float af[FI], bf[FI];
#pragma unroll
            for (int i = 0; i < FI; ++i) {
                const int ca = (wm * WT + 16 * i + li) * 4;
                af[i] = *reinterpret_cast<const float*>(A + row * WG_ROWB + (((ca >> 4) ^ swz) << 4) + (ca & 15));
                const int cb = (wn * WT + 16 * i + li) * 4;
                bf[i] = *reinterpret_cast<const float*>(B + row * WG_ROWB + (((cb >> 4) ^ swz) << 4) + (cb & 15));
            }
#pragma unroll
            for (int i = 0; i < FI; ++i)
#pragma unroll
                for (int j = 0; j < FI; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
    }
}

// Loads run TWO pixel tiles ahead of the MFMAs (two register sets: the tile staged into LDS at the end of a step was
// requested a whole step earlier).  Workgroups that read the same pixel range (all output tiles of one split) are placed
// on one XCD (p.xcd_map) so they share its L2.  Knob-ablated on the batch-16 training step (wgrad ~13.5 ms of 38.7):
// operand loads ~5-9 ms, MFMA + transposed reads ~0.7-4 ms (hidden behind the loads), float atomics 1.9 ms - every one of the
// (N/128)*(K/128) output tiles re-reads all pixels (6.4 GB of L2->LDS traffic per head layer at 65 FLOP/B), which is what
// bounds this kernel.
template <int ES>
__global__ __launch_bounds__(256, 2) void conv_wgrad_kernel(const WParams p) {
    constexpr int CE = 16 / ES;                // elements per 16-byte chunk
    constexpr int CH = 16 * CE;                // channels per tile side: 128 (bf16) / 64 (f32)
    constexpr int WT = CH / 2;                 // per-wave extent
    constexpr int FI = WT / 16;                // 16x16 MFMA tiles per wave side: 4 / 2
    __shared__ __attribute__((aligned(16))) char lds[4 * WG_TILE_B];   // [buf][dY | X]

    int otile, split;
    if (p.xcd_map) {                           // 1-D grid; gridDim.x = out_tiles * nsplit, nsplit a multiple of 8
        const int L = blockIdx.x, xcd = L & 7, j = L >> 3;
        const int sl = j / p.out_tiles;
        otile = j - sl * p.out_tiles;
        split = sl * 8 + xcd;
    } else {
        otile = blockIdx.x;
        split = blockIdx.y;
    }
    const int tile_n = otile / p.ntiles_k;
    const int tile_k = otile - tile_n * p.ntiles_k;
    const int n0 = tile_n * CH, k0 = tile_k * CH;
    const int tlo = split * p.tiles_per_split;
    int thi = tlo + p.tiles_per_split;
    thi = thi < p.total_tiles ? thi : p.total_tiles;
    if (tlo >= thi) return;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int ch = t & 15, r0 = t >> 4;
    const int st_off = r0 * WG_ROWB + ((ch ^ (((r0 >> 3) & 1) << 3)) << 4);

    // this thread's X chunk: fixed tap and channel offset for the whole kernel
    const int kk = k0 + ch * CE;
    const bool kvalid = kk < p.Ktot;
    const int kpos = kk >> p.cshift;
    const int coff = kk & p.crun_mask;
    const int kh = (kpos * p.kw_inv) >> 16;
    const int kw = kpos - kh * p.KW;
    const int nn = n0 + ch * CE;
    const bool nvalid = nn < p.N;
    const unsigned dyo = (unsigned)(nn * ES);

    const int wm = wave >> 1, wn = wave & 1;
    f32x4 acc[FI][FI];
#pragma unroll
    for (int i = 0; i < FI; ++i)
#pragma unroll
        for (int j = 0; j < FI; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const bool do_bias = p.db != nullptr && tile_k == 0;
    float bsum[CE];
#pragma unroll
    for (int j = 0; j < CE; ++j) bsum[j] = 0.f;
    uint4 ra0[4], rb0[4], ra1[4], rb1[4];
    uint4 ri[4];                                  // row info of the NEXT tile to load (prefetched one load ahead)
#define WG_ROWINFO(TILE)                                                                                            \
    {                                                                                                               \
        const int tt_ = (TILE) < thi ? (TILE) : thi - 1;                                                            \
        _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_) ri[i_] = p.rowinfo[(long long)tt_ * 64 + r0 + 16 * i_];    \
    }
#define WG_LOAD(TILE, RA, RB)                                                                                       \
    {                                                                                                               \
        int gi_ = 0;                                                                                                \
        _Pragma("unroll") for (int i_ = 1; i_ < RTN_MAX_GROUPS; ++i_)                                               \
            if (i_ < p.ngroups && (TILE) >= p.g[i_].tile_begin) gi_ = i_;                                           \
        const WGroup& G_ = p.g[gi_];                                                                                \
        const __amdgpu_buffer_rsrc_t xs_ = __builtin_amdgcn_make_buffer_rsrc(                                       \
            (void*)G_.x, 0, (int)__builtin_amdgcn_readfirstlane((int)G_.x_bytes), 0x00020000);                      \
        const __amdgpu_buffer_rsrc_t ys_ = __builtin_amdgcn_make_buffer_rsrc(                                       \
            (void*)G_.dy, 0, (int)__builtin_amdgcn_readfirstlane((int)G_.dy_bytes), 0x00020000);                    \
        const unsigned delta_ = (unsigned)(kh * G_.x_row_stride_b + kw * p.pix_stride_b + coff * ES);               \
        const int Hin_ = G_.Hin, Win_ = G_.Win;                                                                     \
        _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_) {                                                          \
            const int iy_ = (int)(short)(ri[i_].z & 0xffffu) + kh, ix_ = (int)(short)(ri[i_].z >> 16) + kw;         \
            const bool ok_ = kvalid && (unsigned)iy_ < (unsigned)Hin_ && (unsigned)ix_ < (unsigned)Win_;            \
            RB[i_] = buffer_load16(xs_, ok_ ? ri[i_].x + delta_ : OOB_OFFSET);                                      \
            RA[i_] = buffer_load16(ys_, (nvalid && ri[i_].y != OOB_OFFSET) ? ri[i_].y + dyo : OOB_OFFSET);          \
        }                                                                                                           \
        WG_ROWINFO((TILE) + 1);                                                                                     \
    }
#define WG_STORE(BUF, RA, RB)                                                                                       \
    {                                                                                                               \
        if (do_bias) {                                                                                              \
            _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_) {                                                      \
                const unsigned w4_[4] = {RA[i_].x, RA[i_].y, RA[i_].z, RA[i_].w};                                   \
                if constexpr (ES == 2) {                                                                            \
                    _Pragma("unroll") for (int j_ = 0; j_ < 4; ++j_) {                                              \
                        bsum[2 * j_] += __uint_as_float(w4_[j_] << 16);                                             \
                        bsum[2 * j_ + 1] += __uint_as_float(w4_[j_] & 0xffff0000u);                                 \
                    }                                                                                               \
                } else {                                                                                            \
                    _Pragma("unroll") for (int j_ = 0; j_ < 4; ++j_) bsum[j_] += __uint_as_float(w4_[j_]);          \
                }                                                                                                   \
            }                                                                                                       \
        }                                                                                                           \
        char* A_ = lds + (BUF) * 2 * WG_TILE_B;                                                                     \
        _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_) {                                                          \
            *reinterpret_cast<uint4*>(A_ + st_off + i_ * 16 * WG_ROWB) = RA[i_];                                    \
            *reinterpret_cast<uint4*>(A_ + WG_TILE_B + st_off + i_ * 16 * WG_ROWB) = RB[i_];                        \
        }                                                                                                           \
    }

    WG_ROWINFO(tlo);
    WG_LOAD(tlo, ra0, rb0);
    WG_STORE(0, ra0, rb0);
    if (tlo + 1 < thi) WG_LOAD(tlo + 1, ra1, rb1);
    __syncthreads();
    int cur = 0;
#pragma unroll 1
    for (int tile = tlo; tile < thi; tile += 2) {
        // LDS[cur] = tile, set 1 = tile+1 (requested a step ago); request tile+2 into set 0
        if (tile + 2 < thi) WG_LOAD(tile + 2, ra0, rb0);
        wgrad_step<ES, FI, WT>(lds + cur * 2 * WG_TILE_B, lds + cur * 2 * WG_TILE_B + WG_TILE_B, lane, wm, wn, acc);
        if (tile + 1 < thi) WG_STORE(cur ^ 1, ra1, rb1);
        __syncthreads();
        cur ^= 1;
        if (tile + 1 >= thi) break;
        // LDS[cur] = tile+1, set 0 = tile+2; request tile+3 into set 1
        if (tile + 3 < thi) WG_LOAD(tile + 3, ra1, rb1);
        wgrad_step<ES, FI, WT>(lds + cur * 2 * WG_TILE_B, lds + cur * 2 * WG_TILE_B + WG_TILE_B, lane, wm, wn, acc);
        if (tile + 2 < thi) WG_STORE(cur ^ 1, ra0, rb0);
        __syncthreads();
        cur ^= 1;
    }
#undef WG_LOAD
#undef WG_ROWINFO
#undef WG_STORE

    if (do_bias) {       // threads t = ch + 16*r0 share chunk column ch: sum their partials through LDS, one atomic per channel
        float* sb = reinterpret_cast<float*>(lds);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < CE; ++j) sb[t * CE + j] = bsum[j];
        __syncthreads();
        if (t < 16) {
#pragma unroll
            for (int j = 0; j < CE; ++j) {
                float v = 0.f;
                for (int rr = 0; rr < 16; ++rr) v += sb[(t + 16 * rr) * CE + j];
                const int n = n0 + t * CE + j;
                if (n < p.db_n) { if (p.slab) p.bslab[(long long)split * p.N + n] = v; else unsafeAtomicAdd(p.db + n, v); }
            }
        }
    }
    // D[row = n][col = k]: lane holds rows 4*(lane>>4)+r, column lane&15 of each 16x16 tile.  The tile goes through this wave's
    // LDS slice so that every atomic wave-instruction adds WT consecutive k of ONE filter row (256 contiguous bytes for bf16:
    // the shape the memory-side atomic units run at full rate; straight from the accumulators it was 4 x 64 B).
    const int lr = (lane >> 4) * 4, lc = lane & 15;
    constexpr int SP = WT + 1;                                   // padded row of the staging slice (floats)
    __syncthreads();                                             // every wave is done with the operand tiles
    float* S = reinterpret_cast<float*>(lds) + wave * (WT * SP);
#pragma unroll
    for (int i = 0; i < FI; ++i)
#pragma unroll
        for (int j = 0; j < FI; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) S[(16 * i + lr + r) * SP + 16 * j + lc] = acc[i][j][r];
    __builtin_amdgcn_s_waitcnt(0xC07F);                          // this wave's LDS writes have landed (slice is wave-private)
    if (lane < WT) {
        const int kc = k0 + wn * WT + lane;
        if (kc < p.Ktot) {
#pragma unroll 4
            for (int nl = 0; nl < WT; ++nl) {
                const int n = n0 + wm * WT + nl;
                if (n < p.N) {
                    if (p.slab) p.slab[((long long)split * p.N + n) * p.Ktot + kc] = S[nl * SP + lane];
                    else unsafeAtomicAdd(p.dW + (long long)n * p.Ktot + kc, S[nl * SP + lane]);
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ 256 x 256, LDS-DMA (bf16)
// The loop above is bound by the L2->LDS volume of its operand loads (65 FLOP/B).  This variant owns a 256 (n) x 256 (k) tile
// with 8 waves (4 x 2, wave tile 64 x 128): 64 KB per 64-pixel step for 8.4 MFLOP, half the volume per FLOP, and stages it by
// LDS-DMA (no staging registers beside 128 accumulator registers; the next step's 64 KB is in flight while this one multiplies).
// LDS image: [64 px][512 B] per operand, UNPADDED (a DMA piece is 1 KiB = 2 rows, lane-linear); the transposed reads stay
// conflict-free through an XOR on the 32-byte granule index with key(row) = (row & 3) | ((row >> 3) & 1) << 2: the 32 lanes
// of a half-wave read 8 rows (q = 0..3, two values of g) x one granule each, 8 distinct keys -> 8 x 8 = 64 banks.  The key
// of the rows a lane stages does not change from piece to piece, so each lane still has ONE source chunk (tap, channel offset).
// NWN x NWK waves, wave tile 64 (n) x 16*FJ (k); square tiles only: TS = 64*NWN = 16*FJ*NWK channels per side.
//   <4, 2, 8>: 256 x 256, 512 threads, 128 KB of LDS  (many-pixel layers)
//   <2, 2, 4>: 128 x 128, 256 threads,  64 KB of LDS  (two workgroups per CU)
template <int NWN, int NWK, int FJ>
__global__ __launch_bounds__(64 * NWN * NWK, 2) void conv_wgrad_dma_kernel(const WParams p) {
    constexpr int NW = NWN * NWK;
    constexpr int TS = 64 * NWN;
    static_assert(TS == 16 * FJ * NWK, "square output tile");
    constexpr int WD_ROWB = TS * 2;               // bytes per pixel row of an operand tile
    constexpr int WD_TILE_B = 64 * WD_ROWB;
    constexpr int CPR = WD_ROWB / 16;             // 16-byte chunks per row
    constexpr int RPP = 1024 / WD_ROWB;           // rows per 1-KiB staging piece
    static_assert(RPP * NW == 16 && 64 / (RPP * NW) == 4, "four pieces per wave and operand, 16 rows apart");
    __shared__ __attribute__((aligned(16))) char lds[4 * WD_TILE_B];   // [stage][dY | X]

    int otile, split;
    if (p.xcd_map) {
        const int L = blockIdx.x, xcd = L & 7, j = L >> 3;
        const int sl = j / p.out_tiles;
        otile = j - sl * p.out_tiles;
        split = sl * 8 + xcd;
    } else {
        otile = blockIdx.x;
        split = blockIdx.y;
    }
    const int tile_n = otile / p.ntiles_k;
    const int tile_k = otile - tile_n * p.ntiles_k;
    const int n0 = tile_n * TS, k0 = tile_k * TS;
    const int tlo = split * p.tiles_per_split;
    int thi = tlo + p.tiles_per_split;
    thi = thi < p.total_tiles ? thi : p.total_tiles;
    if (tlo >= thi) return;

    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    // ---- staging role: piece i of this wave = rows RPP*(wave + NW*i) + lane / CPR, LDS chunk position lane % CPR
    const int rsub = lane / CPR;
    const int srow0 = RPP * wave + rsub;                       // + 16 i
    const int skey = (srow0 & 3) | (((srow0 >> 3) & 1) << 2);  // the same for every i (+16 keeps row & 3 and bit 3)
    const int sc = (lane % CPR) ^ (skey << 1);                 // source chunk (8 elements) this lane fetches
    const int kk = k0 + sc * 8;
    const bool kvalid = kk < p.Ktot;
    const int kpos = kk >> p.cshift;
    const int coff = kk & p.crun_mask;
    const int kh = (kpos * p.kw_inv) >> 16;
    const int kw = kpos - kh * p.KW;
    const int nn = n0 + sc * 8;
    const bool nvalid = nn < p.N;
    const unsigned dyo = (unsigned)(nn * 2);
    const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) char*)lds;

    const int wm = wave / NWK, wn = wave % NWK;
    f32x4 acc[4][FJ];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < FJ; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const bool do_bias = p.db != nullptr && tile_k == 0 && wn == 0;
    float bsum[4] = {0.f, 0.f, 0.f, 0.f};

    uint4 ri[4];
#define WD_ROWINFO(TILE)                                                                                            \
    {                                                                                                               \
        const int tt_ = (TILE) < thi ? (TILE) : thi - 1;                                                            \
        _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_) ri[i_] = p.rowinfo[(long long)tt_ * 64 + srow0 + 16 * i_]; \
    }
#define WD_STAGE(TILE, STG)                                                                                         \
    {                                                                                                               \
        int gi_ = 0;                                                                                                \
        _Pragma("unroll") for (int i_ = 1; i_ < RTN_MAX_GROUPS; ++i_)                                               \
            if (i_ < p.ngroups && (TILE) >= p.g[i_].tile_begin) gi_ = i_;                                           \
        const WGroup& G_ = p.g[gi_];                                                                                \
        const i32x4 xs_ = make_srd(G_.x, G_.x_bytes);                                                               \
        const i32x4 ys_ = make_srd(G_.dy, G_.dy_bytes);                                                             \
        const unsigned delta_ = (unsigned)(kh * G_.x_row_stride_b + kw * p.pix_stride_b + coff * 2);                \
        const int Hin_ = G_.Hin, Win_ = G_.Win;                                                                     \
        _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_) {                                                          \
            const int iy_ = (int)(short)(ri[i_].z & 0xffffu) + kh, ix_ = (int)(short)(ri[i_].z >> 16) + kw;         \
            const bool ok_ = kvalid && (unsigned)iy_ < (unsigned)Hin_ && (unsigned)ix_ < (unsigned)Win_;            \
            const unsigned piece_ = (unsigned)((wave + NW * i_) * 1024);                                             \
            dma16(ys_, (nvalid && ri[i_].y != OOB_OFFSET) ? ri[i_].y + dyo : OOB_OFFSET,                            \
                  lds_base + (unsigned)((STG) * 2 * WD_TILE_B) + piece_);                                           \
            dma16(xs_, ok_ ? ri[i_].x + delta_ : OOB_OFFSET,                                                        \
                  lds_base + (unsigned)((STG) * 2 * WD_TILE_B + WD_TILE_B) + piece_);                               \
        }                                                                                                           \
    }

    WD_ROWINFO(tlo);
    WD_STAGE(tlo, 0);
    WD_ROWINFO(tlo + 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const int g = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3;
    const int rkey = q | ((g & 1) << 2);
    int cur = 0;
#pragma unroll 1
    for (int tile = tlo; tile < thi; ++tile) {
        const char* A = lds + cur * 2 * WD_TILE_B;     // dY tile
        const char* B = A + WD_TILE_B;                 // X tile
        // the tile's first A fragments are requested before the next tile's staging is issued (as in the forward kernels)
        s16x8 af0[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int ca = (wm * 64 + 16 * i + 4 * pp) * 2;
            const int aoff = (8 * g + q) * WD_ROWB + (((ca >> 5) ^ rkey) << 5) + (ca & 31);
            const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(A + aoff));
            const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(A + aoff + 4 * WD_ROWB));
            af0[i] = (s16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        }
        if (tile + 1 < thi) {
            WD_STAGE(tile + 1, cur ^ 1);
            WD_ROWINFO(tile + 2);
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int row = 32 * s + 8 * g + q;
            s16x8 af[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (s == 0) { af[i] = af0[i]; continue; }
                const int ca = (wm * 64 + 16 * i + 4 * pp) * 2;            // byte column inside the 512-byte row
                const int aoff = row * WD_ROWB + (((ca >> 5) ^ rkey) << 5) + (ca & 31);
                const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(A + aoff));
                const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(A + aoff + 4 * WD_ROWB));
                af[i] = (s16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            }
            if (do_bias) {                              // BiasAddGrad: the A fragment of lane (m, kq) holds 8 pixels of channel m
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int e = 0; e < 8; ++e) bsum[i] += __uint_as_float(((unsigned)(unsigned short)af[i][e]) << 16);
            }
#pragma unroll
            for (int jh = 0; jh < FJ; jh += 4) {
                s16x8 bf[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int cb = (wn * 16 * FJ + 16 * (jh + j) + 4 * pp) * 2;
                    const int boff = row * WD_ROWB + (((cb >> 5) ^ rkey) << 5) + (cb & 31);
                    const s16x4 lo2 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(B + boff));
                    const s16x4 hi2 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(B + boff + 4 * WD_ROWB));
                    bf[j] = (s16x8){lo2[0], lo2[1], lo2[2], lo2[3], hi2[0], hi2[1], hi2[2], hi2[3]};
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc[i][jh + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[i]),
                                                                                 __builtin_bit_cast(bf16x8, bf[j]), acc[i][jh + j], 0, 0, 0);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the next stage (and the row info behind it) has landed
        __syncthreads();
        cur ^= 1;
    }
#undef WD_STAGE
#undef WD_ROWINFO

    const int lr = (lane >> 4) * 4, lc = lane & 15;
    if (do_bias) {       // lane (m = lane & 15, kq = lane >> 4): fold the four pixel groups, lanes 0..15 add channel m
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float v = bsum[i];
            v += __shfl_xor(v, 16, 64);
            v += __shfl_xor(v, 32, 64);
            const int n = n0 + wm * 64 + 16 * i + lc;
            if (lane < 16 && n < p.db_n) { if (p.slab) p.bslab[(long long)split * p.N + n] = v; else unsafeAtomicAdd(p.db + n, v); }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < FJ; ++j) {
            const int kc = k0 + wn * 16 * FJ + 16 * j + lc;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = n0 + wm * 64 + 16 * i + lr + r;
                if (n < p.N && kc < p.Ktot) {
                    if (p.slab) p.slab[((long long)split * p.N + n) * p.Ktot + kc] = acc[i][j][r];
                    else unsafeAtomicAdd(p.dW + (long long)n * p.Ktot + kc, acc[i][j][r]);
                }
            }
        }
}

// (A ring-of-four variant of the 256 x 256 kernel - 32-pixel stages, one counted wait per iteration, row info through scalar loads -
// was built in round 3, bit-identical and 1-16 % slower on every layer (profiles/r3_wgrad_ring_ab.txt, r3_wgrad_ring128_ab.txt: the loop
// is bound by instruction issue, not by the latency its vmcnt(0) exposes); removed in round 4.)

// ------------------------------------------------------------------------------------------------ ordered reduction of the pixel splits
// dW[i] += slab[0][i] + slab[1][i] + ... + slab[S-1][i] with a FIXED association: the S splits are cut into SL consecutive ranges, every
// range is summed in order by one "split lane" (SL lanes x 256 / SL float4 columns per block), and the SL partial sums are added in
// lane order.  Same bits on every run; SL only spreads the loads of a many-split, few-weights layer (res2: 256 splits x 16 K weights)
// over enough threads.  Blocks past `main_blocks` do the same for the bias slabs (scalar columns).
template <int SL>
__global__ __launch_bounds__(256) void wgrad_finish_kernel(float* __restrict__ dW, const float* __restrict__ slab, int S, long long NK,
                                                           float* __restrict__ db, const float* __restrict__ bslab, int N, int db_n, int main_blocks,
                                                           int bS, rtn_wgrad_frag_t fr) {
    constexpr int CB = 256 / SL;
    __shared__ float4 part[SL][CB];
    const int c = threadIdx.x % CB, sl = threadIdx.x / CB;
    const bool is_main = (int)blockIdx.x < main_blocks;
    const int Sx = is_main ? S : bS;                      // the bias slabs may come in a different number of parts (rtn_wgrad_win.hip)
    const int per = (Sx + SL - 1) / SL;
    const int s0 = sl * per < Sx ? sl * per : Sx, s1 = s0 + per < Sx ? s0 + per : Sx;
    if (is_main) {
        const long long i = (long long)blockIdx.x * CB + c;          // float4 column
        const bool live = i < NK / 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (live)
#pragma unroll 8
            for (int s = s0; s < s1; ++s) {                               // (unrolled: the loads of eight splits in flight, the sums in the same order)
                const float4 a = reinterpret_cast<const float4*>(slab + (size_t)s * NK)[i];
                v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
            }
        part[sl][c] = v;
        __syncthreads();
        if (sl == 0 && live) {
#pragma unroll
            for (int l = 1; l < SL; ++l) { const float4 a = part[l][c]; v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w; }
            if (fr.ncb > 0) {
                // slabs in accumulator-fragment order (rtn_wgrad_win.hip): float4 i = [tile][wave][tap j][i4][lane] holds rows
                // n .. n + 3 of ONE column: n = co_tile tn + 64 wm + 16 i4 + 4 (lane / 16), k = j C + 64 cb + 16 wk + lane % 16
                const int lane = (int)(i & 63);
                const unsigned f = (unsigned)(i >> 6);                  // NK < 2^32
                const int i4 = (int)(f & 3);
                const unsigned t2 = f >> 2, t3 = t2 / 9u;
                const int j = (int)(t2 - t3 * 9u);
                const int tile = (int)(t3 / (unsigned)fr.wpt), wave = (int)t3 - tile * fr.wpt;
                const int tn = tile / fr.ncb, cb = tile - tn * fr.ncb;
                const int n = fr.co_tile * tn + 64 * (wave >> 2) + 16 * i4 + 4 * (lane >> 4);
                const int k = j * fr.C + 64 * cb + 16 * (wave & 3) + (lane & 15);
                float* o = dW + (size_t)n * fr.Ktot + k;
                o[0] += v.x; o[fr.Ktot] += v.y; o[2 * (size_t)fr.Ktot] += v.z; o[3 * (size_t)fr.Ktot] += v.w;
            } else {
                float4 w = reinterpret_cast<float4*>(dW)[i];
                w.x += v.x; w.y += v.y; w.z += v.z; w.w += v.w;
                reinterpret_cast<float4*>(dW)[i] = w;
            }
        }
    } else {
        const int n = ((int)blockIdx.x - main_blocks) * CB + c;
        const bool live = n < db_n;
        float v = 0.f;
        if (live)
            for (int s = s0; s < s1; ++s) v += bslab[(size_t)s * N + n];
        part[sl][c].x = v;
        __syncthreads();
        if (sl == 0 && live) {
#pragma unroll
            for (int l = 1; l < SL; ++l) v += part[l][c].x;
            db[n] += v;
        }
    }
}

}  // namespace

// (rtn_wgrad_halo.hip, the one-kernel-row-per-tile 3x3 kernel of round 2, lost every layer of the benchmark shapes to the window
// kernel and left the library in round 4: profiles/r2_v3_ab_wgrad_halo.txt, r3_wgrad_win_ab.txt.)

// dW[0..NK) += slab[0] + slab[1] + ... + slab[S-1] (in that order), db[0..db_n) likewise from bslab[S][N]: the ordered reduction
// of the pixel splits of every weight-gradient kernel
int rtn_wgrad_finish(rtn_handle_t h, float* dW, const float* slab, int S, long long NK, float* db, const float* bslab, int N, int db_n, int bS,
                     const rtn_wgrad_frag_t* frag) {
    if (!dW || !slab || S < 1 || NK < 4 || NK % 4) return rtn_fail(h, RTN_EINVAL, "wgrad finish: bad argument");
    const int nb = db ? db_n : 0;
    if (bS < 1) bS = S;
    rtn_wgrad_frag_t fr = {0, 0, 0, 8, 128};
    if (frag) fr = *frag;
#define RTN_WF(SL_)                                                                                               \
    do {                                                                                                          \
        const long long mb = (NK / 4 + 256 / SL_ - 1) / (256 / SL_);                                              \
        const long long bb = (nb + 256 / SL_ - 1) / (256 / SL_);                                                  \
        hipLaunchKernelGGL((wgrad_finish_kernel<SL_>), dim3((unsigned)(mb + bb)), dim3(256), 0, h->stream, dW, slab, S, NK, db, bslab, N, nb, (int)mb, bS, fr); \
    } while (0)
    if (S >= 64) RTN_WF(16); else if (S >= 16) RTN_WF(8); else if (S >= 8) RTN_WF(4); else RTN_WF(1);
#undef RTN_WF
    RTN_CHECK_LAUNCH(h, "wgrad_finish_kernel");
    return RTN_OK;
}

// ---- the wgrad launcher: check the descriptor -> plan -> try the window kernel -> check the groups and fill WParams -> launch the
// row-info kernel and / or the main kernel -> finish.  The sizing call (rtn_conv2d_wgrad_workspace_bytes) reads the same plan.
namespace {

// Which general kernel runs a layer, how its pixels are split, and the layout of the workspace the three weight-gradient kernels
// share: the row-info table (16 B per pixel of the 64-pixel tiles), then, from `table_bytes` on, EITHER the per-split slabs of the
// general kernels' ordered reduction OR the slabs of the nine-tap window kernel (rtn_wgrad_win.hip) - behind the table, so that a
// table built once by rtn_conv2d_wgrad_rowinfo stays valid whichever kernel later prepared calls select.  Computed here and nowhere
// else, for the launch and for the sizing call (which has no handle: the 256 CUs of an MI355X).
struct WgradPlan {
    bool dma, dma_small, xcd_map;
    int CH;
    long long tiles, out_tiles, nsplit, nsplit_used;     // tiles: the 64-pixel tiles of all groups
    int tiles_per_split;
    int tile_begin[RTN_MAX_GROUPS];                      // first 64-pixel tile of each group
    size_t table_min;       // the table as it is: the least a launch accepts (no room for slabs: float atomics)
    size_t table_bytes;     // ... rounded up to 256 B: where the slabs start
    size_t slab_bytes;      // nsplit_used x ([N][Ktot] + [N]) floats of the general kernels
    bool slab_on;           // RTN_WGRAD_SLAB=0: never use them
    size_t win_bytes;       // > 0: the window kernel takes the layer (wgrad_takes_win), with this many bytes of slabs
    size_t workspace_bytes() const { return table_bytes + std::max(slab_on ? slab_bytes : 0, win_bytes); }
};

// rtn_wgrad_win.hip (all nine taps per output tile over a sliding window of the input; stride-1 3x3 layers with whole blocks of 128
// filters and 64 channels, image rows of up to 254 pixels) against the kernels above, measured per shape at batch 8 (tools/ab_wgrad.py,
// profiles/r3_wgrad_win_ab.txt): head towers 0.197 vs 0.285 ms, P3 0.157 vs 0.216, res4 branch2b / P4 0.068 vs 0.076, res3 branch2b
// 0.065 vs 0.068, res5 branch2b 0.071 vs 0.087, but P5 (8,400 pixels x 8 output tiles = 64 workgroups) 0.048 vs 0.042: it takes the
// layers with enough work for a chip-wide grid, 64-pixel tiles x output tiles >= 3000 (res5 4,192, res4 4,200, P5 1,048).
// RTN_WGRAD_WIN=1: wherever the shape allows (tests, A/B), 0: never.  Returns the bytes of its slabs, 0 when it does not take the layer.
size_t wgrad_takes_win(const rtn_conv_desc_t* d, long long tiles) {
    const int knob = rtn_env_int("RTN_WGRAD_WIN", -1);
    const size_t bytes = knob == 0 ? 0 : rtn_wgrad_win_workspace_bytes(d);
    if (bytes == 0 || knob > 0) return bytes;
    // (the 64-filter form, res2 branch2b and the head outputs: half the work per tile)
    return tiles * (long long)(d->N == 64 ? 1 : 2 * (d->N / 128)) * (d->Crun / 64) >= 6000 ? bytes : 0;
}

WgradPlan wgrad_plan(const rtn_conv_desc_t* d, int cus) {
    WgradPlan w;
    const int es = rtn_dtype_size(d->dtype);
    const long long Ktot = (long long)d->KH * d->KW * d->Crun;
    w.tiles = 0;
    for (int i = 0; i < d->ngroups; ++i) {
        w.tile_begin[i] = (int)w.tiles;
        w.tiles += ((long long)d->g[i].Hout * d->g[i].Wout * d->batch + 63) / 64;
    }
    // bf16 layers with more than 128 filters and at least one 256-wide K tile: the 256 x 256 LDS-DMA kernel (RTN_WGRAD_DMA=0: off)
    // Measured per layer (tools/profile_train.py, batch 16): -27 % on the head layers (5575 pixel tiles, 0.71 -> 0.52 ms) and
    // -21 % on P3, but +25..40 % on the layers with ~1000 pixel tiles or fewer (res4/res5, C4/C5, P5, P6: short loops, and each
    // workgroup ends with 128 accumulator registers of output), hence the pixel-count condition.
    w.dma = es == 2 && d->N > 128 && Ktot >= 256 && w.tiles >= 2048;
    const int dma_env = rtn_env_int("RTN_WGRAD_DMA", -1);       // 0: never; 2: wherever the shape allows (tests, A/B); -1: unset
    if (dma_env >= 0) w.dma = dma_env == 2 ? (es == 2 && d->N > 128 && Ktot >= 256) : (w.dma && dma_env != 0);
    // the same staging on the 128 x 128 tile for the other bf16 layers with whole 128-wide tiles (RTN_WGRAD_DMA_SMALL=0: register-staged kernel)
    w.dma_small = !w.dma && es == 2;                       // measured: train step 37.4 -> 36.8 ms against the register-staged kernel
    if (rtn_env_int("RTN_WGRAD_DMA_SMALL", 1) == 0 || dma_env == 0) w.dma_small = false;
    w.CH = w.dma ? 256 : (es == 2 ? 128 : 64);
    const int ntn = (d->N + w.CH - 1) / w.CH;
    const long long ntk = (Ktot + w.CH - 1) / w.CH;
    w.out_tiles = (long long)ntn * ntk;
    // Workgroup count: whole rounds of the resident slots (two 256-thread workgroups per CU), rounded DOWN - 1044 workgroups
    // on 1024 slots cost a third round (training step 40.8 -> 38.8 ms).  RTN_WGRAD_BLOCKS overrides the target.
    // (A 256 x 256-tile, 512-thread variant of the kernel was built and measured: no faster at equal rounds - the loop is
    // bound by the latency of its register-staged loads, not by MFMA work per byte.)
    const long long slots = (long long)(cus > 0 ? cus : 256) * (w.dma ? 1 : 2);
    // measured (RTN_WGRAD_BLOCKS sweep): one round for both LDS-DMA kernels.  Round 3, 256 x 256 kernel with the slab reduction
    // (profiles/r3_wgrad_blocks_ab.txt): 256 workgroups 0.268 ms against 0.282 with 512 on a head-tower layer, 0.209 / 0.223 on P3 -
    // every split writes a 2.4 MB slab that the finish kernel reads back (PMC: 132 MB written per layer with 56 splits)
    long long target = slots * ((w.dma_small || w.dma) ? 1 : 2);
    { const long long v = rtn_env_int("RTN_WGRAD_BLOCKS", 0); if (v >= 64 && v <= 65536) target = v; }
    long long nsplit = target / w.out_tiles;
    if (nsplit > w.tiles) nsplit = w.tiles;
    if (nsplit < 1) nsplit = 1;
    if (nsplit > 65535) nsplit = 65535;
    w.xcd_map = nsplit >= 8;
    if (w.xcd_map) nsplit &= ~7ll;
    w.tiles_per_split = (int)((w.tiles + nsplit - 1) / nsplit);
    if (w.tiles_per_split < 1) w.tiles_per_split = 1;                           // (a descriptor without pixels: the group checks refuse it)
    w.nsplit_used = (w.tiles + w.tiles_per_split - 1) / w.tiles_per_split;      // splits that own at least one pixel tile
    w.nsplit = w.nsplit_used;
    if (w.xcd_map && (w.nsplit & 7)) w.nsplit = (w.nsplit + 7) & ~7ll;          // the XCD map wants a multiple of 8: the extra splits are empty
    w.table_min = (size_t)w.tiles * 64 * sizeof(uint4);
    w.table_bytes = (w.table_min + 255) & ~(size_t)255;
    w.slab_bytes = (size_t)w.nsplit_used * (size_t)d->N * ((size_t)Ktot + 1) * sizeof(float);
    w.slab_on = rtn_env_int("RTN_WGRAD_SLAB", 1) != 0;
    w.win_bytes = wgrad_takes_win(d, w.tiles);
    return w;
}

// build the row-info table and run / build it only (rtn_conv2d_wgrad_rowinfo) / run on a table built earlier (rtn_conv2d_wgrad_prepared)
enum class WgradMode { TableAndRun, TableOnly, RunPrepared };

struct WgradShape { int es, cshift; long long Ktot, pix_b; };   // what the descriptor checks derive on the way

// Step 1: everything about the call that does not depend on a group's tensors.
int wgrad_check_desc(rtn_handle_t h, const rtn_conv_desc_t* d, const float* dW, const void* workspace, WgradMode mode, WgradShape* sh) {
    if (!d || (!dW && mode != WgradMode::TableOnly) || !workspace) return rtn_fail(h, RTN_EINVAL, "wgrad: null argument");
    if (d->dtype != RTN_BF16 && d->dtype != RTN_F32) return rtn_fail(h, RTN_EINVAL, "wgrad: bad dtype");
    const int es = rtn_dtype_size(d->dtype);
    if (d->ngroups < 1 || d->ngroups > RTN_MAX_GROUPS || d->batch < 1 || d->N < 1) return rtn_fail(h, RTN_EINVAL, "wgrad: bad group/batch/N");
    const int cshift = ilog2_exact(d->Crun);
    if (cshift < 0 || (d->Crun * es) % 16) return rtn_fail(h, RTN_EINVAL, "wgrad: Crun %d", d->Crun);
    const long long Ktot = (long long)d->KH * d->KW * d->Crun;
    if ((Ktot * es) % 16 || Ktot > (1 << 24)) return rtn_fail(h, RTN_EINVAL, "wgrad: K %lld", Ktot);
    if ((d->N * es) % 16 || (d->out_ld * es) % 16) return rtn_fail(h, RTN_EINVAL, "wgrad: N %d / out_ld %d must span whole 16-byte chunks (pad dY)", d->N, d->out_ld);
    if (d->w_rows < d->N) return rtn_fail(h, RTN_EINVAL, "wgrad: w_rows < N");
    if (((uintptr_t)dW & 15) || ((uintptr_t)workspace & 15)) return rtn_fail(h, RTN_EINVAL, "wgrad: dW/workspace alignment");
    const long long pix_b = (long long)d->pix_stride * es;
    if (pix_b % 16 && (d->KW != 1 || (d->sx * pix_b) % 16 || (d->pad_l * pix_b) % 16)) return rtn_fail(h, RTN_EINVAL, "wgrad: unaligned taps");
    *sh = WgradShape{es, cshift, Ktot, pix_b};
    return RTN_OK;
}

// Step 2: the stride-1 3x3 layers the nine-tap window kernel takes (its slabs start behind the row-info table).  RTN_OK: it ran;
// 1: the general kernels run the layer; < 0: error.  (It checks the groups' tensors itself and turns down what it cannot run.)
int wgrad_try_win(rtn_handle_t h, const rtn_conv_desc_t* d, const WgradPlan& w, float* dW, float* db, int db_n, void* workspace,
                  size_t workspace_bytes) {
    if (!w.win_bytes || workspace_bytes <= w.table_bytes) return 1;
    const int rc = rtn_wgrad_win_try(h, d, dW, db, db_n, (char*)workspace + w.table_bytes, workspace_bytes - w.table_bytes);
    if (rc == RTN_OK) h->last_wgrad_impl = 4;
    return rc;
}

// Step 3: the checks of every group's tensors, and the kernel parameters (all but the slab pointers).
int wgrad_fill_params(rtn_handle_t h, const rtn_conv_desc_t* d, const WgradShape& sh, const WgradPlan& w, float* dW, float* db, int db_n,
                      const void* workspace, WParams* pp) {
    WParams& p = *pp;
    memset(&p, 0, sizeof(p));
    const int es = sh.es;
    for (int i = 0; i < d->ngroups; ++i) {
        const rtn_conv_group_t& s = d->g[i];
        WGroup& g = p.g[i];
        if (!s.in || !s.out) return rtn_fail(h, RTN_EINVAL, "wgrad: group %d null x/dY", i);
        if (((uintptr_t)s.in & 15) || ((uintptr_t)s.out & 15)) return rtn_fail(h, RTN_EINVAL, "wgrad: group %d alignment", i);
        if (s.Hin < 1 || s.Win < 1 || s.Hout < 1 || s.Wout < 1 || s.Hout > 32000 || s.Wout > 32000) return rtn_fail(h, RTN_EINVAL, "wgrad: group %d extent", i);
        if ((s.in_img_stride * es) % 16 || ((long long)s.in_row_stride * es) % 16 || (s.out_img_stride * es) % 16 || (s.out_off * es) % 16)
            return rtn_fail(h, RTN_EINVAL, "wgrad: group %d strides not 16-byte multiples", i);
        const long long in_max = (long long)(d->batch - 1) * s.in_img_stride + (long long)(s.Hin - 1) * s.in_row_stride + (long long)(s.Win - 1) * d->pix_stride + d->Crun;
        if (in_max > s.in_elems) return rtn_fail(h, RTN_EBOUNDS, "wgrad: group %d x taps reach %lld of %lld", i, in_max, (long long)s.in_elems);
        const long long cells = (long long)s.Hout * s.Wout;
        const long long dy_max = (long long)(d->batch - 1) * s.out_img_stride + s.out_off + (cells - 1) * d->out_ld + d->N;
        if (s.out_off < 0 || dy_max > s.out_elems) return rtn_fail(h, RTN_EBOUNDS, "wgrad: group %d dY reads reach %lld of %lld", i, dy_max, (long long)s.out_elems);
        if (s.in_elems * es >= (long long)OOB_OFFSET || s.out_elems * es >= (long long)OOB_OFFSET) return rtn_fail(h, RTN_EINVAL, "wgrad: group %d tensor exceeds the 4 GiB descriptor range", i);
        g.x = (const char*)s.in; g.dy = (const char*)s.out;
        g.x_bytes = (unsigned)(s.in_elems * es); g.dy_bytes = (unsigned)(s.out_elems * es);
        g.x_img_stride_b = s.in_img_stride * es;
        g.dy_img_stride_b = s.out_img_stride * es;
        g.dy_off_b = s.out_off * es;
        g.x_row_stride_b = (int)((long long)s.in_row_stride * es);
        g.Hin = s.Hin; g.Win = s.Win; g.Hout = s.Hout; g.Wout = s.Wout;
        g.M = (int)(cells * d->batch);
        g.tile_begin = w.tile_begin[i];
    }
    if (w.tiles > (1 << 24)) return rtn_fail(h, RTN_EINVAL, "wgrad: too many pixels");
    p.dW = dW;
    p.db = db;
    p.db_n = db_n;
    p.rowinfo = (const uint4*)workspace;
    p.ngroups = d->ngroups;
    p.total_tiles = (int)w.tiles;
    p.N = d->N;
    p.Ktot = (int)sh.Ktot;
    p.cshift = sh.cshift; p.crun_mask = d->Crun - 1; p.KW = d->KW;
    p.kw_inv = (65536 + d->KW - 1) / d->KW;
    for (int kp = 0; kp < d->KH * d->KW; ++kp)
        if (((kp * p.kw_inv) >> 16) != kp / d->KW) return rtn_fail(h, RTN_EINVAL, "wgrad: KW %d unsupported", d->KW);
    p.pix_stride_b = (int)sh.pix_b;
    p.sy = d->sy; p.sx = d->sx; p.pad_t = d->pad_t; p.pad_l = d->pad_l;
    p.dy_ld_b = d->out_ld * es;
    p.ntiles_k = (int)((sh.Ktot + w.CH - 1) / w.CH);
    p.tiles_per_split = w.tiles_per_split;
    p.out_tiles = (int)w.out_tiles;
    p.xcd_map = w.xcd_map ? 1 : 0;
    return RTN_OK;
}

int wgrad_launch(rtn_handle_t h, const rtn_conv_desc_t* d, float* dW, float* db, int db_n, void* workspace, size_t workspace_bytes,
                 WgradMode mode = WgradMode::TableAndRun) {
    if (!h) return RTN_EINVAL;
    rtn_env_sync();
    WgradShape sh;
    if (int rc = wgrad_check_desc(h, d, dW, workspace, mode, &sh)) return rc;
    const WgradPlan w = wgrad_plan(d, h->num_cus > 0 ? h->num_cus : 256);
    // required: the row-info table; the slabs of the ordered reduction behind it are used when there is room (else float atomics)
    if (workspace_bytes < w.table_min) return rtn_fail(h, RTN_ENOMEM, "wgrad: workspace %zu < %zu", workspace_bytes, w.table_min);
    // TableOnly never stops at the window kernel: the row-info table is built for every layer, so that a later prepared call that
    // selects the general kernels (a knob flipped in between, a shape the window kernel turns down) never runs on an unprepared table.
    if (mode != WgradMode::TableOnly)
        if (int rc = wgrad_try_win(h, d, w, dW, db, db_n, workspace, workspace_bytes); rc <= 0) return rc;
    WParams p;
    if (int rc = wgrad_fill_params(h, d, sh, w, dW, db, db_n, workspace, &p)) return rc;

    if (mode != WgradMode::RunPrepared) {   // the table depends on the layer's geometry and the dY / X base offsets only: a caller may build it once
        if (sh.es == 2) hipLaunchKernelGGL((wgrad_rowinfo_kernel<2>), dim3(rtn_grid_for(w.tiles * 64)), dim3(256), 0, h->stream, p, (uint4*)workspace);
        else            hipLaunchKernelGGL((wgrad_rowinfo_kernel<4>), dim3(rtn_grid_for(w.tiles * 64)), dim3(256), 0, h->stream, p, (uint4*)workspace);
        RTN_CHECK_LAUNCH(h, "wgrad_rowinfo_kernel");
        if (mode == WgradMode::TableOnly) return RTN_OK;
    }
    // ordered reduction: slabs behind the row-info table when the workspace has room for them (rtn_conv2d_wgrad_workspace_bytes asks
    // for it); otherwise float atomics into dW (the same values, run-to-run differences in the last bits)
    const long long NK = (long long)d->N * sh.Ktot;
    const bool use_slab = w.slab_on && workspace_bytes >= w.table_bytes + w.slab_bytes && NK % 4 == 0;
    if (use_slab) {
        p.slab = (float*)((char*)workspace + w.table_bytes);
        p.bslab = p.slab + (size_t)w.nsplit_used * NK;
    }
    const dim3 grid = w.xcd_map ? dim3((unsigned)(w.out_tiles * w.nsplit)) : dim3((unsigned)w.out_tiles, (unsigned)w.nsplit);
    if (w.dma)            hipLaunchKernelGGL((conv_wgrad_dma_kernel<4, 2, 8>), grid, dim3(512), 0, h->stream, p);
    else if (w.dma_small) hipLaunchKernelGGL((conv_wgrad_dma_kernel<2, 2, 4>), grid, dim3(256), 0, h->stream, p);
    else if (sh.es == 2)  hipLaunchKernelGGL((conv_wgrad_kernel<2>), grid, dim3(256), 0, h->stream, p);
    else                  hipLaunchKernelGGL((conv_wgrad_kernel<4>), grid, dim3(256), 0, h->stream, p);
    RTN_CHECK_LAUNCH(h, "conv_wgrad_kernel");
    h->last_wgrad_impl = w.dma ? 2 : w.dma_small ? 3 : 0;
    if (use_slab) return rtn_wgrad_finish(h, dW, p.slab, (int)w.nsplit_used, NK, db, p.bslab, d->N, db ? db_n : 0);
    return RTN_OK;
}

}  // namespace

extern "C" size_t rtn_conv2d_wgrad_workspace_bytes(const rtn_conv_desc_t* d) {
    rtn_env_sync();
    if (!d || d->ngroups < 1 || d->ngroups > RTN_MAX_GROUPS || d->N < 1 || d->Crun < 1 || d->KH < 1 || d->KW < 1) return 0;
    if (d->dtype != RTN_BF16 && d->dtype != RTN_F32) return 0;
    return wgrad_plan(d, 256).workspace_bytes();
}

extern "C" int rtn_debug_last_wgrad_impl(rtn_handle_t h) { return h ? h->last_wgrad_impl : RTN_EINVAL; }

extern "C" int rtn_conv2d_wgrad(rtn_handle_t h, const rtn_conv_desc_t* d, float* dW, void* workspace, size_t workspace_bytes) {
    return wgrad_launch(h, d, dW, nullptr, 0, workspace, workspace_bytes);
}

/* The per-pixel row-info table alone (workspace), and the weight gradient on a table built earlier for the SAME descriptor. */
extern "C" int rtn_conv2d_wgrad_rowinfo(rtn_handle_t h, const rtn_conv_desc_t* d, void* workspace, size_t workspace_bytes) {
    return wgrad_launch(h, d, nullptr, nullptr, 0, workspace, workspace_bytes, WgradMode::TableOnly);
}
extern "C" int rtn_conv2d_wgrad_prepared(rtn_handle_t h, const rtn_conv_desc_t* d, float* dW, float* db, int db_n, const void* workspace,
                                         size_t workspace_bytes) {
    if (h && db && (db_n < 1 || (d && db_n > d->N))) return rtn_fail(h, RTN_EINVAL, "wgrad_prepared: bad db_n");
    return wgrad_launch(h, d, dW, db, db ? db_n : 0, const_cast<void*>(workspace), workspace_bytes, WgradMode::RunPrepared);
}

/* wgrad with the bias gradient fused: db[0..db_n) += column sums of dY (BiasAddGrad) */
extern "C" int rtn_conv2d_wgrad_bias(rtn_handle_t h, const rtn_conv_desc_t* d, float* dW, float* db, int db_n, void* workspace,
                                     size_t workspace_bytes) {
    if (h && (!db || db_n < 1 || (d && db_n > d->N))) return rtn_fail(h, RTN_EINVAL, "wgrad_bias: bad db / db_n");
    return wgrad_launch(h, d, dW, db, db_n, workspace, workspace_bytes);
}

