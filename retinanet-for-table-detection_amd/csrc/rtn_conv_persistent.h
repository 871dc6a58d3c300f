// rtn_conv_persistent.h — the host-side planning of the three persistent convolution kernels (generation 4 rtn_conv_halo8.hip,
// generation 5 rtn_conv_gemm8.hip, generation 6 rtn_conv_halon.hip).  Nothing of HIP in here: a plain C++ program can include it
// (tools/conv_plan_check.cpp does).
//
// Per generation two functions:
//   *_takes(call, knobs)    "is this layer mine?" from the descriptor alone: dtype, flags, N range, channel and padding rules, pointers,
//                           strides, *_elems and the ranges the kernels' buffer descriptors reach.  false = "not mine", never an error:
//                           the generic checks of the conv launcher name what is wrong with a descriptor.
//   *_choose(call, cus, capacity, have_scratch, knobs, Choice*)
//                           the cost model and the chip-share heuristics: tile height, K slices / stream-K grid, workgroups, and the
//                           scratch bytes that choice needs.  A pure function of its arguments: it launches nothing, reads no environment
//                           and never sees the handle.  `capacity` = bytes of scratch on offer (kMaxConvWorkspace when the caller is
//                           sizing a workspace), `have_scratch` = whether scratch can be used at all (a sizing call: yes).
//                           false = "not mine".  Call it only after *_takes said yes.
// The `.hip` files fill their kernel parameters from (call, choice) and launch; conv_try_persistent (rtn_conv.hip) is the one driver
// and the only place that knows a sizing call from a launch.
#pragma once
#include <cstddef>
#include <cstdint>
#include "rtn.h"

// what a workspace query offers as capacity: no conv launch ever uses more scratch than this behind the sync block
static constexpr long long kMaxConvWorkspace = 256ll << 20;

struct ConvCall {                  // one launch as the entry points see it
    const rtn_conv_desc_t* d;
    const rtn_conv_src2_t* s2;     // K-concatenated second source (rtn_conv1x1_dual_fwd) or null
    const rtn_conv_fp8_t* q8;      // fp8 operands (rtn_conv2d_fp8_fwd) or null
    float out8_scale;              // != 0: bf16 layer with e4m3 output (rtn_conv2d_fwd_fp8out)
};

// every tuning knob the persistent launchers consult, read once per call by conv_try_persistent (names and defaults there)
struct ConvKnobs {
    int forced;                    // RTN_CONV_IMPL: 4 / 5 / 6 = take every eligible layer on that generation (tests), else the heuristics decide
    int grid_limit;                // RTN_CONV_H8_GRID: at most this many workgroups (0: the CUs) - all three generations
    bool stagger;                  // RTN_CONV_H8_STAGGER: 0 = the two wave groups in lockstep (A/B) - generations 4 and 5
    int h8_mi, h8_ksplit;          // RTN_CONV_H8_MI (3 | 4 row fragments per wave); RTN_CONV_H8_KSPLIT (0 = cost model, 1 = never slice, n = n slices when n divides the group count)
    bool h8_half;                  // RTN_CONV_H8_HALF: 0 = no 128-column instance
    int g8_mi, g8_sk;              // RTN_CONV_G8_MI (2 | 3); RTN_CONV_G8_SK (-1 = cost model, 0 = never, 1 = wherever the shape allows)
    bool g8_n128, g8_narrow;       // RTN_CONV_G8_N128: 0 = N = 128 is not taken; RTN_CONV_G8_NARROW: 0 = N = 128 on the 256-column tile (A/B)
};

// Buffer-descriptor ranges.  A kernel addresses every tensor through a descriptor of at most this many bytes and uses the value itself
// as the offset of "no access" (loads return zeros, stores are dropped), so every tensor must end below it.
constexpr unsigned H8_OOB = 0xFFFFFF00u;              // generation 4: beyond every descriptor
constexpr unsigned G8_OOB = 0xFFFF0000u;              // generation 5: beyond every descriptor even with the largest uniform offset (K bytes) added
constexpr unsigned HN_OOB = 0xFFFFFF00u;              // generation 6
constexpr long long PERSISTENT_MAX_ROWS = 1ll << 24;  // GEMM rows of a group: row -> (image, y, x) runs through 24-bit float reciprocals
constexpr long long PERSISTENT_MAX_ITEMS = 0x3fffffff;       // work items / tiles of a launch
constexpr long long G8_MAX_KBYTES = 16384;            // generation 5: bytes of one K row (both sources)
constexpr long long G8_MAX_SK_STEPS = 1ll << 30;      // generation 5: tiles x K steps of a stream-K launch
constexpr int G8_THREADS = 512;
constexpr int SK_ERR_WORD = 1023;                     // the sync block's word that counts poll timeouts: stream-K grids stay below it
constexpr int HN_R = 256, HN_TM = HN_R - 3;           // generation 6: halo rows / output pixels of a tile (row 255 of a halo = zeros)

inline bool conv_misaligned16(const void* p) { return ((uintptr_t)p & 15) != 0; }

// ------------------------------------------------------------------------------------------------ generation 4 (rtn_conv_halo8.hip)
struct H8Shape {                   // what the descriptor fixes
    int es;                        // bytes per input / weight element
    int epi;                       // bit 0 = residual, bit 1 = ReLU mask
    int ncb;                       // column blocks of 256 channels
    bool half;                     // the 128-column instance (NW = 4): plain epilogue, no slices
    int nchunk, G;                 // 128-byte chunks of a pixel; (kernel row, chunk) groups of a tile
    long long Kbytes, Mtot, slab_ld;
};
inline H8Shape h8_shape(const ConvCall& c) {
    const rtn_conv_desc_t* d = c.d;
    H8Shape s;
    s.es = c.q8 ? 1 : 2;
    s.epi = ((d->flags & RTN_CONV_RES_SAME) ? 1 : 0) | ((d->flags & RTN_CONV_RELU_MASK) ? 2 : 0);
    s.ncb = (d->N + 255) / 256;
    s.half = d->N <= 128;
    s.nchunk = d->Crun * s.es / 128;
    s.G = d->KH * s.nchunk;
    s.Kbytes = (long long)d->KH * d->KW * d->Crun * s.es;
    s.Mtot = 0;
    for (int i = 0; i < d->ngroups; ++i) s.Mtot += (long long)d->g[i].Hout * d->g[i].Wout * d->batch;
    s.slab_ld = 256ll * s.ncb;
    return s;
}

struct H8Choice {
    int mi;                        // row fragments per wave: tiles of 64 mi rows
    int S;                         // K slices (1: none)
    bool half, split;              // kernel instance: 128-column tile; work items carry a column block and a K slice
    int epi;
    long long tiles, items;        // row tiles of all groups; tiles x column blocks x S
    int grid;
    long long slab_ld, slice_bytes;        // f32 slab of one K slice: [Mtot][slab_ld]
    size_t workspace_bytes;
    bool fp8, stagger;             // kernel instance: e4m3 operands; the two wave groups one barrier apart
};

inline bool h8_takes(const ConvCall& c, const ConvKnobs& k) {
    const rtn_conv_desc_t* d = c.d;
    const rtn_conv_fp8_t* q8 = c.q8;
    const bool forced = k.forced == 4;
    if (q8 ? d->dtype != RTN_FP8 : d->dtype != RTN_BF16) return false;
    const int es = q8 ? 1 : 2;
    if (q8 && ((d->flags & ~RTN_CONV_RELU) || d->N <= 128 || d->N > 256)) return false;     // fp8: one full-width column block, bias / ReLU
    if (d->KW != 3 || d->KH < 1 || d->KH > 7 || d->sy != 1 || d->sx != 1) return false;
    if (d->flags & ~(RTN_CONV_RELU | RTN_CONV_RES_SAME | RTN_CONV_RELU_MASK | RTN_CONV_MASK_PRE)) return false;
    if ((d->flags & RTN_CONV_MASK_PRE) && !(d->flags & RTN_CONV_RELU_MASK)) return false;
    const int epi = ((d->flags & RTN_CONV_RES_SAME) ? 1 : 0) | ((d->flags & RTN_CONV_RELU_MASK) ? 2 : 0);
    const int ncb = (d->N + 255) / 256;
    if (d->N <= 64 || ncb > 8 || d->w_rows < d->N || d->N % 8 || d->out_ld % 8) return false;    // weight rows past w_rows read as zeros (descriptor range)
    if (ncb > 1 && epi) return false;
    const bool half = d->N <= 128;
    if (half && !forced && !k.h8_half) return false;
    if (d->Crun != d->pix_stride || (d->Crun * es) % 128 || d->Crun <= 0) return false;
    if (d->pad_l < 0 || d->pad_l >= d->KW || d->pad_t < 0 || d->pad_t >= d->KH) return false;
    if (conv_misaligned16(d->w) || conv_misaligned16(d->bias)) return false;
    const long long Kbytes = (long long)d->KH * d->KW * d->Crun * es;
    if (Kbytes * 256 * ncb >= (long long)H8_OOB) return false;           // the staging offsets of the last column block
    for (int i = 0; i < d->ngroups; ++i) {
        const rtn_conv_group_t& s = d->g[i];
        if (s.Hin != s.Hout || s.Win != s.Wout || s.in_row_stride != (long long)s.Win * d->pix_stride ||
            s.in_img_stride < (long long)s.Hin * s.in_row_stride) return false;
        if (s.in_elems < (long long)(d->batch - 1) * s.in_img_stride + (long long)s.Hin * s.in_row_stride) return false;
        const long long cells = (long long)s.Hout * s.Wout, M = cells * d->batch;
        if (s.out_step > 1 || s.out_off != 0 || s.out_img_stride != cells * d->out_ld) return false;      // dense [M][out_ld] output
        if (M >= PERSISTENT_MAX_ROWS || M < 1) return false;
        if (!s.in || !s.out || conv_misaligned16(s.in) || conv_misaligned16(s.out)) return false;
        if (s.in_elems < M * d->Crun || s.out_elems < (M - 1) * d->out_ld + d->N) return false;
        if (s.in_elems * 2 >= (long long)H8_OOB || s.out_elems * 2 >= (long long)H8_OOB) return false;
        if (epi & 1) {
            if (!s.res || conv_misaligned16(s.res) || s.res_ld % 8 || s.res_img_stride != cells * s.res_ld) return false;
            if (s.res_elems < (M - 1) * s.res_ld + d->N || s.res_elems * 2 >= (long long)H8_OOB) return false;
        }
        if (epi & 2) {
            if (!s.mask || conv_misaligned16(s.mask) || s.mask_ld % 8 || s.mask_img_stride != cells * s.mask_ld) return false;
            if (s.mask_elems < (M - 1) * s.mask_ld + d->N || s.mask_elems * 2 >= (long long)H8_OOB) return false;
        }
        if (i > 0 && ((epi & 1) && s.res_ld != d->g[0].res_ld)) return false;
        if (i > 0 && ((epi & 2) && s.mask_ld != d->g[0].mask_ld)) return false;
    }
    return true;
}

// Tile height (rows = 64 mi) and K slices by a cost model in microseconds: rounds of workgroups x K steps of an item (+ 5 for its
// prologue / epilogue) x 1.53 us per 256-row step, + for S > 1 the finish launch and the slabs' round trip at 4 TB/s.
// RTN_CONV_H8_MI / RTN_CONV_H8_KSPLIT pin them (A/B, tests).
inline bool h8_choose(const ConvCall& c, int cus, long long capacity, bool have_scratch, const ConvKnobs& k, H8Choice* ch) {
    const rtn_conv_desc_t* d = c.d;
    const bool q8 = c.q8 != nullptr, forced = k.forced == 4;
    const H8Shape sh = h8_shape(c);
    const int G = sh.G, ncb = sh.ncb, mi_force = k.h8_mi, ksplit_force = k.h8_ksplit;
    const long long Mtot = sh.Mtot, slab_ld = sh.slab_ld;
    const bool can_split = !sh.half && !q8 && d->ngroups == 1 && sh.epi == 0 && ksplit_force != 1 && capacity > 0;
    int mi = 0, S = 1;
    {
        double best = 0;
        for (int cand = 4; cand >= 3; --cand) {
            if (!q8 && mi_force >= 3 && mi_force <= 4 && cand != mi_force) continue;
            if (q8 && cand == 4) continue;                 // fp8 holds both k halves' A fragments: the 256-row instance spills, 192 rows fit (256 VGPRs)
            long long t = 0;
            for (int i = 0; i < d->ngroups; ++i) t += ((long long)d->g[i].Hout * d->g[i].Wout * d->batch + 64 * cand - 4) / (64 * cand - 3);
            const double step_us = 1.53 * (cand + 0.3) / 4.3;
            for (int sc = 1; sc <= 8; ++sc) {
                if (sc > 1 && (!can_split || G % sc || (ksplit_force > 1 && sc != ksplit_force))) continue;
                if (sc == 1 && ksplit_force > 1 && can_split && G % ksplit_force == 0) continue;
                if (sc > 1 && (double)sc * Mtot * slab_ld * 4 > (double)capacity) continue;
                const long long items = t * ncb * sc;
                double cost = (double)((items + cus - 1) / cus) * (3.0 * G / sc + 5.0) * step_us;
                if (sc > 1) cost += 4.0 + ((double)sc * Mtot * slab_ld * 4 + (double)Mtot * d->N * 2) / 4.0e6;
                if (mi == 0 || cost < best * 0.97) { best = cost; mi = cand; S = sc; }
            }
        }
        if (mi == 0) return false;
    }
    // slices chosen, but the scratch on offer is null or misaligned: "not mine" - the choice is not made again with S = 1
    if (S > 1 && !have_scratch) return false;
    const int TM = 64 * mi - 3;
    long long tiles = 0;
    for (int i = 0; i < d->ngroups; ++i) tiles += ((long long)d->g[i].Hout * d->g[i].Wout * d->batch + TM - 1) / TM;
    const long long items = tiles * ncb * S;
    if (tiles < 1 || items > PERSISTENT_MAX_ITEMS) return false;
    // one 256 x 256 tile per CU: below a quarter of the chip the narrow tiles of generation 2 (four times the workgroups) are
    // faster (P5 at batch 8 unsliced: 34 tiles, 0.049 ms here against 0.037 ms); from half the chip on this kernel wins (res4 3x3,
    // P4: 133 tiles, 0.054 against 0.067 ms)
    if (!forced && items * 4 < cus) return false;
    const long long slice_bytes = Mtot * slab_ld * 4;
    if (S > 1 && slice_bytes >= (long long)H8_OOB) return false;
    ch->mi = mi; ch->S = S;
    ch->half = sh.half; ch->split = ncb > 1 || S > 1;
    ch->epi = sh.epi;
    ch->tiles = tiles; ch->items = items;
    int grid = cus;
    if (k.grid_limit > 0 && k.grid_limit < grid) grid = k.grid_limit;
    if (grid > (int)items) grid = (int)items;
    ch->grid = grid;
    ch->slab_ld = slab_ld; ch->slice_bytes = slice_bytes;
    ch->workspace_bytes = S > 1 ? (size_t)(slice_bytes * S) : 0;
    ch->fp8 = q8; ch->stagger = k.stagger;
    return true;
}

// ------------------------------------------------------------------------------------------------ generation 5 (rtn_conv_gemm8.hip)
struct G8Shape {
    bool res_up, n128, scatter;
    int epi;                       // bit 0 = residual (same extent or upsampled), bit 1 = ReLU mask
    long long cells, M;            // output pixels per image, GEMM rows
    long long img_pix, last_pix;   // pixels per image of out / res / mask; the farthest pixel of an image a row maps to
    long long Kbytes;              // both sources
};
inline G8Shape g8_shape(const ConvCall& c, const ConvKnobs& k) {
    const rtn_conv_desc_t* d = c.d;
    const rtn_conv_group_t& g = d->g[0];
    G8Shape s;
    s.res_up = d->flags & RTN_CONV_RES_UPSAMPLE;
    s.epi = ((d->flags & (RTN_CONV_RES_SAME | RTN_CONV_RES_UPSAMPLE)) ? 1 : 0) | ((d->flags & RTN_CONV_RELU_MASK) ? 2 : 0);
    // N = 128: half of the 256-column tile multiplies zeros (weight rows past w_rows come from the descriptor's range check).  The
    // layers this is for are bound by their pixel traffic: res3 branch2a in the step's sequence 0.063 -> 0.055 ms (RTN_CONV_G8_N128=0: off)
    s.n128 = d->N == 128 && (k.forced == 5 || k.g8_n128);
    s.cells = (long long)g.Hout * g.Wout;
    s.M = s.cells * d->batch;
    s.scatter = g.out_step > 1;                           // dgrad of a stride-2 1x1 'valid' conv: rows land on the stride grid
    s.img_pix = s.scatter && d->out_ld ? g.out_img_stride / d->out_ld : s.cells;
    s.last_pix = s.scatter ? (long long)(g.Hout - 1) * g.out_step * g.out_pix_w + (long long)(g.Wout - 1) * g.out_step : s.cells - 1;
    s.Kbytes = ((long long)d->Crun + (c.s2 ? c.s2->C : 0)) * 2;
    return s;
}

struct G8Choice {
    int mi;                        // row fragments per wave: tiles of 64 mi rows
    int sk_grid;                   // workgroups of the stream-K form (0: whole tiles per workgroup)
    bool narrow, scatter;          // kernel instance: 128-column tile; rows land on the stride grid (out_step > 1)
    int epi;
    long long ntm;                 // row tiles
    int ntn;                       // column tiles
    long long tiles;
    int grid;
    size_t workspace_bytes;        // stream-K slabs: one partial tile per workgroup
    bool stagger;                  // kernel instance
};

inline bool g8_takes(const ConvCall& c, const ConvKnobs& k) {
    const rtn_conv_desc_t* d = c.d;
    const rtn_conv_src2_t* s2 = c.s2;
    const bool forced = k.forced == 5;
    if (d->dtype != RTN_BF16 || d->ngroups != 1) return false;
    if (d->KH != 1 || d->KW != 1 || d->pad_t != 0 || d->pad_l != 0 || d->sy != d->sx || d->sy < 1 || d->sy > 2) return false;
    if (d->flags & ~(RTN_CONV_RELU | RTN_CONV_RES_SAME | RTN_CONV_RES_UPSAMPLE | RTN_CONV_RELU_MASK | RTN_CONV_MASK_PRE)) return false;
    if ((d->flags & RTN_CONV_MASK_PRE) && !(d->flags & RTN_CONV_RELU_MASK)) return false;
    if ((d->flags & RTN_CONV_RES_SAME) && (d->flags & RTN_CONV_RES_UPSAMPLE)) return false;
    const G8Shape sh = g8_shape(c, k);
    const bool res_up = sh.res_up, n128 = sh.n128, scatter = sh.scatter;
    const int epi = sh.epi;
    if (epi && s2) return false;
    if (!n128 && (d->N < 256 || d->N % 256)) return false;
    if (d->N > 2048 || d->w_rows != d->N || d->out_ld % 8) return false;
    if ((d->Crun * 2) % 128 || d->Crun <= 0 || d->pix_stride < d->Crun || (d->pix_stride * 2) % 16) return false;
    if (conv_misaligned16(d->w) || conv_misaligned16(d->bias)) return false;
    const rtn_conv_group_t& g = d->g[0];
    if (!g.in || !g.out || conv_misaligned16(g.in) || conv_misaligned16(g.out)) return false;
    const long long cells = sh.cells, M = sh.M;
    if (M < 1 || M >= PERSISTENT_MAX_ROWS) return false;
    if (scatter && (res_up || g.out_pix_w < (g.Wout - 1) * g.out_step + 1 || d->out_ld == 0 || g.out_img_stride % d->out_ld || g.out_img_stride <= 0)) return false;
    const long long img_pix = sh.img_pix, last_pix = sh.last_pix;
    if (scatter && last_pix >= img_pix) return false;
    // measured (tools/profile_train.py, batch 8): the scatter pays on the long-K gradients (res3a / res5a branch1: 0.096 -> 0.077,
    // 0.071 -> 0.063 ms) and loses on the short-K ones (res3a / res4a branch2a, K = 128 / 256: 0.061 -> 0.076, 0.037 -> 0.049 against
    // generation 2's 64-wide tiles): taken from K = 512 on
    if (scatter && !forced && d->Crun < 512) return false;
    if (g.out_off != 0 || (!scatter && g.out_img_stride != cells * d->out_ld)) return false;
    if ((long long)(g.Hout - 1) * d->sy >= g.Hin || (long long)(g.Wout - 1) * d->sx >= g.Win) return false;
    if (g.in_elems * 2 >= (long long)G8_OOB || g.out_elems * 2 >= (long long)G8_OOB) return false;
    const long long max_pix = (long long)(d->batch - 1) * img_pix + last_pix;             // the farthest pixel a row maps to
    if (g.out_elems < max_pix * d->out_ld + d->N) return false;
    if ((epi & 1) && !res_up) {
        if (!g.res || conv_misaligned16(g.res) || g.res_ld % 8 || g.res_img_stride != img_pix * g.res_ld) return false;
        if (g.res_elems < max_pix * g.res_ld + d->N || g.res_elems * 2 >= (long long)G8_OOB) return false;
    }
    if (res_up) {
        if (!g.res || conv_misaligned16(g.res) || g.res_ld % 8 || g.res_img_stride % 8 || g.Hres < 1 || g.Wres < 1) return false;
        if (g.res_img_stride < 0 || (long long)(d->batch - 1) * g.res_img_stride + ((long long)g.Hres * g.Wres - 1) * g.res_ld + d->N > g.res_elems) return false;
        if (g.res_elems * 2 >= (long long)G8_OOB) return false;
    }
    if (epi & 2) {
        if (!g.mask || conv_misaligned16(g.mask) || g.mask_ld % 8 || g.mask_img_stride != img_pix * g.mask_ld) return false;
        if (g.mask_elems < max_pix * g.mask_ld + d->N || g.mask_elems * 2 >= (long long)G8_OOB) return false;
    }
    const long long in_max = (long long)(d->batch - 1) * g.in_img_stride + (long long)(g.Hout - 1) * d->sy * g.in_row_stride +
                             (long long)(g.Wout - 1) * d->sx * d->pix_stride + d->Crun;
    if (in_max > g.in_elems) return false;
    if (s2) {
        if (!s2->in || conv_misaligned16(s2->in) || s2->C < 1 || (s2->C * 2) % 128 || s2->step < 1) return false;
        if ((long long)(g.Hout - 1) * s2->step >= s2->Hin || (long long)(g.Wout - 1) * s2->step >= s2->Win) return false;
        const long long in2_max = (long long)(d->batch - 1) * s2->in_img_stride + (long long)(g.Hout - 1) * s2->step * s2->in_row_stride +
                                  (long long)(g.Wout - 1) * s2->step * s2->pix_stride + s2->C;
        if (in2_max > s2->in_elems || s2->in_elems * 2 >= (long long)G8_OOB) return false;
    }
    if (sh.Kbytes > G8_MAX_KBYTES || sh.Kbytes * d->N >= (long long)G8_OOB) return false;
    return true;
}

// `have_scratch`: a sync block and slabs can be used (a sizing call, or a launch whose workspace is there and aligned); without, only
// the plain form (whole tiles per workgroup) is considered.
inline bool g8_choose(const ConvCall& c, int cus, long long capacity, bool have_scratch, const ConvKnobs& k, G8Choice* ch) {
    const rtn_conv_desc_t* d = c.d;
    const bool forced = k.forced == 5, stagger = k.stagger;
    const G8Shape sh = g8_shape(c, k);
    const long long M = sh.M;
    const int mi_force = k.g8_mi, grid_limit = k.grid_limit, sk_mode = k.g8_sk;
    const int ntn = sh.n128 ? 1 : (d->N + 255) / 256;      // N = 128: the 128-column instance, one column tile
    const long long nk_all = sh.Kbytes / 128;
    int mi = mi_force;
    double plain_cost = 0;                             // in units of one 64-row fragment row x one K step
    {                                                  // tile height by rounds x K steps x (rows + a fixed per-step cost)
        double best = 0;
        int pick = 0;
        for (int cand = 3; cand >= 2; --cand) {
            if (mi_force >= 2 && mi_force <= 3 && cand != mi_force) continue;
            const long long tl = ((M + 64 * cand - 1) / (64 * cand)) * ntn;
            const double cost = (double)((tl + cus - 1) / cus) * (cand + 0.4);
            if (pick == 0 || cost < best * 0.97) { best = cost; pick = cand; }
        }
        mi = pick;
        plain_cost = best * (double)nk_all;
    }
    // Stream-K: every workgroup an equal share of the tiles x K steps (see the header of rtn_conv_gemm8.hip).  Taken when it saves at
    // least TEN K steps per workgroup against whole rounds of whole tiles - measured at batch 8, 800 x 1333 (profiles/r4_streamk_gemm8.txt):
    // the hand-off costs 8-10 us whatever the layer (every workgroup publishes one partial tile and owns one: 50 MB out and back at the end
    // of the launch, all owners at once), and a K step does not stay 1.25 us when more CUs run it - between 175 and 256 busy CUs it grows to
    // 1.6-1.9 us (shader clock 2.08 -> 2.01 GHz only; the staging rate of the chip, 8-9 TB/s L2 -> LDS, is the same in both cases).  So the
    // layers with 175 of 256 tiles (stage 4, C4_reduced: 5 steps saved) LOSE 4-7 us, and the ones on 44-88 CUs (stage 5 branch2a 21 steps,
    // C5_reduced 26, res5a branch2c + shortcut 15) gain 6-15 us.  Grid: the CUs, at most 8 pieces per tile.
    int sk_grid = 0;
    const bool sk_shape = !sh.n128 && !(sh.epi & 2) && !sh.scatter && stagger && nk_all >= 2 && nk_all <= 256;
    if (sk_shape && sk_mode != 0 && have_scratch) {
        double best = 0;
        int pick = 0, pick_grid = 0;
        for (int cand = 3; cand >= 2; --cand) {
            if (mi_force >= 2 && mi_force <= 3 && cand != mi_force) continue;
            const long long tl = ((M + 64 * cand - 1) / (64 * cand)) * ntn, total = tl * nk_all;
            long long G = cus;
            if (grid_limit > 0 && grid_limit < G) G = grid_limit;
            if (G > tl * 8) G = tl * 8;
            if (G > total) G = total;
            if (G > SK_ERR_WORD) G = SK_ERR_WORD;
            if (G < 1 || total >= G8_MAX_SK_STEPS) continue;
            const long long slab_need = G * (long long)(cand * 4 * 2) * G8_THREADS * 16;
            // (a sizing call offers kMaxConvWorkspace, which never binds here: slab_need <= SK_ERR_WORD * 24 * G8_THREADS * 16
            // = 201,129,984 bytes < 256 MiB - so the sizing call and the launch run the same test)
            if (slab_need > capacity) continue;
            if (slab_need >= (long long)G8_OOB) continue;
            const long long share_i = (total + G - 1) / G;
            const double share = (double)share_i;
            const bool whole = total % G == 0 && share_i % nk_all == 0;               // every range = whole tiles: nothing is handed over
            const double partners = (double)((nk_all + share_i - 1) / share_i);      // pieces the longest-cut tile has besides its head
            const double fix = whole ? 0.0 : 10.0 + 2.0 * (partners > 2.0 ? partners - 2.0 : 0.0);
            const double cost = (share + fix) * (cand + 0.4);
            if (pick == 0 || cost < best * 0.97) { best = cost; pick = cand; pick_grid = (int)G; }
        }
        if (pick && (sk_mode > 0 || best <= plain_cost)) { mi = pick; sk_grid = pick_grid; }
    }
    const long long ntm = (M + 64 * mi - 1) / (64 * mi), tiles = ntm * ntn;
    if (tiles > PERSISTENT_MAX_ITEMS) return false;
    // too few tiles to be worth one workgroup per CU: below ~5/8 of the chip the 64-wide tiles of generation 2 (four times the
    // workgroups) win (res5 branch2a, 132 tiles: 0.049 ms here against 0.043; C5_reduced, 66 tiles: 0.046 against 0.041), above
    // it this kernel does (res4 branch2a, 175 tiles: 0.037 against 0.046).  (Round 3 re-measured: back-to-back launches of ONE layer
    // say the opposite for res5 branch2a - 0.034 against 0.039 - because its 2 MB of filters then sit in the L2; in the step's own
    // sequence, tools/profile_layers.py, it is 0.049 against 0.046-0.047 as before.  Judge such layers in sequence.)
    if (!forced && !sk_grid && tiles * 8 < (long long)cus * 5) return false;
    ch->mi = mi; ch->sk_grid = sk_grid;
    ch->narrow = sh.n128 && !c.s2 && stagger && k.g8_narrow;
    ch->scatter = sh.scatter;
    ch->epi = sh.epi;
    ch->ntm = ntm; ch->ntn = ntn; ch->tiles = tiles;
    int grid = cus;
    if (grid_limit > 0 && grid_limit < grid) grid = grid_limit;
    if (grid > (int)tiles) grid = (int)tiles;
    ch->grid = sk_grid ? sk_grid : grid;
    ch->workspace_bytes = (size_t)sk_grid * (size_t)(mi * 4 * 2) * G8_THREADS * 16;
    ch->stagger = stagger;
    return true;
}

// ------------------------------------------------------------------------------------------------ generation 6 (rtn_conv_halon.hip)
struct HNChoice {
    int nf;                        // 16-channel fragments of the output: the kernel instance
    long long tiles;
    int grid;
    bool vec;                      // 16-byte stores (every group's output 16-byte aligned, channel count a multiple of 4)
    size_t workspace_bytes;        // always 0: the kernel has no scratch
};

inline bool hn_takes(const ConvCall& c, const ConvKnobs&) {
    const rtn_conv_desc_t* d = c.d;
    if (d->dtype != RTN_BF16) return false;
    if (d->KW != 3 || d->KH != 3 || d->sy != 1 || d->sx != 1) return false;
    if (!(d->flags & RTN_CONV_OUT_F32) || (d->flags & ~(RTN_CONV_OUT_F32 | RTN_CONV_RELU | RTN_CONV_SIGMOID))) return false;
    if (d->N < 1 || d->N > 48 || d->out_ld < d->N) return false;
    const int nf = (d->N + 15) / 16;
    if (d->w_rows < 16 * nf) return false;
    if (d->Crun != d->pix_stride || (d->Crun * 2) % 128 || d->Crun <= 0) return false;
    if (d->pad_l < 0 || d->pad_l >= 3 || d->pad_t < 0 || d->pad_t >= 3) return false;
    if (conv_misaligned16(d->w) || conv_misaligned16(d->bias)) return false;
    const long long Kbytes = 9ll * d->Crun * 2;
    if (Kbytes * d->w_rows >= (long long)HN_OOB) return false;
    for (int i = 0; i < d->ngroups; ++i) {
        const rtn_conv_group_t& s = d->g[i];
        if (s.Hin != s.Hout || s.Win != s.Wout || s.in_row_stride != (long long)s.Win * d->pix_stride ||
            s.in_img_stride != (long long)s.Hin * s.in_row_stride) return false;
        const long long cells = (long long)s.Hout * s.Wout, M = cells * d->batch;
        if (s.out_step > 1 || s.out_off < 0 || M >= PERSISTENT_MAX_ROWS || M < 1) return false;
        if (!s.in || !s.out || conv_misaligned16(s.in) || ((uintptr_t)s.out & 3)) return false;
        if (s.in_elems < M * d->Crun || s.in_elems * 2 >= (long long)HN_OOB || s.out_elems * 4 >= (long long)HN_OOB) return false;
        if (s.out_img_stride < 0 || (d->batch - 1) * s.out_img_stride + s.out_off + (cells - 1) * d->out_ld + d->N > s.out_elems) return false;
    }
    return true;
}

// (no scratch: capacity and have_scratch are there for the common shape of the three planners)
inline bool hn_choose(const ConvCall& c, int cus, long long /*capacity*/, bool /*have_scratch*/, const ConvKnobs& k, HNChoice* ch) {
    const rtn_conv_desc_t* d = c.d;
    long long tiles = 0;
    bool vec = d->N % 4 == 0 && d->out_ld % 4 == 0;
    for (int i = 0; i < d->ngroups; ++i) {
        const rtn_conv_group_t& s = d->g[i];
        if (conv_misaligned16(s.out) || s.out_img_stride % 4 || s.out_off % 4) vec = false;
        tiles += ((long long)s.Hout * s.Wout * d->batch + HN_TM - 1) / HN_TM;
    }
    if (tiles < 1 || tiles > PERSISTENT_MAX_ITEMS) return false;
    if (k.forced != 6 && tiles * 4 < cus) return false;      // below a quarter of the chip: generation 2's narrow tiles
    ch->nf = (d->N + 15) / 16;
    ch->tiles = tiles;
    int grid = cus;
    if (k.grid_limit > 0 && k.grid_limit < grid) grid = k.grid_limit;
    if (grid > (int)tiles) grid = (int)tiles;
    ch->grid = grid;
    ch->vec = vec;
    ch->workspace_bytes = 0;
    return true;
}
