// rtn_eval.hip — detection evaluation on the device: per-class AP at up to 16 IoU thresholds and P/R/F1 at a score threshold.
//
// Device restatement of model/eval.py's host path (split_detections -> evaluate_detections -> compute_ap):
//   stage (a) rtn_eval_match, once per batch, one workgroup per image: score threshold + max_detections, boxes back to original
//     coordinates ((double)box / scale), per-class stable sort by descending score, IoU with rtn_iou_f64 (the arithmetic of
//     rtn_compute_overlap), first-index argmax over the image's class-c annotations, one greedy walk per (class, threshold).
//     Every kept detection lands in slot [image][kept index] as {f32 score bits, T-bit hit mask | class << 16}.
//   stage (b) rtn_eval_finalize, once per evaluation: compaction of the valid slots (prefix sums over tiles), a stable LSD radix
//     sort on (class, descending score) - the np.argsort(-s, kind="stable") of the host path, ties in slot order - and per class
//     and threshold tiled scans of TP, the f64 precision / recall curve, the precision envelope (reverse max-scan) and the AP
//     terms, summed in one fixed order.  P/R/F1 at the score threshold come from integer counts.
// No float atomics and no host read-back: results are bit-reproducible.  Integer atomics only count.
// FP contraction is OFF in this file (Makefile STRICT): the host path rounds every op.
#include "rtn_internal.h"
#include "rtn_iou_dev.h"
#include <cfloat>
#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int EV_MATCH_NT = 320;        // >= RTN_MAX_DET: one thread per detection row
constexpr int EV_NT = 256;              // finalize workgroups: 4 waves
constexpr int EV_ITEMS = 4;
constexpr int EV_TILE = EV_NT * EV_ITEMS;   // element e of a tile = round * 256 + thread: rounds are consecutive runs of 256
constexpr int EV_MAX_T = 16;
constexpr unsigned EV_INVALID = 0xFFFFFFFFu;
constexpr long long EV_MAX_SLOTS = 1ll << 28;
constexpr int EV_MAX_CLASSES = 65535;   // the class lives in the upper 16 bits of a slot's value word

struct EvThr { float t[EV_MAX_T]; };

__device__ __forceinline__ unsigned long long lanemask_lt() {
    const int lane = threadIdx.x & 63;
    return lane ? (~0ull >> (64 - lane)) : 0ull;
}

// ---------------------------------------------------------------------------------------------------------------- stage (a)
__global__ __launch_bounds__(EV_MATCH_NT) void eval_match_kernel(
        int D, const float* __restrict__ boxes, const float* __restrict__ scores, const int* __restrict__ labels,
        const double* __restrict__ scales, const double* __restrict__ gt_boxes, const int* __restrict__ gt_labels,
        const int* __restrict__ gt_count, int gt_stride, int K, int T, EvThr thr, double score_thr, int max_det,
        uint2* __restrict__ slots, int* __restrict__ counts) {
    __shared__ double s_box[RTN_MAX_DET][4];     // by kept index
    __shared__ float s_score[RTN_MAX_DET];
    __shared__ int s_lab[RTN_MAX_DET];           // -1: label outside [0, K)
    __shared__ int s_pos[RTN_MAX_DET];           // kept index -> sorted position
    __shared__ int s_order[RTN_MAX_DET];         // sorted position -> kept index
    __shared__ float s_best[RTN_MAX_DET];        // by sorted position: best IoU over the class's annotations
    __shared__ int s_arg[RTN_MAX_DET];           //   its first index (-1: the image has no annotation of that class)
    __shared__ unsigned s_hits[RTN_MAX_DET];
    __shared__ double s_gt[RTN_MAX_GT][4];
    __shared__ int s_glab[RTN_MAX_GT];
    __shared__ float s_thr[EV_MAX_T];
    __shared__ int s_wave[2][EV_MATCH_NT / 64];

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int G = gt_count[b];
    G = G < 0 ? 0 : (G > gt_stride ? gt_stride : G);
    for (int i = tid; i < G; i += EV_MATCH_NT) {
        const double* g = gt_boxes + ((long long)b * gt_stride + i) * 4;
        s_gt[i][0] = g[0]; s_gt[i][1] = g[1]; s_gt[i][2] = g[2]; s_gt[i][3] = g[3];
        s_glab[i] = gt_labels[(long long)b * gt_stride + i];
    }
    if (tid < T) s_thr[tid] = thr.t[tid];

    // split_detections: keep = where(scores > score_threshold)[:max_detections], in row order
    const int r = tid;
    float sc = 0.f;
    bool keep = false;
    if (r < D) {
        sc = scores[(long long)b * D + r];
        keep = (double)sc > score_thr;
    }
    const unsigned long long km = __ballot(keep);
    if (lane == 0) s_wave[0][w] = __popcll(km);
    __syncthreads();
    int k = __popcll(km & lanemask_lt()), nk = 0;
    for (int i = 0; i < EV_MATCH_NT / 64; ++i) {
        if (i < w) k += s_wave[0][i];
        nk += s_wave[0][i];
    }
    nk = nk < max_det ? nk : max_det;
    const bool kept = keep && k < max_det;
    int lab = -1;
    if (kept) {
        lab = labels[(long long)b * D + r];
        if (lab < 0 || lab >= K) lab = -1;                 // split_detections keeps classes 0..K-1 only
        const double s = scales[b];
        const float* bx = boxes + ((long long)b * D + r) * 4;
        s_box[k][0] = (double)bx[0] / s; s_box[k][1] = (double)bx[1] / s;
        s_box[k][2] = (double)bx[2] / s; s_box[k][3] = (double)bx[3] / s;
        s_score[k] = sc;
        s_lab[k] = lab;
    }
    const unsigned long long vm = __ballot(kept && lab >= 0);
    if (lane == 0) s_wave[1][w] = __popcll(vm);
    __syncthreads();
    int nvalid = 0;
    for (int i = 0; i < EV_MATCH_NT / 64; ++i) nvalid += s_wave[1][i];

    // sorted position: (class ascending, score descending, kept index ascending) = per-class np.argsort(-s, kind="stable")
    if (kept && lab >= 0) {
        int pos = 0;
        for (int q = 0; q < nk; ++q) {
            const int lq = s_lab[q];
            if (lq < 0) continue;
            const float sq = s_score[q];
            pos += (lq < lab) || (lq == lab && (sq > sc || (sq == sc && q < k)));
        }
        s_order[pos] = k;
        s_pos[k] = pos;
    }
    __syncthreads();

    // best IoU and its first index over the image's class-c annotations (np.argmax: the first maximum, NaN counts as maximum)
    if (tid < nvalid) {
        const int kk = s_order[tid], c = s_lab[kk];
        float best = 0.f;
        int arg = -1;
        for (int g = 0; g < G; ++g) {
            if (s_glab[g] != c) continue;
            const float iou = rtn_iou_f64(s_box[kk], s_gt[g]);
            if (arg < 0 || (!isnan(best) && (isnan(iou) || iou > best))) { best = iou; arg = g; }
        }
        s_best[tid] = best;
        s_arg[tid] = arg;
        s_hits[tid] = 0u;
    }
    __syncthreads();

    // greedy walks: one lane per (class segment, threshold); a hit takes its annotation for that threshold only
    for (int L = tid; L < nvalid * T; L += EV_MATCH_NT) {
        const int p = L / T, t = L - p * T;
        const int c = s_lab[s_order[p]];
        if (p > 0 && s_lab[s_order[p - 1]] == c) continue;
        const float th = s_thr[t];
        unsigned long long taken = 0ull;
        for (int q = p; q < nvalid && s_lab[s_order[q]] == c; ++q) {
            const int j = s_arg[q];
            if (j >= 0 && s_best[q] >= th && !((taken >> j) & 1ull)) {   // float32 compare (NumPy 2: f32 array vs Python float)
                taken |= 1ull << j;
                atomicOr(&s_hits[q], 1u << t);
            }
        }
    }
    __syncthreads();

    if (tid < max_det) {
        uint2 v = make_uint2(0u, EV_INVALID);
        if (tid < nk && s_lab[tid] >= 0) {
            v.x = __float_as_uint(s_score[tid]);
            v.y = (s_hits[s_pos[tid]] & 0xFFFFu) | ((unsigned)s_lab[tid] << 16);
        }
        slots[(long long)b * max_det + tid] = v;
    }
    // per-class counters: annotations (counts[c]) and kept detections (counts[K + c]), one atomic per (image, class)
    if (tid < G) {
        const int c = s_glab[tid];
        if (c >= 0 && c < K) {
            int n = 0;
            bool first = true;
            for (int g = 0; g < G; ++g)
                if (s_glab[g] == c) { ++n; if (g < tid) first = false; }
            if (first) atomicAdd(&counts[c], n);
        }
    }
    if (tid < nvalid) {
        const int c = s_lab[s_order[tid]];
        if (tid == 0 || s_lab[s_order[tid - 1]] != c) {
            int n = 0;
            for (int q = tid; q < nvalid && s_lab[s_order[q]] == c; ++q) ++n;
            atomicAdd(&counts[K + c], n);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- stage (b)
struct EvLayout {
    long long N;           // slots
    int ntN, K, T;         // tiles over N
    size_t meta, tile_off, keyA, valA, keyB, valB, hist, dsum, tcnt, tf1, tmax, tap, total;
};

// meta: [0] = M (valid slots), [1] = tiles over M, [2 .. 2+K] = class bases, [3+K .. 3+2K] = first class-tile of each class
__device__ __forceinline__ int* meta_cbase(int* meta) { return meta + 2; }
__device__ __forceinline__ int* meta_ctile(int* meta, int K) { return meta + 3 + K; }

// exclusive scan of one int per thread over the 256 threads; returns the block total
__device__ int block_scan_excl(int v, int& excl, int* s_tmp /* >= 4 */) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int x = v;
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    if (lane == 63) s_tmp[w] = x;
    __syncthreads();
    int before = 0, total = 0;
    for (int i = 0; i < EV_NT / 64; ++i) {
        if (i < w) before += s_tmp[i];
        total += s_tmp[i];
    }
    __syncthreads();
    excl = before + x - v;
    return total;
}

// in-place exclusive scan of a[i * stride] for i < n (one workgroup); returns the total
__device__ int block_scan_array(int* a, int n, int stride, int* s_tmp) {
    int carry = 0;
    for (int i0 = 0; i0 < n; i0 += EV_NT) {
        const int i = i0 + threadIdx.x;
        const int v = i < n ? a[(long long)i * stride] : 0;
        int ex;
        const int tot = block_scan_excl(v, ex, s_tmp);
        if (i < n) a[(long long)i * stride] = carry + ex;
        carry += tot;
    }
    return carry;
}

// valid slots per tile
__global__ __launch_bounds__(EV_NT) void ev_compact_count(const uint2* __restrict__ slots, long long N, int* __restrict__ tile_off) {
    __shared__ int s_tmp[4];
    const long long t0 = (long long)blockIdx.x * EV_TILE;
    int n = 0;
    for (int it = 0; it < EV_ITEMS; ++it) {
        const long long e = t0 + it * EV_NT + threadIdx.x;
        if (e < N && slots[e].y != EV_INVALID) ++n;
    }
    int ex;
    const int tot = block_scan_excl(n, ex, s_tmp);
    if (threadIdx.x == 0) tile_off[blockIdx.x] = tot;
}

// one workgroup: tile offsets, class bases and class-tile starts
__global__ __launch_bounds__(EV_NT) void ev_compact_scan(int* __restrict__ tile_off, int ntN, const int* __restrict__ counts, int K,
                                                         int* __restrict__ meta) {
    __shared__ int s_tmp[4];
    const int M = block_scan_array(tile_off, ntN, 1, s_tmp);
    int* cbase = meta_cbase(meta);
    int* ctile = meta_ctile(meta, K);
    for (int c = threadIdx.x; c < K; c += EV_NT) {
        const int n = counts[K + c];
        cbase[c] = n;
        ctile[c] = (n + EV_TILE - 1) / EV_TILE;
    }
    __syncthreads();
    const int Mc = block_scan_array(cbase, K, 1, s_tmp);
    const int tiles = block_scan_array(ctile, K, 1, s_tmp);
    if (threadIdx.x == 0) {
        meta[0] = M < Mc ? M : Mc;            // equal by construction (stage (a) counts what it writes)
        meta[1] = (meta[0] + EV_TILE - 1) / EV_TILE;
        cbase[K] = Mc;
        ctile[K] = tiles;
    }
}

// stable compaction: key = ~score bits (ascending = score descending), value = hits | class << 16
__global__ __launch_bounds__(EV_NT) void ev_compact_scatter(const uint2* __restrict__ slots, long long N, const int* __restrict__ tile_off,
                                                            unsigned* __restrict__ key, unsigned* __restrict__ val) {
    __shared__ int s_tmp[4];
    const long long t0 = (long long)blockIdx.x * EV_TILE;
    int run = tile_off[blockIdx.x];
    for (int it = 0; it < EV_ITEMS; ++it) {
        const long long e = t0 + it * EV_NT + threadIdx.x;
        uint2 v = make_uint2(0u, EV_INVALID);
        if (e < N) v = slots[e];
        const bool ok = v.y != EV_INVALID;
        int ex;
        const int tot = block_scan_excl(ok ? 1 : 0, ex, s_tmp);
        if (ok) {
            key[run + ex] = ~v.x;
            val[run + ex] = v.y;
        }
        run += tot;
    }
}

__device__ __forceinline__ int radix_digit(unsigned k, unsigned v, int pass) {
    // passes 0..3: the key bytes, least significant first; 4, 5: the class bytes
    return pass < 4 ? (int)((k >> (8 * pass)) & 255u) : (int)((v >> (16 + 8 * (pass - 4))) & 255u);
}

__global__ __launch_bounds__(EV_NT) void ev_radix_hist(const unsigned* __restrict__ key, const unsigned* __restrict__ val,
                                                       const int* __restrict__ meta, int ntN, int pass, int* __restrict__ hist) {
    __shared__ int s_h[256];
    const int M = meta[0];
    if ((long long)blockIdx.x * EV_TILE >= M) return;
    s_h[threadIdx.x] = 0;
    __syncthreads();
    for (int it = 0; it < EV_ITEMS; ++it) {
        const int e = blockIdx.x * EV_TILE + it * EV_NT + threadIdx.x;
        if (e < M) atomicAdd(&s_h[radix_digit(key[e], val[e], pass)], 1);
    }
    __syncthreads();
    hist[(long long)threadIdx.x * ntN + blockIdx.x] = s_h[threadIdx.x];
}

// one workgroup per digit: exclusive scan of the digit's per-tile counts; dsum[digit] = its total
__global__ __launch_bounds__(EV_NT) void ev_radix_scan(int* __restrict__ hist, const int* __restrict__ meta, int ntN, int* __restrict__ dsum) {
    __shared__ int s_tmp[4];
    const int tot = block_scan_array(hist + (long long)blockIdx.x * ntN, meta[1], 1, s_tmp);
    if (threadIdx.x == 0) dsum[blockIdx.x] = tot;
}

__global__ __launch_bounds__(EV_NT) void ev_radix_scatter(const unsigned* __restrict__ key, const unsigned* __restrict__ val,
                                                          const int* __restrict__ meta, int ntN, int pass, const int* __restrict__ hist,
                                                          const int* __restrict__ dsum, unsigned* __restrict__ okey,
                                                          unsigned* __restrict__ oval) {
    __shared__ int s_tmp[4];
    __shared__ int s_run[256];
    __shared__ int s_wcnt[EV_NT / 64][256];
    const int M = meta[0];
    if ((long long)blockIdx.x * EV_TILE >= M) return;
    const int tid = threadIdx.x, w = tid >> 6;
    int ex;
    block_scan_excl(dsum[tid], ex, s_tmp);
    s_run[tid] = ex + hist[(long long)tid * ntN + blockIdx.x];
    for (int i = 0; i < EV_NT / 64; ++i) s_wcnt[i][tid] = 0;
    __syncthreads();
    for (int it = 0; it < EV_ITEMS; ++it) {
        const int e = blockIdx.x * EV_TILE + it * EV_NT + tid;
        const bool act = e < M;
        unsigned k = 0u, v = 0u;
        int dg = 0;
        if (act) { k = key[e]; v = val[e]; dg = radix_digit(k, v, pass); }
        unsigned long long peers = __ballot(act);
        for (int bit = 0; bit < 8; ++bit) {
            const bool on = (dg >> bit) & 1;
            const unsigned long long bb = __ballot(on);
            peers &= on ? bb : ~bb;
        }
        const int rank = __popcll(peers & lanemask_lt());
        if (act && rank == 0) s_wcnt[w][dg] = __popcll(peers);
        __syncthreads();
        if (act) {
            int dst = s_run[dg] + rank;
            for (int i = 0; i < w; ++i) dst += s_wcnt[i][dg];
            okey[dst] = k;
            oval[dst] = v;
        }
        __syncthreads();
        int add = 0;
        for (int i = 0; i < EV_NT / 64; ++i) { add += s_wcnt[i][tid]; s_wcnt[i][tid] = 0; }
        s_run[tid] += add;
        __syncthreads();
    }
}

// class-tile g -> class c with ctile[c] <= g < ctile[c + 1]; false past the last class-tile
__device__ __forceinline__ bool class_tile(const int* meta, int K, int g, int& c, int& i0, int& n) {
    const int* ctile = meta_ctile(const_cast<int*>(meta), K);
    if (g >= ctile[K]) return false;
    int lo = 0, hi = K;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (ctile[mid] <= g) lo = mid; else hi = mid;
    }
    c = lo;
    const int* cbase = meta_cbase(const_cast<int*>(meta));
    i0 = (g - ctile[c]) * EV_TILE;
    n = cbase[c + 1] - cbase[c];
    return true;
}

__device__ __forceinline__ int wave_sum_int(int x) {
    for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d);
    return x;
}

// per class-tile: hits per threshold (tcnt), and among the detections with score >= f1_thr: hits per threshold + their number (tf1)
__global__ __launch_bounds__(EV_NT) void ev_stats_tile(const unsigned* __restrict__ key, const unsigned* __restrict__ val,
                                                       const int* __restrict__ meta, int K, int T, float f1_thr, int* __restrict__ tcnt,
                                                       int* __restrict__ tf1) {
    __shared__ int s_acc[2 * EV_MAX_T + 1];
    int c, i0, n;
    if (!class_tile(meta, K, blockIdx.x, c, i0, n)) return;
    const int base = meta_cbase(const_cast<int*>(meta))[c];
    if (threadIdx.x < 2 * EV_MAX_T + 1) s_acc[threadIdx.x] = 0;
    __syncthreads();
    unsigned hits[EV_ITEMS];
    bool above[EV_ITEMS];
    for (int it = 0; it < EV_ITEMS; ++it) {
        const int i = i0 + it * EV_NT + threadIdx.x;
        hits[it] = 0u;
        above[it] = false;
        if (i < n) {
            hits[it] = val[base + i] & 0xFFFFu;
            above[it] = __uint_as_float(~key[base + i]) >= f1_thr;
        }
    }
    for (int t = 0; t <= T; ++t) {
        int a = 0, f = 0;
        for (int it = 0; it < EV_ITEMS; ++it) {
            const int h = t < T ? (int)((hits[it] >> t) & 1u) : 1;
            a += h;
            f += above[it] ? h : 0;
        }
        a = wave_sum_int(a);
        f = wave_sum_int(f);
        if ((threadIdx.x & 63) == 0) {
            if (t < T) atomicAdd(&s_acc[t], a);
            atomicAdd(&s_acc[EV_MAX_T + t], f);
        }
    }
    __syncthreads();
    if (threadIdx.x < T) tcnt[(long long)blockIdx.x * T + threadIdx.x] = s_acc[threadIdx.x];
    if (threadIdx.x <= T) tf1[(long long)blockIdx.x * (T + 1) + threadIdx.x] = s_acc[EV_MAX_T + threadIdx.x];
}

// one workgroup per class: TP prefix over the class's tiles (in place) and the P/R/F1 block of the result
__global__ __launch_bounds__(EV_NT) void ev_stats_scan(const int* __restrict__ meta, int K, int T, const int* __restrict__ counts,
                                                       int* __restrict__ tcnt, const int* __restrict__ tf1, double* __restrict__ result) {
    __shared__ int s_tmp[4];
    const int c = blockIdx.x;
    const int* ctile = meta_ctile(const_cast<int*>(meta), K);
    const int g0 = ctile[c], ng = ctile[c + 1] - ctile[c];
    const long long n_ann = counts[c];
    for (int t = 0; t < T; ++t) {
        block_scan_array(tcnt + (long long)g0 * T + t, ng, T, s_tmp);
        int tp = 0, m = 0;
        for (int j0 = 0; j0 < ng; j0 += EV_NT) {       // integer sums: any order gives the same
            const int j = j0 + threadIdx.x;
            const int* f = tf1 + (long long)(g0 + j) * (T + 1);
            int ex;
            tp += block_scan_excl(j < ng ? f[t] : 0, ex, s_tmp);
            m += block_scan_excl(j < ng ? f[T] : 0, ex, s_tmp);
        }
        if (threadIdx.x == 0) {
            const double TP = tp, FP = (double)(m - tp), FN = (double)(n_ann - tp);
            const double P = (TP + FP) > 0.0 ? TP / (TP + FP) : 0.0;
            const double R = n_ann > 0 ? TP / (double)n_ann : 0.0;
            const double F1 = (P + R) > 0.0 ? 2.0 * P * R / (P + R) : 0.0;
            double* o = result + ((long long)c * T + t) * 8;
            o[1] = (double)n_ann;
            o[2] = TP; o[3] = FP; o[4] = FN; o[5] = P; o[6] = R; o[7] = F1;
        }
    }
}

// block-inclusive count of one bit per element (element order it * 256 + thread) -> cumulative TP of every item
__device__ __forceinline__ void tile_cum_hits(const unsigned* hits, int t, int carry0, int* cum, int* s_tmp) {
    int carry = carry0;
    for (int it = 0; it < EV_ITEMS; ++it) {
        const int h = (int)((hits[it] >> t) & 1u);
        int ex;
        const int tot = block_scan_excl(h, ex, s_tmp);
        cum[it] = carry + ex + h;
        carry += tot;
    }
}

__device__ __forceinline__ double precision_at(int tp, int pos) {
    const double tpd = (double)tp, fpd = (double)(pos + 1 - tp);
    return tpd / fmax(tpd + fpd, DBL_EPSILON);
}

__device__ __forceinline__ double wave_max_dbl(double x) {
    for (int d = 32; d > 0; d >>= 1) x = fmax(x, __shfl_xor(x, d));
    return x;
}

// per class-tile and threshold: the largest precision in the tile (tmax)
__global__ __launch_bounds__(EV_NT) void ev_stats_prec(const unsigned* __restrict__ val, const int* __restrict__ meta, int K, int T,
                                                       const int* __restrict__ tcnt, double* __restrict__ tmax) {
    __shared__ int s_tmp[4];
    __shared__ double s_m[EV_NT / 64];
    int c, i0, n;
    if (!class_tile(meta, K, blockIdx.x, c, i0, n)) return;
    const int base = meta_cbase(const_cast<int*>(meta))[c];
    unsigned hits[EV_ITEMS];
    for (int it = 0; it < EV_ITEMS; ++it) {
        const int i = i0 + it * EV_NT + threadIdx.x;
        hits[it] = i < n ? (val[base + i] & 0xFFFFu) : 0u;
    }
    for (int t = 0; t < T; ++t) {
        int cum[EV_ITEMS];
        tile_cum_hits(hits, t, tcnt[(long long)blockIdx.x * T + t], cum, s_tmp);
        double m = 0.0;
        for (int it = 0; it < EV_ITEMS; ++it) {
            const int i = i0 + it * EV_NT + threadIdx.x;
            if (i < n) m = fmax(m, precision_at(cum[it], i));
        }
        m = wave_max_dbl(m);
        if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = m;
        __syncthreads();
        if (threadIdx.x == 0) {
            double x = 0.0;
            for (int i = 0; i < EV_NT / 64; ++i) x = fmax(x, s_m[i]);
            tmax[(long long)blockIdx.x * T + t] = x;
        }
        __syncthreads();
    }
}

// one workgroup per class: tmax -> the largest precision in the LATER tiles of the class (0 for the last), in place
__global__ __launch_bounds__(EV_NT) void ev_stats_suffix(const int* __restrict__ meta, int K, int T, double* __restrict__ tmax) {
    __shared__ double s_v[EV_NT];
    const int c = blockIdx.x;
    const int* ctile = meta_ctile(const_cast<int*>(meta), K);
    const int g0 = ctile[c], ng = ctile[c + 1] - ctile[c];
    for (int t = 0; t < T; ++t) {
        double carry = 0.0;
        for (int hi = ng; hi > 0; hi -= EV_NT) {
            const int lo = hi - EV_NT > 0 ? hi - EV_NT : 0;
            const int i = lo + threadIdx.x;
            const double v = i < hi ? tmax[(long long)(g0 + i) * T + t] : 0.0;
            s_v[threadIdx.x] = v;
            __syncthreads();
            for (int d = 1; d < EV_NT; d <<= 1) {         // inclusive suffix max within the chunk
                const double o = threadIdx.x + d < EV_NT ? s_v[threadIdx.x + d] : 0.0;
                __syncthreads();
                s_v[threadIdx.x] = fmax(s_v[threadIdx.x], o);
                __syncthreads();
            }
            const double later = threadIdx.x + 1 < EV_NT ? s_v[threadIdx.x + 1] : 0.0;
            if (i < hi) tmax[(long long)(g0 + i) * T + t] = fmax(carry, i + 1 < hi ? later : 0.0);
            const double all = s_v[0];
            __syncthreads();
            carry = fmax(carry, all);
        }
    }
}

// per class-tile and threshold: sum of the AP terms (recall step * precision envelope) at the hits of the tile, fixed order
__global__ __launch_bounds__(EV_NT) void ev_stats_ap(const unsigned* __restrict__ val, const int* __restrict__ meta, int K, int T,
                                                     const int* __restrict__ counts, const int* __restrict__ tcnt,
                                                     const double* __restrict__ tsuf, double* __restrict__ tap) {
    __shared__ int s_tmp[4];
    __shared__ double s_chunk[EV_ITEMS * EV_NT / 64];   // max precision of each run of 64 elements, then the partial sums
    int c, i0, n;
    if (!class_tile(meta, K, blockIdx.x, c, i0, n)) return;
    const int base = meta_cbase(const_cast<int*>(meta))[c];
    const double n_ann = (double)counts[c];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned hits[EV_ITEMS];
    for (int it = 0; it < EV_ITEMS; ++it) {
        const int i = i0 + it * EV_NT + threadIdx.x;
        hits[it] = i < n ? (val[base + i] & 0xFFFFu) : 0u;
    }
    for (int t = 0; t < T; ++t) {
        int cum[EV_ITEMS];
        tile_cum_hits(hits, t, tcnt[(long long)blockIdx.x * T + t], cum, s_tmp);
        double suf[EV_ITEMS];
        for (int it = 0; it < EV_ITEMS; ++it) {            // suffix max of precision within each run of 64 (one wave, one round)
            const int i = i0 + it * EV_NT + threadIdx.x;
            double x = i < n ? precision_at(cum[it], i) : 0.0;
            for (int d = 1; d < 64; d <<= 1) {
                const double y = __shfl_down(x, d);
                if (lane + d < 64) x = fmax(x, y);
            }
            suf[it] = x;
            if (lane == 0) s_chunk[it * (EV_NT / 64) + w] = x;
        }
        __syncthreads();
        const double after_tile = tsuf[(long long)blockIdx.x * T + t];
        double part = 0.0;
        for (int it = 0; it < EV_ITEMS; ++it) {
            const int i = i0 + it * EV_NT + threadIdx.x;
            double env = fmax(suf[it], after_tile);
            for (int ch = it * (EV_NT / 64) + w + 1; ch < EV_ITEMS * EV_NT / 64; ++ch) env = fmax(env, s_chunk[ch]);
            double term = 0.0;
            if (i < n && n_ann > 0.0 && ((hits[it] >> t) & 1u)) {
                const int tp = cum[it];
                term = ((double)tp / n_ann - (double)(tp - 1) / n_ann) * env;    // (mrec[i+1] - mrec[i]) * mpre[i+1]
            }
            for (int d = 32; d > 0; d >>= 1) term += __shfl_xor(term, d);      // fixed butterfly: same order every run
            part = it == 0 ? term : part + term;
        }
        __syncthreads();
        if (lane == 0) s_chunk[w] = part;
        __syncthreads();
        if (threadIdx.x == 0) {
            double s = 0.0;
            for (int i = 0; i < EV_NT / 64; ++i) s += s_chunk[i];
            tap[(long long)blockIdx.x * T + t] = s;
        }
        __syncthreads();
    }
}

// one workgroup per class: AP = the tile partials summed in tile order (a fixed tree per chunk of 256 tiles)
__global__ __launch_bounds__(EV_NT) void ev_stats_final(const int* __restrict__ meta, int K, int T, const int* __restrict__ counts,
                                                        const double* __restrict__ tap, double* __restrict__ result) {
    __shared__ double s_p[EV_NT / 64];
    const int c = blockIdx.x;
    const int* ctile = meta_ctile(const_cast<int*>(meta), K);
    const int g0 = ctile[c], ng = ctile[c + 1] - ctile[c];
    for (int t = 0; t < T; ++t) {
        double acc = 0.0;
        for (int j0 = 0; j0 < ng; j0 += EV_NT) {
            const int j = j0 + threadIdx.x;
            double x = j < ng ? tap[(long long)(g0 + j) * T + t] : 0.0;
            for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d);
            if ((threadIdx.x & 63) == 0) s_p[threadIdx.x >> 6] = x;
            __syncthreads();
            if (threadIdx.x == 0)
                for (int i = 0; i < EV_NT / 64; ++i) acc += s_p[i];
            __syncthreads();
        }
        if (threadIdx.x == 0) result[((long long)c * T + t) * 8] = counts[c] > 0 ? acc : 0.0;
    }
}

inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

EvLayout eval_layout(long long N, int K, int T) {
    EvLayout L;
    L.N = N; L.K = K; L.T = T;
    L.ntN = (int)((N + EV_TILE - 1) / EV_TILE);
    const long long ct = (long long)L.ntN + K;         // class-tiles: sum over classes of ceil(n_c / TILE) <= ntN + K
    size_t o = 0;
    L.meta = o;     o = al256(o + sizeof(int) * (4 + 2 * (size_t)(K + 1)));
    L.tile_off = o; o = al256(o + sizeof(int) * (size_t)L.ntN);
    L.keyA = o;     o = al256(o + sizeof(unsigned) * (size_t)N);
    L.valA = o;     o = al256(o + sizeof(unsigned) * (size_t)N);
    L.keyB = o;     o = al256(o + sizeof(unsigned) * (size_t)N);
    L.valB = o;     o = al256(o + sizeof(unsigned) * (size_t)N);
    L.hist = o;     o = al256(o + sizeof(int) * 256 * (size_t)L.ntN);
    L.dsum = o;     o = al256(o + sizeof(int) * 256);
    L.tcnt = o;     o = al256(o + sizeof(int) * (size_t)ct * T);
    L.tf1 = o;      o = al256(o + sizeof(int) * (size_t)ct * (T + 1));
    L.tmax = o;     o = al256(o + sizeof(double) * (size_t)ct * T);
    L.tap = o;      o = al256(o + sizeof(double) * (size_t)ct * T);
    L.total = o;
    return L;
}

bool eval_shape_ok(long long N, int K, int T) {
    return N >= 1 && N <= EV_MAX_SLOTS && K >= 1 && K <= EV_MAX_CLASSES && T >= 1 && T <= EV_MAX_T;
}

}  // namespace

extern "C" size_t rtn_eval_workspace_bytes(int64_t num_slots, int num_classes, int num_thresholds) {
    if (!eval_shape_ok(num_slots, num_classes, num_thresholds)) return 0;
    return eval_layout(num_slots, num_classes, num_thresholds).total;
}

extern "C" int rtn_eval_match(rtn_handle_t h, int B, int D, const float* boxes, const float* scores, const int32_t* labels,
                              const double* scales, const double* gt_boxes, const int32_t* gt_labels, const int32_t* gt_count,
                              int gt_stride, int num_classes, int num_thresholds, const double* iou_thresholds, double score_threshold,
                              int max_detections, uint32_t* slots, int32_t* counts) {
    if (!h) return RTN_EINVAL;
    if (B < 1 || !boxes || !scores || !labels || !scales || !gt_boxes || !gt_labels || !gt_count || !slots || !counts || !iou_thresholds)
        return rtn_fail(h, RTN_EINVAL, "eval_match: null pointer or B < 1");
    if (D < 1 || D > RTN_MAX_DET) return rtn_fail(h, RTN_EINVAL, "eval_match: D = %d detections per image, must be in [1, %d]", D, RTN_MAX_DET);
    if (max_detections < 1 || max_detections > RTN_MAX_DET)
        return rtn_fail(h, RTN_EINVAL, "eval_match: max_detections = %d, must be in [1, %d]", max_detections, RTN_MAX_DET);
    if (gt_stride < 1 || gt_stride > RTN_MAX_GT)
        return rtn_fail(h, RTN_EINVAL, "eval_match: %d annotations per image, at most %d are supported", gt_stride, RTN_MAX_GT);
    if (num_classes < 1 || num_classes > EV_MAX_CLASSES)
        return rtn_fail(h, RTN_EINVAL, "eval_match: num_classes = %d, must be in [1, %d]", num_classes, EV_MAX_CLASSES);
    if (num_thresholds < 1 || num_thresholds > EV_MAX_T)
        return rtn_fail(h, RTN_EINVAL, "eval_match: %d IoU thresholds, must be between 1 and %d", num_thresholds, EV_MAX_T);
    if (!(score_threshold >= 0.0)) return rtn_fail(h, RTN_EINVAL, "eval_match: score_threshold = %g, must be >= 0", score_threshold);
    EvThr thr;
    for (int t = 0; t < EV_MAX_T; ++t) thr.t[t] = 0.f;
    for (int t = 0; t < num_thresholds; ++t) {
        const double v = iou_thresholds[t];
        if (!(v > 0.0 && v <= 1.0)) return rtn_fail(h, RTN_EINVAL, "eval_match: IoU threshold %d = %g, must be in (0, 1]", t, v);
        thr.t[t] = (float)v;             // NumPy 2 compares the float32 IoU with the threshold rounded to float32
    }
    hipLaunchKernelGGL(eval_match_kernel, dim3(B), dim3(EV_MATCH_NT), 0, h->stream, D, boxes, scores, (const int*)labels, scales, gt_boxes,
                       (const int*)gt_labels, (const int*)gt_count, gt_stride, num_classes, num_thresholds, thr, score_threshold,
                       max_detections, (uint2*)slots, (int*)counts);
    RTN_CHECK_LAUNCH(h, "eval_match_kernel");
    return RTN_OK;
}

extern "C" int rtn_eval_finalize(rtn_handle_t h, int64_t num_images, int max_detections, const uint32_t* slots, const int32_t* counts,
                                 int num_classes, int num_thresholds, double f1_score_threshold, double* result, void* workspace,
                                 size_t workspace_bytes) {
    if (!h) return RTN_EINVAL;
    if (!slots || !counts || !result || !workspace) return rtn_fail(h, RTN_EINVAL, "eval_finalize: null pointer");
    if (max_detections < 1 || max_detections > RTN_MAX_DET)
        return rtn_fail(h, RTN_EINVAL, "eval_finalize: max_detections = %d, must be in [1, %d]", max_detections, RTN_MAX_DET);
    if (num_thresholds < 1 || num_thresholds > EV_MAX_T)
        return rtn_fail(h, RTN_EINVAL, "eval_finalize: %d IoU thresholds, must be between 1 and %d", num_thresholds, EV_MAX_T);
    if (num_classes < 1 || num_classes > EV_MAX_CLASSES)
        return rtn_fail(h, RTN_EINVAL, "eval_finalize: num_classes = %d, must be in [1, %d]", num_classes, EV_MAX_CLASSES);
    if (num_images < 1 || num_images * max_detections > EV_MAX_SLOTS)
        return rtn_fail(h, RTN_EINVAL, "eval_finalize: %lld images x %d slots out of range", (long long)num_images, max_detections);
    if (!(f1_score_threshold >= 0.0))
        return rtn_fail(h, RTN_EINVAL, "eval_finalize: f1_score_threshold = %g, must be >= 0", f1_score_threshold);
    const long long N = (long long)num_images * max_detections;
    const int K = num_classes, T = num_thresholds;
    const EvLayout L = eval_layout(N, K, T);
    if (workspace_bytes < L.total)
        return rtn_fail(h, RTN_ENOMEM, "eval_finalize: workspace %zu bytes, needs %zu", workspace_bytes, L.total);
    char* ws = (char*)workspace;
    int* meta = (int*)(ws + L.meta);
    int* tile_off = (int*)(ws + L.tile_off);
    unsigned* key[2] = {(unsigned*)(ws + L.keyA), (unsigned*)(ws + L.keyB)};
    unsigned* val[2] = {(unsigned*)(ws + L.valA), (unsigned*)(ws + L.valB)};
    int* hist = (int*)(ws + L.hist);
    int* dsum = (int*)(ws + L.dsum);
    int* tcnt = (int*)(ws + L.tcnt);
    int* tf1 = (int*)(ws + L.tf1);
    double* tmax = (double*)(ws + L.tmax);
    double* tap = (double*)(ws + L.tap);
    const uint2* sl = (const uint2*)slots;
    hipStream_t s = h->stream;

    hipLaunchKernelGGL(ev_compact_count, dim3(L.ntN), dim3(EV_NT), 0, s, sl, N, tile_off);
    RTN_CHECK_LAUNCH(h, "ev_compact_count");
    hipLaunchKernelGGL(ev_compact_scan, dim3(1), dim3(EV_NT), 0, s, tile_off, L.ntN, (const int*)counts, K, meta);
    RTN_CHECK_LAUNCH(h, "ev_compact_scan");
    hipLaunchKernelGGL(ev_compact_scatter, dim3(L.ntN), dim3(EV_NT), 0, s, sl, N, (const int*)tile_off, key[0], val[0]);
    RTN_CHECK_LAUNCH(h, "ev_compact_scatter");
    // stable LSD radix sort: 4 passes over the inverted score bits, then the class bytes when there is more than one class
    const int passes = 4 + (K > 1 ? 1 : 0) + (K > 256 ? 1 : 0);
    int cur = 0;
    for (int p = 0; p < passes; ++p) {
        const int pass = p < 4 ? p : 4 + (p - 4);
        hipLaunchKernelGGL(ev_radix_hist, dim3(L.ntN), dim3(EV_NT), 0, s, key[cur], val[cur], (const int*)meta, L.ntN, pass, hist);
        RTN_CHECK_LAUNCH(h, "ev_radix_hist");
        hipLaunchKernelGGL(ev_radix_scan, dim3(256), dim3(EV_NT), 0, s, hist, (const int*)meta, L.ntN, dsum);
        RTN_CHECK_LAUNCH(h, "ev_radix_scan");
        hipLaunchKernelGGL(ev_radix_scatter, dim3(L.ntN), dim3(EV_NT), 0, s, key[cur], val[cur], (const int*)meta, L.ntN, pass,
                           (const int*)hist, (const int*)dsum, key[cur ^ 1], val[cur ^ 1]);
        RTN_CHECK_LAUNCH(h, "ev_radix_scatter");
        cur ^= 1;
    }
    const unsigned ct = (unsigned)(L.ntN + K);
    hipLaunchKernelGGL(ev_stats_tile, dim3(ct), dim3(EV_NT), 0, s, key[cur], val[cur], (const int*)meta, K, T, (float)f1_score_threshold,
                       tcnt, tf1);
    RTN_CHECK_LAUNCH(h, "ev_stats_tile");
    hipLaunchKernelGGL(ev_stats_scan, dim3(K), dim3(EV_NT), 0, s, (const int*)meta, K, T, (const int*)counts, tcnt, (const int*)tf1, result);
    RTN_CHECK_LAUNCH(h, "ev_stats_scan");
    hipLaunchKernelGGL(ev_stats_prec, dim3(ct), dim3(EV_NT), 0, s, val[cur], (const int*)meta, K, T, (const int*)tcnt, tmax);
    RTN_CHECK_LAUNCH(h, "ev_stats_prec");
    hipLaunchKernelGGL(ev_stats_suffix, dim3(K), dim3(EV_NT), 0, s, (const int*)meta, K, T, tmax);
    RTN_CHECK_LAUNCH(h, "ev_stats_suffix");
    hipLaunchKernelGGL(ev_stats_ap, dim3(ct), dim3(EV_NT), 0, s, val[cur], (const int*)meta, K, T, (const int*)counts, (const int*)tcnt,
                       (const double*)tmax, tap);
    RTN_CHECK_LAUNCH(h, "ev_stats_ap");
    hipLaunchKernelGGL(ev_stats_final, dim3(K), dim3(EV_NT), 0, s, (const int*)meta, K, T, (const int*)counts, (const double*)tap, result);
    RTN_CHECK_LAUNCH(h, "ev_stats_final");
    return RTN_OK;
}
