// rtn_optimizer.hip — the optimizer of the training step: clipnorm Adam over element ranges of the flat parameter vector
// (rtn_sumsq_ranges, rtn_adam_clipnorm_step_ranges[_pertensor]).
// Keras-2 Adam (RetinaNet.py:130: lr, beta 0.9/0.999, epsilon 1e-7, no decay), per element of the flat f32 vector
// [weights | bias slots] that holds the unfolded master copy w, the moments m, v and the gradient:
//   g = grad * gscale * grad_mul * clip;  lr_t = lr * sqrt(1 - b2^t) / (1 - b1^t)
//   m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;  w -= lr_t * m / (sqrt(v) + eps);  w_fwd = cast(w * fold)
// gscale is the frozen-BN scale of the element's output channel (the gradient arrives w.r.t. the folded kernel) and 0 on slots
// that never train (padding rows, structural zeros of the stem); fold is the same scale, 1 elsewhere, and re-emits the forward
// weights from the master copy.
// Which elements take part is a table of nr rows (begin, end, vbegin): range r is the flat slice [begin, end) and occupies
// [vbegin, vbegin + end - begin) of the launch's index space, which is cut into quads of 4.  A thread finds the range of its quad
// by a binary search over vbegin (the prefix sums), then walks on for the quad's other elements.  A quad that lies inside one
// range at a 4-aligned flat index is one 16-byte access per array; everything else goes element by element.  Slots outside every
// range are never read or written.  The full step is the table with one range per weight tensor and per bias vector; a
// frozen-layer step is the same table without the frozen layers' rows.  Ranges that touch may be given as one row when no sum per
// range is wanted: every element keeps its place in the index space, and the search has fewer rows.
// Clipping: global norm (standalone Keras 2.x) takes one sum over all ranges, clip = min(1, clipnorm / norm); per tensor
// (tf.keras / Keras >= 2.4) takes one sum per range and clips every range by its own norm.
#include "rtn_internal.h"

namespace {

struct RangeRow { long long begin, end, vbegin; };

__device__ __forceinline__ int range_of(const RangeRow* __restrict__ t, int nr, long long q) {
    int lo = 0, hi = nr;                                  // last range whose vbegin <= q (ranges are in vbegin order)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (t[mid].vbegin <= q) lo = mid; else hi = mid;
    }
    return lo;
}

// flat index of virtual element q, or -1 when q falls in a gap between ranges (r: the range at or before q, advanced in place)
__device__ __forceinline__ long long range_flat(const RangeRow* __restrict__ t, int nr, long long q, int& r, long long n) {
    while (r + 1 < nr && t[r + 1].vbegin <= q) ++r;
    const long long off = q - t[r].vbegin;
    if (off < 0 || off >= t[r].end - t[r].begin) return -1;
    const long long f = t[r].begin + off;
    return (f >= 0 && f < n) ? f : -1;
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// sum of the 256 threads' values in a fixed order (wave sums, then the four waves in turn); thread 0 stores it
__device__ __forceinline__ void block_sum_store_d(double s, double* __restrict__ dst) {
    __shared__ double sh[4];
    s = wave_sum_d(s);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) *dst = sh[0] + sh[1] + sh[2] + sh[3];
}

// sum of (g*scale)^2 over the ranges: per-block partials in a fixed order, finished by sumsq_final_kernel
template <bool VEC>
__global__ __launch_bounds__(256) void sumsq_ranges_kernel(const float* __restrict__ g, const float* __restrict__ scale, long long n,
                                                           const RangeRow* __restrict__ t, int nr, long long span,
                                                           double* __restrict__ partial) {
    double s = 0.0;
    const long long nq = (span + 3) >> 2;
    for (long long qi = (long long)blockIdx.x * blockDim.x + threadIdx.x; qi < nq; qi += (long long)gridDim.x * blockDim.x) {
        const long long q = qi << 2;
        int r = range_of(t, nr, q);
        const long long off = q - t[r].vbegin, f0 = t[r].begin + off;
        if (VEC && off >= 0 && off + 4 <= t[r].end - t[r].begin && (f0 & 3) == 0 && f0 >= 0 && f0 + 4 <= n) {
            const float4 gv = *reinterpret_cast<const float4*>(g + f0);
            const float4 sv = scale ? *reinterpret_cast<const float4*>(scale + f0) : make_float4(1.f, 1.f, 1.f, 1.f);
            const float a0 = gv.x * sv.x, a1 = gv.y * sv.y, a2 = gv.z * sv.z, a3 = gv.w * sv.w;
            s += (double)a0 * (double)a0;
            s += (double)a1 * (double)a1;
            s += (double)a2 * (double)a2;
            s += (double)a3 * (double)a3;
            continue;
        }
        for (int j = 0; j < 4; ++j) {
            const long long f = range_flat(t, nr, q + j, r, n);
            if (f < 0) continue;
            const float a = g[f] * (scale ? scale[f] : 1.f);
            s += (double)a * (double)a;
        }
    }
    block_sum_store_d(s, partial + blockIdx.x);
}
__global__ __launch_bounds__(256) void sumsq_final_kernel(const double* __restrict__ partial, int nb, double* __restrict__ out) {
    __shared__ double sh[256];
    double v = 0.0;
    for (int i = threadIdx.x; i < nb; i += 256) v += partial[i];
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = sh[0];
}

// one workgroup per range (the per-tensor norms of tf.keras clipping when every range is one tensor), fixed order
__global__ __launch_bounds__(256) void sumsq_each_range_kernel(const float* __restrict__ g, const float* __restrict__ scale, long long n,
                                                               const RangeRow* __restrict__ t, double* __restrict__ out) {
    const long long lo = t[blockIdx.x].begin;
    const long long hi = t[blockIdx.x].end < n ? t[blockIdx.x].end : n;
    double s = 0.0;
    long long i = (lo > 0 ? lo : 0) + threadIdx.x;
    // one workgroup walks a whole tensor, so the loop is bound by load latency: eight loads in flight, added in the order of the plain loop
    for (; i + 7 * 256 < hi; i += 8 * 256) {
        float a[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) a[k] = g[i + k * 256] * (scale ? scale[i + k * 256] : 1.f);
#pragma unroll
        for (int k = 0; k < 8; ++k) s += (double)a[k] * (double)a[k];
    }
    for (; i < hi; i += 256) {
        const float v = g[i] * (scale ? scale[i] : 1.f);
        s += (double)v * (double)v;
    }
    block_sum_store_d(s, out + blockIdx.x);
}

__device__ __forceinline__ float range_clip(const double* __restrict__ sumsq, int idx, float clipnorm, float grad_mul) {
    if (!(clipnorm > 0.f) || !sumsq) return 1.f;
    const float norm = sqrtf((float)sumsq[idx]) * fabsf(grad_mul);
    return norm > clipnorm ? clipnorm / norm : 1.f;
}

// the Adam update of one element; gi is the scaled and clipped gradient
struct AdamElem { float m, v, w; };
__device__ __forceinline__ AdamElem adam_elem(float gi, float m, float v, float w, float lr_t, float b1, float b2, float eps) {
    AdamElem e;
    e.m = b1 * m + (1.f - b1) * gi;
    e.v = b2 * v + (1.f - b2) * gi * gi;
    e.w = w - lr_t * e.m / (sqrtf(e.v) + eps);
    return e;
}

template <int ES>
__device__ __forceinline__ void store_fwd(char* __restrict__ w_fwd, long long i, float wf) {
    if constexpr (ES == 2) {
        const __bf16 hb = (__bf16)wf;
        reinterpret_cast<unsigned short*>(w_fwd)[i] = __builtin_bit_cast(unsigned short, hb);
    } else {
        reinterpret_cast<float*>(w_fwd)[i] = wf;
    }
}

// PER: sumsq holds one sum per range (per-tensor clipping), else one global sum.
template <int ES, bool VEC, bool PER>
__global__ __launch_bounds__(256) void adam_ranges_kernel(float* __restrict__ w, float* __restrict__ m, float* __restrict__ v,
                                                          const float* __restrict__ g, const float* __restrict__ gscale,
                                                          const float* __restrict__ fold, char* __restrict__ w_fwd, long long n,
                                                          const RangeRow* __restrict__ t, int nr, long long span, float lr_t,
                                                          float b1, float b2, float eps, const double* __restrict__ sumsq, float clipnorm,
                                                          float grad_mul) {
    const float clip_all = PER ? 1.f : range_clip(sumsq, 0, clipnorm, grad_mul);
    const long long nq = (span + 3) >> 2;
    for (long long qi = (long long)blockIdx.x * blockDim.x + threadIdx.x; qi < nq; qi += (long long)gridDim.x * blockDim.x) {
        const long long q = qi << 2;
        int r = range_of(t, nr, q);
        const long long off = q - t[r].vbegin, f0 = t[r].begin + off;
        if (VEC && off >= 0 && off + 4 <= t[r].end - t[r].begin && (f0 & 3) == 0 && f0 >= 0 && f0 + 4 <= n) {
            const float clip = PER ? range_clip(sumsq, r, clipnorm, grad_mul) : clip_all;
            const float4 gv = *reinterpret_cast<const float4*>(g + f0);
            const float4 sv = gscale ? *reinterpret_cast<const float4*>(gscale + f0) : make_float4(1.f, 1.f, 1.f, 1.f);
            const float4 fv = fold ? *reinterpret_cast<const float4*>(fold + f0) : make_float4(1.f, 1.f, 1.f, 1.f);
            float4 mv = *reinterpret_cast<const float4*>(m + f0);
            float4 vv = *reinterpret_cast<const float4*>(v + f0);
            float4 wv = *reinterpret_cast<const float4*>(w + f0);
            float gg[4] = {gv.x, gv.y, gv.z, gv.w}, ss[4] = {sv.x, sv.y, sv.z, sv.w}, ff[4] = {fv.x, fv.y, fv.z, fv.w};
            float mm[4] = {mv.x, mv.y, mv.z, mv.w}, vq[4] = {vv.x, vv.y, vv.z, vv.w}, ww[4] = {wv.x, wv.y, wv.z, wv.w};
            float wf[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const AdamElem e = adam_elem(gg[j] * ss[j] * grad_mul * clip, mm[j], vq[j], ww[j], lr_t, b1, b2, eps);
                mm[j] = e.m; vq[j] = e.v; ww[j] = e.w;
                wf[j] = e.w * ff[j];
            }
            *reinterpret_cast<float4*>(m + f0) = make_float4(mm[0], mm[1], mm[2], mm[3]);
            *reinterpret_cast<float4*>(v + f0) = make_float4(vq[0], vq[1], vq[2], vq[3]);
            *reinterpret_cast<float4*>(w + f0) = make_float4(ww[0], ww[1], ww[2], ww[3]);
            if (w_fwd) {
                if constexpr (ES == 2) {
                    unsigned short hb[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) hb[j] = __builtin_bit_cast(unsigned short, (__bf16)wf[j]);
                    *reinterpret_cast<uint2*>(w_fwd + f0 * 2) = make_uint2((unsigned)hb[0] | ((unsigned)hb[1] << 16),
                                                                           (unsigned)hb[2] | ((unsigned)hb[3] << 16));
                } else {
                    *reinterpret_cast<float4*>(w_fwd + f0 * 4) = make_float4(wf[0], wf[1], wf[2], wf[3]);
                }
            }
            continue;
        }
        for (int j = 0; j < 4; ++j) {
            const long long i = range_flat(t, nr, q + j, r, n);
            if (i < 0) continue;
            const float clip = PER ? range_clip(sumsq, r, clipnorm, grad_mul) : clip_all;
            const AdamElem e = adam_elem(g[i] * (gscale ? gscale[i] : 1.f) * grad_mul * clip, m[i], v[i], w[i], lr_t, b1, b2, eps);
            m[i] = e.m; v[i] = e.v; w[i] = e.w;
            if (w_fwd) store_fwd<ES>(w_fwd, i, e.w * (fold ? fold[i] : 1.f));
        }
    }
}

}  // namespace

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static int check_ranges(rtn_handle_t h, const char* what, const float* g, int64_t n, const int64_t* table_dev, int nr, int64_t span) {
    if (!g || n < 1 || nr < 0 || span < 0 || (nr > 0 && !table_dev) || (nr == 0 && span != 0))
        return rtn_fail(h, RTN_EINVAL, "%s: bad argument (n %lld, %d ranges, span %lld)", what, (long long)n, nr, (long long)span);
    return RTN_OK;
}

// Keras 2: lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t)
static float adam_lr_t(float lr, float beta1, float beta2, int64_t step) {
    return (float)((double)lr * sqrt(1.0 - pow((double)beta2, (double)step)) / (1.0 - pow((double)beta1, (double)step)));
}

extern "C" size_t rtn_sumsq_workspace_bytes(void) { return 2048 * sizeof(double); }

extern "C" int rtn_sumsq_ranges(rtn_handle_t h, const float* g, const float* scale, int64_t n, const int64_t* table_dev, int nr,
                                int64_t span, double* out, double* out_each, void* workspace, size_t workspace_bytes) {
    if (!h) return RTN_EINVAL;
    if (int e = check_ranges(h, "sumsq_ranges", g, n, table_dev, nr, span)) return e;
    if (out && (!workspace || workspace_bytes < rtn_sumsq_workspace_bytes())) return rtn_fail(h, RTN_ENOMEM, "sumsq_ranges: workspace too small");
    const RangeRow* t = (const RangeRow*)table_dev;
    if (out) {
        unsigned nb = 0;                                   // no ranges: the final kernel writes 0
        if (span > 0) {
            nb = rtn_grid_for((span + 3) / 4, 2048);
            if (aligned16(g) && (!scale || aligned16(scale)))
                hipLaunchKernelGGL((sumsq_ranges_kernel<true>), dim3(nb), dim3(256), 0, h->stream, g, scale, (long long)n, t, nr, (long long)span, (double*)workspace);
            else
                hipLaunchKernelGGL((sumsq_ranges_kernel<false>), dim3(nb), dim3(256), 0, h->stream, g, scale, (long long)n, t, nr, (long long)span, (double*)workspace);
            RTN_CHECK_LAUNCH(h, "sumsq_ranges_kernel");
        }
        hipLaunchKernelGGL(sumsq_final_kernel, dim3(1), dim3(256), 0, h->stream, (const double*)workspace, (int)nb, out);
        RTN_CHECK_LAUNCH(h, "sumsq_final_kernel");
    }
    if (out_each && nr > 0) {
        hipLaunchKernelGGL(sumsq_each_range_kernel, dim3((unsigned)nr), dim3(256), 0, h->stream, g, scale, (long long)n, t, out_each);
        RTN_CHECK_LAUNCH(h, "sumsq_each_range_kernel");
    }
    return RTN_OK;
}

template <bool PER>
static int adam_ranges_launch(rtn_handle_t h, float* w, float* m, float* v, const float* g, const float* gscale, const float* fold,
                              void* w_fwd, int fwd_dtype, int64_t n, const int64_t* table_dev, int nr, int64_t span, int64_t step,
                              float lr, float beta1, float beta2, float eps, const double* sumsq, float clipnorm, float grad_mul) {
    if (!h) return RTN_EINVAL;
    if (int e = check_ranges(h, "adam_ranges", g, n, table_dev, nr, span)) return e;
    if (!w || !m || !v || step < 1) return rtn_fail(h, RTN_EINVAL, "adam_ranges: bad argument");
    if (PER && !sumsq && clipnorm > 0.f) return rtn_fail(h, RTN_EINVAL, "adam_ranges: per-range sums missing");
    if (w_fwd && fwd_dtype != RTN_BF16 && fwd_dtype != RTN_F32) return rtn_fail(h, RTN_EINVAL, "adam_ranges: bad forward dtype");
    if (span == 0) return RTN_OK;
    const float lr_t = adam_lr_t(lr, beta1, beta2, step);
    const unsigned nb = rtn_grid_for((span + 3) / 4, 4096);
    const bool vec = aligned16(w) && aligned16(m) && aligned16(v) && aligned16(g) && (!gscale || aligned16(gscale)) &&
                     (!fold || aligned16(fold)) && (!w_fwd || ((uintptr_t)w_fwd & (fwd_dtype == RTN_BF16 ? 7 : 15)) == 0);
    const RangeRow* t = (const RangeRow*)table_dev;
#define RTN_ADAM_RANGES(ES, VEC) hipLaunchKernelGGL((adam_ranges_kernel<ES, VEC, PER>), dim3(nb), dim3(256), 0, h->stream, w, m, v, g, gscale, \
        fold, (char*)w_fwd, (long long)n, t, nr, (long long)span, lr_t, beta1, beta2, eps, sumsq, clipnorm, grad_mul)
    if (fwd_dtype == RTN_BF16) { if (vec) RTN_ADAM_RANGES(2, true); else RTN_ADAM_RANGES(2, false); }
    else                       { if (vec) RTN_ADAM_RANGES(4, true); else RTN_ADAM_RANGES(4, false); }
#undef RTN_ADAM_RANGES
    RTN_CHECK_LAUNCH(h, "adam_ranges_kernel");
    return RTN_OK;
}

extern "C" int rtn_adam_clipnorm_step_ranges(rtn_handle_t h, float* w, float* m, float* v, const float* g, const float* gscale,
                                             const float* fold, void* w_fwd, int fwd_dtype, int64_t n, const int64_t* table_dev, int nr,
                                             int64_t span, int64_t step, float lr, float beta1, float beta2, float eps,
                                             const double* sumsq, float clipnorm, float grad_mul) {
    return adam_ranges_launch<false>(h, w, m, v, g, gscale, fold, w_fwd, fwd_dtype, n, table_dev, nr, span, step, lr, beta1, beta2, eps,
                                     sumsq, clipnorm, grad_mul);
}

extern "C" int rtn_adam_clipnorm_step_ranges_pertensor(rtn_handle_t h, float* w, float* m, float* v, const float* g, const float* gscale,
                                                       const float* fold, void* w_fwd, int fwd_dtype, int64_t n, const int64_t* table_dev,
                                                       int nr, int64_t span, int64_t step, float lr, float beta1, float beta2, float eps,
                                                       const double* sumsq_each, float clipnorm, float grad_mul) {
    return adam_ranges_launch<true>(h, w, m, v, g, gscale, fold, w_fwd, fwd_dtype, n, table_dev, nr, span, step, lr, beta1, beta2, eps,
                                    sumsq_each, clipnorm, grad_mul);
}
