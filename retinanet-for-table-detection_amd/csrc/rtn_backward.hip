// rtn_backward.hip — the small kernels of the backward pass (RetinaNet.py:125-131,280: Keras compile + fit_generator => TF
// autodiff).  The weight gradients are in rtn_wgrad.hip / rtn_wgrad_win.hip, the data gradient in rtn_conv.hip (rtn_conv2d_dgrad),
// the optimizer in rtn_optimizer.hip.
//
//   rtn_bias_grad         db[n] += sum_pixels dY[pix][n]
//   rtn_zero_insert2      dY -> zero-inserted dY for the data gradient of the stride-2 3x3 convs (P6, P7)
//   rtn_upsample_add_bwd  adjoint of UpsampleLike (legacy-TF nearest) + Add  (model/layers.py:89-98)
//   rtn_maxpool3x3s2_tfsame_fwd_idx / _bwd_idx / _bwd
//   rtn_pad_cast_rows     f32 loss gradients -> the padded dY of the head outputs
#include "rtn_internal.h"

namespace {

template <int ES>
__global__ __launch_bounds__(256) void bias_grad_kernel(const char* __restrict__ dy, long long rows, int N, long long ld_b,
                                                        float* __restrict__ db) {
    // thread = (16-byte chunk column c, row lane r); rows are strided over row lanes and blocks; the row lanes of a block are
    // summed through LDS so that each block issues ONE atomic per channel (same-address atomics serialise).
    constexpr int CE = 16 / ES;
    __shared__ float sh[256 * CE];
    const int nch = (N + CE - 1) / CE;
    const int RP = 256 / nch;                          // row lanes per block (host guarantees nch <= 256)
    const int c = threadIdx.x % nch, r = threadIdx.x / nch;
    float s[CE];
#pragma unroll
    for (int j = 0; j < CE; ++j) s[j] = 0.f;
    if (r < RP) {
        const long long step = (long long)gridDim.x * RP;
        for (long long row = (long long)blockIdx.x * RP + r; row < rows; row += 8 * step) {
            uint4 q[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {                 // 8 independent row loads in flight (rows past the end: zeros)
                const long long rr = row + u * step;
                q[u] = rr < rows ? *reinterpret_cast<const uint4*>(dy + rr * ld_b + (long long)c * 16) : make_uint4(0, 0, 0, 0);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const unsigned w4[4] = {q[u].x, q[u].y, q[u].z, q[u].w};
                if constexpr (ES == 2) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        s[2 * j] += __uint_as_float(w4[j] << 16);
                        s[2 * j + 1] += __uint_as_float(w4[j] & 0xffff0000u);
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) s[j] += __uint_as_float(w4[j]);
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < CE; ++j) sh[threadIdx.x * CE + j] = s[j];
    __syncthreads();
    if (threadIdx.x < nch) {
#pragma unroll
        for (int j = 0; j < CE; ++j) {
            float v = 0.f;
            for (int rr = 0; rr < RP; ++rr) v += sh[(threadIdx.x + rr * nch) * CE + j];
            if (threadIdx.x * CE + j < N) unsafeAtomicAdd(db + threadIdx.x * CE + j, v);
        }
    }
}

// out[b][2*oy][2*ox][:] = in[b][oy][ox][:], zeros elsewhere; out is [B][Hu][Wu][C]
__global__ __launch_bounds__(256) void zero_insert2_kernel(const uint4* __restrict__ in, uint4* __restrict__ out, int B, int H, int W,
                                                           int Hu, int Wu, int cv) {
    const long long total = (long long)B * Hu * Wu * cv;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % cv);
        long long r = i / cv;
        const int x = (int)(r % Wu);
        r /= Wu;
        const int y = (int)(r % Hu);
        const int b = (int)(r / Hu);
        uint4 v = make_uint4(0, 0, 0, 0);
        if (!(x & 1) && !(y & 1) && (y >> 1) < H && (x >> 1) < W) v = in[(((long long)b * H + (y >> 1)) * W + (x >> 1)) * cv + c];
        out[i] = v;
    }
}

// d_src[b][sy][sx][:] (+)= sum over destination pixels (y,x) with floor(y*rh)==sy (clamped) && floor(x*rw)==sx of d_dst
template <int ES>
__global__ __launch_bounds__(256) void upsample_add_bwd_kernel(const char* __restrict__ d_dst, char* __restrict__ d_src, int B,
                                                               int Hd, int Wd, int Hs, int Ws, int C, float rh, float rw, int accumulate) {
    constexpr int CE = 16 / ES;
    const int cv = C / CE;
    const long long total = (long long)B * Hs * Ws * cv;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % cv);
        long long r = i / cv;
        const int sx = (int)(r % Ws);
        r /= Ws;
        const int sy = (int)(r % Hs);
        const int b = (int)(r / Hs);
        float s[CE];
#pragma unroll
        for (int j = 0; j < CE; ++j) s[j] = 0.f;
        // candidate destination rows: the preimage of sy under y -> min(floor(y*rh), Hs-1) is a short contiguous run
        int y0 = (int)floorf((float)sy / rh) - 1; if (y0 < 0) y0 = 0;
        int x0 = (int)floorf((float)sx / rw) - 1; if (x0 < 0) x0 = 0;
        for (int y = y0; y < Hd; ++y) {
            int my = (int)floorf((float)y * rh); my = my < Hs - 1 ? my : Hs - 1;
            if (my < sy) continue;
            if (my > sy) break;
            for (int x = x0; x < Wd; ++x) {
                int mx = (int)floorf((float)x * rw); mx = mx < Ws - 1 ? mx : Ws - 1;
                if (mx < sx) continue;
                if (mx > sx) break;
                const uint4 q = *reinterpret_cast<const uint4*>(d_dst + ((((long long)b * Hd + y) * Wd + x) * C + c * CE) * ES);
                const unsigned w4[4] = {q.x, q.y, q.z, q.w};
                if constexpr (ES == 2) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) { s[2 * j] += __uint_as_float(w4[j] << 16); s[2 * j + 1] += __uint_as_float(w4[j] & 0xffff0000u); }
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) s[j] += __uint_as_float(w4[j]);
                }
            }
        }
        char* op = d_src + i * 16;
        if (accumulate) {
            const uint4 q = *reinterpret_cast<const uint4*>(op);
            const unsigned w4[4] = {q.x, q.y, q.z, q.w};
            if constexpr (ES == 2) {
#pragma unroll
                for (int j = 0; j < 4; ++j) { s[2 * j] += __uint_as_float(w4[j] << 16); s[2 * j + 1] += __uint_as_float(w4[j] & 0xffff0000u); }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) s[j] += __uint_as_float(w4[j]);
            }
        }
        uint4 o;
        if constexpr (ES == 2) {
            typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
            unsigned w[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) { bf16x2 v = {(__bf16)s[2 * j], (__bf16)s[2 * j + 1]}; w[j] = __builtin_bit_cast(unsigned, v); }
            o = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
            o = make_uint4(__float_as_uint(s[0]), __float_as_uint(s[1]), __float_as_uint(s[2]), __float_as_uint(s[3]));
        }
        *reinterpret_cast<uint4*>(op) = o;
    }
}

// Training-mode max-pool: also records which of the 9 window taps (kh*3+kw, first maximum in scan order — TF MaxPoolGrad's
// choice) won, one byte per output element, so that the backward pass is a gather with no atomics.
template <int ES>
__global__ __launch_bounds__(256) void maxpool_fwd_idx_kernel(const char* __restrict__ in, char* __restrict__ out,
                                                              unsigned char* __restrict__ idx, int B, int Hin, int Win, int C, int Hout,
                                                              int Wout, int pad_t, int pad_l) {
    constexpr int CE = 16 / ES;
    const int cv = C / CE;
    const long long total = (long long)B * Hout * Wout * cv;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int cc = (int)(i % cv);
        long long r = i / cv;
        const int ox = (int)(r % Wout);
        r /= Wout;
        const int oy = (int)(r % Hout);
        const int b = (int)(r / Hout);
        float mx[CE];
        unsigned char am[CE];
#pragma unroll
        for (int j = 0; j < CE; ++j) { mx[j] = -INFINITY; am[j] = 255; }
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
            const int iy = oy * 2 - pad_t + kh;
            if ((unsigned)iy >= (unsigned)Hin) continue;
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int ix = ox * 2 - pad_l + kw;
                if ((unsigned)ix >= (unsigned)Win) continue;
                const uint4 q = *reinterpret_cast<const uint4*>(in + ((((long long)b * Hin + iy) * Win + ix) * C + cc * CE) * ES);
                const unsigned w4[4] = {q.x, q.y, q.z, q.w};
                float v[CE];
                if constexpr (ES == 2) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) { v[2 * j] = __uint_as_float(w4[j] << 16); v[2 * j + 1] = __uint_as_float(w4[j] & 0xffff0000u); }
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = __uint_as_float(w4[j]);
                }
#pragma unroll
                for (int j = 0; j < CE; ++j)
                    if (v[j] > mx[j]) { mx[j] = v[j]; am[j] = (unsigned char)(kh * 3 + kw); }
            }
        }
        uint4 o;
        if constexpr (ES == 2) {
            o.x = (__float_as_uint(mx[0]) >> 16) | (__float_as_uint(mx[1]) & 0xffff0000u);
            o.y = (__float_as_uint(mx[2]) >> 16) | (__float_as_uint(mx[3]) & 0xffff0000u);
            o.z = (__float_as_uint(mx[4]) >> 16) | (__float_as_uint(mx[5]) & 0xffff0000u);
            o.w = (__float_as_uint(mx[6]) >> 16) | (__float_as_uint(mx[7]) & 0xffff0000u);
        } else {
            o = make_uint4(__float_as_uint(mx[0]), __float_as_uint(mx[1]), __float_as_uint(mx[2]), __float_as_uint(mx[3]));
        }
        *reinterpret_cast<uint4*>(out + i * 16) = o;
#pragma unroll
        for (int j = 0; j < CE; ++j) idx[i * CE + j] = am[j];
    }
}

// dx[b][iy][ix][c] = sum over the (at most 4) windows containing (iy,ix) whose recorded winner is this tap of dy,
// zeroed where x <= 0 when relu_mask (x is a ReLU output).
template <int ES>
__global__ __launch_bounds__(256) void maxpool_bwd_idx_kernel(const char* __restrict__ dy, const unsigned char* __restrict__ idx,
                                                              const char* __restrict__ x, char* __restrict__ dx, int B, int Hin, int Win,
                                                              int C, int Hout, int Wout, int pad_t, int pad_l, int relu_mask) {
    constexpr int CE = 16 / ES;
    const int cv = C / CE;
    // grid: x = 16-byte items of an image row, y = image rows of the batch (strided).  One 32-bit division per item: the three 64-bit
    // ones of the flat index were a third of the kernel's time (0.32 -> 0.2x ms at batch 16, last kernel but one of the backward pass).
    const unsigned jrow = blockIdx.x * blockDim.x + threadIdx.x;
    if (jrow >= (unsigned)(Win * cv)) return;
    const int ix = (int)(jrow / (unsigned)cv), cc = (int)(jrow - (unsigned)ix * (unsigned)cv);
    for (int row = blockIdx.y; row < B * Hin; row += gridDim.y) {
        const int b = row / Hin, iy = row - b * Hin;
        const long long i = (long long)row * Win * cv + jrow;
        float s[CE];
#pragma unroll
        for (int j = 0; j < CE; ++j) s[j] = 0.f;
        // windows oy with oy*2 - pad_t <= iy <= oy*2 - pad_t + 2
        const int ty = iy + pad_t, tx = ix + pad_l;
        for (int oy = (ty - 2 + 1) >> 1; oy <= (ty >> 1); ++oy) {
            if (oy < 0 || oy >= Hout) continue;
            const int kh = ty - 2 * oy;
            for (int ox = (tx - 2 + 1) >> 1; ox <= (tx >> 1); ++ox) {
                if (ox < 0 || ox >= Wout) continue;
                const int kw = tx - 2 * ox;
                const unsigned char tap = (unsigned char)(kh * 3 + kw);
                const long long o = (((long long)b * Hout + oy) * Wout + ox) * cv + cc;
                const uint4 gq = *reinterpret_cast<const uint4*>(dy + o * 16);
                const unsigned g4[4] = {gq.x, gq.y, gq.z, gq.w};
                const unsigned char* ip = idx + o * CE;
                // relu_mask == 2: x is the POOLED tensor: the winner's value IS the window's maximum, so "x > 0 at the winner" is
                // "pooled > 0" (the fused stem kernel never writes the pre-pool tensor)
                uint4 yq = make_uint4(0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u);
                if (relu_mask == 2) yq = *reinterpret_cast<const uint4*>(x + o * 16);
                const unsigned y4[4] = {yq.x, yq.y, yq.z, yq.w};
                if constexpr (ES == 2) {
                    const uint2 iq = *reinterpret_cast<const uint2*>(ip);
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const unsigned char a = (unsigned char)(((j < 4 ? iq.x : iq.y) >> (8 * (j & 3))) & 0xffu);
                        const float g = (j & 1) ? __uint_as_float(g4[j >> 1] & 0xffff0000u) : __uint_as_float(g4[j >> 1] << 16);
                        const float yv = (j & 1) ? __uint_as_float(y4[j >> 1] & 0xffff0000u) : __uint_as_float(y4[j >> 1] << 16);
                        if (a == tap && yv > 0.f) s[j] += g;
                    }
                } else {
                    const unsigned iq = *reinterpret_cast<const unsigned*>(ip);
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if ((unsigned char)((iq >> (8 * j)) & 0xffu) == tap && (relu_mask != 2 || __uint_as_float(y4[j]) > 0.f)) s[j] += __uint_as_float(g4[j]);
                }
            }
        }
        if (relu_mask == 1) {
            const uint4 xq = *reinterpret_cast<const uint4*>(x + i * 16);
            const unsigned x4[4] = {xq.x, xq.y, xq.z, xq.w};
            if constexpr (ES == 2) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float xv = (j & 1) ? __uint_as_float(x4[j >> 1] & 0xffff0000u) : __uint_as_float(x4[j >> 1] << 16);
                    if (!(xv > 0.f)) s[j] = 0.f;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (!(__uint_as_float(x4[j]) > 0.f)) s[j] = 0.f;
            }
        }
        uint4 o;
        if constexpr (ES == 2) {
            typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
            unsigned w[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) { bf16x2 v = {(__bf16)s[2 * j], (__bf16)s[2 * j + 1]}; w[j] = __builtin_bit_cast(unsigned, v); }
            o = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
            o = make_uint4(__float_as_uint(s[0]), __float_as_uint(s[1]), __float_as_uint(s[2]), __float_as_uint(s[3]));
        }
        *reinterpret_cast<uint4*>(dx + i * 16) = o;
    }
}

// gradient goes to the first window position (row-major scan) holding the maximum — TF MaxPoolGrad's choice
template <int ES>
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const char* __restrict__ x, const char* __restrict__ dy, float* __restrict__ dx32,
                                                          int B, int Hin, int Win, int C, int Hout, int Wout, int pad_t, int pad_l) {
    constexpr int CE = 16 / ES;
    const int cv = C / CE;
    const long long total = (long long)B * Hout * Wout * cv;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int cc = (int)(i % cv);
        long long r = i / cv;
        const int ox = (int)(r % Wout);
        r /= Wout;
        const int oy = (int)(r % Hout);
        const int b = (int)(r / Hout);
        float mx[CE];
        int arg[CE];
#pragma unroll
        for (int j = 0; j < CE; ++j) { mx[j] = -INFINITY; arg[j] = -1; }
        for (int kh = 0; kh < 3; ++kh) {
            const int iy = oy * 2 - pad_t + kh;
            if ((unsigned)iy >= (unsigned)Hin) continue;
            for (int kw = 0; kw < 3; ++kw) {
                const int ix = ox * 2 - pad_l + kw;
                if ((unsigned)ix >= (unsigned)Win) continue;
                const int pix = iy * Win + ix;
                const uint4 q = *reinterpret_cast<const uint4*>(x + (((long long)b * Hin * Win + pix) * C + cc * CE) * ES);
                const unsigned w4[4] = {q.x, q.y, q.z, q.w};
                float v[CE];
                if constexpr (ES == 2) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) { v[2 * j] = __uint_as_float(w4[j] << 16); v[2 * j + 1] = __uint_as_float(w4[j] & 0xffff0000u); }
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = __uint_as_float(w4[j]);
                }
#pragma unroll
                for (int j = 0; j < CE; ++j)
                    if (v[j] > mx[j]) { mx[j] = v[j]; arg[j] = pix; }
            }
        }
        const uint4 gq = *reinterpret_cast<const uint4*>(dy + i * 16);
        const unsigned g4[4] = {gq.x, gq.y, gq.z, gq.w};
        float g[CE];
        if constexpr (ES == 2) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { g[2 * j] = __uint_as_float(g4[j] << 16); g[2 * j + 1] = __uint_as_float(g4[j] & 0xffff0000u); }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) g[j] = __uint_as_float(g4[j]);
        }
#pragma unroll
        for (int j = 0; j < CE; ++j)
            if (arg[j] >= 0 && g[j] != 0.f)
                unsafeAtomicAdd(dx32 + ((long long)b * Hin * Win + arg[j]) * C + cc * CE + j, g[j]);
    }
}

template <int ES>
__global__ __launch_bounds__(256) void cast_from_f32_kernel(const float* __restrict__ in, char* __restrict__ out, long long n,
                                                            const char* __restrict__ relu_src) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        float val = in[i];
        if (relu_src) {
            float xv;
            if constexpr (ES == 2) xv = __uint_as_float(((unsigned)reinterpret_cast<const unsigned short*>(relu_src)[i]) << 16);
            else xv = reinterpret_cast<const float*>(relu_src)[i];
            if (!(xv > 0.f)) val = 0.f;
        }
        if constexpr (ES == 2) {
            const __bf16 hb = (__bf16)val;
            reinterpret_cast<unsigned short*>(out)[i] = __builtin_bit_cast(unsigned short, hb);
        } else {
            reinterpret_cast<float*>(out)[i] = val;
        }
    }
}

// out[r][0..cout) = cast(in[r][0..cin)), zero for c >= cin   (f32 loss gradients -> 64-channel dY of the head outputs)
template <int ES>
__global__ __launch_bounds__(256) void pad_cast_rows_kernel(const float* __restrict__ in, char* __restrict__ out, long long rows,
                                                            int cin, int cout) {
    const long long total = rows * cout;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / cout;
        const int c = (int)(i - r * cout);
        const float v = c < cin ? in[r * cin + c] : 0.f;
        if constexpr (ES == 2) {
            const __bf16 hb = (__bf16)v;
            reinterpret_cast<unsigned short*>(out)[i] = __builtin_bit_cast(unsigned short, hb);
        } else {
            reinterpret_cast<float*>(out)[i] = v;
        }
    }
}

// bf16, cout a multiple of 8, 16-byte aligned out: one thread = 8 consecutive columns of a row (one 16-byte store instead of eight
// 2-byte ones; 32-bit index arithmetic)
__global__ __launch_bounds__(256) void pad_cast_rows8_kernel(const float* __restrict__ in, uint4* __restrict__ out, unsigned items,
                                                             int cin, int cg) {
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < items; i += gridDim.x * blockDim.x) {
        const unsigned r = i / (unsigned)cg;
        const int c0 = (int)(i - r * (unsigned)cg) * 8;
        const float* src = in + (long long)r * cin;
        unsigned w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float a = c0 + 2 * j < cin ? src[c0 + 2 * j] : 0.f, b = c0 + 2 * j + 1 < cin ? src[c0 + 2 * j + 1] : 0.f;
            typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
            const bf16x2 v = {(__bf16)a, (__bf16)b};
            w[j] = __builtin_bit_cast(unsigned, v);
        }
        out[i] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

}  // namespace

extern "C" int rtn_bias_grad(rtn_handle_t h, const void* dy, int dtype, int64_t rows, int N, int64_t ld, float* db) {
    if (!h) return RTN_EINVAL;
    if (!dy || !db || rows < 1 || N < 1 || ld < N) return rtn_fail(h, RTN_EINVAL, "bias_grad: bad argument");
    if (dtype != RTN_BF16 && dtype != RTN_F32) return rtn_fail(h, RTN_EINVAL, "bias_grad: bad dtype");
    const int es = rtn_dtype_size(dtype);
    if ((ld * es) % 16 || ((uintptr_t)dy & 15)) return rtn_fail(h, RTN_EINVAL, "bias_grad: ld/pointer not 16-byte aligned");
    const int ce = 16 / es, nch = (N + ce - 1) / ce;
    if ((long long)nch * ce > ld) return rtn_fail(h, RTN_EINVAL, "bias_grad: last chunk leaves the row");
    if (nch > 256) return rtn_fail(h, RTN_EINVAL, "bias_grad: N %d too wide", N);
    const int rp = 256 / nch;
    long long blocks = (rows + (long long)rp * 32 - 1) / ((long long)rp * 32);     // ~32 rows per row lane
    if (blocks < 1) blocks = 1;
    if (blocks > 1024) blocks = 1024;
    if (es == 2) hipLaunchKernelGGL((bias_grad_kernel<2>), dim3((unsigned)blocks), dim3(256), 0, h->stream, (const char*)dy, (long long)rows, N, (long long)ld * es, db);
    else         hipLaunchKernelGGL((bias_grad_kernel<4>), dim3((unsigned)blocks), dim3(256), 0, h->stream, (const char*)dy, (long long)rows, N, (long long)ld * es, db);
    RTN_CHECK_LAUNCH(h, "bias_grad_kernel");
    return RTN_OK;
}

extern "C" int rtn_zero_insert2(rtn_handle_t h, const void* in, void* out, int dtype, int B, int H, int W, int C, int Hu, int Wu) {
    if (!h) return RTN_EINVAL;
    if (!in || !out || B < 1 || H < 1 || W < 1 || C < 1) return rtn_fail(h, RTN_EINVAL, "zero_insert2: bad argument");
    if (dtype != RTN_BF16 && dtype != RTN_F32) return rtn_fail(h, RTN_EINVAL, "zero_insert2: bad dtype");
    const int es = rtn_dtype_size(dtype);
    if ((C * es) % 16 || ((uintptr_t)in & 15) || ((uintptr_t)out & 15)) return rtn_fail(h, RTN_EINVAL, "zero_insert2: alignment");
    if (Hu < 2 * H - 1 || Wu < 2 * W - 1) return rtn_fail(h, RTN_EINVAL, "zero_insert2: %dx%d too small for %dx%d", Hu, Wu, H, W);
    const int cv = C * es / 16;
    hipLaunchKernelGGL(zero_insert2_kernel, dim3(rtn_grid_for((long long)B * Hu * Wu * cv)), dim3(256), 0, h->stream, (const uint4*)in, (uint4*)out, B, H, W, Hu, Wu, cv);
    RTN_CHECK_LAUNCH(h, "zero_insert2_kernel");
    return RTN_OK;
}

extern "C" int rtn_upsample_add_bwd(rtn_handle_t h, const void* d_dst, void* d_src, int dtype, int B, int Hd, int Wd, int Hs, int Ws,
                                    int C, int accumulate) {
    if (!h) return RTN_EINVAL;
    if (!d_dst || !d_src || B < 1 || Hd < 1 || Wd < 1 || Hs < 1 || Ws < 1 || C < 1) return rtn_fail(h, RTN_EINVAL, "upsample_add_bwd: bad argument");
    if (dtype != RTN_BF16 && dtype != RTN_F32) return rtn_fail(h, RTN_EINVAL, "upsample_add_bwd: bad dtype");
    const int es = rtn_dtype_size(dtype);
    if ((C * es) % 16 || ((uintptr_t)d_dst & 15) || ((uintptr_t)d_src & 15)) return rtn_fail(h, RTN_EINVAL, "upsample_add_bwd: alignment");
    const float rh = (float)Hs / (float)Hd, rw = (float)Ws / (float)Wd;
    const long long total = (long long)B * Hs * Ws * (C * es / 16);
    if (es == 2) hipLaunchKernelGGL((upsample_add_bwd_kernel<2>), dim3(rtn_grid_for(total)), dim3(256), 0, h->stream, (const char*)d_dst, (char*)d_src, B, Hd, Wd, Hs, Ws, C, rh, rw, accumulate);
    else         hipLaunchKernelGGL((upsample_add_bwd_kernel<4>), dim3(rtn_grid_for(total)), dim3(256), 0, h->stream, (const char*)d_dst, (char*)d_src, B, Hd, Wd, Hs, Ws, C, rh, rw, accumulate);
    RTN_CHECK_LAUNCH(h, "upsample_add_bwd_kernel");
    return RTN_OK;
}

extern "C" int rtn_maxpool3x3s2_tfsame_bwd(rtn_handle_t h, const void* x, const void* dy, void* dx, int dtype, int B, int Hin, int Win,
                                           int C, float* scratch_f32, int relu_mask) {
    if (!h) return RTN_EINVAL;
    if (!x || !dy || !dx || !scratch_f32 || B < 1 || Hin < 1 || Win < 1 || C < 1) return rtn_fail(h, RTN_EINVAL, "maxpool_bwd: bad argument");
    if (dtype != RTN_BF16 && dtype != RTN_F32) return rtn_fail(h, RTN_EINVAL, "maxpool_bwd: bad dtype");
    const int es = rtn_dtype_size(dtype);
    if ((C * es) % 16 || ((uintptr_t)x & 15) || ((uintptr_t)dy & 15)) return rtn_fail(h, RTN_EINVAL, "maxpool_bwd: alignment");
    const int Hout = (Hin + 1) / 2, Wout = (Win + 1) / 2;
    int pth = (Hout - 1) * 2 + 3 - Hin; if (pth < 0) pth = 0;
    int ptw = (Wout - 1) * 2 + 3 - Win; if (ptw < 0) ptw = 0;
    const long long nin = (long long)B * Hin * Win * C;
    RTN_HIP(h, hipMemsetAsync(scratch_f32, 0, (size_t)nin * 4, h->stream));
    const long long total = (long long)B * Hout * Wout * (C * es / 16);
    if (es == 2) hipLaunchKernelGGL((maxpool_bwd_kernel<2>), dim3(rtn_grid_for(total)), dim3(256), 0, h->stream, (const char*)x, (const char*)dy, scratch_f32, B, Hin, Win, C, Hout, Wout, pth / 2, ptw / 2);
    else         hipLaunchKernelGGL((maxpool_bwd_kernel<4>), dim3(rtn_grid_for(total)), dim3(256), 0, h->stream, (const char*)x, (const char*)dy, scratch_f32, B, Hin, Win, C, Hout, Wout, pth / 2, ptw / 2);
    RTN_CHECK_LAUNCH(h, "maxpool_bwd_kernel");
    if (es == 2) hipLaunchKernelGGL((cast_from_f32_kernel<2>), dim3(rtn_grid_for(nin)), dim3(256), 0, h->stream, (const float*)scratch_f32, (char*)dx, nin, relu_mask ? (const char*)x : (const char*)nullptr);
    else         hipLaunchKernelGGL((cast_from_f32_kernel<4>), dim3(rtn_grid_for(nin)), dim3(256), 0, h->stream, (const float*)scratch_f32, (char*)dx, nin, relu_mask ? (const char*)x : (const char*)nullptr);
    RTN_CHECK_LAUNCH(h, "cast_from_f32_kernel");
    return RTN_OK;
}

extern "C" int rtn_pad_cast_rows(rtn_handle_t h, const float* in, void* out, int dtype, int64_t rows, int cin, int cout) {
    if (!h) return RTN_EINVAL;
    if (!in || !out || rows < 1 || cin < 1 || cout < cin) return rtn_fail(h, RTN_EINVAL, "pad_cast_rows: bad argument");
    if (dtype != RTN_BF16 && dtype != RTN_F32) return rtn_fail(h, RTN_EINVAL, "pad_cast_rows: bad dtype");
    const unsigned nb = rtn_grid_for((long long)rows * cout);
    if (dtype == RTN_BF16 && cout % 8 == 0 && !((uintptr_t)out & 15) && (long long)rows * (cout / 8) < (1ll << 31)) {
        const long long items = (long long)rows * (cout / 8);
        hipLaunchKernelGGL(pad_cast_rows8_kernel, dim3(rtn_grid_for(items)), dim3(256), 0, h->stream, in, (uint4*)out, (unsigned)items, cin, cout / 8);
        RTN_CHECK_LAUNCH(h, "pad_cast_rows8_kernel");
        return RTN_OK;
    }
    if (dtype == RTN_BF16) hipLaunchKernelGGL((pad_cast_rows_kernel<2>), dim3(nb), dim3(256), 0, h->stream, in, (char*)out, (long long)rows, cin, cout);
    else                   hipLaunchKernelGGL((pad_cast_rows_kernel<4>), dim3(nb), dim3(256), 0, h->stream, in, (char*)out, (long long)rows, cin, cout);
    RTN_CHECK_LAUNCH(h, "pad_cast_rows_kernel");
    return RTN_OK;
}

extern "C" int rtn_maxpool3x3s2_tfsame_fwd_idx(rtn_handle_t h, const void* in, void* out, uint8_t* idx, int dtype, int B, int Hin,
                                               int Win, int C) {
    if (!h) return RTN_EINVAL;
    if (!in || !out || !idx || B < 1 || Hin < 1 || Win < 1 || C < 1) return rtn_fail(h, RTN_EINVAL, "maxpool_fwd_idx: bad argument");
    if (dtype != RTN_BF16 && dtype != RTN_F32) return rtn_fail(h, RTN_EINVAL, "maxpool_fwd_idx: bad dtype");
    const int es = rtn_dtype_size(dtype);
    if ((C * es) % 16 || ((uintptr_t)in & 15) || ((uintptr_t)out & 15) || ((uintptr_t)idx & 7)) return rtn_fail(h, RTN_EINVAL, "maxpool_fwd_idx: alignment");
    const int Hout = (Hin + 1) / 2, Wout = (Win + 1) / 2;
    int pth = (Hout - 1) * 2 + 3 - Hin; if (pth < 0) pth = 0;
    int ptw = (Wout - 1) * 2 + 3 - Win; if (ptw < 0) ptw = 0;
    const long long total = (long long)B * Hout * Wout * (C * es / 16);
    if (es == 2) hipLaunchKernelGGL((maxpool_fwd_idx_kernel<2>), dim3(rtn_grid_for(total)), dim3(256), 0, h->stream, (const char*)in, (char*)out, idx, B, Hin, Win, C, Hout, Wout, pth / 2, ptw / 2);
    else         hipLaunchKernelGGL((maxpool_fwd_idx_kernel<4>), dim3(rtn_grid_for(total)), dim3(256), 0, h->stream, (const char*)in, (char*)out, idx, B, Hin, Win, C, Hout, Wout, pth / 2, ptw / 2);
    RTN_CHECK_LAUNCH(h, "maxpool_fwd_idx_kernel");
    return RTN_OK;
}

extern "C" int rtn_maxpool3x3s2_tfsame_bwd_idx(rtn_handle_t h, const void* dy, const uint8_t* idx, const void* x, void* dx, int dtype,
                                               int B, int Hin, int Win, int C, int relu_mask) {
    if (!h) return RTN_EINVAL;
    if (!dy || !idx || !dx || (relu_mask && !x) || B < 1 || Hin < 1 || Win < 1 || C < 1) return rtn_fail(h, RTN_EINVAL, "maxpool_bwd_idx: bad argument");
    if (dtype != RTN_BF16 && dtype != RTN_F32) return rtn_fail(h, RTN_EINVAL, "maxpool_bwd_idx: bad dtype");
    const int es = rtn_dtype_size(dtype);
    if ((C * es) % 16 || ((uintptr_t)dy & 15) || ((uintptr_t)dx & 15) || ((uintptr_t)x & 15) || ((uintptr_t)idx & 7)) return rtn_fail(h, RTN_EINVAL, "maxpool_bwd_idx: alignment");
    const int Hout = (Hin + 1) / 2, Wout = (Win + 1) / 2;
    int pth = (Hout - 1) * 2 + 3 - Hin; if (pth < 0) pth = 0;
    int ptw = (Wout - 1) * 2 + 3 - Win; if (ptw < 0) ptw = 0;
    const long long row_items = (long long)Win * (C * es / 16), rows = (long long)B * Hin;
    if (row_items >= (1ll << 31) || rows >= (1ll << 31)) return rtn_fail(h, RTN_EINVAL, "maxpool_bwd_idx: extent");
    const dim3 grid((unsigned)((row_items + 255) / 256), (unsigned)(rows < 65535 ? rows : 65535));
    if (es == 2) hipLaunchKernelGGL((maxpool_bwd_idx_kernel<2>), grid, dim3(256), 0, h->stream, (const char*)dy, idx, (const char*)x, (char*)dx, B, Hin, Win, C, Hout, Wout, pth / 2, ptw / 2, relu_mask);
    else         hipLaunchKernelGGL((maxpool_bwd_idx_kernel<4>), grid, dim3(256), 0, h->stream, (const char*)dy, idx, (const char*)x, (char*)dx, B, Hin, Win, C, Hout, Wout, pth / 2, ptw / 2, relu_mask);
    RTN_CHECK_LAUNCH(h, "maxpool_bwd_idx_kernel");
    return RTN_OK;
}
