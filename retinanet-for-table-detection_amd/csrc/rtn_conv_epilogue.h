// rtn_conv_epilogue.h — the register epilogue of the persistent convolution kernels (rtn_conv_halo8.hip, rtn_conv_gemm8.hip):
//   [mask] [+ residual] [mask] -> ReLU -> bf16 -> guarded buffer store (a row past the tile or M goes to an out-of-range offset),
// one definition of the arithmetic and of every guarded store.  A lane holds NW consecutive channels of a pixel row (8: 16-byte
// accesses, 4: 8-byte); EPI: bit 0 = residual, bit 1 = mask.  What stays in the kernels: which rows they fetch when (how many
// fragments' residual / mask rows are in flight is tuned per kernel) and their address math.
#pragma once
#include "rtn_device.h"

// Buffer resource over [ptr, ptr + bytes); `on` false (an epilogue mode that is compiled out): 0 bytes over `dflt`, every load zeros.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t epi_rsrc(const void* ptr, unsigned bytes, bool on = true, const void* dflt = nullptr) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)(on ? ptr : dflt), 0, (int)__builtin_amdgcn_readfirstlane((int)(on ? bytes : 0u)), 0x00020000);
}

// Guarded stores (RTN_STORE_GUARD, rtn_device.h).  AUX: cache policy of the instruction (0, or 16 = sc1, write-through).
template <int AUX = 0>
__device__ __forceinline__ void epi_store16(const u32x4 o, __amdgpu_buffer_rsrc_t rsrc, unsigned off) {
    __builtin_amdgcn_raw_buffer_store_b128(o, rsrc, (int)off, 0, AUX);
    RTN_STORE_GUARD(o)
}
__device__ __forceinline__ void epi_store8(const u32x2 o, __amdgpu_buffer_rsrc_t rsrc, unsigned off) {
    __builtin_amdgcn_raw_buffer_store_b64(o, rsrc, (int)off, 0, 0);
    RTN_STORE_GUARD2(o)
}

// One residual / mask row of a lane: NW bf16 (the upper dwords of the 8-byte form are never read).
template <int NW>
__device__ __forceinline__ u32x4 epi_load_row(__amdgpu_buffer_rsrc_t rsrc, unsigned off) {
    if constexpr (NW == 8) return __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)off, 0, 0);
    else { const u32x2 t2 = __builtin_amdgcn_raw_buffer_load_b64(rsrc, (int)off, 0, 0); return (u32x4){t2.x, t2.y, 0u, 0u}; }
}

// v = [mask] v [+ residual] [mask]: the mask (keep where the masking tensor is > 0) before the add with `mask_pre`, else after it.
// The values are read into locals, selected and written back once: written as conditional stores into v[] the same arithmetic
// compiles, once inlined, into selects over the whole row and spills on the 256-row instances of generation 4.
template <int NW, int EPI>
__device__ __forceinline__ void epi_mask_res(float (&v)[NW], const u32x4 rw, const u32x4 mw, int mask_pre) {
#pragma unroll
    for (int j = 0; j < NW / 2; ++j) {
        const unsigned mj = (EPI & 2) ? mw[j] : 0x3f803f80u, rj = (EPI & 1) ? rw[j] : 0u;
        const bool keep_lo = __uint_as_float(mj << 16) > 0.f, keep_hi = __uint_as_float(mj & 0xffff0000u) > 0.f;
        float lo = v[2 * j], hi = v[2 * j + 1];
        if (EPI == 2 || (EPI == 3 && mask_pre)) { lo = keep_lo ? lo : 0.f; hi = keep_hi ? hi : 0.f; }      // (no residual: either side is the same)
        if (EPI & 1) { lo += __uint_as_float(rj << 16); hi += __uint_as_float(rj & 0xffff0000u); }
        if (EPI == 3 && !mask_pre) { lo = keep_lo ? lo : 0.f; hi = keep_hi ? hi : 0.f; }
        v[2 * j] = lo; v[2 * j + 1] = hi;
    }
}

template <int NW>
__device__ __forceinline__ void epi_relu(float (&v)[NW]) {
#pragma unroll
    for (int j = 0; j < NW; ++j) v[j] = v[j] > 0.f ? v[j] : 0.f;
}

// bf16 (round to nearest even) -> one guarded store of 2 NW bytes
template <int NW>
__device__ __forceinline__ void epi_store_bf16(const float (&v)[NW], __amdgpu_buffer_rsrc_t rsrc, unsigned off) {
    if constexpr (NW == 8) {
        u32x4 o;
        o.x = pack2(v[0], v[1]); o.y = pack2(v[2], v[3]); o.z = pack2(v[4], v[5]); o.w = pack2(v[6], v[7]);
        epi_store16(o, rsrc, off);
    } else {
        u32x2 o;
        o.x = pack2(v[0], v[1]); o.y = pack2(v[2], v[3]);
        epi_store8(o, rsrc, off);
    }
}

// Row r of the eight f32 accumulator fragments a[0 .. 7] -> two 16-byte stores (the partial sums of a K slice / of a stream-K range)
template <int AUX>
__device__ __forceinline__ void epi_store_f32x8(const __attribute__((ext_vector_type(4))) float* a, int r, __amdgpu_buffer_rsrc_t rsrc,
                                                unsigned off0, unsigned off1) {
    u32x4 o0, o1;
    o0.x = __float_as_uint(a[0][r]); o0.y = __float_as_uint(a[1][r]); o0.z = __float_as_uint(a[2][r]); o0.w = __float_as_uint(a[3][r]);
    o1.x = __float_as_uint(a[4][r]); o1.y = __float_as_uint(a[5][r]); o1.z = __float_as_uint(a[6][r]); o1.w = __float_as_uint(a[7][r]);
    epi_store16<AUX>(o0, rsrc, off0);
    epi_store16<AUX>(o1, rsrc, off1);
}

// fp8 (OCP e4m3) output: clamp(v * scale, +-448), four per dword
__device__ __forceinline__ unsigned pack_fp8x4(float a, float b, float c, float d) {
    unsigned w = 0;
    w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, w, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
    return w;
}
__device__ __forceinline__ u32x2 epi_quant_fp8(const float (&v)[8], float scale) {
    float c[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float q = v[j] * scale;
        c[j] = q > 448.f ? 448.f : (q < -448.f ? -448.f : q);
    }
    u32x2 o;
    o.x = pack_fp8x4(c[0], c[1], c[2], c[3]); o.y = pack_fp8x4(c[4], c[5], c[6], c[7]);
    return o;
}
