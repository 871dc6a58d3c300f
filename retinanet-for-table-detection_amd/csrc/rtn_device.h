// rtn_device.h — device-only helpers shared by several kernel files (each kernel file includes it after rtn_internal.h).
#pragma once
#include <hip/hip_runtime.h>

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;

// Buffer descriptor words in SGPRs (raw buffer, stride 0, range = `bytes`); every input is made wave-uniform.
__device__ __forceinline__ i32x4 make_srd(const void* ptr, unsigned bytes) {
    const unsigned long long a = (unsigned long long)ptr;
    i32x4 r;
    r.x = __builtin_amdgcn_readfirstlane((int)(unsigned)a);
    r.y = __builtin_amdgcn_readfirstlane((int)((unsigned)(a >> 32) & 0xffffu));
    r.z = __builtin_amdgcn_readfirstlane((int)bytes);
    r.w = 0x00020000;
    return r;
}

// 16 bytes per lane through a raw buffer resource (lanes whose `voff` is outside its range read zeros)
__device__ __forceinline__ uint4 buffer_load16(__amdgpu_buffer_rsrc_t rsrc, unsigned voff) {
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)voff, 0, 0);
    return make_uint4(v.x, v.y, v.z, v.w);
}

// LDS-DMA: 64 lanes x 16 B from (descriptor, per-lane byte offset `voff`) to LDS bytes [lds_addr, lds_addr + 1024), lane-linear;
// `lds_addr` is wave-uniform, lanes whose `voff` is outside the descriptor range write zeros.  Issued from asm so that hipcc's
// waitcnt insertion neither counts nor drains it (it would wait for vmcnt(0) before the next ds_read and lose the overlap with the
// MFMAs): the kernel's own counted waits cover it.  M0 is saved / restored inside the statement.  The literal 0 offset is a form of
// its own: a zero passed to the `soff` overload below occupies an SGPR and moves the callers' register allocation.
__device__ __forceinline__ void dma16(const i32x4& srd, unsigned voff, unsigned lds_addr) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %3, 0 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(lds_addr), "s"(srd)
                 : "memory");
}
// ... with `lds_addr` forced into an SGPR (readfirstlane), for callers whose address the compiler cannot prove uniform
__device__ __forceinline__ void dma16_uniform(const i32x4& srd, unsigned voff, unsigned lds_addr) {
    dma16(srd, voff, (unsigned)__builtin_amdgcn_readfirstlane((int)lds_addr));
}
// ... with a wave-uniform byte offset `soff` added to every lane's `voff`
__device__ __forceinline__ void dma16(const i32x4& srd, unsigned voff, unsigned soff, unsigned lds_addr) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %3, %4 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(lds_addr), "s"(srd), "s"(soff)
                 : "memory");
}
// The same with `soff` and `lds_addr` forced into SGPRs (readfirstlane): for callers whose uniform operands the compiler cannot prove
// uniform (rtn_conv_halon.hip derives them from a ring cursor inside its K loop).
__device__ __forceinline__ void dma16_uniform(const i32x4& srd, unsigned voff, unsigned soff, unsigned lds_addr) {
    const unsigned la = (unsigned)__builtin_amdgcn_readfirstlane((int)lds_addr), so = (unsigned)__builtin_amdgcn_readfirstlane((int)soff);
    dma16(srd, voff, so, la);
}

// A 16-byte buffer store whose data registers the following VALU instructions rewrite needs two wait states on gfx940+; LLVM pads
// them except when the store's soffset is an SGPR (its hazard table treats that form as immune), which left ZERO wait states in the
// fused bottleneck kernel and corrupted dword 0 of such stores (profiles/r3_store_hazard_isa.txt).  Naming the data registers as
// inputs of an asm statement keeps them intact for four wait states whatever the compiler schedules next or wherever it keeps the
// offset; tools/scan_store_hazard.py checks the built library.  The guard goes directly behind EVERY raw buffer store of a kernel
// that computes on after it: 16-byte, 8-byte (RTN_STORE_GUARD2) and 4-byte (RTN_STORE_GUARD1, two wait states) data.  The guarded
// stores of rtn_conv_epilogue.h are the way to issue one; a kernel that writes its own store writes the guard next to it.
#define RTN_STORE_GUARD(V) asm volatile("s_nop 3" :: "v"(V.x), "v"(V.y), "v"(V.z), "v"(V.w));
#define RTN_STORE_GUARD2(V) asm volatile("s_nop 3" :: "v"(V.x), "v"(V.y));
#define RTN_STORE_GUARD1(V) asm volatile("s_nop 1" :: "v"(V));

// f / d for 0 <= f < 2^24 with inv = 1.0f / d: the float product is within one of the quotient
__device__ __forceinline__ void divmod24(int f, int d, float inv, int& q, int& r) {
    q = (int)((float)f * inv);
    r = f - q * d;
    if (r < 0) { --q; r += d; }
    if (r >= d) { ++q; r -= d; }
}

// two floats -> two bf16 (round to nearest even) in one register
__device__ __forceinline__ unsigned pack2(float a, float b) {
    bf16x2 v = {(__bf16)a, (__bf16)b};
    return __builtin_bit_cast(unsigned, v);
}
