// rtn_device.h — device-only helpers shared by several kernel files (each kernel file includes it after rtn_internal.h).
#pragma once
#include <hip/hip_runtime.h>

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) int i32x4;

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

// 64 lanes x 16 B from (descriptor, per-lane byte offset `voff` + uniform `soff`) to LDS bytes [lds_addr, lds_addr + 1024).
// asm so that hipcc neither counts nor drains it; the kernel's own counted waits cover it.
__device__ __forceinline__ void dma16(const i32x4& srd, unsigned voff, unsigned soff, unsigned lds_addr) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %3, %4 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(lds_addr), "s"(srd), "s"(soff)
                 : "memory");
}

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
