// rtn_png_crc.h — CRC-32 arithmetic shared by the PNG encoder and decoder (zlib's representation: bit 31 is x^0).  A buffer's CRC
// state is computed in slices, one per thread; slice states are joined by multiplying with x^(8 n) mod P, n the bytes that follow.
#pragma once
#include <stdint.h>

constexpr uint32_t PE_POLY = 0xedb88320u;      // CRC-32, reflected
constexpr uint32_t PE_ADLER = 65521u;          // modulus of the Adler-32 sums (zlib's BASE)

__host__ __device__ inline uint32_t pe_crc_byte(uint32_t c, uint32_t b) {     // table-free update by one byte
    c ^= b;
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ PE_POLY : c >> 1;
    return c;
}
__host__ __device__ inline uint32_t pe_mulmod(uint32_t a, uint32_t b) {       // a(x) b(x) mod P
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ PE_POLY : b >> 1;
    }
    return p;
}
__host__ __device__ inline uint32_t pe_xpow8(uint32_t n) {                    // x^(8 n) mod P
    uint32_t p = 0x80000000u, sq = 0x00800000u;
    while (n) {
        if (n & 1u) p = pe_mulmod(sq, p);
        sq = pe_mulmod(sq, sq);
        n >>= 1;
    }
    return p;
}
