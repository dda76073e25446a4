// binary16 <-> binary64 with integer operations on the bits, one text for the host (scs_convert.cpp), the device (the partition kernels of
// csrc/ap_partition_kernels.hip, the F16 scatter of uspmv_api.hip) and the stand-alone check tests/cpp/f16_round_check.cpp.
// gfx950 has no f64 -> f16 instruction and the compiler's path through f32 rounds twice (1 + 2^-11 + 2^-30 is 0x3C01 in one rounding,
// 0x3C00 through float), so nothing here converts through float.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define USPMV_HD __host__ __device__
#else
#define USPMV_HD
#endif

// binary16 from the bits of a double in ONE rounding step (to nearest, ties to even): subnormal results kept, overflow to +-inf, -0.0
// kept, NaN -> quiet NaN with the top mantissa bits (numpy's npy_doublebits_to_halfbits, so that the result equals numpy's
// float64 -> float16 bit for bit).
USPMV_HD inline uint16_t uspmv_f64_bits_to_f16(uint64_t b) {
    const uint16_t sign = (uint16_t)((b >> 48) & 0x8000u);
    const int e = (int)((b >> 52) & 0x7FF);
    const uint64_t m = b & 0xFFFFFFFFFFFFFull;
    if (e == 0x7FF) {
        if (m == 0) return (uint16_t)(sign | 0x7C00u);
        const uint16_t q = (uint16_t)(m >> 42);
        return (uint16_t)(sign | 0x7C00u | (q ? q : 1u));
    }
    const int E = e - 1023;
    if (E >= 16) return (uint16_t)(sign | 0x7C00u);                   // |v| >= 65536: beyond every rounding to 65504
    if (e == 0 || E < -26) return sign;                                // below half the smallest subnormal (2^-25): +-0
    uint64_t q, rem, half;
    if (E >= -14) {                                                    // normal: 10 mantissa bits kept, 42 rounded away
        q = ((uint64_t)(E + 15) << 10) | (m >> 42);
        rem = m & ((1ull << 42) - 1); half = 1ull << 41;
    } else {                                                           // subnormal: units of 2^-24
        const uint64_t M = m | (1ull << 52);
        const int sh = 28 - E;                                         // 43 .. 54
        q = M >> sh;
        rem = M & ((1ull << sh) - 1); half = 1ull << (sh - 1);
    }
    if (rem > half || (rem == half && (q & 1))) ++q;                   // a carry moves into the exponent (0x7BFF + 1 = inf)
    return (uint16_t)(sign | q);
}

// the bits of the double that holds a binary16 value (exact)
USPMV_HD inline uint64_t uspmv_f16_to_f64_bits(uint16_t h) {
    const uint64_t sign = (uint64_t)(h & 0x8000u) << 48;
    const int e = (h >> 10) & 0x1F;
    const uint64_t m = h & 0x3FFu;
    if (e == 0x1F) return sign | (0x7FFull << 52) | (m << 42);
    if (e != 0) return sign | ((uint64_t)(e - 15 + 1023) << 52) | (m << 42);
    if (m == 0) return sign;
    int p = 9;                                                         // subnormal m * 2^-24: top set bit p -> 2^(p - 24) * 1.xxx
    while (!(m >> p)) --p;
    return sign | ((uint64_t)(p - 24 + 1023) << 52) | ((m << (52 - p)) & 0xFFFFFFFFFFFFFull);
}
