// fixed_point.h -- the conversion the fixed-point M-step forms share (k_mstep_tiles, the fixed-point work-item form, k_mincr_delta*):
// plain C++, so that the device code and the host-side check of the live floor (tests/live_floor_check.cpp) run the same arithmetic.
#pragma once

#if defined(__HIPCC__)
#define DMX_FIXED_HD __host__ __device__
#else
#define DMX_FIXED_HD
#endif

namespace dmx {

constexpr int FIXED_SHIFT_MAX = 50;  // the largest exponent of a tile's grid (repack_device.hip: cut_mstep_tiles)

// c in [0, 1] -> rint(c 2^shift) as an integer: adding 1.5 x 2^52 leaves the rounded value (ties to even) in the low bits of the
// sum's mantissa (c 2^shift < 2^51)
DMX_FIXED_HD inline unsigned long long fixed_of(float c, int shift)
{
    constexpr double MAGIC = 6755399441055744.0;
    const double d = __builtin_ldexp((double)c, shift) + MAGIC;
    return (unsigned long long)(__builtin_bit_cast(long long, d) - __builtin_bit_cast(long long, MAGIC));
}

}  // namespace dmx
