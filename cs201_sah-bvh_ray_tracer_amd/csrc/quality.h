// The SAH quality of a flat tree (mirt_tree_quality): the pieces
// bvh_quality.cpp (host) and quality_device.hip (kernel) share, so that both
// paths form every term and every sum from the same operations.
//
//   area      box_area of tree.h (bvh.c:48-57), fp32, uncontracted;
//   e         ilogb(A0) + 1 of the root's area A0: every area in [0, A0] is
//             below 2^e;
//   term      trunc((double)area * 2^(48 - e)) as a uint64, below 2^48 (the
//             product is exact: a power of two, no underflow for any float). An
//             area that is not >= 0 gives 0, one above A0 gives 2^48; both are
//             counted as clamped;
//   sums      the terms' high (t >> 24) and low (t & 0xffffff) halves are added
//             apart in two uint64: integers, so the order of addition does not
//             show, and neither half can overflow below 2^31 nodes;
//   value     ldexp((double)hi * 2^24 + (double)lo, e - 48): quality_sum_value.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/mirt.h"
#include "tree.h"

namespace mirt {

struct QualitySums {
    uint64_t inner_hi, inner_lo, leaf_hi, leaf_lo;
    int32_t inner_nodes, leaves, dead_leaves, clamped;
    uint32_t root_area_bits, pad;
};

// a positive finite float (else the tree is degenerate)
MIRT_HD inline bool quality_root_ok(float a0)
{
    return a0 > 0.0f && (float_bits(a0) & 0x7f800000u) != 0x7f800000u;
}

// ilogb(a0) + 1 of a positive finite float: in [-148, 128]
MIRT_HD inline int quality_exponent(float a0)
{
    const uint32_t b = float_bits(a0);
    const int ex = (int)((b >> 23) & 0xffu);
    if (ex) return ex - 126;
    uint32_t m = b & 0x7fffffu;  // subnormal: m * 2^-149, m > 0
    int top = -1;
    while (m) {
        m >>= 1;
        top++;
    }
    return top - 148;
}

// 2^(48 - e), a normal double for every e of quality_exponent
MIRT_HD inline double quality_scale(int e)
{
    const uint64_t b = (uint64_t)(1023 + 48 - e) << 52;
    double d;
    memcpy(&d, &b, 8);
    return d;
}

MIRT_HD inline uint64_t quality_term(float area, float a0, double scale, int32_t* clamped)
{
    if (!(area >= 0.0f)) {
        (*clamped)++;
        return 0;
    }
    if (area > a0) {
        (*clamped)++;
        return (uint64_t)1 << 48;
    }
    return (uint64_t)((double)area * scale);
}

inline double quality_sum_value(uint64_t hi, uint64_t lo, int e)
{
    return std::ldexp((double)hi * 16777216.0 + (double)lo, e - 48);
}

// bvh_quality.cpp: the public struct from the integer sums; both paths end here
void quality_finish(const QualitySums& q, mirt_tree_quality* out);

// cost_now / cost_base; 1 whenever either is not a positive finite number
inline double quality_decay(double cost, double base)
{
    const bool ok = cost > 0.0 && std::isfinite(cost) && base > 0.0 && std::isfinite(base);
    return ok ? cost / base : 1.0;
}

}  // namespace mirt
