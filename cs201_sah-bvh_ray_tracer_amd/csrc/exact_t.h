// hit.c:28's t from float pairs: the binary32 value of
//
//     T = RN32(T64),  T64 = RN64(RN64((double)(-b) - RN64(sqrt((double)disc))) / (double)D),  D = 2.0f * a,
//
// computed in binary32 alone and CERTIFIED equal to T, or reported as not
// certified, in which case the caller runs the binary64 expression itself
// (trace.h sphere_t). Shared by the kernels and the host
// (tests/test_exact_t_host.py reads it through mirt_exact_t_pairs); built
// without contraction like coop.h: every fused operation below is an explicit
// fmaf and nothing else may fuse.
//
// The caller passes the three seeds, so the bound can be checked against any
// hardware within the stated accuracy:
//     s  ~ sqrt(disc)   |s  - S|   <= 8u S,    S = sqrt(disc) (real)
//     rs ~ 1 / s        |rs - 1/s| <= 8u / s
//     rd ~ 1 / D        |rd - 1/D| <= 8u / D,  u = 2^-24.
// v_sqrt_f32 and v_rcp_f32 are accurate to 1 ulp <= 2u relative; 8u leaves room
// for 3 ulp more (the host test moves each seed by -2 .. +2 ulp).
//
// Sequence (each line one binary32 operation, RN; the two-sum is Knuth's):
//     r  = fma(-s, s, disc)            sl = r * (0.5 * rs)
//     nh = (-b) - s                    e  = the two-sum error: nh + e = -b - s exactly
//     nl = e - sl                      q  = nh * rd
//     r2 = fma(-q, D, nh)              ql = (r2 + nl) * rd
//     th = q + ql                      tl = (q - th) + ql
//
// Bound. Write M = |b| + S, N = -b - S and Q = N / D (reals; Q is the t that
// T64 approximates). Certification needs the RANGE
//     2^-30 <= disc, D <= 2^30  and  |b| <= 2^30,
// so S, s are in [2^-15.1, 2^15.1], rd in [2^-30.1, 2^30.1], every value below
// is finite, and one UNIT  U = u^2 M / D  is at least 2^-48 2^-15 2^-30 = 2^-93.
// Every "(1 + e)" is a rounding, |e| <= u, valid for a normal result; results in
// the subnormal range are collected in (6).
//
// (1) The root. rho = disc - s^2 = (S - s)(S + s), so |rho| <= 8u S (2 + 8u) S
//     and r = rho (1 + e). S - s = rho / (S + s), while sl approximates
//     rho / (2 s): the two differ by |rho| |s - S| / (2 s (S + s))
//     <= (8u)^2 S (1 + 8u) / (2 (1 - 8u)) <= 33 u^2 S, and sl = rho / (2 s) times
//     (1 + e)(1 + 8u)(1 + e) (r's rounding, rs, the product; 0.5 rs is exact) is
//     within 10.1u |rho / (2 s)| <= 10.1u 8.1u S <= 82 u^2 S of it. So
//         |S - (s + sl)| <= 115 u^2 S   and   |sl| <= 8.2u S.
// (2) The numerator. nh + e = -b - s exactly (two-sum, no overflow in range),
//     |e| <= u |nh|, |nh| <= (|b| + s)(1 + u) <= 1.01 M. nl = (e - sl)(1 + e'),
//     |e - sl| <= 1.01u M + 8.2u S <= 9.3u M, so nl is within 9.3 u^2 M of e - sl.
//     N = nh + e - (S - s), hence
//         |N - (nh + nl)| <= 115 u^2 S + 9.3 u^2 M <= 125 u^2 M.
// (3) The quotient. q = nh rd (1 + e) = (nh / D)(1 + 8u)(1 + e), so
//     |nh - q D| <= 9.1u |nh| <= 9.2u M; r2 = (nh - q D)(1 + e). With
//     R = (nh - q D) + nl (exact), (nh + nl) / D = q + R / D and |R| <= 18.5u M.
//     ql = (R + (nh - q D) e)(1 + e)(1 + 8u)(1 + e) / D (the sum, rd, the
//     product), so
//         |ql - R / D| <= (10.1u 18.5u M + 1.01u 9.2u M) / D <= 197 U.
// (4) The final pair. If |q| >= |ql| the fast two-sum is exact:
//     th + tl = q + ql. Otherwise (deep cancellation in nh) z = RN(q - th) and
//     tl = RN(ql - z) each round once: |th - q| <= 3.1 |ql|, so the pair
//     misses q + ql by at most 3.2u |ql| <= 3.2u 18.7u M / D <= 61 U.
// (5) The reference's own roundings, v = 2^-53: RN64(sqrt) is off by <= v S,
//     the subtraction by <= v (|N| + v S), the division by <= v |N64 / D|:
//     |T64 - Q| <= 3.01 v M / D -- ABSOLUTE in M / D, because -b - S may cancel
//     -- which is 3.01 2^-5 U < 0.1 U. (No binary64 value here leaves the
//     normal range: the operands are binary32 normals within 2^+-31.)
// (6) Underflow. A binary32 result in the subnormal range, rounded or flushed
//     to zero, is off by less than 2^-126 instead of the relative u assumed
//     above. nh (zero or at least an ulp of min(|b|, s) >= 2^-40), q (>= 2^-71
//     then) and r (a multiple of ulp(s)^2 >= 2^-78) cannot be; e is exact
//     whatever its size. sl, nl, r2 and the sum r2 + nl can: each reaches
//     th + tl times at most |rd| (1 + u) < 2^30.2, in all < 4 2^-95.8 = 2^-93.8.
//     ql, z and tl enter unscaled (3 2^-126), and a subnormal th is never
//     certified (below). Together < 2^-93 <= 1 U.
//
//     |th + tl - T64| <= (125 + 197 + 61 + 0.1 + 1) U < 385 U  <  E = 512 U = 2^-39 M / D.
//
// The computed Ef = RN(RN(RN(|b| + s) |rd|) 2^-39) >= 512 U (1 - 8u)^2 (1 - u)^2
// > 511 U (the last product is an exact scaling: Ef >= 2^-94), so Ef bounds the
// error with a quarter to spare.
//
// Certification. th is returned as T only if
//   * the RANGE above holds (a subnormal, zero, negative, infinite or NaN disc,
//     D or b: not certified);
//   * th's significand field is not zero: th is no power of two, so both its
//     neighbours lie ulp(th) away (the binade edge, where the lower neighbour is
//     half as far, is never certified, whatever the side);
//   * RN(|tl| + Ef) < h, h = 2^(exponent of th) 2^-24 = ulp(th) / 2. RN is
//     monotone and h a binary32 number, so this implies |tl| + Ef < h strictly:
//     every real within Ef of th + tl, T64 among them, lies strictly inside
//     (th - ulp/2, th + ulp/2) and rounds to th. For a zero or subnormal th the
//     exponent field is 0 and h = 0: not certified. For a normal th below
//     2^-102, h <= 2^-126 < Ef: not certified. th is finite in range
//     (|q| <= 2^15.2 2^30.2).
#pragma once
#include <cmath>
#include <cstdint>

#include "rng.h"  // MIRT_HD

namespace mirt {

constexpr float kExactTLo = 0x1p-30f, kExactTHi = 0x1p30f;  // the certified range of disc, D and |b|
constexpr float kExactTBound = 0x1p-39f;                    // E = 2^-39 (|b| + s) |rd|

// b, disc: hit.c:24-25's floats (disc > 0); d2a: 2.0f * a; s, rs, rd: the
// seeds above. Returns whether th is certified to be T; th is meaningless
// otherwise.
MIRT_HD bool exact_t_pair(float b, float disc, float d2a, float s, float rs, float rd, float& th)
{
    // the RANGE, on bit patterns (ordered as the values for non-negative floats; a negative number or a NaN of
    // either sign lies above every finite positive pattern, so fails the upper test)
    const uint32_t ud = __builtin_bit_cast(uint32_t, disc), ua = __builtin_bit_cast(uint32_t, d2a);
    const uint32_t ub = __builtin_bit_cast(uint32_t, b) & 0x7fffffffu;
    const uint32_t lo = ud < ua ? ud : ua, hi0 = ud < ua ? ua : ud, hi = hi0 < ub ? ub : hi0;
    const bool range = lo >= __builtin_bit_cast(uint32_t, kExactTLo) && hi <= __builtin_bit_cast(uint32_t, kExactTHi);
    const float r = fmaf(-s, s, disc);
    const float sl = r * (0.5f * rs);
    const float nb = -b, ns = -s;
    const float nh = nb - s;
    const float bb = nh - nb;
    const float e = (nb - (nh - bb)) + (ns - bb);
    const float nl = e - sl;
    const float q = nh * rd;
    const float r2 = fmaf(-q, d2a, nh);
    const float ql = (r2 + nl) * rd;
    th = q + ql;
    const float tl = (q - th) + ql;
    const float ef = ((fabsf(b) + s) * fabsf(rd)) * kExactTBound;
    const uint32_t hb = __builtin_bit_cast(uint32_t, th);
    const float h = __builtin_bit_cast(float, hb & 0x7f800000u) * 0x1p-24f;
    return range && (hb & 0x007fffffu) != 0u && fabsf(tl) + ef < h;
}

}  // namespace mirt
