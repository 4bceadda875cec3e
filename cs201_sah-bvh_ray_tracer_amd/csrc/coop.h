// Pure index math shared by the kernels and the host (tests/test_coop_host.py
// reads it through mirt_coop_geometry / mirt_pixel_rows):
//
//  * the group geometry of hemisphere_wave (trace.h): how a wave's 64 lanes
//    are dealt to the lanes whose rejection sampling is still pending;
//  * division by a per-frame constant as multiply-high, shift and one
//    correction step (chain_key and the row mapping of render.hip).
#pragma once
#include <cstdint>

#include "rng.h"    // MIRT_HD
#include "shard.h"

namespace mirt {

// ---- hemisphere_wave's groups ------------------------------------------
// np lanes are pending (1 <= np <= 64). Each of them ("owner", rank = its
// position among the pending lanes in lane order) gets an aligned group of
// g = 64 >> ceil_log2(np) lanes: 64 for one owner, 1 above 32 owners. Lane i
// serves the owner of rank i / g (none if that is >= np) and computes that
// owner's next try number i % g. Returned: log2(g).
MIRT_HD uint32_t coop_group_shift(uint32_t np)
{
    const uint32_t ceil_log2 = np <= 1u ? 0u : 32u - (uint32_t)__builtin_clz(np - 1u);
    return 6u - ceil_log2;
}
MIRT_HD uint32_t coop_lane_rank(uint32_t lane, uint32_t shift) { return lane >> shift; }
MIRT_HD uint32_t coop_lane_try(uint32_t lane, uint32_t shift) { return lane & ((1u << shift) - 1u); }

// The lowest try offset the group of owner `rank` accepted, from the wave's
// ballot of accepting lanes; -1 if the group accepted none.
MIRT_HD int coop_first_accept(uint64_t accepted, uint32_t rank, uint32_t shift)
{
    uint64_t bits = accepted >> ((rank << shift) & 63u);
    if (shift < 6u) bits &= (1ull << (1u << shift)) - 1ull;
    return bits ? __builtin_ctzll(bits) : -1;
}

// ---- division by a per-frame constant ----------------------------------
// n / d for any 32-bit n and d >= 1: with s = floor(log2 d) and
// m = min(floor(2^(32+s) / d), 2^32 - 1), m = 2^(32+s) / d - e with
// 0 <= e <= 1, so n m / 2^(32+s) = n / d - n e / 2^(32+s) lies less than 1
// below n / d and its floor (mul_hi, then the shift) is the quotient or one
// less: one correction step makes it exact.
struct MagicDiv {
    uint32_t mul, shift;
};
inline MagicDiv magic_div_make(uint32_t d)
{
    if (d == 0) return MagicDiv{0u, 0u};
    const uint32_t s = 31u - (uint32_t)__builtin_clz(d);
    const uint64_t m = (1ull << (32u + s)) / d;
    return MagicDiv{m > 0xffffffffull ? 0xffffffffu : (uint32_t)m, s};
}
MIRT_HD uint32_t magic_div(uint32_t n, uint32_t d, MagicDiv m)
{
    uint32_t q = (uint32_t)(((uint64_t)n * m.mul) >> 32) >> m.shift;
    if (n - q * d >= d) q++;
    return q;
}

// The divisors of a frame's pixel -> (row, x) -> image row mapping.
struct RowMagic {
    MagicDiv width, shard_rows, row_block;
};
inline RowMagic row_magic_make(int width, int shard_rows, int row_block)
{
    return RowMagic{magic_div_make((uint32_t)width), magic_div_make((uint32_t)shard_rows),
                    magic_div_make((uint32_t)row_block)};
}

// Image row of launch row r >= 0: compacted shard row r % shard_rows (of
// frame r / shard_rows when the launch holds several), its row block mapped
// to the image by shard_block.
MIRT_HD int magic_row_to_y(const RowMagic& m, int r, int samples, int shard_rows, int row_block, int shard,
                           int num_shards, int lead_skip)
{
    if (samples > 1) r -= (int)magic_div((uint32_t)r, (uint32_t)shard_rows, m.shard_rows) * shard_rows;
    const int blk = (int)magic_div((uint32_t)r, (uint32_t)row_block, m.row_block);
    return shard_block(shard, blk, num_shards, lead_skip) * row_block + (r - blk * row_block);
}

}  // namespace mirt
