// Host entry points over the index math of coop.h, which the kernels share
// (mirt_coop_geometry, mirt_pixel_rows): what tests/test_coop_host.py checks
// on the CPU is the code the device compiles.
#include "coop.h"
#include "internal.h"

using namespace mirt;

extern "C" int mirt_coop_geometry(int num_pending, uint64_t accepted, int32_t* group, int32_t* lane_rank,
                                  int32_t* lane_try, int32_t* first_accept)
{
    if (num_pending < 1 || num_pending > 64 || !group || !lane_rank || !lane_try || !first_accept) {
        set_error("mirt_coop_geometry: invalid arguments");
        return MIRT_E_INVALID;
    }
    const uint32_t shift = coop_group_shift((uint32_t)num_pending);
    *group = (int32_t)(1u << shift);
    for (uint32_t i = 0; i < 64; i++) {
        lane_rank[i] = (int32_t)coop_lane_rank(i, shift);
        lane_try[i] = (int32_t)coop_lane_try(i, shift);
    }
    for (uint32_t r = 0; r < (uint32_t)num_pending; r++) first_accept[r] = coop_first_accept(accepted, r, shift);
    return MIRT_OK;
}

extern "C" int mirt_pixel_rows(int width, int shard_rows, int samples, int row_block, int shard, int num_shards,
                               const uint32_t* pixels, int64_t n, int32_t* out)
{
    if (width < 1 || shard_rows < 1 || samples < 1 || row_block < 1 || num_shards < 1 || shard < 0 ||
        shard >= num_shards || n < 0 || (n > 0 && (!pixels || !out))) {
        set_error("mirt_pixel_rows: invalid arguments");
        return MIRT_E_INVALID;
    }
    const RowMagic m = row_magic_make(width, shard_rows, row_block);
    for (int64_t i = 0; i < n; i++) {
        const uint32_t p = pixels[i];
        const uint32_t r = magic_div(p, (uint32_t)width, m.width);
        out[4 * i] = (int32_t)r;
        out[4 * i + 1] = (int32_t)(p - r * (uint32_t)width);
        out[4 * i + 2] = magic_row_to_y(m, (int)r, samples, shard_rows, row_block, shard, num_shards, 0);
        out[4 * i + 3] = (int32_t)magic_div(r, (uint32_t)shard_rows, m.shard_rows);
    }
    return MIRT_OK;
}
