"""The index math the kernels share with the host (csrc/coop.h), on the CPU
through mirt_coop_geometry and mirt_pixel_rows: the group geometry of the
wave-cooperative bounce sampling, and the multiply-high divisions of the
pixel -> (row, x) -> image row mapping. Every expected value is plain Python /
numpy integer arithmetic."""
import ctypes as C

import numpy as np
import pytest


def _geometry(mirt, L, n_pending, accepted):
    group = C.c_int32()
    rank = np.zeros(64, np.int32)
    tri = np.zeros(64, np.int32)
    first = np.full(64, -7, np.int32)
    p = mirt.abi.ptr
    rc = L.mirt_coop_geometry(n_pending, accepted, C.byref(group), p(rank), p(tri), p(first))
    assert rc == 0, L.mirt_last_error()
    return group.value, rank, tri, first


def test_group_geometry_exhaustive(mirt):
    L = mirt.load()
    rng = np.random.default_rng(5)
    sizes = set()
    for n_pending in range(1, 65):
        ceil_log2 = (n_pending - 1).bit_length()
        g_want = 64 >> ceil_log2
        ballots = [0, (1 << 64) - 1, 1, 1 << 63] + [int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2))
                                                     for _ in range(20)]
        ballots += [int(rng.integers(0, 1 << 63)) & int(rng.integers(0, 1 << 63)) & int(rng.integers(0, 1 << 63))
                    for _ in range(20)]   # sparse: groups that accept nothing
        for accepted in ballots:
            g, rank, tri, first = _geometry(mirt, L, n_pending, accepted)
            assert g == g_want
            assert g * n_pending <= 64 and (g == 1 or 2 * g * n_pending > 64)   # the largest power of two that fits
            assert (rank == np.arange(64) // g).all() and (tri == np.arange(64) % g).all()
            for r in range(n_pending):
                want = next((j for j in range(g) if accepted >> (r * g + j) & 1), -1)   # the plain scan
                assert first[r] == want, (n_pending, hex(accepted), r)
            assert (first[n_pending:] == -7).all()   # nothing written past the owners
        sizes.add(g)
    assert sizes == {1, 2, 4, 8, 16, 32, 64}
    assert L.mirt_coop_geometry(0, 0, None, None, None, None) == -1
    assert L.mirt_coop_geometry(65, 0, None, None, None, None) == -1


@pytest.fixture(scope="module")
def pixels():
    rng = np.random.default_rng(11)
    return np.concatenate([np.arange(1 << 22, dtype=np.uint32),
                           rng.integers(0, 1 << 31, 10**6).astype(np.uint32),
                           np.array([(1 << 31) - 1, (1 << 31) - 2], np.uint32)])


def _check_rows(mirt, L, px, W, row_block, shards, shard, samples, shard_rows):
    p = px.astype(np.int64)
    r, x = p // W, p % W
    out = np.zeros((len(p), 4), np.int32)
    rc = L.mirt_pixel_rows(W, shard_rows, samples, row_block, shard, shards, mirt.abi.ptr(px), len(p),
                           mirt.abi.ptr(out))
    assert rc == 0, L.mirt_last_error()
    assert (out[:, 0] == r).all() and (out[:, 1] == x).all()
    assert (out[:, 3] == r // shard_rows).all()
    rr = r % shard_rows if samples > 1 else r
    blk = rr // row_block
    y = (blk * shards + shard) * row_block + rr % row_block
    fits = y < (1 << 31)   # a launch row whose image row an int holds
    assert 2 * fits.sum() > len(p)
    assert (out[fits, 2] == y[fits]).all(), (W, row_block, shards, shard, samples, shard_rows)


WIDTHS = [1, 2, 3, 7, 160, 640, 1919, 1920, 3840, 65535]


@pytest.mark.parametrize("W", WIDTHS)
def test_magic_division(mirt, pixels, W):
    """pixel / W, pixel % W, the launch row's frame and its image row, for
    every pixel below 2^22 and 10^6 random ones below 2^31: row blocks 1 / 8 /
    64 with shards 1 / 3 / 8, one frame per launch and several."""
    L = mirt.load()
    for row_block, shards, shard, samples, shard_rows in [(1, 1, 0, 1, 1080), (8, 3, 1, 4, 360), (64, 8, 7, 3, 270)]:
        _check_rows(mirt, L, pixels, W, row_block, shards, shard, samples, shard_rows)


def test_magic_division_every_shard(mirt, pixels):
    """Row blocks 1 / 8 / 64 x shards 1 / 3 / 8, every shard of each, divisors
    of shard_rows from 1 to 65535, on a thinned set of the same pixels."""
    L = mirt.load()
    px = np.ascontiguousarray(pixels[::61])
    for W in WIDTHS:
        for row_block in (1, 8, 64):
            for shards in (1, 3, 8):
                for shard in range(shards):
                    samples, shard_rows = [(1, 1080), (4, 1), (2, 719), (5, 65535)][(shard + row_block + W) % 4]
                    _check_rows(mirt, L, px, W, row_block, shards, shard, samples, shard_rows)


def test_pixel_rows_rejects_bad_arguments(mirt):
    L = mirt.load()
    one = np.zeros(1, np.uint32)
    out = np.zeros(4, np.int32)
    p = mirt.abi.ptr
    assert L.mirt_pixel_rows(0, 8, 1, 8, 0, 1, p(one), 1, p(out)) == -1
    assert L.mirt_pixel_rows(8, 8, 1, 0, 0, 1, p(one), 1, p(out)) == -1
    assert L.mirt_pixel_rows(8, 8, 1, 8, 1, 1, p(one), 1, p(out)) == -1
    assert L.mirt_pixel_rows(8, 8, 1, 8, 0, 1, None, 1, p(out)) == -1
    assert L.mirt_last_error().decode() == "mirt_pixel_rows: invalid arguments"
