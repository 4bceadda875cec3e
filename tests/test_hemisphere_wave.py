"""hemisphere_wave (csrc/trace.h), the wave-cooperative form of the bounce
direction sampling, against a numpy restatement of the RNG contract (csrc/rng.h)
and of the per-lane rejection loop it replaces.

mirt_hemisphere_probe runs the device function on caller-given lanes: each
wave gets a `need` mask of a chosen size at scattered lanes (every group size
of the scheme: 64, 32, 16, 8, 4, 2, 1) and, among ordinary pixels, keys whose
first accepted try comes late, in the first, a middle and the last sampling
lane, so that several rounds with shrinking and growing groups run. Directions
are compared as bit patterns, the draw counters exactly; lanes that only help
must keep what they had.
"""
import numpy as np
import pytest

U64 = np.uint64
F32 = np.float32
W, H = 1920, 1080
POPCOUNTS = [0, 1, 2, 3, 5, 8, 16, 17, 32, 33, 63, 64]


# ------------------------------------------------- csrc/rng.h, restated

def mix64(z):
    z = z ^ (z >> U64(30))
    z = z * U64(0xBF58476D1CE4E5B9)
    z = z ^ (z >> U64(27))
    z = z * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def pixel_key(seed, pixel, sample):
    with np.errstate(over="ignore"):
        inner = mix64((np.asarray(sample, U64) << U64(32)) | np.asarray(pixel, U64))
        return mix64(np.asarray(seed, U64) ^ inner)


def draw(key, k):
    with np.errstate(over="ignore"):
        return (mix64(key + (np.asarray(k, U64) + U64(1)) * U64(0x9E3779B97F4A7C15)) >> U64(33)).astype(np.int64)


def _coord(key, k):
    return F32(-1.0) + (draw(key, k).astype(F32) / F32(2147483648.0)) * F32(2.0)


def one_try(key, k):
    """Draws k, k + 1, k + 2 -> the point and whether the loop accepts it."""
    x, y, z = _coord(key, k), _coord(key, k + 1), _coord(key, k + 2)
    l2 = x * x
    l2 = l2 + y * y
    l2 = l2 + z * z
    return x, y, z, (l2 < F32(1.0)) & (l2 != F32(0.0))


def first_accept(key, k0, limit=64):
    """Index of the first accepted try of each stream (the per-lane loop)."""
    key = np.asarray(key, U64)
    k0 = np.broadcast_to(np.asarray(k0, np.int64), key.shape)
    j = np.full(key.shape, -1, np.int64)
    todo = np.arange(key.size)
    for t in range(limit):
        if not todo.size:
            break
        ok = one_try(key[todo], k0[todo] + 3 * t)[3]
        j[todo[ok]] = t
        todo = todo[~ok]
    assert not todo.size
    return j


def hemisphere_model(key, k0, normal):
    """sphere.c:19-32 on the per-pixel stream, as csrc/trace.h hemisphere()."""
    key = np.asarray(key, U64)
    k0 = np.asarray(k0, np.int64)
    j = first_accept(key, k0)
    x, y, z, ok = one_try(key, k0 + 3 * j)
    assert ok.all()
    sq = x * x
    sq = sq + y * y
    sq = sq + z * z
    ln = np.sqrt(sq.astype(np.float64)).astype(F32)
    x, y, z = x / ln, y / ln, z / ln
    d = x * normal[:, 0]
    d = d + y * normal[:, 1]
    d = d + z * normal[:, 2]
    flip = ~(d > F32(0.0))
    out = np.stack([x, y, z], axis=1)
    out[flip] = out[flip] * F32(-1.0)
    return out, (k0 + 3 * (j + 1)).astype(np.uint32)


# ------------------------------------------------------------ CPU checks

def test_model_matches_contract(golden):
    for seed, px, smp, k, v in golden["contract"]:
        assert int(draw(pixel_key(seed, px, smp), k)) == v


@pytest.fixture(scope="module")
def late():
    """Per k0: 1080p pixels (seed 1, sample 0) whose first accepted try is
    latest, and that try's index."""
    keys = pixel_key(1, np.arange(W * H), 0)
    found = {}
    for k0 in (0, 7, 300):
        j = first_accept(keys, k0)
        order = np.argsort(-j, kind="stable")[:6]
        found[k0] = (order, j[order], j)
    return found


def test_late_pixels(late):
    """The inputs do make the loop run long: at k0 = 0 these pixels of the
    1080p frame first accept at try index 16 or later."""
    _, _, j = late[0]
    assert abs(j.mean() + 1 - 6 / np.pi) < 0.01           # 1.91 tries per pixel
    assert (j[[70333, 419465, 496364, 723920]] >= 16).all()
    assert j[1052312] == 20 and j.max() == 20
    assert (j >= 12).sum() == 273
    for k0 in (7, 300):
        assert late[k0][1].min() >= 14


# ------------------------------------------------------------------ GPU

def _wave(rng, late_px, popcount):
    """One wave's lanes: (pixels, need) with `popcount` sampling lanes at
    scattered positions, the late pixels in the first, middle and last of them."""
    need = np.zeros(64, np.int32)
    lanes = np.sort(rng.choice(64, popcount, replace=False))
    need[lanes] = 1
    px = rng.integers(0, W * H, 64)
    if popcount:
        spots = [lanes[0], lanes[popcount // 2], lanes[-1]]
        px[spots] = rng.permutation(late_px)[:3]
    return px, need


def _run(gpu, rng, late_px, k0, popcounts):
    px, need = map(np.concatenate, zip(*[_wave(rng, late_px, pc) for pc in popcounts]))
    n = len(px)
    keys = pixel_key(1, px, 0)
    normal = rng.normal(size=(n, 3))
    normal = (normal / np.linalg.norm(normal, axis=1)[:, None]).astype(F32)
    before = rng.normal(size=(n, 3)).astype(F32)           # what the helper lanes must keep
    kk = np.full(n, k0, np.uint32)
    got_d, got_k = gpu.hemisphere_probe(keys, kk, normal, need, before)
    want_d, want_k = hemisphere_model(keys, kk, normal)
    s = need != 0
    assert (got_k[s] == want_k[s]).all()
    assert (got_d[s].view(np.uint32) == want_d[s].view(np.uint32)).all()
    assert (got_k[~s] == k0).all()
    assert got_d[~s].tobytes() == before[~s].tobytes()
    return (want_k[s].astype(np.int64) - k0) // 3          # tries of the sampling lanes


@pytest.mark.gpu
@pytest.mark.parametrize("k0", [0, 7, 300])
def test_one_wave(gpu, late, k0):
    """64 threads: one wave per launch, every popcount."""
    rng = np.random.default_rng(100 + k0)
    longest = 0
    for pc in POPCOUNTS:
        tries = _run(gpu, rng, late[k0][0], k0, [pc])
        assert len(tries) == pc
        longest = max(longest, tries.max(initial=0))
    assert longest >= 14   # long runs took part


@pytest.mark.gpu
@pytest.mark.parametrize("k0", [0, 7, 300])
def test_two_workgroups(gpu, late, k0):
    """256 threads x 2 workgroups: eight waves with different masks side by side."""
    rng = np.random.default_rng(200 + k0)
    for pcs in (POPCOUNTS[:8], POPCOUNTS[4:], [64, 0, 33, 1, 32, 64, 2, 17]):
        tries = _run(gpu, rng, late[k0][0], k0, pcs)
        assert len(tries) == sum(pcs) and tries.max() >= 14


@pytest.mark.gpu
def test_probe_rejects_other_shapes(gpu, mirt):
    z = np.zeros(128)
    with pytest.raises(mirt.MirtError, match="mirt_hemisphere_probe: invalid arguments"):
        gpu.hemisphere_probe(z, z, np.zeros((128, 3)), z, np.zeros((128, 3)))
