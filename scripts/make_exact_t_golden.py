"""Makes tests/golden/exact_t_midpoints.npz: of a seeded scan of 10^8
scene-like (ray, sphere) pairs (tests/exact_t_cases.py, set (a)'s
distribution), the 10,000 hits with t > kEps whose binary64 t (hit.c:28 before
the cast) lies nearest a float32 rounding midpoint -- the pairs on which a
float-pair t is hardest to certify and a wrong certification most likely.

    python scripts/make_exact_t_golden.py        (about two minutes, CPU only)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import exact_t_cases as X  # noqa: E402

SEED, CHUNK, CHUNKS, KEEP = 20260901, 4_000_000, 25, 10_000


def main():
    rng = np.random.default_rng(SEED)
    best = None
    for k in range(CHUNKS):
        o, d, c, r = X.scene_like(rng, CHUNK)
        b, disc, d2a = X.quadratic(o, d, c, r)
        with np.errstate(all="ignore"):
            ok = (disc > 0) & (X.reference_t(b, disc, d2a) > X.KEPS)
        dist = np.where(ok, X.midpoint_distance(b, disc, d2a), np.inf)
        idx = np.argpartition(dist, KEEP)[:KEEP]
        part = (dist[idx], o[idx], d[idx], c[idx], r[idx])
        best = part if best is None else tuple(np.concatenate([p, q]) for p, q in zip(best, part))
        keep = np.argsort(best[0], kind="stable")[:KEEP]
        best = tuple(p[keep] for p in best)
        print(f"chunk {k + 1}/{CHUNKS}: farthest kept {best[0][-1]:.3e} ulp", flush=True)
    np.savez_compressed(X.GOLDEN_MIDPOINTS, origin=best[1], direction=best[2], center=best[3], radius=best[4],
                        midpoint_distance_ulp=best[0].astype(np.float64))
    print(X.GOLDEN_MIDPOINTS, os.path.getsize(X.GOLDEN_MIDPOINTS), "bytes")


if __name__ == "__main__":
    main()
