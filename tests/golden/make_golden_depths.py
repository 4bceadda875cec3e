"""Generate tests/golden/depths.json from the REFERENCE ITSELF: SHA-256 of the
unmodified reference's frames at every depth mirt_frame_desc admits (0..8).

Runs only where oracle/_ref/libref_160x90.so can be built (oracle/Makefile: the
unmodified reference hot-path sources + oracle/ref_harness.c). Nothing here
uses the oracle restatement or the product: the scenes are the reference's own
create_random_sphere loop, the tree its build_bvh_node, the frames its
trace_ray under the per-pixel RNG contract (mode 1). The tests then check the
oracle (test_frame_edges_host.py) and the kernels (test_frame_edges_gpu.py)
against these hashes.

    python tests/golden/make_golden_depths.py          # ~10 s

Output (data only): depths.json, {"frames": {key: sha256}} with the keys of
frame_edge_cases.GOLDEN -- S1 (1000 spheres, seed 2, default camera) at depths
0..8 with seeds 3 and 0xDEADBEEF12345678, S2 (3000 spheres, seed 11, camera at
the origin) at depths 6 and 8, S1 brute force at depths 4 and 8; all 160x90.
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle.lib import Reference, abi, build  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
W, H = 160, 90
SEED_HI = 0xDEADBEEF12345678
SCENES = {"S1": (1000, 2, (0.0, 4.0, 50.0)), "S2": (3000, 11, (0.0, 0.0, 0.0))}   # spheres, seed, camera position


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    build(ref=True)
    R = Reference(W, H)
    frames = {}
    for name, (n, seed, pos) in SCENES.items():
        cam = abi.default_camera()
        cam.position = abi.Vec3(*pos)
        s = R.render_scene(seed, n)
        t = R.build(s)   # points into s: s stays alive and is the sphere base

        def frame(key, **kw):
            frames[key] = sha(R.render(cam, s, t, mode=1, threads=8, **kw))
            print(key, frames[key], flush=True)

        if name == "S1":
            for d in range(9):
                frame(f"S1_d{d}_s3", depth=d, seed=3)
                frame(f"S1_d{d}_s{SEED_HI:x}", depth=d, seed=SEED_HI)
            for d in (4, 8):
                frame(f"S1_brute_d{d}_s3", depth=d, seed=3, use_bvh=False)
        else:
            for d in (6, 8):
                frame(f"S2_d{d}_s3", depth=d, seed=3)
        R.free(t)
    G = {"generated_by": "tests/golden/make_golden_depths.py from oracle/_ref (unmodified reference sources)",
         "size": [W, H], "frames": dict(sorted(frames.items()))}
    with open(os.path.join(OUT, "depths.json"), "w") as f:
        json.dump(G, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
