"""Generate tests/golden/hostile_spheres.json from the REFERENCE ITSELF: what the
unmodified reference does with the hostile scenes of
tests/hostile_sphere_cases.py (negative, zero, subnormal, NaN, infinite and
overflowing radii, non-finite and far centres, duplicates, giants, dust).

Runs only where oracle/_ref/libref_160x90.so can be built (oracle/Makefile: the
unmodified reference hot-path sources + oracle/ref_harness.c). Nothing
recorded here comes from the oracle restatement or the product: the input
spheres are the cases' (their base scene is checked against the reference's
own create_random_sphere loop); the tree is its build_bvh_node, the hit
records its ray_bvh_intersect over its own camera rays, the frames its
trace_ray under the per-pixel RNG contract (mode 1). tests/
test_hostile_spheres_host.py holds the oracle to these hashes, and through the
oracle the host builder and the kernels.

    python tests/golden/make_golden_hostile_spheres.py          # ~20 s

Output (data only): hostile_spheres.json, {"scenes": {name: {"spheres",
"tree", "hits", "frame_tree", "frame_brute": sha256, "nodes": count}}}: the
reordered spheres, the flat tree, the 160 x 90 hit records of the default camera
and the depth-5 frames with the tree and by brute force.
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle.lib import Reference, abi, build  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
W, H = 160, 90


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    build(ref=True)
    import hostile_sphere_cases as sc
    R = Reference(W, H)
    assert R.render_scene(1, sc.N).tobytes() == sc.base().tobytes()
    cam = abi.default_camera()
    cam.position = abi.Vec3(0.0, 4.0, 50.0)
    rays = R.camera_rays(cam).reshape(-1)
    scenes = {}
    for name in sc.SCENES:
        s = sc.inputs(name)[0].copy()
        t = R.build(s)   # points into s: s stays alive and is the sphere base
        nodes = R.flatten(t, s)
        rec = {"spheres": sha(s), "tree": sha(nodes), "nodes": len(nodes), "hits": sha(R.intersect(t, s, rays)),
               "frame_tree": sha(R.render(cam, s, t, depth=5, mode=1, threads=8)),
               "frame_brute": sha(R.render(cam, s, t, depth=5, mode=1, threads=8, use_bvh=False))}
        R.free(t)
        scenes[name] = rec
        print(name, rec["nodes"], rec["tree"][:16], flush=True)
    G = {"generated_by": "tests/golden/make_golden_hostile_spheres.py from oracle/_ref (unmodified reference sources)",
         "size": [W, H], "scenes": scenes}
    with open(os.path.join(OUT, "hostile_spheres.json"), "w") as f:
        json.dump(G, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
