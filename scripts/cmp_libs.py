#!/usr/bin/env python3
"""Bit-for-bit comparison of two librtx builds (A/B kernel variants) on small renders.

    python scripts/cmp_libs.py A.so B.so [renders|queries]     (run on the GPU box; default: both)

Each library renders the same scenes in a child process (RTX_LIB selects the build); the
linear framebuffers, per-pixel sample counts and segment counts must be identical for a
variant that claims to be a pure scheduling / code-motion change.

The query section (query_cases) does the same for the ray queries, the sampled films and their test
hooks on a 32 x 24 frame: every array either library returns is compared as a uint64 / uint32 view.
"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [  # scene recipe, camera preset, width, spp, depth, mode, precision, adaptive
    ("final", "c2_final", 96, 16, 50, "persistent", "fast", False),
    ("final", "c2_final", 96, 16, 50, "persistent", "parity", True),
    ("mixed", "c5_mixed", 96, 8, 50, "persistent", "fast", False),
    ("bunny", "c3_bunny", 96, 8, 20, "persistent", "fast", False),
    ("cornell", "cornell", 64, 16, 50, "persistent", "fast", False),
    ("final", "c2_final", 64, 8, 50, "wavefront", "fast", False),
    ("final", "c2_final", 48, 100, 50, "persistent", "fast", False),  # many accumulate chunks
    ("bunny", "c3_bunny", 48, 37, 20, "persistent", "fast", False),  # odd K: unaligned runs
    ("bunny", "c3_bunny", 160, 16, 20, "persistent", "fast", False, "park"),  # the PARK kernel, forced
    ("mixed", "c5_mixed", 96, 8, 50, "persistent", "fast", False, "park"),
    ("cornell", "cornell", 64, 16, 50, "persistent", "fast", False, "park"),
    ("bunny", "c3_bunny", 160, 16, 20, "persistent", "fast", False, "park_step"),  # PARK, leaf-step walk
    ("bunny", "c3_bunny", 400, 64, 20, "persistent", "fast", True),  # adaptive, two sub-renders
    ("final", "c2_final", 400, 48, 50, "persistent", "fast", True),
]


def query_cases(rtx, res):
    """Every query form on the smallest shapes that reach its seams, into res[name] = array."""
    spp, s0, depth = 5, 3, 6
    for scene in ("cornell", "mixed"):
        dev = rtx.DeviceScene(rtx.HostScene.recipe(scene, 1234), device=0)
        cam = rtx.camera(rtx.camera_config("cornell" if scene == "cornell" else "c5_mixed", width=32, aspect=32 / 24))
        assert (cam.image_width, cam.image_height) == (32, 24)
        rays = rtx.camera_rays(dev, cam, 1, seed=7)[:, 0, :]
        n = len(rays)
        ids = (np.arange(n, dtype=np.uint32) * 7919 + 11) % 100003  # explicit, non-contiguous
        hits = dev.intersect(rays, precision="parity")
        on = hits["hit"] != 0
        pts, nrm = np.ascontiguousarray(hits["p"][on]), np.ascontiguousarray(hits["normal"][on])
        sid = ids[on]

        def put(name, value):
            for k, a in enumerate(value if isinstance(value, tuple) else (value,)):
                res[f"q {scene} {name} [{k}]"] = np.ascontiguousarray(a)

        for prec in ("parity", "fast"):
            for chunk in (0, 64, 3):  # default; whole-ray chunks with seams; spp above the cap (the carry)
                rtx.radiance_chunk(chunk)
                t = f"{prec} chunk {chunk}"
                kw = dict(seed=99, first_sample=s0, precision=prec)
                put(f"radiance {t}", dev.radiance(rays, spp, depth, ids=ids, segments=True, **kw))
                put(f"irradiance {t}", dev.irradiance(pts, nrm, spp, depth, ids=sid, segments=True, **kw))
                put(f"direct {t}", dev.direct(pts, nrm, spp, ids=sid, visible=True, **kw))
                put(f"radiance_nee {t}", dev.radiance_nee(rays, spp, depth, ids=ids, segments=True, **kw))
                put(f"radiance_mis {t}", dev.radiance_mis(rays, spp, depth, ids=ids, segments=True, **kw))
                put(f"render_nee {t}", dev.render_nee(cam, spp, depth, seed=99, precision=prec, tile=(5, 3, 17, 11)))
                put(f"render_mis {t}", dev.render_mis(cam, spp, depth, seed=99, precision=prec))
            rtx.radiance_chunk(0)
            for est in ("nee", "mis"):
                f = dev.film(cam, depth, seed=99, adaptive=False, precision=prec, estimator=est)
                for budget in (2, 5):
                    f.render(budget)
                    put(f"film {est} fixed {prec} at {budget}", f.resolve())
                f.close()
                rtx.film_group(1, 3)
                f = dev.film(cam, depth, seed=99, adaptive=True, precision=prec, estimator=est, min_spp=2,
                             rel_threshold=0.05)
                st = f.render(12)
                put(f"film {est} adaptive {prec}", f.resolve() + (np.array([st["rays_recorded"]], np.uint64),))
                f.close()
                rtx.film_group(0, 0)
            t = dict(spp=spp, max_depth=depth, seed=99, cap=8, ids=ids, first_sample=s0, precision=prec)
            for name, tr in (("nee_trace", rtx.nee_trace(dev, rays, **t)), ("mis_trace", rtx.mis_trace(dev, rays, **t))):
                put(f"{name} {prec}", tuple(tr[k] for k in sorted(tr)))
        put("irradiance_rays", rtx.irradiance_rays(dev, pts, nrm, spp, 99, ids=sid, first_sample=s0))
        put("direct_samples", rtx.direct_samples(dev, pts, nrm, spp, 99, ids=sid, first_sample=s0))
        for d in (0, 3):
            put(f"nee_samples depth {d}", rtx.nee_samples(dev, pts, nrm, spp, 99, d, ids=sid, first_sample=s0))


def tree_cases(rtx, res):
    """The trees each stock scene holds on the device after its upload (rtx.scene_trees), as bytes."""
    for scene in ("three", "final", "mixed", "bunny", "cornell"):
        dev = rtx.DeviceScene(rtx.HostScene.recipe(scene, 1234), device=0)
        for k, a in enumerate(rtx.scene_trees(dev)):
            res[f"q trees {scene} [{k}]"] = np.frombuffer(a.tobytes(), np.uint8)


def child(out, what):
    sys.path.insert(0, os.path.join(ROOT, "3360-ray-tracer_amd"))
    import torch  # noqa: F401  (HIP runtime before librtx, as bench.py)

    import rtx

    res = {}
    if what != "renders":
        query_cases(rtx, res)
        tree_cases(rtx, res)
    for i, (scene, preset, w, spp, depth, mode, prec, adaptive, *sched) in enumerate(CASES if what != "queries" else []):
        dev = rtx.DeviceScene(rtx.HostScene.recipe(scene, 1234), device=0)
        cam = rtx.camera(rtx.camera_config(preset, width=w))
        rgb, n, st = dev.render(cam, spp, depth, seed=1234, adaptive=adaptive, mode=mode, precision=prec,
                                **({"schedule": sched[0]} if sched else {}))
        res[f"rgb{i}"], res[f"spp{i}"] = rgb, n
        res[f"rays{i}"] = np.array([st["rays_total"]])
    np.savez(out, **res)


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        return child(sys.argv[2], sys.argv[3])
    a, b = sys.argv[1:3]
    what = sys.argv[3] if len(sys.argv) > 3 else "all"
    outs = []
    for k, lib in enumerate((a, b)):
        out = os.path.join(ROOT, "gpurun_out", f"cmp_{k}.npz")
        env = dict(os.environ, RTX_LIB=os.path.abspath(lib) if lib != "default" else "")
        subprocess.run([sys.executable, __file__, "--child", out, what], env=env, check=True)
        outs.append(np.load(out))
    report = {}
    ok = True
    names = sorted(k for k in set(outs[0].files) | set(outs[1].files) if k.startswith("q "))
    for k in names:  # the query section: every array, bit for bit
        same = k in outs[0].files and k in outs[1].files and outs[0][k].shape == outs[1][k].shape
        if same:
            view = np.uint64 if outs[0][k].dtype.itemsize == 8 else np.uint32 if outs[0][k].dtype.itemsize == 4 else np.uint8
            same = outs[0][k].dtype == outs[1][k].dtype and np.array_equal(outs[0][k].view(view), outs[1][k].view(view))
        report[k] = {"bit_identical": bool(same), "shape": list(outs[0][k].shape) if k in outs[0].files else None}
        ok &= bool(same)
    for i, case in enumerate(CASES if what != "queries" else []):
        ra, rb = outs[0][f"rgb{i}"], outs[1][f"rgb{i}"]
        same = np.array_equal(ra.view(np.uint64), rb.view(np.uint64))
        frac = float(np.mean(np.all(ra.view(np.uint64) == rb.view(np.uint64), axis=-1)))
        spp_same = np.array_equal(outs[0][f"spp{i}"], outs[1][f"spp{i}"])
        rays_same = int(outs[0][f"rays{i}"][0]) == int(outs[1][f"rays{i}"][0])
        report[" ".join(map(str, case))] = {"bit_identical": bool(same), "pixels_identical": frac,
                                            "spp_identical": bool(spp_same), "rays_identical": bool(rays_same)}
        # adaptive renders trace whole batches, so the segments traced (not the result) depend on
        # the batch schedule
        ok &= same and spp_same and (rays_same or case[7])
    print(json.dumps(report, indent=1))
    print("ALL BIT-IDENTICAL" if ok else "DIFFERENCES FOUND")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
