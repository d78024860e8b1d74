#!/usr/bin/env python3
"""Times the MIS frame (rtx_render_mis_device) beside the light-sampling frame
(rtx_render_nee_device) and rtx_radiance_device on the same camera rays, with HIP events on one
stream, and records all three estimators' error against a long plain render, far from the light
(the Cornell box) and next to one.  scripts/measure_nee.py with a third estimator.
Needs a GPU.

    python scripts/measure_mis.py [--preset cornell] [--spp 16] [--repeats 10] [--out FILE.json]

The Cornell box at the preset's size and depth.  Each timing: 3 warm-up calls, then the median (and
minimum) of `repeats`; the rows of one run are compared with each other, not with stored figures.
The MIS frame's segment counts must equal the light-sampling frame's: asserted.  The error rows: a
60 x 40 tile in the middle of the frame, the reference a 4096-spp plain render of it, each
estimator's RMS error at `spp` samples over 8 seeds; once for the Cornell box and once for a shelf
0.09 below a 4 x 4 light seen through the gap between the two (the scene of
tests/test_gpu_mis.py).  No threshold is attached to any figure."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3360-ray-tracer_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from measure_direct import timed  # noqa: E402

NEAR_LIGHT = """rtxscene 1
bvh 1
tex 0 solid 0.72999999999999998 0.72999999999999998 0.72999999999999998
mat 0 lambertian 0
tex 1 solid 15 15 15
mat 1 light 1
rect xz 0 10 0 10 0 0
rect xz 3 7 3 7 9.9900000000000002 1
rect xz 4 6 4 6 9.9000000000000004 0
"""


def tile_errors(dev, cam, tile, K, depth, ref_spp, name):
    """RMS of the three estimators at K spp against a ref_spp plain render of the tile, 8 seeds."""
    ref, _, _ = dev.render(cam, ref_spp, depth, seed=99, adaptive=False, mode="wavefront", tile=tile)
    mse = {"mis": [], "nee": [], "plain": []}
    for s in range(8):
        a, _ = dev.render_mis(cam, K, depth, seed=1000 + s, tile=tile)
        b, _ = dev.render_nee(cam, K, depth, seed=1000 + s, tile=tile)
        c, _, _ = dev.render(cam, K, depth, seed=1000 + s, adaptive=False, mode="wavefront", tile=tile)
        for key, img in (("mis", a), ("nee", b), ("plain", c)):
            mse[key].append(float(np.mean((img - ref) ** 2)))
    m = {k: float(np.mean(v)) for k, v in mse.items()}
    return dict(scene=name, tile=list(tile), reference_spp=ref_spp, spp=K, seeds=8, max_depth=depth,
                reference_mean=float(ref.mean()), rms_mis=m["mis"] ** 0.5, rms_nee=m["nee"] ** 0.5,
                rms_plain=m["plain"] ** 0.5, mse_nee_over_mis=m["nee"] / m["mis"], mse_plain_over_mis=m["plain"] / m["mis"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="cornell")
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    torch.cuda.init()
    import rtx

    seed, K = 1234, args.spp
    stream = torch.cuda.Stream()  # the library's launches and the events share this stream
    sp = stream.cuda_stream
    dev = rtx.DeviceScene(rtx.HostScene.load(os.path.join(ROOT, "tests", "golden", "scenes", "cornell.rtxs")))
    cfg = rtx.camera_config(args.preset)
    cam = rtx.camera(cfg)
    depth = cfg.max_depth
    W, H = cam.image_width, cam.image_height
    n = W * H
    R = rtx.camera_rays(dev, cam, K, seed=seed)  # (n, K, 6)
    d_rays = [torch.from_numpy(np.ascontiguousarray(R[:, k])).cuda() for k in range(K)]
    del R
    d_ids = torch.arange(n, dtype=torch.int32, device="cuda")
    d_rgb = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    d_segs = torch.zeros(n, dtype=torch.int32, device="cuda")
    count, area = dev.emitters()
    res = {"device": torch.cuda.get_device_name(0), "frame": "%dx%d" % (W, H), "spp": K, "max_depth": depth,
           "repeats": args.repeats, "emitters": count, "emitting_area": area, "rows": [], "error": []}
    for precision in ("parity", "fast"):
        def mis(counts=False):
            dev.render_mis_device(cam, d_rgb.data_ptr(), K, depth, seed=seed, precision=precision,
                                  d_segments=d_segs.data_ptr() if counts else 0, stream=sp)

        def nee(counts=False):
            dev.render_nee_device(cam, d_rgb.data_ptr(), K, depth, seed=seed, precision=precision,
                                  d_segments=d_segs.data_ptr() if counts else 0, stream=sp)

        def query(counts=False):
            for k in range(K):
                dev.radiance_device(d_rays[k].data_ptr(), n, d_rgb.data_ptr(), 1, depth, seed=seed, first_sample=k,
                                    precision=precision, d_ids=d_ids.data_ptr(),
                                    d_segments=d_segs.data_ptr() if counts else 0, stream=sp)

        per_pixel, closest = {}, 0
        for name, fn in (("mis", mis), ("nee", nee)):
            fn(counts=True)
            stream.synchronize()
            per_pixel[name] = d_segs.cpu().numpy().copy()
        assert np.array_equal(per_pixel["mis"], per_pixel["nee"]), "the MIS frame's segment counts are not the NEE frame's"
        segments = int(per_pixel["mis"].astype(np.int64).sum())
        for k in range(K):  # (each call of the query overwrites d_segs)
            dev.radiance_device(d_rays[k].data_ptr(), n, d_rgb.data_ptr(), 1, depth, seed=seed, first_sample=k,
                                precision=precision, d_ids=d_ids.data_ptr(), d_segments=d_segs.data_ptr(), stream=sp)
            stream.synchronize()
            closest += int(d_segs.sum(dtype=torch.int64).item())
        both = dict(segments=segments, closest_hit=closest, shadow=segments - closest)
        for what, fn, segs in (("rtx_render_mis_device", mis, both), ("rtx_render_nee_device", nee, both),
                               ("rtx_radiance_device, the camera rays, one call per sample", query,
                                dict(segments=closest))):
            med, mn = timed(fn, stream, args.repeats)
            row = dict(what="%s (%d spp, depth %d, %s)" % (what, K, depth, precision), ms=med, min_ms=mn, **segs)
            row["segments_per_s"] = row["segments"] / (med * 1e-3)
            res["rows"].append(row)
            print(json.dumps(row), flush=True)

    # the three estimators' error against a long plain render of a tile (parity walk): far from the light ...
    tile = ((W - 60) // 2, (H - 40) // 2, 60, 40)
    row = tile_errors(dev, cam, tile, K, depth, args.ref_spp, "cornell")
    res["error"].append(row)
    print(json.dumps(row), flush=True)
    # ... and next to one: the shelf's top seen through the 0.09 gap under the light, from outside both
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "near_light.rtxs")
        with open(path, "w") as f:
            f.write(NEAR_LIGHT)
        near = rtx.DeviceScene(rtx.HostScene.load(path))
    ncfg = rtx.camera_config(args.preset, vfov=2.0, defocus=0.0)
    ncfg.lookfrom[:] = [5.0, 9.945, 1.0]
    ncfg.lookat[:] = [5.0, 9.9, 5.0]
    ncfg.vup[:] = [0.0, 1.0, 0.0]
    ncam = rtx.camera(ncfg)
    hits = near.intersect(rtx.camera_rays(near, ncam, 1, seed=seed, tile=tile)[:, 0])
    on_shelf = float(np.mean((hits["hit"] != 0) & (np.abs(hits["p"][:, 1] - 9.9) < 1e-9)))
    row = tile_errors(near, ncam, tile, K, depth, args.ref_spp, "near light")
    row["first_hits_on_the_shelf"] = on_shelf
    res["error"].append(row)
    print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
