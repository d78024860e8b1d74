#!/usr/bin/env python3
"""Times the light-sampling frame (rtx_render_nee_device) against the plain fixed-spp wavefront
frame (rtx_render_device) and against rtx_radiance_device on the same camera rays, with HIP events
on one stream, and records both estimators' error against a long plain render.
Needs a GPU.

    python scripts/measure_nee.py [--preset cornell] [--spp 16] [--repeats 10] [--out FILE.json]

The Cornell box at the preset's size and depth.  Each timing: 3 warm-up calls, then the median (and
minimum) of `repeats`.  The error rows: a 60 x 40 tile in the middle of the frame, the reference a
4096-spp plain render of it; each estimator's RMS error at `spp` samples over 8 seeds; the
equal-time variance ratio is (MSE_plain x ms_plain) / (MSE_nee x ms_nee) with the whole frame's
times.  No threshold is attached to any figure."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3360-ray-tracer_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from measure_direct import timed  # noqa: E402


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
    ms = {}
    for precision in ("parity", "fast"):
        prm = rtx.RenderParams()
        prm.spp, prm.max_depth, prm.adaptive, prm.seed = K, depth, 0, seed
        prm.mode, prm.precision = rtx.MODES["wavefront"], rtx.PRECISIONS[precision]

        def nee(counts=False):
            dev.render_nee_device(cam, d_rgb.data_ptr(), K, depth, seed=seed, precision=precision,
                                  d_segments=d_segs.data_ptr() if counts else 0, stream=sp)

        def plain(counts=False):
            return dev.render_device(cam, prm, d_rgb.data_ptr(), stream=sp, stats=counts)

        def query(counts=False):
            for k in range(K):
                dev.radiance_device(d_rays[k].data_ptr(), n, d_rgb.data_ptr(), 1, depth, seed=seed, first_sample=k,
                                    precision=precision, d_ids=d_ids.data_ptr(),
                                    d_segments=d_segs.data_ptr() if counts else 0, stream=sp)

        nee(counts=True)
        stream.synchronize()
        nee_segments = int(d_segs.sum(dtype=torch.int64).item())
        closest = int(plain(counts=True)["rays_total"])
        for what, fn, segs in (("rtx_render_nee_device", nee, dict(segments=nee_segments, closest_hit=closest,
                                                                   shadow=nee_segments - closest)),
                               ("rtx_render_device, wavefront, fixed", plain, dict(segments=closest)),
                               ("rtx_radiance_device, the camera rays, one call per sample", query,
                                dict(segments=closest))):
            med, mn = timed(fn, stream, args.repeats)
            row = dict(what="%s (%d spp, depth %d, %s)" % (what, K, depth, precision), ms=med, min_ms=mn, **segs)
            row["segments_per_s"] = row["segments"] / (med * 1e-3)
            res["rows"].append(row)
            ms[(what.split(",")[0], precision)] = med
            print(json.dumps(row), flush=True)

    # both estimators' error against a long plain render of a tile (parity walk)
    tile = ((W - 60) // 2, (H - 40) // 2, 60, 40)
    ref, _, _ = dev.render(cam, args.ref_spp, depth, seed=99, adaptive=False, mode="wavefront", tile=tile)
    mse = {"nee": [], "plain": []}
    for s in range(8):
        a, _ = dev.render_nee(cam, K, depth, seed=1000 + s, tile=tile)
        b, _, _ = dev.render(cam, K, depth, seed=1000 + s, adaptive=False, mode="wavefront", tile=tile)
        mse["nee"].append(float(np.mean((a - ref) ** 2)))
        mse["plain"].append(float(np.mean((b - ref) ** 2)))
    m_nee, m_plain = float(np.mean(mse["nee"])), float(np.mean(mse["plain"]))
    t_nee, t_plain = ms[("rtx_render_nee_device", "parity")], ms[("rtx_render_device", "parity")]
    row = dict(tile=list(tile), reference_spp=args.ref_spp, spp=K, seeds=8, rms_nee=m_nee ** 0.5, rms_plain=m_plain ** 0.5,
               mse_ratio_equal_spp=m_plain / m_nee, ms_nee=t_nee, ms_plain=t_plain,
               variance_ratio_equal_time=(m_plain * t_plain) / (m_nee * t_nee))
    res["error"].append(row)
    print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
