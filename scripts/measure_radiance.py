#!/usr/bin/env python3
"""Times rtx_radiance_device against rtx_render_device (wavefront and persistent) on the same
samples, with HIP events on one stream.  Needs a GPU.

    python scripts/measure_radiance.py [--width 1000] [--spp 16] [--repeats 10] [--out FILE.json]

The bunny frame of the c3_bunny camera, fast precision, fixed spp, depth 20.  The query runs on the
renderer's own primary rays (rtx_internal_camera_rays), device resident, in two shapes: `per_sample`,
spp calls of one sample each (sample k of every pixel: exactly the render's paths, segment totals
equal), and `one_call`, one call on each pixel's first ray at spp samples (a ray's samples on
adjacent lanes; the same number of paths, statistically the same work).  Each timing: 3 warm-up
calls, then the median (and minimum) of `repeats`."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3360-ray-tracer_amd"))


def timed(fn, stream, repeats):
    torch.cuda.synchronize()
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1000)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--depth", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    torch.cuda.init()
    import rtx

    seed, spp, depth = 1234, args.spp, args.depth
    stream = torch.cuda.Stream()  # the library's launches and the events share this stream
    sp = stream.cuda_stream
    dev = rtx.DeviceScene(rtx.HostScene.load(os.path.join(ROOT, "tests", "golden", "scenes", "bunny.rtxs")))
    cam = rtx.camera(rtx.camera_config("c3_bunny", width=args.width))
    npix = cam.image_width * cam.image_height
    R = rtx.camera_rays(dev, cam, spp, seed=seed)
    d_rays = [torch.from_numpy(np.ascontiguousarray(R[:, k])).cuda() for k in range(spp)]
    del R
    d_ids = torch.arange(npix, dtype=torch.int32, device="cuda")
    d_out = torch.zeros((npix, 3), dtype=torch.float64, device="cuda")
    d_sum = torch.zeros((npix, 3), dtype=torch.float64, device="cuda")
    d_segs = torch.zeros(npix, dtype=torch.int32, device="cuda")
    d_rgb = torch.zeros((npix, 3), dtype=torch.float64, device="cuda")
    res = {"device": torch.cuda.get_device_name(0), "frame": "%dx%d" % (cam.image_width, cam.image_height), "spp": spp,
           "max_depth": depth, "precision": "fast", "repeats": args.repeats, "rows": []}

    def params(mode):
        p = rtx.RenderParams()
        p.spp, p.max_depth, p.adaptive, p.seed = spp, depth, 0, seed
        p.mode, p.precision = rtx.MODES[mode], rtx.PRECISIONS["fast"]
        return p

    # the renders: segment totals from a call with statistics, timings from calls without
    renders = {}
    for mode in ("wavefront", "persistent"):
        p = params(mode)
        st = dev.render_device(cam, p, d_rgb.data_ptr(), stream=sp, stats=True)
        stream.synchronize()
        renders[mode] = d_rgb.cpu().numpy().copy()
        med, mn = timed(lambda: dev.render_device(cam, p, d_rgb.data_ptr(), stream=sp, stats=False), stream, args.repeats)
        row = dict(what="rtx_render_device " + mode, ms=med, min_ms=mn, segments=int(st["rays_total"]),
                   gsegments_per_s=st["rays_total"] / med / 1e6)
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
    res["renders_equal"] = bool(np.array_equal(renders["wavefront"], renders["persistent"]))

    def per_sample(segments=False):
        for k in range(spp):
            dev.radiance_device(d_rays[k].data_ptr(), npix, d_out.data_ptr(), 1, depth, seed=seed, first_sample=k,
                                precision="fast", d_ids=d_ids.data_ptr(), d_segments=d_segs.data_ptr() if segments else 0,
                                stream=sp)
            if segments:
                with torch.cuda.stream(stream):
                    d_sum.add_(d_out)
                    total.add_(d_segs.sum())

    total = torch.zeros((), dtype=torch.int64, device="cuda")
    with torch.cuda.stream(stream):
        d_sum.zero_()
    per_sample(segments=True)
    stream.synchronize()
    segs = int(total.item())
    got = d_sum.cpu().numpy() * (1.0 / float(np.float32(spp)))
    med, mn = timed(per_sample, stream, args.repeats)
    row = dict(what="rtx_radiance_device per_sample (%d calls, spp 1)" % spp, ms=med, min_ms=mn, segments=segs,
               gsegments_per_s=segs / med / 1e6, equals_render=bool(np.array_equal(got, renders["wavefront"])))
    res["rows"].append(row)
    print(json.dumps(row), flush=True)

    def one_call(segments=False):
        dev.radiance_device(d_rays[0].data_ptr(), npix, d_out.data_ptr(), spp, depth, seed=seed, precision="fast",
                            d_ids=d_ids.data_ptr(), d_segments=d_segs.data_ptr() if segments else 0, stream=sp)

    one_call(segments=True)
    stream.synchronize()
    segs = int(d_segs.sum().item())
    med, mn = timed(one_call, stream, args.repeats)
    row = dict(what="rtx_radiance_device one_call (spp %d)" % spp, ms=med, min_ms=mn, segments=segs,
               gsegments_per_s=segs / med / 1e6)
    res["rows"].append(row)
    print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
