#!/usr/bin/env python3
"""Times rtx_occluded_device against rtx_intersect_device on the same device-resident rays, and
rtx_ao_device against the two-step path (first hit, ray buffer, rtx_occluded_device), with HIP
events on one stream.  Needs a GPU.

    python scripts/measure_occlusion.py [--repeats 10] [--ao-width 1024] [--out FILE.json]

Ray sets, both on the bunny: the 64 x 36 x 16 AO sample rays (rtx_internal_ao_rays, radius 1.5;
the rays of missed pixels dropped) tiled to at least 4 M rays and traced on (tmin, radius); and
2732 x 1536 = 4.2 M primary rays of the c3_bunny camera on (tmin, inf).  Each timing: 3 warm-up
launches of both kernels, then `repeats` rounds alternating the two, the median per kernel."""
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
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def ab(fa, fb, stream, repeats):
    torch.cuda.synchronize()  # the buffers were filled on the default stream
    for _ in range(3):
        fa(), fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(repeats):
        ta.append(timed(fa, stream, repeats))
        tb.append(timed(fb, stream, repeats))
    return float(np.median(ta)), float(np.median(tb)), float(np.min(ta)), float(np.min(tb))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--ao-width", type=int, default=1024, help="width of the AO frame (16:9)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    torch.cuda.init()
    import rtx

    lib = rtx.lib()
    stream = torch.cuda.Stream()  # the library's launches and the events share this stream
    sp = C.c_void_p(stream.cuda_stream)
    dev = rtx.DeviceScene(rtx.HostScene.load(os.path.join(ROOT, "tests", "golden", "scenes", "bunny.rtxs")))
    tmin, radius = rtx.RTX_SEAM_TMIN, 1.5
    cam64 = rtx.camera(rtx.camera_config("c3_bunny", width=64))
    ao = rtx.ao_rays(dev, cam64, samples=16, radius=radius, seed=1234).reshape(-1, 6)
    ao = ao[np.any(ao[:, 3:] != 0, 1)]
    ao = np.tile(ao, (-(-(4 << 20) // len(ao)), 1))
    big = rtx.camera(rtx.camera_config("c3_bunny", width=2732))
    jj, ii = np.mgrid[0:big.image_height, 0:big.image_width]
    c, p00, du, dv = (np.array(list(v)) for v in (big.center, big.pixel00, big.pixel_delta_u, big.pixel_delta_v))
    d = p00 + ii.reshape(-1, 1) * du + jj.reshape(-1, 1) * dv - c
    primary = np.hstack([np.broadcast_to(c, d.shape), d])
    res = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "rays": []}
    for name, rays, tmax in (("ao_rays_tiled", ao, radius), ("primary_2732x1536", primary, float("inf"))):
        n = len(rays)
        d_rays = torch.from_numpy(np.ascontiguousarray(rays)).cuda()
        d_hits = torch.empty(n * 88, dtype=torch.uint8, device="cuda")
        d_occ = torch.empty(n, dtype=torch.uint8, device="cuda")
        for prec in ("parity", "fast"):
            p = rtx.PRECISIONS[prec]

            def f_int():
                rtx._check(lib.rtx_intersect_device(dev.h, C.c_void_p(d_rays.data_ptr()), n, C.c_void_p(d_hits.data_ptr()),
                                                    tmin, tmax, p, sp), "rtx_intersect_device")

            def f_occ():
                rtx._check(lib.rtx_occluded_device(dev.h, C.c_void_p(d_rays.data_ptr()), n, C.c_void_p(d_occ.data_ptr()),
                                                   tmin, tmax, p, sp), "rtx_occluded_device")

            ti, to, mi, mo = ab(f_int, f_occ, stream, args.repeats)
            hit = d_hits.cpu().numpy().view(np.int32).reshape(n, 22)[:, 0] != 0
            same = bool(np.array_equal(hit, d_occ.cpu().numpy() != 0))
            row = dict(rays=name, n=n, precision=prec, intersect_ms=ti, occluded_ms=to, intersect_min_ms=mi,
                       occluded_min_ms=mo, ratio=ti / to, hit_share=float(hit.mean()), flags_equal=same)
            res["rays"].append(row)
            print(json.dumps(row), flush=True)
        del d_rays, d_hits, d_occ
    # the fused AO kernel against first hit + ray buffer + rtx_occluded_device.  The ray buffer is
    # made beforehand (writing it is NOT charged to the two-step path) and holds the rays of the hit
    # pixels only, as a caller would build it (the hook's all-zero rays of missed pixels have no
    # direction: the fast walk's slabs cannot cull them and they would visit the whole tree)
    cam = rtx.camera(rtx.camera_config("c3_bunny", width=args.ao_width))
    npix = cam.image_width * cam.image_height
    res["ao"] = []
    for prec in ("parity", "fast"):
        prm, aop, _ = dev._ao_args(cam, 16, radius, 1234, None, None, prec)
        rays = rtx.ao_rays(dev, cam, samples=16, radius=radius, seed=1234, precision=prec).reshape(-1, 6)
        jj, ii = np.mgrid[0:cam.image_height, 0:cam.image_width]
        c, p00, du, dv = (np.array(list(v)) for v in (cam.center, cam.pixel00, cam.pixel_delta_u, cam.pixel_delta_v))
        dd = p00 + ii.reshape(-1, 1) * du + jj.reshape(-1, 1) * dv - c
        d_first = torch.from_numpy(np.ascontiguousarray(np.hstack([np.broadcast_to(c, dd.shape), dd]))).cuda()
        d_hits = torch.empty(npix * 88, dtype=torch.uint8, device="cuda")
        live = np.any(rays[:, 3:] != 0, 1)
        rays = rays[live]
        d_rays = torch.from_numpy(np.ascontiguousarray(rays)).cuda()
        d_occ = torch.empty(len(rays), dtype=torch.uint8, device="cuda")
        d_ao = torch.empty(npix, dtype=torch.float64, device="cuda")
        p = rtx.PRECISIONS[prec]

        def f_fused():
            rtx._check(lib.rtx_ao_device(dev.h, C.byref(cam), C.byref(prm), C.byref(aop), C.c_void_p(d_ao.data_ptr()), sp),
                       "rtx_ao_device")

        def f_two():
            rtx._check(lib.rtx_intersect_device(dev.h, C.c_void_p(d_first.data_ptr()), npix, C.c_void_p(d_hits.data_ptr()),
                                                tmin, float("inf"), p, sp), "rtx_intersect_device")
            rtx._check(lib.rtx_occluded_device(dev.h, C.c_void_p(d_rays.data_ptr()), len(rays), C.c_void_p(d_occ.data_ptr()),
                                               tmin, radius, p, sp), "rtx_occluded_device")

        tf, tt, mf, mt = ab(f_fused, f_two, stream, args.repeats)
        occ = np.zeros(npix * 16, np.uint8)
        occ[live] = d_occ.cpu().numpy()
        want = 1.0 - occ.reshape(npix, 16).mean(1)
        row = dict(frame="%dx%d" % (cam.image_width, cam.image_height), samples=16, precision=prec, fused_ms=tf,
                   two_step_ms=tt, fused_min_ms=mf, two_step_min_ms=mt, ratio=tt / tf, hit_pixels=float(live.mean()),
                   equal=bool(np.array_equal(d_ao.cpu().numpy(), want)))
        res["ao"].append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
