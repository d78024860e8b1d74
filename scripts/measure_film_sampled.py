#!/usr/bin/env python3
"""Times the sampled films (rtx_film_create_sampled) beside the one-shot MIS frame
(rtx_render_mis_device) in one process, and records the adaptive film's error beside fixed films'.
scripts/measure_mis.py's pattern.  Needs a GPU.

    python scripts/measure_film_sampled.py [--preset cornell] [--repeats 10] [--out FILE.json]

The Cornell box at the preset's size and depth, seed 1234.  Each timing: 3 warm-up calls, then the
median (and minimum) of `repeats`, HIP events on one stream: the one-shot frame's around the call on
a stream of the caller's, a film's from rtx_stats.kernel_ms of its render calls on the scene's
stream (the film is reset before each).  Rows: the one-shot frame at 16 and 64 spp; the fixed film at
those budgets in 1 and in 4 chunks; the adaptive film at budget 64, min_spp 16, threshold 0.05f,
with later groups of 4 and of 8 samples, with its traced and recorded segments, mean spp and groups
(path-kernel launches).  Error rows: RMS of the adaptive film and of fixed films at 16 and 64 spp
against a 4096-spp MIS render of the 60 x 40 tile in the middle of the frame, over 8 seeds.  No
threshold is attached to any figure."""
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


def film_timed(make, budgets, repeats):
    """(median ms, min ms, last call's summed stats) of a film rendered to `budgets` in turn."""
    film = make()
    ms, total = [], None
    for i in range(3 + repeats):
        film.reset()
        total = {}
        for b in budgets:
            for k, v in film.render(b).items():
                total[k] = total.get(k, 0) + v
        if i >= 3:
            ms.append(total["kernel_ms"])
    spp = film.resolve()[1]
    film.close()
    return float(np.median(ms)), float(np.min(ms)), total, float(spp.mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="cornell")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    torch.cuda.init()
    import rtx

    seed = 1234
    stream = torch.cuda.Stream()
    dev = rtx.DeviceScene(rtx.HostScene.load(os.path.join(ROOT, "tests", "golden", "scenes", "cornell.rtxs")))
    cfg = rtx.camera_config(args.preset)
    cam = rtx.camera(cfg)
    depth = cfg.max_depth
    W, H = cam.image_width, cam.image_height
    d_rgb = torch.zeros((W * H, 3), dtype=torch.float64, device="cuda")
    res = {"device": torch.cuda.get_device_name(0), "frame": "%dx%d" % (W, H), "max_depth": depth,
           "repeats": args.repeats, "rows": [], "error": []}

    def row(what, med, mn, **more):
        r = dict(what=what, ms=med, min_ms=mn, **more)
        res["rows"].append(r)
        print(json.dumps(r), flush=True)

    for K in (16, 64):
        med, mn = timed(lambda: dev.render_mis_device(cam, d_rgb.data_ptr(), K, depth, seed=seed,
                                                      stream=stream.cuda_stream), stream, args.repeats)
        row("rtx_render_mis_device (%d spp)" % K, med, mn)
        for chunks in (1, 4):
            budgets = [-(-k * K // chunks) for k in range(1, chunks + 1)]
            med, mn, st, _ = film_timed(lambda: dev.film(cam, depth, seed=seed, adaptive=False, estimator="mis"),
                                        budgets, args.repeats)
            row("fixed MIS film (%d spp, %d chunks)" % (K, chunks), med, mn, segments=st["rays_total"],
                hot_ms=st["hot_kernel_ms"])
    for G in (4, 8):
        rtx.film_group(0, G)
        med, mn, st, mean_spp = film_timed(lambda: dev.film(cam, depth, seed=seed, adaptive=True, estimator="mis"),
                                           [64], args.repeats)
        row("adaptive MIS film (budget 64, min_spp 16, rel 0.05f, G = %d)" % G, med, mn, traced=st["rays_total"],
            recorded=st["rays_recorded"], mean_spp=mean_spp, groups=st["hot_launches"], hot_ms=st["hot_kernel_ms"],
            samples_traced=st["paths"])
    rtx.film_group()

    tile = ((W - 60) // 2, (H - 40) // 2, 60, 40)
    ref, _ = dev.render_mis(cam, args.ref_spp, depth, seed=99, tile=tile)
    mse = {"adaptive": [], "fixed16": [], "fixed64": []}
    spp_mean = []
    for s in range(8):
        fa = dev.film(cam, depth, seed=1000 + s, adaptive=True, estimator="mis", tile=tile)
        fa.render(64)
        rgb, spp = fa.resolve()
        spp_mean.append(float(spp.mean()))
        mse["adaptive"].append(float(np.mean((rgb - ref) ** 2)))
        fa.close()
        for K in (16, 64):
            img, _ = dev.render_mis(cam, K, depth, seed=1000 + s, tile=tile)
            mse["fixed%d" % K].append(float(np.mean((img - ref) ** 2)))
    err = dict(tile=list(tile), reference_spp=args.ref_spp, seeds=8, adaptive_mean_spp=float(np.mean(spp_mean)),
               **{"rms_" + k: float(np.mean(v)) ** 0.5 for k, v in mse.items()})
    res["error"].append(err)
    print(json.dumps(err), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
