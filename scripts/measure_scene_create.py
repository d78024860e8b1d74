#!/usr/bin/env python3
"""Wall time of rtx_scene_create (plan, upload, one wait) on the bunny scene, on the GPU box.

    RTX_LIB=<librtx build> python scripts/measure_scene_create.py [--runs 5]

One warm-up create (the device's first use), then `runs` timed create / destroy cycles; prints
one JSON line with every run in ms.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3360-ray-tracer_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    import torch  # noqa: F401  (HIP runtime before librtx, as bench.py)

    import rtx

    host = rtx.HostScene.recipe("bunny", 1234)
    del_ = rtx.DeviceScene(host, device=0)
    del del_
    ms = []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        dev = rtx.DeviceScene(host, device=0)
        ms.append((time.perf_counter() - t0) * 1e3)
        del dev
    print(json.dumps({"lib": os.environ.get("RTX_LIB") or "default", "scene": "bunny",
                      "prims": int(host.desc().n_prims), "create_ms": [round(v, 3) for v in ms],
                      "median_ms": round(sorted(ms)[len(ms) // 2], 3), "max_ms": round(max(ms), 3)}))


if __name__ == "__main__":
    main()
