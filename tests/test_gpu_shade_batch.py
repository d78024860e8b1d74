"""Batched shading in the persistent kernel (k_persistent, kShade): a lane whose walk missed or is
at the depth limit ends its path at once (shade_terminal), a lane with a hit to shade waits until
enough lanes of its wave hold one.  When a segment is shaded must not change what it computes, so
every persistent schedule has to render the frame the wavefront renderer does, which shades each
segment of a queue independently: equal pixels bit for bit and equal segment counts, at the same
precision.  The cases are the ones where the loop's progress rule, the depth limit or the mix of
pending and ending lanes is unusual: frames of fewer slots than the threshold and than one wave,
the depth limit at 1 and 2, closed rooms (no ray ever misses: lanes turn pending as fast as they
finish, and paths end inside the batched shading, by roulette, absorption or on a light), a sky-only
view (nothing ever waits), and the non-Lambertian / textured builds.

Every case that is meant to run the PARK kernel asserts that it did (`parked`).  The Cornell box
cannot: its rectangles keep it out of the fast tree, so fast precision renders it with the parity
walk and every schedule launches the plain kernel, which shades every round.  It stays as a check of
that kernel's refactored loop; the closed rooms below are the almost-miss-free case for the PARK
kernel.

The adaptive phase kernel (MAP 1) shades every round and has no case here.

The lanes of a shading round are not in rtx_stats; the last test reads them from the region stamps
a counting build prints with RTX_DEBUG_REGIONS set, in a process of its own (the variable is read
once per process)."""

import json
import os
import re
import subprocess
import sys

import ctypes as C

import numpy as np
import pytest

from conftest import scene_path

pytestmark = pytest.mark.gpu
SCHEDULES = ("plain", "park", "park_step")
# case -> (scene, camera preset, camera overrides, spp, depth)
UP = dict(lookfrom=(0.0, 2.0, 20.0), lookat=(0.0, 22.0, 10.0))  # over the bunny and the ground: sky only
INSIDE = dict(lookfrom=(0.0, 0.5, 7.0), lookat=(0.0, 0.0, 0.0), vfov=70.0)  # inside the rooms' outer sphere
NO_PARK = {"cornell"}  # not in the fast tree: the plain kernel whatever the schedule
# closed rooms: a camera inside a big sphere with smaller ones in it (enough of them for a tree with
# an internal root), so every segment hits; all Lambertian (paths end by roulette, by a failed
# sample or at the depth limit), and the same with a light (the build with every material, paths
# also end on the emitter)
ROOM = ["rtxscene 1", "bvh 1", "tex 0 solid 0.7 0.7 0.7", "mat 0 lambertian 0", "tex 1 solid 0.8 0.3 0.3",
        "mat 1 lambertian 1", "sphere 0 0 0 12 0", "sphere -2.5 -1 0 1.5 1", "sphere 2.5 -1 -1 1.5 0",
        "sphere 0 2 -2 1 1", "sphere -1 -2.5 2 0.75 0", "sphere 1.5 1.5 1.5 0.5 1", "sphere -3 2 1 0.5 0"]
ROOM_LIGHT = ROOM[:6] + ["tex 2 solid 4 4 4", "mat 2 light 2"] + ROOM[6:] + ["sphere 0 5 0 1.5 2"]
CASES = {
    "tiny_3x2": ("bunny", "c3_bunny", dict(width=3, aspect=1.5), 1, 20),
    "tiny_64_slots": ("bunny", "c3_bunny", dict(width=4, aspect=1.0), 4, 20),
    "bunny": ("bunny", "c3_bunny", dict(width=64), 8, 20),
    "bunny_depth1": ("bunny", "c3_bunny", dict(width=64), 8, 1),
    "bunny_depth2": ("bunny", "c3_bunny", dict(width=64), 8, 2),
    "cornell": ("cornell", "cornell", dict(width=36), 4, 20),
    "room": ("room", "c3_bunny", dict(width=48, **INSIDE), 4, 20),
    "room_light": ("room_light", "c3_bunny", dict(width=48, **INSIDE), 4, 20),
    "sky_only": ("bunny", "c3_bunny", dict(width=64, **UP), 8, 20),
    "final": ("final", "c2_final", dict(width=48), 4, 50),
    "mixed": ("mixed", "c5_mixed", dict(width=48), 4, 50),
}


@pytest.fixture(scope="module")
def scenes(rtx_mod, gpu, mixed_scene_file, tmp_path_factory):
    cache = {}
    rooms = {"room": ROOM, "room_light": ROOM_LIGHT}

    def get(name):
        if name not in cache:
            path = mixed_scene_file if name == "mixed" else scene_path(name)
            if name in rooms:
                path = str(tmp_path_factory.mktemp("rooms") / (name + ".rtxs"))
                with open(path, "w") as f:
                    f.write("\n".join(rooms[name]) + "\n")
            cache[name] = rtx_mod.DeviceScene(rtx_mod.HostScene.load(path))
        return cache[name]

    return get


def make_camera(rtx_mod, preset, over):
    over = {k: (C.c_double * 3)(*v) if isinstance(v, tuple) else v for k, v in over.items()}
    return rtx_mod.camera(rtx_mod.camera_config(preset, **over))


@pytest.mark.parametrize("case", list(CASES))
def test_persistent_equals_wavefront(rtx_mod, scenes, case):
    scene, preset, over, spp, depth = CASES[case]
    d = scenes(scene)
    cam = make_camera(rtx_mod, preset, over)
    if case == "tiny_3x2":
        assert (cam.image_width, cam.image_height) == (3, 2)
    if case == "tiny_64_slots":
        assert cam.image_width * cam.image_height * spp == 64
    kw = dict(spp=spp, max_depth=depth, seed=1234, adaptive=False, precision="fast")
    ref, _, ref_st = d.render(cam, mode="wavefront", **kw)
    ref = np.array(ref, copy=True)
    if case == "sky_only":
        assert ref_st["rays_total"] == cam.image_width * cam.image_height * spp  # every primary misses
    if scene.startswith("room"):  # closed: no path ends after one segment, which only a miss does
        assert ref_st["rays_total"] >= 2 * cam.image_width * cam.image_height * spp
    if case == "bunny_depth1":  # primaries, and one more segment for each that hit
        assert cam.image_width * cam.image_height * spp < ref_st["rays_total"] <= 2 * cam.image_width * cam.image_height * spp
    for sched in SCHEDULES:
        rgb, _, st = d.render(cam, mode="persistent", schedule=sched, **kw)
        print(case, sched, "rays", st["rays_total"], "wavefront", ref_st["rays_total"], "parked", st["parked"])
        assert st["parked"] == (0 if sched == "plain" or case in NO_PARK else 1), (case, sched, st["parked"])
        assert st["rays_total"] == ref_st["rays_total"], (case, sched, st["rays_total"], ref_st["rays_total"])
        assert np.array_equal(np.asarray(rgb).view(np.uint8), ref.view(np.uint8)), (case, sched)


def test_counting_build_counts(rtx_mod, scenes):
    """The counting builds of the bunny case: segments as the timed builds count them, and the
    leaf-step PARK kernel, whose lanes make the plain kernel's node visits and primitive tests in
    the same order (trace4_run_step), reports the plain kernel's counts.  The speculative walk
    (`park`) makes those visits and tests and some extra ones, which depend on how a wave's lanes
    line up, so any change of schedule moves its counts: it is held to at least the plain kernel's
    counts and at most 10 % more (before batching it made 3.1 % more visits and 2.2 % more tests on
    this frame: 176684 / 171427 and 65808 / 64373)."""
    d = scenes("bunny")
    cam = make_camera(rtx_mod, "c3_bunny", dict(width=64))
    kw = dict(spp=8, max_depth=20, seed=1234, adaptive=False, mode="persistent", precision="fast")
    _, _, timed = d.render(cam, schedule="park", **kw)
    got = {s: d.render(cam, schedule=s, count=True, **kw)[2] for s in SCHEDULES}
    for s, st in got.items():
        print(s, {k: st[k] for k in ("rays_total", "rays_recorded", "node_visits", "prim_tests")})
        assert "count" in rtx_mod.build_names(st["build"]), s
        assert st["rays_total"] == timed["rays_total"] and st["rays_recorded"] == timed["rays_total"], s
    for k in ("node_visits", "prim_tests"):
        assert got["park_step"][k] == got["plain"][k] > 0, (k, got["park_step"][k], got["plain"][k])
        assert got["plain"][k] <= got["park"][k] <= 1.10 * got["plain"][k], (k, got["park"][k], got["plain"][k])


REGIONS_CHILD = """
import json, sys
sys.path.insert(0, sys.argv[1])
import rtx
d = rtx.DeviceScene(rtx.HostScene.load(sys.argv[2]))
cam = rtx.camera(rtx.camera_config("c3_bunny", width=64))
for sched in ("park", "park_step"):
    st = d.render(cam, spp=8, max_depth=1, seed=1234, adaptive=False, mode="persistent", precision="fast",
                  schedule=sched, count=True)[2]
    sys.stderr.flush()
    print(json.dumps({k: st[k] for k in ("rays_total", "paths", "parked", "build")}), flush=True)
"""


def test_shading_rounds_count_full_shadings_only(rtx_mod, gpu):
    """The counting build's shading rounds and their lanes (`wshade`, `lshade`) count the full
    shading only.  At depth limit 1 the full shading runs exactly once for every primary that hit
    (its second segment is at the depth limit and ends on the sky at once), so with N paths and S
    segments the shaded lanes number at least S - N (the primaries that went on) and at most N;
    counting every lane that finished a walk, as before batching, would give S > N."""
    pkg = os.path.dirname(os.path.dirname(os.path.abspath(rtx_mod.__file__)))
    env = dict(os.environ, RTX_DEBUG_REGIONS="1")
    r = subprocess.run([sys.executable, "-c", REGIONS_CHILD, pkg, scene_path("bunny")], env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    stats = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    regions = re.findall(r"shading rounds (\d+), lanes per shading round ([0-9.]+); segments (\d+)", r.stderr)
    print(stats, regions)
    assert len(stats) == 2 and len(regions) == 2, (r.stdout, r.stderr[-2000:])
    for st, (rounds, lanes, segs) in zip(stats, regions):
        rounds, lanes, segs = int(rounds), float(lanes), int(segs)
        assert st["parked"] == 1 and "count" in rtx_mod.build_names(st["build"])
        n, s = st["paths"], st["rays_total"]
        assert segs == s and n == 64 * 36 * 8 and n < s <= 2 * n
        assert rounds > 0 and 1.0 <= lanes <= 64.0
        shaded, slack = rounds * lanes, rounds * 0.005 + 1  # (the mean is printed to two decimals)
        assert s - n - slack <= shaded <= n + slack, (shaded, s - n, n)
