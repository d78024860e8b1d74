"""The global primitives' test specialised for plain spheres (trav_globals, rtx_device.h: uniform
loads of a record whose g[4] the host filled with radius * radius, one division where h - sq <= 0
decides the near root): fast precision must report the parity walk's closest hit, bit for bit,
except for exact t ties between two primitives, which are checked with the oracle's brute force
as test_gpu_parity.py::test_intersect_fast_matches_parity does.  No agreement rate is tolerated.
And every schedule's kernel, which all start their walks through trav_globals, renders the same
bunny frame bit for bit, in as many segments as the oracle.

What these cases do not show: whether a scene took the specialised or the generic test.  The flag
lives in the kernel argument only (no query exposes it; the export list is pinned), so with the
flag never set every case here would still pass, and `negative_radius` cannot show that it took
the generic path.  That the specialised path runs on the bunny is shown by the profile pair under
profiles/r07 (vector-memory reads per launch 311 M -> 288 M), not by this file."""

import numpy as np
import pytest

from conftest import scene_path

pytestmark = pytest.mark.gpu
COLS = [0, 1, 2, 3, 4, 5, 6, 7, 10, 11]
HEAD = ["rtxscene 1", "bvh 1", "tex 0 solid 0.5 0.5 0.5", "mat 0 lambertian 0"]
SMALL = ["sphere -1.5 0.5 0 0.5 0", "sphere 1.25 0.75 0.5 0.75 0"]
MORE = ["sphere 0 2.5 -2 0.5 0", "sphere 3 0.4 2 0.4 0", "sphere -3 1 -3 1 0"]
# name -> (scene lines or a scene file, the ground's centre and radius, globals the fast tree leaves out)
SCENES = {
    "bunny": (None, (0.0, -1003.9, 0.0), 1000.0, 1),
    # (three primitives: the reference tree's root is a leaf, the fast path walks the flat list)
    "ground_two": (HEAD + ["sphere 0 -1000 0 1000 0"] + SMALL, (0.0, -1000.0, 0.0), 1000.0, None),
    "ground_five": (HEAD + ["sphere 0 -1000 0 1000 0"] + SMALL + MORE, (0.0, -1000.0, 0.0), 1000.0, 1),
    "two_globals": (HEAD + ["sphere 0 -1000 0 1000 0", "sphere 0 -1000 0 950 0"] + SMALL +
                    ["sphere 0 2.5 -2 0.5 0"], (0.0, -1000.0, 0.0), 1000.0, 2),
    # fmax(0, radius) makes it a point: its record is read as any primitive's (the unspecialised path)
    "negative_radius": (HEAD + ["sphere 0 -1000 0 -1000 0"] + SMALL + MORE, (0.0, -1000.0, 0.0), 1000.0, 1),
}


def hit_matrix(h):
    return np.column_stack([h["hit"], h["t"], h["p"], h["normal"], h["u"], h["v"], h["front_face"], h["material"]])


def rays_for(centre, radius, seed):
    """4096 rays: a quarter as a render sends them, a quarter starting on the global's surface, a quarter
    from there along its tangent plane, a quarter just off the surface aimed across the horizon."""
    rng = np.random.default_rng(seed)
    n = 1024
    c = np.asarray(centre)
    o = np.column_stack([rng.uniform(-8, 8, n), rng.uniform(0.05, 6, n), rng.uniform(-8, 8, n)])
    t = np.column_stack([rng.uniform(-6, 6, n), rng.uniform(-3, 3, n), rng.uniform(-6, 6, n)])
    free = np.hstack([o, t - o])
    xz = rng.uniform(-6, 6, (3 * n, 2))
    up = np.column_stack([xz[:, 0], np.sqrt(radius * radius - (xz ** 2).sum(1)), xz[:, 1]])
    on = c + up  # points of the surface near its top
    nrm = up / radius
    d = rng.normal(size=(3 * n, 3))
    tang = d - (d * nrm).sum(1, keepdims=True) * nrm  # in the tangent plane
    d[n:2 * n] = tang[n:2 * n]
    on[2 * n:] += nrm[2 * n:] * rng.choice([1e-9, -1e-9, 1e-4, 2e-3], n)[:, None]
    d[2 * n:] = tang[2 * n:] + nrm[2 * n:] * (rng.uniform(-1, 1, n) * 2.0 ** -rng.integers(4, 50, n))[:, None]
    return np.vstack([free, np.hstack([on, d])])


@pytest.mark.parametrize("name", list(SCENES))
def test_fast_hits_equal_parity_hits(rtx_mod, orc, gpu, tmp_path, name):
    lines, centre, radius, want_globals = SCENES[name]
    path = scene_path("bunny") if lines is None else str(tmp_path / (name + ".rtxs"))
    if lines is not None:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
    host = rtx_mod.HostScene.load(path)
    info, _ = rtx_mod.fast_tree(host)
    if want_globals is not None:
        assert info["fast_ok"] == 1 and info["n_global"] == want_globals, info
    d = rtx_mod.DeviceScene(host)
    rays = rays_for(centre, radius, 7)
    a = hit_matrix(d.intersect(rays, precision="parity"))
    b = hit_matrix(d.intersect(rays, precision="fast"))
    differ = np.nonzero(~np.all(a[:, COLS] == b[:, COLS], 1))[0]
    osc = orc.Scene(path) if len(differ) else None
    for i in differ:
        assert a[i, 0] == 1 and b[i, 0] == 1, ("hit/miss mismatch", i, a[i], b[i])
        assert a[i, 1] == b[i, 1], ("closest distances differ", i, a[i, 1], b[i, 1])
        tied, n = osc.tied_hits(rays[i], a[i, 1])
        assert n >= 2, ("not a tie", i, n, a[i], b[i])
        recs = tied[:, COLS]
        assert np.any(np.all(recs == a[i, COLS], 1)) and np.any(np.all(recs == b[i, COLS], 1)), (i, tied, a[i], b[i])


def test_bunny_frame_identical_through_every_schedule(rtx_mod, orc, gpu):
    path = scene_path("bunny")
    d = rtx_mod.DeviceScene(rtx_mod.HostScene.load(path))
    cam = rtx_mod.camera(rtx_mod.camera_config("c3_bunny", width=64))
    assert (cam.image_width, cam.image_height) == (64, 36)
    frames = {}
    for key, kw in (("plain", dict(schedule="plain")), ("park", dict(schedule="park")),
                    ("park_step", dict(schedule="park_step")), ("auto", dict(schedule="auto")),
                    ("generic", dict(schedule="auto", generic=True))):
        rgb, _, st = d.render(cam, spp=8, max_depth=20, seed=1234, adaptive=False, mode="persistent",
                              precision="fast", **kw)
        frames[key] = (np.array(rgb, copy=True), st["rays_total"])
    _, _, ref_st = orc.Scene(path).render(orc.camera_preset("c3_bunny"), 64, 8, 20, 1234, adaptive=0, rng="philox",
                                          mode="per_pixel", threads=4)
    first = frames["plain"][0]
    for key, (rgb, rays) in frames.items():
        assert rays == ref_st["rays"], (key, rays, ref_st["rays"])
        assert np.array_equal(rgb.view(np.uint8), first.view(np.uint8)), key
