"""The oracle's step-level export (orc_shade_steps) and the device hook's arguments, without a GPU.

orc_shade_steps runs one shade() per case, the function every oracle render goes through, which
the reference's goldens pin (tests/test_oracle_golden.py).  This file pins the export to that path:
chained over the oracle's own primary rays and closest hits at max_depth = 1 (the primary segment's
step, then the depth-limit sky end of whatever continues), it reproduces render_samples' per-sample
radiance and segment counts bit for bit.  The knobs (the cos / sin nudge, orc_set_perturb) change
records only while they are set.  The case families of tests/test_gpu_shade_steps.py are checked
here for what the oracle alone must show (both outcomes of a fuzzed metal, the three of a
dielectric, the doubles around st == 1.0, the edge keys), so a family cannot go vacuous unnoticed
where no GPU runs."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import shade_step_cases as ssc
from conftest import scene_path

SEED = 777
INVALID = -1
# scene -> camera preset, width
FRAMES = {"three": ("c1_three", 24), "cornell": ("cornell", 18)}


def primary_rays(orc, preset, width, spp, seed):
    """Camera::GetRay without a lens, in its operations: the y offset is the stream's first draw."""
    cam = orc.make_camera(orc.camera_preset(preset), width)
    basis = np.zeros(21)
    orc.lib().orc_camera_init(C.byref(cam), basis.ctypes.data_as(C.c_void_p))
    center, p00, du, dv = basis[0:3], basis[3:6], basis[6:9], basis[9:12]
    assert cam.defocus <= 0
    W, H = cam.width, cam.height
    rays = np.zeros((H * W, spp, 6))
    for pix in range(H * W):
        i, j = pix % W, pix // W
        for s in range(spp):
            oy, ox = orc.philox(seed, pix, s, 2) - 0.5
            ps = p00 + ((i + ox) * du) + ((j + oy) * dv)
            rays[pix, s, :3], rays[pix, s, 3:] = center, ps - center
    return rays, W, H


def cases_from_hits(orc, rays, hits, pixel, sample, depth, max_depth, thr, seed):
    c = orc.shade_cases(len(rays))
    c["hit"] = hits[:, 0] != 0
    c["p"], c["normal"], c["u"], c["v"] = hits[:, 2:5], hits[:, 5:8], hits[:, 8], hits[:, 9]
    c["front_face"], c["mat"] = hits[:, 10], hits[:, 11]
    c["o"], c["d"], c["thr"] = rays[:, :3], rays[:, 3:], thr
    c["seed"], c["pixel"], c["sample"], c["depth"], c["max_depth"] = seed, pixel, sample, depth, max_depth
    return c


@pytest.mark.parametrize("name", list(FRAMES))
def test_chained_steps_are_render_samples(orc, name):
    preset, width = FRAMES[name]
    spp = 3
    scene = orc.Scene(scene_path(name))
    rays, W, H = primary_rays(orc, preset, width, spp, SEED)
    L_ref, segs_ref = scene.render_samples(orc.camera_preset(preset), width, spp, 1, SEED)
    L_ref, segs_ref = L_ref.reshape(-1, 3), segs_ref.reshape(-1)
    flat = rays.reshape(-1, 6)
    pixel, sample = np.repeat(np.arange(W * H), spp), np.tile(np.arange(spp), W * H)
    c0 = cases_from_hits(orc, flat, scene.intersect(flat), pixel, sample, 0, 1, 1.0, SEED)
    r0 = orc.shade_steps(scene, c0)
    go = r0["cont"] == 1
    assert go.any() and (c0["hit"] == 1).any()
    assert (~go).any() or name == "cornell"  # (a closed box: every primary segment hits and scatters)
    child = np.concatenate([r0["o"][go], r0["d"][go]], 1)
    c1 = cases_from_hits(orc, child, scene.intersect(child), pixel[go], sample[go], r0["depth"][go], 1, r0["thr"][go], SEED)
    assert (c1["depth"] == 1).all()
    r1 = orc.shade_steps(scene, c1)
    assert (r1["cont"] == 0).all(), "a segment at the depth limit ends"
    L = r0["L"].copy()
    L[go] = r1["L"]
    assert np.array_equal(L.view(np.uint64), L_ref.view(np.uint64))
    assert np.array_equal(1 + go, segs_ref)
    assert len(np.unique(L, axis=0)) > len(L) // 8


def test_the_knobs_change_records_only_while_set(orc, tmp_path):
    scene = orc.Scene(ssc.write_scene(tmp_path, "table"))
    fams = {k: ssc.family(k) for k in ("sky", "lambertian", "dielectric")}
    base = {k: orc.shade_steps(scene, f["cases"]) for k, f in fams.items()}
    try:
        orc.set_cos_sin_nudge(1, -1)
        got = orc.shade_steps(scene, fams["lambertian"]["cases"])
        moved = ~ssc.same(got, base["lambertian"])
        assert moved.any() and not moved[base["lambertian"]["cont"] == 0].any()
        for k in ("cont", "depth", "next"):
            assert np.array_equal(got[k], base["lambertian"][k])
        assert ssc.same(orc.shade_steps(scene, fams["dielectric"]["cases"]), base["dielectric"]).all()
    finally:
        orc.set_cos_sin_nudge(0, 0)
    for perturb, fam in ((1, "lambertian"), (2, "sky"), (3, "dielectric")):
        old = orc.set_perturb(perturb)
        try:
            assert old == 0
            for k, f in fams.items():
                differ = ~ssc.same(orc.shade_steps(scene, f["cases"]), base[k])
                assert differ.any() == (k == fam), (perturb, k, int(differ.sum()))
        finally:
            orc.set_perturb(0)
    for k, f in fams.items():
        assert ssc.same(orc.shade_steps(scene, f["cases"]), base[k]).all()


def test_the_families_reach_their_branches(orc, tmp_path):
    scene = orc.Scene(ssc.write_scene(tmp_path, "table"))
    # metal: both outcomes of a fuzzed reflection
    f = ssc.family("metal")
    r = orc.shade_steps(scene, f["cases"])
    go = r["cont"][f["fuzzed"] & (f["cases"]["depth"] < 5)] == 1
    print("metal, fuzzed: continue", go.mean())
    assert 0.05 <= go.mean() <= 0.95
    assert (r["cont"][~f["fuzzed"]][f["cases"]["depth"][~f["fuzzed"]] < 5] == 1).all(), "a mirror never absorbs"
    # dielectric: reflect, refract and total internal reflection
    f = ssc.family("dielectric")
    what = ssc.dielectric_outcomes(f["cases"], orc.shade_steps(scene, f["cases"]))
    share = {k: float((what == k).mean()) for k in ("tir", "reflect", "refract")}
    print("dielectric:", share)
    assert min(share.values()) >= 0.05
    # Lambertian: the roulette's three ranges kill and keep, the edge keys exist, every texture kind is read
    f = ssc.family("lambertian")
    r = orc.shade_steps(scene, f["cases"])
    assert f["n_edge"] >= 6
    deep = f["cases"]["depth"] >= 5
    assert (r["cont"][deep] == 0).any() and (r["cont"][deep] == 1).any() and (r["cont"][~deep] == 1).mean() > 0.9
    thr_in = f["cases"]["thr"][:, 0]
    kept = deep & (r["cont"] == 1) & (f["cases"]["mat"] == ssc.LAMB_SOLID) & (f["cases"]["pixel"] >= 100000)
    for t, scale in ((0.05, 1 / 0.1), (3.0, 1 / 0.95)):  # the clamps: thr' = c / 0.1 and c / 0.95
        k = kept & (thr_in == t)
        assert k.any()
        assert np.allclose(r["thr"][k].max(1), t * 0.8 * scale, rtol=1e-6), t
    missing = f["cases"]["mat"] == ssc.LAMB_MISSING
    k = missing & (r["cont"] == 1) & ~deep
    assert np.allclose(r["thr"][k], (0.0, 1.0, 1.0), atol=1e-6)
    # emitter: radiance, a dead path and the sky all occur
    f = ssc.family("emitter")
    r = orc.shade_steps(scene, f["cases"])
    assert (r["cont"] == 0).all()
    lit = (r["L"] != 0).any(1)
    dim = f["cases"]["mat"] == ssc.LIGHT_DIM
    assert lit.any() and not lit[dim & ~ssc.sky_end(f["cases"])].any() and lit[dim & ssc.sky_end(f["cases"])].any()
    # scatter API: the near_zero fallback returns the normal as the direction
    c = ssc.scatter_fallback_cases()
    r = orc.shade_steps(scene, c, scatter=True)
    assert (r["cont"] == 1).all() and np.array_equal(r["d"], c["normal"])
    assert (r["depth"] == c["depth"] - 1).all()


def test_hook_is_exported_and_checks_its_arguments(rtx_mod):
    rtx = rtx_mod
    name = "rtx_internal_shade_steps"
    nm = subprocess.run(["nm", "-D", "--defined-only", rtx.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(rf"\bT {name}\b", nm)
    assert name not in rtx.EXPORTS
    assert rtx.SHADE_CASE_DTYPE == ssc.orc.SHADE_CASE and rtx.SHADE_RECORD_DTYPE == ssc.orc.SHADE_RECORD
    f = getattr(rtx.lib(), name)
    f.argtypes, f.restype = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, C.c_void_p], C.c_int
    dummy = C.cast(C.create_string_buffer(64), C.c_void_p)  # never dereferenced: the checks below come first
    cases, out = C.create_string_buffer(176), C.create_string_buffer(112)

    def invalid(rc, word):
        msg = rtx.lib().rtx_last_error().decode()
        assert rc == INVALID and word in msg, (rc, msg)

    invalid(f(None, cases, 1, 0, out), "scene is NULL")
    invalid(f(dummy, None, 1, 0, out), "NULL buffer")
    invalid(f(dummy, cases, 1, 0, None), "NULL buffer")
    for variant in (-1, 3, 7, 16):
        invalid(f(dummy, cases, 1, variant, out), "variant")
    for variant in rtx.SHADE_VARIANTS.values():
        assert f(dummy, cases, 0, variant, out) == 0
