"""Every query family on a 64-entry traversal stack.

The query entry points pick their kernel's <STACK, FAST> pair in one place (with_walk,
csrc/rtx_host.h), and the stock scenes only ever reach the 32-entry arms.  Here the occlusion, AO,
radiance, irradiance and direct-lighting queries run on the two scenes of test_fast_tree.py whose
walks need 64 entries, in each precision that does, and are held to identities the suite already
asserts on 32-entry scenes (test_gpu_ao.py, test_gpu_radiance.py, test_gpu_irradiance.py,
test_gpu_direct.py): every comparison is exact, so there is no tolerance.
"""
import ctypes as C

import numpy as np
import pytest

from test_fast_tree import LINES, look_at, scene_rays, scenes  # noqa: F401  (scenes: a fixture)
from test_gpu_irradiance import centre_rays
from test_gpu_radiance import in_order_sum, resolve

pytestmark = pytest.mark.gpu
SEED = 4242
SAMPLES, DEPTH = 16, 6
LIGHT = 3  # RTX_MAT_DIFFUSE_LIGHT
# scene -> (lookfrom, lookat, vfov) of test_renders_on_64_entry_stacks, AO radius (the line's
# spheres span 28 orders of magnitude: every scale's neighbours lie within the radius)
VIEWS = {
    "line64": ((-0.5, 0.02, 0.03), (1.0, 0.0, 0.0), 12.0, 1e30),
    "chain_left_62": ((-6.0, 1.5, 2.0), (40.0, 0.0, 0.0), 40.0, 4.0),
}
_cases = {}


def stack_of(info, precision):
    fast = precision == "fast" and info["fast_ok"]
    return info["stack_fast"] if fast else info["stack_parity"]


def cases64(rtx, scenes):
    """[(name, precision, device scene, camera, AO radius)] of the (scene, precision) pairs whose
    walk runs on a 64-entry stack, made once."""
    if not _cases:
        for name, (lookfrom, lookat, vfov, radius) in VIEWS.items():
            sc = scenes(name)[0]
            info, _ = rtx.fast_tree(sc)
            dev = None
            for precision in ("parity", "fast"):
                if stack_of(info, precision) == 64:
                    dev = dev or rtx.DeviceScene(sc)
                    _cases[(name, precision)] = (name, precision, dev, look_at(rtx, lookfrom, lookat, vfov), radius)
    return list(_cases.values())


def surfels(dev, cam, precision):
    """Points and normals of the frame's pixels that hit, and explicit ids."""
    hits = dev.intersect(centre_rays(cam), precision=precision)
    hit = hits["hit"] != 0
    assert 0 < hit.sum() < len(hit), "some pixels must hit, some miss"
    ids = ((np.flatnonzero(hit).astype(np.uint64) * 2654435761 + 12345) % (1 << 32)).astype(np.uint32)
    return hits["p"][hit].copy(), hits["normal"][hit].copy(), ids


class LitCopy:
    """The test's own copy of a scene description with primitive `light` given a DiffuseLight
    material (a new material on the scene's texture 0); the tree, and so the stacks, stay."""

    def __init__(self, rtx, sc, light):
        self.rtx, self.sc = rtx, sc  # (sc owns the nodes, textures and images)
        d = sc.desc()
        self.prims = (rtx.Prim * d.n_prims)()
        C.memmove(self.prims, d.prims, C.sizeof(self.prims))
        self.mats = (rtx.Material * (d.n_materials + 1))()
        C.memmove(self.mats, d.materials, d.n_materials * C.sizeof(rtx.Material))
        self.mats[d.n_materials].kind, self.mats[d.n_materials].texture = LIGHT, 0
        self.prims[light].material = d.n_materials

    def desc(self):
        d = self.sc.desc()
        d.prims, d.materials, d.n_materials = self.prims, self.mats, len(self.mats)
        return d


def test_both_precisions_reach_a_64_entry_stack(rtx_mod, gpu, scenes):
    got = {(name, precision) for name, precision, *_ in cases64(rtx_mod, scenes)}
    print(sorted(got))
    assert {p for _, p in got} == {"parity", "fast"}
    assert LINES["line64"][1] == 64  # the fast walk of line64 needs all 64 entries


def test_occluded_is_the_hit_flag(rtx_mod, gpu, scenes):
    for name, precision, dev, _, _ in cases64(rtx_mod, scenes):
        rays = scene_rays(scenes, name)
        q = 4000 // 6
        rays = np.concatenate([rays[:300], rays[-2 * (q // 2):-(q // 2)][:150]])  # mixed, and the forward corner rays
        hit = dev.intersect(rays, precision=precision)["hit"]
        occ = dev.occluded(rays, precision=precision)
        print(name, precision, "rays", len(rays), "hit", int((hit != 0).sum()))
        assert np.array_equal(occ != 0, hit != 0)
        assert 0 < (hit != 0).sum() < len(rays)


def test_ao_equals_its_rays_through_occluded(rtx_mod, gpu, scenes):
    rtx = rtx_mod
    for name, precision, dev, cam, radius in cases64(rtx, scenes):
        npix = cam.image_width * cam.image_height
        ao = dev.ao(cam, samples=SAMPLES, radius=radius, seed=77, precision=precision)
        rays = rtx.ao_rays(dev, cam, samples=SAMPLES, radius=radius, seed=77, precision=precision)
        assert ao.shape == (npix,) and rays.shape == (npix, SAMPLES, 6)
        occ = dev.occluded(rays.reshape(-1, 6), tmin=rtx.RTX_SEAM_TMIN, tmax=radius, precision=precision)
        want = 1.0 - occ.reshape(npix, SAMPLES).mean(1)
        print(name, precision, "occluded pixels", int((ao < 1.0).sum()), "of", npix)
        assert ao.tobytes() == want.tobytes(), int((ao != want).sum())
        assert (ao < 1.0).any() and (ao == 1.0).any(), "some pixels must be occluded, some open"


def test_radiance_equals_the_renderer(rtx_mod, gpu, scenes):
    rtx = rtx_mod
    for name, precision, dev, cam, _ in cases64(rtx, scenes):
        spp = 2
        R = rtx.camera_rays(dev, cam, spp, seed=SEED)
        ids = np.arange(cam.image_width * cam.image_height, dtype=np.uint32)
        L, S = np.zeros((len(ids), spp, 3)), np.zeros((len(ids), spp), np.uint64)
        for k in range(spp):
            L[:, k], S[:, k] = dev.radiance(R[:, k], 1, DEPTH, seed=SEED, ids=ids, first_sample=k, precision=precision,
                                            segments=True)
        got = resolve(in_order_sum(L), spp)
        rgb, _, st = dev.render(cam, spp, DEPTH, seed=SEED, adaptive=False, mode="wavefront", precision=precision)
        print(name, precision, "pixels that differ:", int((got != rgb).any(1).sum()), "segments", int(S.sum()))
        assert st["rays_total"] > st["rays_primary"] == len(ids) * spp, "paths bounce"
        assert np.array_equal(got, rgb)
        assert int(S.sum()) == st["rays_total"]


def test_irradiance_equals_its_rays_through_radiance(rtx_mod, gpu, scenes):
    rtx = rtx_mod
    bounced = False
    for name, precision, dev, cam, _ in cases64(rtx, scenes):
        P, N, ids = surfels(dev, cam, precision)
        n = len(P)
        rays = rtx.irradiance_rays(dev, P, N, SAMPLES, SEED, ids=ids, first_sample=3)
        L, S = np.zeros((n, SAMPLES, 3)), np.zeros((n, SAMPLES), np.uint64)
        for k in range(SAMPLES):
            L[:, k], S[:, k] = dev.radiance(rays[:, k], 1, DEPTH, seed=SEED, ids=ids, first_sample=3 + k,
                                            precision=precision, segments=True)
        want = resolve(in_order_sum(L), SAMPLES)
        got, segs = dev.irradiance(P, N, SAMPLES, DEPTH, seed=SEED, ids=ids, first_sample=3, precision=precision,
                                   segments=True)
        print(name, precision, "surfels", n, "that differ:", int((got != want).any(1).sum()), "segments", int(S.sum()))
        assert got.tobytes() == want.tobytes()
        assert np.array_equal(segs.astype(np.uint64), S.sum(1))
        bounced = bounced or bool((S > 1).any())
    assert bounced, "some paths bounce"


def test_direct_equals_its_samples(rtx_mod, gpu, scenes):
    rtx = rtx_mod
    for name, precision, dev, cam, _ in cases64(rtx, scenes):
        P, N, ids = surfels(dev, cam, precision)
        # the light: the sphere in front of the one most pixels see (its neighbour towards the camera)
        g = scenes(name)[0].arrays()["prims"]["g"]
        seen = np.abs(np.linalg.norm(P[:, None, :] - g[None, :, :3], axis=2) - np.abs(g[None, :, 3])).argmin(1)
        light = max(0, int(np.bincount(seen).argmax()) - 1)
        lit = rtx.DeviceScene(LitCopy(rtx, scenes(name)[0], light))
        assert lit.emitters()[0] == 1
        n = len(P)
        smp = rtx.direct_samples(lit, P, N, SAMPLES, SEED, ids=ids, first_sample=3)
        assert smp.shape == (n, SAMPLES, 9)
        seg, Cs = smp[:, :, :6], smp[:, :, 6:]
        occ = lit.occluded(seg.reshape(-1, 6), rtx.RTX_SEAM_TMIN, rtx.RTX_DIRECT_TMAX, precision=precision)
        V = 1.0 - occ.reshape(n, SAMPLES).astype(np.float64)
        want = resolve(in_order_sum(Cs * V[:, :, None]), SAMPLES)
        want_vis = (Cs.any(2) & (V == 1.0)).sum(1)
        got, vis = lit.direct(P, N, SAMPLES, seed=SEED, ids=ids, first_sample=3, precision=precision, visible=True)
        print(name, precision, "light", light, "surfels", n, "traced", int(Cs.any(2).sum()), "visible",
              int(want_vis.sum()), "max", got.max())
        assert got.tobytes() == want.tobytes()
        assert np.array_equal(vis.astype(np.int64), want_vis)
        assert got.max() > 0.0, "the emitter's light arrives somewhere"
