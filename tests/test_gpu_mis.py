"""Multiple importance sampling (rtx_radiance_mis*, rtx_render_mis*, csrc/rtx_nee.h).

The estimator is pinned from outside, as tests/test_gpu_nee.py pins the light-sampling one: the
degenerate cases equal the plain radiance query bit for bit; on the Cornell box every slot is
rebuilt in numpy from the path records of rtx_internal_mis_trace, the emitter samples of
rtx_internal_nee_samples and the public rtx_occluded and rtx_radiance; the weights are the power
heuristic's; the estimator agrees with the plain one in expectation, has less variance than the
light-sampling one next to a light and than the plain one far from it, and stays unbiased for a
light the emitter table does not hold; keys, chunk seams, tiles, live scenes, the device entry
points and the command line behave as the other query families do.

`resolve` is k_radiance_sum's last step: the in-order sum times 1 / (double)(float)spp."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG, scene_path

pytestmark = pytest.mark.gpu
SEED = 4242
PRECISIONS = ("parity", "fast")
LAMBERTIAN, METAL, DIELECTRIC, LIGHT = 0, 1, 2, 3
CAP = 8  # segments recorded per path by the trace hooks (>= the largest max_depth decomposed + 1)
FIRST, SAMPLES = 5, 3
LE = 15.0  # the emission of the Cornell box's light and of the near-light scene's
_cache = {}

# A lamp close to a surface: a 4 x 4 light 0.09 above a small Lambertian shelf, over a floor.
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


def resolve(total, n):
    return total * (1.0 / float(np.float64(np.float32(n))))


def scene(rtx, name):
    if name not in _cache:
        host = rtx.HostScene.load(scene_path(name))
        _cache[name] = (rtx.DeviceScene(host), host)
    return _cache[name]


def near_light_scene(rtx, tmp_path):
    path = tmp_path / "near_light.rtxs"
    path.write_text(NEAR_LIGHT)
    dev = rtx.DeviceScene(rtx.HostScene.load(str(path)))
    assert dev.emitters() == (1, 16.0)
    return dev


def cornell_rays(rtx):
    """(rays (n, 6), ids (n,), cam): the ray set of tests/test_gpu_nee.py, rebuilt here: sample 0's
    camera rays of the 36-wide Cornell preset with their global pixel ids, then rays from the middle
    of the box at the light, at the three spheres (Lambertian, metal, glass), at the floor and a
    wall, and out of the open front, and one onto the metal sphere that reflects into the light,
    with ids of their own.  Made once and left unchanged."""
    if "rays" not in _cache:
        dev, _ = scene(rtx, "cornell")
        cam = rtx.camera(rtx.camera_config("cornell", width=36))
        R = rtx.camera_rays(dev, cam, 1, seed=SEED)[:, 0]
        o = np.array([5.0, 5.0, 5.0])
        targets = [[5, 9.99, 5], [4, 9.99, 6], [3.2, 1, 7], [7, 1, 4], [5, 1, 2.5], [7.2, 1.3, 4.1], [5.1, 1.2, 2.4],
                   [5, 0, 5], [0, 5, 5], [10, 4, 6], [5, 5, -3], [2, 7, -3], [8, 2, -1]]
        aimed = np.array([np.concatenate([o, np.array(t, dtype=np.float64) - o]) for t in targets])
        aimed = np.concatenate([aimed, [[6.9, 9.0, 4.0, 0.0, -1.0, 0.0]]])
        rays = np.ascontiguousarray(np.concatenate([R, aimed]))
        ids = np.concatenate([np.arange(len(R)), 100000 + 17 * np.arange(len(aimed))]).astype(np.uint32)
        rays.setflags(write=False), ids.setflags(write=False)
        _cache["rays"] = (rays, ids, cam)
    return _cache["rays"]


def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def ratio(x, nx, y, ny, area):
    """g = p_bsdf / p_light = cos_x cos_y A / (pi |y - x|^2) of the pairs (x, y), in numpy."""
    seg = y - x
    d2 = (seg * seg).sum(-1)
    w = seg / np.sqrt(d2)[..., None]
    cx = np.maximum(0.0, (unit(nx) * w).sum(-1))
    cy = np.abs((ny * w).sum(-1))
    return cx * cy * area / (np.pi * d2)


def decompose(rtx, dev, rays, ids, max_depth, precision, sample, area, light_normal=(0.0, -1.0, 0.0)):
    """Sample `sample` of every ray, taken apart: the records of mis_trace, every eligible vertex's
    term rebuilt in numpy as w * (C V) * (1.0 / (1.0 + g * g)) with C from nee_samples() and V from
    the public occluded(), the slot as the in-order sum plus L_end, and the plain query of the same
    keys.  light_normal: the (flat) emitters' normal, for the recomputation of g."""
    kw = dict(ids=ids, first_sample=sample, precision=precision)
    T = rtx.mis_trace(dev, rays, 1, max_depth, SEED, CAP, **kw)
    out = {k: v[:, 0] for k, v in T.items()}
    n = len(rays)
    flags, P, N, Wt, G = out["flags"], out["p"], out["n"], out["w"], out["g"]
    elig, traced, vis = (flags & rtx.NEE_ELIGIBLE) != 0, (flags & rtx.NEE_TRACED) != 0, (flags & rtx.NEE_VISIBLE) != 0
    total = np.zeros((n, 3))
    terms = np.zeros((n, CAP, 3))
    want_shadow = np.zeros(n, np.int64)
    g_err = 0.0
    for d in range(CAP):
        rows = np.flatnonzero(elig[:, d])
        if not len(rows):
            continue
        assert d + 1 < max_depth
        smp = rtx.nee_samples(dev, P[rows, d], N[rows, d], 1, SEED, d, ids=ids[rows], first_sample=sample)[:, 0]
        seg, C = smp[:, :6], smp[:, 6:]
        tr = C.any(1)
        assert np.array_equal(tr, traced[rows, d]), d
        occ = dev.occluded(seg[tr], rtx.RTX_SEAM_TMIN, rtx.RTX_DIRECT_TMAX, precision=precision) if tr.any() else []
        V = np.zeros(len(rows))
        V[tr] = 1.0 - np.asarray(occ, dtype=np.float64)
        assert np.array_equal(V == 1.0, vis[rows, d]), d
        g = G[rows, d]
        # the recorded g: zero where nothing was traceable; C = g Le bit for bit; and the ratio of
        # the two densities recomputed from the recorded point and normal and the sample's segment
        assert not g[~tr].any() and (g[tr] > 0).all()
        assert (g[:, None] * np.full(3, LE)).tobytes() == C.tobytes()
        if tr.any():
            x, y = seg[tr, :3], seg[tr, :3] + seg[tr, 3:]
            assert x.tobytes() == P[rows, d][tr].tobytes()
            want_g = ratio(x, N[rows, d][tr], y, np.array(light_normal), area)
            g_err = max(g_err, float(np.max(np.abs(g[tr] - want_g) / want_g)))
        term = Wt[rows, d] * (C * V[:, None]) * (1.0 / (1.0 + g * g))[:, None]
        terms[rows, d] = term
        total[rows] = total[rows] + term
        want_shadow[rows] += tr
    out.update(elig=elig, traced=traced, vis=vis, weighted=(flags & rtx.MIS_WEIGHTED) != 0, terms=terms,
               slot=total + out["L_end"], want_shadow=want_shadow, g_err=g_err)
    out["plain"], out["plain_segs"] = dev.radiance(rays, 1, max_depth, seed=SEED, segments=True, **kw)
    return out


# ---- degenerate equalities -------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
def test_without_emitters_it_is_the_radiance_query(rtx_mod, gpu, precision):
    rtx = rtx_mod
    dev, _ = scene(rtx, "three")
    assert dev.emitters() == (0, 0.0)
    cam = rtx.camera(rtx.camera_config("c1_three", width=32))
    R = rtx.camera_rays(dev, cam, 3, seed=SEED)
    ids = np.arange(len(R), dtype=np.uint32)
    kw = dict(seed=SEED, ids=ids, first_sample=0, precision=precision, segments=True)
    for k in range(3):
        kw["first_sample"] = k
        a, sa = dev.radiance_mis(R[:, k], 1, 10, **kw)
        b, sb = dev.radiance(R[:, k], 1, 10, **kw)
        assert a.tobytes() == b.tobytes() and np.array_equal(sa, sb)
        assert sb.max() > 1 and len(np.unique(b, axis=0)) > len(b) // 8
    # the frame: a 16 x 9 tile of it equals the fixed-spp wavefront render's
    tile = (7, 4, 16, 9)
    rgb, segs = dev.render_mis(cam, 3, 10, seed=SEED, precision=precision, tile=tile)
    want, _, st = dev.render(cam, 3, 10, seed=SEED, adaptive=False, mode="wavefront", precision=precision, tile=tile)
    assert rgb.shape == (16 * 9, 3) and rgb.tobytes() == want.tobytes()
    assert int(segs.sum(dtype=np.uint64)) == st["rays_total"] > st["rays_primary"] == 16 * 9 * 3


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("max_depth", [0, 1])
def test_no_term_fits_below_depth_two(rtx_mod, gpu, max_depth, precision):
    dev, _ = scene(rtx_mod, "cornell")
    rays, ids, _ = cornell_rays(rtx_mod)
    kw = dict(seed=SEED, ids=ids, first_sample=FIRST, precision=precision, segments=True)
    a, sa = dev.radiance_mis(rays, 2, max_depth, **kw)
    b, sb = dev.radiance(rays, 2, max_depth, **kw)
    assert a.tobytes() == b.tobytes() and np.array_equal(sa, sb)
    assert (sb == 2).all() if max_depth == 0 else (sb.min() >= 2 and sb.max() == 4)
    assert len(np.unique(b, axis=0)) > 8


# ---- the decomposition -----------------------------------------------------------------------

def sphere_of(host, kind):
    """Centre and radius of the Cornell box's sphere whose material is of `kind`."""
    arr = host.arrays()
    for p in arr["prims"]:
        if p["kind"] == 0 and arr["materials"][p["material"]]["kind"] == kind:
            return p["g"][:3].copy(), float(p["g"][3])
    raise AssertionError(kind)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("max_depth", [2, 6])
def test_every_slot_is_its_weighted_terms_plus_its_end(rtx_mod, gpu, max_depth, precision):
    rtx = rtx_mod
    dev, host = scene(rtx, "cornell")
    rays, ids, _ = cornell_rays(rtx)
    n = len(rays)
    count, area = dev.emitters()
    assert (count, area) == (1, 16.0)
    slots, nseg = [], np.zeros(n, np.int64)
    seen = dict(elig=0, traced=0, vis=0, weighted=0, kept=0, deep=0, g_err=0.0, gb_err=0.0)
    for k in range(SAMPLES):
        sample = FIRST + k
        D = decompose(rtx, dev, rays, ids, max_depth, precision, sample, area)
        kw = dict(ids=ids, first_sample=sample, precision=precision)
        flags, P, N, Wt, GB = D["flags"], D["p"], D["n"], D["w"], D["gb"]
        elig, traced, vis, weighted = D["elig"], D["traced"], D["vis"], D["weighted"]
        L_end, closest, shadow, plain = D["L_end"], D["closest"], D["shadow"], D["plain"]
        assert closest.max() <= max_depth + 1 <= CAP
        # the path is the light-sampling estimator's: vertices, w, flags except suppression, and
        # both segment counts equal nee_trace's for the same key
        E = rtx.nee_trace(dev, rays, 1, max_depth, SEED, CAP, **kw)
        for name in ("p", "n", "w"):
            assert D[name].tobytes() == E[name][:, 0].tobytes(), name
        e_flags = E["flags"][:, 0]
        supp = (e_flags & rtx.NEE_SUPPRESSED) != 0
        assert not (flags & rtx.NEE_SUPPRESSED).any()
        assert np.array_equal(flags & 7, e_flags & 7)
        assert np.array_equal(closest, E["closest"][:, 0]) and np.array_equal(shadow, E["shadow"][:, 0])
        # (in this scene every light is in the table: what that estimator suppresses is weighted here)
        assert np.array_equal(weighted, supp)
        # flags nest, and records past a path's end are empty
        assert not (traced & ~elig).any() and not (vis & ~traced).any()
        reach = np.arange(CAP)[None, :] < closest[:, None]
        assert not flags[~reach].any() and not Wt[~elig].any() and not D["g"][~traced].any() and not GB[~weighted].any()
        # the slot: the weighted terms in depth order plus the path's end
        got, segs = dev.radiance_mis(rays, 1, max_depth, seed=SEED, segments=True, **kw)
        print(precision, "depth", max_depth, "sample", sample, "eligible", int(elig.sum()), "traced",
              int(traced.sum()), "visible", int(vis.sum()), "weighted", int(weighted.sum()), "differ",
              int((got != resolve(D["slot"], 1)).any(1).sum()), "g rel err", D["g_err"])
        assert got.tobytes() == resolve(D["slot"], 1).tobytes()
        assert np.array_equal(closest, D["plain_segs"])
        assert np.array_equal(shadow.astype(np.int64), D["want_shadow"])
        assert np.array_equal(segs.astype(np.int64), closest.astype(np.int64) + D["want_shadow"])
        assert D["g_err"] <= 1e-12
        # the end: a weighted segment's L_end is wb times the plain emission, wb from the recorded
        # gb in the documented order; every other end is the plain query's
        ended = weighted.any(1)
        assert L_end[~ended].tobytes() == plain[~ended].tobytes()
        rows, ds = np.nonzero(weighted)
        assert len(np.unique(rows)) == len(rows)
        gb = GB[rows, ds]
        wb = 1.0 - 1.0 / (1.0 + gb * gb)
        assert L_end[rows].tobytes() == (wb[:, None] * plain[rows]).tobytes()
        assert plain[rows].any(1).all() and (wb >= 0).all() and (wb <= 1).all()
        # gb again from the recorded vertices: the parent's point and normal, the hit's, the area
        for i, d in zip(rows, ds):
            assert d == closest[i] - 1 and 1 <= d < max_depth and elig[i, d - 1]
        if len(rows):
            want_gb = ratio(P[rows, ds - 1], N[rows, ds - 1], P[rows, ds], N[rows, ds], area)
            gb_err = float(np.max(np.abs(gb - want_gb) / want_gb))
            assert gb_err <= 1e-12, gb_err
            seen["gb_err"] = max(seen["gb_err"], gb_err)
        # gb is absent at segment 0, after metal or glass parents, and at the depth limit: a path
        # that ends on the light is weighted exactly when a term was eligible at its parent vertex
        last = closest.astype(np.int64) - 1
        every = np.arange(n)
        Pl = P[every, np.minimum(last, CAP - 1)]
        on_light = ((np.abs(Pl[:, 1] - 9.99) < 1e-9) & (Pl[:, 0] >= 3) & (Pl[:, 0] <= 7) & (Pl[:, 2] >= 3)
                    & (Pl[:, 2] <= 7) & (last < max_depth))
        parent_elig = np.where(last >= 1, elig[every, np.maximum(last - 1, 0)], False)
        assert np.array_equal(ended, on_light & parent_elig)
        assert not GB[:, 0].any() and not GB[:, max_depth:].any()
        kept = on_light & ~parent_elig
        assert L_end[kept].tobytes() == plain[kept].tobytes() and L_end[kept].any(1).all()
        for kind in (METAL, DIELECTRIC):
            c, r = sphere_of(host, kind)
            on = (np.abs(np.linalg.norm(P - c, axis=2) - r) < 1e-6) & reach
            assert on.any() and not elig[on].any(), kind
            after = np.zeros_like(on)
            after[:, 1:] = on[:, :-1]
            assert not GB[after].any() and not weighted[after].any(), kind
        assert not elig[:, max_depth - 1:].any()
        # emission straight from the camera (segment 0) and after a specular parent is unweighted
        assert (L_end[n - 14] == LE).all() and closest[n - 14] == 1
        assert kept[n - 1] and last[n - 1] == 1 and L_end[n - 1].all()  # camera -> metal -> light
        slots.append(D["slot"])
        nseg += closest.astype(np.int64) + D["want_shadow"]
        seen["elig"] += int(elig.sum()); seen["traced"] += int(traced.sum()); seen["vis"] += int(vis.sum())
        seen["weighted"] += int(weighted.sum()); seen["kept"] += int((kept & (last >= 1)).sum())
        seen["deep"] += int(elig[:, 1:].sum())
        seen["g_err"] = max(seen["g_err"], D["g_err"])
        if max_depth == 6 and k == 0:
            _cache[("decomposed", precision)] = D
    # the three samples of a ray in one call: the in-order sum, resolved
    got, segs = dev.radiance_mis(rays, SAMPLES, max_depth, seed=SEED, ids=ids, first_sample=FIRST, precision=precision,
                                 segments=True)
    assert got.tobytes() == resolve(slots[0] + slots[1] + slots[2], SAMPLES).tobytes()
    assert np.array_equal(segs.astype(np.int64), nseg)
    # not vacuous
    print(seen)
    assert seen["elig"] > n and 0 < seen["vis"] <= seen["traced"] <= seen["elig"] and seen["kept"] > 0
    if max_depth > 2:
        assert seen["weighted"] > 0 and seen["deep"] > 0 and seen["vis"] < seen["traced"] < seen["elig"]


# ---- the weights ----------------------------------------------------------------------------

def test_weights_are_the_power_heuristic(rtx_mod, gpu, tmp_path):
    """Every eligible vertex's term is at most half of w Le per channel (g / (1 + g^2) <= 1 / 2),
    on the Cornell box and, where g reaches the hundreds, next to a light."""
    rtx = rtx_mod
    dev, _ = scene(rtx, "cornell")
    rays, ids, _ = cornell_rays(rtx)
    cases = []
    for precision in PRECISIONS:
        D = _cache.get(("decomposed", precision)) or decompose(rtx, dev, rays, ids, 6, precision, FIRST, 16.0)
        cases.append(("cornell " + precision, D))
    near = near_light_scene(rtx, tmp_path)
    N = 512
    down = np.tile([5.0, 9.95, 5.0, 0.0, -1.0, 0.0], (N, 1))
    cases.append(("near light", decompose(rtx, near, down, np.arange(N, dtype=np.uint32), 2, "parity", 0, 16.0)))
    for name, D in cases:
        elig, Wt = D["elig"], D["w"]
        assert elig.sum() > 100 and (Wt[elig] > 0).all()
        share = D["terms"][elig] / (Wt[elig] * LE)
        g = D["g"][elig]
        print(name, "eligible", int(elig.sum()), "largest g", g.max(), "largest term / (w Le)", share.max())
        assert (share >= 0.0).all() and (share <= 0.5).all()
    # next to the light g spans both sides of 1, where the weight peaks, and reaches the hundreds:
    # the light-sampling estimator's fireflies (C = g Le)
    assert share.max() > 0.25 and g.max() > 100.0 and g[g > 0].min() < 0.01


# ---- expectation and variance ---------------------------------------------------------------

def stats(a):
    return a.mean(0), a.var(0, ddof=1)


def test_near_a_light(rtx_mod, gpu, tmp_path):
    """A Lambertian shelf 0.09 below the centre of a 4 x 4 light, seen from straight above: 4096
    single-sample paths at max_depth 2.  Per channel the MIS and the plain means differ by at most
    5 standard errors of their difference (the project's margin; the seed is fixed,
    so the outcome is deterministic); the MIS sample variance is below the light-sampling
    estimator's on the same keys; and no MIS sample exceeds rho Le (1/2 + 1): at most half of
    w Le from the light side and all of thr Le from the BSDF side, with w = rho and thr = rho up to
    the f32 rounding of the cosine and the density in the throughput (2^-23 relative)."""
    rtx = rtx_mod
    dev = near_light_scene(rtx, tmp_path)
    N = 4096
    ids = np.arange(N, dtype=np.uint32) + 7
    rays = np.tile([5.0, 9.95, 5.0, 0.0, -1.0, 0.0], (N, 1))
    hit = dev.intersect(rays[:1])
    assert hit["hit"][0] and abs(hit["p"][0][1] - 9.9) < 1e-12
    a = dev.radiance_mis(rays, 1, 2, seed=SEED, ids=ids)
    b = dev.radiance(rays, 1, 2, seed=SEED, ids=ids)
    c = dev.radiance_nee(rays, 1, 2, seed=SEED, ids=ids)
    (ma, va), (mb, vb), (mc, vc) = stats(a), stats(b), stats(c)
    bound = 5.0 * np.sqrt(va / N + vb / N)
    print("mis", ma, va, "max", a.max(), "plain", mb, vb, "max", b.max(), "nee", mc, vc, "max", c.max(),
          "|mis - plain|", np.abs(ma - mb), "bound", bound, "var nee / var mis", vc / va)
    assert (np.abs(ma - mb) <= bound).all()
    assert (va < vc).all()
    assert (ma > 0).all() and (mb > 0).all()
    assert a.max() <= 1.5 * 0.73 * LE * (1.0 + 2.0 ** -22)


def test_far_from_the_light(rtx_mod, gpu):
    """Cornell, the open floor point (5, 0, 5) and the wall point (0, 5, 5) from the middle of the
    box, 4096 single-sample paths at max_depth 8: the MIS mean is within 5 standard errors of the
    plain one per channel, and the MIS sample variance is below the plain one's."""
    dev, _ = scene(rtx_mod, "cornell")
    N = 4096
    ids = np.arange(N, dtype=np.uint32) + 7
    for target in ([5.0, 0.0, 5.0], [0.0, 5.0, 5.0]):
        o = np.array([5.0, 5.0, 5.0])
        rays = np.tile(np.concatenate([o, np.array(target) - o]), (N, 1))
        a = dev.radiance_mis(rays, 1, 8, seed=SEED, ids=ids)
        b = dev.radiance(rays, 1, 8, seed=SEED, ids=ids)
        (ma, va), (mb, vb) = stats(a), stats(b)
        bound = 5.0 * np.sqrt(va / N + vb / N)
        print(target, "mis", ma, va, "plain", mb, vb, "|diff|", np.abs(ma - mb), "bound", bound, "var ratio", vb / va)
        assert (np.abs(ma - mb) <= bound).all()
        assert (va < vb).all()
        assert (ma > 0).all() and (mb > 0).all()


def test_a_light_the_table_does_not_know(rtx_mod, gpu):
    """update_prims gives the Cornell box's back wall the light's material: the emitter table keeps
    its one entry, so the light sampler never chooses the wall.  MIS gives its hits BSDF weight 1
    and agrees with the plain estimator; the light-sampling estimator suppresses them and renders
    darker (measured and printed; asserted only when it lies more than 5 standard errors below)."""
    rtx = rtx_mod
    host = rtx.HostScene.load(scene_path("cornell"))
    dev = rtx.DeviceScene(host)
    arr = host.arrays()
    prims = arr["prims"]
    light = int(rtx.emitter_table(dev)[0][0])
    wall = [i for i, p in enumerate(prims)
            if p["kind"] == 2 and p["g"][4] == 10.0 and arr["materials"][p["material"]]["kind"] == LAMBERTIAN]
    assert len(wall) == 1
    lit = prims[wall[0]:wall[0] + 1].copy()
    lit[0]["material"] = prims[light]["material"]
    dev.update_prims(lit, first=wall[0])
    assert dev.emitters() == (1, 16.0)
    N = 4096
    ids = np.arange(N, dtype=np.uint32) + 7
    rays = np.tile([5.0, 5.0, 5.0, 0.0, -5.0, 0.0], (N, 1))
    a = dev.radiance_mis(rays, 1, 3, seed=SEED, ids=ids)
    b = dev.radiance(rays, 1, 3, seed=SEED, ids=ids)
    c = dev.radiance_nee(rays, 1, 3, seed=SEED, ids=ids)
    (ma, va), (mb, vb), (mc, vc) = stats(a), stats(b), stats(c)
    bound = 5.0 * np.sqrt(va / N + vb / N)
    below = 5.0 * np.sqrt(va / N + vc / N)
    print("mis", ma, va, "plain", mb, vb, "|mis - plain|", np.abs(ma - mb), "bound", bound)
    print("nee", mc, vc, "mis - nee", ma - mc, "5 sigma", below)
    assert (np.abs(ma - mb) <= bound).all()
    assert (ma > 0).all() and (mb > 0).all()
    if (ma - mc > below).all():
        assert (mc < ma).all()
    # the records: the wall's hits after a diffuse vertex keep the plain emission (wb = 1)
    M = 1024  # (M x CAP records stay below the hook's limit)
    T = rtx.mis_trace(dev, rays[:M], 1, 3, SEED, CAP, ids=ids[:M])
    closest, flags, P = T["closest"][:, 0], T["flags"][:, 0], T["p"][:, 0]
    last = closest.astype(np.int64) - 1
    rows = np.arange(M)
    Pl = P[rows, last]
    elig = (flags & rtx.NEE_ELIGIBLE) != 0
    on_wall = (np.abs(Pl[:, 2] - 10.0) < 1e-9) & (last >= 1) & (last < 3) & elig[rows, np.maximum(last - 1, 0)]
    print("paths that end on the wall light after a diffuse vertex:", int(on_wall.sum()), "of", M)
    assert on_wall.sum() > 50
    assert not (flags[on_wall] & rtx.MIS_WEIGHTED).any() and not T["gb"][:, 0][on_wall].any()
    assert T["L_end"][:, 0][on_wall].tobytes() == b[:M][on_wall].tobytes() and b[:M][on_wall].all()
    # ... while the table's own light is still weighted
    weighted = ((flags & rtx.MIS_WEIGHTED) != 0).any(1)
    assert weighted.any() and (np.abs(Pl[weighted][:, 1] - 9.99) < 1e-9).all()


# ---- keys and seams -------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
def test_chunking_and_order_change_nothing(rtx_mod, gpu, precision):
    rtx = rtx_mod
    dev, _ = scene(rtx, "cornell")
    rays, ids, cam = cornell_rays(rtx)
    pick = np.linspace(0, len(rays) - 1, 200).astype(np.int64)
    r, pid = rays[pick], ids[pick]
    kw = dict(seed=SEED, first_sample=2, precision=precision, segments=True)
    runs = {}
    try:
        for chunk in (64, 7, 3, 0):  # whole rays per chunk; one ray per chunk; a ray's samples split; default
            rtx.radiance_chunk(chunk)
            runs[chunk] = dev.radiance_mis(r, 5, 6, ids=pid, **kw) + dev.render_mis(cam, 5, 6, seed=SEED,
                                                                                  precision=precision, tile=(3, 2, 9, 4))
    finally:
        rtx.radiance_chunk(0)
    ref = runs[0]
    assert len(np.unique(ref[0], axis=0)) > 50 and ref[1].max() > 10
    for chunk in (64, 7, 3):
        for a, b in zip(runs[chunk], ref):
            assert a.tobytes() == b.tobytes(), chunk
    # batch order: a permutation of the rays with their ids permutes the results
    perm = np.random.default_rng(3).permutation(len(r))
    a, sa = dev.radiance_mis(r[perm], 5, 6, ids=pid[perm], **kw)
    assert a.tobytes() == ref[0][perm].tobytes() and np.array_equal(sa, ref[1][perm])
    # ... and the key is the id, not the position: without ids the ray's index keys it
    b = dev.radiance_mis(r, 5, 6, ids=np.arange(len(r), dtype=np.uint32), **kw)
    c = dev.radiance_mis(r, 5, 6, **kw)
    assert b[0].tobytes() == c[0].tobytes() and b[0].tobytes() != ref[0].tobytes()
    # it is a third estimator: other values than the light-sampling one's, the same segments
    e = dev.radiance_nee(r, 5, 6, ids=pid, **kw)
    assert e[0].tobytes() != ref[0].tobytes() and np.array_equal(e[1], ref[1])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_frame_is_the_query_on_the_camera_rays(rtx_mod, gpu, precision):
    rtx = rtx_mod
    dev, _ = scene(rtx, "cornell")
    cam = rtx.camera(rtx.camera_config("cornell", width=36))
    W, H, spp, depth = cam.image_width, cam.image_height, 3, 6
    rgb, segs = dev.render_mis(cam, spp, depth, seed=SEED, precision=precision)
    assert rgb.shape == (W * H, 3) and segs.shape == (W * H,)
    R = rtx.camera_rays(dev, cam, spp, seed=SEED)
    ids = np.arange(W * H, dtype=np.uint32)
    total, nseg = np.zeros((W * H, 3)), np.zeros(W * H, np.int64)
    for k in range(spp):
        L, s = dev.radiance_mis(R[:, k], 1, depth, seed=SEED, ids=ids, first_sample=k, precision=precision,
                                segments=True)
        total, nseg = total + L, nseg + s
    assert rgb.tobytes() == resolve(total, spp).tobytes() and np.array_equal(segs.astype(np.int64), nseg)
    # another image than the light-sampling frame's, with the same segments
    nee, nee_segs = dev.render_nee(cam, spp, depth, seed=SEED, precision=precision)
    assert rgb.tobytes() != nee.tobytes() and np.array_equal(segs, nee_segs)
    assert np.isfinite(rgb).all() and rgb.min() >= 0.0
    # a tile and stripes of the frame are the whole frame's pixels
    x0, y0, w, h = 5, 3, 17, 7
    t_rgb, t_segs = dev.render_mis(cam, spp, depth, seed=SEED, precision=precision, tile=(x0, y0, w, h))
    sel = (np.arange(y0, y0 + h)[:, None] * W + np.arange(x0, x0 + w)[None, :]).ravel()
    assert t_rgb.tobytes() == rgb[sel].tobytes() and np.array_equal(t_segs, segs[sel])
    s_rgb, s_segs = dev.render_mis(cam, spp, depth, seed=SEED, precision=precision, stripes=(2, 1, 3))
    rows = [y for y in range(H) if (y // 2) % 3 == 1]
    sel = (np.array(rows)[:, None] * W + np.arange(W)[None, :]).ravel()
    assert s_rgb.tobytes() == rgb[sel].tobytes() and np.array_equal(s_segs, segs[sel])


def test_live_scene(rtx_mod, gpu, tmp_path):
    """The Cornell box's light is moved in place and compared with a scene made from the new file."""
    rtx = rtx_mod
    rays, ids, cam = cornell_rays(rtx)
    text = open(scene_path("cornell")).read()
    old = "rect xz 3 7 3 7 9.9900000000000002 3\n"
    assert old in text
    path = tmp_path / "cornell_moved.rtxs"
    path.write_text(text.replace(old, "rect xz 1 7 2 8 9.5 3\n"))
    fresh = rtx.DeviceScene(rtx.HostScene.load(str(path)))
    host = rtx.HostScene.load(scene_path("cornell"))
    dev = rtx.DeviceScene(host)
    prims = host.arrays()["prims"]
    li = int(rtx.emitter_table(dev)[0][0])
    kw = dict(seed=SEED, ids=ids, first_sample=1, segments=True)
    before = dev.radiance_mis(rays, 2, 6, **kw)
    moved = prims[li:li + 1].copy()
    moved[0]["g"][:5] = [1.0, 7.0, 2.0, 8.0, 9.5]
    dev.update_prims(moved, first=li)
    assert dev.emitters() == (1, 36.0)
    for precision in PRECISIONS:
        after = dev.radiance_mis(rays, 2, 6, precision=precision, **kw)
        want = fresh.radiance_mis(rays, 2, 6, precision=precision, **kw)
        assert after[0].tobytes() == want[0].tobytes() and np.array_equal(after[1], want[1])
        assert after[0].tobytes() != before[0].tobytes()
        f_after = dev.render_mis(cam, 2, 6, seed=SEED, precision=precision, tile=(8, 5, 16, 9))
        f_want = fresh.render_mis(cam, 2, 6, seed=SEED, precision=precision, tile=(8, 5, 16, 9))
        assert f_after[0].tobytes() == f_want[0].tobytes() and np.array_equal(f_after[1], f_want[1])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_device_entries_on_a_stream(rtx_mod, gpu, precision):
    import torch

    rtx = rtx_mod
    dev, _ = scene(rtx, "cornell")
    rays, ids, cam = cornell_rays(rtx)
    n = len(rays)
    want, want_segs = dev.radiance_mis(rays, 3, 6, seed=SEED, ids=ids, first_sample=1, precision=precision,
                                       segments=True)
    d_rays = torch.from_numpy(rays.copy()).cuda()
    d_ids = torch.from_numpy(ids.copy().view(np.int32)).cuda()
    d_out = torch.full((n + 8, 3), -7.0, dtype=torch.float64, device="cuda")
    d_segs = torch.full((n + 8,), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for stream in (None, torch.cuda.Stream()):
        d_out.fill_(-7.0)
        d_segs.fill_(77)
        torch.cuda.synchronize()
        dev.radiance_mis_device(d_rays.data_ptr(), n, d_out.data_ptr(), 3, 6, seed=SEED, first_sample=1,
                                precision=precision, d_ids=d_ids.data_ptr(), d_segments=d_segs.data_ptr(),
                                stream=stream.cuda_stream if stream else 0)
        if stream:
            stream.synchronize()
        else:
            dev.emitters()  # waits for the scene's stream
            torch.cuda.synchronize()
        out, segs = d_out.cpu().numpy(), d_segs.cpu().numpy().view(np.uint32)
        assert out[:n].tobytes() == want.tobytes() and np.array_equal(segs[:n], want_segs)
        assert (out[n:] == -7.0).all() and (segs[n:] == 77).all()
    # n == 0 writes nothing
    stream = torch.cuda.Stream()
    d_out.fill_(-7.0)
    torch.cuda.synchronize()
    dev.radiance_mis_device(d_rays.data_ptr(), 0, d_out.data_ptr(), 3, 6, seed=SEED, stream=stream.cuda_stream)
    stream.synchronize()
    assert (d_out.cpu().numpy() == -7.0).all()
    # the frame
    tile = (4, 3, 20, 10)
    f_want, f_segs = dev.render_mis(cam, 3, 6, seed=SEED, precision=precision, tile=tile)
    m = len(f_want)
    d_rgb = torch.full((m + 8, 3), -7.0, dtype=torch.float64, device="cuda")
    d_fs = torch.full((m + 8,), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    got = dev.render_mis_device(cam, d_rgb.data_ptr(), 3, 6, seed=SEED, precision=precision, tile=tile,
                                d_segments=d_fs.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    out, segs = d_rgb.cpu().numpy(), d_fs.cpu().numpy().view(np.uint32)
    assert got == m == 200
    assert out[:m].tobytes() == f_want.tobytes() and np.array_equal(segs[:m], f_segs)
    assert (out[m:] == -7.0).all() and (segs[m:] == 77).all()


def test_command_line_mis_frame(rtx_mod, gpu, tmp_path):
    rtx = rtx_mod
    exe = os.path.join(PKG, "raytracer")
    cams = json.load(open(os.path.join(os.path.dirname(PKG), "configs", "cameras.json")))
    small = dict(cams["cornell"], imageWidth=30, samplesPerPixel=3, maxDepth=6)
    path = tmp_path / "cameras.json"
    path.write_text(json.dumps({"default": cams["default"], "small": small}))
    base = [exe, "small", "--scene", scene_path("cornell"), "--cameras", str(path), "--seed", str(SEED)]
    r = subprocess.run(base + ["--mis"], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    dev, _ = scene(rtx, "cornell")
    cam = rtx.camera(rtx.camera_config("small", cameras=str(path)))
    assert (cam.image_width, cam.image_height) == (30, 20)
    rgb, segs = dev.render_mis(cam, 3, 6, seed=SEED)
    assert r.stdout == rtx.encode_p3(dev, rgb, 30, 20)
    tok = r.stdout.split()
    assert tok[:4] == [b"P3", b"30", b"20", b"255"] and len(tok) == 4 + 3 * 600
    line = "mis: 3 spp, 1 emitters, %d segments\n" % int(segs.sum(dtype=np.uint64))
    assert line.encode() in r.stderr, r.stderr.decode()
    assert b"nee:" not in r.stderr
    # --spp overrides the preset's samples
    r2 = subprocess.run(base + ["--mis", "--spp", "2"], capture_output=True, timeout=120)
    assert r2.returncode == 0 and r2.stdout == rtx.encode_p3(dev, dev.render_mis(cam, 2, 6, seed=SEED)[0], 30, 20)
    # the two estimators' flags exclude each other: nothing is rendered
    both = subprocess.run(base + ["--nee", "--mis"], capture_output=True, timeout=120)
    assert both.returncode == 2 and both.stdout == b"" and b"--nee and --mis" in both.stderr
