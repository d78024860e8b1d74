"""Direct-lighting queries (rtx_direct*, k_direct in csrc/rtx_direct.h) at small
shapes: the fused kernel against its own samples (rtx_internal_direct_samples, the device function
the kernel calls) and the public any-hit query, bit for bit; the samples against the contract in
numpy; the closed form under the Cornell light; the hemisphere estimator it replaces; the emitter
table; keys, chunk seams, edges, the device entry point, live scenes and the command line."""
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG, scene_path

pytestmark = pytest.mark.gpu
SEED = 777
SAMPLES = 8
W, H = 32, 18
PRECISIONS = ("parity", "fast")
LIGHT = 3  # RTX_MAT_DIFFUSE_LIGHT
_cache = {}

# a floor, a wall and a blocker under three lights: a triangle, a sphere and a checker-textured rect
MIXED = """rtxscene 1
bvh %d
tex 0 solid 0.7 0.7 0.7
mat 0 lambertian 0
tex 1 solid 9 8 7
mat 1 light 1
tex 2 solid 4 5 6
mat 2 light 2
tex 3 solid 10 10 10
tex 4 solid 2 4 8
tex 5 checker 0.7 3 4
mat 3 light 5
rect xz 0 10 0 10 0 0
rect yz 0 10 0 10 0 0
sphere 5 1.5 5 1 0
tri 1 9 1 4 9.5 1.5 1.5 8.5 4 1
sphere 2.5 6 7 0.5 2
rect xz 6 9 6 9 9.5 3
"""
# two rect lights of areas 1 and 3 over a floor
TWO = """rtxscene 1
bvh 1
tex 0 solid 0.5 0.5 0.5
mat 0 lambertian 0
tex 1 solid 3 3 3
mat 1 light 1
rect xz 0 10 0 10 0 0
rect xz 1 2 1 2 8 1
rect xz 5 8 5 6 8 1
"""


def resolve(total, n):
    """k_radiance_sum's last step: a multiplication by the reciprocal of (double)(float)n."""
    return total * (1.0 / float(np.float64(np.float32(n))))


def in_order_sum(L):
    """L[:, k] added for k = 0, 1, ... starting from 0, as the device adds them."""
    total = np.zeros_like(L[:, 0])
    for k in range(L.shape[1]):
        total = total + L[:, k]
    return total


def centre_rays(cam):
    c, p00 = np.array(cam.center), np.array(cam.pixel00)
    du, dv = np.array(cam.pixel_delta_u), np.array(cam.pixel_delta_v)
    y, x = np.mgrid[0:cam.image_height, 0:cam.image_width]
    d = ((p00 + x.reshape(-1, 1) * du) + y.reshape(-1, 1) * dv) - c
    return np.concatenate([np.broadcast_to(c, d.shape), d], axis=1)


def scene_from(rtx, tmp_path_factory, key, text):
    if key not in _cache:
        path = tmp_path_factory.mktemp("direct") / (key + ".rtxs")
        path.write_text(text)
        host = rtx.HostScene.load(str(path))
        _cache[key] = (rtx.DeviceScene(host), host)
    return _cache[key]


def cornell(rtx):
    """(device scene, points, normals, ids) of the first hits of a 32 x 18 frame of the Cornell
    box, once and left unchanged; the ids are explicit and not the surfels' indices."""
    if "cornell" not in _cache:
        dev = rtx.DeviceScene(rtx.HostScene.load(scene_path("cornell")))
        cam = rtx.camera(rtx.camera_config("cornell_wide", width=W, aspect=16.0 / 9.0))
        assert (cam.image_width, cam.image_height) == (W, H)
        hits = dev.intersect(centre_rays(cam))
        hit = hits["hit"] != 0
        assert 0 < hit.sum() < W * H
        P, N = hits["p"][hit].copy(), hits["normal"][hit].copy()
        ids = ((np.flatnonzero(hit).astype(np.uint64) * 2654435761 + 12345) % (1 << 32)).astype(np.uint32)
        for a in (P, N, ids):
            a.setflags(write=False)
        _cache["cornell"] = (dev, P, N, ids)
    return _cache["cornell"]


def mixed_surfels():
    """A 12 x 12 grid on the floor (normal +y) and one on the wall x = 0 (normal +x)."""
    g = (np.arange(12) + 0.5) * (10.0 / 12.0)
    a, b = [v.ravel() for v in np.meshgrid(g, g)]
    floor = np.stack([a, np.zeros_like(a), b], axis=1)
    wall = np.stack([np.zeros_like(a), a, b], axis=1)
    P = np.concatenate([floor, wall])
    N = np.concatenate([np.tile([0.0, 1.0, 0.0], (len(a), 1)), np.tile([2.0, 0.0, 0.0], (len(a), 1))])
    return P, N


def check_equals_samples(rtx, dev, P, N, ids, first_sample, precision):
    n = len(P)
    smp = rtx.direct_samples(dev, P, N, SAMPLES, SEED, ids=ids, first_sample=first_sample)
    assert smp.shape == (n, SAMPLES, 9)
    seg, Cs = smp[:, :, :6], smp[:, :, 6:]
    occ = dev.occluded(seg.reshape(-1, 6), rtx.RTX_SEAM_TMIN, rtx.RTX_DIRECT_TMAX, precision=precision)
    V = 1.0 - occ.reshape(n, SAMPLES).astype(np.float64)
    want = resolve(in_order_sum(Cs * V[:, :, None]), SAMPLES)
    traced = Cs.any(2)
    want_vis = (traced & (V == 1.0)).sum(1)
    got, vis = dev.direct(P, N, SAMPLES, seed=SEED, ids=ids, first_sample=first_sample, precision=precision,
                          visible=True)
    print(precision, "surfels", n, "traced", int(traced.sum()), "visible", int(want_vis.sum()), "differ",
          int((got != want).any(1).sum()), "max", got.max())
    assert got.shape == (n, 3) and vis.shape == (n,) and vis.dtype == np.uint32
    assert got.tobytes() == want.tobytes()
    assert np.array_equal(vis.astype(np.int64), want_vis)
    assert np.isfinite(got).all() and got.min() >= 0.0
    assert 0 < want_vis.sum() < traced.sum(), "some segments are shadowed, some are not"
    assert not smp[~traced].any(), "all zero where nothing is traced"
    return smp


@pytest.mark.parametrize("precision", PRECISIONS)
def test_equals_its_samples_cornell(rtx_mod, gpu, precision):
    dev, P, N, ids = cornell(rtx_mod)
    check_equals_samples(rtx_mod, dev, P, N, ids, 5, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("bvh", [0, 1])
def test_equals_its_samples_mixed_lights(rtx_mod, gpu, tmp_path_factory, bvh, precision):
    """bvh 0: the flat list; bvh 1: the trees; a triangle, a sphere and a checker-textured rect light."""
    dev, _ = scene_from(rtx_mod, tmp_path_factory, "mixed%d" % bvh, MIXED % bvh)
    P, N = mixed_surfels()
    check_equals_samples(rtx_mod, dev, P, N, None, 0, precision)


def light_geometry(host):
    """The light primitives of a host scene: (index, kind, g, Le(p) callable), areas."""
    arr = host.arrays()
    prims, mats, texs = arr["prims"], arr["materials"], arr["textures"]

    def tex_value(t, p):
        T = texs[t]
        if T["kind"] == 0:
            return np.broadcast_to(T["color"], p.shape).copy()
        assert T["kind"] == 1
        cell = np.floor(T["inv_scale"] * p).astype(np.int64).sum(1)
        even = (cell % 2 == 0)  # (coordinates are positive here: C's % and Python's agree)
        return np.where(even[:, None], tex_value(T["even"], p), tex_value(T["odd"], p))

    lights = []
    for i, q in enumerate(prims):
        if mats[q["material"]]["kind"] == LIGHT:
            lights.append((i, int(q["kind"]), q["g"].copy(), (lambda p, t=int(mats[q["material"]]["texture"]): tex_value(t, p))))
    return lights


def area_of(kind, g):
    if kind == 0:
        return 4.0 * math.pi * g[3] * g[3]
    if kind == 1:
        return 0.5 * np.linalg.norm(np.cross(g[3:6] - g[0:3], g[6:9] - g[0:3]))
    return (g[1] - g[0]) * (g[3] - g[2])


def on_light(kind, g, y, tol=1e-9):
    """Which points y lie on the primitive, and its unit normal there."""
    if kind == 0:
        r = np.linalg.norm(y - g[:3], axis=1)
        return np.abs(r - g[3]) <= tol * g[3], (y - g[:3]) / g[3]
    if kind == 1:
        a, e1, e2 = g[0:3], g[3:6] - g[0:3], g[6:9] - g[0:3]
        nrm = np.cross(e1, e2)
        scale = np.abs(g).max()
        M = np.stack([e1, e2, nrm], axis=1)
        uvw = np.linalg.solve(M, (y - a).T).T
        u, v, w = uvw[:, 0], uvw[:, 1], uvw[:, 2] * np.linalg.norm(nrm)
        ok = (u >= -tol) & (v >= -tol) & (u + v <= 1.0 + tol) & (np.abs(w) <= tol * scale)
        return ok, np.broadcast_to(nrm / np.linalg.norm(nrm), y.shape)
    ax, a0, a1 = {2: (2, 0, 1), 3: (1, 0, 2), 4: (0, 1, 2)}[kind]
    scale = np.abs(g[:5]).max()
    ok = ((y[:, a0] >= g[0] - tol * scale) & (y[:, a0] <= g[1] + tol * scale) & (y[:, a1] >= g[2] - tol * scale)
          & (y[:, a1] <= g[3] + tol * scale) & (np.abs(y[:, ax] - g[4]) <= tol * scale))
    nrm = np.zeros(3)
    nrm[ax] = 1.0
    return ok, np.broadcast_to(nrm, y.shape)


def check_contract(rtx, dev, host, P, N, ids):
    lights = light_geometry(host)
    A = sum(area_of(k, g) for _, k, g, _ in lights)
    smp = rtx.direct_samples(dev, P, N, SAMPLES, SEED, ids=ids).reshape(-1, 9)
    Pn = np.repeat(P, SAMPLES, axis=0)
    unit = np.repeat(N / np.linalg.norm(N, axis=1, keepdims=True), SAMPLES, axis=0)
    traced = smp[:, 6:].any(1)
    assert traced.any()
    o, d, Cs = smp[traced, :3], smp[traced, 3:6], smp[traced, 6:]
    assert o.tobytes() == np.ascontiguousarray(Pn[traced]).tobytes()
    y = o + d
    owner = np.full(len(y), -1)
    want = np.zeros_like(Cs)
    d2 = (d * d).sum(1)
    w = d / np.sqrt(d2)[:, None]
    for li, (_, kind, g, Le) in enumerate(lights):
        ok, ny = on_light(kind, g, y)
        new = ok & (owner < 0)
        owner[new] = li
        cx = np.maximum(0.0, (unit[traced][new] * w[new]).sum(1))
        cy = np.abs((ny[new] * w[new]).sum(1))
        want[new] = Le(y[new]) * (cx * cy * A / (math.pi * d2[new]))[:, None]
    assert (owner >= 0).all(), "every end point lies on a light"
    err = np.abs(Cs - want).max() / np.abs(want).max()
    print("samples", len(smp), "traced", int(traced.sum()), "per light", np.bincount(owner, minlength=len(lights)),
          "C rel err %.2e" % err)
    assert np.abs(Cs - want).max() <= 1e-12 * np.abs(want).max()
    assert (Cs >= 0.0).all() and (Cs > 0.0).any(1).all()
    assert (np.bincount(owner, minlength=len(lights)) > 0).all(), "every light is sampled"
    return A


def test_samples_follow_the_contract(rtx_mod, gpu, tmp_path_factory):
    rtx = rtx_mod
    dev, P, N, ids = cornell(rtx)
    A = check_contract(rtx, dev, dev.host, P, N, ids)
    assert A == 16.0
    mdev, mhost = scene_from(rtx, tmp_path_factory, "mixed1", MIXED % 1)
    MP, MN = mixed_surfels()
    check_contract(rtx, mdev, mhost, MP, MN, None)
    # a point that faces away from every light: C = 0 and all-zero segments, nothing visible
    down = rtx.direct_samples(dev, [[5.0, 5.0, 5.0]], [[0.0, -1.0, 0.0]], 64, SEED)
    assert not down.any()
    rgb, vis = dev.direct([[5.0, 5.0, 5.0]], [[0.0, -1.0, 0.0]], 64, seed=SEED, visible=True)
    assert not rgb.any() and vis[0] == 0


def test_sample_statistics(rtx_mod, gpu, tmp_path_factory):
    rtx = rtx_mod
    dev, _, _, _ = cornell(rtx)
    count = 4096
    smp = rtx.direct_samples(dev, [[5.0, 0.0, 5.0]], [[0.0, 1.0, 0.0]], count, SEED)[0]
    assert smp[:, 6:].any(1).all()
    y = smp[:, :3] + smp[:, 3:6]
    var = 16.0 / 12.0
    for ax in (0, 2):  # uniform on [3, 7]: mean 5, variance 16/12, fourth central moment 4^4 / 80
        m, s2 = y[:, ax].mean(), y[:, ax].var()
        print("axis", ax, "mean", m, "variance", s2)
        assert abs(m - 5.0) <= 5.0 * math.sqrt(var / count)
        assert abs(s2 - var) <= 5.0 * math.sqrt((256.0 / 80.0 - var * var) / count)
    tdev, _ = scene_from(rtx, tmp_path_factory, "two", TWO)
    assert tdev.emitters() == (2, 4.0)
    smp = rtx.direct_samples(tdev, [[4.0, 0.0, 4.0]], [[0.0, 1.0, 0.0]], count, SEED)[0]
    assert smp[:, 6:].any(1).all()
    y = smp[:, :3] + smp[:, 3:6]
    small = (y[:, 0] <= 2.0 + 1e-9)
    big = (y[:, 0] >= 5.0 - 1e-9)
    assert (small ^ big).all()
    share = small.mean()
    print("share of the area-1 light", share)
    assert abs(share - 0.25) <= 5.0 * math.sqrt(0.25 * 0.75 / count)


def form_factor(a, b, h):
    """A differential element to a parallel a x b rect with a corner above it at height h."""
    p, q = math.sqrt(a * a + h * h), math.sqrt(b * b + h * h)
    return (a / p * math.atan(b / p) + b / q * math.atan(a / q)) / (2.0 * math.pi)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_closed_form_under_the_cornell_light(rtx_mod, gpu, precision):
    rtx = rtx_mod
    dev, _, _, _ = cornell(rtx)
    count = 4096
    point, up = [[5.0, 0.0, 5.0]], [[0.0, 1.0, 0.0]]
    got, vis = dev.direct(point, up, count, seed=SEED, precision=precision, visible=True)
    assert vis[0] == count, "nothing shadows the point: the closed form applies"
    want = 15.0 * 4.0 * form_factor(2.0, 2.0, 9.99)
    per = rtx.direct_samples(dev, point, up, count, SEED)[0][:, 6]
    sigma = per.std(ddof=1) / math.sqrt(count)
    print(precision, "direct", got[0], "closed form", want, "sigma", sigma)
    assert got[0, 0] == got[0, 1] == got[0, 2]
    assert abs(got[0, 0] - want) <= 5.0 * sigma


def test_agrees_with_the_hemisphere_estimator(rtx_mod, gpu):
    rtx = rtx_mod
    dev, _, _, _ = cornell(rtx)
    mats = dev.host.arrays()["materials"]
    count = 4096
    # open floor; the wall x = 0; the floor beside the sphere at (3.2, 1, 7), partly in its shadow
    P = np.array([[5.0, 0.0, 5.0], [0.0, 5.0, 5.0], [4.3, 0.0, 7.6]])
    N = np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    smp = rtx.direct_samples(dev, P, N, count, SEED)
    seg, Cs = smp[:, :, :6], smp[:, :, 6]
    occ = dev.occluded(seg.reshape(-1, 6), rtx.RTX_SEAM_TMIN, rtx.RTX_DIRECT_TMAX).reshape(len(P), count)
    d_per = Cs * (1.0 - occ)
    direct = dev.direct(P, N, count, seed=SEED)[:, 0]
    assert np.abs(direct - d_per.mean(1)).max() <= 1e-12 * direct.max()
    rays = rtx.irradiance_rays(dev, P, N, count, SEED)
    hits = dev.intersect(rays.reshape(-1, 6))
    lit = (hits["hit"] != 0) & (mats["kind"][np.maximum(hits["material"], 0)] == LIGHT)
    h_per = 15.0 * lit.reshape(len(P), count).astype(np.float64)
    assert 0 < occ[2].sum() < count, "the third point is partly shadowed"
    for i in range(len(P)):
        dv, hv = d_per[i].var(ddof=1), h_per[i].var(ddof=1)
        se = math.sqrt(dv / count + hv / count)
        print("surfel", i, "direct %.5f hemisphere %.5f combined se %.5f; per-sample variance %.4f vs %.4f (ratio %.1f)"
              % (d_per[i].mean(), h_per[i].mean(), se, dv, hv, hv / dv if dv else float("inf")))
        assert hv > 0.0
        assert abs(d_per[i].mean() - h_per[i].mean()) <= 5.0 * se
    assert d_per[0].var(ddof=1) < h_per[0].var(ddof=1), "the point of the feature"


def fan_scene(count=300):
    """`count` triangle lights fanned about (5, 9, 5), the first and the last of zero area, over a
    floor; a flat list, so the table keeps the file's order."""
    lines = ["rtxscene 1", "bvh 0", "tex 0 solid 0.5 0.5 0.5", "mat 0 lambertian 0", "tex 1 solid 2 2 2",
             "mat 1 light 1", "rect xz 0 10 0 10 0 0"]
    for i in range(count):
        a0, a1 = 2.0 * math.pi * i / count, 2.0 * math.pi * (i + 1) / count
        r = 1.0 + 0.01 * (i % 7)
        if i in (0, count - 1):
            a1 = a0  # b == c: no area
        lines.append("tri 5 9 5 %r 9 %r %r 9 %r 1" % (5 + r * math.cos(a0), 5 + r * math.sin(a0),
                                                      5 + r * math.cos(a1), 5 + r * math.sin(a1)))
    return "\n".join(lines) + "\n"


def test_emitter_table(rtx_mod, gpu, tmp_path):
    rtx = rtx_mod
    path = tmp_path / "fan.rtxs"
    path.write_text(fan_scene())
    host = rtx.HostScene.load(str(path))
    dev = rtx.DeviceScene(host)
    arr = host.arrays()
    prims = arr["prims"]
    is_light = arr["materials"]["kind"][prims["material"]] == LIGHT
    idx, cum = rtx.emitter_table(dev)
    assert idx.dtype == np.int64 and cum.dtype == np.float64
    assert np.array_equal(idx, np.flatnonzero(is_light)) and len(idx) == 300
    areas = np.array([area_of(1, prims[i]["g"]) for i in idx])
    assert (areas == 0.0).sum() == 2 and areas[0] == 0.0 and areas[-1] == 0.0
    assert cum[0] == 0.0 and cum[-1] == cum[-2]
    want = np.cumsum(areas)
    print("emitters", len(idx), "A", cum[-1], "max rel err", np.abs(cum - want).max() / want[-1])
    assert np.abs(cum - want).max() <= 1e-12 * want[-1]
    assert (np.diff(cum) >= 0.0).all()
    assert dev.emitters() == (300, float(cum[-1]))
    again = rtx.DeviceScene(rtx.HostScene.load(str(path)))
    idx2, cum2 = rtx.emitter_table(again)
    assert idx2.tobytes() == idx.tobytes() and cum2.tobytes() == cum.tobytes()
    # no sample lands on an emitter without area: every end point is inside a triangle of the fan
    g = (np.arange(10) + 0.5)
    a, b = [v.ravel() for v in np.meshgrid(g, g)]
    P = np.stack([a, np.zeros_like(a), b], axis=1)
    N = np.tile([0.0, 1.0, 0.0], (len(P), 1))
    smp = rtx.direct_samples(dev, P, N, SAMPLES, SEED).reshape(-1, 9)
    assert smp[:, 6:].any(1).all()
    y = smp[:, :3] + smp[:, 3:6]
    rel = y[:, [0, 2]] - 5.0
    sector = np.floor((np.arctan2(rel[:, 1], rel[:, 0]) % (2.0 * math.pi)) / (2.0 * math.pi / 300)).astype(int)
    radius = np.linalg.norm(rel, axis=1)
    inner = radius > 1e-3  # (the fan's shared apex belongs to every triangle)
    assert not np.isin(sector[inner], (0, 299)).any()
    assert len(np.unique(sector)) > 200
    got, vis = dev.direct(P, N, SAMPLES, seed=SEED, visible=True)
    assert (vis == SAMPLES).all() and (got > 0.0).all()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_keys_and_order(rtx_mod, gpu, precision):
    dev, P, N, ids = cornell(rtx_mod)
    kw = dict(precision=precision, visible=True)
    a = dev.direct(P, N, SAMPLES, seed=SEED, ids=ids, **kw)
    perm = np.random.default_rng(1).permutation(len(P))
    b = dev.direct(P[perm], N[perm], SAMPLES, seed=SEED, ids=ids[perm], **kw)
    assert b[0].tobytes() == a[0][perm].tobytes() and b[1].tobytes() == a[1][perm].tobytes()
    assert b[0].tobytes() != a[0].tobytes()
    c = dev.direct(P, N, SAMPLES, seed=SEED + 1, ids=ids, **kw)
    lit = a[0].any(1)
    assert (c[0] != a[0]).any(1).sum() > lit.sum() // 2
    again = dev.direct(P, N, SAMPLES, seed=SEED, ids=ids, **kw)
    assert again[0].tobytes() == a[0].tobytes() and again[1].tobytes() == a[1].tobytes()
    d = dev.direct(P, N, SAMPLES, seed=SEED, **kw)
    e = dev.direct(P, N, SAMPLES, seed=SEED, ids=np.arange(len(P)), **kw)
    assert d[0].tobytes() == e[0].tobytes() and d[1].tobytes() == e[1].tobytes()
    assert d[0].tobytes() != a[0].tobytes()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_chunking_changes_nothing(rtx_mod, gpu, precision):
    rtx = rtx_mod
    dev, P, N, ids = cornell(rtx)
    pick = (np.arange(200) * 7) % len(P)  # (spread over the frame)
    P, N, pid = P[pick], N[pick], np.arange(1000, 1200, dtype=np.uint32)
    runs = {}
    try:
        for chunk in (64, 7, 3, 0):  # whole surfels per chunk; one per chunk; less than one's samples; default
            rtx.radiance_chunk(chunk)
            runs[chunk] = dev.direct(P, N, 5, seed=SEED, ids=pid, precision=precision, visible=True)
            runs[chunk] += (dev.direct(P, N, 5, seed=SEED, precision=precision),)
    finally:
        rtx.radiance_chunk(0)
    ref = runs[0]
    assert len(np.unique(ref[0], axis=0)) > 50 and 0 < ref[1].max() <= 5
    for chunk in (64, 7, 3):
        for a, b in zip(runs[chunk], ref):
            assert a.tobytes() == b.tobytes(), chunk


@pytest.mark.parametrize("precision", PRECISIONS)
def test_edges(rtx_mod, gpu, precision):
    rtx = rtx_mod
    dev, P, N, ids = cornell(rtx)
    n = len(P)
    kw = dict(seed=SEED, ids=ids, precision=precision, visible=True)
    whole = dev.direct(P, N, SAMPLES, **kw)
    bad = np.zeros(n, bool)
    bad[::3] = True
    N2 = N.copy()
    N2[bad] = 0.0
    N2[1] = [np.nan, 1.0, 0.0]
    N2[2] = [0.0, np.inf, 0.0]
    N2[4] = [1e200, 1e200, 0.0]  # the squared length overflows
    bad[[1, 2, 4]] = True
    got, vis = dev.direct(P, N2, SAMPLES, **kw)
    assert not got[bad].any() and not np.signbit(got[bad]).any() and not vis[bad].any()
    assert got[~bad].tobytes() == whole[0][~bad].tobytes() and vis[~bad].tobytes() == whole[1][~bad].tobytes()
    assert not rtx.direct_samples(dev, P, N2, SAMPLES, SEED, ids=ids)[bad].any()
    # a scene without emitters
    three = rtx.DeviceScene(rtx.HostScene.load(scene_path("three")))
    assert three.emitters() == (0, 0.0)
    idx, cum = rtx.emitter_table(three)
    assert len(idx) == 0 and len(cum) == 0
    z, zv = three.direct(P, N, SAMPLES, **kw)
    assert z.shape == (n, 3) and not z.any() and not zv.any()
    assert not rtx.direct_samples(three, P, N, SAMPLES, SEED).any()
    # surfels on the light itself, its corners included: finite, and 0 (the light is edge-on)
    on = np.array([[3.0, 9.99, 3.0], [7.0, 9.99, 7.0], [5.0, 9.99, 5.0]])
    for nrm in ([0.0, -1.0, 0.0], [0.0, 1.0, 0.0], [1.0, -1.0, 0.0]):
        g, gv = dev.direct(on, np.tile(nrm, (3, 1)), 64, seed=SEED, precision=precision, visible=True)
        assert np.isfinite(g).all() and (g >= 0.0).all()
        assert np.isfinite(rtx.direct_samples(dev, on, np.tile(nrm, (3, 1)), 64, SEED)).all()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_device_entry_on_a_stream(rtx_mod, gpu, precision):
    import torch

    dev, P, N, ids = cornell(rtx_mod)
    n = len(P)
    want, want_vis = dev.direct(P, N, SAMPLES, seed=SEED, ids=ids, first_sample=1, precision=precision, visible=True)
    d_surfels = torch.from_numpy(np.ascontiguousarray(np.concatenate([P, N], axis=1))).cuda()
    d_ids = torch.from_numpy(ids.copy().view(np.int32)).cuda()
    d_out = torch.full((n + 8, 3), -7.0, dtype=torch.float64, device="cuda")
    d_vis = torch.full((n + 8,), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    args = (d_surfels.data_ptr(), n, d_out.data_ptr(), SAMPLES)
    for stream in (None, torch.cuda.Stream()):
        d_out.fill_(-7.0)
        d_vis.fill_(77)
        torch.cuda.synchronize()
        kw = dict(seed=SEED, first_sample=1, precision=precision, stream=stream.cuda_stream if stream else 0)
        dev.direct_device(*args, d_ids=d_ids.data_ptr(), d_visible=d_vis.data_ptr(), **kw)
        if stream:
            stream.synchronize()
        else:
            dev.emitters()  # waits for the scene's stream
            torch.cuda.synchronize()
        out, vis = d_out.cpu().numpy(), d_vis.cpu().numpy().view(np.uint32)
        assert out[:n].tobytes() == want.tobytes() and np.array_equal(vis[:n], want_vis)
        assert (out[n:] == -7.0).all() and (vis[n:] == 77).all()
    # without ids (the surfel's index) and without the counts; then n == 0 writes nothing
    stream = torch.cuda.Stream()
    kw = dict(seed=SEED, first_sample=1, precision=precision, stream=stream.cuda_stream)
    dev.direct_device(*args, **kw)
    stream.synchronize()
    assert d_out.cpu().numpy()[:n].tobytes() == dev.direct(P, N, SAMPLES, seed=SEED, first_sample=1,
                                                           precision=precision).tobytes()
    d_out.fill_(-7.0)
    torch.cuda.synchronize()
    dev.direct_device(d_surfels.data_ptr(), 0, d_out.data_ptr(), SAMPLES, **kw)
    stream.synchronize()
    assert (d_out.cpu().numpy() == -7.0).all()


def test_live_scene(rtx_mod, gpu, tmp_path):
    import torch

    rtx = rtx_mod
    _, P, N, ids = cornell(rtx)
    text = open(scene_path("cornell")).read()
    old = "rect xz 3 7 3 7 9.9900000000000002 3\n"
    assert old in text
    path = tmp_path / "cornell_moved.rtxs"
    path.write_text(text.replace(old, "rect xz 1 7 2 8 9.5 3\n"))
    fresh_host = rtx.HostScene.load(str(path))
    fresh = rtx.DeviceScene(fresh_host)
    kw = dict(seed=SEED, ids=ids, visible=True)
    for how in ("prims", "device"):
        host = rtx.HostScene.load(scene_path("cornell"))
        dev = rtx.DeviceScene(host)
        prims = host.arrays()["prims"]
        li = int(rtx.emitter_table(dev)[0][0])
        assert list(prims[li]["g"][:5]) == [3.0, 7.0, 3.0, 7.0, 9.99] and dev.emitters() == (1, 16.0)
        assert list(fresh_host.arrays()["prims"][li]["g"][:5]) == [1.0, 7.0, 2.0, 8.0, 9.5]
        before = dev.direct(P, N, SAMPLES, **kw)
        table_before = rtx.emitter_table(dev)
        moved = prims[li:li + 1].copy()
        moved[0]["g"][:5] = [1.0, 7.0, 2.0, 8.0, 9.5]
        if how == "prims":
            dev.update_prims(moved, first=li)
        else:
            d_g = torch.from_numpy(moved["g"].copy()).cuda()
            torch.cuda.synchronize()
            dev.update_geometry_device(d_g.data_ptr(), li, 1)
        assert dev.epoch() == 1
        assert dev.emitters() == (1, 36.0)
        t_new, t_want = rtx.emitter_table(dev), rtx.emitter_table(fresh)
        assert t_new[0].tobytes() == t_want[0].tobytes() and t_new[1].tobytes() == t_want[1].tobytes()
        assert t_new[1].tobytes() != table_before[1].tobytes()
        for precision in PRECISIONS:
            after = dev.direct(P, N, SAMPLES, precision=precision, **kw)
            want = fresh.direct(P, N, SAMPLES, precision=precision, **kw)
            assert after[0].tobytes() == want[0].tobytes() and after[1].tobytes() == want[1].tobytes()
            assert after[0].tobytes() != before[0].tobytes()


def test_command_line_direct_pass(rtx_mod, gpu):
    exe = os.path.join(PKG, "raytracer")
    cams = os.path.join(os.path.dirname(PKG), "configs", "cameras.json")
    # (the wide preset sees past the box and the light itself; the `cornell` one sees neither)
    r = subprocess.run([exe, "cornell_wide", "--scene", scene_path("cornell"), "--cameras", cams, "--direct", "4"],
                       capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    tok = r.stdout.split()
    assert tok[0] == b"P3" and tok[3] == b"255"
    w, h = int(tok[1]), int(tok[2])
    cam = rtx_mod.camera(rtx_mod.camera_config("cornell_wide"))
    assert (w, h) == (cam.image_width, cam.image_height)
    px = np.array(tok[4:], dtype=np.int64).reshape(h * w, 3)
    assert px.min() >= 0 and px.max() <= 255
    assert (px == 0).all(1).any(), "black: a miss, the light itself, a shadow"
    assert (px > 0).any(1).any(), "lit"
    assert b"direct: 4 samples, 1 emitters\n" in r.stderr, r.stderr.decode()
    bad = subprocess.run([exe, "cornell", "--direct", "0"], capture_output=True, timeout=120)
    assert bad.returncode == 2
