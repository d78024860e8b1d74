"""The device's hemisphere and light samplers (cosine_direction in csrc/rtx_occlusion.h,
direct_sample_from in csrc/rtx_direct.h) against the reference of tests/query_sample_cases.py:
every direction of the irradiance and AO hooks, the emitter table bit for bit at sizes around the
scan's 256 lanes, every sample of the direct and next-event hooks (the emitter picked, y - x bit for
bit on rects and triangles, C), the all-zero rows, and rtx_direct itself against the closed forms
under a sphere, a triangle and the three rects.  tests/test_query_samples_host.py shows, without a
GPU, that the reference is right and that these comparisons have power."""
import numpy as np
import pytest

import query_sample_cases as qs
from conftest import scene_path

pytestmark = pytest.mark.gpu
SEED = 4242
SAMPLES = 8
TOL = 1e-12
W, H = 64, 36
AO_FRAMES = {"three": ("c1_three", 0.75), "bunny": ("c3_bunny", 1.5)}  # test_gpu_ao.py's frames
_scenes = {}


def device_scene(rtx, key, text=None):
    """A device scene of inline text, or of a golden scene file by name, made once."""
    if key not in _scenes:
        host = rtx.HostScene.load(scene_path(key)) if text is None else qs.load_host(rtx, text)
        _scenes[key] = rtx.DeviceScene(host)
    return _scenes[key]


# ---------------------------------------------------------------------------------------
# directions
# ---------------------------------------------------------------------------------------
def test_irradiance_directions(rtx_mod, orc, gpu):
    rtx = rtx_mod
    dev = device_scene(rtx, "three")
    N = qs.direction_normals()
    n = len(N)
    assert n == 213
    P = np.random.default_rng(8).uniform(-3.0, 3.0, size=(n, 3))
    ids = qs.odd_ids(n)
    assert (ids != np.arange(n)).all()
    both = {abs(qs.basis(v)[2][0]) > 0.9 for v in N[6:9]}
    assert both == {False, True}, "the basis choice flips between the neighbours of x = 0.9"
    for first in (0, 5):
        rays = rtx.irradiance_rays(dev, P, N, SAMPLES, SEED, ids=ids, first_sample=first)
        assert rays.shape == (n, SAMPLES, 6)
        assert rays[:, :, :3].tobytes() == np.ascontiguousarray(np.repeat(P[:, None, :], SAMPLES, 1)).tobytes()
        want = np.stack([qs.cosine_direction_ref(SEED, ids[i], first, qs.STREAM_IRR, N[i], SAMPLES) for i in range(n)])
        err = np.abs(rays[:, :, 3:] - want).max(axis=(1, 2))
        print("first_sample", first, "directions", n * SAMPLES, "largest deviation %.3e" % err.max(), "at normal",
              N[err.argmax()])
        assert err.max() <= TOL


@pytest.mark.parametrize("precision", ["parity", "fast"])
@pytest.mark.parametrize("name", list(AO_FRAMES))
def test_ao_directions(rtx_mod, orc, gpu, name, precision):
    rtx = rtx_mod
    preset, radius = AO_FRAMES[name]
    dev = device_scene(rtx, name)
    cam = rtx.camera(rtx.camera_config(preset, width=W))
    assert (cam.image_width, cam.image_height) == (W, H)
    rays = rtx.ao_rays(dev, cam, samples=SAMPLES, radius=radius, seed=SEED, precision=precision)
    c, p00 = np.array(cam.center), np.array(cam.pixel00)
    du, dv = np.array(cam.pixel_delta_u), np.array(cam.pixel_delta_v)
    y, x = np.mgrid[0:H, 0:W]
    d = ((p00 + x.reshape(-1, 1) * du) + y.reshape(-1, 1) * dv) - c
    hits = dev.intersect(np.concatenate([np.broadcast_to(c, d.shape), d], axis=1), precision=precision)
    hit = hits["hit"] != 0
    assert 0 < hit.sum() < W * H and rays.shape == (W * H, SAMPLES, 6)
    assert not rays[~hit].any(), "a pixel that misses has no rays"
    o_err = np.abs(rays[hit][:, :, :3] - hits["p"][hit][:, None, :]).max()
    worst = 0.0
    for pix in np.flatnonzero(hit):  # pix = y W + x: the row-major index itself
        want = qs.cosine_direction_ref(SEED, pix, 0, qs.STREAM_AO, hits["normal"][pix], SAMPLES)
        worst = max(worst, np.abs(rays[pix, :, 3:] - want).max())
    print(name, precision, "pixels that hit", int(hit.sum()), "largest deviation: direction %.3e origin %.3e"
          % (worst, o_err))
    assert worst <= TOL
    assert o_err <= TOL * np.abs(hits["p"][hit]).max()


# ---------------------------------------------------------------------------------------
# the emitter table
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", qs.TABLE_SIZES)
def test_emitter_table(rtx_mod, gpu, n):
    rtx = rtx_mod
    text = qs.table_scene(n)
    L = qs.lights_of(text)
    host = qs.load_host(rtx, text)
    dev = rtx.DeviceScene(host)
    idx, cum = rtx.emitter_table(dev)
    assert len(idx) == n and idx.tobytes() == L.idx.tobytes()
    differ = int((cum != L.cum).sum())
    print("n", n, "A", cum[-1] if n else 0.0, "entries that differ", differ, "largest deviation",
          np.abs(cum - L.cum).max())
    assert cum.tobytes() == L.cum.tobytes()
    assert dev.emitters() == (n, float(L.cum[-1]))
    # one light rescaled in place: the table of a fresh scene with that light
    k = int(np.flatnonzero(L.areas > 0.0)[len(L.areas.nonzero()[0]) // 2])
    li = int(L.idx[k])
    prim = host.arrays()["prims"][li:li + 1].copy()
    a = prim[0]["g"][0:3].copy()
    for s in (3, 6):
        prim[0]["g"][s:s + 3] = a + 1.75 * (prim[0]["g"][s:s + 3] - a)
    dev.update_prims(prim, first=li)
    lines = text.splitlines()
    at = len(lines) - n + k
    assert lines[at].startswith("tri ")
    lines[at] = "tri " + " ".join(repr(float(v)) for v in prim[0]["g"]) + " 1"
    fresh_text = "\n".join(lines) + "\n"
    fresh = rtx.DeviceScene(qs.load_host(rtx, fresh_text))
    t_new, t_want = rtx.emitter_table(dev), rtx.emitter_table(fresh)
    assert t_new[0].tobytes() == t_want[0].tobytes() and t_new[1].tobytes() == t_want[1].tobytes()
    assert t_new[1].tobytes() == qs.lights_of(fresh_text).cum.tobytes()
    assert t_new[1].tobytes() != cum.tobytes() and dev.emitters() == (n, float(t_want[1][-1]))


# ---------------------------------------------------------------------------------------
# samples
# ---------------------------------------------------------------------------------------
SAMPLE_SCENES = list(qs.ONE_LIGHT) + ["mixed", "table300", "table513"]


def sample_scene(name):
    """(scene text, points, normals): a one-light scene with its query points and its all-zero
    rows, the scene of every kind, or an emitter table.  (Built inside the test: the library is
    loaded by the rtx_mod fixture, not while the tests are collected.)"""
    if name in qs.ONE_LIGHT:
        P, N = qs.one_light_points(name)
        ZP, ZN = qs.zero_rows(name)
        return qs.one_light_text(name), np.concatenate([P, ZP]), np.concatenate([N, ZN])
    if name == "mixed":
        return (qs.MIXED,) + qs.mixed_surfels()
    return (qs.table_scene(int(name[5:])),) + qs.floor_surfels(3)


@pytest.mark.parametrize("name", SAMPLE_SCENES)
def test_samples(rtx_mod, orc, gpu, name):
    rtx = rtx_mod
    text, P, N = sample_scene(name)
    dev = device_scene(rtx, "samples_" + name, text)
    L = qs.lights_of(text)
    idx, cum = rtx.emitter_table(dev)
    assert idx.tobytes() == L.idx.tobytes() and cum.tobytes() == L.cum.tobytes()
    n = len(P)
    ids = qs.odd_ids(n, salt=len(text))
    count = 64 if name.startswith("table") else SAMPLES
    reasons, kinds, rows = set(), set(), 0
    worst_c = worst_seg = 0.0
    for depth, first in ((None, 0), (None, 5), (0, 0), (1, 3), (3, 0)):
        if depth is None:
            got = rtx.direct_samples(dev, P, N, count, SEED, ids=ids, first_sample=first)
        else:
            got = rtx.nee_samples(dev, P, N, count, SEED, depth, ids=ids, first_sample=first)
        want, pick, why = qs.direct_table_ref(L, SEED, P, N, ids, count, first, depth)
        assert got.shape == want.shape == (n, count, 9)
        traced = why == qs.TRACED
        assert ((got != 0.0).any(2) == traced).all(), "the same rows are all zero"
        assert not got[~traced].any() and not want[~traced].any()
        assert got[:, :, 0:3].tobytes() == want[:, :, 0:3].tobytes(), "the origin is the point itself"
        flat = L.kind[np.maximum(pick, 0)]
        exact = traced & (flat != qs.SPHERE)
        gs, ws = got[:, :, 3:6], want[:, :, 3:6]
        bad = int((gs[exact] != ws[exact]).any(1).sum())
        seg_err = np.abs(gs - ws).max() / np.abs(ws).max()
        c_err = np.abs(got[:, :, 6:9] - want[:, :, 6:9]).max() / np.abs(want[:, :, 6:9]).max()
        print(name, "depth", depth, "first", first, "samples", n * count, "traced", int(traced.sum()),
              "rect / triangle segments", int(exact.sum()), "not bit-equal", bad,
              "largest deviation: segment %.3e C %.3e" % (seg_err, c_err))
        assert bad == 0, "y - x of a rect or a triangle is the header's formula bit for bit"
        # a segment within the bound ends on the emitter the reference picked: y is the reference's
        assert seg_err <= TOL and c_err <= TOL
        worst_c, worst_seg = max(worst_c, c_err), max(worst_seg, seg_err)
        reasons |= set(why.ravel())
        kinds |= set(flat[traced])
        rows += int(traced.sum())
    print(name, "largest deviation over all: segment %.3e C %.3e" % (worst_seg, worst_c), "reasons", sorted(int(r) for r in reasons),
          "kinds", sorted(int(k) for k in kinds))
    assert rows > 0
    if name in qs.ONE_LIGHT:
        zero = {qs.FACES_AWAY, qs.BAD_NORMAL} | ({qs.EDGE_ON} if name.endswith("rect") else set())
        assert zero <= reasons, "every all-zero class of the scene is met"
        assert kinds == {int(L.kind[0])}
    elif name == "mixed":
        assert {qs.FACES_AWAY, qs.BAD_NORMAL, qs.EDGE_ON, qs.BLACK} <= reasons
        assert kinds == {0, 1, 2, 3, 4}, "hits on every light kind"
    else:
        assert len(np.unique(pick)) > 150 and (L.areas[pick.ravel()] > 0.0).all()


# ---------------------------------------------------------------------------------------
# the closed forms through rtx_direct
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["parity", "fast"])
@pytest.mark.parametrize("bvh", [0, 1])
@pytest.mark.parametrize("name", list(qs.ONE_LIGHT))
def test_direct_reaches_the_closed_form(rtx_mod, orc, gpu, name, bvh, precision):
    rtx = rtx_mod
    dev = device_scene(rtx, "%s_bvh%d" % (name, bvh), qs.one_light_text(name, bvh))
    P, N = qs.one_light_points(name)
    ref = qs.mean_reference(name)
    got, vis = dev.direct(P, N, qs.N_MEAN, seed=qs.MEAN_SEED, ids=qs.MEAN_IDS, precision=precision, visible=True)
    worst = 0.0
    for i, (want, mean, sigma, _) in enumerate(ref):
        z = (got[i] - want) / sigma
        print(name, "bvh", bvh, precision, "point", i, "direct", got[i], "closed form", want, "sigma", sigma,
              "z", np.round(z, 2), "visible", int(vis[i]), "reference mean", mean,
              "device - reference %.3e" % np.abs(got[i] - mean).max())
        worst = max(worst, np.abs(z).max())
        assert np.abs(z).max() <= 5.0
        if name != "sphere":
            assert vis[i] == qs.N_MEAN, "nothing shadows the light"
        else:
            assert 0 < vis[i] < qs.N_MEAN, "the sphere's far side is rejected by its own occlusion"
    print(name, "bvh", bvh, precision, "largest |z|", worst)
