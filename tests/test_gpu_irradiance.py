"""Irradiance queries (rtx_irradiance*, k_irradiance in csrc/rtx_irradiance.h) on
32 x 18 frames at 8 samples, depth 8: the fused kernel against its own depth-0 rays
(rtx_internal_irradiance_rays, the device function the kernel calls) traced one sample at a time
through rtx_radiance, bit for bit; the rays' geometry and the moments of a cosine-weighted
hemisphere; the open sky in closed form; keys, chunk seams, degenerate normals, the device entry
point, live scenes and the command line.

Surfels are the first hits (point, record normal) of the rays through the pixel centres."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG, scene_path

pytestmark = pytest.mark.gpu
SEED = 4242
SAMPLES, DEPTH = 8, 8
W, H = 32, 18
PRECISIONS = ("parity", "fast")
# scene -> camera preset and overrides (32 x 18 frames)
FRAMES = {
    "cornell": ("cornell_wide", dict(aspect=16.0 / 9.0)),  # emitter, closed box (wide enough to see past it)
    "three": ("c1_three", {}),                             # global sphere; the flat list
    "bunny": ("c3_bunny", {}),                             # the fast tree, triangles
}
_frames = {}


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
    """The ray through each pixel's centre (the ray of rtx_aov), row-major, (H * W, 6)."""
    c, p00 = np.array(cam.center), np.array(cam.pixel00)
    du, dv = np.array(cam.pixel_delta_u), np.array(cam.pixel_delta_v)
    y, x = np.mgrid[0:cam.image_height, 0:cam.image_width]
    d = ((p00 + x.reshape(-1, 1) * du) + y.reshape(-1, 1) * dv) - c
    return np.concatenate([np.broadcast_to(c, d.shape), d], axis=1)


def frame(rtx, name):
    """(device scene, points, normals, ids) of the pixels of a 32 x 18 frame that hit, once per
    scene and left unchanged.  The ids are explicit and not the surfels' indices."""
    if name not in _frames:
        preset, over = FRAMES[name]
        dev = rtx.DeviceScene(rtx.HostScene.load(scene_path(name)))
        cam = rtx.camera(rtx.camera_config(preset, width=W, **over))
        assert (cam.image_width, cam.image_height) == (W, H)
        hits = dev.intersect(centre_rays(cam))
        hit = hits["hit"] != 0
        assert 0 < hit.sum() < W * H, "some pixels must hit, some miss"
        P, N = hits["p"][hit].copy(), hits["normal"][hit].copy()
        ids = ((np.flatnonzero(hit).astype(np.uint64) * 2654435761 + 12345) % (1 << 32)).astype(np.uint32)
        assert len(np.unique(ids)) == len(ids)
        for a in (P, N, ids):
            a.setflags(write=False)
        _frames[name] = (dev, P, N, ids)
    return _frames[name]


def emitter_bound(name, depth):
    """The largest radiance a path of `depth` bounces can carry in scene `name`, from its scene
    file: the brightest source is the sky (at most 1.0 per channel, sky() in rtx_device.h) or the
    brightest `light` texture; a bounce multiplies the throughput by an albedo of at most 1 (a
    dielectric: exactly 1), and Russian roulette, which acts on children of depth 6 and more,
    divides it by q <= 0.95 at most once per bounce and only down to a largest component of 1
    unless it was above 0.95 already (shade_finish): (1 / 0.95)^(depth - 5) in all.  A diffuse
    bounce's cos / pdf is pi only to f32 rounding (the pdf is a float, shade_core): a factor of at
    most 1 + 2^-23 per bounce on top."""
    tex, lights = {}, []
    for line in open(scene_path(name)):
        t = line.split()
        if t[:1] == ["tex"] and t[2] == "solid":
            tex[int(t[1])] = max(float(v) for v in t[3:6])
        if t[:1] == ["mat"] and t[2] == "light":
            lights.append(tex[int(t[3])])
    return max([1.0] + lights) * (1.0 / 0.95) ** max(0, depth - 5) * (1.0 + 2.0 ** -23) ** depth, lights


@pytest.mark.parametrize("first_sample", [0, 5])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(FRAMES))
def test_equals_its_rays_through_radiance(rtx_mod, gpu, name, precision, first_sample):
    rtx = rtx_mod
    dev, P, N, ids = frame(rtx, name)
    n = len(P)
    rays = rtx.irradiance_rays(dev, P, N, SAMPLES, SEED, ids=ids, first_sample=first_sample)
    assert rays.shape == (n, SAMPLES, 6)
    L, S = np.zeros((n, SAMPLES, 3)), np.zeros((n, SAMPLES), np.uint64)
    for k in range(SAMPLES):
        L[:, k], S[:, k] = dev.radiance(rays[:, k], 1, DEPTH, seed=SEED, ids=ids, first_sample=first_sample + k,
                                        precision=precision, segments=True)
    want = resolve(in_order_sum(L), SAMPLES)
    got, segs = dev.irradiance(P, N, SAMPLES, DEPTH, seed=SEED, ids=ids, first_sample=first_sample,
                               precision=precision, segments=True)
    differ = int((got != want).any(1).sum())
    print(name, precision, first_sample, "surfels", n, "that differ:", differ, "segments", int(S.sum()),
          "range", got.min(), got.max())
    assert got.shape == (n, 3) and segs.shape == (n,) and segs.dtype == np.uint32
    assert got.tobytes() == want.tobytes(), differ
    assert np.array_equal(segs.astype(np.uint64), S.sum(1))
    assert len(np.unique(got, axis=0)) > n // 4, "not all values are equal"
    assert (S > 1).any(), "paths bounce"
    assert segs.min() >= SAMPLES
    # the finite, non-negative range the values must lie in (the mean of values in it)
    top, lights = emitter_bound(name, DEPTH)
    assert np.isfinite(got).all() and got.min() >= 0.0 and got.max() <= top, (got.max(), top)
    if name == "cornell":
        assert lights == [15.0] and 15.0 * (1.0 / 0.95) ** 3 <= top < 17.5
        # more than the sky could give at this depth: the emitter's light arrives
        assert got.max() > (1.0 / 0.95) ** 3
    else:
        assert not lights


@pytest.mark.parametrize("name", list(FRAMES))
def test_ray_geometry(rtx_mod, gpu, name):
    rtx = rtx_mod
    dev, P, N, ids = frame(rtx, name)
    unit = N / np.linalg.norm(N, axis=1, keepdims=True)
    rays = rtx.irradiance_rays(dev, P, N, SAMPLES, SEED, ids=ids)
    o, d = rays[:, :, :3], rays[:, :, 3:]
    assert o.tobytes() == np.ascontiguousarray(np.broadcast_to(P[:, None, :], o.shape)).tobytes()
    assert np.abs(np.linalg.norm(d, axis=2) - 1.0).max() <= 1e-12
    cos = (d * unit[:, None, :]).sum(2)
    assert cos.min() >= 0.0
    # moments of a cosine-weighted hemisphere: E cos = 2/3, Var cos = 1/2 - 4/9 = 1/18
    sigma = np.sqrt((1.0 / 18.0) / cos.size)
    print(name, "mean cos %.5f over %d rays, sigma %.2e" % (cos.mean(), cos.size, sigma))
    assert abs(cos.mean() - 2.0 / 3.0) <= 5.0 * sigma
    assert len(np.unique(d.reshape(-1, 3), axis=0)) == d.size // 3, "every sample has a direction of its own"
    # the normal's length does not matter
    scaled = rtx.irradiance_rays(dev, P, 3.7 * N, SAMPLES, SEED, ids=ids)
    ds = scaled[:, :, 3:]
    assert scaled[:, :, :3].tobytes() == o.tobytes()
    assert np.abs(np.linalg.norm(ds, axis=2) - 1.0).max() <= 1e-12
    assert ((ds * unit[:, None, :]).sum(2) >= 0.0).all()
    assert np.abs(ds - d).max() <= 1e-12


@pytest.mark.parametrize("name", list(FRAMES))
def test_open_sky_is_analytic(rtx_mod, gpu, name):
    rtx = rtx_mod
    dev, _, _, _ = frame(rtx, name)
    box = rtx.prim_bounds(dev.host.arrays()["prims"])
    lo, hi = box[:, :3].min(0), box[:, 3:].max(0)
    point = np.array([[0.5 * (lo[0] + hi[0]), hi[1] + 1.0, 0.5 * (lo[2] + hi[2])]])
    up = np.array([[0.0, 1.0, 0.0]])
    count = 4096
    rays = rtx.irradiance_rays(dev, point, up, count, SEED)[0]
    d = rays[:, 3:]
    assert (d[:, 1] >= 0.0).all()
    ud = d * (1.0 / np.sqrt((d * d).sum(1)))[:, None]
    t = 0.5 * (ud[:, 1] + 1.0)
    sky = (1.0 - t)[:, None] * np.ones(3) + t[:, None] * np.array([0.5, 0.7, 1.0])
    want = resolve(in_order_sum(sky[None]), count)[0]
    for precision in PRECISIONS:
        got, segs = dev.irradiance(point, up, count, DEPTH, seed=SEED, precision=precision, segments=True)
        print(name, precision, got[0], want)
        assert segs[0] == count, "every path is one segment"
        assert np.abs(got[0] - want).max() <= 1e-12 * np.abs(want).max()
        # E t = (E cos + 1) / 2 = 5/6 and Var t = Var cos / 4 = 1/72 for the normal +y
        for ch, c in ((0, 0.5), (1, 0.7)):
            sigma = (1.0 - c) * np.sqrt((1.0 / 72.0) / count)
            assert abs(got[0, ch] - (1.0 - (5.0 / 6.0) * (1.0 - c))) <= 5.0 * sigma, (ch, got[0, ch])
        assert abs(got[0, 2] - 1.0) <= 1e-12


@pytest.mark.parametrize("precision", PRECISIONS)
def test_keys_and_order(rtx_mod, gpu, precision):
    dev, P, N, ids = frame(rtx_mod, "cornell")
    kw = dict(precision=precision, segments=True)
    a = dev.irradiance(P, N, SAMPLES, DEPTH, seed=SEED, ids=ids, **kw)
    perm = np.random.default_rng(1).permutation(len(P))
    b = dev.irradiance(P[perm], N[perm], SAMPLES, DEPTH, seed=SEED, ids=ids[perm], **kw)
    assert b[0].tobytes() == a[0][perm].tobytes() and b[1].tobytes() == a[1][perm].tobytes()
    assert b[0].tobytes() != a[0].tobytes()
    c = dev.irradiance(P, N, SAMPLES, DEPTH, seed=SEED + 1, ids=ids, **kw)
    assert (c[0] != a[0]).any(1).sum() > len(P) // 2
    again = dev.irradiance(P, N, SAMPLES, DEPTH, seed=SEED, ids=ids, **kw)
    assert again[0].tobytes() == a[0].tobytes() and again[1].tobytes() == a[1].tobytes()
    # ids = None is the surfel's index
    d = dev.irradiance(P, N, SAMPLES, DEPTH, seed=SEED, **kw)
    e = dev.irradiance(P, N, SAMPLES, DEPTH, seed=SEED, ids=np.arange(len(P)), **kw)
    assert d[0].tobytes() == e[0].tobytes() and d[1].tobytes() == e[1].tobytes()
    assert d[0].tobytes() != a[0].tobytes()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_chunking_changes_nothing(rtx_mod, gpu, precision):
    rtx = rtx_mod
    dev, P, N, ids = frame(rtx, "bunny")
    pick = np.arange(200) % len(P)
    P, N, pid = P[pick], N[pick], np.arange(1000, 1200, dtype=np.uint32)
    runs = {}
    try:
        for chunk in (64, 7, 3, 0):  # whole surfels per chunk; one per chunk; less than one's samples; default
            rtx.radiance_chunk(chunk)
            runs[chunk] = dev.irradiance(P, N, 5, DEPTH, seed=SEED, ids=pid, precision=precision, segments=True)
            # the host entry point without ids keys by the surfel's index, whatever the chunking
            runs[chunk] += (dev.irradiance(P, N, 5, DEPTH, seed=SEED, precision=precision),)
    finally:
        rtx.radiance_chunk(0)
    ref = runs[0]
    assert len(np.unique(ref[0], axis=0)) > 50 and ref[1].min() >= 5 and ref[1].max() > 5
    for chunk in (64, 7, 3):
        for a, b in zip(runs[chunk], ref):
            assert a.tobytes() == b.tobytes(), chunk


@pytest.mark.parametrize("precision", PRECISIONS)
def test_degenerate_normals(rtx_mod, gpu, precision):
    rtx = rtx_mod
    dev, P, N, ids = frame(rtx, "three")
    n = len(P)
    whole = dev.irradiance(P, N, SAMPLES, DEPTH, seed=SEED, ids=ids, precision=precision, segments=True)
    bad = np.zeros(n, bool)
    bad[::3] = True
    N2 = N.copy()
    N2[bad] = 0.0
    nan_at = 1
    N2[nan_at] = [np.nan, 1.0, 0.0]
    bad[nan_at] = True
    assert 0 < bad.sum() < n
    got, segs = dev.irradiance(P, N2, SAMPLES, DEPTH, seed=SEED, ids=ids, precision=precision, segments=True)
    assert not got[bad].any() and not np.signbit(got[bad]).any() and not segs[bad].any()
    assert got[~bad].tobytes() == whole[0][~bad].tobytes() and segs[~bad].tobytes() == whole[1][~bad].tobytes()
    assert whole[1].min() >= SAMPLES
    rays = rtx.irradiance_rays(dev, P, N2, SAMPLES, SEED, ids=ids)
    assert not rays[bad].any()
    assert rays[~bad].tobytes() == rtx.irradiance_rays(dev, P, N, SAMPLES, SEED, ids=ids)[~bad].tobytes()
    # an infinite normal has no finite squared length either
    N3 = N.copy()
    N3[0] = [0.0, np.inf, 0.0]
    got3, segs3 = dev.irradiance(P, N3, SAMPLES, DEPTH, seed=SEED, ids=ids, precision=precision, segments=True)
    assert not got3[0].any() and segs3[0] == 0 and got3[1:].tobytes() == whole[0][1:].tobytes()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_device_entry_on_a_stream(rtx_mod, gpu, precision):
    import torch

    dev, P, N, ids = frame(rtx_mod, "bunny")
    n = len(P)
    want, want_segs = dev.irradiance(P, N, SAMPLES, DEPTH, seed=SEED, ids=ids, first_sample=1, precision=precision,
                                     segments=True)
    d_surfels = torch.from_numpy(np.ascontiguousarray(np.concatenate([P, N], axis=1))).cuda()
    d_ids = torch.from_numpy(ids.copy().view(np.int32)).cuda()
    d_out = torch.full((n + 8, 3), -7.0, dtype=torch.float64, device="cuda")
    d_segs = torch.full((n + 8,), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    args = (d_surfels.data_ptr(), n, d_out.data_ptr(), SAMPLES, DEPTH)
    kw = dict(seed=SEED, first_sample=1, precision=precision, stream=stream.cuda_stream)
    dev.irradiance_device(*args, d_ids=d_ids.data_ptr(), d_segments=d_segs.data_ptr(), **kw)
    stream.synchronize()
    out, segs = d_out.cpu().numpy(), d_segs.cpu().numpy().view(np.uint32)
    assert out[:n].tobytes() == want.tobytes() and np.array_equal(segs[:n], want_segs)
    assert (out[n:] == -7.0).all() and (segs[n:] == 77).all()
    # without ids (the surfel's index) and without segments
    d_out.fill_(-7.0)
    torch.cuda.synchronize()
    dev.irradiance_device(*args, **kw)
    stream.synchronize()
    assert d_out.cpu().numpy()[:n].tobytes() == dev.irradiance(P, N, SAMPLES, DEPTH, seed=SEED, first_sample=1,
                                                               precision=precision).tobytes()
    # n == 0: OK, nothing written
    d_out.fill_(-7.0)
    d_segs.fill_(77)
    torch.cuda.synchronize()
    dev.irradiance_device(d_surfels.data_ptr(), 0, d_out.data_ptr(), SAMPLES, DEPTH, d_ids=d_ids.data_ptr(),
                          d_segments=d_segs.data_ptr(), **kw)
    stream.synchronize()
    assert (d_out.cpu().numpy() == -7.0).all() and (d_segs.cpu().numpy() == 77).all()
    out0, segs0 = dev.irradiance(np.zeros((0, 3)), np.zeros((0, 3)), SAMPLES, DEPTH, segments=True)
    assert out0.shape == (0, 3) and segs0.shape == (0,)


def test_live_scene(rtx_mod, gpu, tmp_path):
    rtx = rtx_mod
    _, P, N, ids = frame(rtx, "three")
    host = rtx.HostScene.load(scene_path("three"))
    dev = rtx.DeviceScene(host)
    kw = dict(seed=SEED, ids=ids, segments=True)
    before = dev.irradiance(P, N, SAMPLES, DEPTH, **kw)
    prims = host.arrays()["prims"]
    assert prims[2]["kind"] == 0 and list(prims[2]["g"][:4]) == [1.0, 0.0, -1.0, 0.5]
    # a surfel on the ground, in the open: the sphere goes right above it
    assert list(prims[0]["g"][:4]) == [0.0, -100.5, -1.0, 100.0] and list(prims[1]["g"][:4]) == [0.0, 0.0, -1.2, 0.5]
    on_ground = np.abs(np.linalg.norm(P - prims[0]["g"][:3], axis=1) - 100.0) < 1e-6
    clear = np.minimum(np.linalg.norm(P - prims[1]["g"][:3], axis=1), np.linalg.norm(P - prims[2]["g"][:3], axis=1))
    near = on_ground & (np.linalg.norm(P, axis=1) < 4.0) & (clear > 1.5)
    assert near.any()
    s = int(np.flatnonzero(near)[0])
    centre = [float(P[s, 0]), float(P[s, 1]) + 0.6, float(P[s, 2])]
    moved = prims[2:3].copy()
    moved[0]["g"][:3] = centre
    dev.update_prims(moved, first=2)
    assert dev.epoch() == 1
    text = open(scene_path("three")).read()
    assert "sphere 1 0 -1 0.5 2\n" in text
    path = tmp_path / "three_moved.rtxs"
    path.write_text(text.replace("sphere 1 0 -1 0.5 2\n", "sphere %r %r %r 0.5 2\n" % tuple(centre)))
    fresh_host = rtx.HostScene.load(str(path))
    assert list(fresh_host.arrays()["prims"][2]["g"][:3]) == centre
    fresh = rtx.DeviceScene(fresh_host)
    for precision in PRECISIONS:
        after = dev.irradiance(P, N, SAMPLES, DEPTH, precision=precision, **kw)
        want = fresh.irradiance(P, N, SAMPLES, DEPTH, precision=precision, **kw)
        assert after[0].tobytes() == want[0].tobytes() and after[1].tobytes() == want[1].tobytes()
        assert (after[0][s] != before[0][s]).any()
        assert after[1][s] > before[1][s], "paths that reached the sky now bounce off the sphere"


def test_command_line_irradiance_pass(rtx_mod, gpu):
    exe = os.path.join(PKG, "raytracer")
    cams = os.path.join(os.path.dirname(PKG), "configs", "cameras.json")
    r = subprocess.run([exe, "c1_three", "--scene", scene_path("three"), "--cameras", cams, "--irradiance", "4"],
                       capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    tok = r.stdout.split()
    assert tok[0] == b"P3" and tok[3] == b"255"
    w, h = int(tok[1]), int(tok[2])
    cfg = rtx_mod.camera_config("c1_three")
    cam = rtx_mod.camera(cfg)
    assert (w, h) == (cam.image_width, cam.image_height)
    px = np.array(tok[4:], dtype=np.int64).reshape(h * w, 3)
    assert px.min() >= 0 and px.max() <= 255 and len(np.unique(px, axis=0)) > 2
    assert (px == 0).all(1).any(), "a pixel whose ray misses is black"
    # the default depth is the preset's
    assert re.search(rb"irradiance: 4 samples, depth %d\b" % cfg.max_depth, r.stderr), r.stderr.decode()
    r2 = subprocess.run([exe, "c1_three", "--scene", scene_path("three"), "--cameras", cams, "--irradiance", "2,3"],
                        capture_output=True, timeout=120)
    assert r2.returncode == 0 and r2.stdout.startswith(b"P3"), r2.stderr.decode()
    assert b"irradiance: 2 samples, depth 3\n" in r2.stderr
    bad = subprocess.run([exe, "c1_three", "--irradiance", "0"], capture_output=True, timeout=120)
    assert bad.returncode == 2
