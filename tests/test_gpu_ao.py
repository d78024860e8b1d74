"""The ambient-occlusion pass (rtx_ao, k_ao in csrc/rtx_occlusion.h) on 64 x 36
frames at 16 samples: the fused kernel against its own sample rays (rtx_internal_ao_rays, the
device function the kernel calls) traced through rtx_occluded, bit for bit; the rays' geometry and
the moments of a cosine-weighted hemisphere; subsets, seeds and the command line."""
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG, scene_path

pytestmark = pytest.mark.gpu
SAMPLES = 16
W, H = 64, 36
# scene -> camera preset and overrides (64 x 36 frames), AO radius
FRAMES = {
    "cornell": ("cornell_wide", dict(aspect=16.0 / 9.0), 4.0),  # (wide enough to see past the box: some pixels miss)
    "three": ("c1_three", {}, 0.75),
    "bunny": ("c3_bunny", {}, 1.5),
}
_frames = {}


def frame(rtx, name):
    """(device scene, camera, radius, first-hit normal and depth), made once per scene."""
    if name not in _frames:
        preset, over, radius = FRAMES[name]
        dev = rtx.DeviceScene(rtx.HostScene.load(scene_path(name)))
        cam = rtx.camera(rtx.camera_config(preset, width=W, **over))
        assert (cam.image_width, cam.image_height) == (W, H)
        _, normal, depth = dev.aov(cam)
        _frames[name] = (dev, cam, radius, normal, depth)
    return _frames[name]


@pytest.mark.parametrize("precision", ["parity", "fast"])
@pytest.mark.parametrize("name", list(FRAMES))
def test_ao_equals_its_rays_through_occluded(rtx_mod, gpu, name, precision):
    rtx = rtx_mod
    dev, cam, radius, normal, depth = frame(rtx, name)
    npix = W * H
    ao = dev.ao(cam, samples=SAMPLES, radius=radius, seed=77, precision=precision)
    rays = rtx.ao_rays(dev, cam, samples=SAMPLES, radius=radius, seed=77, precision=precision)
    assert ao.shape == (npix,) and rays.shape == (npix, SAMPLES, 6)
    occ = dev.occluded(rays.reshape(-1, 6), tmin=rtx.RTX_SEAM_TMIN, tmax=radius, precision=precision)
    want = 1.0 - occ.reshape(npix, SAMPLES).mean(1)
    assert ao.tobytes() == want.tobytes(), int((ao != want).sum())
    assert (ao < 1.0).any() and (ao == 1.0).any(), "some pixels must be occluded, some open"
    if True:
        _, normal, depth = dev.aov(cam, precision=precision)  # the first hits of the same walk
        miss = depth == 0
        assert 0 < miss.sum() < npix
        assert (ao[miss] == 1.0).all() and not rays[miss].any()
        d, o = rays[~miss][:, :, 3:], rays[~miss][:, :, :3]
        n = normal[~miss][:, None, :]
        assert np.abs(np.linalg.norm(d, axis=2) - 1.0).max() <= 1e-12
        cos = (d * n).sum(2)
        assert cos.min() >= 0.0
        assert (o == o[:, :1, :]).all(), "a pixel's rays share its hit point"
        # moments of a cosine-weighted hemisphere: E cos = 2/3, Var cos = 1/2 - 4/9 = 1/18
        count = cos.size
        sigma = np.sqrt((1.0 / 18.0) / count)
        print(name, "mean cos %.5f over %d rays, sigma %.2e" % (cos.mean(), count, sigma))
        assert abs(cos.mean() - 2.0 / 3.0) <= 5.0 * sigma


@pytest.mark.parametrize("name", list(FRAMES))
def test_subsets_seeds_and_repeats(rtx_mod, gpu, name):
    rtx = rtx_mod
    dev, cam, radius, _, _ = frame(rtx, name)
    for precision in ("parity", "fast"):
        kw = dict(samples=SAMPLES, radius=radius, precision=precision)
        whole = dev.ao(cam, seed=5, **kw).reshape(H, W)
        x0, y0, w, h = 19, 7, 33, 17
        tile = dev.ao(cam, seed=5, tile=(x0, y0, w, h), **kw)
        assert tile.tobytes() == np.ascontiguousarray(whole[y0:y0 + h, x0:x0 + w]).tobytes()
        rows = rtx.stripe_rows_of(H, 5, 1, 3, W)
        stripe = dev.ao(cam, seed=5, stripes=(5, 1, 3), **kw)
        assert stripe.tobytes() == np.ascontiguousarray(whole[rows]).tobytes()
        assert dev.ao(cam, seed=5, **kw).tobytes() == whole.tobytes()
        other = dev.ao(cam, seed=6, **kw).reshape(H, W)
        assert (other != whole).any()


def test_command_line_ao_pass(rtx_mod, gpu):
    exe = os.path.join(PKG, "raytracer")
    cams = os.path.join(os.path.dirname(PKG), "configs", "cameras.json")
    r = subprocess.run([exe, "c1_three", "--scene", scene_path("three"), "--cameras", cams, "--ao", "8,0.75"],
                       capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    tok = r.stdout.split()
    assert tok[0] == b"P3" and tok[3] == b"255"
    w, h = int(tok[1]), int(tok[2])
    cam = rtx_mod.camera(rtx_mod.camera_config("c1_three"))
    assert (w, h) == (cam.image_width, cam.image_height)
    px = np.array(tok[4:], dtype=np.int64).reshape(h * w, 3)
    assert (px[:, 0] == px[:, 1]).all() and (px[:, 1] == px[:, 2]).all()
    assert px.min() >= 0 and px.max() <= 255 and len(np.unique(px[:, 0])) > 2
    # the default radius: a quarter of the scene's bounding-box diagonal
    r2 = subprocess.run([exe, "c1_three", "--scene", scene_path("three"), "--cameras", cams, "--ao", "4"],
                        capture_output=True, timeout=120)
    assert r2.returncode == 0 and r2.stdout.startswith(b"P3"), r2.stderr.decode()
    assert b"AO: 4 samples, radius" in r2.stderr
    bad = subprocess.run([exe, "c1_three", "--ao", "0"], capture_output=True, timeout=120)
    assert bad.returncode == 2
