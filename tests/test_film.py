"""Films (rtx_film_*, rtx.Film): a frame rendered in steps, resolved on demand, saved and continued.

Every GPU comparison is bit for bit (np.array_equal on the linear framebuffer and on the sample
counts) against the one-shot DeviceScene.render / render_p3 of the same arguments at spp =
the film's budget: entry points that are themselves pinned to the oracle (test_gpu_parity.py).
The expected side is never a film.  The CPU tests check the saved blob's documented layout
(DESIGN.md "Film") through rtx.film_blob_check, which needs no device.
"""
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT, scene_path

# the blob header, field for field (DESIGN.md "Film"; little-endian, 104 bytes)
HEADER = struct.Struct("<8sII2ii4i3iQ4id2iq")
MAGIC = b"RTXFILM\0"


def make_blob(W=4, H=3, adaptive=0, done=0, magic=MAGIC, version=1, sampler=0, body=None):
    npix = W * H
    head = HEADER.pack(magic, version, HEADER.size, W, H, 0, 0, 0, W, H, 0, 0, 0, 7, 5, adaptive, 16, sampler,
                       float(np.float32(0.05)), done, 0, npix)
    if body is None:
        body = bytes(npix * (9 * 8 + 4 + 1 if adaptive else 3 * 8 + 4))
    return head + body


# ---- CPU: the blob check and the names ---------------------------------------------------------

def test_header_is_104_bytes():
    assert HEADER.size == 104


def test_blob_check_accepts_the_documented_layout(rtx_mod):
    rtx_mod.film_blob_check(make_blob())  # header + zero state of a 4 x 3 fixed film
    rtx_mod.film_blob_check(make_blob(done=12))
    rtx_mod.film_blob_check(make_blob(adaptive=1, done=3))


@pytest.mark.parametrize("what, blob", [
    ("magic", make_blob(magic=b"RTXFILE\0")),
    ("version", make_blob(version=2)),
    ("truncated", make_blob()[:-1]),
    ("negative samples done", make_blob(done=-1)),
], ids=["magic", "version", "short_by_one_byte", "negative_done"])
def test_blob_check_rejects(rtx_mod, what, blob):
    with pytest.raises(rtx_mod.RtxError, match=what):
        rtx_mod.film_blob_check(blob)


def test_blob_check_rejects_more(rtx_mod):
    for blob in (b"", make_blob() + b"\0", make_blob(sampler=1, adaptive=1), make_blob(W=0)):
        with pytest.raises(rtx_mod.RtxError):
            rtx_mod.film_blob_check(blob)


def test_film_names_exist_and_fail_loudly_without_a_scene(rtx_mod):
    assert isinstance(rtx_mod.Film, type) and callable(rtx_mod.DeviceScene.film)
    for name in ("render", "resolve", "p3", "save", "load", "close", "samples"):
        assert hasattr(rtx_mod.Film, name), name
    # a DeviceScene that holds no device scene (what a host without a GPU can make at most:
    # DeviceScene(...) itself raises there, test_capi_exports.py): no film comes out of it
    d = rtx_mod.DeviceScene.__new__(rtx_mod.DeviceScene)
    d.h = None
    cam = rtx_mod.camera(rtx_mod.camera_config("c2_final", width=8))
    with pytest.raises(rtx_mod.RtxError):
        d.film(cam, 5)
    if rtx_mod.device_count() == 0:
        with pytest.raises(rtx_mod.RtxError):
            rtx_mod.DeviceScene(rtx_mod.HostScene.load(scene_path("three"))).film(cam, 5)


# ---- GPU ---------------------------------------------------------------------------------------

SCENES = {  # name -> (scene file, camera preset, width, depth)
    "final": ("final", "c2_final", 64, 50),
    "bunny": ("bunny", "c3_bunny", 64, 20),
}
MODES = {  # arguments shared by DeviceScene.render and DeviceScene.film
    "wavefront": dict(mode="wavefront", precision="parity"),
    "park": dict(mode="persistent", precision="fast", schedule="park"),
    "plain": dict(mode="persistent", precision="fast", schedule="plain"),
    "megakernel": dict(mode="megakernel", precision="parity"),
    "persistent": dict(mode="persistent", precision="parity"),
}


@pytest.fixture(scope="module")
def film_scene(rtx_mod, gpu):
    """(DeviceScene, camera, depth) per scene, and the one-shot frames, each rendered once."""
    scenes, shots = {}, {}

    def scene(name):
        if name not in scenes:
            f, preset, width, depth = SCENES[name]
            dev = rtx_mod.DeviceScene(rtx_mod.HostScene.load(scene_path(f)))
            scenes[name] = (dev, rtx_mod.camera(rtx_mod.camera_config(preset, width=width)), depth)
        return scenes[name]

    def one_shot(name, spp, **kw):
        key = (name, spp, tuple(sorted(kw.items())))
        if key not in shots:
            dev, cam, depth = scene(name)
            rgb, n, _ = dev.render(cam, spp, depth, **kw)
            rgb.setflags(write=False), n.setflags(write=False)
            shots[key] = (rgb, n)
        return shots[key]

    scene.one_shot = one_shot
    return scene


def assert_same(film, ref, what):
    rgb, spp = film.resolve()
    assert np.array_equal(spp, ref[1]), what
    assert np.array_equal(rgb, ref[0]), what


@pytest.mark.gpu
@pytest.mark.parametrize("name, mode", [("final", "wavefront"), ("final", "park"), ("final", "plain"),
                                        ("final", "megakernel"), ("bunny", "park")])
def test_fixed_prefixes(film_scene, name, mode):
    dev, cam, depth = film_scene(name)
    kw = dict(seed=7, adaptive=False, **MODES[mode])
    film = dev.film(cam, depth, **kw)
    for b in (1, 6, 8, 16):
        st = film.render(b)
        assert film.samples == b and st["rays_primary"] > 0
        assert_same(film, film_scene.one_shot(name, b, **kw), (name, mode, b))
    film.close()


ADAPT = dict(seed=3, adaptive=True, min_spp=16, rel_threshold=0.05)
ADAPT_SCENE = "final"


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["wavefront", "persistent"])
def test_adaptive_prefixes(film_scene, mode):
    # (the Cornell box at width 24 converges nowhere within 40 samples in the one-shot render, so
    # the final scene at width 64 it is)
    dev, cam, depth = film_scene(ADAPT_SCENE)
    kw = dict(ADAPT, **MODES[mode])
    spp40 = film_scene.one_shot(ADAPT_SCENE, 40, **kw)[1]
    # some pixels converge before 40 samples and some do not: the prefixes cross both
    assert 0 < int((spp40 < 40).sum()) < spp40.size
    film = dev.film(cam, depth, **kw)
    for b in (10, 16, 17, 40):  # below, at and above min_spp; 17 -> 40 resumes with converged pixels
        film.render(b)
        assert_same(film, film_scene.one_shot(ADAPT_SCENE, b, **kw), (mode, b))
    film.close()


@pytest.mark.gpu
@pytest.mark.parametrize("subset", [dict(stripes=(4, 1, 3)), dict(stripes=(5, 1, 2)), dict(tile=(5, 3, 20, 11))])
def test_subsets(rtx_mod, film_scene, subset):
    dev, cam, depth = film_scene("final")
    kw = dict(seed=7, adaptive=True, **MODES["park"])
    W, H = cam.image_width, cam.image_height
    full_rgb, full_spp = film_scene.one_shot("final", 6, **kw)
    full_rgb, full_spp = full_rgb.reshape(H, W, 3), full_spp.reshape(H, W)
    if "stripes" in subset:
        rows = rtx_mod.stripe_rows_of(H, *subset["stripes"], width=W)
        if subset["stripes"] == (5, 1, 2):
            assert H % 5 != 0 and rows[-1] == H - 1  # the short last block is this stripe's
        want = full_rgb[rows].reshape(-1, 3), full_spp[rows].ravel()
    else:
        x0, y0, w, h = subset["tile"]
        want = full_rgb[y0:y0 + h, x0:x0 + w].reshape(-1, 3), full_spp[y0:y0 + h, x0:x0 + w].ravel()
    film = dev.film(cam, depth, **kw, **subset)
    film.render(3)
    film.render(6)
    assert_same(film, want, subset)
    film.close()


@pytest.mark.gpu
def test_two_films_and_a_plain_render_do_not_share_state(rtx_mod, film_scene):
    dev, cam, depth = film_scene("final")
    other_cam = rtx_mod.camera(rtx_mod.camera_config("c2_final", width=40))
    for mode, adaptive in (("park", False), ("persistent", True)):
        kw = dict(adaptive=adaptive, **MODES[mode])
        a, b = dev.film(cam, depth, seed=11, **kw), dev.film(cam, depth, seed=12, **kw)
        for budget_a, budget_b in ((3, 5), (17, 16), (20, 24)):
            a.render(budget_a)
            dev.render(other_cam, 5, depth, seed=99, **kw)  # the scene's own state, another size
            b.render(budget_b)
            dev.render(other_cam, 2, depth, seed=98, adaptive=not adaptive, **MODES[mode])
        assert_same(a, film_scene.one_shot("final", 20, seed=11, **kw), (mode, "a"))
        assert_same(b, film_scene.one_shot("final", 24, seed=12, **kw), (mode, "b"))
        a.close(), b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name, mode, adaptive, first, last", [
    ("final", "park", False, 6, 16),
    (ADAPT_SCENE, "persistent", True, 6, 16),
    (ADAPT_SCENE, "persistent", True, 17, 40),   # the saved state holds converged pixels
    (ADAPT_SCENE, "wavefront", True, 17, 40),
])
def test_save_load(rtx_mod, film_scene, name, mode, adaptive, first, last):
    dev, cam, depth = film_scene(name)
    kw = dict(ADAPT, **MODES[mode]) if adaptive else dict(seed=7, adaptive=False, **MODES[mode])
    film = dev.film(cam, depth, **kw)
    film.render(first)
    blob = film.save()
    film.close()
    rtx_mod.film_blob_check(blob)
    assert HEADER.unpack_from(blob)[-3] == first  # samples done
    film = dev.film(cam, depth, **kw)
    film.load(blob)
    assert film.samples == first
    assert_same(film, film_scene.one_shot(name, first, **kw), "loaded")
    film.render(last)
    assert_same(film, film_scene.one_shot(name, last, **kw), "continued")
    film.close()


@pytest.mark.gpu
def test_load_refuses_a_blob_of_another_film(rtx_mod, film_scene):
    dev, cam, depth = film_scene("final")
    kw = dict(adaptive=False, **MODES["plain"])
    src = dev.film(cam, depth, seed=7, **kw)
    src.render(6)
    blob = src.save()
    src.close()
    narrow = rtx_mod.camera(rtx_mod.camera_config("c2_final", width=48))
    film = dev.film(cam, depth, seed=8, **kw)
    film.render(2)
    with pytest.raises(rtx_mod.RtxError, match="seed"):
        film.load(blob)
    other = dev.film(narrow, depth, seed=7, **kw)
    with pytest.raises(rtx_mod.RtxError, match="image size"):
        other.load(blob)
    other.close()
    with pytest.raises(rtx_mod.RtxError, match="truncated"):
        film.load(blob[:-8])
    with pytest.raises(rtx_mod.RtxError):
        film.load(blob[:50])
    # unchanged and usable
    assert film.samples == 2
    assert_same(film, film_scene.one_shot("final", 2, seed=8, **kw), "after refused loads")
    film.render(16)
    assert_same(film, film_scene.one_shot("final", 16, seed=8, **kw), "after refused loads, continued")
    film.close()


@pytest.mark.gpu
def test_p3(film_scene):
    dev, cam, depth = film_scene("final")
    kw = dict(seed=7, adaptive=True, mode="persistent", precision="parity")
    film = dev.film(cam, depth, **kw)
    film.render(4)
    film.render(18)
    want, _ = dev.render_p3(cam, 18, depth, **kw)
    assert film.p3() == want
    film.close()


@pytest.mark.gpu
def test_refusals_and_no_ops(rtx_mod, film_scene):
    dev, cam, depth = film_scene("final")
    with pytest.raises(rtx_mod.RtxError, match="megakernel"):
        dev.film(cam, depth, adaptive=True, mode="megakernel")
    film = dev.film(cam, depth, seed=7, adaptive=False, **MODES["plain"])
    with pytest.raises(rtx_mod.RtxError, match="budget"):
        film.render(-1)
    assert film.samples == 0
    film.render(6)
    before = film.resolve()
    for b in (6, 3, 0):
        st = film.render(b)
        assert st["rays_total"] == 0 and film.samples == 6
        assert_same(film, before, b)
    film.close()
    with pytest.raises(rtx_mod.RtxError, match="closed"):
        film.render(8)


@pytest.mark.gpu
def test_film_outlives_its_scene_as_an_empty_shell(rtx_mod, gpu):
    dev = rtx_mod.DeviceScene(rtx_mod.HostScene.load(scene_path("three")))
    cam = rtx_mod.camera(rtx_mod.camera_config("c1_three", width=16))
    film = dev.film(cam, 4, adaptive=False)
    film.render(2)
    rtx_mod.lib().rtx_scene_destroy(dev.h)
    dev.h = None
    assert film.samples == 2
    with pytest.raises(rtx_mod.RtxError, match="scene was destroyed"):
        film.render(4)
    with pytest.raises(rtx_mod.RtxError, match="scene was destroyed"):
        film.resolve()
    film.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fixed", [True, False])
def test_cli_chunks_checkpoint_resume(gpu, tmp_path, fixed):
    import json

    cams = json.load(open(os.path.join(ROOT, "configs", "cameras.json")))
    cams["c1_three"]["imageWidth"] = 32
    cam_file = tmp_path / "cameras.json"
    cam_file.write_text(json.dumps(cams))
    base = [os.path.join(PKG, "raytracer"), "c1_three", "--scene", "three", "--cameras", str(cam_file), "--depth", "4",
            "--seed", "77"] + (["--fixed"] if fixed else [])

    def run(*args):  # each run: a fresh child process under its own time limit
        out = subprocess.run(base + list(args), capture_output=True, timeout=120)
        assert out.returncode == 0, out.stderr.decode()
        return out.stdout

    plain = run("--spp", "16")
    assert plain.startswith(b"P3\n32 18\n255\n")
    prefix = str(tmp_path / "pre")
    assert run("--spp", "16", "--chunks", "3", "--preview", prefix) == plain
    assert open(prefix + "_16.ppm", "rb").read() == plain  # budgets ceil(k * 16 / 3): 6, 11, 16
    assert open(prefix + "_6.ppm", "rb").read() == run("--spp", "6")
    assert os.path.exists(prefix + "_11.ppm")
    ck = str(tmp_path / "film.ckpt")
    assert run("--spp", "6", "--checkpoint", ck) == open(prefix + "_6.ppm", "rb").read()
    assert run("--spp", "16", "--resume", ck) == plain
    # a checkpoint of another seed is refused
    bad = subprocess.run(base + ["--spp", "16", "--resume", ck, "--seed", "78"], capture_output=True, timeout=120)
    assert bad.returncode != 0 and b"seed" in bad.stderr
