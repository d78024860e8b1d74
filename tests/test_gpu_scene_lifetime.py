"""A destroyed scene gives its device memory back, whatever it rendered.

One cycle is create, render, destroy on the three-sphere scene: 512 x 512, persistent mode,
adaptive with min_spp 16 and a budget of 17.  With RTX_FLAG_COUNT the first pass reserves a
u16 per slot in the scene's `segs1`, 512 * 512 * 16 * 2 B = 8 MiB, a buffer no plain render
makes: a destroy that forgets it shows as free memory that drops by that much more per cycle
than a plain cycle's.  The bound is half the buffer, from the shape used here.
"""
import pytest

from conftest import scene_path

WIDTH, MIN_SPP, SPP, DEPTH = 512, 16, 17, 8
SEGS1_BYTES = WIDTH * WIDTH * MIN_SPP * 2
BOUND = SEGS1_BYTES // 2


def free_bytes():
    import torch

    return torch.cuda.mem_get_info(0)[0]


@pytest.fixture(scope="module")
def setup(rtx_mod, gpu, tmp_path_factory):
    with open(scene_path("three")) as f:  # the golden file is a flat list: the same spheres under a BVH
        text = f.read().replace("\nbvh 0\n", "\nbvh 1\n", 1)
    path = tmp_path_factory.mktemp("lifetime") / "three_bvh.rtxs"
    path.write_text(text)
    host = rtx_mod.HostScene.load(str(path))
    assert host.desc().n_nodes > 0
    cam = rtx_mod.camera(rtx_mod.camera_config("c1_three", width=WIDTH, aspect=1.0))
    assert (cam.image_width, cam.image_height) == (WIDTH, WIDTH)
    return host, cam


def destroy(rtx, dev):
    rtx._check(rtx.lib().rtx_scene_destroy(dev.h), "rtx_scene_destroy")
    dev.h = None


def render_cycle(rtx, host, cam, count):
    dev = rtx.DeviceScene(host)
    _, spp, _ = dev.render(cam, SPP, DEPTH, adaptive=True, mode="persistent", min_spp=MIN_SPP, count=count)
    assert spp.min() >= MIN_SPP
    destroy(rtx, dev)


def film_cycle(rtx, host, cam):
    dev = rtx.DeviceScene(host)
    film = dev.film(cam, DEPTH, adaptive=True, mode="persistent", min_spp=MIN_SPP)
    film.render(SPP)
    destroy(rtx, dev)
    assert film.samples == SPP
    with pytest.raises(rtx.RtxError, match="scene was destroyed"):
        film.render(SPP + 1)
    with pytest.raises(rtx.RtxError, match="scene was destroyed"):
        film.resolve()
    film.close()


def drop(cycle):
    """Free device memory lost over one cycle, in bytes."""
    before = free_bytes()
    cycle()
    return before - free_bytes()


@pytest.mark.gpu
def test_counting_render_leaves_no_memory_behind(rtx_mod, setup):
    host, cam = setup
    for count in (True, False):  # warm-up: what the runtime keeps after a first cycle of each kind
        render_cycle(rtx_mod, host, cam, count)
    with_flag = drop(lambda: render_cycle(rtx_mod, host, cam, True))
    without = drop(lambda: render_cycle(rtx_mod, host, cam, False))
    print(f"free memory lost per cycle: {with_flag} B with RTX_FLAG_COUNT, {without} B without; bound {BOUND} B")
    assert with_flag - without < BOUND


@pytest.mark.gpu
def test_film_that_outlives_its_scene_leaves_no_memory_behind(rtx_mod, setup):
    host, cam = setup
    film_cycle(rtx_mod, host, cam)
    render_cycle(rtx_mod, host, cam, False)
    with_film = drop(lambda: film_cycle(rtx_mod, host, cam))
    without = drop(lambda: render_cycle(rtx_mod, host, cam, False))
    print(f"free memory lost per cycle: {with_film} B with a film, {without} B without; bound {BOUND} B")
    assert with_film - without < BOUND
