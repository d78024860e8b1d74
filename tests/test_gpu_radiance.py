"""Radiance queries (rtx_radiance*, k_radiance in csrc/rtx_radiance.h) on small
frames: the renderer's own primary rays (rtx_internal_camera_rays) traced through the query give
the wavefront render bit for bit; the in-order accumulate, chunk seams, the RNG keys, the device
entry point, the CPU oracle's per-sample radiances, and live scenes.

`resolve` is the renderer's fixed-spp resolve as k_accumulate_sum computes it: the in-order sum
times 1 / (double)(float)spp (a multiplication by the reciprocal, not a division: the two differ in
the last bit for spp = 3, 5, ...)."""
import numpy as np
import pytest

from conftest import scene_path
from test_gpu_parity import RMS_TOL

pytestmark = pytest.mark.gpu
SEED = 4242
PRECISIONS = ("parity", "fast")
# name -> scene, camera preset, width, spp, depth, camera overrides
CASES = {
    "three": ("three", "c1_three", 32, 4, 10, {}),       # the flat list
    "cornell": ("cornell", "cornell", 24, 4, 10, {}),    # rects and an emitter
    "final": ("final", "c2_final", 32, 3, 50, {}),       # metal, glass and global spheres
    "bunny": ("bunny", "c3_bunny", 40, 3, 20, {}),       # triangles and the fast tree
    "three_lens": ("three", "c1_three", 32, 4, 10, dict(defocus=2.0, focus=3.4)),  # thin-lens rays
}
_scenes, _frames, _samples = {}, {}, {}


def resolve(total, n):
    return total * (1.0 / float(np.float32(n)))


def in_order_sum(L):
    """L[:, k] added for k = 0, 1, ... starting from 0, as the device adds them."""
    total = np.zeros_like(L[:, 0])
    for k in range(L.shape[1]):
        total = total + L[:, k]
    return total


def device_scene(rtx, scene):
    if scene not in _scenes:
        _scenes[scene] = rtx.DeviceScene(rtx.HostScene.load(scene_path(scene)))
    return _scenes[scene]


def frame(rtx, name):
    """(device scene, camera, spp, depth, primary rays (npix, spp, 6), global pixel ids), once per case."""
    if name not in _frames:
        scene, preset, width, spp, depth, over = CASES[name]
        dev = device_scene(rtx, scene)
        cam = rtx.camera(rtx.camera_config(preset, width=width, **over))
        R = rtx.camera_rays(dev, cam, spp, seed=SEED)
        npix = cam.image_width * cam.image_height
        assert R.shape == (npix, spp, 6)
        _frames[name] = (dev, cam, spp, depth, R, np.arange(npix, dtype=np.uint32))
    return _frames[name]


def samples(rtx, name, precision):
    """Per-sample radiance L (npix, spp, 3) and segments (npix, spp) of a case through single-sample
    queries: sample k of every pixel is radiance(R[:, k], spp=1, first_sample=k, ids=pixel).  Made
    once and left unchanged."""
    key = (name, precision)
    if key not in _samples:
        dev, cam, spp, depth, R, ids = frame(rtx, name)
        L, S = np.zeros((len(ids), spp, 3)), np.zeros((len(ids), spp), np.uint32)
        for k in range(spp):
            L[:, k], S[:, k] = dev.radiance(R[:, k], 1, depth, seed=SEED, ids=ids, first_sample=k,
                                            precision=precision, segments=True)
        L.setflags(write=False), S.setflags(write=False)
        _samples[key] = (L, S)
    return _samples[key]


def test_the_lens_case_has_a_lens(rtx_mod, gpu):
    _, cam, _, _, R, _ = frame(rtx_mod, "three_lens")
    assert cam.defocus_angle > 0
    assert len(np.unique(R[:, :, :3].reshape(-1, 3), axis=0)) > 100, "thin-lens rays start all over the lens"
    _, _, _, _, R0, _ = frame(rtx_mod, "three")
    assert len(np.unique(R0[:, :, :3].reshape(-1, 3), axis=0)) == 1, "pinhole rays share the origin"


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(CASES))
def test_equals_the_renderer_bit_for_bit(rtx_mod, gpu, name, precision):
    dev, cam, spp, depth, R, ids = frame(rtx_mod, name)
    L, S = samples(rtx_mod, name, precision)
    got = resolve(in_order_sum(L), spp)
    rgb, _, st = dev.render(cam, spp, depth, seed=SEED, adaptive=False, mode="wavefront", precision=precision)
    differ = int((got != rgb).any(1).sum())
    print(name, precision, "pixels that differ:", differ, "of", len(rgb), "segments", int(S.sum()), st["rays_total"])
    # not vacuous: paths bounce, and the image has content
    assert st["rays_total"] > st["rays_primary"] == len(ids) * spp
    assert len(np.unique(rgb, axis=0)) > len(rgb) // 8
    assert (S > 1).any()
    assert np.array_equal(got, rgb), differ
    assert int(S.sum(dtype=np.uint64)) == st["rays_total"]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_accumulate_is_the_in_order_sum(rtx_mod, gpu, precision):
    dev, cam, _, depth, R, ids = frame(rtx_mod, "final")
    pick = np.linspace(0, len(ids) - 1, 64).astype(np.int64)
    rays, pid = R[pick, 0], ids[pick]
    single = [dev.radiance(rays, 1, depth, seed=SEED, ids=pid, first_sample=k, precision=precision, segments=True)
              for k in range(64)]
    L1 = np.stack([s[0] for s in single], 1)
    S1 = np.stack([s[1] for s in single], 1).astype(np.uint64)
    assert len(np.unique(L1.reshape(-1, 3), axis=0)) > 64
    for spp in (1, 5, 64):
        got, segs = dev.radiance(rays, spp, depth, seed=SEED, ids=pid, precision=precision, segments=True)
        want = resolve(in_order_sum(L1[:, :spp]), spp)
        assert np.array_equal(got, want), (spp, int((got != want).any(1).sum()))
        assert np.array_equal(segs.astype(np.uint64), S1[:, :spp].sum(1)), spp


@pytest.mark.parametrize("precision", PRECISIONS)
def test_chunking_changes_nothing(rtx_mod, gpu, precision):
    rtx = rtx_mod
    dev, cam, _, depth, R, ids = frame(rtx, "bunny")
    pick = np.linspace(0, len(ids) - 1, 200).astype(np.int64)
    rays, pid = R[pick, 0], ids[pick]
    runs = {}
    try:
        for chunk in (64, 7, 3, 0):  # whole rays per chunk; one ray per chunk; less than one ray's samples; default
            rtx.radiance_chunk(chunk)
            runs[chunk] = dev.radiance(rays, 5, depth, seed=SEED, ids=pid, precision=precision, segments=True)
            # the host entry point without ids keys by the ray's index, whatever the chunking
            runs[chunk] += (dev.radiance(rays, 5, depth, seed=SEED, precision=precision),)
    finally:
        rtx.radiance_chunk(0)
    ref = runs[0]
    assert len(np.unique(ref[0], axis=0)) > 50 and ref[1].min() >= 5 and ref[1].max() > 5
    for chunk in (64, 7, 3):
        for a, b in zip(runs[chunk], ref):
            assert np.array_equal(a, b), chunk


def diffuse_pixels(rtx, dev, rays):
    """Rays whose closest hit is a Lambertian surface."""
    hits = dev.intersect(rays)
    kinds = dev.host.arrays()["materials"]["kind"]
    return np.flatnonzero((hits["hit"] != 0) & (kinds[np.maximum(hits["material"], 0)] == 0))


def test_keys(rtx_mod, gpu):
    rtx = rtx_mod
    dev, cam, _, depth, R, ids = frame(rtx, "cornell")
    rays = R[:, 0]
    n = len(rays)
    kw = dict(seed=SEED, precision="parity", segments=True)
    # ids = None is the ray's index
    a = dev.radiance(rays, 2, depth, **kw)
    b = dev.radiance(rays, 2, depth, ids=np.arange(n), **kw)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # rays and ids permuted together: the output permuted
    perm = np.random.default_rng(1).permutation(n)
    c = dev.radiance(rays[perm], 2, depth, ids=np.arange(n)[perm], **kw)
    assert np.array_equal(c[0], a[0][perm]) and np.array_equal(c[1], a[1][perm])
    assert not np.array_equal(c[0], a[0])
    # one diffuse-hitting ray: the same id gives the same value, other ids other values
    d = diffuse_pixels(rtx, dev, rays)
    assert len(d) > n // 2
    ray = rays[d[len(d) // 2]]
    same = dev.radiance(np.stack([ray] * 4), 4, depth, ids=[9, 9, 9, 9], **kw)
    assert (same[0] == same[0][0]).all() and (same[1] == same[1][0]).all()
    other = dev.radiance(np.stack([ray] * 16), 4, depth, ids=np.arange(100, 116), **kw)
    assert len(np.unique(other[0], axis=0)) == 16, "16 ids, 16 different 4-sample estimates"
    # sample ranges recombine: [a, a + b) then [a + b, a + b + c) against [a, a + b + c), through the
    # single samples (x * f32(b) + y * f32(c) is not exact in general)
    s0, nb, nc = 3, 2, 4
    single = [dev.radiance(rays, 1, depth, first_sample=k, **kw) for k in range(s0, s0 + nb + nc)]
    L1 = np.stack([s[0] for s in single], 1)
    S1 = np.stack([s[1] for s in single], 1).astype(np.uint64)
    x = dev.radiance(rays, nb, depth, first_sample=s0, **kw)
    y = dev.radiance(rays, nc, depth, first_sample=s0 + nb, **kw)
    z = dev.radiance(rays, nb + nc, depth, first_sample=s0, **kw)
    assert np.array_equal(x[0], resolve(in_order_sum(L1[:, :nb]), nb))
    assert np.array_equal(y[0], resolve(in_order_sum(L1[:, nb:]), nc))
    assert np.array_equal(z[0], resolve(in_order_sum(L1), nb + nc))
    assert np.array_equal(z[1].astype(np.uint64), x[1].astype(np.uint64) + y[1])
    assert np.array_equal(z[1].astype(np.uint64), S1.sum(1))
    assert not np.array_equal(x[0], a[0]), "samples 3, 4 are not samples 0, 1"


@pytest.mark.parametrize("precision", PRECISIONS)
def test_device_entry_on_a_stream(rtx_mod, gpu, precision):
    import torch

    dev, cam, _, depth, R, ids = frame(rtx_mod, "bunny")
    rays = np.ascontiguousarray(R[:, 1])
    n = len(rays)
    perm = np.random.default_rng(2).permutation(n).astype(np.uint32)
    want, want_segs = dev.radiance(rays, 3, depth, seed=SEED, ids=perm, first_sample=1, precision=precision,
                                   segments=True)
    d_rays = torch.from_numpy(rays).cuda()
    d_ids = torch.from_numpy(perm.view(np.int32)).cuda()
    d_out = torch.full((n + 8, 3), -7.0, dtype=torch.float64, device="cuda")
    d_segs = torch.full((n + 8,), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    args = (d_rays.data_ptr(), n, d_out.data_ptr(), 3, depth)
    kw = dict(seed=SEED, first_sample=1, precision=precision, stream=stream.cuda_stream)
    dev.radiance_device(*args, d_ids=d_ids.data_ptr(), d_segments=d_segs.data_ptr(), **kw)
    stream.synchronize()
    out, segs = d_out.cpu().numpy(), d_segs.cpu().numpy().view(np.uint32)
    assert np.array_equal(out[:n], want) and np.array_equal(segs[:n], want_segs)
    assert (out[n:] == -7.0).all() and (segs[n:] == 77).all()
    # without ids (the ray's index) and without segments
    d_out.fill_(-7.0)
    torch.cuda.synchronize()
    dev.radiance_device(*args, **kw)
    stream.synchronize()
    assert np.array_equal(d_out.cpu().numpy()[:n], dev.radiance(rays, 3, depth, seed=SEED, first_sample=1,
                                                                precision=precision))
    # n == 0: OK, nothing written
    d_out.fill_(-7.0)
    d_segs.fill_(77)
    torch.cuda.synchronize()
    dev.radiance_device(d_rays.data_ptr(), 0, d_out.data_ptr(), 3, depth, d_ids=d_ids.data_ptr(),
                        d_segments=d_segs.data_ptr(), **kw)
    stream.synchronize()
    assert (d_out.cpu().numpy() == -7.0).all() and (d_segs.cpu().numpy() == 77).all()
    out0, segs0 = dev.radiance(np.zeros((0, 6)), 3, depth, segments=True)
    assert out0.shape == (0, 3) and segs0.shape == (0,)


@pytest.mark.parametrize("name", ["cornell", "final"])
def test_against_the_oracle(rtx_mod, orc, gpu, name):
    scene, preset, width, spp, depth, _ = CASES[name]
    L, S = samples(rtx_mod, name, "parity")
    ref_L, ref_S = orc.Scene(scene_path(scene)).render_samples(orc.camera_preset(preset), width, spp, depth, SEED,
                                                               threads=4)
    ref_L, ref_S = ref_L.reshape(L.shape), ref_S.reshape(S.shape)
    rms = float(np.sqrt(np.mean((L - ref_L) ** 2)))
    exact = (L == ref_L).all(2)
    print(name, "rms", rms, "bit-identical samples", exact.mean())
    assert rms <= RMS_TOL, rms
    assert exact.mean() >= 0.95, exact.mean()
    assert np.array_equal(S[exact], ref_S[exact])


def test_live_scene(rtx_mod, gpu, tmp_path):
    rtx = rtx_mod
    _, cam, _, depth, R, ids = frame(rtx, "three")
    rays = R[:, 0]
    host = rtx.HostScene.load(scene_path("three"))
    dev = rtx.DeviceScene(host)
    kw = dict(seed=SEED, ids=ids, segments=True)
    before = dev.radiance(rays, 2, depth, **kw)
    prims = host.arrays()["prims"]
    assert prims[2]["kind"] == 0 and list(prims[2]["g"][:4]) == [1.0, 0.0, -1.0, 0.5]
    moved = prims[2:3].copy()
    moved[0]["g"][:3] = [0.25, 0.5, -1.5]
    dev.update_prims(moved, first=2)
    assert dev.epoch() == 1
    text = open(scene_path("three")).read()
    assert "sphere 1 0 -1 0.5 2\n" in text
    path = tmp_path / "three_moved.rtxs"
    path.write_text(text.replace("sphere 1 0 -1 0.5 2\n", "sphere 0.25 0.5 -1.5 0.5 2\n"))
    fresh = rtx.DeviceScene(rtx.HostScene.load(str(path)))
    for precision in PRECISIONS:
        after = dev.radiance(rays, 2, depth, precision=precision, **kw)
        want = fresh.radiance(rays, 2, depth, precision=precision, **kw)
        assert np.array_equal(after[0], want[0]) and np.array_equal(after[1], want[1])
        assert (after[0] != before[0]).any(1).sum() > 20
