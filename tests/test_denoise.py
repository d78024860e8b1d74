"""First-hit AOVs (rtx_aov) and the edge-avoiding a-trous denoiser (rtx_denoise, rtx_film_denoise).

AOVs are compared bit for bit: depth and normal against DeviceScene.intersect of the pixel-centre
rays built here in numpy (an entry point pinned to the reference's records, test_gpu_parity.py),
albedo against a numpy restatement from the host scene's material and texture tables.  The filter
is compared against a float64 numpy restatement of DESIGN.md section 4b written below
(atrous_ref); the films against rtx.denoise of their own resolved frame.
"""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT, scene_path

LUM = (0.2126, 0.7152, 0.0722)
FLOOR = 1e-3

# ---- host, no GPU -------------------------------------------------------------------------------


def test_default_parameters(rtx_mod):
    p = rtx_mod.denoise_params()
    assert (p.iterations, p.flags, p.normal_power, p.sigma_depth, p.sigma_color) == (5, 1, 64.0, 0.05, 4.0)
    assert rtx_mod.RTX_DENOISE_DEMODULATE == 1
    q = rtx_mod.denoise_params(iterations=3, demodulate=False, sigma_color=2.0)
    assert (q.iterations, q.flags, q.sigma_color, q.sigma_depth) == (3, 0, 2.0, 0.05)
    with pytest.raises(TypeError):
        rtx_mod.denoise_params(sigma=1.0)
    assert C.sizeof(rtx_mod.DenoiseParams) == 32


def test_null_arguments_are_refused_with_a_message(rtx_mod):
    L = rtx_mod.lib()
    cam = rtx_mod.camera(rtx_mod.camera_config("c1_three", width=8))
    prm, dp = rtx_mod.RenderParams(), rtx_mod.denoise_params()
    buf = np.zeros(8 * 4 * 3)
    b = buf.ctypes.data_as(C.c_void_p)
    size = C.c_size_t()
    calls = {
        "rtx_denoise_params_default": lambda: L.rtx_denoise_params_default(None),
        "rtx_aov": lambda: L.rtx_aov(None, C.byref(cam), C.byref(prm), b, b, b),
        "rtx_aov_device": lambda: L.rtx_aov_device(None, C.byref(cam), C.byref(prm), b, b, b, None),
        "rtx_denoise": lambda: L.rtx_denoise(None, 8, 4, b, b, b, b, None, C.byref(dp), b),
        "rtx_denoise_device": lambda: L.rtx_denoise_device(None, 8, 4, b, b, b, b, None, C.byref(dp), b, None),
        "rtx_film_denoise": lambda: L.rtx_film_denoise(None, C.byref(dp), b),
        "rtx_film_denoise_p3": lambda: L.rtx_film_denoise_p3(None, C.byref(dp), b, 16, C.byref(size)),
    }
    assert set(calls) <= set(rtx_mod.EXPORTS)
    for name, call in calls.items():
        assert call() == -1, name  # RTX_ERR_INVALID
        assert b"NULL" in L.rtx_last_error(), (name, L.rtx_last_error())


def test_names_exist(rtx_mod):
    assert callable(rtx_mod.denoise) and callable(rtx_mod.DeviceScene.aov)
    assert callable(rtx_mod.Film.denoise) and callable(rtx_mod.Film.denoise_p3)


# ---- the float64 restatement of the filter ----------------------------------

H5 = np.array([1, 4, 6, 4, 1]) / 16.0
H3 = np.array([1, 2, 1]) / 4.0


def lum(c):
    return LUM[0] * c[..., 0] + LUM[1] * c[..., 1] + LUM[2] * c[..., 2]


def atrous_ref(rgb, albedo, normal, depth, variance, W, H, iterations=5, normal_power=64.0, sigma_depth=0.05,
               sigma_color=4.0, demodulate=True, step_of=lambda k: 2 ** k):
    """A direct loop over the taps, each tap vectorised over the image, all in float64."""
    c = np.array(rgb, dtype=np.float64).reshape(H, W, 3)
    if iterations == 0:
        return c.reshape(-1, 3)
    a = np.maximum(np.asarray(albedo, dtype=np.float64).reshape(H, W, 3), FLOOR)
    n = np.asarray(normal, dtype=np.float64).reshape(H, W, 3)
    z = np.asarray(depth, dtype=np.float64).reshape(H, W)
    v = np.zeros((H, W)) if variance is None else np.array(variance, dtype=np.float64).reshape(H, W)
    if demodulate:
        c = c / a
    ys, xs = np.mgrid[0:H, 0:W]
    hit = z > 0
    for k in range(iterations):
        s = step_of(k)
        g = np.ones((H, W))
        if variance is not None:  # 3 x 3 Gaussian of var at step 1, taps outside skipped and renormalised
            num, den = np.zeros((H, W)), np.zeros((H, W))
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    qy, qx = ys + dy, xs + dx
                    ok = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                    w = np.where(ok, H3[dy + 1] * H3[dx + 1], 0.0)
                    num += w * v[np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)]
                    den += w
            g = np.sqrt(np.maximum(0.0, num / den))
        lp = lum(c)
        sc, sw, sv = np.zeros((H, W, 3)), np.zeros((H, W)), np.zeros((H, W))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                qy, qx = ys + dy * s, xs + dx * s
                ok = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                qy, qx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                cq, nq, zq, hq = c[qy, qx], n[qy, qx], z[qy, qx], hit[qy, qx]
                hh = H5[dy + 2] * H5[dx + 2]
                if dx == 0 and dy == 0:
                    w = np.full((H, W), hh)
                else:
                    both = hit & hq
                    with np.errstate(divide="ignore", invalid="ignore"):
                        wn = np.where(both, np.maximum(0.0, (n * nq).sum(-1)) ** normal_power, 1.0)
                        wz = np.where(both, np.exp(-np.abs(z - zq) / (sigma_depth * np.maximum(z, zq))), 1.0)
                    wl = np.exp(-np.abs(lp - lum(cq)) / (sigma_color * g + 1e-6))
                    w = np.where(ok & (hit == hq), hh * wn * wz * wl, 0.0)
                sc += w[..., None] * cq
                sv += w * w * v[qy, qx]
                sw += w
        c, v = sc / sw[..., None], sv / (sw * sw)
    if demodulate:
        c = c * a
    return c.reshape(-1, 3)


def synthetic(W, H, seed=5):
    """A noisy frame over a bumpy surface with a miss region and an object with its own depth."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    gx, gy = 0.25 * np.cos(0.9 * xs + 0.3 * ys), 0.25 * np.sin(0.7 * ys - 0.2 * xs)
    normal = np.stack([gx, gy, np.ones_like(gx)], -1)
    normal /= np.linalg.norm(normal, axis=-1, keepdims=True)
    depth = 5.0 + 0.02 * xs + 0.03 * ys
    obj = (xs - 0.6 * W) ** 2 + (ys - 0.5 * H) ** 2 < (0.22 * H) ** 2
    depth = np.where(obj, 3.0 + 0.01 * xs, depth)
    depth = np.where((xs < 0.15 * W) & (ys < 0.4 * H), 0.0, depth)  # misses
    normal[depth == 0] = 0.0
    albedo = np.where(obj[..., None], (0.8, 0.3, 0.2), 0.25 + 0.7 * rng.random((H, W, 3)))
    albedo[depth == 0] = 1.0
    light = 0.6 + 0.3 * np.sin(0.11 * xs) * np.cos(0.13 * ys)
    sigma = 0.05 + 0.25 * rng.random((H, W))
    rgb = albedo * (light[..., None] + sigma[..., None] * rng.standard_normal((H, W, 3)))
    variance = sigma ** 2 * (0.5 + rng.random((H, W)))
    return (rgb.reshape(-1, 3), albedo.reshape(-1, 3), normal.reshape(-1, 3), depth.ravel(), variance.ravel())


# ---- GPU: AOVs -----------------------------------------------------------------------------------

TEXTURED = """rtxscene 1
bvh 1
tex 0 image earthmap
mat 0 lambertian 0
tex 1 solid 0.72999999999999998 0.72999999999999998 0.72999999999999998
tex 2 solid 0.12 0.45000000000000001 0.14999999999999999
tex 3 checker 0.37 1 2
mat 1 lambertian 3
tex 4 solid 15 15 15
mat 2 light 4
mat 3 metal 0.8 0.6 0.2 0.1
mat 4 dielectric 1.5
rect yz 0 10 0 10 10 0
rect yz 0 10 0 10 0 0
rect xz 0 10 0 10 0 1
rect xz 0 10 0 10 10 0
rect xy 0 10 0 10 10 1
rect xy 4 6 6 8 9.9000000000000004 2
sphere 5 2 5 1.5 0
sphere 2 1 8 1 3
sphere 8 1 8 1 4
"""

AOV_SCENES = {  # name -> (camera preset, width)
    "three": ("c1_three", 64), "rects": ("c1_three", 64), "cornell": ("cornell", 64), "final": ("c2_final", 64),
    "bunny": ("c3_bunny", 48), "textured": ("cornell", 64),
}


def centre_rays(cam, xs, ys):
    """origin center, direction ((pixel00 + i du) + j dv) - center, float64, this operation order."""
    c, p00 = np.array(cam.center[:]), np.array(cam.pixel00[:])
    du, dv = np.array(cam.pixel_delta_u[:]), np.array(cam.pixel_delta_v[:])
    i, j = np.asarray(xs, dtype=np.float64)[:, None], np.asarray(ys, dtype=np.float64)[:, None]
    d = ((p00 + (i * du)) + (j * dv)) - c
    return np.concatenate([np.broadcast_to(c, d.shape), d], axis=1)


def frame_rays(cam):
    ys, xs = np.mgrid[0:cam.image_height, 0:cam.image_width]
    return centre_rays(cam, xs.ravel(), ys.ravel())


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def albedo_ref(arrays, hits, orc):
    """The AOV albedo restated from the host scene's tables and the hit records."""
    mats, texs = arrays["materials"], arrays["textures"]
    out = np.ones((len(hits), 3))
    image_cases, image_at = [], []
    for i in np.nonzero(hits["hit"])[0]:
        m = mats[hits["material"][i]]
        if m["kind"] == 1:  # metal
            out[i] = m["albedo"]
        if m["kind"] != 0:  # dielectric, light: ones
            continue
        t, p = texs[m["texture"]], hits["p"][i]
        while t["kind"] == 1:  # checker: the parity of floor(inv_scale p) picks the next texture
            cell = np.floor(t["inv_scale"] * p).astype(np.int64)
            t = texs[t["even"] if int(cell.sum()) % 2 == 0 else t["odd"]]
        if t["kind"] == 0:
            out[i] = t["color"]
        else:
            image_cases.append([1, 1.0, hits["u"][i], hits["v"][i], p[0], p[1], p[2], 0.0])
            image_at.append(i)
    if image_at:
        out[image_at] = orc.texture(np.array(image_cases))
    return out, len(image_at)


@pytest.fixture(scope="module")
def aov_scene(rtx_mod, gpu, tmp_path_factory):
    """(host scene, device scene, camera, file) per scene, and its whole-frame parity AOVs, once."""
    made = {}

    def get(name):
        if name not in made:
            preset, width = AOV_SCENES[name]
            path = scene_path(name)
            if name == "textured":
                path = str(tmp_path_factory.mktemp("dn") / "textured.rtxs")
                open(path, "w").write(TEXTURED)
            host = rtx_mod.HostScene.load(path)
            dev = rtx_mod.DeviceScene(host)
            cam = rtx_mod.camera(rtx_mod.camera_config(preset, width=width))
            aov = dev.aov(cam)
            for a in aov:
                a.setflags(write=False)
            made[name] = (host, dev, cam, path, aov)
        return made[name]

    return get


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(AOV_SCENES))
def test_aov_parity(rtx_mod, orc, aov_scene, name):
    host, dev, cam, path, (albedo, normal, depth) = aov_scene(name)
    rays = frame_rays(cam)
    hits = dev.intersect(rays, precision="parity")
    assert 0 < int(hits["hit"].sum())
    assert np.array_equal(depth > 0, hits["hit"] != 0)
    assert np.array_equal(bits(depth), bits(hits["t"]))
    assert np.array_equal(bits(normal), bits(hits["normal"]))
    want, n_image = albedo_ref(host.arrays(), hits, orc)
    assert np.array_equal(bits(albedo), bits(want))
    if name == "textured":  # every branch of the albedo table is in the frame
        kinds = set(host.arrays()["materials"]["kind"][hits["material"][hits["hit"] != 0]])
        assert kinds == {0, 1, 2, 3} and n_image > 0 and int((hits["hit"] == 0).sum()) == 0
    if name == "three":
        assert int((hits["hit"] == 0).sum()) > 0
        ref = orc.Scene(path).intersect(rays)
        assert np.array_equal(ref[:, 0] != 0, depth > 0)
        assert np.array_equal(bits(ref[:, 1]), bits(depth)) and np.array_equal(bits(ref[:, 5:8]), bits(normal))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["three", "rects", "cornell", "final", "bunny"])
def test_aov_fast_depth_is_the_parity_depth(aov_scene, name):
    _, dev, cam, _, (_, _, depth) = aov_scene(name)
    assert np.array_equal(bits(dev.aov(cam, precision="fast")[2]), bits(depth))


@pytest.mark.gpu
def test_aov_subsets(rtx_mod, gpu):
    dev = rtx_mod.DeviceScene(rtx_mod.HostScene.load(scene_path("three")))
    cam = rtx_mod.camera(rtx_mod.camera_config("c1_three", width=70))
    W, H = cam.image_width, cam.image_height
    assert (W, H) == (70, 39)
    full = [a.reshape(H, W, -1) for a in dev.aov(cam)]
    x0, y0, w, h = 5, 3, 33, 17
    for got, whole in zip(dev.aov(cam, tile=(x0, y0, w, h)), full):
        assert np.array_equal(bits(got.reshape(h, w, -1)), bits(whole[y0:y0 + h, x0:x0 + w]))
    rows = rtx_mod.stripe_rows_of(H, 4, 1, 3, width=W)
    for got, whole in zip(dev.aov(cam, stripes=(4, 1, 3)), full):
        assert np.array_equal(bits(got.reshape(len(rows), W, -1)), bits(whole[rows]))


# ---- GPU: the filter -----------------------------------------------------------------------------

GRIDS = [(70, 37), (3, 2), (1, 1)]


@pytest.fixture(scope="module")
def plain_scene(rtx_mod, gpu):
    return rtx_mod.DeviceScene(rtx_mod.HostScene.load(scene_path("three")))


@pytest.mark.gpu
@pytest.mark.parametrize("W, H", GRIDS)
def test_zero_iterations_copy_the_input(rtx_mod, plain_scene, W, H):
    rgb, albedo, normal, depth, var = synthetic(W, H)
    rgb[0, 0] = 1.0 + 2.0 ** -40  # not a float32 value
    out = rtx_mod.denoise(plain_scene, rgb, albedo, normal, depth, W, H, variance=var, iterations=0)
    assert np.array_equal(bits(out), bits(rgb))


@pytest.mark.gpu
@pytest.mark.parametrize("W, H", GRIDS)
@pytest.mark.parametrize("iterations", [1, 5, 8])
def test_constant_colour_stays_constant(rtx_mod, plain_scene, W, H, iterations):
    """The filter is a convex combination: a constant frame comes back within iterations * 64 *
    2^-24 relative (25 float32 products and sums plus the division per iteration), whatever the
    guides say.  Demodulated, the albedo is constant too (a varying one makes colour / albedo vary)."""
    _, albedo, normal, depth, var = synthetic(W, H)
    const = np.array([0.3, 0.71, 1.9])
    rgb = np.broadcast_to(const, (W * H, 3))
    bound = iterations * 64 * 2.0 ** -24
    for demodulate, alb in ((False, albedo), (True, np.full((W * H, 3), 0.37))):
        for v in (None, var):
            out = rtx_mod.denoise(plain_scene, rgb, alb, normal, depth, W, H, variance=v, iterations=iterations,
                                  demodulate=demodulate)
            rel = np.abs(out / const - 1.0).max()
            print(f"constant {W}x{H} it={iterations} demod={demodulate} var={v is not None}: rel {rel:.3g} bound {bound:.3g}")
            assert rel <= bound


@pytest.mark.gpu
@pytest.mark.parametrize("edge", ["normal", "hit_miss"])
def test_no_leak_across_a_geometric_edge(rtx_mod, plain_scene, edge):
    """Normals +x left and +y right (a dot of exactly 0), or hits left and misses right: the left
    half does not see the right half's colours.  Without a variance: its 3 x 3 pre-filter is not
    edge-aware by definition, so g_p next to the edge would carry the other side's filtered variance."""
    W, H = 70, 37
    rgb, albedo, _, _, _ = synthetic(W, H)
    left = (np.mgrid[0:H, 0:W][1] < W // 2).ravel()
    normal = np.where(left[:, None], (1.0, 0.0, 0.0), (0.0, 1.0, 0.0))
    depth = np.full(W * H, 4.0)
    if edge == "hit_miss":
        normal = np.where(left[:, None], (1.0, 0.0, 0.0), (0.0, 0.0, 0.0))
        depth = np.where(left, 4.0, 0.0)
    other = rgb.copy()
    other[~left] = np.random.default_rng(9).random((int((~left).sum()), 3)) * 3.0
    a = rtx_mod.denoise(plain_scene, rgb, albedo, normal, depth, W, H)
    b = rtx_mod.denoise(plain_scene, other, albedo, normal, depth, W, H)
    assert np.array_equal(bits(a[left]), bits(b[left]))
    assert not np.array_equal(a[~left], b[~left])
    assert not np.array_equal(a[left], rgb[left])  # and the left half was filtered


# measured on the MI355X: the largest |GPU - atrous_ref| over the four cases below, and 8 x that
MEASURED_MAX_ABS = 7.70027e-07
BOUND = 8 * MEASURED_MAX_ABS  # 6.16e-06


@pytest.mark.gpu
def test_against_the_float64_restatement(rtx_mod, plain_scene):
    """70 x 37 noisy frame, default parameters, with and without variance and demodulation.
    The bound is 8 x the largest absolute difference measured on the MI355X (the margin covers
    exp / log differences between ROCm releases); the restatement with one defect (step k + 1
    instead of 2^k; normal_power halved) must miss the GPU output by at least 10 x the bound.
    Measured: largest difference 7.70e-07 (per case 6.02e-07, 7.70e-07, 7.29e-07, 7.63e-07), so the
    bound is 6.16e-06; the defective restatements differ by 0.066 .. 0.167."""
    W, H = 70, 37
    rgb, albedo, normal, depth, var = synthetic(W, H)
    worst, defects = 0.0, []
    for v in (None, var):
        for demodulate in (False, True):
            got = rtx_mod.denoise(plain_scene, rgb, albedo, normal, depth, W, H, variance=v, demodulate=demodulate)
            want = atrous_ref(rgb, albedo, normal, depth, v, W, H, demodulate=demodulate)
            diff = np.abs(got - want).max()
            step = np.abs(got - atrous_ref(rgb, albedo, normal, depth, v, W, H, demodulate=demodulate,
                                           step_of=lambda k: k + 1)).max()
            power = np.abs(got - atrous_ref(rgb, albedo, normal, depth, v, W, H, demodulate=demodulate,
                                            normal_power=32.0)).max()
            print(f"restatement var={v is not None} demod={demodulate}: max abs {diff:.4g}; wrong step {step:.4g}; "
                  f"halved power {power:.4g}")
            worst = max(worst, diff)
            defects += [step, power]
    print(f"restatement: worst {worst:.6g}, smallest defect {min(defects):.6g}")
    assert worst <= BOUND
    assert min(defects) >= 10 * BOUND


@pytest.mark.gpu
def test_host_and_device_entry_points_agree(rtx_mod, plain_scene):
    import torch

    W, H = 70, 37
    rgb, albedo, normal, depth, var = synthetic(W, H)
    want = rtx_mod.denoise(plain_scene, rgb, albedo, normal, depth, W, H, variance=var)
    dev = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (rgb, albedo, normal, depth, var)]
    out = torch.empty((W * H, 3), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    p = rtx_mod.denoise_params()
    rc = rtx_mod.lib().rtx_denoise_device(plain_scene.h, W, H, *[C.c_void_p(t.data_ptr()) for t in dev], C.byref(p),
                                          C.c_void_p(out.data_ptr()), C.c_void_p(s.cuda_stream))
    assert rc == 0, rtx_mod.lib().rtx_last_error()
    s.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), bits(want))


@pytest.mark.gpu
def test_bad_parameters_are_refused(rtx_mod, plain_scene):
    rgb, albedo, normal, depth, _ = synthetic(3, 2)
    for bad in (dict(iterations=9), dict(iterations=-1), dict(sigma_color=0.0), dict(sigma_depth=-1.0),
                dict(normal_power=0.0), dict(normal_power=float("nan")), dict(flags=2)):
        with pytest.raises(rtx_mod.RtxError, match="denoise"):
            rtx_mod.denoise(plain_scene, rgb, albedo, normal, depth, 3, 2, **bad)
    big = np.zeros(1)
    p = rtx_mod.denoise_params()
    ptr = big.ctypes.data_as(C.c_void_p)
    assert rtx_mod.lib().rtx_denoise(plain_scene.h, 65536, 32768, ptr, ptr, ptr, ptr, None, C.byref(p), ptr) == -1
    assert b"2^31" in rtx_mod.lib().rtx_last_error()


# ---- GPU: films ----------------------------------------------------------------------------------

FILM_SCENES = {"three": ("c1_three", 64, 4), "cornell": ("cornell", 48, 20)}  # preset, width, depth
HEADER_BYTES = 104


@pytest.fixture(scope="module")
def film_scene(rtx_mod, gpu):
    made = {}

    def get(name):
        if name not in made:
            preset, width, depth = FILM_SCENES[name]
            dev = rtx_mod.DeviceScene(rtx_mod.HostScene.load(scene_path(name)))
            cam = rtx_mod.camera(rtx_mod.camera_config(preset, width=width))
            made[name] = (dev, cam, depth, dev.aov(cam))
        return made[name]

    return get


def blob_variance(blob, npix, albedo, demodulate=True):
    """Section 3's variance of an adaptive film's estimate from its saved state (header,
    then sum, mean, m2 as 3 x npix float64 channel-major, samples npix int32, conv npix uint8)."""
    body = np.frombuffer(blob, dtype=np.uint8)[HEADER_BYTES:]
    f64 = body[:9 * npix * 8].view(np.float64)
    m2 = f64[6 * npix:9 * npix].reshape(3, npix)
    n = body[9 * npix * 8:9 * npix * 8 + 4 * npix].view(np.int32).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        vc = np.where(n >= 2, (m2 / (n - 1)) / n, 0.0)
    v = ((LUM[0] * LUM[0]) * vc[0] + (LUM[1] * LUM[1]) * vc[1]) + (LUM[2] * LUM[2]) * vc[2]
    if demodulate:  # by the film's float32 albedo record
        a = np.maximum(albedo.astype(np.float32), np.float32(FLOOR)).astype(np.float64)
        l = (LUM[0] * a[:, 0] + LUM[1] * a[:, 1]) + LUM[2] * a[:, 2]
        v = v / (l * l)
    return v


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FILM_SCENES))
@pytest.mark.parametrize("adaptive", [False, True])
def test_film_denoise_is_denoise_of_its_frame(rtx_mod, film_scene, name, adaptive):
    dev, cam, depth, aov = film_scene(name)
    W, H = cam.image_width, cam.image_height
    assert (W, H) == {"three": (64, 36), "cornell": (48, 32)}[name]
    kw = dict(seed=7, adaptive=adaptive, mode="persistent", precision="parity")
    film = dev.film(cam, depth, **kw)
    bytes_before = rtx_mod.lib().rtx_film_state_bytes(film.h)
    for budget in (4, 16):
        film.render(budget)
        rgb, spp = film.resolve()
        state, p3 = film.save(), film.p3()
        for over in (dict(), dict(demodulate=False, iterations=3)):
            v = None
            if adaptive:
                v = blob_variance(state, film.npix, aov[0], over.get("demodulate", True))
                assert v.max() > 0
            want = rtx_mod.denoise(dev, rgb, *aov, W, H, variance=v, **over)
            got = film.denoise(**over)
            assert np.array_equal(bits(got), bits(want)), (budget, over)
            assert not np.array_equal(got, rgb)
        assert film.denoise_p3() == rtx_mod.encode_p3(dev, film.denoise(), W, H)
        # the film itself is what it was
        again_rgb, again_spp = film.resolve()
        assert np.array_equal(bits(again_rgb), bits(rgb)) and np.array_equal(again_spp, spp)
        assert film.save() == state and film.p3() == p3
        assert rtx_mod.lib().rtx_film_state_bytes(film.h) == bytes_before == len(state)
    fresh = dev.film(cam, depth, **kw)
    fresh.render(16)
    assert np.array_equal(bits(fresh.denoise()), bits(film.denoise()))
    film.close(), fresh.close()


@pytest.mark.gpu
def test_film_refusals_and_tiles(rtx_mod, film_scene):
    dev, cam, depth, aov = film_scene("three")
    W, H = cam.image_width, cam.image_height
    stripes = dev.film(cam, depth, adaptive=False, stripes=(4, 1, 3))
    stripes.render(2)
    with pytest.raises(rtx_mod.RtxError, match="stripes are not adjacent rows"):
        stripes.denoise()
    with pytest.raises(rtx_mod.RtxError, match="stripes are not adjacent rows"):
        stripes.denoise_p3()
    stripes.close()
    x0, y0, w, h = 5, 3, 33, 17
    tile = dev.film(cam, depth, seed=3, adaptive=False, tile=(x0, y0, w, h))
    tile.render(4)
    cut = [a.reshape(H, W, -1)[y0:y0 + h, x0:x0 + w].reshape(w * h, -1) for a in aov]
    want = rtx_mod.denoise(dev, tile.resolve()[0], *cut, w, h)
    assert np.array_equal(bits(tile.denoise()), bits(want))
    assert tile.denoise_p3().startswith(b"P3\n33 17\n255\n")
    tile.close()
    # a film whose scene is gone
    gone = rtx_mod.DeviceScene(rtx_mod.HostScene.load(scene_path("three")))
    film = gone.film(cam, depth, adaptive=False)
    film.render(2)
    film.denoise()
    rtx_mod.lib().rtx_scene_destroy(gone.h)
    gone.h = None
    with pytest.raises(rtx_mod.RtxError, match="scene was destroyed"):
        film.denoise()
    with pytest.raises(rtx_mod.RtxError, match="scene was destroyed"):
        film.denoise_p3()
    film.close()


@pytest.mark.gpu
def test_denoised_frame_is_closer_to_the_converged_one(rtx_mod, film_scene):
    dev, cam, depth, _ = film_scene("cornell")
    tile = (0, 2, 48, 27)
    kw = dict(seed=11, adaptive=False, mode="persistent", precision="parity", tile=tile)
    truth, _, _ = dev.render(cam, 1024, depth, **dict(kw, seed=12))
    film = dev.film(cam, depth, **kw)
    film.render(16)
    raw, clean = film.resolve()[0], film.denoise()
    film.close()
    rms = lambda a: float(np.sqrt(np.mean((a - truth) ** 2)))
    print(f"cornell 48x27 at 16 spp: rms raw {rms(raw):.4g}, denoised {rms(clean):.4g}")
    assert rms(clean) < rms(raw)


# ---- GPU: the CLI --------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("fixed", [True, False])
def test_cli_denoise(rtx_mod, gpu, tmp_path, fixed):
    cams = json.load(open(os.path.join(ROOT, "configs", "cameras.json")))
    cams["c1_three"]["imageWidth"] = 32
    cam_file = tmp_path / "cameras.json"
    cam_file.write_text(json.dumps(cams))
    base = [os.path.join(PKG, "raytracer"), "c1_three", "--scene", "three", "--cameras", str(cam_file), "--depth", "4",
            "--seed", "77", "--spp", "16"] + (["--fixed"] if fixed else [])

    def run(*args):  # each run: a fresh child process under its own time limit
        out = subprocess.run(base + list(args), capture_output=True, timeout=120)
        assert out.returncode == 0, out.stderr.decode()
        return out.stdout

    dev = rtx_mod.DeviceScene(rtx_mod.HostScene.recipe("three", 1234))
    cam = rtx_mod.camera(rtx_mod.camera_config("c1_three", cameras=str(cam_file)))
    kw = dict(seed=77, adaptive=not fixed, mode="persistent", precision="parity")
    plain = run()
    assert plain == dev.render_p3(cam, 16, 4, **kw)[0]  # the bytes of the run without the option
    clean = run("--denoise")
    head = b"P3\n32 18\n255\n"
    assert clean.startswith(head) and clean != plain
    assert len(clean[len(head):].split()) == 32 * 18 * 3
    film = dev.film(cam, 4, **kw)
    film.render(16)
    assert clean == film.denoise_p3()
    prefix = str(tmp_path / "pre")
    assert run("--denoise", "--chunks", "2", "--preview", prefix) == clean
    film6 = dev.film(cam, 4, **kw)
    film6.render(8)
    assert open(prefix + "_8.ppm", "rb").read() == film6.denoise_p3()
    film.close(), film6.close()
