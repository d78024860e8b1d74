"""Next-event estimation (rtx_radiance_nee*, rtx_render_nee*, csrc/rtx_nee.h).

The estimator is pinned from outside: the degenerate cases equal the plain radiance query bit for
bit; on the Cornell box every slot is rebuilt in numpy from the path records of
rtx_internal_nee_trace, the emitter samples of rtx_internal_nee_samples and the public rtx_occluded
and rtx_radiance; the two estimators agree in expectation; and keys, chunk seams, tiles, live
scenes, the device entry points and the command line behave as the other query families do.

`resolve` is k_radiance_sum's last step: the in-order sum times 1 / (double)(float)spp."""
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG, scene_path

pytestmark = pytest.mark.gpu
SEED = 4242
PRECISIONS = ("parity", "fast")
LAMBERTIAN, METAL, DIELECTRIC, LIGHT = 0, 1, 2, 3
CAP = 8  # segments recorded per path by the trace hook (>= the largest max_depth decomposed + 1)
_cache = {}


def resolve(total, n):
    return total * (1.0 / float(np.float64(np.float32(n))))


def scene(rtx, name):
    if name not in _cache:
        host = rtx.HostScene.load(scene_path(name))
        _cache[name] = (rtx.DeviceScene(host), host)
    return _cache[name]


def cornell_rays(rtx):
    """(rays (n, 6), ids (n,)): sample 0's camera rays of the 36-wide Cornell preset with their
    global pixel ids, then rays from the middle of the box at the light, at the three spheres
    (Lambertian, metal, glass), at the floor and a wall, and out of the open front, and one onto
    the metal sphere that reflects into the light, with ids of their own.  Made once and left
    unchanged."""
    if "rays" not in _cache:
        dev, _ = scene(rtx, "cornell")
        cam = rtx.camera(rtx.camera_config("cornell", width=36))
        R = rtx.camera_rays(dev, cam, 1, seed=SEED)[:, 0]
        o = np.array([5.0, 5.0, 5.0])
        targets = [[5, 9.99, 5], [4, 9.99, 6], [3.2, 1, 7], [7, 1, 4], [5, 1, 2.5], [7.2, 1.3, 4.1], [5.1, 1.2, 2.4],
                   [5, 0, 5], [0, 5, 5], [10, 4, 6], [5, 5, -3], [2, 7, -3], [8, 2, -1]]
        aimed = np.array([np.concatenate([o, np.array(t, dtype=np.float64) - o]) for t in targets])
        # ... and one straight down onto the metal sphere near its top, which reflects into the light
        aimed = np.concatenate([aimed, [[6.9, 9.0, 4.0, 0.0, -1.0, 0.0]]])
        rays = np.ascontiguousarray(np.concatenate([R, aimed]))
        ids = np.concatenate([np.arange(len(R)), 100000 + 17 * np.arange(len(aimed))]).astype(np.uint32)
        rays.setflags(write=False), ids.setflags(write=False)
        _cache["rays"] = (rays, ids, cam)
    return _cache["rays"]


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
        a, sa = dev.radiance_nee(R[:, k], 1, 10, **kw)
        b, sb = dev.radiance(R[:, k], 1, 10, **kw)
        assert a.tobytes() == b.tobytes() and np.array_equal(sa, sb)
        assert sb.max() > 1 and len(np.unique(b, axis=0)) > len(b) // 8
    # the frame: a 16 x 9 tile of it equals the fixed-spp wavefront render's
    tile = (7, 4, 16, 9)
    rgb, segs = dev.render_nee(cam, 3, 10, seed=SEED, precision=precision, tile=tile)
    want, _, st = dev.render(cam, 3, 10, seed=SEED, adaptive=False, mode="wavefront", precision=precision, tile=tile)
    assert rgb.shape == (16 * 9, 3) and rgb.tobytes() == want.tobytes()
    assert int(segs.sum(dtype=np.uint64)) == st["rays_total"] > st["rays_primary"] == 16 * 9 * 3


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("max_depth", [0, 1])
def test_no_term_fits_below_depth_two(rtx_mod, gpu, max_depth, precision):
    dev, _ = scene(rtx_mod, "cornell")
    rays, ids, _ = cornell_rays(rtx_mod)
    kw = dict(seed=SEED, ids=ids, first_sample=5, precision=precision, segments=True)
    a, sa = dev.radiance_nee(rays, 2, max_depth, **kw)
    b, sb = dev.radiance(rays, 2, max_depth, **kw)
    assert a.tobytes() == b.tobytes() and np.array_equal(sa, sb)
    # two samples of one segment each at depth 0; at depth 1 a scattered sample has a second one
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


def albedo_of(host, material):
    arr = host.arrays()
    m = arr["materials"][material]
    return np.array(arr["textures"][m["texture"]]["color"] if m["texture"] >= 0 else m["albedo"], dtype=np.float64)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("max_depth", [2, 6])
def test_every_slot_is_its_terms_plus_its_end(rtx_mod, gpu, max_depth, precision):
    rtx = rtx_mod
    dev, host = scene(rtx, "cornell")
    rays, ids, _ = cornell_rays(rtx)
    n, first = len(rays), 5
    kw = dict(seed=SEED, ids=ids, first_sample=first, precision=precision)
    T = rtx.nee_trace(dev, rays, 1, max_depth, SEED, CAP, ids=ids, first_sample=first, precision=precision)
    flags, P, N, Wt = T["flags"][:, 0], T["p"][:, 0], T["n"][:, 0], T["w"][:, 0]
    L_end, closest, shadow = T["L_end"][:, 0], T["closest"][:, 0], T["shadow"][:, 0]
    assert closest.max() <= max_depth + 1 <= CAP
    elig = (flags & rtx.NEE_ELIGIBLE) != 0
    traced = (flags & rtx.NEE_TRACED) != 0
    vis = (flags & rtx.NEE_VISIBLE) != 0
    supp = (flags & rtx.NEE_SUPPRESSED) != 0
    # flags nest, and records past a path's end are empty
    assert not (traced & ~elig).any() and not (vis & ~traced).any()
    reach = np.arange(CAP)[None, :] < closest[:, None]
    assert not flags[~reach].any() and not Wt[~elig].any()
    # each eligible vertex's sample, from the hook on its depth's stream, and its visibility from
    # the public any-hit query on the documented interval
    total = np.zeros((n, 3))
    want_shadow = np.zeros(n, np.int64)
    for d in range(CAP):
        rows = np.flatnonzero(elig[:, d])
        if not len(rows):
            continue
        assert d + 1 < max_depth
        smp = rtx.nee_samples(dev, P[rows, d], N[rows, d], 1, SEED, d, ids=ids[rows], first_sample=first)[:, 0]
        seg, C = smp[:, :6], smp[:, 6:]
        tr = C.any(1)
        assert np.array_equal(tr, traced[rows, d]), d
        assert not smp[~tr].any()
        occ = dev.occluded(seg[tr], rtx.RTX_SEAM_TMIN, rtx.RTX_DIRECT_TMAX, precision=precision) if tr.any() else []
        V = np.zeros(len(rows))
        V[tr] = 1.0 - np.asarray(occ, dtype=np.float64)
        assert np.array_equal(V == 1.0, vis[rows, d]), d
        total[rows] = total[rows] + Wt[rows, d] * (C * V[:, None])
        want_shadow[rows] += tr
    # the plain query of the same keys: the path is its path
    plain, plain_segs = dev.radiance(rays, 1, max_depth, segments=True, **kw)
    got, segs = dev.radiance_nee(rays, 1, max_depth, segments=True, **kw)
    want = resolve(total + L_end, 1)
    print(precision, "depth", max_depth, "eligible", int(elig.sum()), "traced", int(traced.sum()), "visible",
          int(vis.sum()), "suppressed", int(supp.sum()), "differ", int((got != want).any(1).sum()))
    assert got.tobytes() == want.tobytes()
    ended_suppressed = supp.any(1)
    assert L_end[~ended_suppressed].tobytes() == plain[~ended_suppressed].tobytes()
    assert not L_end[ended_suppressed].any() and plain[ended_suppressed].any(1).all()
    assert np.array_equal(closest, plain_segs)
    assert np.array_equal(shadow.astype(np.int64), want_shadow)
    assert np.array_equal(segs.astype(np.int64), closest.astype(np.int64) + want_shadow)
    # suppression: only at a path's last segment, and only right after an eligible vertex
    for i, d in zip(*np.nonzero(supp)):
        assert d == closest[i] - 1 and d >= 1 and elig[i, d - 1]
    # a path that ends on the light below the depth limit is suppressed exactly when a term was
    # eligible at its parent vertex: emission at segment 0 and after a metal or glass vertex stays
    last = closest.astype(np.int64) - 1
    rows = np.arange(n)
    Pl = P[rows, np.minimum(last, CAP - 1)]
    on_light = ((np.abs(Pl[:, 1] - 9.99) < 1e-9) & (Pl[:, 0] >= 3) & (Pl[:, 0] <= 7) & (Pl[:, 2] >= 3)
                & (Pl[:, 2] <= 7) & (last < max_depth))
    assert on_light.any()
    parent_elig = np.where(last >= 1, elig[rows, np.maximum(last - 1, 0)], False)
    assert np.array_equal(ended_suppressed[on_light], parent_elig[on_light])
    assert np.array_equal(ended_suppressed, on_light & parent_elig)
    kept = on_light & ~parent_elig
    print("ends on the light:", int(on_light.sum()), "kept", int(kept.sum()), "of them past segment 0",
          int((kept & (last >= 1)).sum()))
    assert L_end[kept].any(1).all() and (kept & (last >= 1)).any()
    # depth 0: w is the hit material's albedo (the throughput is 1 there)
    hits = dev.intersect(rays, precision=precision)
    kinds = host.arrays()["materials"]["kind"]
    for i in np.flatnonzero(elig[:, 0]):
        m = int(hits["material"][i])
        assert hits["hit"][i] and kinds[m] == LAMBERTIAN
        assert Wt[i, 0].tobytes() == albedo_of(host, m).tobytes()
    # no term at a metal or glass vertex, nor at a vertex with d + 1 == max_depth
    for kind in (METAL, DIELECTRIC):
        c, r = sphere_of(host, kind)
        on = (np.abs(np.linalg.norm(P - c, axis=2) - r) < 1e-6) & reach
        assert on.any(), kind
        assert not elig[on].any(), kind
    assert not elig[:, max_depth - 1:].any()
    # not vacuous
    assert elig.sum() > n // 2 and 0 < vis.sum() <= traced.sum() <= elig.sum()
    if max_depth > 2:  # (at depth 2 only first hits sample, and the camera sees few shadowed points)
        assert supp.any() and elig[:, 1:].any() and vis.sum() < traced.sum() < elig.sum()
    # emission straight from the camera (segment 0) and after a specular parent is still collected
    assert (L_end[n - 14] == 15.0).all() and closest[n - 14] == 1
    assert kept[n - 1] and last[n - 1] == 1 and L_end[n - 1].all()  # camera -> metal -> light


# ---- the two estimators agree ---------------------------------------------------------------

def test_same_expectation_less_variance(rtx_mod, gpu):
    """One ray straight down onto the open floor point (5, 0, 5) and one onto the wall x = 0, 4096
    single-sample paths each at max_depth 8: per channel the means differ by at most 5 standard
    errors of their difference (the project's margin; the seed is fixed, so the
    outcome is deterministic), and the light-sampling estimator's sample variance is below the
    plain one's."""
    dev, _ = scene(rtx_mod, "cornell")
    N = 4096
    ids = np.arange(N, dtype=np.uint32) + 7
    for target in ([5.0, 0.0, 5.0], [0.0, 5.0, 5.0]):
        o = np.array([5.0, 5.0, 5.0])
        rays = np.tile(np.concatenate([o, np.array(target) - o]), (N, 1))
        a = dev.radiance_nee(rays, 1, 8, seed=SEED, ids=ids)
        b = dev.radiance(rays, 1, 8, seed=SEED, ids=ids)
        ma, mb, va, vb = a.mean(0), b.mean(0), a.var(0, ddof=1), b.var(0, ddof=1)
        bound = 5.0 * np.sqrt(va / N + vb / N)
        print(target, "nee", ma, va, "plain", mb, vb, "|diff|", np.abs(ma - mb), "bound", bound)
        assert (np.abs(ma - mb) <= bound).all()
        assert (va < vb).all()
        assert (ma > 0).all() and (mb > 0).all()


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
            runs[chunk] = dev.radiance_nee(r, 5, 6, ids=pid, **kw) + dev.render_nee(cam, 5, 6, seed=SEED,
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
    a, sa = dev.radiance_nee(r[perm], 5, 6, ids=pid[perm], **kw)
    assert a.tobytes() == ref[0][perm].tobytes() and np.array_equal(sa, ref[1][perm])
    # ... and the key is the id, not the position: without ids the ray's index keys it
    b = dev.radiance_nee(r, 5, 6, ids=np.arange(len(r), dtype=np.uint32), **kw)
    c = dev.radiance_nee(r, 5, 6, **kw)
    assert b[0].tobytes() == c[0].tobytes() and b[0].tobytes() != ref[0].tobytes()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_frame_is_the_query_on_the_camera_rays(rtx_mod, gpu, precision):
    rtx = rtx_mod
    dev, _ = scene(rtx, "cornell")
    cam = rtx.camera(rtx.camera_config("cornell", width=36))
    W, H, spp, depth = cam.image_width, cam.image_height, 3, 6
    rgb, segs = dev.render_nee(cam, spp, depth, seed=SEED, precision=precision)
    assert rgb.shape == (W * H, 3) and segs.shape == (W * H,)
    R = rtx.camera_rays(dev, cam, spp, seed=SEED)
    ids = np.arange(W * H, dtype=np.uint32)
    total, nseg = np.zeros((W * H, 3)), np.zeros(W * H, np.int64)
    for k in range(spp):
        L, s = dev.radiance_nee(R[:, k], 1, depth, seed=SEED, ids=ids, first_sample=k, precision=precision,
                                segments=True)
        total, nseg = total + L, nseg + s
    assert rgb.tobytes() == resolve(total, spp).tobytes() and np.array_equal(segs.astype(np.int64), nseg)
    # it is another image than the plain render's, with the same pixels black or lit
    plain, _, _ = dev.render(cam, spp, depth, seed=SEED, adaptive=False, mode="wavefront", precision=precision)
    assert rgb.tobytes() != plain.tobytes() and np.isfinite(rgb).all() and rgb.min() >= 0.0
    # a tile and stripes of the frame are the whole frame's pixels
    x0, y0, w, h = 5, 3, 17, 7
    t_rgb, t_segs = dev.render_nee(cam, spp, depth, seed=SEED, precision=precision, tile=(x0, y0, w, h))
    sel = (np.arange(y0, y0 + h)[:, None] * W + np.arange(x0, x0 + w)[None, :]).ravel()
    assert t_rgb.tobytes() == rgb[sel].tobytes() and np.array_equal(t_segs, segs[sel])
    s_rgb, s_segs = dev.render_nee(cam, spp, depth, seed=SEED, precision=precision, stripes=(2, 1, 3))
    rows = [y for y in range(H) if (y // 2) % 3 == 1]
    sel = (np.array(rows)[:, None] * W + np.arange(W)[None, :]).ravel()
    assert s_rgb.tobytes() == rgb[sel].tobytes() and np.array_equal(s_segs, segs[sel])


# ---- live scenes ----------------------------------------------------------------------------

def test_live_scene(rtx_mod, gpu, tmp_path):
    """(tests/scene_update_fixture.py holds metals only: no light to move.  As test_gpu_direct.py
    does, the Cornell box's light is moved and compared with a scene made from the new file.)"""
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
    before = dev.radiance_nee(rays, 2, 6, **kw)
    moved = prims[li:li + 1].copy()
    moved[0]["g"][:5] = [1.0, 7.0, 2.0, 8.0, 9.5]
    dev.update_prims(moved, first=li)
    assert dev.emitters() == (1, 36.0)
    for precision in PRECISIONS:
        after = dev.radiance_nee(rays, 2, 6, precision=precision, **kw)
        want = fresh.radiance_nee(rays, 2, 6, precision=precision, **kw)
        assert after[0].tobytes() == want[0].tobytes() and np.array_equal(after[1], want[1])
        assert after[0].tobytes() != before[0].tobytes()
        f_after = dev.render_nee(cam, 2, 6, seed=SEED, precision=precision, tile=(8, 5, 16, 9))
        f_want = fresh.render_nee(cam, 2, 6, seed=SEED, precision=precision, tile=(8, 5, 16, 9))
        assert f_after[0].tobytes() == f_want[0].tobytes() and np.array_equal(f_after[1], f_want[1])


# ---- device entry points --------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
def test_device_entries_on_a_stream(rtx_mod, gpu, precision):
    import torch

    rtx = rtx_mod
    dev, _ = scene(rtx, "cornell")
    rays, ids, cam = cornell_rays(rtx)
    n = len(rays)
    want, want_segs = dev.radiance_nee(rays, 3, 6, seed=SEED, ids=ids, first_sample=1, precision=precision,
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
        dev.radiance_nee_device(d_rays.data_ptr(), n, d_out.data_ptr(), 3, 6, seed=SEED, first_sample=1,
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
    dev.radiance_nee_device(d_rays.data_ptr(), 0, d_out.data_ptr(), 3, 6, seed=SEED, stream=stream.cuda_stream)
    stream.synchronize()
    assert (d_out.cpu().numpy() == -7.0).all()
    # the frame
    tile = (4, 3, 20, 10)
    f_want, f_segs = dev.render_nee(cam, 3, 6, seed=SEED, precision=precision, tile=tile)
    m = len(f_want)
    d_rgb = torch.full((m + 8, 3), -7.0, dtype=torch.float64, device="cuda")
    d_fs = torch.full((m + 8,), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    got = dev.render_nee_device(cam, d_rgb.data_ptr(), 3, 6, seed=SEED, precision=precision, tile=tile,
                                d_segments=d_fs.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    out, segs = d_rgb.cpu().numpy(), d_fs.cpu().numpy().view(np.uint32)
    assert got == m == 200
    assert out[:m].tobytes() == f_want.tobytes() and np.array_equal(segs[:m], f_segs)
    assert (out[m:] == -7.0).all() and (segs[m:] == 77).all()


# ---- the command line -----------------------------------------------------------------------

def test_command_line_nee_frame(rtx_mod, gpu, tmp_path):
    import json

    rtx = rtx_mod
    exe = os.path.join(PKG, "raytracer")
    # a small preset of the Cornell camera in a cameras file of the test's own
    cams = json.load(open(os.path.join(os.path.dirname(PKG), "configs", "cameras.json")))
    small = dict(cams["cornell"], imageWidth=30, samplesPerPixel=3, maxDepth=6)
    path = tmp_path / "cameras.json"
    path.write_text(json.dumps({"default": cams["default"], "small": small}))
    base = [exe, "small", "--scene", scene_path("cornell"), "--cameras", str(path), "--seed", str(SEED)]
    r = subprocess.run(base + ["--nee"], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    dev, _ = scene(rtx, "cornell")
    cam = rtx.camera(rtx.camera_config("small", cameras=str(path)))
    assert (cam.image_width, cam.image_height) == (30, 20)
    rgb, segs = dev.render_nee(cam, 3, 6, seed=SEED)
    assert r.stdout == rtx.encode_p3(dev, rgb, 30, 20)
    tok = r.stdout.split()
    assert tok[:4] == [b"P3", b"30", b"20", b"255"] and len(tok) == 4 + 3 * 600
    line = "nee: 3 spp, 1 emitters, %d segments\n" % int(segs.sum(dtype=np.uint64))
    assert line.encode() in r.stderr, r.stderr.decode()
    # --spp overrides the preset's samples
    r2 = subprocess.run(base + ["--nee", "--spp", "2"], capture_output=True, timeout=120)
    assert r2.returncode == 0 and r2.stdout == rtx.encode_p3(dev, dev.render_nee(cam, 2, 6, seed=SEED)[0], 30, 20)
    # without --nee the output is the plain render's, byte for byte what the library encodes
    plain = subprocess.run(base + ["--fixed", "--mode", "wavefront"], capture_output=True, timeout=120)
    assert plain.returncode == 0, plain.stderr.decode()
    want, _ = dev.render_p3(cam, 3, 6, seed=SEED, adaptive=False, mode="wavefront")
    assert plain.stdout == want and plain.stdout != r.stdout
    assert b"nee:" not in plain.stderr
