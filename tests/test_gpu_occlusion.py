"""Occlusion (any-hit) queries (rtx_occluded*, csrc/rtx_occlusion.h).

The oracle is the library's own closest hit: for the same scene, rays, interval and precision
occluded[i] == (intersect hit[i] != 0) for EVERY ray, no tolerated exceptions and no tie cases
(the argument is in rtx_occlusion.h).  Each case's rays mix four classes (render-like rays, rays
leaving a surface point, grazing / tangent rays aimed so that t = 1 at the point of contact, and
segments whose far end lies just short of or just past the closest surface), every direction is
target - origin, so the same rays serve the interval (tmin, inf) and the segment interval
(tmin, 1).  The shares asserted per case (SHARES) keep a case from passing on all hits or all
misses; the seeds were chosen with the CPU oracle (tests/oracle_ctypes.py), which alone meets them.
"""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import scene_path

pytestmark = pytest.mark.gpu
INF = float("inf")
N_RAYS = 4096 + 37  # the last block of 256 is partial
SPHERE, TRIANGLE, XY, XZ, YZ = 0, 1, 2, 3, 4
HEAD = ["rtxscene 1", "bvh 1", "tex 0 solid 0.5 0.5 0.5", "mat 0 lambertian 0"]
SMALL = ["sphere -1.5 0.5 0 0.5 0", "sphere 1.25 0.75 0.5 0.75 0"]
MORE = ["sphere 0 2.5 -2 0.5 0", "sphere 3 0.4 2 0.4 0", "sphere -3 1 -3 1 0"]
# inline scenes as in test_gpu_global_spheres.py: lines, and the globals the fast tree leaves out
INLINE = {
    "ground_two": (HEAD + ["sphere 0 -1000 0 1000 0"] + SMALL, None),  # root is a leaf: the flat fast path
    "ground_five": (HEAD + ["sphere 0 -1000 0 1000 0"] + SMALL + MORE, 1),
    "two_globals": (HEAD + ["sphere 0 -1000 0 1000 0", "sphere 0 -1000 0 950 0"] + SMALL + ["sphere 0 2.5 -2 0.5 0"], 2),
    "negative_radius": (HEAD + ["sphere 0 -1000 0 -1000 0"] + SMALL + MORE, 1),  # the generic global test
}
GOLDEN = ["one_sphere", "one_triangle", "rects", "three", "cornell", "bunny"]
SCENES = GOLDEN + list(INLINE)
SEEDS = {name: 11 for name in SCENES}
# (hits at tmax = inf, misses at inf, hits at tmax = 1, misses at 1, hit at inf and miss at 1), minimum shares
SHARES = (0.10, 0.10, 0.10, 0.10, 0.05)


# ---- rays ---------------------------------------------------------------------------------------
def unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def region(rtx, prims):
    """Centre and half-size of the scene's primitives, huge ones (ground spheres) left out."""
    b = rtx.prim_bounds(prims)
    size = (b[:, 3:] - b[:, :3]).max(1)
    keep = size < 100.0 if (size < 100.0).any() else size > -1.0
    lo, hi = b[keep, :3].min(0), b[keep, 3:].max(0)
    return 0.5 * (lo + hi), max(0.5 * float((hi - lo).max()), 0.5)


def free_rays(rng, mid, rad, n):
    """As a render sends them: origins on a shell round the scene or anywhere inside it (bounce
    rays start inside), aimed at points of a box twice the scene's size."""
    shell = mid + unit(rng.normal(size=(n, 3))) * (2.5 * rad)
    inside = mid + rng.uniform(-1.2, 1.2, (n, 3)) * rad
    o = np.where(rng.random((n, 1)) < 0.5, shell, inside)
    t = mid + rng.uniform(-2.0, 2.0, (n, 3)) * rad
    return np.hstack([o, t - o])


def feature_points(rng, prims, o):
    """One point per origin where a ray from it grazes a primitive: the tangent point of a sphere
    as seen from the origin (so that the ray touches it at t = 1), a point of a triangle's edge, a
    point of a rect's border; then moved by 0 or a tiny to small step across the silhouette."""
    n = len(o)
    pick = prims[rng.integers(0, len(prims), n)]
    out = np.zeros((n, 3))
    scale = np.ones(n)
    side = np.zeros((n, 3))
    for i in range(n):
        g, k = pick[i]["g"], int(pick[i]["kind"])
        if k == SPHERE:
            c, r = g[:3], abs(g[3])
            L = c - o[i]
            dist = np.linalg.norm(L)
            e = np.cross(L, rng.normal(size=3))
            e /= np.linalg.norm(e)
            if dist > r > 0:
                s = r / dist
                cth = np.sqrt(1.0 - s * s)
                out[i] = o[i] + (dist * cth) * (cth * L / dist + s * e)
                side[i] = (out[i] - c) / r
            else:
                out[i], side[i] = c + e * r, e
            scale[i] = max(r, 1e-3)
        elif k == TRIANGLE:
            v = g.reshape(3, 3)
            j = int(rng.integers(0, 3))
            a, b = v[j], v[(j + 1) % 3]
            out[i] = a + rng.random() * (b - a)
            side[i] = unit(rng.normal(size=(1, 3)))[0]
            scale[i] = max(float(np.abs(v - v.mean(0)).max()), 1e-6)
        else:
            a0, a1 = {XY: (0, 1), XZ: (0, 2), YZ: (1, 2)}[k]
            ax = 3 - a0 - a1
            p = np.zeros(3)
            u, w = rng.uniform(g[0], g[1]), rng.uniform(g[2], g[3])
            if rng.random() < 0.5:
                u = g[int(rng.integers(0, 2))]
            else:
                w = g[2 + int(rng.integers(0, 2))]
            p[a0], p[a1], p[ax] = u, w, g[4]
            out[i] = p
            side[i] = unit(rng.normal(size=(1, 3)))[0]
            scale[i] = max(abs(g[1] - g[0]), abs(g[3] - g[2]))
    step = rng.choice([0.0, 1e-13, -1e-13, 1e-9, -1e-9, 1e-5, -1e-5, 1e-2, -1e-2], n)
    return out + side * (step * scale)[:, None]


def make_rays(rtx, prims, seed, closest):
    """N_RAYS rays (origin, target - origin) in four classes.  closest(rays) -> (hit flags, t,
    hit points, normals) of a closest-hit query on (RTX_SEAM_TMIN, inf): the parity intersect in
    the tests, the CPU oracle when the seeds were chosen."""
    rng = np.random.default_rng(seed)
    mid, rad = region(rtx, prims)
    n = N_RAYS // 4
    a = free_rays(rng, mid, rad, N_RAYS - 3 * n)
    # leaving a surface point: origins are hit points of the first class
    hit, _, p, nrm = closest(a)
    src = np.nonzero(hit)[0]
    assert len(src) > 0
    src = src[rng.integers(0, len(src), n)]
    d = unit(rng.normal(size=(n, 3)))
    out = nrm[src] + 0.999 * d  # into the hemisphere about the record's normal
    d = np.where(rng.random((n, 1)) < 0.7, out, d)  # the rest anywhere, also into the surface
    b = np.hstack([p[src], d * (rad * rng.uniform(0.2, 3.0, (n, 1)))])
    # grazing and tangent rays
    o = free_rays(rng, mid, rad, n)[:, :3]
    c = np.hstack([o, feature_points(rng, prims, o) - o])
    # segments that end just short of or just past the closest surface (missing rays stay as they are)
    e = free_rays(rng, mid, rad, 16 * n)  # (enough candidates that four in five segments come from hits)
    hit, t, _, _ = closest(e)
    hs, ms = np.nonzero(hit)[0], np.nonzero(~hit)[0]
    nh = min(len(hs), n - n // 5) if len(ms) else n
    take = np.concatenate([hs[:nh], ms[:n - nh]])
    assert len(take) == n
    s = np.where(hit[take], t[take] * rng.choice([1 - 1e-2, 1 - 1e-6, 1 - 1e-12, 1 + 1e-12, 1 + 1e-6, 1 + 1e-2], n), 1.0)
    dseg = np.hstack([e[take, :3], e[take, 3:] * s[:, None]])
    rays = np.ascontiguousarray(np.vstack([a, b, c, dseg]))
    assert rays.shape == (N_RAYS, 6) and np.isfinite(rays).all()
    return rays


def shares(hit_inf, hit_one):
    return (hit_inf.mean(), 1 - hit_inf.mean(), hit_one.mean(), 1 - hit_one.mean(), (hit_inf & ~hit_one).mean())


# ---- scenes -------------------------------------------------------------------------------------
def scene_file(name, tmp):
    if name in GOLDEN:
        return scene_path(name)
    path = str(tmp / (name + ".rtxs"))
    if not os.path.exists(path):
        with open(path, "w") as f:
            f.write("\n".join(INLINE[name][0]) + "\n")
    return path


def gpu_closest(dev):
    def closest(rays):
        h = dev.intersect(rays, precision="parity")
        return h["hit"] != 0, h["t"], h["p"], h["normal"]
    return closest


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("occlusion")


_cases = {}


def case(rtx, tmp, name):
    """(device scene, rays, parity hit flags at tmax = inf and at tmax = 1), made once per scene."""
    if name not in _cases:
        host = rtx.HostScene.load(scene_file(name, tmp))
        if name in INLINE and INLINE[name][1] is not None:
            info, _ = rtx.fast_tree(host)
            assert info["fast_ok"] == 1 and info["n_global"] == INLINE[name][1], info
        dev = rtx.DeviceScene(host)
        rays = make_rays(rtx, host.arrays()["prims"], SEEDS[name], gpu_closest(dev))
        ref = {tmax: dev.intersect(rays, tmax=tmax, precision="parity")["hit"] != 0 for tmax in (INF, 1.0)}
        _cases[name] = (dev, rays, ref)
    return _cases[name]


# ---- equality -----------------------------------------------------------------------------------
@pytest.mark.parametrize("tmax", [INF, 1.0])
@pytest.mark.parametrize("precision", ["parity", "fast"])
@pytest.mark.parametrize("name", SCENES)
def test_occluded_equals_the_hit_flag(rtx_mod, gpu, tmp, name, precision, tmax):
    dev, rays, ref = case(rtx_mod, tmp, name)
    got = shares(ref[INF], ref[1.0])
    print(name, "shares (hit inf, miss inf, hit 1, miss 1, hit inf & miss 1): " + " ".join("%.3f" % v for v in got))
    for have, want in zip(got, SHARES):  # the existing code's flags alone: the case is not vacuous
        assert have >= want, (name, got)
    hit = dev.intersect(rays, tmax=tmax, precision=precision)["hit"] != 0
    occ = dev.occluded(rays, tmax=tmax, precision=precision)
    assert occ.dtype == np.uint8 and occ.shape == (N_RAYS,) and set(np.unique(occ)) <= {0, 1}
    bad = np.nonzero((occ != 0) != hit)[0]
    assert len(bad) == 0, (name, precision, tmax, len(bad), bad[:8], rays[bad[:2]])


def test_one_ray_and_no_ray(rtx_mod, gpu, tmp):
    dev, rays, ref = case(rtx_mod, tmp, "three")
    i, j = int(np.argmax(ref[INF])), int(np.argmin(ref[INF]))
    assert ref[INF][i] and not ref[INF][j]
    for prec in ("parity", "fast"):
        assert dev.occluded(rays[i:i + 1], precision=prec).tolist() == [1]
        assert dev.occluded(rays[j:j + 1], precision=prec).tolist() == [0]
        assert dev.occluded(rays[:0], precision=prec).shape == (0,)
    lib = rtx_mod.lib()
    assert lib.rtx_occluded(dev.h, None, 0, None, 0.001, 1.0, 0) == 0  # n == 0: nothing is read
    assert lib.rtx_occluded_device(dev.h, None, 0, None, 0.001, 1.0, 0, None) == 0
    assert lib.rtx_occluded(dev.h, None, 1, None, 0.001, 1.0, 0) == -1 and b"NULL buffer" in lib.rtx_last_error()
    with pytest.raises(rtx_mod.RtxError, match="tmin"):
        dev.occluded(rays[:4], tmin=1.0, tmax=1.0)


@pytest.mark.parametrize("name", ["bunny", "ground_two"])
def test_device_buffers_equal_host_buffers(rtx_mod, gpu, tmp, name):
    import torch

    dev, rays, _ = case(rtx_mod, tmp, name)
    d_rays = torch.from_numpy(rays).cuda()
    for prec in ("parity", "fast"):
        for tmax in (INF, 1.0):
            d_out = torch.full((N_RAYS + 64,), 7, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            dev.occluded_device(d_rays.data_ptr(), N_RAYS, d_out.data_ptr(), tmax=tmax, precision=prec)
            host = dev.occluded(rays, tmax=tmax, precision=prec)  # same stream: runs after the device call
            out = d_out.cpu().numpy()
            assert np.array_equal(out[:N_RAYS], host), (prec, tmax)
            assert (out[N_RAYS:] == 7).all(), "bytes past n must stay untouched"


# ---- after an in-place update -------------------------------------------------------------------
class ArrayScene:
    """A scene description over numpy arrays (what DeviceScene needs: .desc()), for a scene
    created afresh from moved primitives with the host's refit of the old nodes."""

    def __init__(self, rtx, prims, nodes, mats, texs):
        self.keep = [np.ascontiguousarray(a) for a in (prims, nodes, mats, texs)]
        self.rtx = rtx

    def desc(self):
        rtx = self.rtx
        prims, nodes, mats, texs = self.keep
        d = rtx.SceneDesc()
        d.prims, d.n_prims = C.cast(prims.ctypes.data, C.POINTER(rtx.Prim)), len(prims)
        d.nodes, d.n_nodes = C.cast(nodes.ctypes.data, C.POINTER(rtx.BvhNode)), len(nodes)
        d.materials, d.n_materials = C.cast(mats.ctypes.data, C.POINTER(rtx.Material)), len(mats)
        d.textures, d.n_textures = C.cast(texs.ctypes.data, C.POINTER(rtx.Texture)), len(texs)
        return d


def moved(prims, first, count):
    """Primitives [first, first + count) displaced (each by its own offset, so boxes change shape),
    kinds and materials kept."""
    out = prims.copy()
    rng = np.random.default_rng(5)
    for i in range(first, first + count):
        off = np.array([0.4, 0.25, -0.3]) + rng.uniform(-0.1, 0.1, 3)
        g = out[i]["g"]
        if out[i]["kind"] == SPHERE:
            if abs(g[3]) > 100:
                off = np.array([0.0, -0.25, 0.0])  # the ground sinks
            g[:3] += off
        elif out[i]["kind"] == TRIANGLE:
            g[:] = (g.reshape(3, 3) + off).ravel()
    return out


@pytest.mark.parametrize("name,first,count", [("ground_five", 0, 6), ("bunny", 1000, 400)])
def test_occlusion_after_update_prims(rtx_mod, gpu, tmp, name, first, count):
    rtx = rtx_mod
    host = rtx.HostScene.load(scene_file(name, tmp))
    arr = host.arrays()
    old = arr["prims"]  # leaf order
    assert first + count <= len(old)
    new = moved(old, first, count)
    fresh = rtx.DeviceScene(ArrayScene(rtx, new, rtx.bvh_refit(arr["nodes"], rtx.prim_bounds(new)), arr["materials"],
                                       arr["textures"]))
    dev = rtx.DeviceScene(host)
    rays = make_rays(rtx, new[first:first + count], 3, gpu_closest(fresh))
    before = {(p, t): dev.occluded(rays, tmax=t, precision=p) for p in ("parity", "fast") for t in (INF, 1.0)}
    dev.update_prims(new[first:first + count], first=first)
    changed = 0
    for (p, t), was in before.items():
        want = fresh.occluded(rays, tmax=t, precision=p)
        got = dev.occluded(rays, tmax=t, precision=p)
        assert np.array_equal(got, want), (p, t, int((got != want).sum()))
        assert np.array_equal(got != 0, dev.intersect(rays, tmax=t, precision=p)["hit"] != 0), (p, t)
        assert 0.05 < got.mean() < 0.95, (p, t, got.mean())
        changed += int((got != was).sum())
    assert changed > 0, "the update must change some ray's answer"
