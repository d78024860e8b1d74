"""Light probes (rtx_probe_sh*, k_probe and k_probe_sum in csrc/rtx_probe.h) at the
cell centres of a 6 x 4 x 2 grid over each scene's bounding box, 8 samples, depth 8: the fused
kernels against their own depth-0 rays (rtx_internal_probe_rays, the device function the kernels
call) traced one sample at a time through rtx_radiance / rtx_radiance_nee / rtx_radiance_mis and
folded in numpy, bit for bit; the rays' geometry and the moments of the uniform sphere; back-faces;
the open sky in closed form; the estimators against each other; keys, chunk seams, non-finite
points, the device entry point, live scenes and the command line."""
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG, scene_path

pytestmark = pytest.mark.gpu
SEED = 4242
SAMPLES, DEPTH = 8, 8
GRID = (6, 4, 2)
PRECISIONS = ("parity", "fast")
ESTIMATORS = (None, "nee", "mis")
SCENES = ("cornell", "three", "bunny")
_grids = {}


def resolve(total, n):
    """k_probe_sum's last step: kFourPi * ((1.0 / (double)(float)n) * sum)."""
    return (4.0 * np.pi) * ((1.0 / float(np.float64(np.float32(n)))) * total)


def basis(rtx, d):
    """The nine basis values at directions d (..., 3) -> (..., 9): rtx.h's order and operations."""
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    k0, k1, k4, k6, k8 = rtx.SH_K0, rtx.SH_K1, rtx.SH_K4, rtx.SH_K6, rtx.SH_K8
    return np.stack([np.full_like(x, k0), k1 * y, k1 * z, k1 * x, k4 * (x * y), k4 * (y * z),
                     k6 * (3.0 * (z * z) - 1.0), k4 * (x * z), k8 * (x * x - y * y)], axis=-1)


def fold(rtx, d, L):
    """d (n, K, 3), L (n, K, 3) -> (n, 9, 3): the products added in sample order from 0."""
    Y = basis(rtx, d)
    total = np.zeros((len(d), 9, 3))
    for k in range(d.shape[1]):
        total = total + Y[:, k, :, None] * L[:, k, None, :]
    return total


def cell_centres(lo, hi, grid):
    """x fastest"""
    iz, iy, ix = np.meshgrid(*(np.arange(g) for g in grid[::-1]), indexing="ij")
    at = np.stack([ix, iy, iz], axis=-1).reshape(-1, 3)
    return lo + (hi - lo) * ((at + 0.5) / np.array(grid, dtype=np.float64))


def probes(rtx, name):
    """(device scene, points, ids) of the 48 probes of a scene, once per scene and left unchanged.
    The ids are explicit and not the probes' indices."""
    if name not in _grids:
        dev = rtx.DeviceScene(rtx.HostScene.load(scene_path(name)))
        box = rtx.prim_bounds(dev.host.arrays()["prims"])
        lo, hi = box[:, :3].min(0), box[:, 3:].max(0)
        P = np.ascontiguousarray(cell_centres(lo, hi, GRID))
        assert P.shape == (48, 3) and np.isfinite(P).all()
        ids = ((np.arange(len(P), dtype=np.uint64) * 2654435761 + 977) % (1 << 32)).astype(np.uint32)
        assert len(np.unique(ids)) == len(ids) and (ids != np.arange(len(P))).all()
        for a in (P, ids):
            a.setflags(write=False)
        _grids[name] = (dev, P, ids)
    return _grids[name]


def query(dev, estimator):
    return {None: dev.radiance, "nee": dev.radiance_nee, "mis": dev.radiance_mis}[estimator]


@pytest.mark.parametrize("first_sample", [0, 5])
@pytest.mark.parametrize("estimator", ESTIMATORS)
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", SCENES)
def test_equals_its_rays_through_the_radiance_queries(rtx_mod, gpu, name, precision, estimator, first_sample):
    rtx = rtx_mod
    dev, P, ids = probes(rtx, name)
    n = len(P)
    rays = rtx.probe_rays(dev, P, SAMPLES, SEED, ids=ids, first_sample=first_sample)
    assert rays.shape == (n, SAMPLES, 6)
    L, S = np.zeros((n, SAMPLES, 3)), np.zeros((n, SAMPLES), np.uint64)
    B = np.zeros((n, SAMPLES), np.uint64)
    for k in range(SAMPLES):
        L[:, k], S[:, k] = query(dev, estimator)(rays[:, k], 1, DEPTH, seed=SEED, ids=ids,
                                                 first_sample=first_sample + k, precision=precision, segments=True)
        hits = dev.intersect(rays[:, k], precision=precision)
        B[:, k] = (hits["hit"] != 0) & (hits["front_face"] == 0)
    want = resolve(fold(rtx, rays[:, :, 3:], L), SAMPLES)
    got, segs, back = dev.probe_sh(P, SAMPLES, DEPTH, seed=SEED, ids=ids, first_sample=first_sample,
                                   precision=precision, estimator=estimator, segments=True, backfaces=True)
    differ = int((got != want).any((1, 2)).sum())
    print(name, precision, estimator, first_sample, "probes", n, "that differ:", differ, "segments", int(S.sum()),
          "back-faces", int(B.sum()), "c0 range", got[:, 0].min(), got[:, 0].max())
    assert got.shape == (n, 9, 3) and segs.shape == (n,) and segs.dtype == np.uint32 and back.dtype == np.uint32
    assert got.tobytes() == want.tobytes(), differ
    assert np.array_equal(segs.astype(np.uint64), S.sum(1))
    assert np.array_equal(back.astype(np.uint64), B.sum(1))
    assert np.isfinite(got).all() and (got[:, 0] >= 0.0).all()
    assert len(np.unique(got.reshape(n, -1), axis=0)) > n // 2, "not all values are equal"
    assert (S > 1).any(), "paths bounce"
    assert segs.min() >= SAMPLES and back.max() <= SAMPLES


@pytest.mark.parametrize("name", SCENES)
def test_ray_geometry(rtx_mod, gpu, name):
    rtx = rtx_mod
    dev, P, ids = probes(rtx, name)
    rays = rtx.probe_rays(dev, P, SAMPLES, SEED, ids=ids)
    o, d = rays[:, :, :3], rays[:, :, 3:]
    assert o.tobytes() == np.ascontiguousarray(np.broadcast_to(P[:, None, :], o.shape)).tobytes()
    assert np.abs((d * d).sum(2) - 1.0).max() <= 1e-12
    assert len(np.unique(d.reshape(-1, 3), axis=0)) == d.size // 3, "every sample has a direction of its own"
    # 4096 directions of one probe against the uniform sphere: E d = 0 with Var d_i = 1/3;
    # E d_i^2 = 1/3 with Var d_i^2 = 1/5 - 1/9 = 4/45; E d_i d_j = 0 with Var = E d_i^2 d_j^2 = 1/15
    count = 4096
    dd = rtx.probe_rays(dev, P[:1], count, SEED, ids=ids[:1])[0, :, 3:]
    m1, m2 = dd.mean(0), (dd[:, :, None] * dd[:, None, :]).mean(0)
    s1, s2d, s2o = np.sqrt((1.0 / 3.0) / count), np.sqrt((4.0 / 45.0) / count), np.sqrt((1.0 / 15.0) / count)
    print(name, "mean", m1, "second moments", np.diag(m2), m2[0, 1], m2[0, 2], m2[1, 2], "sigmas", s1, s2d, s2o)
    assert np.abs(m1).max() <= 5.0 * s1
    assert np.abs(np.diag(m2) - 1.0 / 3.0).max() <= 5.0 * s2d
    assert max(abs(m2[0, 1]), abs(m2[0, 2]), abs(m2[1, 2])) <= 5.0 * s2o
    # another first_sample shifts the same stream of samples
    shifted = rtx.probe_rays(dev, P, SAMPLES, SEED, ids=ids, first_sample=3)
    assert shifted[:, :SAMPLES - 3].tobytes() == np.ascontiguousarray(rays[:, 3:]).tobytes()


@pytest.mark.parametrize("estimator", ESTIMATORS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_backfaces_tell_inside_from_outside(rtx_mod, gpu, precision, estimator):
    rtx = rtx_mod
    dev, _, _ = probes(rtx, "three")
    prims = dev.host.arrays()["prims"]
    assert list(prims[1]["g"][:4]) == [0.0, 0.0, -1.2, 0.5] and list(prims[2]["g"][:4]) == [1.0, 0.0, -1.0, 0.5]
    P = np.array([[0.0, 0.0, -1.2], [1.0, 0.0, -1.0], [0.0, 3.0, 2.0], [-2.0, 1.0, 0.5]])
    for c in P[2:]:  # outside all three spheres
        assert all(np.linalg.norm(c - p["g"][:3]) > p["g"][3] for p in prims)
    _, segs, back = dev.probe_sh(P, 16, DEPTH, seed=SEED, precision=precision, estimator=estimator, segments=True,
                                 backfaces=True)
    assert list(back) == [16, 16, 0, 0] and segs.min() >= 16


def sphere_quadrature(nz=32, nphi=32):
    """Directions (m, 3) and weights (sum 4 pi): Gauss-Legendre in z, equally spaced azimuths; exact
    for the polynomials integrated below (degree <= 6)."""
    zs, wz = np.polynomial.legendre.leggauss(nz)
    phis = 2.0 * np.pi * (np.arange(nphi) + 0.5) / nphi
    z, phi = np.meshgrid(zs, phis, indexing="ij")
    r = np.sqrt(1.0 - z * z)
    d = np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=2).reshape(-1, 3)
    return d, (wz[:, None] * np.full(nphi, 2.0 * np.pi / nphi)[None, :]).reshape(-1)


def sky(d):
    """sky() of rtx_device.h at unit directions: white to (0.5, 0.7, 1.0) in t = (y + 1) / 2."""
    return np.stack([0.75 - 0.25 * d[:, 1], 0.85 - 0.15 * d[:, 1], np.ones(len(d))], axis=1)


def test_open_sky_is_analytic(rtx_mod, gpu, tmp_path):
    rtx = rtx_mod
    path = tmp_path / "speck.rtxs"
    path.write_text("rtxscene 1\nbvh 0\ntex 0 solid 0.5 0.5 0.5\nmat 0 lambertian 0\n"
                    "tri 1000 0 0 1000 0.001 0 1000 0 0.001 0\n")
    dev = rtx.DeviceScene(rtx.HostScene.load(str(path)))
    count = 4096
    P = np.array([[0.0, 0.0, 0.0], [0.5, -0.25, 0.125], [-1.0, 2.0, 0.5], [0.0, -3.0, 1.0]])
    want = np.zeros((9, 3))
    want[0] = 2.0 * np.sqrt(np.pi) * np.array([0.75, 0.85, 1.0])
    want[1] = np.sqrt(4.0 * np.pi / 3.0) * np.array([-0.25, -0.15, 0.0])
    # the per-sample value of coefficient j, channel c is X = 4 pi Y_j(d) L_c(d), d uniform: its
    # mean and variance from the sky formula by quadrature
    q, w = sphere_quadrature()
    X = 4.0 * np.pi * basis(rtx, q)[:, :, None] * sky(q)[:, None, :]
    mean = (X * w[:, None, None]).sum(0) / (4.0 * np.pi)
    var = ((X * X) * w[:, None, None]).sum(0) / (4.0 * np.pi) - mean * mean
    assert np.abs(mean - want).max() <= 1e-13
    sigma = np.sqrt(np.maximum(var, 0.0) / count)
    # the constant blue channel of c0 has no variance, only rounding: `count` additions, each within
    # 2^-53 relative of a running sum that stays below the largest value compared here (< 4)
    slack = 4.0 * count * 2.0 ** -53
    axes = np.array([[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, -1.0, 0], [0, 0, 1.0], [0, 0, -1.0]])
    # sh_eval(cosine) is linear in the coefficients: per sample 4 pi L_c(d) sum_j a_j Y_j(d) Y_j(n)
    a = np.array([1.0] + [2.0 / 3.0] * 3 + [0.25] * 5)
    kern = (basis(rtx, q)[:, None, :] * basis(rtx, axes)[None, :, :] * a).sum(2)  # (m, 6)
    Xe = 4.0 * np.pi * kern[:, :, None] * sky(q)[:, None, :]
    me = (Xe * w[:, None, None]).sum(0) / (4.0 * np.pi)
    sigma_e = np.sqrt(np.maximum(((Xe * Xe) * w[:, None, None]).sum(0) / (4.0 * np.pi) - me * me, 0.0) / count)
    # the irradiance query's per-sample value is L_c(d), d cosine-weighted about n: a fine midpoint
    # rule over the sphere with the density max(0, n . d) / pi
    zs = (np.arange(512) + 0.5) / 256.0 - 1.0
    ph = 2.0 * np.pi * (np.arange(512) + 0.5) / 512.0
    zz, pp = np.meshgrid(zs, ph, indexing="ij")
    rr = np.sqrt(1.0 - zz * zz)
    g = np.stack([rr * np.cos(pp), rr * np.sin(pp), zz], axis=2).reshape(-1, 3)
    dens = np.maximum(g @ axes.T, 0.0) / np.pi * (4.0 * np.pi / len(g))  # (m, 6), sums to 1
    Lg = sky(g)
    mi = dens.T @ Lg
    sigma_i = np.sqrt(np.maximum(dens.T @ (Lg * Lg) - mi * mi, 0.0) / count)
    assert np.abs(dens.sum(0) - 1.0).max() <= 1e-4 and np.abs(mi - me).max() <= 1e-4
    for precision in PRECISIONS:
        got, segs, back = dev.probe_sh(P, count, DEPTH, seed=SEED, precision=precision, segments=True, backfaces=True)
        assert (segs == count).all() and not back.any(), "every path is one segment: no sample hit"
        dev_sigma = np.abs(got - want[None]) / np.maximum(sigma, 1e-300)[None]
        print(precision, "largest deviation in sigmas (coefficients with variance):", dev_sigma[:, sigma > 1e-9].max(),
              "c0", got[0, 0], "c1", got[0, 1])
        assert (np.abs(got - want[None]) <= 5.0 * sigma[None] + slack).all()
        for i in range(len(P)):
            e = rtx.sh_eval(got[i], axes, cosine=True)
            irr = dev.irradiance(np.repeat(P[i:i + 1], 6, axis=0), axes, count, DEPTH, seed=SEED, precision=precision)
            both = np.sqrt(sigma_e * sigma_e + sigma_i * sigma_i)
            print(precision, "probe", i, "largest |sh_eval - irradiance| / sigma:",
                  (np.abs(e - irr) / np.maximum(both, 1e-300))[both > 1e-9].max())
            assert (np.abs(e - irr) <= 5.0 * both + slack).all()
            assert (np.abs(e - me) <= 5.0 * sigma_e + slack).all()


def test_plain_and_mis_estimate_the_same_coefficients(rtx_mod, gpu):
    rtx = rtx_mod
    dev, P, ids = probes(rtx, "cornell")
    pick = np.array([8, 27])
    count = 2048
    Pp, pid = P[pick], ids[pick]
    sh = {e: dev.probe_sh(Pp, count, DEPTH, seed=SEED, ids=pid, estimator=e) for e in (None, "mis")}
    # per-sample values the test traces itself: the probes' own directions as independent paths
    # (a key of its own per ray), X = 4 pi Y_j(d) L_c
    rays = rtx.probe_rays(dev, Pp, count, SEED, ids=pid)
    flat = np.ascontiguousarray(rays.reshape(-1, 6))
    keys = np.arange(len(flat), dtype=np.uint32) + 100000
    var = {}
    for e in (None, "mis"):
        L = query(dev, e)(flat, 1, DEPTH, seed=SEED + 1, ids=keys).reshape(2, count, 3)
        X = 4.0 * np.pi * basis(rtx, rays[:, :, 3:])[:, :, :, None] * L[:, :, None, :]
        var[e] = X.var(axis=1, ddof=1)
    sigma = np.sqrt((var[None] + var["mis"]) / count)
    dev_sigma = np.abs(sh[None] - sh["mis"]) / sigma
    print("plain c0", sh[None][:, 0], "mis c0", sh["mis"][:, 0], "largest difference in sigmas", dev_sigma.max(),
          "per-sample variance of c0: plain", var[None][:, 0], "mis", var["mis"][:, 0])
    assert (sh[None] != sh["mis"]).any()
    assert (np.abs(sh[None] - sh["mis"]) <= 5.0 * sigma).all()
    assert (var["mis"][:, 0] < var[None][:, 0]).all()


@pytest.mark.parametrize("estimator", (None, "mis"))
@pytest.mark.parametrize("precision", PRECISIONS)
def test_chunking_changes_nothing(rtx_mod, gpu, precision, estimator):
    rtx = rtx_mod
    dev, P, ids = probes(rtx, "cornell")
    P, pid = P[:20], np.arange(1000, 1020, dtype=np.uint32)
    kw = dict(seed=SEED, precision=precision, estimator=estimator)
    runs = {}
    try:
        for chunk in (64, 7, 3, 0):  # whole probes per chunk; one per chunk; less than one's samples; default
            rtx.radiance_chunk(chunk)
            runs[chunk] = dev.probe_sh(P, 5, DEPTH, ids=pid, segments=True, backfaces=True, **kw)
            # the host entry point without ids keys by the probe's index, whatever the chunking
            runs[chunk] += (dev.probe_sh(P, 5, DEPTH, **kw),)
    finally:
        rtx.radiance_chunk(0)
    ref = runs[0]
    assert len(np.unique(ref[0].reshape(20, -1), axis=0)) == 20 and ref[1].min() >= 5 and ref[1].max() > 5
    for chunk in (64, 7, 3):
        for a, b in zip(runs[chunk], ref):
            assert a.tobytes() == b.tobytes(), chunk


@pytest.mark.parametrize("precision", PRECISIONS)
def test_keys(rtx_mod, gpu, precision):
    dev, P, ids = probes(rtx_mod, "cornell")
    kw = dict(precision=precision, segments=True, backfaces=True)
    a = dev.probe_sh(P, SAMPLES, DEPTH, seed=SEED, ids=ids, **kw)
    perm = np.random.default_rng(1).permutation(len(P))
    b = dev.probe_sh(P[perm], SAMPLES, DEPTH, seed=SEED, ids=ids[perm], **kw)
    for x, y in zip(a, b):
        assert y.tobytes() == x[perm].tobytes()
    c = dev.probe_sh(P, SAMPLES, DEPTH, seed=SEED + 1, ids=ids, **kw)
    assert (c[0] != a[0]).any((1, 2)).all()
    # ids = None is the probe's index; other ids give other values
    d = dev.probe_sh(P, SAMPLES, DEPTH, seed=SEED, **kw)
    e = dev.probe_sh(P, SAMPLES, DEPTH, seed=SEED, ids=np.arange(len(P)), **kw)
    for x, y in zip(d, e):
        assert x.tobytes() == y.tobytes()
    assert (d[0] != a[0]).any((1, 2)).all()


@pytest.mark.parametrize("estimator", ESTIMATORS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_non_finite_points(rtx_mod, gpu, precision, estimator):
    rtx = rtx_mod
    dev, P, ids = probes(rtx, "cornell")
    n = len(P)
    kw = dict(seed=SEED, ids=ids, precision=precision, estimator=estimator, segments=True, backfaces=True)
    whole = dev.probe_sh(P, SAMPLES, DEPTH, **kw)
    P2 = P.copy()
    bad = np.zeros(n, bool)
    for i, (axis, v) in enumerate(((0, np.nan), (1, np.inf), (2, -np.inf), (0, np.nan))):
        P2[5 * i + 1, axis] = v
        bad[5 * i + 1] = True
    got, segs, back = dev.probe_sh(P2, SAMPLES, DEPTH, **kw)
    assert not got[bad].any() and not np.signbit(got[bad]).any() and not segs[bad].any() and not back[bad].any()
    for x, y in zip((got, segs, back), whole):
        assert x[~bad].tobytes() == y[~bad].tobytes()
    assert whole[1].min() >= SAMPLES
    rays = rtx.probe_rays(dev, P2, SAMPLES, SEED, ids=ids)
    assert not rays[bad].any()
    assert rays[~bad].tobytes() == rtx.probe_rays(dev, P, SAMPLES, SEED, ids=ids)[~bad].tobytes()
    # a run of samples longer than the slot cap carries a non-finite probe's zeros too
    try:
        rtx.radiance_chunk(3)
        got3, segs3, back3 = dev.probe_sh(P2[:3], SAMPLES, DEPTH, **dict(kw, ids=ids[:3]))
    finally:
        rtx.radiance_chunk(0)
    assert got3.tobytes() == got[:3].tobytes() and segs3.tobytes() == segs[:3].tobytes()


@pytest.mark.parametrize("estimator", (None, "mis"))
@pytest.mark.parametrize("precision", PRECISIONS)
def test_device_entry_on_a_stream(rtx_mod, gpu, precision, estimator):
    import torch

    dev, P, ids = probes(rtx_mod, "bunny")
    n = len(P)
    common = dict(seed=SEED, first_sample=1, precision=precision, estimator=estimator)
    want, want_segs, want_back = dev.probe_sh(P, SAMPLES, DEPTH, ids=ids, segments=True, backfaces=True, **common)
    d_points = torch.from_numpy(P.copy()).cuda()
    d_ids = torch.from_numpy(ids.copy().view(np.int32)).cuda()
    d_out = torch.full((n + 2, 27), -7.0, dtype=torch.float64, device="cuda")
    d_segs = torch.full((n + 8,), 77, dtype=torch.int32, device="cuda")
    d_back = torch.full((n + 8,), 78, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    args = (d_points.data_ptr(), n, d_out.data_ptr(), SAMPLES, DEPTH)
    kw = dict(stream=stream.cuda_stream, **common)
    dev.probe_sh_device(*args, d_ids=d_ids.data_ptr(), d_segments=d_segs.data_ptr(), d_backfaces=d_back.data_ptr(), **kw)
    stream.synchronize()
    out = d_out.cpu().numpy()
    segs, back = d_segs.cpu().numpy().view(np.uint32), d_back.cpu().numpy().view(np.uint32)
    assert out[:n].tobytes() == want.tobytes()
    assert np.array_equal(segs[:n], want_segs) and np.array_equal(back[:n], want_back)
    assert (out[n:] == -7.0).all() and (segs[n:] == 77).all() and (back[n:] == 78).all()
    # without ids (the probe's index) and without counts
    d_out.fill_(-7.0)
    torch.cuda.synchronize()
    dev.probe_sh_device(*args, **kw)
    stream.synchronize()
    assert d_out.cpu().numpy()[:n].tobytes() == dev.probe_sh(P, SAMPLES, DEPTH, **common).tobytes()
    # n == 0: OK, nothing written
    d_out.fill_(-7.0)
    torch.cuda.synchronize()
    dev.probe_sh_device(d_points.data_ptr(), 0, d_out.data_ptr(), SAMPLES, DEPTH, d_ids=d_ids.data_ptr(),
                        d_segments=d_segs.data_ptr(), **kw)
    stream.synchronize()
    assert (d_out.cpu().numpy() == -7.0).all()
    out0, segs0, back0 = dev.probe_sh(np.zeros((0, 3)), SAMPLES, DEPTH, segments=True, backfaces=True)
    assert out0.shape == (0, 9, 3) and segs0.shape == (0,) and back0.shape == (0,)


def test_live_scene(rtx_mod, gpu, tmp_path):
    rtx = rtx_mod
    _, P, ids = probes(rtx, "three")
    host = rtx.HostScene.load(scene_path("three"))
    dev = rtx.DeviceScene(host)
    kw = dict(seed=SEED, ids=ids, segments=True, backfaces=True)
    before = dev.probe_sh(P, SAMPLES, DEPTH, **kw)
    prims = host.arrays()["prims"]
    assert prims[2]["kind"] == 0 and list(prims[2]["g"][:4]) == [1.0, 0.0, -1.0, 0.5]
    s = 0  # the sphere goes around this probe: every depth-0 segment then leaves through a back face
    assert before[2][s] == 0 and np.linalg.norm(P[s] - prims[0]["g"][:3]) > prims[0]["g"][3] + 1.0
    centre = [float(v) for v in P[s]]
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
        for estimator in ESTIMATORS:
            after = dev.probe_sh(P, SAMPLES, DEPTH, precision=precision, estimator=estimator, **kw)
            want = fresh.probe_sh(P, SAMPLES, DEPTH, precision=precision, estimator=estimator, **kw)
            for x, y in zip(after, want):
                assert x.tobytes() == y.tobytes()
            assert after[2][s] == SAMPLES and (after[0][s] != before[0][s]).any()


@pytest.mark.parametrize("name", ("three", "bunny"))
@pytest.mark.parametrize("precision", PRECISIONS)
def test_without_emitters_the_estimators_are_one(rtx_mod, gpu, name, precision):
    dev, P, ids = probes(rtx_mod, name)
    assert dev.emitters()[0] == 0
    kw = dict(seed=SEED, ids=ids, precision=precision, segments=True, backfaces=True)
    runs = [dev.probe_sh(P, SAMPLES, DEPTH, estimator=e, **kw) for e in ESTIMATORS]
    for other in runs[1:]:
        for x, y in zip(other, runs[0]):
            assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("flag", (None, "--mis"))
def test_command_line_probes(rtx_mod, gpu, flag):
    exe = os.path.join(PKG, "raytracer")
    cams = os.path.join(os.path.dirname(PKG), "configs", "cameras.json")
    cmd = [exe, "cornell_wide", "--scene", scene_path("cornell"), "--cameras", cams, "--probes", "2,2,2,8", "--seed", "77"]
    r = subprocess.run(cmd + ([flag] if flag else []), capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    lines = r.stdout.decode().splitlines()
    assert len(lines) == 8
    table = np.array([[float(t) for t in line.split()] for line in lines])
    assert table.shape == (8, 30)
    cfg = rtx_mod.camera_config("cornell_wide")
    assert b"probes: 8 probes, 8 samples, depth %d\n" % cfg.max_depth in r.stderr, r.stderr.decode()
    dev, _, _ = probes(rtx_mod, "cornell")
    box = rtx_mod.prim_bounds(dev.host.arrays()["prims"])
    centres = cell_centres(box[:, :3].min(0), box[:, 3:].max(0), (2, 2, 2))
    extent = (box[:, 3:].max(0) - box[:, :3].min(0)).max()
    assert np.abs(table[:, :3] - centres).max() <= 1e-3 * extent, "cell centres, x fastest"
    want = dev.probe_sh(table[:, :3], 8, cfg.max_depth, seed=77, estimator="mis" if flag else None)
    assert table[:, 3:].tobytes() == want.reshape(8, 27).tobytes()
