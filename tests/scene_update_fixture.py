"""Fixtures of the scene-update tests (test_scene_update_host.py, test_scene_update_gpu.py).

A pair of scene files A and B: the same primitive list (kinds, materials, order) with different
geometry.  Primitive i lives inside its own cell of a 4-unit grid (every coordinate within 1.7 of
the cell centre), so the primitives are disjoint in A and in B; the large scenes start with one
ground sphere of radius 1000 under the grid.  Every primitive has its own material, so a hit
record names its primitive.  All materials are fuzz-free metals: a path then involves no cos / sin
(Lambertian and fuzzy scatter), whose device and glibc versions differ in the last ulp
(test_gpu_parity.py), so device renders can be compared with the oracle's bit for bit.
"""
import numpy as np

SPHERE, TRIANGLE, XY, XZ, YZ = 0, 1, 2, 3, 4
COLS = [0, 1, 2, 3, 4, 5, 6, 7, 10, 11]  # hit t p3 n3 front_face material (u, v left out: acos / atan2)
COUNTS = (1, 2, 5, 67, 2000)
VARIANTS = ("mixed", "tri")
N_RAYS = 4000
# seed of each fixture's geometry; every hit ray of its 4000 has exactly one primitive at its
# closest t in B (test_scene_update_host.py checks that with the oracle; change the seed if not)
SEEDS = {(n, v): 100 + 10 * k + j for k, n in enumerate(COUNTS) for j, v in enumerate(VARIANTS)}


def cell_centre(i):
    ix, iz, iy = i % 16, (i // 16) % 16, i // 256
    return np.array([4.0 * ix - 30.0, 4.0 + 4.0 * iy, 4.0 * iz - 30.0])


def make_prims(rtx, n, variant, seed, which):
    """The PRIM_DTYPE records (list order) of file A (which = 0) or B (which = 1)."""
    rng = np.random.default_rng([seed, which])
    out = np.zeros(n, rtx.PRIM_DTYPE)
    ground = n >= 1000
    for i in range(n):
        out[i]["material"] = i
        if ground and i == 0:
            out[i]["kind"] = SPHERE
            out[i]["g"][:4] = [0.0, -1000.0 - 0.25 * which, 0.0, 1000.0]
            continue
        c = cell_centre(i) + rng.uniform(-0.5, 0.5, 3)
        kind = TRIANGLE if variant == "tri" else (SPHERE, TRIANGLE, XY + (i // 3) % 3)[i % 3]
        out[i]["kind"] = kind
        if kind == SPHERE:
            out[i]["g"][:4] = [*c, rng.uniform(0.3, 1.2)]
        elif kind == TRIANGLE:
            out[i]["g"][:] = (c[None, :] + rng.uniform(-1.2, 1.2, (3, 3))).ravel()
        else:
            a0, a1 = {XY: (0, 1), XZ: (0, 2), YZ: (1, 2)}[kind]
            ax = 3 - a0 - a1
            h = rng.uniform(0.3, 1.2, 2)
            out[i]["g"][:5] = [c[a0] - h[0], c[a0] + h[0], c[a1] - h[1], c[a1] + h[1], c[ax]]
    return out


def prim_lines(prims):
    out = []
    for p in prims:
        g = [repr(float(v)) for v in p["g"]]
        if p["kind"] == SPHERE:
            out.append("sphere %s %d" % (" ".join(g[:4]), p["material"]))
        elif p["kind"] == TRIANGLE:
            out.append("tri %s %d" % (" ".join(g), p["material"]))
        else:
            out.append("rect %s %s %d" % ({XY: "xy", XZ: "xz", YZ: "yz"}[int(p["kind"])], " ".join(g[:5]), p["material"]))
    return out


def write_scene(path, prims, bvh=1):
    n = len(prims)
    hdr = ["rtxscene 1", "bvh %d" % bvh]
    hdr += ["mat %d metal %r %r %r 0.0" % (i, 0.5 + 0.4 * ((i * 7) % 11) / 10.0, 0.5 + 0.4 * ((i * 5) % 13) / 12.0,
                                           0.5 + 0.4 * ((i * 3) % 7) / 6.0) for i in range(n)]
    with open(path, "w") as f:
        f.write("\n".join(hdr + prim_lines(prims)) + "\n")
    return str(path)


def centres(prims):
    g = prims["g"]
    k = prims["kind"]
    c = np.zeros((len(prims), 3))
    c[k == SPHERE] = g[k == SPHERE][:, :3]
    t = k == TRIANGLE
    c[t] = (g[t][:, 0:3] + g[t][:, 3:6] + g[t][:, 6:9]) / 3.0
    for kind, (a0, a1) in {XY: (0, 1), XZ: (0, 2), YZ: (1, 2)}.items():
        m = k == kind
        c[m, a0], c[m, a1], c[m, 3 - a0 - a1] = 0.5 * (g[m, 0] + g[m, 1]), 0.5 * (g[m, 2] + g[m, 3]), g[m, 4]
    return c


def frame(prims):
    """Centre and radius of the grid primitives (the ground sphere left out)."""
    c = centres(prims)
    if len(prims) >= 1000:
        c = c[1:]
    mid = 0.5 * (c.min(0) + c.max(0))
    return mid, float(np.linalg.norm(c - mid, axis=1).max()) + 2.0


def make_rays(prims, seed):
    """4000 fixed rays at B's primitives: half from a shell above the scene, half from the gaps
    between the cells (corner points, outside every primitive), aimed at a primitive's centre
    with a jitter about its size."""
    rng = np.random.default_rng([seed, 7])
    c = centres(prims)
    grid = c[1:] if len(prims) >= 1000 else c
    mid, rad = frame(prims)
    h = N_RAYS // 2
    u = rng.normal(size=(h, 3))
    u[:, 1] = np.abs(u[:, 1]) + 0.2
    u /= np.linalg.norm(u, axis=1)[:, None]
    o_out = mid + u * (1.5 * rad + 5.0)
    cells = np.array([cell_centre(i) for i in rng.integers(0, max(len(prims), 8), N_RAYS - h)])
    o_in = cells + 2.0 * np.where(rng.random((N_RAYS - h, 3)) < 0.5, -1.0, 1.0) + rng.uniform(-0.05, 0.05, (N_RAYS - h, 3))
    o = np.vstack([o_out, o_in])
    t = grid[rng.integers(0, len(grid), N_RAYS)] + rng.uniform(-1.0, 1.0, (N_RAYS, 3))
    return np.ascontiguousarray(np.column_stack([o, t - o]))


_cache = {}


def pair(rtx, tmp, n, variant):
    """(prims A, prims B (list order), file A, file B, rays) of one fixture, made once per run."""
    key = (n, variant)
    if key not in _cache:
        seed = SEEDS[key]
        a, b = make_prims(rtx, n, variant, seed, 0), make_prims(rtx, n, variant, seed, 1)
        fa = write_scene(tmp / ("upd_%d_%s_a.rtxs" % key), a)
        fb = write_scene(tmp / ("upd_%d_%s_b.rtxs" % key), b)
        _cache[key] = (a, b, fa, fb, make_rays(b, seed))
    return _cache[key]
