"""The reference for the hemisphere and light samplers of the query entry points
(tests/test_query_samples_host.py on the CPU, tests/test_gpu_query_samples.py on the device).

cosine_direction (csrc/rtx_occlusion.h) serves the AO pass and the irradiance queries;
direct_sample_from (csrc/rtx_direct.h) serves rtx_direct* and every vertex of the next-event
estimation.  What follows restates their documented mapping (the two headers' contract text and
DESIGN.md §4d / §4f / §4g) in plain numpy float64, from the CPU oracle's Philox draws, together
with the closed forms the light sampler's mean has to reach: a sphere's (R / D)^2 cos theta and
Lambert's polygon formula.  Nothing here is derived from the device code's structure, and the
reference renderer has no such queries: these functions are the reference.

Every elementwise numpy operation is one correctly rounded IEEE double operation and numpy never
contracts a product into a sum, so where the contract fixes the order of + * sqrt (a rect's and a
triangle's y - x) the reference's bits are the contract's bits.
"""
import functools
import math
import os
import tempfile

import numpy as np

import oracle_ctypes as orc

STREAM_AO, STREAM_IRR, STREAM_DIRECT, STREAM_NEE = 0xA0000000, 0xA1000000, 0xA2000000, 0xA3000000
SEAM_TMIN = float(np.float32(0.001))    # RTX_SEAM_TMIN
DIRECT_TMAX = float(np.float32(0.9999))  # RTX_DIRECT_TMAX
SPHERE, TRIANGLE, XY_RECT, XZ_RECT, YZ_RECT = 0, 1, 2, 3, 4
LIGHT = 3  # RTX_MAT_DIFFUSE_LIGHT
# why a sample is all zero (direct_sample_ref's `why`); 0: it is traced
TRACED, NO_AREA, BAD_NORMAL, NO_LENGTH, FACES_AWAY, EDGE_ON, BLACK = range(7)

N_MOMENTS = 65536   # samples per normal of the hemisphere moments
N_MEAN = 16384      # samples per query point of the closed-form comparisons


# ---------------------------------------------------------------------------------------
# draws
# ---------------------------------------------------------------------------------------
def draws(seed, pix, first_sample, count, stream, n):
    """(count, n): the first n draws of stream `stream` of (seed, pix, first_sample + k)."""
    out = np.empty((count, n))
    for k in range(count):
        out[k] = orc.philox(seed, int(pix), first_sample + k, n, stream)
    return out


# ---------------------------------------------------------------------------------------
# the hemisphere sampler
# ---------------------------------------------------------------------------------------
def basis(n):
    """u, v, w of a normal: w = n / sqrt(n . n), a = (0, 1, 0) where |w.x| > 0.9 and (1, 0, 0)
    elsewhere, v = normalize(w x a), u = v x w.  A division by a length is Vec3's: the product
    with its reciprocal (csrc/rtx_device.h), so the w.x the basis choice tests is the device's."""
    n = np.asarray(n, dtype=np.float64)
    w = (1.0 / math.sqrt(float((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]))) * n
    a = np.array([0.0, 1.0, 0.0]) if abs(w[0]) > 0.9 else np.array([1.0, 0.0, 0.0])
    v = np.cross(w, a)
    v = (1.0 / math.sqrt(float((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]))) * v
    u = np.cross(v, w)
    return u, v, w


def cosine_from_draws(r, n, phi_scale=2.0 * math.pi):
    """r: (count, 2) draws r1, r2.  phi_scale is 2 pi; the power test passes another."""
    u, v, w = basis(n)
    phi = phi_scale * r[:, 0]
    s = np.sqrt(r[:, 1])
    d = (s * np.cos(phi))[:, None] * u + (s * np.sin(phi))[:, None] * v + np.sqrt(1.0 - r[:, 1])[:, None] * w
    return d / np.sqrt((d * d).sum(1))[:, None]


def cosine_direction_ref(seed, pix, smp, stream, n, count=1):
    """Samples smp .. smp + count - 1 of pixel pix about the normal n: (count, 3) unit vectors."""
    return cosine_from_draws(draws(seed, pix, smp, count, stream, 2), n)


# ---------------------------------------------------------------------------------------
# the emitter table
# ---------------------------------------------------------------------------------------
def emitter_cum_ref(areas, lanes=256):
    """The inclusive running sum in k_emitter_scan's documented order: lane t owns the contiguous
    per = ceil(n / lanes) entries from t * per and adds them up from 0; the lanes' starting offsets
    are the left-to-right sum of the partial sums; each lane walks its entries again from its
    offset."""
    areas = [float(a) for a in areas]
    n = len(areas)
    per = -(-n // lanes)
    part = []
    for t in range(lanes):
        s = 0.0
        for i in range(min(t * per, n), min(t * per + per, n)):
            s += areas[i]
        part.append(s)
    cum = np.zeros(n)
    run = 0.0
    for t in range(lanes):
        s = run
        for i in range(min(t * per, n), min(t * per + per, n)):
            s += areas[i]
            cum[i] = s
        run += part[t]
    return cum


class Lights:
    """The emitters of a host scene (HostScene.arrays()), in the order of the primitive array,
    with the device record of each (a triangle holds A, B - A, C - A), their areas as
    k_emitter_area documents them and the cumulative table."""

    def __init__(self, arrays):
        prims, self.mats, self.texs = arrays["prims"], arrays["materials"], arrays["textures"]
        self.idx = np.flatnonzero(self.mats["kind"][prims["material"]] == LIGHT).astype(np.int64)
        self.kind = prims["kind"][self.idx].astype(np.int64)
        self.mat = prims["material"][self.idx].astype(np.int64)
        self.g = prims["g"][self.idx].copy()
        tri = self.kind == TRIANGLE
        self.g[tri, 3:6] = self.g[tri, 3:6] - self.g[tri, 0:3]
        self.g[tri, 6:9] = self.g[tri, 6:9] - self.g[tri, 0:3]
        self.areas = np.array([self.area(k, g) for k, g in zip(self.kind, self.g)])
        self.cum = emitter_cum_ref(self.areas)

    @staticmethod
    def area(kind, g):
        with np.errstate(all="ignore"):
            if kind == SPHERE:
                r = max(0.0, g[3])
                a = (4.0 * math.pi) * (r * r)
            elif kind == TRIANGLE:
                c = np.cross(g[3:6], g[6:9])
                a = 0.5 * math.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
            else:
                a = (g[1] - g[0]) * (g[3] - g[2])
        return float(a) if (a >= 0.0 and a < math.inf) else 0.0

    def tex_value(self, t, p):
        T = self.texs[t]
        if T["kind"] == 0:
            return np.broadcast_to(T["color"], p.shape).copy()
        assert T["kind"] == 1, "solid and checker textures only"
        cell = np.floor(T["inv_scale"] * p).astype(np.int64).sum(1)
        return np.where((cell % 2 == 0)[:, None], self.tex_value(T["even"], p), self.tex_value(T["odd"], p))

    def emitted(self, e, p):
        """Le of emitter e at the points p."""
        return self.tex_value(int(self.mats["texture"][self.mat[e]]), p)


def pick_emitter(cum, u0):
    """The first entry whose cumulative area exceeds u0 A; where the product rounds up to A the
    last entry, stepping back over entries of zero area."""
    n = len(cum)
    target = u0 * cum[-1]
    e = np.searchsorted(cum, target, side="right")
    for j in np.flatnonzero(e >= n):
        lo = n - 1
        while lo > 0 and cum[lo - 1] == cum[lo]:
            lo -= 1
        e[j] = lo
    return e


def place(kind, g, u1, u2, variant=None):
    """y on one emitter's record from (u1, u2), as rtx_direct.h writes it.  variant: one of the
    power test's deliberate errors."""
    if kind == SPHERE:
        r = max(0.0, g[3])
        z = (1.0 - u1) if variant == "sphere_z" else (1.0 - 2.0 * u1)
        rxy = np.sqrt(np.maximum(0.0, 1.0 - z * z))
        phi = 2.0 * math.pi * u2
        return g[0:3] + r * np.stack([rxy * np.cos(phi), rxy * np.sin(phi), z], axis=1)
    if kind == TRIANGLE:
        s = u1 if variant == "tri_no_sqrt" else np.sqrt(u1)
        return (g[0:3] + (s * (1.0 - u2))[:, None] * g[3:6]) + (s * u2)[:, None] * g[6:9]
    if variant == "rect_same_u":
        u2 = u1
    p = g[0] + u1 * (g[1] - g[0])
    q = g[2] + u2 * (g[3] - g[2])
    k = np.full_like(p, g[4])
    return np.stack({XY_RECT: (p, q, k), XZ_RECT: (p, k, q), YZ_RECT: (k, p, q)}[int(kind)], axis=1)


def light_normal(kind, g, p):
    """The unit normal of the hit record at p (either side: only |n_y . w| is used)."""
    if kind == SPHERE:
        return (p - g[0:3]) / max(0.0, g[3])
    if kind == TRIANGLE:
        c = np.cross(g[3:6], g[6:9])
        return np.broadcast_to(c / math.sqrt(float(c @ c)), p.shape)
    nrm = np.zeros(3)
    nrm[{XY_RECT: 2, XZ_RECT: 1, YZ_RECT: 0}[int(kind)]] = 1.0
    return np.broadcast_to(nrm, p.shape)


def samples_from_draws(L, x, n, u, variant=None):
    """u: (count, 3) draws u0, u1, u2 for one surfel (point x, normal n).  Returns the samples
    (count, 9: o, y - x, C), the emitter each draw selects (-1 where none is) and why a row is
    zero (TRACED where it is not)."""
    count = len(u)
    out = np.zeros((count, 9))
    pick = np.full(count, -1, np.int64)
    why = np.full(count, TRACED, np.int64)
    x, n = np.asarray(x, dtype=np.float64), np.asarray(n, dtype=np.float64)
    A = L.cum[-1] if len(L.cum) else 0.0
    if not (A > 0.0 and A < math.inf):
        why[:] = NO_AREA
        return out, pick, why
    with np.errstate(all="ignore"):
        l2 = float(n @ n)
    if not (l2 > 0.0 and l2 < math.inf):
        why[:] = BAD_NORMAL
        return out, pick, why
    unit = n / math.sqrt(l2)
    pick = pick_emitter(L.cum, u[:, 0])
    for e in np.unique(pick):
        rows = np.flatnonzero(pick == e)
        kind, g = L.kind[e], L.g[e]
        y = place(kind, g, u[rows, 1], u[rows, 2], variant)
        seg = y - x
        d2 = (seg * seg).sum(1)
        ok = (d2 > 0.0) & (d2 < math.inf)
        why[rows[~ok]] = NO_LENGTH
        rows, seg, d2 = rows[ok], seg[ok], d2[ok]
        p = x + seg  # the record's point: the segment's end at t = 1
        w = seg / np.sqrt(d2)[:, None]
        cx = np.maximum(0.0, (unit * w).sum(1))
        cy = np.abs((light_normal(kind, g, p) * w).sum(1))
        Le = L.emitted(e, p)
        C = Le * (cx * cy * A / (math.pi * d2))[:, None]
        lit = (C > 0.0).any(1)
        why[rows[~lit]] = np.where(cx[~lit] == 0.0, FACES_AWAY, np.where(cy[~lit] == 0.0, EDGE_ON, BLACK))
        rows = rows[lit]
        out[rows, 0:3], out[rows, 3:6], out[rows, 6:9] = x, seg[lit], C[lit]
    return out, pick, why


def direct_sample_ref(L, seed, pix, smp, x, n, count=1, depth=None):
    """Samples smp .. smp + count - 1 of the surfel (x, n) keyed by pix, from stream
    kRngStreamDirect, or kRngStreamNee + depth for a path vertex of that depth."""
    stream = STREAM_DIRECT if depth is None else STREAM_NEE + depth
    return samples_from_draws(L, x, n, draws(seed, pix, smp, count, stream, 3))


def direct_table_ref(L, seed, P, N, ids, count, first_sample=0, depth=None):
    """direct_sample_ref over surfels: (n, count, 9), picks and reasons (n, count)."""
    res = [direct_sample_ref(L, seed, ids[i], first_sample, P[i], N[i], count, depth) for i in range(len(P))]
    return tuple(np.stack([r[j] for r in res]) for j in range(3))


def sphere_visible(g, o, d, tmax=DIRECT_TMAX):
    """1 unless the segment (o, d) from a point to a sample on the sphere meets the sphere at t in
    (RTX_SEAM_TMIN, tmax).  The segment's end is itself the root t = 1, which lies in no such
    interval; by Vieta the other root is (|o - c|^2 - r^2) / |d|^2, with no cancellation."""
    oc = o - g[0:3]
    with np.errstate(all="ignore"):
        other = ((oc * oc).sum(1) - g[3] * g[3]) / (d * d).sum(1)
    return 1.0 - ((other > SEAM_TMIN) & (other < tmax)).astype(np.float64)


# ---------------------------------------------------------------------------------------
# closed forms (the query's 1 / pi convention)
# ---------------------------------------------------------------------------------------
def sphere_form(Le, g, x, n):
    n = np.asarray(n, dtype=np.float64) / np.linalg.norm(n)
    to = g[0:3] - np.asarray(x, dtype=np.float64)
    D = np.linalg.norm(to)
    assert n @ to > g[3], "the sphere is wholly above the horizon"
    return np.asarray(Le) * ((g[3] / D) ** 2 * (n @ to) / D)


def polygon_form(Le, verts, x, n):
    """Lambert: Le / (2 pi) |sum gamma_i (n . Gamma_i)|."""
    n = np.asarray(n, dtype=np.float64) / np.linalg.norm(n)
    v = np.asarray(verts, dtype=np.float64) - np.asarray(x, dtype=np.float64)
    assert (v @ n > 0.0).all(), "the polygon is wholly above the horizon"
    v = v / np.linalg.norm(v, axis=1, keepdims=True)
    total = 0.0
    for i in range(len(v)):
        a, b = v[i], v[(i + 1) % len(v)]
        c = np.cross(a, b)
        total += math.atan2(np.linalg.norm(c), a @ b) * (n @ (c / np.linalg.norm(c)))
    return np.asarray(Le) * (abs(total) / (2.0 * math.pi))


def light_vertices(kind, g):
    """A polygonal light's corners in order, from its device record."""
    if kind == TRIANGLE:
        return np.array([g[0:3], g[0:3] + g[3:6], g[0:3] + g[6:9]])
    c = [(g[0], g[2]), (g[1], g[2]), (g[1], g[3]), (g[0], g[3])]
    return np.array([{XY_RECT: (p, q, g[4]), XZ_RECT: (p, g[4], q), YZ_RECT: (g[4], p, q)}[int(kind)] for p, q in c])


def closed_form(L, x, n):
    """The direct light at (x, n) under a scene's single unoccluded light of constant Le."""
    kind, g = L.kind[0], L.g[0]
    Le = L.emitted(0, np.zeros((1, 3)))[0]
    return sphere_form(Le, g, x, n) if kind == SPHERE else polygon_form(Le, light_vertices(kind, g), x, n)


# ---------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------
_HEAD = """rtxscene 1
bvh %d
tex 0 solid 0.5 0.5 0.5
mat 0 lambertian 0
tex 1 solid 4 3 2
mat 1 light 1
rect xz -20 20 -20 20 -1 0
"""
# One light over a floor it does not touch.  Per scene: the light's line, then the query points
# (point, normal), each within about one diameter of the light, with the whole light above the
# point's horizon, and placed where a non-uniform sampler shows (the power test): off the rects'
# diagonals, off a sphere's equator, near a triangle's first vertex or far from it.
ONE_LIGHT = {
    "sphere": ("sphere 0 3 0 0.5 1",
               [((0.2, 2.2, -0.9), (0.0, 1.0, 1.0)), ((0.9, 2.6, 0.8), (-0.9, 0.4, -0.8)),
                ((0.2, 4.2, -0.6), (0.0, -2.0, 1.0))]),
    "triangle": ("tri -1 3 -1 1.5 3 -0.5 -0.5 3.4 1.2 1",
                 [((-0.9, 2.3, -0.8), (0.2, 1.0, 0.1)), ((1.2, 2.2, -0.3), (0.0, 1.0, 0.0)),
                  ((-0.4, 2.5, 1.0), (-0.1, 3.0, -0.2))]),
    "xy_rect": ("rect xy -1 1 -0.5 1 2 1",
                [((0.9, -0.4, 1.2), (0.0, 0.0, 1.0)), ((-0.9, 0.9, 1.0), (0.2, 0.1, 1.0)),
                 ((0.7, 0.8, 1.3), (0.0, 0.0, 0.5))]),
    "xz_rect": ("rect xz -1 1 -1 0.5 3 1",
                [((0.9, 2.0, -0.9), (0.0, 1.0, 0.0)), ((-0.8, 2.2, 0.4), (0.1, 1.0, -0.2)),
                 ((-0.9, 2.3, -0.9), (0.0, 2.0, 0.0))]),
    "yz_rect": ("rect yz 1 2.5 -1 1 2 1",
                [((1.0, 1.2, 0.8), (1.0, 0.0, 0.0)), ((0.8, 2.4, -0.9), (1.0, 0.1, 0.2)),
                 ((1.2, 2.3, 0.9), (3.0, 0.0, 0.0))]),
}
MEAN_SEED = 20261  # the closed-form comparisons' key; fixed with the points above
MEAN_IDS = np.array([40503, 977, 3000000001], dtype=np.uint32)


def one_light_text(name, bvh=1):
    return _HEAD % bvh + ONE_LIGHT[name][0] + "\n"


def one_light_points(name):
    pts = ONE_LIGHT[name][1]
    return np.array([p for p, _ in pts]), np.array([n for _, n in pts])


def zero_rows(name):
    """Surfels of a one-light scene whose samples are all zero: a point facing away from the light,
    one with a degenerate normal, and for a rect one on the light's own plane."""
    P, N = one_light_points(name)
    pts, nrm = [P[0], P[1], P[2]], [-N[0], np.zeros(3), np.array([np.nan, 1.0, 0.0])]
    if name.endswith("rect"):
        L = _lights_of(one_light_text(name))
        on = light_vertices(L.kind[0], L.g[0]).mean(0)
        axis = {XY_RECT: 2, XZ_RECT: 1, YZ_RECT: 0}[int(L.kind[0])]
        on[(axis + 1) % 3] += 3.0  # beside the light, on its plane
        pts.append(on)
        nrm.append(np.roll(np.array([1.0, 0.0, 0.0]), (axis + 1) % 3) * -1.0)
    return np.array(pts), np.array(nrm)


# every primitive kind as a light, a checker-textured light and a black one, over a floor, a wall
# and a blocker (which the samples, unlike the queries, do not see)
MIXED = """rtxscene 1
bvh 1
tex 0 solid 0.7 0.7 0.7
mat 0 lambertian 0
tex 1 solid 9 8 7
mat 1 light 1
tex 2 solid 4 5 6
mat 2 light 2
tex 3 solid 10 10 10
tex 4 solid 2 4 8
tex 5 checker 0.7 3 4
mat 3 light 5
tex 6 solid 0 0 0
mat 4 light 6
rect xz 0 10 0 10 0 0
rect yz 0 10 0 10 0 0
sphere 5 1.5 5 1 0
tri 1 9 1 4 9.5 1.5 1.5 8.5 4 1
sphere 2.5 6 7 0.5 2
rect xz 6 9 6 9 9.5 3
rect xy 2 4 3 5 9.8 1
rect yz 4 6 2 4 9.7 2
rect xz 1 3 6 8 9 4
"""


def mixed_surfels():
    """A 5 x 5 grid on the floor (normal +y) and one on the wall x = 0 (normal +x, length 2), then
    a point below the floor facing down (every light behind it), a degenerate normal, and a point
    on the checker light's plane facing down."""
    g = (np.arange(5) + 0.5) * 2.0
    a, b = [v.ravel() for v in np.meshgrid(g, g)]
    P = np.concatenate([np.stack([a, np.zeros_like(a), b], axis=1), np.stack([np.zeros_like(a), a, b], axis=1),
                        [[5.0, -0.5, 5.0], [3.0, 1.0, 3.0], [4.0, 9.5, 4.0]]])
    N = np.concatenate([np.tile([0.0, 1.0, 0.0], (25, 1)), np.tile([2.0, 0.0, 0.0], (25, 1)),
                        [[0.0, -1.0, 0.0], [0.0, 0.0, 0.0], [0.0, -1.0, 0.0]]])
    return P, N


def table_scene(n):
    """n lights over a floor, fanned about (5, 9, 5) with varied areas, in a flat list (the table
    keeps the file's order).  From n = 3 on the first and the last are triangles without area and
    the middle one is a sphere of negative radius; n = 2 starts with a triangle without area."""
    lines = ["rtxscene 1", "bvh 0", "tex 0 solid 0.5 0.5 0.5", "mat 0 lambertian 0", "tex 1 solid 2 2 2",
             "mat 1 light 1", "rect xz 0 10 0 10 0 0"]
    for i in range(n):
        a0 = 2.0 * math.pi * i / n
        a1 = a0 + 0.9 * min(2.0 * math.pi / n, 1.0)
        r = 1.0 + 0.37 * (i % 7) + 0.001 * i
        if (n >= 2 and i == 0) or (n >= 3 and i == n - 1) or (n >= 5 and i == n // 3):
            a1 = a0  # b == c: no area
        if n >= 3 and i == n // 2:
            lines.append("sphere 5 8 5 -0.25 1")
        else:
            lines.append("tri 5 9 5 %r 9 %r %r 9 %r 1" % (5 + r * math.cos(a0), 5 + r * math.sin(a0),
                                                          5 + r * math.cos(a1), 5 + r * math.sin(a1)))
    return "\n".join(lines) + "\n"


TABLE_SIZES = (1, 2, 255, 256, 257, 300, 512, 513, 1000)


def floor_surfels(count=3):
    """A count x count grid on the floor y = 0 of a table scene, normal +y."""
    g = (np.arange(count) + 0.5) * (10.0 / count)
    a, b = [v.ravel() for v in np.meshgrid(g, g)]
    return np.stack([a, np.zeros_like(a), b], axis=1), np.tile([0.0, 1.0, 0.0], (len(a), 1))


def odd_ids(n, salt=12345):
    """Explicit ids that are not the surfels' indices."""
    return ((np.arange(n, dtype=np.uint64) * 2654435761 + salt) % (1 << 32)).astype(np.uint32)


def load_host(rtx, text):
    """A HostScene of inline scene-file text."""
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "scene.rtxs")
        with open(path, "w") as f:
            f.write(text)
        return rtx.HostScene.load(path)


@functools.lru_cache(maxsize=None)
def _lights_of(text):
    import rtx

    host = load_host(rtx, text)
    L = Lights(host.arrays())
    L.host = host  # keeps the arrays alive
    return L


def lights_of(text):
    """The Lights of scene-file text, made once."""
    return _lights_of(text)


@functools.lru_cache(maxsize=None)
def mean_reference(name):
    """The reference estimator at a one-light scene's query points, N_MEAN samples each, made once
    and left unchanged: per point the closed form (3,), the reference's mean (3,) and sigma (3,)
    (its own per-sample standard deviation / sqrt N), and the draws (N_MEAN, 3)."""
    L = lights_of(one_light_text(name))
    P, N = one_light_points(name)
    rows = []
    for i in range(len(P)):
        u = draws(MEAN_SEED, MEAN_IDS[i], 0, N_MEAN, STREAM_DIRECT, 3)
        per = estimator(L, P[i], N[i], u)
        rows.append((closed_form(L, P[i], N[i]), per.mean(0), per.std(0, ddof=1) / math.sqrt(N_MEAN), u))
    return rows


def estimator(L, x, n, u, variant=None, tmax=DIRECT_TMAX):
    """C V per draw for a one-light scene: nothing but a sphere light itself shadows a sample."""
    smp, _, _ = samples_from_draws(L, x, n, u, variant)
    V = sphere_visible(L.g[0], smp[:, 0:3], smp[:, 3:6], tmax) if L.kind[0] == SPHERE else 1.0
    return smp[:, 6:9] * np.reshape(V, (-1, 1))


# ---------------------------------------------------------------------------------------
# normals for the direction tests
# ---------------------------------------------------------------------------------------
def direction_normals():
    """The axes; (0.9, sqrt(0.19), 0) and its neighbours in x, where the basis choice flips;
    lengths 1e-150 .. 1e150; 200 random normals."""
    edge = [0.9, math.sqrt(0.19), 0.0]
    rows = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], edge,
            [np.nextafter(0.9, 0.0), edge[1], 0.0], [np.nextafter(0.9, 1.0), edge[1], 0.0]]
    tilt = np.array([0.3, -0.5, 0.81])
    rows += [list(tilt * s) for s in (1e-150, 1.0, 3.7, 1e150)]
    rng = np.random.default_rng(4)
    rnd = rng.normal(size=(200, 3)) * rng.uniform(0.1, 10.0, size=(200, 1))
    return np.concatenate([np.array(rows, dtype=np.float64), rnd])
