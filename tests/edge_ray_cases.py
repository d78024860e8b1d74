"""Crafted edge rays for the closest-hit and any-hit walks (plain numpy, deterministic, no library).

The primitive arithmetic exists in several hand-written copies that must stay equal (csrc/rtx_device.h:
hit_sphere / hit_triangle / hit_rect, prim_t_rec and its branchless triangle form, finish_hit_at,
sphere_root / trav_globals, the f32 slab tests of visit_slabs and visit_tests).  Each case below is a
small .rtxs scene, rays aimed at the places where the copies can part, and the (tmin, tmax) pairs the
rays are traced on.  Coordinates are small integers and powers of two, so the intended equalities
(disc == 0, u == 0, t == tmin ...) hold exactly in binary; neighbours come from np.nextafter, in f64, or
in f32 where the reference's arithmetic is f32 (the triangle's det, u, v, t).

A case: name, scene (text), rays (n, 6), labels (n strings: what the row is for), tie (n bools: rows
where two primitives are hit at exactly the same distance), ranges ((tmin, tmax) pairs), family.
oracle/gen_edge_hits.py records the reference's own results into tests/golden/edge_hits.npz;
tests/test_edge_rays_host.py shows that each family reaches its target; tests/test_gpu_edge_rays.py
runs the device on them.

Triangles are kept out of every scene that gets rays with an overflowing, NaN or infinite component:
the reference's triangle test accepts a NaN distance (its range test is two negated comparisons), after
which the winner among several triangles depends on the order they are met, which the fast walk does
not promise to keep.  The non-finite rows are traced with tmin >= 0 only: with a negative tmin a rect
accepts t = (k - o) / inf = 0 with a NaN point, the same order dependence.
"""
import numpy as np

INF = float("inf")
NAN = float("nan")
SEAM = float(np.float32(0.001))
N_MATS = 4


def nxt(x, toward):
    return float(np.nextafter(np.float64(x), np.float64(toward)))


def nxt32(x, toward):
    return float(np.nextafter(np.float32(x), np.float32(toward)))


def scene_text(bvh, prims):
    lines = ["rtxscene 1", "bvh %d" % bvh, "tex 0 solid 0.5 0.5 0.5"]
    lines += ["mat %d lambertian 0" % m for m in range(N_MATS)]
    return "\n".join(lines + list(prims)) + "\n"


def num(x):
    return repr(float(x))


def sphere(c, r, m=0):
    return "sphere %s %s %s %s %d" % (num(c[0]), num(c[1]), num(c[2]), num(r), m)


def tri(a, b, c, m=0):
    return "tri " + " ".join(num(x) for x in (*a, *b, *c)) + " %d" % m


RECT_AXES = {"xy": (0, 1, 2), "xz": (0, 2, 1), "yz": (1, 2, 0)}  # first, second in-plane axis, plane axis


def rect(kind, a0, a1, b0, b1, k, m=0):
    return "rect %s %s %s %s %s %s %d" % (kind, num(a0), num(a1), num(b0), num(b1), num(k), m)


class Rows:
    def __init__(self):
        self.rays, self.labels, self.tie = [], [], []

    def add(self, label, o, d, tie=False):
        self.rays.append([float(x) for x in (*o, *d)])
        self.labels.append(label)
        self.tie.append(bool(tie))

    def arrays(self):
        return (np.ascontiguousarray(self.rays, dtype=np.float64).reshape(-1, 6), list(self.labels),
                np.array(self.tie, dtype=bool))


def case(name, family, scene, rows, ranges):
    rays, labels, tie = rows.arrays()
    return {"name": name, "family": family, "scene": scene, "rays": rays, "labels": labels, "tie": tie,
            "ranges": [(float(a), float(b)) for a, b in ranges]}


# far-away fillers (corners of a cube of half-size 8..12: no axis-parallel ray near the targets meets them)
FILL_SPHERES = [sphere((8, 8, 8), 1, 3), sphere((-8, 8, -8), 1, 3), sphere((8, -8, -8), 1, 3), sphere((-8, -8, 8), 1, 3),
                sphere((12, 12, -12), 1, 3), sphere((-12, 12, 12), 1, 3)]
FILL_TRIS = [tri((8, 8, 8), (9, 8, 8), (8, 9, 8), 3), tri((-8, 8, -8), (-9, 8, -8), (-8, 9, -8), 3),
             tri((8, -8, -8), (9, -8, -8), (8, -9, -8), 3), tri((-8, -8, 8), (-9, -8, 8), (-8, -9, 8), 3),
             tri((12, 12, -12), (13, 12, -12), (12, 13, -12), 3)]


def fill_rects(kind):
    return [rect(kind, 8 + 2 * i, 9 + 2 * i, 8, 9, -8 - i, 3) for i in range(5)]


# ---- spheres ------------------------------------------------------------------------------------------
SCALES = (1, -1, 100, -100, 500, -500, 520, -520, 540, -540)


def sphere_rows(c, r, pre=""):
    """Rays against the sphere (c, r), built in the sphere's own units: o = c + r * o_unit."""
    c = np.asarray(c, dtype=np.float64)
    R = Rows()

    def P(u):
        return c + r * np.asarray(u, dtype=np.float64)

    for ou, du, k in (((-1, 1, 0), (1, 0, 0), 1), ((-1, -1, 0), (1, 0, 0), 1), ((0, -1, 1), (0, 1, 0), 2),
                      ((1, 0, -1), (0, 0, 1), 0)):
        R.add(pre + "tangent", P(ou), du)  # disc == 0 exactly
        for tag, toward in (("tangent+ulp", 2 * ou[k]), ("tangent-ulp", 0.0)):
            u = list(ou)
            u[k] = nxt(ou[k], toward)
            R.add(pre + tag, P(u), du)
    R.add(pre + "tangent3", P((-3, 1, 0)), (1, 0, 0))  # disc == 0; the ulp is absorbed by 9 + y * y
    R.add(pre + "inside", P((0.5, 0, 0)), (1, 0, 0))
    R.add(pre + "inside", P((0, 0.25, -0.5)), (0, 1, 0))
    R.add(pre + "centre", P((0, 0, 0)), (0, 0, 1))
    R.add(pre + "centre", P((0, 0, 0)), (-1, 2, 0.5))
    R.add(pre + "surface_in", P((1, 0, 0)), (-1, 0, 0))
    R.add(pre + "surface_out", P((1, 0, 0)), (1, 0, 0))
    R.add(pre + "surface_tan", P((1, 0, 0)), (0, 1, 0))
    R.add(pre + "away", P((-3, 0, 0)), (-1, 0, 0))
    R.add(pre + "through", P((-3, 0, 0)), (1, 0, 0))  # roots 2 r and 4 r exactly
    R.add(pre + "through", P((0, 3, 0)), (0, -1, 0))
    R.add(pre + "segment", P((-2, 0, 0)), (r, 0, 0))  # a -> b with b on the surface: the near root is 1
    for k in SCALES:
        R.add(pre + "scale2^%d" % k, P((-3, 0.5, 0)), (2.0 ** k if abs(k) < 1024 else 0.0, 0, 0))
    return R


def unit_sphere_rows():
    R = sphere_rows((0, 0, 0), 1.0)
    R.add("r0_through", (-3, 5, 0), (1, 0, 0))
    R.add("r0_beside", (-3, 5, 0.5), (1, 0, 0))
    R.add("rneg_through", (-3, -5, 0), (1, 0, 0))
    R.add("rneg_beside", (-3, -5, 0.5), (1, 0, 0))
    return R


SPHERE_TARGETS = [sphere((0, 0, 0), 1, 0), sphere((0, 5, 0), 0, 1), sphere((0, -5, 0), -1, 2)]
SPHERE_RANGES = [(0, INF), (SEAM, INF), (2, INF), (nxt(2, 0), INF), (nxt(2, 3), INF), (0, 4), (0, nxt(4, 5)),
                 (0, nxt(4, 0)), (2, 4), (0, 1), (-8, INF), (-8, 0)]
FILL_RECTS_MIXED = fill_rects("xy")[:2] + fill_rects("xz")[:2] + fill_rects("yz")[:2]


def sphere_cases():
    rows = unit_sphere_rows()
    return [
        case("sph_one", "sphere", scene_text(1, SPHERE_TARGETS[:1]), rows, SPHERE_RANGES),
        case("sph_flat", "sphere", scene_text(0, SPHERE_TARGETS + FILL_SPHERES), rows, SPHERE_RANGES),
        case("sph_tree", "sphere", scene_text(1, SPHERE_TARGETS + FILL_SPHERES), rows, SPHERE_RANGES),
        case("sph_mixed", "sphere", scene_text(1, SPHERE_TARGETS + FILL_SPHERES[:3] + FILL_RECTS_MIXED), rows,
             SPHERE_RANGES),
    ]


GROUND_C, GROUND_R = (0.0, -1000.0, 0.0), 1000.0
GLOBAL_SMALL = [sphere((-3, 1, -3), 1, 1), sphere((3, 1, -3), 1, 1), sphere((-3, 1, 3), 1, 1), sphere((3, 1, 3), 1, 1),
                sphere((0, 3, 0), 1, 2), sphere((6, 2, 0), 2, 2)]
GLOBAL_RANGES = [(0, INF), (SEAM, INF), (2000, INF), (nxt(2000, 0), INF), (0, 4000), (2000, 4000), (0, 1),
                 (-8000, INF), (-8000, 0)]


def global_cases():
    rows = sphere_rows(GROUND_C, GROUND_R, pre="g:")
    rows.add("g:from_above", (0, 1, 0), (0, -1, 0))  # roots 1 and 2001: h - sq > 0
    rows.add("g:from_above", (0.5, 2, 0.25), (0, -2, 0))
    one = [sphere(GROUND_C, GROUND_R, 0)] + GLOBAL_SMALL
    two = [sphere(GROUND_C, GROUND_R, 0), sphere(GROUND_C, 950.0, 3)] + GLOBAL_SMALL
    return [case("glob_one", "global", scene_text(1, one), rows, GLOBAL_RANGES),
            case("glob_two", "global", scene_text(1, two), rows, GLOBAL_RANGES)]


# ---- triangles ----------------------------------------------------------------------------------------
T1 = ((0, 0, 0), (1, 0, 0), (0, 1, 0))
T2 = ((1, 0, 0), (1, 1, 0), (0, 1, 0))  # shares T1's edge B - C
TZ = ((4, 0, 0), (5, 0, 0), (6, 0, 0))  # zero area
TG = ((18.5, -1, -3), (21.25, -1.25, -3.5), (20.1, 1.5, -2.5))  # tilted, away from the others
TG_AIM = (20.0, 0.0, -3.0)


def tri_det32(t, d):
    """(float)det of Triangle::Hit for direction d: dot(e1, cross(d, e2)) in f64, rounded to f32."""
    a, b, c = (np.asarray(v, dtype=np.float64) for v in t)
    e1, e2 = b - a, c - a
    p = np.array([d[1] * e2[2] - d[2] * e2[1], d[2] * e2[0] - d[0] * e2[2], d[0] * e2[1] - d[1] * e2[0]])
    return np.float32(e1[0] * p[0] + e1[1] * p[1] + e1[2] * p[2])


def det_straddle(t, direction):
    """Scales (reject, accept) of `direction`, adjacent doubles, on either side of fabsf((float)det) <
    1e-6f: bisection on the f32 decision."""
    direction = np.asarray(direction, dtype=np.float64)
    eps = np.float32(1e-6)

    def rejected(s):
        return bool(np.abs(tri_det32(t, s * direction)) < eps)

    lo, hi = 0.0, 1.0
    while not rejected(lo) or rejected(hi):
        hi *= 2.0
        assert hi < 1e30
    while True:
        mid = 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            return lo, hi
        if rejected(mid):
            lo = mid
        else:
            hi = mid


def first_sum_above_one(u):
    """The f32 v nearest above 1 - u for which the f32 sum u + v exceeds 1."""
    v = np.float32(1.0) - np.float32(u)
    while not np.float32(u) + v > np.float32(1.0):
        v = np.nextafter(v, np.float32(2.0))
    return float(v)


TINY32 = nxt32(0.0, -1.0)  # the f32 below zero


def tri_rows():
    R = Rows()

    def down(label, x, y, tie=False):
        R.add(label, (x, y, 1), (0, 0, -1), tie)  # det 1, u = x, v = y, t = 1, all exact in f32

    down("inside", 0.25, 0.25)
    for label, on, out in (("edge:u0", (0, 0.5), (TINY32, 0.5)), ("edge:v0", (0.5, 0), (0.5, TINY32)),
                           ("edge:uv1", (0.5, 0.5), (0.5, first_sum_above_one(0.5))),
                           ("edge:uv1", (0.25, 0.75), (0.25, first_sum_above_one(0.25))),
                           ("edge:u1", (1, 0), (nxt32(1, 2), 0)), ("vertex:A", (0, 0), (TINY32, 0)),
                           ("vertex:A", (0, 0), (0, TINY32)), ("vertex:C", (0, 1), (0, nxt32(1, 2)))):
        down(label, *on)
        down(label + ":out", *out)
    # the same edges met by a ray with no zero component (o = (x - 1, y - 0.5, 1), d = (1, 0.5, -1): det 1,
    # u = x, v = y, t = 1, exact): no box is seen edge-on, so the forms inside a tree decide these
    E24, E23 = 2.0 ** -24, 2.0 ** -23
    for label, on, out in (("obl:edge:u0", (0, 0.5), (-E24, 0.5)), ("obl:edge:v0", (0.5, 0), (0.5, -E24)),
                           ("obl:edge:uv1", (0.5, 0.5), (0.5, 0.5 + E23)), ("obl:vertex:A", (0, 0), (-E24, 0)),
                           ("obl:vertex:B", (1, 0), (1 + E23, 0))):
        for lab, (x, y) in ((label, on), (label + ":out", out)):
            R.add(lab, (x - 1, y - 0.5, 1), (1, 0.5, -1))
    R.add("obl:inside", (0.25 - 1, 0.25 - 0.5, 1), (1, 0.5, -1))
    R.add("back", (0.25, 0.25, -1), (0, 0, 1))
    R.add("back:edge:u0", (0, 0.5, -1), (0, 0, 1))
    R.add("back:edge:u0:out", (TINY32, 0.5, -1), (0, 0, 1))
    R.add("oblique", (-0.75, 0.25, 1), (1, 0, -1))
    R.add("zero_area", (5, 0, 1), (0, 0, -1))
    R.add("zero_area", (5, -1, 0), (0, 1, 0))
    for tag, o, d in (("+", (0.25, 0.25, 1), (0, 0, -1)), ("-", (0.25, 0.25, -1), (0, 0, 1))):
        rej, acc = det_straddle(T1, d)
        R.add("det%s:acc" % tag, o, acc * np.asarray(d, dtype=np.float64))
        R.add("det%s:rej" % tag, o, rej * np.asarray(d, dtype=np.float64))
    og = np.array([20.0, 0.0, 3.0])
    dg = np.asarray(TG_AIM) - og
    rej, acc = det_straddle(TG, dg)
    R.add("gdet:full", og, dg)
    R.add("gdet:acc", og, acc * dg)
    R.add("gdet:rej", og, rej * dg)
    return R


TRI_RANGES = [(0, INF), (SEAM, INF), (1, INF), (nxt(1, 2), INF), (0, 1), (0, nxt(1, 0)), (1, 1), (-4, INF)]
TRI_TARGETS = [tri(*T1, 0), tri(*TZ, 1), tri(*TG, 2)]


def tri_cases():
    rows = tri_rows()
    shared = Rows()
    for x, y in ((0.5, 0.5), (0.25, 0.75), (0.75, 0.25), (1, 0), (0, 1)):
        shared.add("shared_edge", (x, y, 1), (0, 0, -1), tie=True)
        shared.add("shared_edge:back", (x, y, -1), (0, 0, 1), tie=True)
    for x, y in ((0.5, 0.5), (0.25, 0.75)):
        shared.add("obl:shared_edge", (x - 1, y - 0.5, 1), (1, 0.5, -1), tie=True)
    shared.add("only_t1", (0.25, 0.25, 1), (0, 0, -1))
    shared.add("only_t2", (0.75, 0.75, 1), (0, 0, -1))
    shared.add("neither", (1.25, 1.25, 1), (0, 0, -1))
    return [
        case("tri_one", "triangle", scene_text(1, TRI_TARGETS[:1]), rows, TRI_RANGES),
        case("tri_flat", "triangle", scene_text(0, TRI_TARGETS + FILL_TRIS), rows, TRI_RANGES),
        case("tri_tree", "triangle", scene_text(1, TRI_TARGETS + FILL_TRIS), rows, TRI_RANGES),
        case("tri_mixed", "triangle", scene_text(1, TRI_TARGETS + FILL_SPHERES[:3] + FILL_RECTS_MIXED), rows,
             TRI_RANGES),
        case("tri_shared", "triangle_tie", scene_text(1, [tri(*T1, 0), tri(*T2, 1)] + FILL_TRIS), shared,
             [(0, INF), (1, INF), (0, 1)]),
    ]


# ---- rects --------------------------------------------------------------------------------------------
RECT_OFFSET = {"xy": (0.0, 0.0, 0.0), "xz": (32.0, 0.0, 0.0), "yz": (0.0, 32.0, 0.0)}


def rect_group(kind, off):
    """The target rects of one kind in local (a, b, k) coordinates, moved by `off` (world x, y, z)."""
    ia, ib, ik = RECT_AXES[kind]
    A, B, K = off[ia], off[ib], off[ik]
    return [rect(kind, A + 0, A + 1, B + 0, B + 2, K, 0),    # the target
            rect(kind, A + 5, A + 4, B + 0, B + 2, K, 1),    # x0 > x1
            rect(kind, A + 3, A + 3, B + 4, B + 4, K, 2)]    # zero size


def rect_rows(kind, off):
    """Rays against rect_group(kind, off).  In-plane coordinates are world values (A0 + ..., B0 + ...)."""
    ia, ib, ik = RECT_AXES[kind]
    A0, B0, K0 = off[ia], off[ib], off[ik]
    R = Rows()

    def pt(a, b, k):  # world point: in-plane world coordinates a, b; k along the plane axis from the plane
        v = [0.0, 0.0, 0.0]
        v[ia], v[ib], v[ik] = a, b, K0 + k
        return v

    def vec(a, b, k):
        v = [0.0, 0.0, 0.0]
        v[ia], v[ib], v[ik] = a, b, k
        return v

    def down(label, a, b):
        R.add(label, pt(a, b, 1), vec(0, 0, -1))  # t = 1, the hit point's in-plane coordinates are a, b

    down("inside", A0 + 0.5, B0 + 1)
    a_lo, a_hi = nxt(A0 + 0, A0 - 1), nxt(A0 + 1, A0 + 2)  # the next doubles outside
    b_lo, b_hi = nxt(B0 + 0, B0 - 1), nxt(B0 + 2, B0 + 3)
    for label, on, out in (("edge:a0", (A0, B0 + 1), (a_lo, B0 + 1)), ("edge:a1", (A0 + 1, B0 + 1), (a_hi, B0 + 1)),
                           ("edge:b0", (A0 + 0.5, B0), (A0 + 0.5, b_lo)), ("edge:b1", (A0 + 0.5, B0 + 2), (A0 + 0.5, b_hi)),
                           ("corner:00", (A0, B0), (a_lo, B0)), ("corner:10", (A0 + 1, B0), (A0 + 1, b_lo)),
                           ("corner:02", (A0, B0 + 2), (A0, b_hi)), ("corner:12", (A0 + 1, B0 + 2), (a_hi, B0 + 2))):
        down(label, *on)
        down(label + ":out", *out)
    # the same edges met by a ray with no zero component (t = 1, in-plane hit coordinates a, b exactly):
    # no box is seen edge-on, so the forms inside a tree decide these
    E30 = 2.0 ** -30
    for label, on, out in (("obl:edge:a0", (A0, B0 + 1), (A0 - E30, B0 + 1)), ("obl:edge:a1", (A0 + 1, B0 + 1), (A0 + 1 + E30, B0 + 1)),
                           ("obl:edge:b0", (A0 + 0.5, B0), (A0 + 0.5, B0 - E30)),
                           ("obl:corner:12", (A0 + 1, B0 + 2), (A0 + 1, B0 + 2 + E30))):
        for lab, (a, b) in ((label, on), (label + ":out", out)):
            R.add(lab, pt(a - 1, b - 0.5, 1), vec(1, 0.5, -1))
    R.add("obl:inside", pt(A0 + 0.5 - 1, B0 + 1 - 0.5, 1), vec(1, 0.5, -1))
    R.add("back", pt(A0 + 0.5, B0 + 1, -1), vec(0, 0, 1))
    R.add("neg2", pt(A0 + 0.5, B0 + 1, 1), vec(0, 0, -2))
    R.add("oblique", pt(A0 - 0.5, B0 + 1, 1), vec(1, 0, -1))
    R.add("par_off", pt(A0 + 0.5, B0 + 1, 1), vec(1, 0, 0))    # t = -inf
    R.add("par_off", pt(A0 + 0.5, B0 + 1, -1), vec(1, 0, 0))   # t = +inf
    R.add("par_in", pt(A0 - 1, B0 + 1, 0), vec(1, 0, 0))       # t = 0 / 0
    R.add("reversed", pt(A0 + 4.5, B0 + 1, 1), vec(0, 0, -1))
    R.add("zero_size", pt(A0 + 3, B0 + 4, 1), vec(0, 0, -1))
    R.add("zero_size:out", pt(nxt(A0 + 3, A0 + 4), B0 + 4, 1), vec(0, 0, -1))
    return R


RECT_RANGES = [(0, INF), (SEAM, INF), (1, INF), (nxt(1, 0), INF), (0, 1), (0, nxt(1, 2)), (-4, INF)]


def merge(*rows):
    R = Rows()
    for r in rows:
        R.rays += r.rays
        R.labels += r.labels
        R.tie += r.tie
    return R


def rect_cases():
    out = []
    zero = (0.0, 0.0, 0.0)
    for kind in ("xy", "xz", "yz"):
        rows = rect_rows(kind, zero)
        out.append(case("rect_one_" + kind, "rect", scene_text(1, rect_group(kind, zero)[:1]), rows, RECT_RANGES))
        out.append(case("rect_tree_" + kind, "rect", scene_text(1, rect_group(kind, zero) + fill_rects(kind)), rows,
                        RECT_RANGES))
        ia, ib, ik = RECT_AXES[kind]
        tie = Rows()
        for a, b in ((0.5, 1), (0.25, 0.5), (0.75, 1.5)):
            o = [0.0, 0.0, 0.0]
            o[ia], o[ib], o[ik] = a, b, 1.0
            d = [0.0, 0.0, 0.0]
            d[ik] = -1.0
            tie.add("coincident", o, d, tie=True)
        o = [0.0, 0.0, 0.0]
        o[ia], o[ib], o[ik] = 1.5, 1.0, 1.0
        tie.add("coincident:miss", o, d)
        two = [rect(kind, 0, 1, 0, 2, 0, 0), rect(kind, 0, 1, 0, 2, 0, 1)]
        out.append(case("rect_tie_" + kind, "rect_tie", scene_text(1, two + fill_rects(kind)), tie,
                        [(0, INF), (SEAM, INF), (0, 1)]))
    groups, rows = [], []
    for kind in ("xy", "xz", "yz"):
        groups += rect_group(kind, RECT_OFFSET[kind])
        rows.append(rect_rows(kind, RECT_OFFSET[kind]))
    rows = merge(*rows)
    out.append(case("rect_flat", "rect", scene_text(0, groups), rows, RECT_RANGES))
    out.append(case("rect_mixed", "rect", scene_text(1, groups + FILL_SPHERES[:3]), rows, RECT_RANGES))
    return out


# ---- the walk -----------------------------------------------------------------------------------------
WALK_PRIMS = [rect("yz", 0, 2, 0, 2, 0, 1), rect("xy", -4, 4, 0, 4, -2, 0), rect("xz", -4, 4, -4, 4, -1, 0),
              sphere((2, 1, 2), 1, 2), sphere((-2, 1, 2), 1, 2), sphere((2, 1, -1), 0.5, 2), sphere((-2, 3, 0), 1, 3),
              sphere((0, 5, 0), 1, 3), sphere((3, 3, 3), 0.5, 3)]
P126, P125, P127, P128 = 2.0 ** 126, 2.0 ** 125, 2.0 ** 127, 2.0 ** 128


def walk_rows():
    R = Rows()
    # origin exactly in the plane of a node box's face (a rect's box is its plane -/+ 0.0001)
    R.add("inplane", (-6, 1, -2 + 0.0001), (1, 0, 0))
    R.add("inplane", (-6, 1, -2 - 0.0001), (1, 0, 0))
    R.add("inplane", (-6, 1, -2), (1, 0, 0))
    R.add("inplane", (-6, -1 + 0.0001, 1), (1, 0, 0))
    R.add("inplane", (0 + 0.0001, 1, 6), (0, 0, -1))
    R.add("inplane", (1, 0, 6), (0, 0, -1))       # the face y = 0 of the spheres' boxes
    # box edges and corners
    R.add("boxedge", (-6, 2, 3), (1, 0, 0))
    R.add("boxedge", (1, 2, 6), (0, 0, -1))
    R.add("boxcorner", (-4, -5, -4), (1, 1, 1))
    R.add("boxcorner", (6, 5, 6), (-1, -1, -1))
    R.add("ordinary", (-6, 1, 2), (1, 0, 0))
    R.add("ordinary", (5, 6, 4), (-3, -4, -1.5))
    # geometry behind the origin (a negative tmin reaches it)
    R.add("behind", (-6, 1, 2), (-1, 0, 0))
    R.add("behind", (6, 1, 2), (1, 0, 0))
    R.add("behind", (1, 1, 6), (0, 0, 2))
    R.add("behind", (0.5, 8, 0.5), (0.25, 1, 0.125))
    # degenerate directions
    R.add("dzero", (2, 1, 2), (0, 0, 0))
    R.add("dzero", (-6, 1, 1), (0, 0, 0))
    R.add("ddenorm", (-6, 1, 2), (1e-40, 1e-40, 1e-40))
    R.add("ddenorm", (2, 1, 2), (1e-40, -1e-40, 1e-40))
    R.add("ddenorm1", (-6, 1, 2), (1, 1e-40, 1e-40))
    # components beyond the f32 range, small |o| ...
    R.add("dbig:small_o", (-6, 1, 2), (1e39, 0, 0))
    R.add("dbig:small_o", (-6, 1, 2), (1e39, 1, 1))
    R.add("dbig:small_o", (-4, -5, -4), (1e39, 1e39, 1e39))
    R.add("dbig:small_o", (-4, -5, -4), (1e300, 1e300, 1e300))
    R.add("dbig:small_o", (-6, 1, 1), (1e300, 1, 1))
    # ... one component beyond the f32 range and another inside it, aimed at the sphere (2, 1, 2) from
    # outside its box's y slab: the y entry distance is positive, of the order of 1 / d.y
    R.add("dbig:mixed", (-14, -1, 2), (P128, P125, 0))
    R.add("dbig:mixed", (-2, -1, 2), (P128, P127, 0))  # d.y is f32-finite, its reciprocal an f32 denormal
    R.add("dbig:mixed", (-14, -1, 2), (1e39, 1.25e38, 0))
    R.add("dbig:mixed", (2, -3, -14), (0, 2.0 ** 298, 2.0 ** 300))
    # ... and large |o|: a box is thinner than an ulp of o there, and the f64 slab test rejects it
    R.add("dbig:large_o", (-3 * P126, 0.25, 1), (P128, 1, 0))
    R.add("dbig:large_o", (-1e300, 0, 1), (1e300, 1, 0))
    R.add("dbig:large_o", (-3 * P126, -3 * P126, -3 * P126), (P128, P128, P128))
    # |o| beyond the f32 range
    R.add("obig", (1e39, 5, 0), (-1, 0, 0))
    R.add("obig", (1, 1e39, 1), (0, -1, 0))
    return R


def nonfinite_rows():
    R = Rows()
    R.add("nan", (NAN, 1, 2), (1, 0, 0))
    R.add("nan", (-6, 1, 2), (NAN, 0, 0))
    R.add("nan", (-6, 1, 2), (1, NAN, 0))
    R.add("nan", (-6, 1, 2), (NAN, NAN, NAN))
    R.add("inf", (INF, 1, 2), (-1, 0, 0))
    R.add("inf", (-6, 1, 2), (INF, 0, 0))
    R.add("inf", (-6, 1, 2), (INF, 1, 0))
    R.add("inf", (-6, 1, 2), (-INF, -INF, -INF))
    R.add("ordinary", (-6, 1, 2), (1, 0, 0))
    return R


WALK_RANGES = [(0, INF), (SEAM, INF), (0, 10), (-20, INF), (-20, -1), (-INF, INF)]


def walk_cases():
    return [case("walk", "walk", scene_text(1, WALK_PRIMS), walk_rows(), WALK_RANGES),
            case("walk_nonfinite", "walk_nonfinite", scene_text(1, WALK_PRIMS), nonfinite_rows(),
                 [(0, INF), (SEAM, INF), (0, 10)])]


def triangle_only_materials(scene):
    """Material ids that only triangles of the scene text carry; asserts that no id is shared between a
    triangle and another kind (a hit's kind is then known from its material)."""
    tri_m, other = set(), set()
    for line in scene.splitlines():
        w = line.split()
        if w and w[0] == "tri":
            tri_m.add(int(w[-1]))
        elif w and w[0] in ("sphere", "rect"):
            other.add(int(w[-1]))
    assert not (tri_m & other), (tri_m, other)
    return sorted(tri_m)


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = sphere_cases() + global_cases() + tri_cases() + rect_cases() + walk_cases()
        names = [c["name"] for c in _CASES]
        assert len(set(names)) == len(names)
    return _CASES


def by_name(name):
    return next(c for c in cases() if c["name"] == name)
