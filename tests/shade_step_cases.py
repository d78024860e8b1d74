"""Cases of the step-level shading tests (tests/test_shade_steps_host.py, tests/test_gpu_shade_steps.py):
small scene files that hold the material and texture tables under test, the case families, and the
comparison of step records.  A case is one shading step: a hit record, a path state and the Philox
key of its path (oracle_ctypes.SHADE_CASE, the layout of the device hook too); its record
(SHADE_RECORD) is the step's whole outcome.  Everything here runs on the CPU.

Every family is a dict: cases, lamb (rows whose material is a Lambertian), and whatever its own
assertions need.  All cases are wavefront-mode cases (depth counts up); scatter_form() turns them
into the scatter API's (depth counts down from max_depth, the same stream)."""
import os

import numpy as np

import oracle_ctypes as orc

SEED = 20240607
MAX_DEPTH = 50
NUDGES = sorted(((c, s) for c in range(-2, 3) for s in range(-2, 3)), key=lambda t: (abs(t[0]) + abs(t[1]), t))
assert NUDGES[0] == (0, 0) and len(NUDGES) == 25

# ---- scenes: one dummy sphere (and three rects for the deferred u, v) plus the tables under test ----
# material ids of TABLE
LAMB_SOLID, LAMB_CHECKER, LAMB_CHECKER2, LAMB_CHECKER_IMG, LAMB_IMAGE, LAMB_MISSING = 0, 1, 2, 3, 4, 5
METALS = (6, 7, 8, 9)          # fuzz 0, 0.3, 1, 1.7 in the file (clamped to 1 at load)
GLASS = (10, 11, 12, 13)       # ri 1.5, 1.0, 2.4, 1 / 1.5
GLASS_RI = (1.5, 1.0, 2.4, 1 / 1.5)
LIGHT_SOLID, LIGHT_DIM, LIGHT_CHECKER, LIGHT_IMAGE = 14, 15, 16, 17
SPHERE, RECT_XY, RECT_XZ, RECT_YZ = 0, 1, 2, 3  # primitive indices (bvh 0: the file's order)
SPHERE_G = (1.0, 2.0, 3.0, 2.0)
RECTS_G = {RECT_XY: (0.0, 4.0, 0.0, 2.0, 1.0), RECT_XZ: (-1.0, 3.0, 0.0, 5.0, 2.0), RECT_YZ: (1.0, 2.0, -3.0, 3.0, 0.0)}
TABLE = f"""rtxscene 1
bvh 0
tex 0 solid 0.8 0.3 0.1
tex 1 solid 0.9 0.9 0.9
tex 2 solid 0.2 0.3 0.1
tex 3 checker 0.5 1 2
tex 4 checker 2 3 1
tex 5 image earthmap
tex 6 checker 1 5 0
tex 7 image no_such_image
tex 8 solid 4 4 4
tex 9 solid 1e-9 0 5e-9
tex 10 checker 0.25 8 9
mat 0 lambertian 0
mat 1 lambertian 3
mat 2 lambertian 4
mat 3 lambertian 6
mat 4 lambertian 5
mat 5 lambertian 7
mat 6 metal 0.8 0.6 0.2 0
mat 7 metal 0.7 0.7 0.7 0.3
mat 8 metal 0.9 0.5 0.5 1
mat 9 metal 0.5 0.5 0.9 1.7
mat 10 dielectric 1.5
mat 11 dielectric 1
mat 12 dielectric 2.4
mat 13 dielectric {1 / 1.5!r}
mat 14 light 8
mat 15 light 9
mat 16 light 10
mat 17 light 5
sphere 1 2 3 2 0
rect xy 0 4 0 2 1 0
rect xz -1 3 0 5 2 0
rect yz 1 2 -3 3 0 0
"""
# every material a Lambertian with a solid colour: all four LAMB / NOTEX forms are legal
LAMB_NOTEX = """rtxscene 1
bvh 0
tex 0 solid 0.8 0.3 0.1
mat 0 lambertian 0
tex 1 solid 0.25 0.5 0.95
mat 1 lambertian 1
sphere 0 0 0 1 0
"""
# mixed materials, no texture table read: the NOTEX forms only
MIXED_NOTEX = """rtxscene 1
bvh 0
tex 0 solid 0.8 0.3 0.1
mat 0 lambertian 0
mat 1 metal 0.8 0.6 0.2 0.3
mat 2 dielectric 1.5
tex 1 solid 4 4 4
mat 3 light 1
sphere 0 0 0 1 0
"""
SCENES = {"table": TABLE, "lamb_notex": LAMB_NOTEX, "mixed_notex": MIXED_NOTEX}
# the core forms a scene's flags allow (rtx.SHADE_VARIANTS names), SET_ORIGIN true and false
CORE_FORMS = {"table": ("core",), "lamb_notex": ("core", "core_lamb", "core_notex", "core_lamb_notex"),
              "mixed_notex": ("core", "core_notex")}


def write_scene(tmp_dir, name):
    path = os.path.join(str(tmp_dir), name + ".rtxs")
    with open(path, "w") as f:
        f.write(SCENES[name])
    return path


def image_size():
    with open(os.path.join(orc.TEXELS, "earthmap.ppm"), "rb") as f:
        tok = f.read(64).split()
    assert tok[0] == b"P6"
    return int(tok[1]), int(tok[2])


# ---- small helpers ----
def ulps(x, k):
    x = np.float64(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, np.inf if k > 0 else -np.inf)
    return float(x)


def unit_vectors(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def new_cases(n, mat, first_pixel):
    """n hits of `mat` (an id or an array) at depth 0 with throughput 1 1 1, keys (SEED, first_pixel + i, i % 7)."""
    c = orc.shade_cases(n)
    c["hit"], c["front_face"], c["mat"] = 1, 1, mat
    c["max_depth"] = MAX_DEPTH
    c["seed"] = SEED
    c["pixel"] = first_pixel + np.arange(n)
    c["sample"] = np.arange(n) % 7
    c["normal"] = (0.0, 1.0, 0.0)
    c["d"] = (0.3, -1.0, 0.2)
    c["o"] = (0.0, 5.0, 0.0)
    return c


def stream_draws(case, n):
    """The first n draws of the stream a wavefront-mode case shades from."""
    return orc.philox(int(case["seed"]), int(case["pixel"]), int(case["sample"]), n, stream=int(case["depth"]) + 1)


def unit_vector_of(draws):
    """random_unit_vector (RandomUnitVector: z, y, x drawn in that order, rejection) over `draws`."""
    for k in range(0, len(draws) - 2, 3):
        z, y, x = (-1.0 + 2.0 * draws[k + i] for i in range(3))
        l2 = x * x + y * y + z * z
        if 1e-12 < l2 <= 1.0:
            inv = 1.0 / np.sqrt(l2)
            return np.array([inv * x, inv * y, inv * z])
    raise AssertionError("no unit vector in the draws")


# ---- families ----
def sky_family():
    """Misses, and hits at depth == max_depth and depth > max_depth: every path ends on the sky."""
    rng = np.random.default_rng(1)
    u = unit_vectors(rng, 24)
    dirs = [(0, 1, 0), (0, -1, 0), (1, 0, 0), (0, 0, -1), (-0.6, 0, 0.8), (0, 0, 0), (0, 1e-3, 0), (0, -1e3, 0)]
    dirs += list(u[:8]) + list(1e-3 * u[8:16]) + list(1e3 * u[16:24])
    thrs = [(1, 1, 1), (0.5, 0, 2), (1e6, 3e5, 7e7)]
    ends = [(0, 0, 5), (0, 3, 5), (1, 5, 5), (1, 6, 5), (1, 0, 0), (1, 49, 7)]  # hit, depth, max_depth
    rows = [(d, t, e) for d in dirs for t in thrs for e in ends]
    c = new_cases(len(rows), 0, 1000)
    for i, (d, t, (hit, depth, md)) in enumerate(rows):
        c["d"][i], c["thr"][i] = d, t
        c["hit"][i], c["depth"][i], c["max_depth"][i] = hit, depth, md
        c["mat"][i] = (LAMB_SOLID, METALS[1], GLASS[0], LIGHT_SOLID)[i % 4]
    return dict(cases=c, lamb=np.zeros(len(c), bool))


def normals_at_09():
    """Normals whose normalized x is 0.9 and each of its two neighbouring doubles (the Lambertian
    basis switches at |w.x| > 0.9): found among (0.9 + j ulps, y0 + k ulps, 0), normalized as the
    step does."""
    out = {}
    y = np.sqrt(1.0 - 0.81) * (1.0 + np.arange(-400, 401) * 2.0 ** -52)[None, :]
    x = 0.9 * (1.0 + np.arange(-16, 17) * 2.0 ** -52)[:, None] + 0.0 * y
    l = np.sqrt(x * x + y * y + 0.0 * 0.0)
    wx = (1.0 / l) * x
    for target in (ulps(0.9, -1), 0.9, ulps(0.9, 1)):
        j, k = np.nonzero(wx == target)
        assert len(j), target
        for sx in (1.0, -1.0):
            out[(target, sx)] = (sx * float(x[j[0], k[0]]), float(y[0, k[0]]), 0.0)
    return out


def edge_keys(limit=100000):
    """Keys (pixel, sample 0, depth 0) whose r2 (the stream's second draw) is below 1e-4 or above
    1 - 1e-4: the grazing and the pdf edge of the cosine sampling.  At most `limit` keys are tried."""
    lo, hi = [], []
    for pixel in range(limit):
        r2 = orc.philox(SEED, pixel, 0, 2, stream=1)[1]
        if r2 < 1e-4:
            lo.append(pixel)
        elif r2 > 1 - 1e-4:
            hi.append(pixel)
        if len(lo) >= 3 and len(hi) >= 3:
            break
    return lo, hi


def lambertian_family():
    rng = np.random.default_rng(2)
    W, H = image_size()
    parts = []

    def add(n, mat, **f):
        c = new_cases(n, mat, 100000 + 4096 * len(parts))
        for k, v in f.items():
            c[k] = v
        parts.append(c)
        return c

    # normals x depths x roulette ranges, solid colour (albedo 0.8 0.3 0.1: q ~ 0.8 thr)
    axis = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    n09 = list(normals_at_09().values())
    u = unit_vectors(rng, 48)
    scaled = list(1e-3 * u[:6]) + list(7.5 * u[6:12]) + list(1e3 * u[12:18])
    normals = axis + n09 + scaled + list(u[18:])
    thrs = [(0.05, 0.05, 0.05), (0.6, 0.6, 0.6), (3, 3, 3)]  # q below 0.1, inside, above 0.95
    rows = [(n, d, t) for n in normals for d in (0, 4, 5, 6) for t in thrs]
    c = add(len(rows), LAMB_SOLID)
    for i, (n, d, t) in enumerate(rows):
        c["normal"][i], c["depth"][i], c["thr"][i] = n, d, t
    # the grazing and pdf edges
    lo, hi = edge_keys()
    assert lo and hi, "no key with r2 at an edge among the keys tried"
    c = add(len(lo + hi) * 3, LAMB_SOLID)
    c["pixel"], c["sample"] = np.repeat(lo + hi, 3), 0
    c["normal"] = np.tile(np.array([(0, 1, 0), (0.6, 0, -0.8), (-0.9, 0.1, 0.4)], float), (len(lo + hi), 1))
    n_edge = len(c)
    # checker of solids (scale 0.5): negative cells, an odd negative sum, p on a boundary and beside it
    b = [ulps(0.5, -1), 0.5, ulps(0.5, 1), ulps(-0.5, -1), -0.5, ulps(-0.5, 1), -0.0, 0.0, ulps(0.0, -1), ulps(0.0, 1)]
    ps = [(-0.3, -0.7, -1.2), (-0.3, 0.2, 0.2), (-0.3, -0.2, 0.2), (0.3, 0.2, 0.2), (-7.75, 3.25, -0.25)]
    ps += [(x, 0.1, 0.1) for x in b] + [(0.1, x, -0.1) for x in b] + [(-0.1, -0.1, x) for x in b]
    ps += list(rng.uniform(-3, 3, size=(40, 3)))
    for mat in (LAMB_CHECKER, LAMB_CHECKER2):
        c = add(len(ps), mat)
        c["p"] = np.array(ps, float)
    # image: u, v outside [0, 1], on texel boundaries, and inside; through a checker; a missing image
    uvs = [-0.5, 0.0, 1.0 / W, 7.0 / W, (W - 1.0) / W, 1.0, 1.5, 0.37]
    vvs = [-0.5, 0.0, 1.0 / H, 5.0 / H, (H - 1.0) / H, 1.0, 1.5, 0.61]
    grid = [(a, bb) for a in uvs for bb in vvs]
    for mat in (LAMB_IMAGE, LAMB_CHECKER_IMG, LAMB_MISSING):
        c = add(len(grid), mat)
        c["u"], c["v"] = np.array(grid).T
        c["p"] = rng.uniform(-3, 3, size=(len(grid), 3))
    # image through the deferred u, v of a sphere and of each rect kind (u, v of the case are decoys)
    m = 48
    c = add(m, LAMB_IMAGE, lazy_uv=SPHERE, u=0.123, v=0.456)
    cx, cy, cz, r = SPHERE_G
    c["p"] = np.array([cx, cy, cz]) + r * unit_vectors(rng, m)
    for prim, (a0, a1, b0, b1, k) in RECTS_G.items():
        c = add(m, LAMB_IMAGE, lazy_uv=prim, u=0.123, v=0.456)
        s, t = rng.uniform(a0, a1, m), rng.uniform(b0, b1, m)
        s[:4], t[:4] = (a0, a1, a0, a1), (b0, b0, b1, b1)  # the corners: u, v exactly 0 and 1
        kk = np.full(m, k)
        c["p"] = np.stack({RECT_XY: (s, t, kk), RECT_XZ: (s, kk, t), RECT_YZ: (kk, s, t)}[prim], 1)
    cases = np.concatenate(parts)
    return dict(cases=cases, lamb=np.ones(len(cases), bool), n_edge=n_edge)


def incidence(theta_deg, phi_deg, scale=1.0):
    """A direction arriving on the plane y = 0 (normal 0 1 0) at theta from the normal."""
    t, p = np.radians(theta_deg), np.radians(phi_deg)
    return scale * np.array([np.sin(t) * np.cos(p), -np.cos(t), np.sin(t) * np.sin(p)])


def metal_family():
    """Fuzz 0, 0.3, 1 and 1.7 (clamped), incidence from normal to grazing, non-unit directions,
    depths below and above the roulette's start.  fuzzed: the rows whose fuzz is not 0."""
    thetas = (0.0, 30.0, 60.0, 80.0, 85.0, 88.0, 89.5, 89.99)
    rows = [(m, th, k) for m in METALS for th in thetas for k in range(24)]
    c = new_cases(len(rows), 0, 300000)
    for i, (m, th, k) in enumerate(rows):
        c["mat"][i] = m
        c["d"][i] = incidence(th, 37.0 * k, scale=(1.0, 1e-3, 1e3, 2.5)[k % 4])
        c["depth"][i] = (0, 6)[k % 2]
        c["thr"][i] = ((1, 1, 1), (0.3, 0.9, 0.05))[(k // 2) % 2]
    return dict(cases=c, lamb=np.zeros(len(c), bool), fuzzed=c["mat"] != METALS[0])


def sin_theta_t(d, n, eta):
    """st = eta * sqrt(max(0, 1 - ci^2)) of the dielectric step, in its operations: the direction
    normalized twice (wo = -normalize(d), win = -normalize(wo)), ci = dot(win, n) clamped."""
    def normalize(v):
        l = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
        inv = 1.0 / l
        return [inv * v[0], inv * v[1], inv * v[2]]
    w = normalize(normalize(d))
    ci = np.clip(w[0] * n[0] + w[1] * n[1] + w[2] * n[2], -1.0, 1.0)
    return eta * np.sqrt(np.maximum(0.0, 1.0 - ci * ci))


def critical_directions(eta):
    """Directions (x, -1, 0) onto the normal (0, 1, 0), for eta > 1, at the test st >= 1.0: the two
    largest values of st below 1.0 that the step's arithmetic reaches, 1.0 itself where it reaches
    it, and the two smallest above (st = eta * sqrt(1 - ci^2) does not reach every double: for eta
    1.5 its values lie 1.5 ulps apart).  Scanned a few thousand ulps around tan(theta_c).  Returns
    the directions and whether 1.0 itself is among them."""
    x0 = (1.0 / eta) / np.sqrt(1.0 - 1.0 / (eta * eta))
    x = x0 * (1.0 + np.arange(-4000, 4001) * 2.0 ** -52)
    st = sin_theta_t([x, np.full_like(x, -1.0), np.zeros_like(x)], (0.0, 1.0, 0.0), eta)
    values = np.unique(st)
    below, above = values[values < 1.0][-2:], values[values > 1.0][:2]
    assert len(below) == 2 and len(above) == 2 and 1.0 - below[0] < 4e-15 and above[1] - 1.0 < 4e-15
    out = []
    for target in list(below) + [1.0] + list(above):
        k = np.nonzero(st == target)[0]
        out += [(float(x[j]), -1.0, 0.0) for j in k[:2]]
    return out, bool((st == 1.0).any())


def dielectric_family():
    """ri 1.5, 1.0, 2.4 and 1 / 1.5, front and back face: normal incidence with ci exactly -1 and
    +1, grazing incidence, the critical angle and the doubles around st == 1.0 on both sides,
    non-unit and zero-length directions.  All below depth 5, so the draws consumed tell a total
    internal reflection (none) from a Fresnel decision (one): outcome()."""
    rows = []  # mat, front_face, d
    exact = []  # the etas whose st reaches 1.0 itself
    for m, ri in zip(GLASS, GLASS_RI):
        for ff in (1, 0):
            eta = 1.0 / ri if ff else ri
            ds = [(0, -1, 0), (0, 1, 0), (0, -2.5, 0), (0, 0, 0), (-0.0, -0.0, -0.0)]
            ds += [incidence(th, 20.0 * j, scale=(1.0, 1e-3, 1e3)[j % 3]) for j, th in
                   enumerate((5, 20, 35, 41, 43, 50, 60, 70, 80, 87, 89.9, 89.9999))]
            if eta > 1.0:
                crit, at_one = critical_directions(eta)
                ds += crit
                exact += [eta] * at_one
            for d in ds:
                rows += [(m, ff, d)] * 6  # six keys each: both sides of the Fresnel decision
    assert exact, "no eta reaches st == 1.0 exactly"
    c = new_cases(len(rows), 0, 500000)
    for i, (m, ff, d) in enumerate(rows):
        c["mat"][i], c["front_face"][i], c["d"][i] = m, ff, d
        c["depth"][i] = i % 5
        c["thr"][i] = ((1, 1, 1), (0.3, 0.9, 0.05))[i % 2]
    return dict(cases=c, lamb=np.zeros(len(c), bool))


def dielectric_outcomes(cases, records):
    """'tir', 'reflect' or 'refract' per row of the dielectric family, from the oracle's records."""
    out = []
    for c, r in zip(cases, records):
        assert r["cont"] == 1 and c["depth"] < 5
        d0, d1 = stream_draws(c, 2)
        assert r["next"] in (d0, d1)
        if r["next"] == d0:
            out.append("tir")
        elif GLASS_RI[GLASS.index(c["mat"])] != 1.0:  # a refraction scales the throughput by eta^2
            out.append("reflect" if np.array_equal(r["thr"], c["thr"]) else "refract")
        else:  # ri 1: by the side the child leaves on
            out.append("refract" if np.dot(r["d"], c["normal"]) < 0 else "reflect")
    return np.array(out)


def emitter_family():
    """Front and back face; a solid, a checker (a bright and a near_zero cell) and an image emission;
    an emission that is near_zero (a dead path); a light hit at the depth limit (the sky)."""
    rng = np.random.default_rng(5)
    W, H = image_size()
    rows = []
    for ff in (1, 0):
        for depth, md in ((0, 50), (7, 50), (5, 5), (6, 5)):
            for mat in (LIGHT_SOLID, LIGHT_DIM):
                rows += [(mat, ff, depth, md, (0.1, 0.2, 0.3), 0.0, 0.0)] * 2
            for p in [(0.1, 0.1, 0.1), (0.3, 0.1, 0.1), (-0.1, 0.1, 0.1), (-0.3, -0.3, -0.3)] + list(rng.uniform(-2, 2, (6, 3))):
                rows.append((LIGHT_CHECKER, ff, depth, md, p, 0.0, 0.0))
            for u, v in [(-0.5, 0.5), (0.0, 1.0), (3.0 / W, 2.0 / H), (1.5, -0.5), (0.37, 0.61), (0.9, 0.2)]:
                rows.append((LIGHT_IMAGE, ff, depth, md, (0.0, 0.0, 0.0), u, v))
    c = new_cases(len(rows), 0, 700000)
    for i, (mat, ff, depth, md, p, u, v) in enumerate(rows):
        c["mat"][i], c["front_face"][i], c["depth"][i], c["max_depth"][i] = mat, ff, depth, md
        c["p"][i], c["u"][i], c["v"][i] = p, u, v
        c["thr"][i] = ((1, 1, 1), (0.25, 0.0, 3.0))[i % 2]
    return dict(cases=c, lamb=np.zeros(len(c), bool))


FAMILIES = {"sky": sky_family, "lambertian": lambertian_family, "metal": metal_family,
            "dielectric": dielectric_family, "emitter": emitter_family}
_family_cache = {}


def family(name):
    """A family, built once and left unchanged."""
    if name not in _family_cache:
        f = FAMILIES[name]()
        f["cases"].setflags(write=False)
        _family_cache[name] = f
    return _family_cache[name]


def sky_end(cases):
    """Rows whose path ends on the sky: a miss, or a segment at the depth limit."""
    return (cases["hit"] == 0) | (cases["depth"] >= cases["max_depth"])


def scatter_form(cases):
    """The same cases for the scatter API: depth is the remaining depth (the stream stays
    max_depth - depth + 1); rows at the depth limit are left out (GetPixel returns before it traces)."""
    c = cases[cases["depth"] < cases["max_depth"]].copy()
    c["depth"] = c["max_depth"] - c["depth"]
    return c


def scatter_fallback_cases(n=16):
    """Scatter-API Lambertian cases whose normal is exactly minus the unit vector their key draws:
    normal + random_unit_vector is 0 0 0, near_zero, and the direction falls back to the normal."""
    c = new_cases(n, LAMB_SOLID, 900000)
    for i in range(n):
        c["normal"][i] = -unit_vector_of(stream_draws(c[i], 60))
    return scatter_form(c)


def mixed_notex_cases():
    """Cases for the MIXED_NOTEX table (materials 0..3: Lambertian, metal, glass, light)."""
    rng = np.random.default_rng(7)
    n = 512
    c = new_cases(n, np.arange(n) % 4, 1100000)
    c["normal"] = unit_vectors(rng, n)
    d = unit_vectors(rng, n)
    d[np.sum(d * c["normal"], 1) > 0] *= -1.0  # arriving against the normal
    c["d"] = d * rng.choice([1.0, 1e-3, 40.0], n)[:, None]
    c["front_face"] = rng.integers(0, 2, n)
    c["depth"] = rng.choice([0, 4, 5, 6, 50], n)
    c["hit"] = rng.random(n) > 0.05
    c["p"] = rng.uniform(-3, 3, (n, 3))
    c["thr"] = rng.choice([0.05, 0.6, 3.0], (n, 1)) * np.ones(3)
    return c, (c["mat"] == 0)


def lamb_notex_cases():
    """Cases for the LAMB_NOTEX table (two solid Lambertians)."""
    rng = np.random.default_rng(8)
    n = 512
    c = new_cases(n, np.arange(n) % 2, 1200000)
    c["normal"] = unit_vectors(rng, n) * rng.choice([1.0, 1e-3, 40.0], n)[:, None]
    c["depth"] = rng.choice([0, 4, 5, 6, 50], n)
    c["hit"] = rng.random(n) > 0.05
    c["p"] = rng.uniform(-3, 3, (n, 3))
    c["thr"] = rng.choice([0.05, 0.6, 3.0], (n, 1)) * np.ones(3)
    return c, np.ones(n, bool)


# ---- comparison ----
def rows(records):
    """Records as bytes, one row each: equality of rows is equality bit for bit, NaNs included."""
    r = np.ascontiguousarray(records)
    return r.view(np.uint8).reshape(len(r), r.dtype.itemsize)


def same(a, b):
    return (rows(a) == rows(b)).all(1)


def oracle_nudged(scene, cases):
    """The oracle's records under each of the 25 cos / sin nudges, {(dc, ds): records}."""
    out = {}
    try:
        for dc, ds in NUDGES:
            orc.set_cos_sin_nudge(dc, ds)
            out[(dc, ds)] = orc.shade_steps(scene, cases)
    finally:
        orc.set_cos_sin_nudge(0, 0)
    return out


def mismatches(got, nudged, lamb):
    """Rows of `got` that break the step-level rule against the oracle's records (oracle_nudged),
    and the histogram {nudge: rows} of the Lambertian rows that continue.  The rule: a record equals
    the oracle's 0 / 0 record bit for bit; a Lambertian sample that continues may instead equal, as
    a whole record, the oracle's under one nudge of at most 2 ulps each; its flag, depth and next
    draw equal the 0 / 0 record's in any case."""
    base = nudged[(0, 0)]
    free = lamb & (base["cont"] == 1)
    bad = ~same(got, base) & ~free
    for k in ("cont", "depth", "next"):
        bad |= (rows(got[k]) != rows(base[k])).any(1)
    hist = {}
    todo = free.copy()
    for nd in NUDGES:
        hit = todo & same(got, nudged[nd])
        if hit.any():
            hist[nd] = int(hit.sum())
        todo &= ~hit
    bad |= todo
    return bad, hist
