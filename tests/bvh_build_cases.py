"""Crafted box sets for the BVH builders (tests/test_bvh_build_host.py on the CPU,
tests/test_bvh_build.py on the GPU).  No GPU and no library here: numpy only, closed forms and
fixed seeds.  Every family is a function returning [(name, bounds[n, 6] float64)], n <= 1100,
each aimed at one place where the device build (csrc/rtx_bvh_build.hip) can leave the host
builder's bytes: its 256-thread chunk loop, the four-wave reductions, the rank arithmetic of the
two-ended partition, first-wins ties, bin rounding and deep chains.

Most boxes are written in the exact form of a primitive's bounding box, so that the same case
can be loaded as an .rtxs scene (scene_text) and the host builder compared with the oracle:
  * rect(): the box of `rect xy a0 a1 b0 b1 0`: x and y are the caller's doubles exactly
    (-0.0 included), z is (0 - 0.0001, 0 + 0.0001), so every centroid has z = 0;
  * cube(): the box of `sphere cx cy cz r` with c +- r exact in binary.
"""
import numpy as np

FAMILIES = ["root_sizes", "partition_T", "cost_ties", "axis_ties", "bin_edges", "signed_zero_positions", "chains",
            "magnitudes", "odd_boxes"]
THICK = 0.0001  # half thickness of an axis rect's box (rect.h)
NEXT = np.nextafter


def rect(x0, x1, y0, y1):
    """Boxes of `rect xy x0 x1 y0 y1 0` (arrays or scalars, x0 <= x1, y0 <= y1)."""
    x0, x1, y0, y1 = np.broadcast_arrays(*[np.atleast_1d(np.asarray(v, np.float64)) for v in (x0, x1, y0, y1)])
    z = np.full(x0.shape, THICK)
    return np.stack([x0, y0, 0.0 - z, x1, y1, 0.0 + z], axis=1)


def cube(c, r):
    """Boxes of spheres with centres c[n, 3] and radius r (scalar or [n])."""
    c = np.asarray(c, np.float64).reshape(-1, 3)
    r = np.broadcast_to(np.asarray(r, np.float64).reshape(-1, 1), c.shape)
    return np.concatenate([c - r, c + r], axis=1)


def points_on_line(x, h=2.0 ** -10):
    """Tiny rect boxes whose centroids are exactly x (zero width in x, +-h in y)."""
    x = np.asarray(x, np.float64)
    return rect(x, x, -h, h)


def turn(bounds, axes):
    """The same boxes with the axes permuted: new axis a takes old axis axes[a]."""
    b = np.asarray(bounds)
    return np.concatenate([b[:, list(axes)], b[:, [3 + a for a in axes]]], axis=1)


def centroids(bounds):
    b = np.asarray(bounds, np.float64)
    return 0.5 * (b[:, :3] + b[:, 3:])  # Aabb::center()


# ------------------------------------------------------------------------------------------
def root_sizes():
    """Root ranges around the wave (64) and chunk (256) sizes: centroids 0..n-1 on a line, in a
    seeded shuffle, so that the root's partition swaps in every chunk."""
    out = []
    for n in (5, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1025):
        x = np.random.default_rng(n).permutation(n).astype(np.float64)
        out.append((f"line_n{n}", points_on_line(x)))
    return out


PARTITION_N = (257, 600)
PARTITION_T = (1, 2, 63, 64, 65, 255, 256, 257)


def partition_T_values(n):
    return sorted({t for t in PARTITION_T + (n - 2, n - 1) if 1 <= t <= n - 1})


def two_clusters(n, T, order):
    """T centroids near x = 0 (bin 0 of the root) and n - T near x = 100 (bin 15): every split
    plane of the root costs the same, the first (split 0) wins, and T primitives go left.
    order: asc (left cluster first: no swaps), desc (right cluster first: min(T, n - T) swaps),
    alt (right, left, right, ... until the smaller cluster runs out, then the rest)."""
    left = [j * 2.0 ** -8 for j in range(T)]
    right = [100.0 + j * 2.0 ** -8 for j in range(n - T)]
    if order == "asc":
        x = left + right
    elif order == "desc":
        x = right + left
    else:
        m = min(T, n - T)
        x = [v for pair in zip(right[:m], left[:m]) for v in pair] + right[m:] + left[m:]
    return points_on_line(x)


def partition_T():
    return [(f"n{n}_T{T}_{order}", two_clusters(n, T, order)) for n in PARTITION_N for T in partition_T_values(n)
            for order in ("asc", "desc", "alt")]


def partition_T_target(name):
    """T of a partition_T case; its left set is the primitives whose centroid x is below 50."""
    return int(name.split("_")[1][1:])


def cost_ties():
    """Equal SAH costs at several planes of the root (`cost < best` keeps the first).
    mirror_*: boxes symmetric about x = 0 with a power-of-two extent, so the split after bin i
    and the split after bin 14 - i see mirrored halves; lattice_*: empty bins between occupied
    ones, so adjacent planes separate the same two sets."""
    out = []
    # four clusters of cubes at x = -8, -0.5, 0.5, 8 (bins 0, 7, 8, 15)
    for m in (2, 5):
        c = [(sx * ax, 0.25 * j, 0.0) for ax in (8.0, 0.5) for sx in (-1.0, 1.0) for j in range(m)]
        out.append((f"mirror_cubes_m{m}", cube(c, 0.125)))
    # a symmetric line: three points at either end and a pair about the centre
    out.append(("mirror_line", points_on_line([-8.0, 0.5, 7.5, -7.0, 8.0, -0.5, 7.0, -7.5])))
    # two far clusters and a symmetric pair close to the centre
    x = np.concatenate([np.full(6, -8.0), [-1.5, 1.5], np.full(6, 8.0)])
    y = np.concatenate([np.arange(6.0), [0.0, 0.0], np.arange(6.0)]) * 2.0 ** -4
    out.append(("mirror_rects", rect(x - 0.25, x + 0.25, y, y + 0.5)))
    for k in (3, 4, 6):  # k x k lattice over a 12 x 12 square: k occupied bins, gaps between
        g = np.arange(k) * (12.0 / (k - 1))
        xx, yy = np.meshgrid(g, g, indexing="ij")
        out.append((f"lattice_{k}x{k}", rect(xx.ravel() - 0.25, xx.ravel() + 0.25, yy.ravel() - 0.25,
                                             yy.ravel() + 0.25)))
    return out


def axis_ties():
    """Equal centroid extents: LongestAxis takes x when dx >= dy and dx >= dz, else y when
    dy >= dz.  Cubes on an integer lattice: centroids and extents are exact."""
    out = []
    for name, dims in (("dx_eq_dy_eq_dz", (2, 2, 2)), ("dx_eq_dy_gt_dz", (4, 4, 2)), ("dy_eq_dz_gt_dx", (2, 4, 4)),
                       ("dx_eq_dz_gt_dy", (4, 2, 4))):
        g = np.stack(np.meshgrid(*[np.arange(0, d + 1, 2 if d == 4 else 1) for d in dims], indexing="ij"),
                     axis=-1).reshape(-1, 3).astype(np.float64)
        g = g[np.random.default_rng(7).permutation(len(g))]
        out.append((name, cube(g, 0.25)))
    return out


AXIS_TIE_AXIS = {"dx_eq_dy_eq_dz": 0, "dx_eq_dy_gt_dz": 0, "dy_eq_dz_gt_dx": 1, "dx_eq_dz_gt_dy": 0}


def bin_edges():
    """Centroids exactly on the 17 bin edges mn + extent * k / 16 of a power-of-two extent, and
    one ulp to either side of each (not outside the ends, which would move the extent)."""
    out = []
    for tag, mn, extent in (("1_2", 1.0, 1.0), ("m4_4", -4.0, 8.0), ("0_eighth", 0.0, 0.125), ("m1024_0", -1024.0,
                                                                                              1024.0)):
        edges = mn + extent * np.arange(17) / 16.0
        x = np.concatenate([edges, NEXT(edges[:-1], np.inf), NEXT(edges[1:], -np.inf)])
        x = x[np.random.default_rng(17).permutation(len(x))]
        b = points_on_line(x)
        out.append((f"x_{tag}", b))
        out.append((f"y_{tag}", turn(b, (1, 0, 2))))
    out.append(("z_1_2", turn(out[0][1], (2, 1, 0))))  # thin in x: a yz rect
    return out


ZERO_N = 300
ZERO_POSITIONS = (0, 1, 63, 64, 255, 256, ZERO_N - 1)


def signed_zero_positions():
    """All 300 boxes share a zero bound (lo y, or hi y); the box at input position p carries the
    other sign of zero.  In the root, p sits on a wave or chunk boundary and must lose to
    position 0 (for p = 0 it wins).  Positions [0, p) lie near x = 0 and [p, n) near x = 100,
    so the root splits between them and p is the first primitive of the right child, where its
    sign is the one that reaches the node's box."""
    out = []
    n = ZERO_N
    for p in ZERO_POSITIONS:
        x = np.array([(0.0 if i < p else 100.0) + i * 2.0 ** -8 for i in range(n)])
        for which in ("lo", "hi"):
            for odd in (-0.0, 0.0):
                zero = np.full(n, -odd)
                zero[p] = odd
                b = rect(x, x, zero, 1.0) if which == "lo" else rect(x, x, -1.0, zero)
                out.append((f"{which}_p{p}_odd{'neg' if np.signbit(odd) else 'pos'}", b))
    return out


def without_odd_sign(bounds):
    """A signed_zero_positions case with the one odd zero given the sign of the others."""
    b = np.array(bounds)
    for c in range(6):
        if np.all(b[:, c] == 0.0):
            neg = np.signbit(b[:, c])
            b[:, c] = -0.0 if neg.sum() * 2 > len(b) else 0.0
    return b


def chain(n, mirrored=False, form="rect"):
    """Centroids at 2^i with boxes of half size 2^(i-2): self-similar, so every level peels the
    few largest primitives off one end and the tree is a chain.  The many small primitives
    near 0 fall into bin 0, so the deep side is the left child; mirrored: centroids at -2^i, they
    fall into bin 15 and the deep side is the right child."""
    c = 2.0 ** np.arange(n)
    r = 0.25 * c
    if mirrored:
        c = -c
    if form == "cube":
        return cube(np.stack([c, np.zeros(n), np.zeros(n)], axis=1), r)
    return rect(c - r, c + r, -r, r)


def chains():
    out = []
    for n in (40, 300):
        out.append((f"n{n}_left", chain(n)))
        out.append((f"n{n}_right", chain(n, mirrored=True)))
        out.append((f"n{n}_left_cubes", chain(n, form="cube")))
        out.append((f"n{n}_right_reversed", chain(n, mirrored=True)[::-1].copy()))
    return out


INV_INF_EXTENTS = (1e-310, 4e-309)


def inv_inf(n, extent):
    """n centroids evenly over a subnormal extent below 2^-1024: 1 / extent is +inf, and
    (c - mn) * inv * 16 is NaN for the smallest centroid and +inf for all others.  The rule that
    sends both to bin 0 makes the root a leaf.  A conversion that saturates +inf (bin 15) would
    split the smallest centroid's box from the rest, and that box is four times as tall as the
    others so that such a split would pass the cost test (inv_inf_stray_split_cost)."""
    tiny = 2.0 ** -1074
    step = max(1, round(extent / tiny / (n - 1)))
    x = (np.arange(n) * step).astype(np.float64) * tiny  # exact multiples of the smallest subnormal
    h = np.where(x == 0.0, 1.0, 0.25)
    order = np.roll(np.arange(n), n // 2)  # the smallest centroid sits mid-array
    return rect(x, x, -h, h)[order]


def inv_inf_stray_split_cost(bounds):
    """SAH cost (the builder's formula) of splitting the smallest centroid's box from the rest."""
    b = np.asarray(bounds)
    first = centroids(b)[:, 0] == centroids(b)[:, 0].min()

    def area(q):
        dx, dy, dz = (float(v) for v in q[:, 3:].max(0) - q[:, :3].min(0))
        return 2.0 * (dx * dy + dy * dz + dz * dx)

    return 1.0 + area(b[first]) / area(b) * int(first.sum()) + area(b[~first]) / area(b) * int((~first).sum())


def magnitudes():
    """Huge, tiny and subnormal coordinates.  Every bound and every lo + hi is finite."""
    out = []
    rng = np.random.default_rng(300)
    for n in (9, 300):
        x = 1e300 * (1.0 + rng.random(n))
        y = 1e300 * (1.0 + rng.random(n))
        out.append((f"huge_n{n}", rect(x, x * (1 + 2.0 ** -20), y, y * (1 + 2.0 ** -20))))  # areas overflow
        c = 1e-300 * (1.0 + rng.random((n, 3)))
        out.append((f"tiny_n{n}", np.concatenate([c, c * (1 + 2.0 ** -20)], axis=1)))  # areas underflow to 0
        for extent in INV_INF_EXTENTS:
            out.append((f"inv_inf_{extent:g}_n{n}", inv_inf(n, extent)))
    wide = np.array([[-1.7e308] * 3 + [1.7e308] * 3] * 6)  # lo + hi = 0: finite centroids
    wide[:, 0] += np.arange(6) * 1e305
    out.append(("full_range_n6", wide))
    return out


def is_inv_inf(name):
    return name.startswith("inv_inf_")


def odd_boxes():
    out = []
    rng = np.random.default_rng(5)
    p = rng.integers(-8, 9, (100, 3)).astype(np.float64)
    out.append(("points_n100", np.concatenate([p, p], axis=1)))  # zero-size boxes
    xy = rng.integers(-8, 9, (100, 2)).astype(np.float64)
    out.append(("flat_points_n100", rect(xy[:, 0], xy[:, 0], xy[:, 1], xy[:, 1])))
    c = rng.random((300, 3)) * 10
    e = rng.random((300, 3)) + 0.125
    out.append(("inverted_n300", np.concatenate([c + e, c - e], axis=1)))  # lo > hi
    mixed = np.concatenate([c - e, c + e], axis=1)
    mixed[::3] = out[-1][1][::3]
    out.append(("some_inverted_n300", mixed))
    out.append(("identical_n300", np.repeat(rect(1.0, 2.0, -0.0, 3.0), 300, axis=0)))
    five = np.repeat(cube([[1.0, 2.0, 3.0]], 0.5), 5, axis=0)
    for k in (0, 2, 4):
        b = five.copy()
        b[k] = cube([[5.0, 2.0, 3.0]], 0.5)[0]
        out.append((f"four_same_one_other_at{k}", b))
    return out


def family(name):
    return globals()[name]()


def case_ids(name):
    return [c[0] for c in family(name)]


# ------------------------------------------------------------------------------------------
HEADER = "rtxscene 1\nbvh 1\ntex 0 solid 0.5 0.5 0.5\nmat 0 lambertian 0\n"


def scene_text(bounds):
    """The .rtxs scene whose primitives have exactly these boxes, in this order, or None if the
    boxes are neither all rect() boxes (about any one axis) nor all cube() boxes."""
    b = np.asarray(bounds, np.float64)
    r = repr
    for ax, kw, (a, c) in ((2, "xy", (0, 1)), (1, "xz", (0, 2)), (0, "yz", (1, 2))):
        if np.all(b[:, ax] == -THICK) and np.all(b[:, 3 + ax] == THICK) and np.all(b[:, [a, c]] <= b[:, [3 + a, 3 + c]]):
            return HEADER + "".join(f"rect {kw} {r(float(q[a]))} {r(float(q[3 + a]))} {r(float(q[c]))} "
                                    f"{r(float(q[3 + c]))} 0.0 0\n" for q in b)
    with np.errstate(over="ignore"):
        ctr, rad = 0.5 * (b[:, :3] + b[:, 3:]), 0.5 * (b[:, 3] - b[:, 0])
    rr = rad[:, None]
    if np.all(rad > 0) and np.all(np.isfinite(ctr)) and np.array_equal(ctr - rr, b[:, :3]) and np.array_equal(
            ctr + rr, b[:, 3:]):
        return HEADER + "".join(f"sphere {r(float(c[0]))} {r(float(c[1]))} {r(float(c[2]))} {r(float(q))} 0\n"
                                for c, q in zip(ctr, rad))
    return None
