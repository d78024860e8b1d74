"""The fast BVH4 tree and the traversal stacks, on small and degenerate trees.

rtx_scene_create builds the fast path's tree on the host (build_global_prims, build_own_sah,
build_fast4 in csrc/rtx_capi.hip) and sizes both walks' LDS stacks (pick_stack, the exact
bound `need`); the kernels trust all of it unchecked.  The first half of this file inspects
that plan on the CPU through the host-only hook rtx.fast_tree, against plain numpy / float64
restatements of what it promises: the partition of the primitives, outward-rounded boxes, the
node layout and both stack bounds.  The second half (marked gpu) traces rays through the
smallest scenes that sit on each boundary and compares parity, fast and the CPU oracle's
brute force over a `bvh 0` copy of the same scene, bit for bit.

Boundary scenes.  The "geometric line" (n spheres at x = ratio^k, radius proportional to x)
makes the binned SAH peel a few spheres per level, so the collapsed tree's exact stack bound
grows with n.  With ratio 1.25 the hook finds (LINES below, asserted by
test_line_scenes_sit_on_the_stack_boundaries, so a change of the builder announces itself):

    n = 138 -> need 32    n = 142 -> need 33    n = 295 -> need 64    n = 300 -> need 65

(the STACK = 32 / 64 steps and the fall-back to the parity walk; the reference-layout tree of
all four is at most 39 levels deep, so the parity walk itself stays available).  The parity
walk's own bound is exercised by hand-made caterpillar trees of D = 30, 31, 62 and 63 levels
(pick_stack: 32, 64, 64, refused).
"""
import ctypes as C
import sys

import numpy as np
import pytest

from conftest import scene_path

HDR = ["rtxscene 1", "tex 0 solid 0.5 0.5 0.5", "tex 1 solid 0.9 0.2 0.1", "mat 0 lambertian 0", "mat 1 lambertian 1",
       "mat 2 metal 0.8 0.8 0.8 0.0"]
SPHERE, TRIANGLE, XY, XZ, YZ = 0, 1, 2, 3, 4
COLS = [0, 1, 2, 3, 4, 5, 6, 7, 10, 11]  # hit t p3 n3 front_face material (u, v left out: acos / atan2)
LINE_RATIO = 1.25
LINES = {"line32": (138, 32), "line33": (142, 33), "line64": (295, 64), "line65": (300, 65)}  # name: (n, need)
CHAIN_STACK = {30: 32, 31: 64, 62: 64, 63: -1}  # levels D -> pick_stack


# ---------------------------------------------------------------------------------------
# Scenes: text lines of primitives (written with `bvh 1` for the product and `bvh 0` for the
# oracle's brute force), plus, for the hand-made trees, a node array of our own
# ---------------------------------------------------------------------------------------
def sphere(x, y, z, r, m=0):
    return "sphere %r %r %r %r %d" % (float(x), float(y), float(z), float(r), m)


def line_prims(n, ratio=LINE_RATIO):
    """n spheres at x = ratio^k with radius proportional to x; neighbours stay apart by half
    the gap between their centres."""
    rf = 0.5 * (ratio - 1) / (ratio + 1)
    return [sphere(ratio ** k, 0, 0, rf * ratio ** k, k % 3) for k in range(n)]


def spheres_prims(n):
    return [sphere(3.0 * k, 0.25 * k, -0.5 * k, 1.0 + 0.125 * k, k % 3) for k in range(n)]


def coincident_prims():
    return [sphere(0.1, 1 / 3, -2.0, 0.75, 1)] * 50 + [sphere(4, 0, 0, 1, 0), sphere(-4, 0.5, 1, 1.25, 2),
                                                        sphere(0, 5, 0, 0.5, 0)]


def rect_plane_prims():
    return ["rect xz %r %r %r %r 0.1 %d" % (1.5 * i, 1.5 * i + 1.25, 1.5 * j, 1.5 * j + 1.25, (i + j) % 3)
            for i in range(8) for j in range(8)]


def triangle_prims():
    """40 triangles: regular ones, zero-area ones (three collinear or identical vertices), ones
    with a repeated vertex and slivers, on coordinates that round-to-nearest would move inward
    in f32 (0.1, 1/3, 1000.3, -1e-3), signed zeros and an f32 denormal (1e-40)."""
    rng = np.random.default_rng(3)
    vals = [0.1, 1 / 3, 1000.3, -1e-3, 0.0, -0.0, 1e-40, 2.7, -5.3, 7.1]
    out = []
    for i in range(40):
        a, b, c = (np.array([vals[j] for j in rng.integers(0, len(vals), 3)]) for _ in range(3))
        base = np.array([12.0 * (i % 5), 9.0 * (i // 5), 0.0]) if i % 4 else np.zeros(3)
        a, b, c = a + base, b + base, c + base
        if i % 8 == 1:
            c = a + 2.0 * (b - a)  # collinear: zero area
        elif i % 8 == 3:
            c = b.copy()  # repeated vertex
        elif i % 8 == 5:
            b, c = a.copy(), a.copy()  # a point
        elif i % 8 == 7:
            c = a + (b - a) * 0.5 + np.array([0.0, 1e-7, 0.0])  # sliver
        out.append("tri " + " ".join(repr(float(v)) for v in np.concatenate([a, b, c])) + " %d" % (i % 3))
    return out


FILE_SCENES = {
    **{"spheres%d" % n: (lambda n=n: spheres_prims(n)) for n in (1, 2, 3, 4, 5)},
    "coincident50": coincident_prims,
    "rect_plane": rect_plane_prims,
    "triangles": triangle_prims,
    "negative_radius": lambda: spheres_prims(5) + [sphere(-6, 1, 2, -1.5, 1)],
    "ground2": lambda: [sphere(0, -1000, 0, 1000, 0), sphere(0, 1, 0, 1, 1), sphere(3, 0.5, 1, 0.5, 2)],
    **{name: (lambda n=n: line_prims(n)) for name, (n, _) in LINES.items()},
}
STOCK = ["three", "cornell", "final", "bunny", "mixed"]


def write_scene(path, prims, bvh):
    with open(path, "w") as f:
        f.write("\n".join([HDR[0], "bvh %d" % bvh] + HDR[1:] + list(prims)) + "\n")
    return str(path)


def parse_prims(rtx, lines):
    """The sphere lines as the C ABI's primitive records (hand-made trees hold spheres only)."""
    out = np.zeros(len(lines), rtx.PRIM_DTYPE)
    for i, ln in enumerate(lines):
        w = ln.split()
        assert w[0] == "sphere"
        out[i]["kind"], out[i]["material"] = SPHERE, int(w[5])
        out[i]["g"][:4] = [float(v) for v in w[1:5]]
    return out


class TreeScene:
    """A scene description with a hand-made reference-layout tree: quacks like rtx.HostScene
    for rtx.DeviceScene and rtx.fast_tree (.desc()) and for the checks here (.arrays()).
    `shape` is a nested pair structure whose leaves are primitive indices."""

    def __init__(self, rtx, prim_lines, shape):
        self.rtx = rtx
        self.prims = parse_prims(rtx, prim_lines)
        box = np.column_stack([self.prims["g"][:, :3] - np.abs(self.prims["g"][:, 3:4]),
                               self.prims["g"][:, :3] + np.abs(self.prims["g"][:, 3:4])])
        nodes = []

        def emit(s):  # pre-order: a node's children follow it
            me = len(nodes)
            nodes.append(None)
            if isinstance(s, tuple):
                l, r = emit(s[0]), emit(s[1])
                lo = np.minimum(nodes[l][0], nodes[r][0])
                hi = np.maximum(nodes[l][1], nodes[r][1])
                nodes[me] = (lo, hi, l, r, 0)
            else:
                nodes[me] = (box[s, :3], box[s, 3:], s, 1, 1)
            return me

        old = sys.getrecursionlimit()
        sys.setrecursionlimit(max(old, 10_000))
        try:
            emit(shape)
        finally:
            sys.setrecursionlimit(old)
        self.nodes = np.zeros(len(nodes), rtx.NODE_DTYPE)
        for i, (lo, hi, a, b, leaf) in enumerate(nodes):
            self.nodes[i] = (lo, hi, a, b, leaf, 0)
        self.mats = (rtx.Material * 3)()
        self.texs = (rtx.Texture * 2)()
        for t, col in zip(self.texs, ((0.5, 0.5, 0.5), (0.9, 0.2, 0.1))):
            t.kind, t.even, t.odd, t.image, t.inv_scale = 0, -1, -1, -1, 1.0
            t.color[:] = col
        for i, m in enumerate(self.mats):
            m.kind, m.texture = (0, i) if i < 2 else (1, -1)
            m.albedo[:] = (0.8, 0.8, 0.8)

    def desc(self):
        d = self.rtx.SceneDesc()
        d.prims = self.prims.ctypes.data_as(C.POINTER(self.rtx.Prim))
        d.n_prims = len(self.prims)
        d.nodes = self.nodes.ctypes.data_as(C.POINTER(self.rtx.BvhNode))
        d.n_nodes = len(self.nodes)
        d.materials, d.n_materials = self.mats, 3
        d.textures, d.n_textures = self.texs, 2
        return d

    def arrays(self):
        return {"prims": self.prims, "nodes": self.nodes}


def chain_prims(depth):
    return [sphere(3.0 * k, 0, 0, 1.0, k % 3) for k in range(depth)]


def chain_shape(depth, side):
    """A caterpillar of `depth` levels over primitives 0 .. depth-1: every internal node has
    one leaf child and the rest of the chain as its left ("left") or right ("right") child."""
    s = (depth - 2, depth - 1)
    for k in range(depth - 3, -1, -1):
        s = (s, k) if side == "left" else (k, s)
    return s


def tree_scene(rtx, name):
    if name.startswith("chain_"):
        _, side, depth = name.split("_")
        return TreeScene(rtx, chain_prims(int(depth)), chain_shape(int(depth), side)), chain_prims(int(depth))
    assert name == "ground2_tree"  # three primitives under an internal root: one global at the most
    prims = FILE_SCENES["ground2"]()
    return TreeScene(rtx, prims, (0, (1, 2))), prims


TREE_SCENES = ["chain_%s_%d" % (s, d) for d in CHAIN_STACK for s in ("left", "right")] + ["ground2_tree"]


@pytest.fixture(scope="module")
def scenes(rtx_mod, tmp_path_factory, mixed_scene_file):
    """name -> (scene for rtx.fast_tree / rtx.DeviceScene, its primitive lines or None, the path
    of its `bvh 0` copy or None), made once."""
    tmp = tmp_path_factory.mktemp("fast_tree")
    cache = {}

    def get(name):
        if name not in cache:
            if name in STOCK:
                path = mixed_scene_file if name == "mixed" else scene_path(name)
                cache[name] = (rtx_mod.HostScene.load(path), None, None)
            else:
                if name in FILE_SCENES:
                    prims = FILE_SCENES[name]()
                    sc = rtx_mod.HostScene.load(write_scene(tmp / (name + ".rtxs"), prims, 1))
                else:
                    sc, prims = tree_scene(rtx_mod, name)
                cache[name] = (sc, prims, write_scene(tmp / (name + "_list.rtxs"), prims, 0))
        return cache[name]

    return get


# ---------------------------------------------------------------------------------------
# float64 restatements
# ---------------------------------------------------------------------------------------
def prim_boxes(prims):
    """(lo, hi) of every primitive in float64: sphere c -+ |r|, a rect on its plane, a
    triangle's exact vertex box (no pad)."""
    g, kind = prims["g"], prims["kind"]
    lo, hi = np.zeros((len(prims), 3)), np.zeros((len(prims), 3))
    for i in range(len(prims)):
        if kind[i] == SPHERE:
            lo[i], hi[i] = g[i, :3] - abs(g[i, 3]), g[i, :3] + abs(g[i, 3])
        elif kind[i] == TRIANGLE:
            v = g[i].reshape(3, 3)
            lo[i], hi[i] = v.min(0), v.max(0)
        else:
            ax, a0, a1 = {XY: (2, 0, 1), XZ: (1, 0, 2), YZ: (0, 1, 2)}[int(kind[i])]
            lo[i, a0], hi[i, a0] = min(g[i, 0], g[i, 1]), max(g[i, 0], g[i, 1])
            lo[i, a1], hi[i, a1] = min(g[i, 2], g[i, 3]), max(g[i, 2], g[i, 3])
            lo[i, ax] = hi[i, ax] = g[i, 4]
    return lo, hi


def padded_boxes(prims):
    """prim_boxes with the documented triangle pad: 2^-19 of the largest extent, each side."""
    lo, hi = prim_boxes(prims)
    tri = prims["kind"] == TRIANGLE
    pad = np.ldexp((hi - lo).max(1), -19) * tri
    return lo - pad[:, None], hi + pad[:, None]


def half_area(lo, hi):
    d = hi - lo
    return d[0] * d[1] + d[1] * d[2] + d[2] * d[0]


def expected_globals(prims):
    """The documented rule: up to two primitives, largest box first, each with a box area of at
    least that of the union of all the others'; at least two primitives stay in the tree."""
    lo, hi = padded_boxes(prims)
    out, n = [], len(prims)
    while len(out) < 2 and n - len(out) > 2:
        rest = [i for i in range(n) if i not in out]
        areas = [half_area(lo[i], hi[i]) for i in rest]
        big = rest[int(np.argmax(areas))]  # the first of equal areas, as a strict > scan keeps it
        others = [i for i in rest if i != big]
        if not (np.isfinite(max(areas)) and max(areas) >= half_area(lo[others].min(0), hi[others].max(0))):
            break
        out.append(big)
    return out


def slot_boxes(nodes):
    """f32 (n, 4, 3) lo and hi of every slot."""
    lo = np.stack([nodes["lox"], nodes["loy"], nodes["loz"]], 2)
    hi = np.stack([nodes["hix"], nodes["hiy"], nodes["hiz"]], 2)
    return lo, hi


def fast_stack_need(nodes):
    """Worst-case stack depth of the lean walk, recomputed over the F4Nodes: a node entered
    with sp = s that has k internal slots hands each child s + max(0, k - 1)."""
    need, work = 0, [(0, 0)]
    while work:
        i, s = work.pop()
        kids = [int(c) for c in nodes["child"][i] if c >= 0]
        s += max(0, len(kids) - 1)
        need = max(need, s)
        work += [(c, s) for c in kids]
    return need


def parity_stack_peak(nodes):
    """Reference-layout walk with every box accepted (push right, push left, pop): the largest
    sp + 2 at a push, which trace_parity compares with its STACK."""
    peak, stack = 0, [0]
    while stack:
        nd = nodes[stack.pop()]
        if not nd["is_leaf"]:
            peak = max(peak, len(stack) + 2)
            stack += [int(nd["right_count"]), int(nd["left_first"])]
    return peak


def levels(nodes):
    d = np.zeros(len(nodes), int)
    for i, nd in enumerate(nodes):
        if not nd["is_leaf"]:
            d[nd["left_first"]] = d[nd["right_count"]] = d[i] + 1
    return int(d.max()) + 1 if len(nodes) else 0


# ---------------------------------------------------------------------------------------
# CPU half
# ---------------------------------------------------------------------------------------
CPU_SCENES = STOCK + list(FILE_SCENES) + TREE_SCENES


@pytest.mark.parametrize("name", CPU_SCENES)
def test_fast_tree_invariants(rtx_mod, scenes, name):
    sc = scenes(name)[0]
    info, f4 = rtx_mod.fast_tree(sc)
    arr = sc.arrays()
    prims, nodes = arr["prims"], arr["nodes"]
    n = len(prims)

    # stack bound, parity
    assert info["depth"] == levels(nodes)
    assert (info["stack_parity"] == -1) == (info["depth"] + 2 > 64)
    if info["stack_parity"] == -1:
        assert info["fast_ok"] == 0 and info["n_f4"] == 0
        return
    assert info["stack_parity"] in (32, 64)
    if len(nodes):
        assert parity_stack_peak(nodes) <= info["stack_parity"]
        assert info["stack_parity"] == (32 if info["depth"] + 2 <= 32 else 64)
    if len(nodes) == 0 or nodes[0]["is_leaf"]:  # flat list / one-leaf root: no fast tree, fast runs the parity walk
        assert (info["fast_ok"], info["n_f4"], info["n_global"], info["tree_kind"]) == (0, 0, 0, -1)
        return
    assert info["n_f4"] == len(f4) >= 1

    # partition
    globs = [info["global0"], info["global1"]][:info["n_global"]]
    assert info["n_global"] <= 2 and n - info["n_global"] >= 2
    assert globs == expected_globals(prims)
    child = f4["child"]
    lo, hi = slot_boxes(f4)
    # ~0 == -1: primitive 0's leaf slot carries the empty slot's child word, and only the
    # inverted box, which no ray enters, tells an empty slot from it
    empty = np.all(lo == np.inf, 2) & np.all(hi == -np.inf, 2) & (child == -1)
    leaf = (child < 0) & ~empty
    in_tree = np.sort(~child[leaf])
    assert np.array_equal(in_tree, np.array([i for i in range(n) if i not in globs])), "each primitive in one leaf slot"
    kinds = set(prims["kind"][in_tree].tolist())
    want_kind = kinds.pop() if len(kinds) == 1 else -1
    assert info["tree_kind"] == (want_kind if info["fast_ok"] else -1)

    # layout
    assert np.all(np.isfinite(lo[~empty]) & np.isfinite(hi[~empty]) & (lo[~empty] <= hi[~empty]))
    assert not empty[:, 0].any() and not empty[:, 1].any(), "every node holds at least two slots"
    assert np.all(empty[:, 2] <= empty[:, 3]), "empty slots come last"
    cnt = np.stack([f4["counts"][:, 0] & 0xFFFF, f4["counts"][:, 0] >> 16, f4["counts"][:, 1] & 0xFFFF,
                    f4["counts"][:, 1] >> 16], 1)
    assert np.array_equal(cnt, leaf.astype(cnt.dtype)), "counts: 1 in leaf slots, 0 elsewhere"
    order, work = [], [0]
    while work:  # slot-order depth-first walk: the nodes must come out as 0, 1, 2, ...
        i = work.pop()
        order.append(i)
        kids = [int(c) for c in child[i] if c >= 0]
        assert all(c > i for c in kids)
        work += kids[::-1]
    assert order == list(range(len(f4))), "pre-order, every node referenced exactly once"

    # conservative leaf boxes (f32 -> f64 is exact)
    plo, phi = prim_boxes(prims)
    qlo, qhi = padded_boxes(prims)
    ids = ~child[leaf]
    llo, lhi = lo[leaf].astype(np.float64), hi[leaf].astype(np.float64)
    assert np.all(llo <= plo[ids]) and np.all(lhi >= phi[ids])
    assert np.all(llo <= qlo[ids]) and np.all(lhi >= qhi[ids]), "triangle pad of 2^-19 ext, rounded outward"
    # ... and no wider than the outward rounding needs: within one f32 step of the padded box
    assert np.all(np.nextafter(lo[leaf], np.float32(np.inf)).astype(np.float64) > qlo[ids])
    assert np.all(np.nextafter(hi[leaf], np.float32(-np.inf)).astype(np.float64) < qhi[ids])

    # conservative inner boxes, exactly, in f32
    for i in range(len(f4)):
        for c in range(4):
            k = child[i, c]
            if k >= 0:
                assert np.all(lo[i, c] <= lo[k]) and np.all(hi[i, c] >= hi[k]), (i, c)

    # stack bound, fast
    need = fast_stack_need(f4)
    assert info["fast_need"] == need
    if need <= 32:
        assert (info["fast_ok"], info["stack_fast"]) == (1, 32)
    elif need <= 64:
        assert (info["fast_ok"], info["stack_fast"]) == (1, 64)
    else:
        assert info["fast_ok"] == 0
    if info["fast_ok"]:
        assert info["fast_need"] + 1 <= info["stack_fast"] + 1  # run_persistent_k1's stack_slots check


def test_line_scenes_sit_on_the_stack_boundaries(rtx_mod, scenes):
    """The (n, ratio) found with the hook: need exactly 32, 33, 64 and 65, and a reference-layout
    tree shallow enough that the parity walk stays available for the last one."""
    for name, (n, need) in LINES.items():
        info, _ = rtx_mod.fast_tree(scenes(name)[0])
        assert (info["fast_need"], info["n_global"]) == (need, 0), (name, info)
        assert info["stack_fast"] == {32: 32, 33: 64, 64: 64, 65: -1}[need]
        assert info["fast_ok"] == (need <= 64) and info["stack_parity"] in (32, 64)


@pytest.mark.parametrize("side", ["left", "right"])
def test_chain_trees_pick_the_parity_stack(rtx_mod, scenes, side):
    """Caterpillars of D levels: the stack grows by one per level when the chain is the left
    child (pushed last, popped first) and stays at 2 when it is the right child; pick_stack
    sizes for the depth either way."""
    for depth, stack in CHAIN_STACK.items():
        sc = scenes("chain_%s_%d" % (side, depth))[0]
        info, _ = rtx_mod.fast_tree(sc)
        assert (info["depth"], info["stack_parity"]) == (depth, stack)
        assert parity_stack_peak(sc.arrays()["nodes"]) == (depth if side == "left" else 2)


def test_small_scene_shapes(rtx_mod, scenes):
    """What the reference builder makes of the small scenes, which the GPU half relies on."""
    for n in (1, 2, 3, 4):
        nodes = scenes("spheres%d" % n)[0].arrays()["nodes"]
        assert len(nodes) == 1 and nodes[0]["is_leaf"] and nodes[0]["right_count"] == n  # froot_leaf
    assert not scenes("spheres5")[0].arrays()["nodes"][0]["is_leaf"]
    nodes = scenes("coincident50")[0].arrays()["nodes"]
    assert (nodes["right_count"][nodes["is_leaf"] == 1] > 4).any(), "a leaf of more than four primitives"
    info, _ = rtx_mod.fast_tree(scenes("ground2_tree")[0])
    assert (info["n_global"], info["global0"], info["fast_ok"], info["n_f4"]) == (1, 0, 1, 1)
    info, _ = rtx_mod.fast_tree(scenes("rect_plane")[0])
    assert info["tree_kind"] == XZ
    info, _ = rtx_mod.fast_tree(scenes("final")[0])
    assert (info["n_global"], info["tree_kind"]) == (1, SPHERE)


def test_hook_rejects_bad_descriptions(rtx_mod, scenes):
    sc = scenes("chain_left_30")[0]
    bad = TreeScene(rtx_mod, chain_prims(30), chain_shape(30, "left"))
    bad.nodes[5]["left_first"] = 3  # a child before its parent
    with pytest.raises(rtx_mod.RtxError, match="pre-order"):
        rtx_mod.fast_tree(bad)
    rtx_mod.fast_tree(sc)


# ---------------------------------------------------------------------------------------
# Rays
# ---------------------------------------------------------------------------------------
def make_rays(prims, seed, n=4000):
    """About n rays through a scene of any scale: along the x axis (the line / chain axis) in
    both directions from outside and from between the primitives, with two exactly zero
    direction components (some of them -0.0); rays aimed from near one primitive at another of comparable size;
    copies of those with one direction component zeroed and with a -0.0 component; and rays
    from beyond either end that cross every box of a line through its corner region, where
    they miss every sphere (the walk's deepest stack)."""
    rng = np.random.default_rng(seed)
    lo, hi = prim_boxes(prims)
    ok = np.all(np.isfinite(lo) & np.isfinite(hi), 1)
    lo, hi = lo[ok], hi[ok]
    c = 0.5 * (lo + hi)
    s = 0.5 * (hi - lo).max(1)
    s = np.where(s > 0, s, 1.0)
    m = len(c)
    q = n // 6
    out = []
    # along x: from just outside a primitive, from midway to the next one and from far outside
    i = rng.integers(0, m, 2 * q)
    start = rng.integers(0, 3, 2 * q)
    sign = np.where(rng.random(2 * q) < 0.5, -1.0, 1.0)
    nxt = np.minimum(i + 1, m - 1)
    first, last = int(np.argmin(lo[:, 0])), int(np.argmax(hi[:, 0]))
    outside = np.where(sign > 0, lo[first, 0] - 3.0 * s[first], hi[last, 0] + 3.0 * s[last])
    x0 = np.where(start == 0, c[i, 0] - sign * 3.0 * s[i], np.where(start == 1, 0.5 * (c[i, 0] + c[nxt, 0]), outside))
    off = rng.uniform(-1.2, 1.2, (2 * q, 2)) * s[i, None]
    o = np.column_stack([x0, c[i, 1] + off[:, 0], c[i, 2] + off[:, 1]])
    zero = np.where(rng.random((2 * q, 2)) < 0.5, -0.0, 0.0)
    out.append(np.column_stack([o, sign * rng.uniform(0.5, 2.0, 2 * q), zero]))
    # aimed: from near one primitive at another
    # (a target within 10^4 of the origin primitive's size: across the 10^29 of a line scene the
    # sphere test's discriminant cancels to noise, and the reference's own BVH and list walks
    # then disagree about hits that its boxes cull)
    i = rng.integers(0, m, 4 * q)
    j = np.array([rng.choice(np.nonzero((s <= 1e4 * s[a]) & (s[a] <= 1e4 * s))[0]) for a in i])
    u = rng.normal(size=(4 * q, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    o = c[i] + u * (s[i] * rng.uniform(1.5, 4.0, 4 * q))[:, None]
    t = c[j] + rng.uniform(-1.1, 1.1, (4 * q, 3)) * s[j, None]
    aimed = np.column_stack([o, t - o])
    out.append(aimed[:2 * q])
    one0 = aimed[2 * q:3 * q].copy()  # one zero component
    one0[np.arange(q), 3 + rng.integers(0, 3, q)] = 0.0
    out.append(one0)
    neg0 = aimed[3 * q:].copy()  # a -0.0 component (and a second zero in half of them)
    k = rng.integers(0, 3, q)
    neg0[np.arange(q), 3 + k] = -0.0
    half = np.arange(q)[::2]
    neg0[half, 3 + (k[half] + 1) % 3] = 0.0
    out.append(neg0)
    # corner grazers: y = z = a x with a below the box's half height over x and above r / sqrt 2
    r = 0.5 * (hi - lo)[:, 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        slope = np.where(c[:, 0] > 0, r / c[:, 0], np.nan)
    if m > 8 and np.nanmax(slope) - np.nanmin(slope) < 1e-9 * np.nanmax(slope):
        a = np.nanmax(slope) * rng.uniform(0.75, 0.95, q)
        far = 2.0 * hi[:, 0].max()
        fwd = np.column_stack([np.zeros((q, 3)), np.ones(q), a, a])
        back = np.column_stack([far * np.ones(q), a * far, a * far, -np.ones(q), -a, -a])
        out += [fwd[:q // 2], back[:q // 2]]
    return np.ascontiguousarray(np.vstack(out))


GPU_SCENES = [n for n in list(FILE_SCENES) + TREE_SCENES if not n.endswith("_63")]


def scene_rays(scenes, name):
    sc = scenes(name)[0]
    return make_rays(sc.arrays()["prims"], seed=1 + CPU_SCENES.index(name))


@pytest.mark.parametrize("name", GPU_SCENES)
def test_oracle_ties_stay_rare(orc, scenes, name):
    """The GPU half allows record differences only at exact t ties between primitives, on at
    most 1 % of the rays: the oracle's brute force alone must stay within that for the rays
    used (coincident50 is all ties by construction and asks for full equality instead)."""
    rays = scene_rays(scenes, name)
    assert 3900 <= len(rays) <= 4700
    osc = orc.Scene(scenes(name)[2])
    ref = osc.intersect(rays)
    hit = np.nonzero(ref[:, 0] == 1)[0]
    assert len(hit) >= 0.2 * len(rays) or name == "triangles", len(hit)
    assert len(hit) >= 100
    if name == "coincident50":
        return
    ties = sum(osc.tied_hits(rays[i], ref[i, 1])[1] >= 2 for i in hit)
    assert ties <= 0.01 * len(rays), ties


@pytest.mark.parametrize("name", list(LINES))
def test_line_rays_fill_the_stack(orc, rtx_mod, scenes, name):
    """The forward corner rays miss every sphere, so nothing culls their walk, and a near-first walk of
    the F4Nodes (float64 slab tests on the f32 boxes) holds `need` entries at its peak: the GPU
    half really stores into the last slot the host allows."""
    sc, _, list_file = scenes(name)
    info, f4 = rtx_mod.fast_tree(sc)
    rays = scene_rays(scenes, name)
    q = 4000 // 6
    corner = rays[-2 * (q // 2):-(q // 2)]  # the forward ones, from the small end
    assert not orc.Scene(list_file).intersect(corner)[:, 0].any()
    lo, hi = (b.astype(np.float64) for b in slot_boxes(f4))
    child = f4["child"]
    peak = 0
    for ray in np.vstack([corner[:4], corner[-4:]]):
        o, inv = ray[:3], 1.0 / ray[3:]
        node, stack = 0, []
        while node is not None:
            t0, t1 = (lo[node] - o) * inv, (hi[node] - o) * inv
            tn, tf = np.maximum(np.minimum(t0, t1).max(1), 0.0), np.maximum(t0, t1).min(1)
            entered = sorted((tn[c], int(child[node, c])) for c in range(4) if tn[c] <= tf[c] and child[node, c] >= 0)
            stack += [c for _, c in entered[:0:-1]]
            peak = max(peak, len(stack))
            node = entered[0][1] if entered else (stack.pop() if stack else None)
    assert peak == info["fast_need"]


# ---------------------------------------------------------------------------------------
# GPU half
# ---------------------------------------------------------------------------------------
def hit_matrix(h):
    return np.column_stack([h["hit"], h["t"], h["p"], h["normal"], h["u"], h["v"], h["front_face"], h["material"]])


@pytest.mark.gpu
@pytest.mark.parametrize("name", GPU_SCENES)
def test_intersect_bit_exact_against_brute_force(rtx_mod, orc, gpu, scenes, name):
    """parity, fast and the oracle's linear list (`bvh 0` copy, the reference's own hit
    arithmetic) report the same hit flags and the same t, bit for bit, and the same record
    except at exact ties between primitives, where each record must be one of the tied ones."""
    sc, _, list_file = scenes(name)
    info, _ = rtx_mod.fast_tree(sc)
    if name == "coincident50":
        nodes = sc.arrays()["nodes"]
        assert (nodes["right_count"][nodes["is_leaf"] == 1] > 4).any()
    rays = scene_rays(scenes, name)
    osc = orc.Scene(list_file)
    ref = osc.intersect(rays)
    d = rtx_mod.DeviceScene(sc)
    a = hit_matrix(d.intersect(rays, precision="parity"))
    b = hit_matrix(d.intersect(rays, precision="fast"))
    hit = ref[:, 0] == 1
    assert hit.sum() >= 100
    ties = 0
    for what, got in (("parity", a), ("fast", b)):
        assert np.array_equal(got[:, 0], ref[:, 0]), (what, np.nonzero(got[:, 0] != ref[:, 0])[0][:5])
        assert np.array_equal(got[hit, 1], ref[hit, 1]), (what, np.nonzero(hit & (got[:, 1] != ref[:, 1]))[0][:5])
        differ = np.nonzero(hit & ~np.all(got[:, COLS] == ref[:, COLS], 1))[0]
        if name == "coincident50":
            assert len(differ) == 0, (what, differ[:5])
        for i in differ:
            tied, n = osc.tied_hits(rays[i], ref[i, 1])
            assert n >= 2, (what, "not a tie", i, got[i], ref[i])
            assert np.any(np.all(tied[:, COLS] == got[i, COLS], 1)), (what, i, tied, got[i])
        ties = max(ties, len(differ))
    assert ties <= 0.01 * len(rays), ties
    if not info["fast_ok"]:  # a fast request served by the parity walk: the same walk, tie order included
        assert np.array_equal(a[hit][:, COLS], b[hit][:, COLS])


@pytest.mark.gpu
@pytest.mark.parametrize("side", ["left", "right"])
def test_chain_of_63_levels_is_refused(rtx_mod, gpu, scenes, side):
    with pytest.raises(rtx_mod.RtxError, match="deeper than 62"):
        rtx_mod.DeviceScene(scenes("chain_%s_63" % side)[0])


def look_at(rtx, lookfrom, lookat, vfov, width=16):
    return rtx.camera(rtx.camera_config("c1_three", width=width, aspect=1.0, vfov=vfov, lookfrom=tuple(lookfrom),
                                        lookat=tuple(lookat), vup=(0.0, 1.0, 0.0), defocus=0.0))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["line64", "chain_left_62"])
def test_renders_on_64_entry_stacks(rtx_mod, gpu, scenes, name):
    """The first runs of the <64, ...> instantiations of the wavefront, persistent (plain, PARK
    leaf-step, PARK speculative) and AOV kernels: every mode and schedule renders the same
    frame, bit for bit, in each precision, and the fast first-hit depth equals the parity one."""
    sc = scenes(name)[0]
    info, _ = rtx_mod.fast_tree(sc)
    assert info["stack_parity"] == 64 and info["fast_ok"] == 1
    if name == "line64":
        assert info["stack_fast"] == 64
        # from beyond the small end, looking along the line: the spheres nest in the view
        cam = look_at(rtx_mod, (-0.5, 0.02, 0.03), (1.0, 0.0, 0.0), 12.0)
    else:
        cam = look_at(rtx_mod, (-6.0, 1.5, 2.0), (40.0, 0.0, 0.0), 40.0)
    d = rtx_mod.DeviceScene(sc)
    variants = [dict(mode="wavefront")] + [dict(mode="persistent", schedule=s) for s in ("plain", "park", "park_step", None)]
    variants.append(dict(mode="persistent", generic=True))
    for precision in ("parity", "fast"):
        first = None
        for v in variants:
            rgb, spp, st = d.render(cam, spp=2, max_depth=8, seed=77, adaptive=False, precision=precision, **v)
            assert np.all(np.isfinite(rgb)) and np.all(spp == 2)
            if first is None:
                first = (rgb, spp, st["rays_total"])
                assert st["rays_total"] > 2 * len(rgb), "some paths must bounce off the spheres"
                continue
            assert rgb.tobytes() == first[0].tobytes(), (precision, v)
            assert np.array_equal(spp, first[1]) and st["rays_total"] == first[2], (precision, v)
    depth_p = d.aov(cam, precision="parity")[2]
    depth_f = d.aov(cam, precision="fast")[2]
    assert depth_p.tobytes() == depth_f.tobytes()
    assert np.isfinite(depth_p).sum() >= len(depth_p) // 4 or (depth_p > 0).sum() >= len(depth_p) // 4
