"""The speculative BVH4 walk's order: which nodes a lane visits and which primitives it tests, in
which order (trace4_run_spec, csrc/rtx_device.h).  Exact t ties between primitives are decided by
that order, so a change to the visit (the slab tests, the leaf queue, the five-comparator sort, the
pushes) must leave it as it is.

The device side is a test hook of the PARK unit (rtx_internal_visit_order): one wave walks up to 64
caller rays, one per lane, with the walk the bench line's kernel runs, and every lane logs the node
index of each visit and ~primitive of each test, with its closest distance after each (the first
64 entries; the count goes on).  It also returns the lane's slab constants (make_fray4l: the
hardware reciprocal has no host twin).

The host side restates the order in plain Python from the fast tree as the device holds it
(rtx.scene_trees): the slab tests with exactly rounded f32 FMAs and fmaxf / fminf's NaN rule, leaf
slots queued in slot order, the network (0,1) (2,3) (0,2) (1,3) (1,2) with strict `<`, the entered
children pushed far to near, and the wave's schedule (a lane visits while at most 4 leaves wait in
its queue; the wave tests one queued leaf per lane once 8 lanes hold some or no lane can visit).
Whether a tested primitive is hit is not restated (other tests hold the primitive tests to the
oracle bit for bit): the closest distance after a test is read from the device's log.
"""
import ctypes as C
import itertools
from fractions import Fraction

import numpy as np
import pytest

import test_fast_tree as ft

CAP = 64
INF = np.float32(np.inf)
SLACK = np.float32(1.00001)


def visit_order(rtx, dev, rays, lanes, tmin=0.001):
    f = rtx.lib().rtx_internal_visit_order
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_double] + [C.c_void_p] * 4
    f.restype = C.c_int
    rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
    n = len(rays)
    seq, tseq = np.zeros((n, CAP), np.int32), np.zeros((n, CAP), np.float64)
    ln, fray = np.zeros(n, np.int32), np.zeros((n, 15), np.uint32)
    rc = f(dev.h, rays.ctypes.data, n, lanes, tmin, seq.ctypes.data, tseq.ctypes.data, ln.ctypes.data, fray.ctypes.data)
    assert rc == 0, rtx.lib().rtx_last_error()
    return seq, tseq, ln, fray


# ---------------------------------------------------------------------------------------
# f32 arithmetic as the device does it
# ---------------------------------------------------------------------------------------
def round_f32(exact):
    """A Fraction rounded once to float32, to nearest, ties to even."""
    x = float(exact)  # correctly rounded to f64
    f = np.float32(x)
    if float(f) == x or not np.isfinite(f):
        return f
    other = np.nextafter(f, np.float32(np.inf) if x > float(f) else np.float32(-np.inf))
    mid = (Fraction(float(f)) + Fraction(float(other))) / 2
    if Fraction(x) != mid:  # x is not a midpoint of two floats: rounding x rounds exact
        return f
    if exact == mid:
        return f  # numpy rounded the tie to even
    return other if (exact > mid) == (float(other) > float(f)) else f


def fma32(a, b, c):
    a, b, c = float(a), float(b), float(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        with np.errstate(invalid="ignore"):
            return np.float32(np.float64(a) * np.float64(b) + np.float64(c))  # inf / NaN rules; finite parts exact
    p = a * b  # exact in f64: 24 x 24 bits
    s = np.float64(p + c)
    if int(s.view(np.uint64)) & ((1 << 29) - 1) != (1 << 28) and abs(s) >= 2.0 ** -100:
        return np.float32(s)  # not halfway between two floats: rounding the rounded sum rounds the exact one
    return round_f32(Fraction(a) * Fraction(b) + Fraction(c))


def fmax(a, b):
    return b if np.isnan(a) else (a if np.isnan(b) else max(a, b))


def fmin(a, b):
    return b if np.isnan(a) else (a if np.isnan(b) else min(a, b))


def round_up_f32(x):
    f = np.float32(x)
    return np.nextafter(f, INF) if float(f) < x else f


def cswap(tt, cc, a, b):
    if tt[b] < tt[a]:
        tt[a], tt[b] = tt[b], tt[a]
        cc[a], cc[b] = cc[b], cc[a]


def network(tt, cc):
    """Today's five comparators, strict <: not a stable sort, and no fixed tie-break."""
    for a, b in ((0, 1), (2, 3), (0, 2), (1, 3), (1, 2)):
        cswap(tt, cc, a, b)


def slab_test(w, k, off, tmax_x):
    """One node's four slots (w: its 32 words as f32; k, off: the ray's constants): the clamped entry
    distances and whether each slot's box is entered before tmax_x."""
    ent = [w[o:o + 4] for o in off]
    ext = [w[(o ^ 4):(o ^ 4) + 4] for o in off]
    tns, hits = [], []
    for c in range(4):
        t = [fma32(ent[a][c], k[a], k[3 + a]) for a in range(3)]
        x = [fma32(ext[a][c], k[6 + a], k[9 + a]) for a in range(3)]
        tn = fmax(fmax(t[0], t[1]), fmax(t[2], np.float32(0)))
        tf = fmin(fmin(x[0], x[1]), fmin(x[2], tmax_x))
        tns.append(tn)
        hits.append(bool(tn <= tf))
    return tns, hits


def ray_consts(fray):
    return fray[:12].view(np.float32), [int(v) // 4 for v in fray[12:15]]


class Lane:
    def __init__(self, fray, dev_t, cap_stop):
        self.k, self.off = ray_consts(fray)
        self.dev_t, self.cap_stop = dev_t, cap_stop
        self.node, self.stack, self.sp = 0, {}, 0
        self.closest, self.tmax_x = np.inf, INF
        self.walking, self.q, self.log = True, [], []

    def blind(self):  # past the device's log: the closest distance is not known any more
        return self.cap_stop and len(self.log) >= CAP

    def visit(self, words, child):
        self.log.append(self.node)
        tns, hits = slab_test(words[self.node], self.k, self.off, self.tmax_x)
        cc = [int(c) for c in child[self.node]]
        tt = []
        for c in range(4):
            if hits[c] and cc[c] < 0:
                self.q.append(~cc[c])
            tt.append(tns[c] if hits[c] and cc[c] >= 0 else INF)
        assert len(self.q) <= 8
        network(tt, cc)
        if tt[0] != INF:
            for c in (3, 2, 1):  # far to near; a store at sp stays only if the child was entered
                self.stack[self.sp] = cc[c]
                self.sp += 1 if tt[c] != INF else 0
            self.node = cc[0]
        elif self.sp == 0:
            self.walking = False
        else:
            self.sp -= 1
            self.node = self.stack[self.sp]

    def leaf(self):
        prim = self.q.pop(0)
        pos = len(self.log)
        self.log.append(~prim)
        if pos < CAP:
            new = self.dev_t[pos]
            assert new <= self.closest
            if new != self.closest:
                self.closest = new
                self.tmax_x = round_up_f32(new) * SLACK


def model_wave(words, child, frays, dev_ts, cap_stop):
    lanes = [Lane(f, t, cap_stop) for f, t in zip(frays, dev_ts)]
    alive = list(lanes)
    while alive:
        for ln in alive:
            if ln.walking and len(ln.q) <= 4:
                ln.visit(words, child)
        can = any(ln.walking and len(ln.q) <= 4 for ln in alive)
        if not can or sum(1 for ln in alive if ln.q) >= 8:
            for ln in alive:
                if ln.q:
                    ln.leaf()
        alive = [ln for ln in alive if (ln.walking or ln.q) and not ln.blind()]
    return [ln.log for ln in lanes]


def check(rtx, dev, rays, lanes, what):
    """Device log against the model, wave by wave.  With one ray per wave a log longer than the cap
    is compared over the entries kept; with more, every lane's log must fit (the lanes' schedules
    depend on each other)."""
    _, f4 = rtx.scene_trees(dev)
    words = f4.view(np.float32).reshape(len(f4), 32)
    child = f4["child"]
    seq, tseq, ln, fray = visit_order(rtx, dev, rays, lanes)
    assert np.all(ln >= 1), what
    if lanes > 1:
        assert ln.max() <= CAP, (what, int(ln.max()))
    for w0 in range(0, len(rays), lanes):
        idx = range(w0, min(w0 + lanes, len(rays)))
        logs = model_wave(words, child, [fray[i] for i in idx], [tseq[i] for i in idx], cap_stop=lanes == 1)
        for i, log in zip(idx, logs):
            n = min(int(ln[i]), CAP)
            assert log[:CAP] == seq[i, :n].tolist(), (what, i, rays[i].tolist(), log[:CAP], seq[i, :n].tolist())
            if ln[i] <= CAP:
                assert len(log) == ln[i], (what, i)
    return seq, ln, fray, words, child


# ---------------------------------------------------------------------------------------
# Shapes
# ---------------------------------------------------------------------------------------
def group_scene(rtx, ranks):
    """Four pairs of unit spheres under a root with four internal children: pair g sits at
    x = 4 * ranks[g], on a 2 x 2 grid in y and z, both spheres with the same x extent, so pairs
    of equal rank share their entry (and exit) plane in x."""
    prims = []
    for g, r in enumerate(ranks):
        y, z = 6.0 * (g & 1), 6.0 * (g >> 1)
        prims += [ft.sphere(4.0 * r, y, z, 0.5, g % 3), ft.sphere(4.0 * r, y + 1.5, z, 0.5, g % 3)]
    return ft.TreeScene(rtx, prims, (((0, 1), (2, 3)), ((4, 5), (6, 7))))


def group_rays():
    """Along +x and -x (y and z neutralised: every child entered, keys by x plane alone), through
    each pair and between them; oblique rays at each pair and across two; rays that turn away."""
    out = []
    for y, z in ((0, 0), (6, 0), (0, 6), (6, 6), (3, 3), (0.75, 0), (6.75, 6)):
        out += [[-10, y, z, 1, 0, 0], [40, y, z, -1, 0, 0], [-10, y, z, 2.5, -0.0, 0.0]]
    for g in range(4):
        y, z = 6.0 * (g & 1), 6.0 * (g >> 1)
        out += [[-10, 3, 3, 10 + 4 * k, y - 3 + 0.25, z - 3 + 0.125] for k in range(4)]
        out += [[-10, y, z, 1, 0.03, 0.02], [30, y + 1.5, z, -1, 0.01, 0.0]]
    out += [[-10, 0, 0, 1, 0.3, 0.3], [-10, 6, 6, 1, -0.3, -0.3], [-10, 0, 6, 1, 0.3, -0.3]]
    out += [[-10, 3, 3, -1, 0, 0], [-10, 3, 3, -1, 0.2, 0.1], [2, 30, 3, 0, 1, 0], [2, 3, -30, 0.1, 0, -1]]  # enter no child
    return np.array(out, dtype=np.float64)


WEAK_ORDERS = [r for r in itertools.product(range(4), repeat=4) if set(r) == set(range(max(r) + 1))]


def test_weak_orders_are_all_there():
    assert len(WEAK_ORDERS) == 75
    assert (0, 0, 0, 0) in WEAK_ORDERS and (0, 1, 2, 3) in WEAK_ORDERS and (1, 0, 0, 0) in WEAK_ORDERS


@pytest.mark.gpu
def test_equal_keys_at_every_position(rtx_mod, gpu):
    """All 75 weak orderings of the four children's entry planes: all four equal, every pair and
    triple of equal keys at every position, all distinct in every order."""
    rays = group_rays()
    seen_all4 = tied_keys = 0
    for ranks in WEAK_ORDERS:
        sc = group_scene(rtx_mod, ranks)
        info, f4 = rtx_mod.fast_tree(sc)
        assert info["fast_ok"] == 1 and info["n_global"] == 0 and len(f4) == 5 and np.all(f4["child"][0] >= 0), ranks
        seq, ln, fray, words, child = check(rtx_mod, rtx_mod.DeviceScene(sc), rays, 64, ranks)
        # the ties are really there: for the axis-parallel rays (+x: rays 0 and 2, -x: ray 1) all four
        # children are entered, and two of them have the same key exactly when their ranks are equal
        # (slot c of the root holds the pair whose first sphere is the first leaf of child c)
        group = [int(~child[k][0]) // 2 for k in child[0]]
        assert sorted(group) == [0, 1, 2, 3], (ranks, group)
        for i in (0, 1, 2):
            tns, hits = slab_test(words[0], *ray_consts(fray[i]), INF)
            assert all(hits), (ranks, i, tns)
            for a in range(4):
                for b in range(4):
                    assert (tns[a] == tns[b]) == (ranks[group[a]] == ranks[group[b]]), (ranks, i, tns, group)
            tied_keys += len(set(tns)) < 4
        # the axis-parallel rays enter all four children: each is visited
        for i in (0, 1):
            assert set(f4["child"][0].tolist()) <= set(seq[i, :ln[i]].tolist()), (ranks, i, seq[i, :ln[i]])
        seen_all4 += 1
        away = seq[len(rays) - 4:]
        assert np.all(ln[len(rays) - 4:] == 1) and np.all(away[:, 0] == 0), ranks
    print("weak orderings checked", seen_all4, "rays each", len(rays), "axis-parallel visits with tied keys", tied_keys)
    assert tied_keys == 3 * (75 - 24)  # every ordering but the 24 strict ones ties some keys


@pytest.mark.gpu
def test_small_trees(rtx_mod, gpu):
    """A root of four leaf slots; a tree of two nodes; one ray per wave and a full wave."""
    four = ft.TreeScene(rtx_mod, [ft.sphere(3.0 * k, 0.5 * k, 0, 1.0, k % 3) for k in range(4)], ((0, 1), (2, 3)))
    info, f4 = rtx_mod.fast_tree(four)
    assert len(f4) == 1 and np.all(f4["child"][0] < 0), "a root of four leaf slots"
    two = None
    for shape in ((0, (1, (2, (3, 4)))), ((0, 1), (2, (3, 4))), (((0, 1), 2), (3, 4))):
        cand = ft.TreeScene(rtx_mod, [ft.sphere(3.0 * k, 0.5 * k, 0, 1.0, k % 3) for k in range(5)], shape)
        if len(rtx_mod.fast_tree(cand)[1]) == 2:
            two = cand
            break
    assert two is not None, "no five-sphere shape collapses to a tree of two nodes"
    for name, sc in (("four_leaves", four), ("two_nodes", two)):
        rays = ft.make_rays(sc.arrays()["prims"], seed=11, n=600)[::5]
        dev = rtx_mod.DeviceScene(sc)
        check(rtx_mod, dev, rays, 1, name)
        check(rtx_mod, dev, rays, 64, name + "/wave")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ft.GPU_SCENES)
def test_degenerate_trees(rtx_mod, gpu, tmp_path, name):
    """The fixtures of test_fast_tree.py (its builders, imported), one ray per wave, 100 of its rays."""
    if name in ft.FILE_SCENES:
        prims = ft.FILE_SCENES[name]()
        sc = rtx_mod.HostScene.load(ft.write_scene(tmp_path / (name + ".rtxs"), prims, 1))
    else:
        sc, _ = ft.tree_scene(rtx_mod, name)
    info, f4 = rtx_mod.fast_tree(sc)
    if not (info["fast_ok"] and 0 < len(f4) < 65536):
        # no fast tree (a one-leaf root) or one deeper than the fast walk's stacks: the speculative
        # walk never runs on it, and the hook says so
        dev = rtx_mod.DeviceScene(sc)
        f = rtx_mod.lib().rtx_internal_visit_order
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_double] + [C.c_void_p] * 4
        f.restype = C.c_int
        z = np.zeros(64 * 8, np.float64)
        assert f(dev.h, z.ctypes.data, 1, 1, 0.001, z.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data) != 0
        return
    rays = ft.make_rays(sc.arrays()["prims"], seed=1 + ft.CPU_SCENES.index(name))
    rays = rays[::max(1, len(rays) // 100)]
    check(rtx_mod, rtx_mod.DeviceScene(sc), rays, 1, name)


# ---------------------------------------------------------------------------------------
# rtx_intersect's fast records
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["one_sphere", "one_triangle", "rects", "three", "cornell", "final", "bunny", "mixed"])
def test_fast_records_unchanged(rtx_mod, gpu, mixed_scene_file, scene):
    """rtx_intersect in fast precision on the 8 hit fixtures' rays (the seam tmin): every field of
    every record, bit for bit, against tests/golden/fast_hits_<scene>.npz, dumped from the build
    before the speculative walk's queueing changed.  The query walks share visit_slabs / visit_next
    with the frame kernels, so a change to either shows here."""
    import os

    from conftest import GOLDEN, scene_path

    rays = np.load(os.path.join(GOLDEN, f"hits_{scene}.npz"))["rays"]
    want = np.load(os.path.join(GOLDEN, f"fast_hits_{scene}.npz"))["seam"]
    d = rtx_mod.DeviceScene(rtx_mod.HostScene.load(mixed_scene_file if scene == "mixed" else scene_path(scene)))
    h = d.intersect(rays, tmin=float(np.float32(0.001)), precision="fast")
    got = np.column_stack([h["hit"], h["t"], h["p"], h["normal"], h["u"], h["v"], h["front_face"], h["material"]])
    assert got.shape == want.shape and np.array_equal(got[:, 0], want[:, 0])
    miss = want[:, 0] == 0  # a miss's other fields are not part of the record
    got[miss], want = 0.0, np.where(miss[:, None], 0.0, want)
    bad = np.nonzero(np.any(got.view(np.uint64) != want.view(np.uint64), 1))[0]
    assert len(bad) == 0, (scene, len(bad), bad[:5], got[bad[:2]], want[bad[:2]])
