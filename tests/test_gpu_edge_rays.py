"""The crafted edge rays (tests/edge_ray_cases.py) on the device, through the public entry points
DeviceScene.intersect / occluded (rtx_intersect, rtx_occluded) and their _device forms, against the
reference's recorded results (tests/golden/edge_hits.npz).

Termination and bounds, argued from csrc/rtx_device.h before the first run (nothing here is meant to
fault: these are ordinary inputs of a public entry point):
  * Every walk's loop is bounded by the tree, not by a distance.  The parity walk pops one node per
    iteration and pushes a node's two children at most once; the fast walks (trace4_run, occluded_fast4)
    visit a node, push the entered internal children and pop.  A distance (NaN, inf, negative)
    only decides whether a child is entered.  A ray with every axis neutralised (d zero, denormal or NaN
    on each axis: inv = 0, offsets -/+inf) enters every slot, so it visits every node of the finite tree
    once; the stack depth is build_fast4's worst case, which already counts every internal child of a
    node as entered.  `bvh 0` scenes and one-leaf roots loop over the primitive list.
  * An empty F4 slot has child word -1 and planes +/-inf.  Under full neutralisation inf * 0 = NaN, fmaxf /
    fminf drop the NaN and the slot counts as entered; as a negative child it is a leaf slot, never
    pushed, and leaf_prim decodes ~(-1) = primitive 0, which every scene has: one extra exact test of a
    primitive the walk may test anyway, in bounds.
  * A NaN distance never becomes `closest` through a sphere or a rect (both accept with
    tmin < t && t < tmax, false for NaN).  The triangle's range test, as the reference's, is two
    negated comparisons and accepts a NaN t; what follows is still a bounded walk, but the winner
    among several triangles then depends on the visiting order, so the cases keep overflowing,
    NaN and infinite rays out of scenes with triangles (edge_ray_cases.py says where).
  * Primitive indices come from the tree's leaf slots and the globals table only; no ray value
    is used as an index.

What the fast half measures.  In fast precision rtx_intersect* / rtx_occluded* run the parity walk for
tmin < 0 or an empty range, and their kernels send a ray to the parity walk in its lane only where the
reference's f64 box test and the conservative f32 one part (csrc/rtx_kernels.h): a component outside
fast_query_domain, or an axis-parallel ray whose hit primitive it touches in or outside a face plane of
that primitive's box (face_plane_hit; Aabb::Hit's 0 * inf rejects such a box).  Every other row is
answered by the fast walk: tests/test_edge_rays_host.py::test_the_fast_walk_receives_the_edge_rows counts
them per case (24 of 38 sphere rows, 23 of 36 global rows, all 41 triangle rows, 26 of 35 rect rows per
tree, every tie row), among them the oblique on-edge rows, the t == tmin / t == tmax rows and the rows of
every arm of sphere_root.

Power, from the CPU side (the four changes made one at a time to a scratch copy of the oracle, whose
arithmetic the device forms restate, counting the fast-decided, non-tie rows whose record changes on a
range the fast walk serves): a sphere range made inclusive changes 4 rows in each sphere tree and 3 in each
global scene; a triangle range made exclusive 18 rows in each triangle tree; a rect edge made exclusive 4
rows per rect tree and 12 in rect_mixed; sphere_root without its near_first fallback 3 rows in glob_one and
1 in glob_two.  Each of them changes a hit flag too, so both the record test and the occluded test fail.
"""
import ctypes as C
import os

import numpy as np
import pytest

import edge_ray_cases as erc

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = erc.cases()
NAMES = [c["name"] for c in CASES]
EXACT = [0, 1, 2, 3, 4, 5, 6, 7, 10, 11]  # hit t p normal front_face material
UV = [8, 9]


def hit_matrix(h):
    return np.column_stack([h["hit"], h["t"], h["p"], h["normal"], h["u"], h["v"], h["front_face"], h["material"]])


def same_bits(a, b):
    return (a == b) | (np.isnan(a) & np.isnan(b))


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "edge_hits.npz"))


@pytest.fixture(scope="module")
def scenes(rtx_mod, gpu, tmp_path_factory):
    """name -> (DeviceScene, scene file), created on first use and kept for the module."""
    d = tmp_path_factory.mktemp("edge_scenes")
    made = {}

    def get(name):
        if name not in made:
            p = d / (name + ".rtxs")
            p.write_text(erc.by_name(name)["scene"])
            made[name] = (rtx_mod.DeviceScene(rtx_mod.HostScene.load(str(p))), str(p))
        return made[name]

    return get


@pytest.fixture(scope="module")
def parity(scenes):
    """name -> [record matrix per range], the parity walk's records, computed once."""
    made = {}

    def get(name):
        if name not in made:
            c = erc.by_name(name)
            dev, _ = scenes(name)
            made[name] = [hit_matrix(dev.intersect(c["rays"], tmin=a, tmax=b, precision="parity")) for a, b in c["ranges"]]
        return made[name]

    return get


@pytest.mark.parametrize("name", NAMES)
def test_parity_equals_the_reference(parity, fixture, name):
    c = erc.by_name(name)
    tri_mats = erc.triangle_only_materials(c["scene"])
    for k, rng in enumerate(c["ranges"]):
        got, ref = parity(name)[k].copy(), fixture[name + ".hits"][k]
        got[ref[:, 0] == 0, 1:] = 0.0  # a miss's record is not defined beyond its flag
        bad = np.nonzero(~same_bits(got[:, EXACT], ref[:, EXACT]).all(1))[0]
        assert len(bad) == 0, (name, rng, bad[:5], [c["labels"][i] for i in bad[:5]], got[bad[:2]], ref[bad[:2]])
        # u, v: a triangle's are not compared (the reference leaves them unwritten); a sphere's come from
        # acos / atan2 (2 ulp at 1.0); a rect's are exact
        cmp = (ref[:, 0] == 1) & ~np.isin(ref[:, 11], tri_mats)
        d = np.abs(got[cmp][:, UV] - ref[cmp][:, UV])
        nan = np.isnan(ref[cmp][:, UV])
        assert np.array_equal(np.isnan(got[cmp][:, UV]), nan), (name, rng)
        assert (d[~nan] <= 4.5e-16).all(), (name, rng, d[~nan].max())


@pytest.mark.parametrize("name", NAMES)
def test_fast_equals_parity_except_marked_ties(parity, scenes, orc, name):
    c = erc.by_name(name)
    dev, path = scenes(name)
    osc = None
    for k, (tmin, tmax) in enumerate(c["ranges"]):
        a = parity(name)[k]
        b = hit_matrix(dev.intersect(c["rays"], tmin=tmin, tmax=tmax, precision="fast"))
        differ = np.nonzero(~same_bits(a[:, EXACT], b[:, EXACT]).all(1))[0]
        assert len(differ) <= int(c["tie"].sum()), (name, tmin, tmax, differ[:8], [c["labels"][i] for i in differ[:8]],
                                                    a[differ[:2]], b[differ[:2]])
        for i in differ:
            assert c["tie"][i], ("records differ on a row that is no tie", name, tmin, tmax, i, c["labels"][i], a[i], b[i])
            assert a[i, 0] == 1 and b[i, 0] == 1 and a[i, 1] == b[i, 1], (name, i, a[i], b[i])
            osc = osc or orc.Scene(path)
            tied, n = osc.tied_hits(c["rays"][i], a[i, 1], tmin=tmin)
            assert n >= 2, (name, i, n)
            recs = tied[:, EXACT]
            assert np.any(np.all(recs == a[i, EXACT], 1)) and np.any(np.all(recs == b[i, EXACT], 1)), (name, i, tied, a[i], b[i])


@pytest.mark.parametrize("name", NAMES)
def test_occluded_equals_the_hit_flag(parity, scenes, fixture, name):
    """Both precisions, every range with tmin < tmax (the entry point refuses the others): the segment form
    is the (0, 1) range of the sphere, triangle and rect families, whose rays end exactly on the surface."""
    c = erc.by_name(name)
    dev, _ = scenes(name)
    for k, (tmin, tmax) in enumerate(c["ranges"]):
        if not tmin < tmax:
            continue
        ref = fixture[name + ".hits"][k][:, 0] != 0
        assert np.array_equal(parity(name)[k][:, 0] != 0, ref)
        for prec in ("parity", "fast"):
            occ = dev.occluded(c["rays"], tmin=tmin, tmax=tmax, precision=prec) != 0
            hit = dev.intersect(c["rays"], tmin=tmin, tmax=tmax, precision=prec)["hit"] != 0
            bad = np.nonzero((occ != ref) | (hit != ref))[0]
            assert len(bad) == 0, (name, prec, tmin, tmax, bad[:8], [c["labels"][i] for i in bad[:8]], occ[bad[:8]], hit[bad[:8]])


@pytest.mark.parametrize("name", ["sph_tree", "glob_two", "tri_tree", "rect_mixed", "walk", "walk_nonfinite"])
def test_device_entry_points_equal_the_host_ones(rtx_mod, scenes, name):
    import torch

    c = erc.by_name(name)
    dev, _ = scenes(name)
    lib = rtx_mod.lib()
    n = len(c["rays"])
    d_rays = torch.from_numpy(c["rays"]).cuda()
    for tmin, tmax in c["ranges"]:
        for prec in ("parity", "fast"):
            d_hits = torch.zeros(n * rtx_mod.HIT_DTYPE.itemsize + 64, dtype=torch.uint8, device="cuda")
            d_occ = torch.full((n + 64,), 7, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            rtx_mod._check(lib.rtx_intersect_device(dev.h, C.c_void_p(d_rays.data_ptr()), n, C.c_void_p(d_hits.data_ptr()),
                                                    tmin, tmax, rtx_mod.PRECISIONS[prec], None), "rtx_intersect_device")
            if tmin < tmax:
                dev.occluded_device(d_rays.data_ptr(), n, d_occ.data_ptr(), tmin=tmin, tmax=tmax, precision=prec)
            host = dev.intersect(c["rays"], tmin=tmin, tmax=tmax, precision=prec)  # same stream: runs after them
            got = d_hits.cpu().numpy()
            assert got[:n * rtx_mod.HIT_DTYPE.itemsize].tobytes() == host.tobytes(), (name, prec, tmin, tmax)
            assert (got[n * rtx_mod.HIT_DTYPE.itemsize:] == 0).all()
            if tmin < tmax:
                occ = d_occ.cpu().numpy()
                assert np.array_equal(occ[:n], dev.occluded(c["rays"], tmin=tmin, tmax=tmax, precision=prec))
                assert (occ[n:] == 7).all()
