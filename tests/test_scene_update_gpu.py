"""In-place scene updates on the device (rtx_scene_update_*).

Scene A is updated to scene B's geometry (scene_update_fixture.py: same primitive list, moved
geometry, no two primitives at one ray's closest t in B, which test_scene_update_host.py checks
with the oracle).  A refit over the unchanged topology reproduces the bytes the host builders
give for that topology, and any conservative tree yields the same closest hit, so every
comparison here is bit for bit: the refit trees against numpy restatements, hits and renders
against a scene freshly created from file B and against the CPU oracle."""
import numpy as np
import pytest

import scene_update_fixture as fx

pytestmark = pytest.mark.gpu
CASES = [(n, v) for n in fx.COUNTS for v in fx.VARIANTS]


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("scene_update_gpu")


_fresh = {}


def setup(rtx, tmp, n, variant):
    """The fixture pair, A's host scene and B's records in A's leaf order; B's own device scene and
    oracle hits are made once."""
    a, b, fa, fb, rays = fx.pair(rtx, tmp, n, variant)
    ha = rtx.HostScene.load(fa)
    idx = ha.prim_indices()
    assert len(idx) == n
    a_leaf, b_leaf = a[idx], b[idx]
    assert a_leaf.tobytes() == ha.arrays()["prims"].tobytes()
    return dict(a=a, b=b, fa=fa, fb=fb, rays=rays, ha=ha, a_leaf=a_leaf, b_leaf=b_leaf, key=(n, variant))


def fresh_b(rtx, orc, s):
    if s["key"] not in _fresh:
        d = rtx.DeviceScene(rtx.HostScene.load(s["fb"]))
        hits = {p: hit_matrix(d.intersect(s["rays"], precision=p)) for p in ("parity", "fast")}
        _fresh[s["key"]] = (d, hits, orc.Scene(s["fb"]).intersect(s["rays"]))
    return _fresh[s["key"]]


def hit_matrix(h):
    return np.column_stack([h["hit"], h["t"], h["p"], h["normal"], h["u"], h["v"], h["front_face"], h["material"]])


def same_hits(got, ref):
    """Hit flags of every ray, and on the hit rays t, p, normal, front_face, material, bit for bit."""
    if not np.array_equal(got[:, 0], ref[:, 0]):
        return False
    hit = ref[:, 0] == 1
    return got[hit][:, fx.COLS].tobytes() == np.ascontiguousarray(ref[hit][:, fx.COLS]).tobytes()


# ---- numpy restatements -----------------------------------------------------------------------
def np_prim_box(prims):
    """prim_box (csrc/rtx_bounds.h) in float64: spheres centre +- |r|, triangles the vertex box
    padded by 2^-19 of its largest extent, rects the rectangle on its plane."""
    n = len(prims)
    lo, hi = np.zeros((n, 3)), np.zeros((n, 3))
    for i, p in enumerate(prims):
        g, k = p["g"], int(p["kind"])
        if k == fx.SPHERE:
            lo[i], hi[i] = g[:3] - abs(g[3]), g[:3] + abs(g[3])
        elif k == fx.TRIANGLE:
            v = g.reshape(3, 3)
            l, h = v.min(0), v.max(0)
            pad = (h - l).max() * 2.0 ** -19
            lo[i], hi[i] = l - pad, h + pad
        else:
            a0, a1 = {fx.XY: (0, 1), fx.XZ: (0, 2), fx.YZ: (1, 2)}[k]
            ax = 3 - a0 - a1
            lo[i, a0], hi[i, a0] = min(g[0], g[1]), max(g[0], g[1])
            lo[i, a1], hi[i, a1] = min(g[2], g[3]), max(g[2], g[3])
            lo[i, ax] = hi[i, ax] = g[4]
    return lo, hi


def round_out(lo, hi):
    """float32 rounded outward."""
    l, h = lo.astype(np.float32), hi.astype(np.float32)
    l = np.where(l.astype(np.float64) > lo, np.nextafter(l, np.float32(-np.inf)), l)
    h = np.where(h.astype(np.float64) < hi, np.nextafter(h, np.float32(np.inf)), h)
    return l.astype(np.float32), h.astype(np.float32)


def np_refit_f4(f4, prims):
    """The fast tree's slot boxes recomputed bottom-up over its own topology (children come after
    their parent): a primitive slot takes the primitive's rounded box, a child slot the float32
    union of the child's four slots, an empty slot stays inverted."""
    lo, hi = round_out(*np_prim_box(prims))
    out = f4.copy()
    names = (("lox", "hix"), ("loy", "hiy"), ("loz", "hiz"))
    for i in range(len(out) - 1, -1, -1):
        for c in range(4):
            child = int(out["child"][i, c])
            leaf = (int(out["counts"][i, c >> 1]) >> (16 * (c & 1))) & 0xFFFF
            for a, (nl, nh) in enumerate(names):
                if child >= 0:
                    out[nl][i, c], out[nh][i, c] = out[nl][child].min(), out[nh][child].max()
                elif leaf:
                    out[nl][i, c], out[nh][i, c] = lo[~child, a], hi[~child, a]
    return out


# ---- trees and hits ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,variant", CASES)
def test_update_matches_a_fresh_scene(rtx_mod, orc, gpu, tmp, n, variant):
    import torch

    rtx = rtx_mod
    s = setup(rtx, tmp, n, variant)
    info, f4_a = rtx.fast_tree(s["ha"])
    nodes_a = s["ha"].arrays()["nodes"]
    if n >= 1000:
        assert info["fast_ok"] and info["n_global"] >= 1 and info["global0"] == int(np.argmin(s["a_leaf"]["material"]))
        assert len(nodes_a) > 256, "many workgroups at height 0"
    d = rtx.DeviceScene(s["ha"])
    assert d.epoch() == 0
    # as created
    nodes, f4 = rtx.scene_trees(d)
    assert nodes.tobytes() == nodes_a.tobytes()
    assert f4.tobytes() == (f4_a.tobytes() if info["fast_ok"] else b"")
    # identity: the scene's own primitives
    d.update_prims(s["a_leaf"])
    assert d.epoch() == 1
    nodes, f4 = rtx.scene_trees(d)
    assert nodes.tobytes() == nodes_a.tobytes()
    assert f4.tobytes() == (f4_a.tobytes() if info["fast_ok"] else b"")
    d.update_prims(s["a_leaf"][:0])
    assert d.epoch() == 1  # count == 0: nothing happens
    # A -> B, against the restatements
    d.update_prims(s["b_leaf"])
    assert d.epoch() == 2
    nodes_b, f4_b = rtx.scene_trees(d)
    want_nodes = rtx.bvh_refit(nodes_a, rtx.prim_bounds(s["b_leaf"]))
    assert nodes_b.tobytes() == want_nodes.tobytes() and nodes_b.tobytes() != nodes_a.tobytes()
    if info["fast_ok"]:
        assert f4_b.tobytes() == np_refit_f4(f4_a, s["b_leaf"]).tobytes() and f4_b.tobytes() != f4_a.tobytes()
    # hits: the fresh scene of file B, and the oracle
    _, fresh_hits, ref = fresh_b(rtx, orc, s)
    for prec in ("parity", "fast"):
        got = hit_matrix(d.intersect(s["rays"], precision=prec))
        assert same_hits(got, fresh_hits[prec]), prec
        assert same_hits(got, ref), prec
    # the device variant: back to A on the host path, then to B from a tensor on the GPU
    d.update_prims(s["a_leaf"])
    g = torch.from_numpy(np.ascontiguousarray(s["b_leaf"]["g"])).cuda()
    torch.cuda.synchronize()
    d.update_geometry_device(g.data_ptr(), 0, n)
    assert d.epoch() == 4
    nodes_d, f4_d = rtx.scene_trees(d)
    assert nodes_d.tobytes() == nodes_b.tobytes() and f4_d.tobytes() == f4_b.tobytes()
    for prec in ("parity", "fast"):
        assert same_hits(hit_matrix(d.intersect(s["rays"], precision=prec)), ref), prec


def test_partial_update(rtx_mod, orc, gpu, tmp):
    """first = 37, count = 130 of the large mixed scene: the same as a scene created from the mixed
    table (its hits), and the trees of the restatements over the mixed table."""
    rtx = rtx_mod
    s = setup(rtx, tmp, 2000, "mixed")
    mixed = s["a_leaf"].copy()
    mixed[37:167] = s["b_leaf"][37:167]
    d = rtx.DeviceScene(s["ha"])
    d.update_prims(s["b_leaf"][37:167], first=37)
    nodes, f4 = rtx.scene_trees(d)
    info, f4_a = rtx.fast_tree(s["ha"])
    assert nodes.tobytes() == rtx.bvh_refit(s["ha"].arrays()["nodes"], rtx.prim_bounds(mixed)).tobytes()
    assert f4.tobytes() == np_refit_f4(f4_a, mixed).tobytes()
    # a scene built from the mixed table: list order restored through A's permutation
    idx = s["ha"].prim_indices()
    listed = np.zeros_like(mixed)
    listed[idx] = mixed
    fm = fx.write_scene(tmp / "upd_partial.rtxs", listed)
    dm = rtx.DeviceScene(rtx.HostScene.load(fm))
    ref = orc.Scene(fm).intersect(s["rays"])
    for prec in ("parity", "fast"):
        got = hit_matrix(d.intersect(s["rays"], precision=prec))
        assert same_hits(got, hit_matrix(dm.intersect(s["rays"], precision=prec))), prec
        assert same_hits(got, ref), prec


# ---- renders and films ------------------------------------------------------------------------
def cameras(rtx, orc, prims):
    """The same 64 x 36 camera for the product and the oracle, looking at the grid."""
    mid, rad = fx.frame(prims)
    lookfrom = [float(v) for v in mid + rad * np.array([1.1, 0.7, 1.3])]
    lookat = [float(v) for v in mid]
    cam = rtx.camera(rtx.camera_config("c1_three", width=64, aspect=16.0 / 9.0, vfov=50.0, lookfrom=tuple(lookfrom),
                                       lookat=tuple(lookat), vup=(0.0, 1.0, 0.0), defocus=0.0))
    cfg = orc.camera_preset("c1_three", aspectRatio=16.0 / 9.0, vfov=50.0, lookfrom=lookfrom, lookat=lookat,
                            vup=[0.0, 1.0, 0.0], defocusAngle=0.0)
    assert (cam.image_width, cam.image_height) == (64, 36)
    return cam, cfg


@pytest.mark.parametrize("n,variant", [(67, "mixed"), (2000, "mixed"), (2000, "tri")])
def test_renders_after_an_update(rtx_mod, orc, gpu, tmp, n, variant):
    rtx = rtx_mod
    s = setup(rtx, tmp, n, variant)
    cam, cfg = cameras(rtx, orc, s["b"])
    kw = dict(spp=4, max_depth=8, seed=2024, adaptive=False)
    db = fresh_b(rtx, orc, s)[0]
    d = rtx.DeviceScene(s["ha"])
    d.update_prims(s["b_leaf"])
    ref, _, ref_st = orc.Scene(s["fb"]).render(cfg, 64, 4, 8, 2024, adaptive=0, rng="philox", mode="per_pixel", threads=8)
    ref = np.ascontiguousarray(ref.reshape(-1, 3))
    wp, _, st = d.render(cam, mode="wavefront", precision="parity", **kw)
    print("wavefront/parity vs oracle: rms %.3g, exact pixels %.4f" % (np.sqrt(np.mean((wp - ref) ** 2)),
                                                                       np.all(wp == ref, 1).mean()))
    assert st["rays_total"] == ref_st["rays"] and st["rays_total"] > 64 * 36 * 4, "some paths must bounce"
    assert wp.tobytes() == ref.tobytes()
    pf, _, _ = d.render(cam, mode="persistent", precision="fast", **kw)
    pf_b, _, _ = db.render(cam, mode="persistent", precision="fast", **kw)
    wp_b, _, _ = db.render(cam, mode="wavefront", precision="parity", **kw)
    assert pf_b.tobytes() == wp_b.tobytes(), "the fixture has a tie (fails with or without updates)"
    assert pf.tobytes() == pf_b.tobytes()
    assert wp.tobytes() == wp_b.tobytes()


def test_films_and_refused_updates(rtx_mod, orc, gpu, tmp):
    rtx = rtx_mod
    s = setup(rtx, tmp, 67, "mixed")
    cam, _ = cameras(rtx, orc, s["b"])
    d = rtx.DeviceScene(s["ha"])
    film = d.film(cam, max_depth=8, seed=5, adaptive=False, mode="wavefront")
    film.render(2)
    d.update_prims(s["b_leaf"])
    for call in (lambda: film.render(4), film.resolve, film.p3, film.save):
        with pytest.raises(rtx.RtxError, match="scene changed since the film was created"):
            call()
    assert film.samples == 2
    film.reset()
    assert film.samples == 0
    film.render(4)
    one, one_spp, _ = d.render(cam, spp=4, max_depth=8, seed=5, adaptive=False, mode="wavefront")
    rgb, spp = film.resolve()
    assert rgb.tobytes() == one.tobytes() and np.array_equal(spp, one_spp)
    # refused updates leave the scene as it is
    before = hit_matrix(d.intersect(s["rays"]))
    epoch = d.epoch()
    k = s["b_leaf"]["kind"]
    bad_kind = s["a_leaf"][:8].copy()
    bad_kind[3]["kind"] = fx.SPHERE if k[3] != fx.SPHERE else fx.TRIANGLE
    bad_mat = s["a_leaf"][:8].copy()
    bad_mat[7]["material"] = 67
    neg_mat = s["a_leaf"][:8].copy()
    neg_mat[0]["material"] = -1
    nan = s["a_leaf"][:8].copy()
    nan[5]["g"][0] = np.nan
    inf = s["a_leaf"][:8].copy()
    inf[2]["g"][1] = np.inf
    for what, prims, first in (("kind", bad_kind, 0), ("material", bad_mat, 0), ("material", neg_mat, 0),
                               ("finite", nan, 0), ("finite", inf, 0), ("range", s["a_leaf"][:8], 60),
                               ("range", s["a_leaf"][:8], -1), ("range", s["a_leaf"], 1)):
        with pytest.raises(rtx.RtxError, match=what):
            d.update_prims(prims, first=first)
    with pytest.raises(rtx.RtxError, match="range"):
        d.update_geometry_device(0, 66, 2)
    assert d.epoch() == epoch
    after = hit_matrix(d.intersect(s["rays"]))
    assert same_hits(after, before) and same_hits(after, fresh_b(rtx, orc, s)[2])
    film.render(6)  # nothing was applied: the film is still current


def test_flat_list_scene_updates_its_records(rtx_mod, orc, gpu, tmp):
    """A scene without nodes only rewrites the primitive records."""
    rtx = rtx_mod
    s = setup(rtx, tmp, 67, "mixed")
    la = fx.write_scene(tmp / "upd_list_a.rtxs", s["a"], bvh=0)
    lb = fx.write_scene(tmp / "upd_list_b.rtxs", s["b"], bvh=0)
    d = rtx.DeviceScene(rtx.HostScene.load(la))
    d.update_prims(s["b"])
    assert d.epoch() == 1
    ref = orc.Scene(lb).intersect(s["rays"])
    for prec in ("parity", "fast"):
        assert same_hits(hit_matrix(d.intersect(s["rays"], precision=prec)), ref), prec
