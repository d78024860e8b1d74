"""In-place scene updates, the half that needs no GPU: the new entry points exist and refuse NULL
handles, rtx_bvh_refit_host reproduces the host builder's node boxes from the primitives' boxes
(the union claim the device refit rests on), and the A / B fixtures of
test_scene_update_gpu.py have no two primitives at one ray's closest t, so the GPU half compares
records without a tie allowance."""
import ctypes as C

import numpy as np
import pytest

import scene_update_fixture as fx
from conftest import scene_path

NEW = ["rtx_scene_update_prims", "rtx_scene_update_geometry_device", "rtx_scene_epoch", "rtx_bvh_refit_host",
       "rtx_film_reset"]
BVH_SCENES = ["three", "cornell", "final", "bunny", "rects"]


def test_new_symbols_are_exported_and_refuse_null(rtx_mod):
    L = rtx_mod.lib()
    for name in NEW:
        assert name in rtx_mod.EXPORTS and hasattr(L, name)
    prim = np.zeros(1, rtx_mod.PRIM_DTYPE)
    e = C.c_int64(7)
    assert L.rtx_scene_update_prims(None, 0, 1, prim.ctypes.data_as(C.c_void_p)) == -1
    assert b"NULL" in L.rtx_last_error()
    assert L.rtx_scene_update_prims(None, 0, 0, None) == -1
    assert L.rtx_scene_update_geometry_device(None, 0, 1, None, None) == -1
    assert L.rtx_scene_epoch(None, C.byref(e)) == -1 and e.value == 7
    assert L.rtx_film_reset(None) == -1
    assert L.rtx_bvh_refit_host(None, 1, None, 1) == -1
    assert L.rtx_bvh_refit_host(None, 0, None, 0) == 0


def numpy_refit(nodes, bounds):
    """Bottom-up union over the unchanged topology (children come after their parent)."""
    out = nodes.copy()
    for i in range(len(out) - 1, -1, -1):
        n = out[i]
        if n["is_leaf"]:
            b = bounds[n["left_first"]:n["left_first"] + n["right_count"]]
            lo, hi = b[:, :3].min(0), b[:, 3:].max(0)
        else:
            l, r = out[n["left_first"]], out[n["right_count"]]
            lo, hi = np.minimum(l["lo"], r["lo"]), np.maximum(l["hi"], r["hi"])
        out[i]["lo"], out[i]["hi"] = lo, hi
    return out


def tree_of(rtx, name):
    """(nodes, primitives in leaf order) of a golden scene; `three` and `rects` are flat lists in
    their files, so the host builder makes their tree here."""
    arr = rtx.HostScene.load(scene_path(name)).arrays()
    nodes, prims = arr["nodes"], arr["prims"]
    if len(nodes) == 0:
        nodes, idx = rtx.bvh_build(rtx.prim_bounds(prims), on="host")
        prims = prims[idx]
    assert len(nodes) >= 1
    return nodes, prims


@pytest.mark.parametrize("name", BVH_SCENES)
def test_refit_reproduces_the_builder(rtx_mod, name):
    """Node boxes zeroed and refit over rtx_prim_bounds of the scene's own primitives are the
    builder's nodes, byte for byte: a node's box is the plain union of its primitives' boxes."""
    nodes, prims = tree_of(rtx_mod, name)
    blank = nodes.copy()
    blank["lo"], blank["hi"] = 0.0, 0.0
    got = rtx_mod.bvh_refit(blank, rtx_mod.prim_bounds(prims))
    assert got.tobytes() == nodes.tobytes()


@pytest.mark.parametrize("name", ["cornell", "bunny", "rects"])
def test_refit_on_moved_geometry(rtx_mod, name):
    nodes, prims = tree_of(rtx_mod, name)
    prims = prims.copy()
    rng = np.random.default_rng(11)
    used = {fx.SPHERE: 3, fx.TRIANGLE: 9}
    for p in prims:  # move every primitive by its own offset
        k = used.get(int(p["kind"]), 5)
        p["g"][:k] += rng.uniform(-0.75, 0.75, k) if p["kind"] != fx.TRIANGLE else np.tile(rng.uniform(-0.75, 0.75, 3), 3)
    bounds = rtx_mod.prim_bounds(prims)
    got = rtx_mod.bvh_refit(nodes, bounds)
    want = numpy_refit(nodes, bounds)
    assert got.tobytes() == want.tobytes()
    assert got.tobytes() != nodes.tobytes()
    for f in ("left_first", "right_count", "is_leaf"):
        assert np.array_equal(got[f], nodes[f])


def test_refit_refuses_bad_nodes(rtx_mod):
    arr = rtx_mod.HostScene.load(scene_path("cornell")).arrays()
    nodes, bounds = arr["nodes"], rtx_mod.prim_bounds(arr["prims"])
    with pytest.raises(rtx_mod.RtxError, match="leaf range"):
        rtx_mod.bvh_refit(nodes, bounds[:-1])
    inner = np.nonzero(nodes["is_leaf"] == 0)[0]
    if len(inner):
        bad = nodes.copy()
        bad[inner[0]]["left_first"] = inner[0]
        with pytest.raises(rtx_mod.RtxError, match="pre-order"):
            rtx_mod.bvh_refit(bad, bounds)


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("scene_update")


@pytest.mark.parametrize("variant", fx.VARIANTS)
@pytest.mark.parametrize("n", fx.COUNTS)
def test_fixture_has_no_ties(rtx_mod, orc, tmp, n, variant):
    """A and B hold the same kinds and materials, and in B no ray of the fixture's 4000 has two
    primitives at its closest t (oracle brute force), so records must agree exactly."""
    a, b, fa, fb, rays = fx.pair(rtx_mod, tmp, n, variant)
    assert np.array_equal(a["kind"], b["kind"]) and np.array_equal(a["material"], b["material"])
    assert not np.array_equal(a["g"], b["g"])
    assert len(set(b["material"])) == n and rays.shape == (fx.N_RAYS, 6)
    ha, hb = rtx_mod.HostScene.load(fa), rtx_mod.HostScene.load(fb)
    assert ha.desc().n_prims == n and hb.desc().n_nodes >= 1
    osc = orc.Scene(fb)
    ref = osc.intersect(rays)
    hit = np.nonzero(ref[:, 0] == 1)[0]
    assert len(hit) >= 200, len(hit)  # a few thin triangles catch few rays; the large scenes 3000 and more
    if n >= 1000:
        assert len(set(ref[hit, 11].astype(int))) >= 300
    for i in hit:
        assert osc.tied_hits(rays[i], ref[i, 1])[1] == 1, i
