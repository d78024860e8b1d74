"""The crafted box sets of tests/bvh_build_cases.py on the CPU.

Power: from the host builder's output, each family does what it claims (the root splits, T
primitives go left, two split planes really tie, the chain is deep, 1 / extent = inf makes a
leaf, the odd zero's sign reaches a node box), so the device-against-host comparison on the
same cases (tests/test_bvh_build.py) is aimed and not lucky.

Pinning: the same cases written as .rtxs scenes, the host builder against the oracle's own
builder (oracle/rtx_oracle.cc) byte for byte, off the four golden scenes.

Refusals: both raw-box entry points refuse NaN and infinite bounds on the host, before any
device call, so the device entry point's refusal runs here too.
"""
import numpy as np
import pytest

import bvh_build_cases as cases

SCENE_FAMILIES = ["partition_T", "cost_ties", "bin_edges", "signed_zero_positions", "chains"]  # every case a scene


def params(fam):
    return [pytest.param(b, id=name) for name, b in cases.family(fam)]


def all_params():
    return [pytest.param(fam, b, id=f"{fam}-{name}") for fam in cases.FAMILIES for name, b in cases.family(fam)]


def build(rtx_mod, b):
    return rtx_mod.bvh_build(b, on="host")


def subtree_prims(nodes, idx, i):
    """Original primitive ids under node i, in leaf order."""
    out, stack = [], [i]
    while stack:
        q = nodes[stack.pop()]
        if q["is_leaf"]:
            out.extend(idx[q["left_first"]:q["left_first"] + q["right_count"]].tolist())
        else:
            stack += [int(q["right_count"]), int(q["left_first"])]
    return out


def depth(nodes):
    """Nodes on the longest root-to-leaf path."""
    d = np.zeros(len(nodes), np.int64)
    d[0] = 1
    for i, q in enumerate(nodes):  # pre-order: parents come first
        if not q["is_leaf"]:
            d[q["left_first"]] = d[q["right_count"]] = d[i] + 1
    return int(d.max())


def area(lo, hi):
    dx, dy, dz = (float(hi[a]) - float(lo[a]) for a in range(3))
    return 2.0 * (dx * dy + dy * dz + dz * dx)


def root_split_costs(b):
    """The root's 15 split costs with the builder's formula (SahBuilder::Emit), in Python
    floats (IEEE doubles, one rounding per operation): [(cost or None, left count)], axis."""
    c = cases.centroids(b)
    ext = c.max(0) - c.min(0)
    axis = 0 if ext[0] >= ext[1] and ext[0] >= ext[2] else (1 if ext[1] >= ext[2] else 2)
    mn, inv = float(c[:, axis].min()), 1.0 / float(ext[axis])
    bins = np.array([min(15, int((float(v) - mn) * inv * 16)) for v in c[:, axis]])
    A = area(b[:, :3].min(0), b[:, 3:].max(0))
    out = []
    for i in range(15):
        L, R = b[bins <= i], b[bins > i]
        if len(L) == 0 or len(R) == 0:
            out.append((None, len(L)))
            continue
        cost = 1.0 + (area(L[:, :3].min(0), L[:, 3:].max(0)) / A) * len(L) * 1.0 + \
            (area(R[:, :3].min(0), R[:, 3:].max(0)) / A) * len(R) * 1.0
        out.append((cost, len(L)))
    return out, axis


# ---------------------------------------------------------------------------------- power
@pytest.mark.parametrize("b", params("root_sizes") + params("partition_T") + params("bin_edges"))
def test_power_root_is_internal(rtx_mod, b):
    nodes, idx = build(rtx_mod, b)
    assert not nodes[0]["is_leaf"] and nodes[0]["left_first"] == 1
    assert sorted(idx.tolist()) == list(range(len(b)))


@pytest.mark.parametrize("name,b", [pytest.param(n, b, id=n) for n, b in cases.partition_T()])
def test_power_partition_sends_T_left(rtx_mod, name, b):
    nodes, idx = build(rtx_mod, b)
    want = np.nonzero(cases.centroids(b)[:, 0] < 50.0)[0]
    assert len(want) == cases.partition_T_target(name)
    left = subtree_prims(nodes, idx, 1)
    assert sorted(left) == want.tolist()
    assert sorted(idx[:len(want)].tolist()) == want.tolist()  # ... and they fill the first T slots


def test_power_partition_covers_every_T():
    got = {(len(b), cases.partition_T_target(n)) for n, b in cases.partition_T()}
    for n in (257, 600):
        for T in (1, 2, 63, 64, 65, 255, 256, 257, n - 2, n - 1):
            if T < n:
                assert (n, T) in got
    assert len(cases.partition_T()) == 3 * len(got)  # three input orders each


@pytest.mark.parametrize("name,b", [pytest.param(n, b, id=n) for n, b in cases.cost_ties()])
def test_power_cost_ties_have_two_equal_minima(rtx_mod, name, b):
    costs, _ = root_split_costs(b)
    valid = [c for c, _ in costs if c is not None]
    best = min(valid)
    assert sum(c == best for c in valid) >= 2, costs
    assert best < len(b)  # the root does split
    first = next(i for i, (c, _) in enumerate(costs) if c == best)
    nodes, idx = build(rtx_mod, b)
    assert not nodes[0]["is_leaf"]
    assert len(subtree_prims(nodes, idx, 1)) == costs[first][1]  # `cost < best` kept the first
    if name.startswith("mirror"):  # the tie is between mirrored planes, not only between neighbours
        assert costs[first][1] != next(n for c, n in reversed(costs) if c == best)


@pytest.mark.parametrize("name,b", [pytest.param(n, b, id=n) for n, b in cases.axis_ties()])
def test_power_axis_ties_split_on_the_first_longest_axis(rtx_mod, name, b):
    nodes, idx = build(rtx_mod, b)
    c = cases.centroids(b)
    ext = c.max(0) - c.min(0)
    axis = cases.AXIS_TIE_AXIS[name]
    assert np.sum(ext == ext.max()) >= 2 and ext[axis] == ext.max()  # a tie, and axis is among the tied
    assert not nodes[0]["is_leaf"]
    left, right = subtree_prims(nodes, idx, 1), subtree_prims(nodes, idx, int(nodes[0]["right_count"]))
    assert c[left, axis].max() < c[right, axis].min()
    for other in set(range(3)) - {axis}:  # ... and on no other axis
        assert not c[left, other].max() < c[right, other].min()


@pytest.mark.parametrize("name,b", [pytest.param(n, b, id=n) for n, b in cases.chains()])
def test_power_chains_are_deep(rtx_mod, name, b):
    nodes, idx = build(rtx_mod, b)
    assert depth(nodes) >= len(b) / 4
    deep = int(nodes[0]["left_first"] if "left" in name else nodes[0]["right_count"])
    assert not nodes[deep]["is_leaf"]  # the deep side is the one the name says


@pytest.mark.parametrize("name,b", [pytest.param(n, b, id=n) for n, b in cases.magnitudes()])
def test_power_magnitudes(rtx_mod, name, b):
    assert np.all(np.isfinite(b)) and np.all(np.isfinite(b[:, :3] + b[:, 3:]))
    nodes, idx = build(rtx_mod, b)
    if cases.is_inv_inf(name):
        c = cases.centroids(b)[:, 0]
        extent = c.max() - c.min()
        assert 0 < extent < 2.0 ** -1024 and len(np.unique(c)) == len(b)
        with np.errstate(over="ignore"):
            assert np.isinf(np.float64(1.0) / extent)
        # were +inf sent to bin 15, the root would split: the case tells the two rules apart
        assert cases.inv_inf_stray_split_cost(b) < len(b)
    if not name.startswith("tiny"):
        assert len(nodes) == 1 and nodes[0]["is_leaf"] and nodes[0]["right_count"] == len(b)
        assert idx.tolist() == list(range(len(b)))
    if name.startswith("huge"):
        with np.errstate(over="ignore"):
            assert np.isinf(area(b[:, :3].min(0), b[:, 3:].max(0)))
    if name.startswith("tiny"):
        assert area(b[:, :3].min(0), b[:, 3:].max(0)) == 0.0


@pytest.mark.parametrize("name,b", [pytest.param(n, b, id=n) for n, b in cases.signed_zero_positions()])
def test_power_signed_zero_reaches_a_node_box(rtx_mod, name, b):
    plain = cases.without_odd_sign(b)
    assert np.array_equal(plain, b) and plain.tobytes() != b.tobytes()  # equal values, one sign differs
    col = [c for c in range(6) if np.all(b[:, c] == 0.0)]
    assert len(col) == 1 and np.signbit(b[:, col[0]]).sum() in (1, len(b) - 1)
    nodes, idx = build(rtx_mod, b)
    pn, pi = build(rtx_mod, plain)
    assert np.array_equal(idx, pi) and np.array_equal(nodes, pn)  # same tree, same values ...
    assert nodes.tobytes() != pn.tobytes()  # ... other bits
    p = int(name.split("_")[1][1:])
    root_changed = nodes[:1].tobytes() != pn[:1].tobytes()
    assert root_changed == (p == 0)  # in the root only position 0 decides


def test_power_odd_boxes(rtx_mod):
    d = dict(cases.odd_boxes())
    assert np.array_equal(d["points_n100"][:, :3], d["points_n100"][:, 3:])
    assert np.all(d["inverted_n300"][:, :3] > d["inverted_n300"][:, 3:])
    nodes, idx = build(rtx_mod, d["identical_n300"])
    assert len(nodes) == 1 and nodes[0]["right_count"] == 300  # zero centroid extent: one leaf
    for k in (0, 2, 4):
        b = d[f"four_same_one_other_at{k}"]
        assert len(b) == 5 and len(np.unique(b, axis=0)) == 2
        nodes, idx = build(rtx_mod, b)
        assert not nodes[0]["is_leaf"]


def test_case_sizes_and_names():
    for fam in cases.FAMILIES:
        names = cases.case_ids(fam)
        assert len(names) == len(set(names)) > 0
        for name, b in cases.family(fam):
            assert b.dtype == np.float64 and b.ndim == 2 and b.shape[1] == 6 and 1 <= len(b) <= 1100, (fam, name)
            assert np.all(np.isfinite(b)), (fam, name)
    assert sorted(len(b) for _, b in cases.root_sizes()) == [5, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1025]
    assert {int(n.split("_")[1][1:]) for n in cases.case_ids("signed_zero_positions")} == {0, 1, 63, 64, 255, 256, 299}


# ------------------------------------------------------------------- host against the oracle
def test_required_families_are_scenes():
    for fam in SCENE_FAMILIES:
        for name, b in cases.family(fam):
            assert cases.scene_text(b) is not None, (fam, name)
    for name, b in cases.magnitudes():
        if cases.is_inv_inf(name):
            assert cases.scene_text(b) is not None, name


@pytest.mark.parametrize("fam,b", [p for p in all_params() if cases.scene_text(p.values[1]) is not None])
def test_host_scene_build_equals_oracle(rtx_mod, orc, tmp_path, fam, b):
    path = tmp_path / "case.rtxs"
    path.write_text(cases.scene_text(b))
    host = rtx_mod.HostScene.load(str(path))
    a = host.arrays()
    n, idx = a["nodes"], host.prim_indices()
    # the scene's primitives have exactly the case's boxes, so this is the case the GPU test runs
    leaf_bounds = rtx_mod.prim_bounds(a["prims"])
    orig = np.zeros_like(leaf_bounds)
    orig[idx] = leaf_bounds
    assert orig.tobytes() == np.ascontiguousarray(b).tobytes()
    boxes = np.stack([n["lo"][:, 0], n["hi"][:, 0], n["lo"][:, 1], n["hi"][:, 1], n["lo"][:, 2], n["hi"][:, 2]], 1)
    links = np.stack([n["left_first"], n["right_count"], n["is_leaf"]], 1).astype(np.uint32)
    oboxes, olinks, oprims = orc.Scene(str(path)).bvh()
    assert len(n) == len(olinks)
    assert np.ascontiguousarray(boxes).tobytes() == oboxes.tobytes()
    assert np.ascontiguousarray(links).tobytes() == olinks.tobytes()
    assert idx.astype(np.int32).tobytes() == oprims.tobytes()
    # ... and the raw-box entry point gives the scene's tree
    rn, ri = build(rtx_mod, b)
    assert rn.tobytes() == n.tobytes() and np.array_equal(ri.astype(np.int64), idx.astype(np.int64))


# ------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("on", ["gpu", "host"])
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf], ids=["nan", "inf", "neginf"])
@pytest.mark.parametrize("col", [1, 5], ids=["lo", "hi"])
@pytest.mark.parametrize("box", [0, -1], ids=["first", "last"])
def test_non_finite_bounds_are_refused(rtx_mod, on, bad, col, box):
    """Checked on the host before any device call, so on="gpu" needs no GPU here."""
    b = cases.root_sizes()[3][1].copy()  # 65 boxes
    b[box, col] = bad
    with pytest.raises(rtx_mod.RtxError) as e:
        rtx_mod.bvh_build(b, on=on)
    msg = str(e.value)
    assert "(-1)" in msg  # RTX_ERR_INVALID
    assert f"box {box % len(b)} " in msg and "rtx_bvh_build" + ("_host" if on == "host" else ":") in msg


def test_first_offending_box_is_named(rtx_mod):
    b = cases.root_sizes()[3][1].copy()
    b[40, 3], b[12, 2], b[64, 0] = np.nan, -np.inf, np.inf
    for on in ("gpu", "host"):
        with pytest.raises(rtx_mod.RtxError, match="box 12 "):
            rtx_mod.bvh_build(b, on=on)


def test_largest_finite_box_is_accepted(rtx_mod):
    b = np.array([[-1.7e308] * 3 + [1.7e308] * 3, [-1.0] * 3 + [1.0] * 3])
    nodes, idx = build(rtx_mod, b)
    assert len(nodes) == 1 and nodes[0]["is_leaf"] and idx.tolist() == [0, 1]
    assert nodes[0]["lo"].tolist() == [-1.7e308] * 3 and nodes[0]["hi"].tolist() == [1.7e308] * 3
