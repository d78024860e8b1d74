"""The pixel-statistics kernels on crafted sample streams, against the CPU oracle, bit for bit.

k_adapt_record / _plan / _floor / _expand, k_accumulate, k_accumulate_sum,
k_accumulate_mk_adaptive and k_resolve turn radiance records into pixels; rendered frames reach
them only with positive radiance far from the convergence threshold, at the frames' own group
sizes.  Here two test hooks run the shipped launches on tables of samples
(tests/pixel_stat_cases.py; their power is asserted on the CPU in tests/test_pixel_stats_host.py):

  rtx.adaptive_replay     render_adaptive's own phase loop, each phase's persistent launch
                          replaced by a gather of the phase's slots from the table
  rtx.accumulate_groups   render_device_impl's accumulate launches over uniform groups

Every comparison is of bits, with the NaN positions equal (a NaN's sign and payload are the
processor's choice); every row counts.
"""
import numpy as np
import pytest

import pixel_stat_cases as psc
from conftest import scene_path

pytestmark = pytest.mark.gpu
RMS_TOL = 1e-4  # tests/test_gpu_parity.py's bound on a frame against the oracle

# rtx.adapt_tune settings: results never depend on them
TUNES = {"default": {}, "kcap4": {"phase_kcap": 4}, "slots64": {"phase_slots": 64}, "first_map0": {"first_map": 0},
         "first_map1": {"first_map": 1}, "unpooled": {"pool_w": 0.0}, "no_margin": {"margin1": 0.0, "phase_mstep": 0.0},
         "wide_margin": {"margin1": 8.0, "phase_mstep": 4.0}, "small_unpooled": {"phase_kcap": 8, "phase_slots": 64,
                                                                                 "pool_w": 0.0}}


def mismatches(got, want):
    """Rows (first axis) where got and want differ: the bits where neither is NaN, NaN against NaN."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype
    if got.dtype.kind == "f":
        nan = np.isnan(got) | np.isnan(want)
        bad = np.where(nan, np.isnan(got) != np.isnan(want), psc.bits(got) != psc.bits(want))
    else:
        bad = got != want
    return np.flatnonzero(bad.reshape(len(got), -1).any(axis=1))


def assert_same(got, want, fields, what):
    bad = {f: mismatches(got[f], want[f]) for f in fields}
    bad = {f: (len(r), r[:8].tolist()) for f, r in bad.items() if len(r)}
    assert not bad, f"{what}: rows that differ (count, first rows) {bad}"


ALL = ("sum", "mean", "m2", "samples", "conv", "rgb")


@pytest.fixture(scope="module")
def dev(rtx_mod, gpu):
    return rtx_mod.DeviceScene(rtx_mod.HostScene.load(scene_path("three")), device=0)


@pytest.fixture(scope="module")
def oracle_adaptive(orc):
    cache = {}

    def get(pair, table=None, key="main"):
        if (pair, key) not in cache:
            t = psc.main_table()[0] if table is None else table
            cache[(pair, key)] = orc.pixel_replay("adaptive", t, pair[1], pair[0])
        return cache[(pair, key)]
    return get


def check_slot_map(r, budget, min_spp, kcap4):
    """Each (pixel, sample) gathered at most once; a pixel's gathered samples are 0 .. m - 1 with
    samples <= m <= budget, m the uniform first pass plus batches that are multiples of 4 unless
    the budget cuts the last (adapt_next_batch); with 4-sample batches (kcap4), m is exactly the
    batch end after the pixel's last record: a converged pixel gets no slot in a later phase."""
    asked, n = r["asked"], r["samples"].astype(np.int64)
    assert asked.max() <= 1
    m = asked.sum(axis=1, dtype=np.int64)
    assert np.array_equal(asked, (np.arange(budget)[None, :] < m[:, None]).astype(np.uint8))
    k1 = min(max(1, min_spp), budget)
    assert (m >= n).all() and (m <= budget).all() and (((m - k1) % 4 == 0) | (m == budget)).all()
    if kcap4:
        end = np.minimum(budget, k1 + 4 * -(-(n - k1) // 4))
        assert np.array_equal(m, np.where(r["conv"] == 1, end, budget))


def run_tunes(rtx_mod, dev, table, width, pair, want, what):
    first = None
    try:
        for name, kw in TUNES.items():
            rtx_mod.adapt_tune(**kw)
            r = rtx_mod.adaptive_replay(dev, table, width, pair[1], pair[0])
            assert_same(r, want, ALL, f"{what} rel {pair[0]!r} min_spp {pair[1]} tune {name}")
            assert np.array_equal(r["spp"], r["samples"])
            check_slot_map(r, table.shape[1], pair[1], name == "kcap4")
            if first is None:
                first = r
            assert_same(r, first, ALL, f"{what} tune {name} against the default")
    finally:
        rtx_mod.adapt_tune()
    return first


@pytest.mark.parametrize("pair", psc.PAIRS, ids=lambda p: f"rel{p[0]!r}-min{p[1]}")
def test_adaptive_replay_equals_oracle(rtx_mod, dev, oracle_adaptive, pair):
    run_tunes(rtx_mod, dev, psc.main_table()[0], psc.WIDTH, pair, oracle_adaptive(pair), "main table")


def test_adaptive_replay_long_budget(rtx_mod, dev, oracle_adaptive):
    """Budget 200, min_spp 16: several phases, batches of every size."""
    t = psc.long_table()
    pair = psc.PAIRS[0]
    want = oracle_adaptive(pair, t, "long")
    assert len(np.unique(want["samples"])) >= 60
    run_tunes(rtx_mod, dev, t, psc.WIDTH, pair, want, "long table")


def groupings(budget, min_spp=psc.MIN0):
    return [[1] * budget, [4] * (budget // 4) + [1] * (budget % 4),
            [min_spp] + [4] * ((budget - min_spp) // 4) + [1] * ((budget - min_spp) % 4), [budget]]


def test_uniform_groups_equal_oracle(rtx_mod, dev, orc, oracle_adaptive, gpu):
    """k_accumulate (the wavefront renderer's and samples_per_group's path) over groups of 1, of 4,
    of 16 then 4s, and one group of the whole budget: the oracle's records, whatever the groups;
    adaptive off: the oracle's fixed-spp statistics; and the phased replay's result."""
    table = psc.main_table()[0]
    want = oracle_adaptive(psc.PAIRS[0])
    for g in groupings(psc.BUDGET):
        r = rtx_mod.accumulate_groups("record_adaptive", table, g, psc.MIN0, psc.REL0)
        assert_same(r, want, ALL, f"k_accumulate adaptive, groups {g[:3]}..")
    for pair in psc.PAIRS[1:]:
        r = rtx_mod.accumulate_groups("record_adaptive", table, [4] * 16, pair[1], pair[0])
        assert_same(r, oracle_adaptive(pair), ALL, f"k_accumulate adaptive, rel {pair[0]!r} min_spp {pair[1]}")
    fixed = orc.pixel_replay("fixed", table, 0, 0.0)
    for g in groupings(psc.BUDGET)[1:]:
        r = rtx_mod.accumulate_groups("record", table, g, psc.MIN0, psc.REL0)
        assert_same(r, fixed, ALL, f"k_accumulate fixed, groups {g[:3]}..")
    replay = rtx_mod.adaptive_replay(dev, table, psc.WIDTH, psc.MIN0, psc.REL0)
    assert_same(rtx_mod.accumulate_groups("record_adaptive", table, [16] + [4] * 12, psc.MIN0, psc.REL0), replay, ALL,
                "k_accumulate against the phased replay")


@pytest.fixture(scope="module")
def sum_rows():
    """The main table with the cancellation rows first: every pixel count takes some."""
    table = psc.main_table()[0]
    first = psc.rows_of("cancellation")
    rest = np.setdiff1d(np.arange(psc.NPIX), first)
    return np.ascontiguousarray(table[np.concatenate([first, rest])])


def splits(k):
    s = [[k]]
    if k >= 2:
        s += [[k // 2, k - k // 2], [1] * k if k <= 3 else [3, k - 3]]
    if k > 4:
        s += [[2, k - 2], [k - 1, 1], [2, 1, k - 3]]
    return s


@pytest.mark.parametrize("k", [1, 2, 3, 7, 8, 9, 15, 16, 17, 24])
def test_fixed_spp_sums(rtx_mod, orc, sum_rows, gpu, k):
    """k_accumulate_sum: the in-order sum and the resolved pixel, as one group and split, whole and
    in bands, for pixel counts around the 16-pixel workgroup."""
    for npix in (1, 15, 16, 17, psc.NPIX):
        table = np.ascontiguousarray(sum_rows[:npix, :k])
        want = orc.pixel_replay("fixed", table, 0, 0.0)
        for g in splits(k):
            r = rtx_mod.accumulate_groups("sum", table, g, resolve=-1)
            assert_same(r, want, ("sum", "samples", "rgb"), f"sum K {k} npix {npix} groups {g} then k_resolve")
            assert (r["spp"] == k).all()
            for resolve, ref in ((0, want["rgb"]), (1, want["rgb_spp"])):
                for bands, align in ((1, 1), (8, 1), (8, 37), (1, 37)):
                    r = rtx_mod.accumulate_groups("sum", table, g, resolve=resolve, bands=bands, align=align)
                    bad = mismatches(r["rgb"], ref)
                    assert not len(bad) and (r["spp"] == k).all(), \
                        f"sum K {k} npix {npix} groups {g} resolve {resolve} bands {bands} align {align}: rows {bad[:8]}"


@pytest.mark.parametrize("setting", psc.MK_SETTINGS, ids=lambda s: f"min{s[0]}-thr{s[1]}")
def test_megakernel_sampler(rtx_mod, orc, gpu, setting):
    """k_accumulate_mk_adaptive over groups of 1, of 4 and of max + 1: the oracle's AdaptiveSampler
    counts and pixels, the rows that run to max + 1 included."""
    mn, thr = setting
    table = psc.mk_table()
    want = orc.pixel_replay("mk_adaptive", table, mn, thr)
    assert (want["samples"] == psc.MK_MAX + 1).any() and (want["samples"] == max(1, mn)).any()
    k = psc.MK_MAX + 1
    for g in ([1] * k, [4] * (k // 4) + [1] * (k % 4), [k]):
        r = rtx_mod.accumulate_groups("mk_adaptive", table, g, mn, thr)
        assert_same(r, want, ALL, f"AdaptiveSampler min {mn} threshold {thr} groups {g[:3]}..")
        assert np.array_equal(r["spp"], r["samples"])


@pytest.mark.parametrize("scene,preset,precision", [("cornell", "cornell", "fast"), ("three", "c1_three", "parity")])
def test_replay_ties_to_the_frames(rtx_mod, orc, gpu, scene, preset, precision):
    """A real frame: the oracle's samples of the scene through the replay hook give the sample
    counts of the device's own adaptive persistent render of that frame (the hook runs the shipped
    phase loop), and its pixels within the frames' bound (in fast precision the device's samples
    differ from the oracle's by the documented cos / sin ulps).  The cornell box at this budget
    samples every pixel to the end; the three spheres stop anywhere from min_spp on."""
    w, budget, depth, seed = 24, 48, 10, 77
    d = rtx_mod.DeviceScene(rtx_mod.HostScene.load(scene_path(scene)), device=0)
    cam = rtx_mod.camera(rtx_mod.camera_config(preset, width=w))
    rgb, spp, _ = d.render(cam, spp=budget, max_depth=depth, seed=seed, adaptive=True, mode="persistent",
                           precision=precision, min_spp=psc.MIN0)
    L, _ = orc.Scene(scene_path(scene)).render_samples(orc.camera_preset(preset), w, budget, depth, seed, threads=4)
    table = np.ascontiguousarray(L.reshape(-1, budget, 3))
    assert len(table) == len(spp)
    r = rtx_mod.adaptive_replay(d, table, w, psc.MIN0, psc.REL0)
    assert np.array_equal(r["samples"], spp)
    if scene == "three":
        assert len(np.unique(spp)) > 8 and (spp == psc.MIN0).sum() > 50 and (spp == budget).sum() > 50
    rms = float(np.sqrt(np.mean((r["rgb"] - rgb) ** 2)))
    assert rms <= RMS_TOL, rms
