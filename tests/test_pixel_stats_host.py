"""The pixel statistics on crafted sample streams, CPU side (no GPU): the oracle's replay
(orc_pixel_replay: record_sample / is_converged, the AdaptiveSampler loop the golden megakernel
renders pin) against the reference's own compiled RecordSample / IsConverged
(tests/golden/pixelstate_edges.npz), and the power of the table the device tests
(tests/test_gpu_pixel_stats.py) compare on: the conditions under which a subtly wrong kernel could
not pass them.
"""
import os

import numpy as np
import pytest

import pixel_stat_cases as psc
from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def default_replay(orc):
    return orc.pixel_replay("adaptive", psc.main_table()[0], psc.MIN0, psc.REL0)


def test_replay_matches_reference_fixture(orc):
    """Record by record, bit for bit: mean, m2, sum after every sample, and IsConverged's answer for
    every (rel, min_spp) pair; the replay's own outputs are the statistics at the first converged
    record (or at the end of the stream)."""
    z = np.load(os.path.join(GOLDEN, "pixelstate_edges.npz"))
    streams = psc.unpack_streams(z["seq"])
    assert 300 <= sum(len(s) for s in streams) <= 1000 and len(z["rel"]) == len(psc.PAIRS)
    ends = np.cumsum([len(s) for s in streams])
    for j, (rel, mn) in enumerate(zip(z["rel"], z["min_spp"])):
        assert (rel, mn) == psc.PAIRS[j] or (np.isinf(rel) and np.isinf(psc.PAIRS[j][0]))
        for s, e in zip(streams, ends):
            want, conv = z["out"][e - len(s):e], z["conv"][j][e - len(s):e]
            r = orc.pixel_replay("adaptive", s[None], int(mn), float(rel), records=True)
            rec = r["records"][0]
            assert np.array_equal(psc.bits(rec[:, :9]), psc.bits(want)), (rel, mn)
            assert np.array_equal(rec[:, 9].astype(np.uint8), conv), (rel, mn)
            stop = int(np.argmax(conv)) if conv.any() else len(s) - 1
            assert r["samples"][0] == stop + 1 and r["conv"][0] == conv.any()
            for k, name in ((0, "mean"), (3, "m2"), (6, "sum")):
                assert np.array_equal(psc.bits(r[name][0]), psc.bits(want[stop, k:k + 3]))


def test_fixture_streams_are_the_tables_rows():
    z = np.load(os.path.join(GOLDEN, "pixelstate_edges.npz"))
    assert np.array_equal(psc.bits(z["seq"]), psc.bits(psc.pack_streams(psc.fixture_streams())))


def test_table_shape_and_families():
    table, family, names, _ = psc.main_table()
    assert table.shape == (psc.NPIX, psc.BUDGET, 3) and psc.NPIX == 1073
    assert all(psc.NPIX % m and psc.WIDTH % m for m in (16, 32, 64))
    for i, name in enumerate(names):
        assert np.count_nonzero(family == i) >= 12, name
    for t in (psc.long_table(), psc.mk_table()):
        assert t.shape[0] % 16 and t.shape[0] * t.shape[1] <= 2000 * 200


def test_constant_rows_have_zero_m2(orc, default_replay):
    rows = psc.rows_of("constant")
    r = orc.pixel_replay("fixed", psc.main_table()[0][rows], 0, 0.0)
    assert not r["m2"].any()
    assert (default_replay["samples"][rows] == psc.MIN0).all()


def test_near_threshold_rows_sit_on_a_flip(orc):
    """At least 64 rows whose decision at sample n changes within +-4 ulps of their amplitude."""
    table, family, names, notes = psc.main_table()
    on_flip = 0
    for p in psc.rows_of("near_threshold"):
        rel, n, mean, a = notes[p]
        d = {psc.decision(mean, psc.ulps(a, k), n, rel) for k in range(-4, 5)}
        on_flip += len(d) == 2
    print("near-threshold rows within 4 ulps of a flip:", on_flip)
    assert on_flip >= 64


def test_near_threshold_rows_reach_their_flip(orc):
    """... and under their own (rel, min_spp) the pixel is still sampling when sample n arrives."""
    table, family, names, notes = psc.main_table()
    for rel, mn in psc.PAIRS[:2] + [(1.0, psc.MIN0)]:
        rows = [p for p in psc.rows_of("near_threshold") if notes[p][0] == rel]
        r = orc.pixel_replay("adaptive", table[rows], mn, rel)
        assert len(rows) >= 18 and all(r["samples"][i] >= notes[p][1] for i, p in enumerate(rows))


def test_cancellation_rows_depend_on_the_order(orc):
    """Summed in reverse order, at least 90 % of the cancellation rows change a bit of sum."""
    rows = psc.main_table()[0][psc.rows_of("cancellation")]
    fwd = orc.pixel_replay("fixed", rows, 0, 0.0)["sum"]
    rev = orc.pixel_replay("fixed", rows[:, ::-1], 0, 0.0)["sum"]
    changed = (psc.bits(fwd) != psc.bits(rev)).any(axis=1)
    print("cancellation rows that change:", changed.sum(), "of", len(rows))
    assert changed.mean() >= 0.9 and len(rows) >= 36


def test_negative_rel_is_not_its_absolute_value(orc, default_replay):
    """err / mu > -0.05 holds for every finite pixel, so it never converges: an implementation
    that squares rel (|rel|) cannot pass."""
    table = psc.main_table()[0]
    neg = orc.pixel_replay("adaptive", table, psc.MIN0, -0.05)
    pos = orc.pixel_replay("adaptive", table, psc.MIN0, 0.05)
    differ = np.count_nonzero(neg["samples"] != pos["samples"])
    print("rows whose counts differ between rel -0.05 and +0.05:", differ)
    assert differ >= 100


def test_rows_stop_where_they_were_built_to(orc, default_replay):
    table, family, names, notes = psc.main_table()
    for p in psc.rows_of("stops_at"):
        assert default_replay["samples"][p] == notes[p] and default_replay["conv"][p] == 1
    heavy = psc.rows_of("heavy_tailed")
    assert (default_replay["samples"][heavy] == psc.BUDGET).all() and not default_replay["conv"][heavy].any()
    # the table spreads the stopping points: every phase geometry gets pixels
    assert len(np.unique(default_replay["samples"])) >= 30


def test_pairs_change_the_counts(orc, default_replay):
    table = psc.main_table()[0]
    seen = {psc.PAIRS[0]: default_replay["samples"]}
    for rel, mn in psc.PAIRS[1:]:
        seen[(rel, mn)] = orc.pixel_replay("adaptive", table, mn, rel)["samples"]
    assert (seen[(psc.REL0, psc.BUDGET + 1)] == psc.BUDGET).all()
    assert (seen[(psc.REL0, 0)] == 1).all() and (seen[(1e-3, 1)] == 1).all()  # var = 0 at one sample
    distinct = {s.tobytes() for s in seen.values()}
    assert len(distinct) >= 8


def test_megakernel_rows_stop_at_min_and_run_past_max(orc):
    t = psc.mk_table()
    for mn, thr in psc.MK_SETTINGS:
        r = orc.pixel_replay("mk_adaptive", t, mn, thr)
        # (at one sample sum_sq - mean * mean is x * x - x * x: min_samples 1 stops nearly every row there)
        assert np.count_nonzero(r["samples"] == psc.MK_MAX + 1) >= (20 if mn > 1 else 1), (mn, thr)
        assert np.count_nonzero(r["samples"] == max(mn, 1)) >= 20, (mn, thr)
    # first sample c then zeros: the variance of the constant running sum rounds below zero for some
    # c (a NaN error: the pixel goes on past min, some to max + 1) and not for others (it stops at min)
    n = orc.pixel_replay("mk_adaptive", t[:126], 5, 0.05)["samples"]
    assert np.count_nonzero(n == 5) >= 20 and np.count_nonzero(n > 5) >= 20 and np.count_nonzero(n == psc.MK_MAX + 1) >= 1
