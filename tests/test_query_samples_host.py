"""The reference of tests/query_sample_cases.py, on the CPU: its hemisphere sampler has the
moments of a cosine-weighted hemisphere, azimuth included; its light sampler's mean reaches the
closed form under a sphere, a triangle and the three rects; deliberately wrong variants of either
miss by 10 sigma at the same points and sample counts (so the device tests that use them have
power); the shadow segment's end gap does not move a mean; the scan reference is a cumulative sum.
"""
import math

import numpy as np
import pytest

import query_sample_cases as qs

MOMENT_NORMALS = [(1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 2.0, 0.0), (0.3, -0.5, 0.81), (-0.95, 0.2, 0.1)]
# (name, expected mean, analytic variance) of a cosine-weighted direction's components in its
# basis: x = s cos phi, y = s sin phi, z = sqrt(1 - s^2), s^2 and phi / 2 pi uniform
MOMENTS = [("cos", 2.0 / 3.0, 1.0 / 18.0), ("d.u", 0.0, 0.25), ("d.v", 0.0, 0.25), ("d.u d.v", 0.0, 1.0 / 24.0),
           ("(d.u)^2", 0.25, 1.0 / 16.0), ("(d.v)^2", 0.25, 1.0 / 16.0)]


def moment_z(d, n):
    """Each moment's distance from its expectation, in analytic sigmas."""
    u, v, w = qs.basis(n)
    x, y, z = d @ u, d @ v, d @ w
    vals = [z, x, y, x * y, x * x, y * y]
    return np.array([(val.mean() - mean) / math.sqrt(var / len(d)) for val, (_, mean, var) in zip(vals, MOMENTS)])


@pytest.fixture(scope="module")
def moment_draws(orc):
    return [qs.draws(99 + i, 1000 + 7 * i, 0, qs.N_MOMENTS, qs.STREAM_IRR, 2) for i in range(len(MOMENT_NORMALS))]


def test_reference_hemisphere_moments(rtx_mod, orc, moment_draws):
    worst = 0.0
    for n, r in zip(MOMENT_NORMALS, moment_draws):
        d = qs.cosine_from_draws(r, n)
        assert np.abs(np.linalg.norm(d, axis=1) - 1.0).max() <= 1e-15
        z = moment_z(d, n)
        print("normal", n, "z of", [m[0] for m in MOMENTS], np.round(z, 2))
        worst = max(worst, np.abs(z).max())
        assert np.abs(z).max() <= 5.0
    print("largest |z|", worst)
    # the keyed entry point is the same mapping of the same draws
    one = qs.cosine_direction_ref(99, 1000, 3, qs.STREAM_IRR, MOMENT_NORMALS[0], count=2)
    assert one.tobytes() == qs.cosine_from_draws(moment_draws[0][3:5], MOMENT_NORMALS[0]).tobytes()


def test_half_circle_azimuth_is_caught(rtx_mod, orc, moment_draws):
    for n, r in zip(MOMENT_NORMALS, moment_draws):
        z = moment_z(qs.cosine_from_draws(r, n, phi_scale=math.pi), n)
        print("normal", n, "phi = pi r1: z", np.round(z, 1))
        assert np.abs(z[1:4]).max() >= 10.0, "d.u, d.v and their product pin the azimuth"
        assert abs(z[0]) <= 5.0, "the one moment the device tests looked at does not see it"


@pytest.mark.parametrize("name", list(qs.ONE_LIGHT))
def test_reference_light_sampler_reaches_the_closed_form(rtx_mod, orc, name):
    worst = 0.0
    for i, (want, mean, sigma, u) in enumerate(qs.mean_reference(name)):
        z = (mean - want) / sigma
        print(name, "point", i, "closed form", want, "mean", mean, "sigma", sigma, "z", np.round(z, 2))
        assert (sigma > 0.0).all() and (want > 0.0).all()
        worst = max(worst, np.abs(z).max())
        assert np.abs(z).max() <= 3.0
    print(name, "largest |z|", worst)


VARIANTS = [("triangle", "tri_no_sqrt"), ("sphere", "sphere_z"), ("xy_rect", "rect_same_u"),
            ("xz_rect", "rect_same_u"), ("yz_rect", "rect_same_u")]


@pytest.mark.parametrize("name,variant", VARIANTS)
def test_wrong_light_samplers_are_caught(rtx_mod, orc, name, variant):
    L = qs.lights_of(qs.one_light_text(name))
    P, N = qs.one_light_points(name)
    for i, (want, _, sigma, u) in enumerate(qs.mean_reference(name)):
        per = qs.estimator(L, P[i], N[i], u, variant=variant)
        # in the larger of the two spreads: the reference's own and the variant's
        s = np.maximum(sigma, per.std(0, ddof=1) / math.sqrt(len(u)))
        z = (per.mean(0) - want) / s
        print(name, variant, "point", i, "mean", per.mean(0), "closed form", want, "z", np.round(z, 1))
        assert np.abs(z).min() >= 10.0


def test_end_gap_moves_no_mean(rtx_mod, orc):
    """Ending the shadow segment at RTX_DIRECT_TMAX instead of at the light itself changes the
    sphere's mean by less than a tenth of a sigma: that gap is never the cause of a failure."""
    L = qs.lights_of(qs.one_light_text("sphere"))
    P, N = qs.one_light_points("sphere")
    for i, (_, mean, sigma, u) in enumerate(qs.mean_reference("sphere")):
        full = qs.estimator(L, P[i], N[i], u, tmax=1.0).mean(0)
        print("point", i, "mean to 0.9999f", mean, "to 1.0", full, "difference in sigma", (full - mean) / sigma)
        assert (np.abs(full - mean) < 0.1 * sigma).all()
    # and the far side is what the occlusion rejects: about half the samples
    smp, _, _ = qs.samples_from_draws(L, P[0], N[0], qs.mean_reference("sphere")[0][3])
    share = qs.sphere_visible(L.g[0], smp[:, :3], smp[:, 3:6]).mean()
    assert 0.1 < share < 0.5


def test_zero_rows_are_zero_in_the_reference(rtx_mod, orc):
    seen = set()
    for name in qs.ONE_LIGHT:
        L = qs.lights_of(qs.one_light_text(name))
        P, N = qs.zero_rows(name)
        smp, pick, why = qs.direct_table_ref(L, 5, P, N, qs.odd_ids(len(P)), 8)
        assert not smp.any() and (why != qs.TRACED).all()
        seen |= set(why.ravel())
    assert {qs.FACES_AWAY, qs.BAD_NORMAL, qs.EDGE_ON} <= seen
    L = qs.lights_of(qs.MIXED)
    assert sorted(L.kind) == [0, 1, 2, 3, 3, 4]
    P, N = qs.mixed_surfels()
    smp, pick, why = qs.direct_table_ref(L, 5, P, N, qs.odd_ids(len(P)), 8)
    assert {qs.TRACED, qs.FACES_AWAY, qs.BAD_NORMAL, qs.EDGE_ON, qs.BLACK} <= set(why.ravel())
    assert (smp.any(2) == (why == qs.TRACED)).all()
    bright = [e for e in range(len(L.idx)) if L.areas[e] > 0.0 and L.emitted(e, np.zeros((1, 3))).any()]
    assert set(pick[why == qs.TRACED]) == set(bright) and sorted(L.kind[bright]) == [0, 1, 2, 3, 4], "every kind is hit"


@pytest.mark.parametrize("n", qs.TABLE_SIZES + (3, 100000))
def test_scan_reference_is_a_cumulative_sum(n):
    rng = np.random.default_rng(n)
    areas = rng.uniform(0.0, 3.0, n) * (rng.uniform(size=n) > 0.1)
    cum = qs.emitter_cum_ref(areas)
    want = np.cumsum(areas)
    err = np.abs(cum - want).max() / want[-1]
    print("n", n, "max relative difference", err)
    assert err <= 1e-12
    if n <= 256:
        assert cum.tobytes() == want.tobytes()
    elif n >= 1000:
        assert cum.tobytes() != want.tobytes(), "the order of the additions shows"


def test_table_scenes(rtx_mod):
    """The emitter tables' scenes hold what the device test says they hold."""
    for n in qs.TABLE_SIZES:
        L = qs.lights_of(qs.table_scene(n))
        assert len(L.idx) == n and (L.areas >= 0.0).all() and L.cum[-1] > 0.0
        if n >= 3:
            assert L.areas[0] == 0.0 and L.areas[-1] == 0.0
            assert L.kind[n // 2] == qs.SPHERE and L.g[n // 2][3] < 0.0 and L.areas[n // 2] == 0.0
        if n >= 5:
            assert (L.areas == 0.0).sum() == 4
        assert len(np.unique(L.areas)) > min(n, 7) // 2
        # the step back: a draw whose product rounds up to A lands on the last emitter with area
        last = np.flatnonzero(L.areas > 0.0)[-1]
        assert qs.pick_emitter(L.cum, np.array([1.0, np.nextafter(1.0, 0.0), 0.0]))[0] == last
        assert qs.pick_emitter(L.cum, np.array([0.0]))[0] == np.flatnonzero(L.areas > 0.0)[0]
