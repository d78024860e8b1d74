"""The Lambertian cos/sin comes in three forms (cos_sin, rtx_device.h): the device library's cos()
and sin(), the restated small-argument reduction run once per value, and run once for both.  Which
one a kernel takes is chosen per build by its register allocation alone, so the three must return
the same bits for every angle the sampler can make, and every schedule must still render the frame
the others do: a form picked for one schedule and not another would show there if the first
property ever broke.

The device check (rtx_internal_cos_sin_forms, a test hook of the PARK unit, compiled with the flags
of the kernels that select among the forms) evaluates all three forms for one angle per lane and
counts the angles at which any bit of cos or sin differs."""

import ctypes as C

import numpy as np
import pytest

from conftest import scene_path

pytestmark = pytest.mark.gpu

TWO_PI = 2.0 * 3.14159265358979323846  # 2.0 * kPi, as shade_core forms it


def forms(rtx_mod, phi, seed=0, n_draws=0, want_cs=False):
    f = rtx_mod.lib().rtx_internal_cos_sin_forms
    f.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_uint64, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_double),
                  C.c_void_p]
    f.restype = C.c_int
    phi = np.ascontiguousarray(phi, dtype=np.float64)
    cs = np.zeros((len(phi), 2)) if want_cs else None
    bad, first = C.c_int64(-1), C.c_double(0.0)
    rc = f(0, phi.ctypes.data if len(phi) else None, len(phi), seed, n_draws, C.byref(bad), C.byref(first),
           cs.ctypes.data if want_cs else None)
    assert rc == 0, rtx_mod.lib().rtx_last_error()
    return bad.value, first.value, cs


def steps(x, k):
    """x moved k doubles up (k > 0) or down (k < 0)"""
    for _ in range(abs(k)):
        x = np.nextafter(x, np.inf if k > 0 else -np.inf)
    return float(x)


def test_forms_agree_on_the_sampler_grid(rtx_mod, gpu):
    """r1 is a 53-bit draw k * 2^-53.  A 2^20-point grid of its mantissa, at both ends of every
    cell: the smallest draw of cell j (k = j * 2^33, r1 = j / 2^20; cell 0 gives phi = 0) and the
    largest (k = (j + 1) * 2^33 - 1; the last cell gives the largest r1 below 1)."""
    j = np.arange(1 << 20, dtype=np.uint64)
    lo = (j << np.uint64(33)).astype(np.float64) * 2.0 ** -53
    hi = (((j + np.uint64(1)) << np.uint64(33)) - np.uint64(1)).astype(np.float64) * 2.0 ** -53
    assert lo[0] == 0.0 and hi[-1] == 1.0 - 2.0 ** -53 and hi.max() < 1.0
    r1 = np.concatenate([lo, hi])
    bad, first, _ = forms(rtx_mod, TWO_PI * r1)
    print("grid angles", len(r1), "mismatches", bad)
    assert bad == 0, f"{bad} of {len(r1)} angles differ between the forms, one of them phi = {first!r}"


@pytest.mark.parametrize("seed", [1234, 0x5EED5EED5EED])
def test_forms_agree_on_philox_draws(rtx_mod, gpu, seed):
    """2^16 angles from the first draw of a segment's Philox stream, made on the device by the
    calls shade_core makes (make_rng, next) over pixels, samples and depths."""
    bad, first, _ = forms(rtx_mod, np.zeros(0), seed=seed, n_draws=1 << 16)
    print("philox angles", 1 << 16, "seed", seed, "mismatches", bad)
    assert bad == 0, f"{bad} of 65536 sampler angles differ between the forms, one of them phi = {first!r}"


def test_forms_agree_at_the_ends_and_quadrant_boundaries(rtx_mod, gpu):
    """0, the smallest positive r1 and the largest r1 below 1; for each quadrant boundary k * pi / 2
    (k = 1..3) the double nearest it and 8 doubles either side.  Here the library's values are also
    read back and held against the host's cos and sin: the device library and the host's are each
    within 2 ulp of the exact value, so 4 ulp apart at the most (a guard against three forms that
    agree on nonsense, not a precision claim)."""
    phi = [0.0, TWO_PI * 2.0 ** -53, TWO_PI * (1.0 - 2.0 ** -53)]
    for k in (1, 2, 3):
        b = k * (np.pi / 2)  # k = 1, 2: exact scalings of the nearest double to pi; k = 3: rounded once
        phi += [steps(b, d) for d in range(-8, 9)]
    phi = np.array(phi)
    assert len(phi) == 3 + 3 * 17 and np.all((phi >= 0) & (phi < 2.0 ** 30))
    bad, first, cs = forms(rtx_mod, phi, want_cs=True)
    print("special angles", len(phi), "mismatches", bad)
    assert bad == 0, f"{bad} angles differ between the forms, one of them phi = {first!r}"
    for got, want in ((cs[:, 0], np.cos(phi)), (cs[:, 1], np.sin(phi))):
        ulp = np.maximum(np.spacing(np.abs(want)), np.finfo(np.float64).tiny)
        assert np.all(np.abs(got - want) <= 4 * ulp), (got, want)
    assert cs[0, 0] == 1.0 and cs[0, 1] == 0.0


@pytest.mark.parametrize("depth", [1, 20])
def test_schedules_render_the_same_frame(rtx_mod, gpu, depth):
    """The bunny at 64 x 36, 8 spp: the park, park_step and plain schedules and the wavefront
    renderer give the same pixels and segment counts, bit for bit.  The PARK schedules must have
    run the PARK kernel in its Lambertian texture-free triangle-tree build (the one that takes the
    shared-reduction form), `park` the speculative walk."""
    d = rtx_mod.DeviceScene(rtx_mod.HostScene.load(scene_path("bunny")))
    cam = rtx_mod.camera(rtx_mod.camera_config("c3_bunny", width=64))
    assert (cam.image_width, cam.image_height) == (64, 36)
    kw = dict(spp=8, max_depth=depth, seed=1234, adaptive=False, precision="fast")
    ref, _, ref_st = d.render(cam, mode="wavefront", **kw)
    ref = np.array(ref, copy=True)
    for sched in ("park", "park_step", "plain"):
        rgb, _, st = d.render(cam, mode="persistent", schedule=sched, **kw)
        names = rtx_mod.build_names(st["build"])
        print("depth", depth, sched, "rays", st["rays_total"], "wavefront", ref_st["rays_total"], names)
        assert st["parked"] == (0 if sched == "plain" else 1), (sched, st["parked"])
        if sched != "plain":
            assert {"park", "triangle_tree", "lambertian", "no_textures"} <= set(names), (sched, names)
            assert ("speculative" in names) == (sched == "park"), (sched, names)
        assert st["rays_total"] == ref_st["rays_total"], (sched, st["rays_total"], ref_st["rays_total"])
        assert np.array_equal(np.asarray(rgb).view(np.uint8), ref.view(np.uint8)), (depth, sched)
