"""The device shading step against the oracle's shade(), material by material.

rtx_internal_shade_steps (csrc/rtx_shade_steps.h) runs one step per case through the device
functions the render kernels call: shade() as k_wf_shade / k_radiance / k_irradiance call it,
shade_core<LAMB, NOTEX, SET_ORIGIN> + shade_finish as the persistent kernel does, shade_terminal,
and the scatter-API branch (sky / mat_scatter / mat_emitted), on a real device scene, so the
uploaded material table (folded solid colours, the dielectric's eta and r0), the texture and image
tables and the scene flags are the renderer's.  orc_shade_steps is the oracle's shade() / one level
of get_pixel on the same cases.

The rule, for every family and every variant the scene's flags allow: the device record equals the
oracle record bit for bit (flag, child depth, next draw, L, o, d, thr; NaNs by bits), and the
variants equal each other.  The one exception is a Lambertian sample that continues: its record must
equal, as a whole, the oracle's record under one of the 25 nudges of the oracle's cos and sin by
-2..+2 ulps each (the device library's cos / sin against glibc's), its flag, depth and next draw the
un-nudged record's in any case.  A case that matches none fails.  The histogram of matching nudges
is printed (DESIGN.md §1 holds the measured one).

The scatter API's Lambertian near_zero(direction) fallback is reached by construction, not by a key
search: the case's normal is minus the unit vector its key draws (shade_step_cases.scatter_fallback_cases).

The cases are built, and checked for reaching their branches on the oracle alone, in
tests/shade_step_cases.py and tests/test_shade_steps_host.py."""
import numpy as np
import pytest

import shade_step_cases as ssc
from conftest import scene_path

pytestmark = pytest.mark.gpu
_scenes, _device = {}, {}


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("shade_steps")


def scenes(rtx, orc, scene_dir, name):
    """(device scene, oracle scene) of a table of shade_step_cases.SCENES, loaded once."""
    if name not in _scenes:
        path = ssc.write_scene(scene_dir, name)
        _scenes[name] = (rtx.DeviceScene(rtx.HostScene.load(path)), orc.Scene(path))
    return _scenes[name]


def variants_of(name):
    core = ssc.CORE_FORMS[name]
    return ("shade",) + core + tuple(v + "_noorigin" for v in core)


def device_records(rtx, dev, key, cases, variants):
    """The device's records of `cases` through every variant, which must equal each other; once per key."""
    if key not in _device:
        got = {v: rtx.shade_steps(dev, cases, v) for v in variants}
        first = got[variants[0]]
        for v in variants[1:]:
            differ = ~ssc.same(got[v], first)
            assert not differ.any(), (key, v, "differs from", variants[0], "in rows", np.nonzero(differ)[0][:8])
        first.setflags(write=False)
        _device[key] = first
    return _device[key]


def explain(cases, got, base, bad):
    lines = []
    for i in np.nonzero(bad)[0][:6]:
        fields = [k for k in got.dtype.names if not (ssc.rows(got[k][i:i + 1]) == ssc.rows(base[k][i:i + 1])).all()]
        lines.append(f"row {i} mat {cases['mat'][i]} depth {cases['depth'][i]} hit {cases['hit'][i]}: {fields} "
                     f"device {[got[k][i].tolist() for k in fields]} oracle {[base[k][i].tolist() for k in fields]}")
    return "\n".join(lines)


def check(rtx, orc, scene_dir, scene, key, cases, lamb):
    dev, osc = scenes(rtx, orc, scene_dir, scene)
    got = device_records(rtx, dev, key, cases, variants_of(scene))
    nudged = ssc.oracle_nudged(osc, cases)
    bad, hist = ssc.mismatches(got, nudged, lamb)
    free = int((lamb & (nudged[(0, 0)]["cont"] == 1)).sum())
    print(f"{key}: {len(cases)} cases x {len(variants_of(scene))} variants, {int(bad.sum())} mismatches; "
          f"Lambertian samples that continue: {free}, matching nudge (cos, sin) -> rows: {hist}")
    assert not bad.any(), explain(cases, got, nudged[(0, 0)], bad)
    # the persistent kernel's form for a path that ends on the sky
    end = ssc.sky_end(cases)
    if end.any():
        term = rtx.shade_steps(dev, cases[end], "terminal")
        assert (term["cont"] == 0).all()
        assert ssc.same(term, got[end]).all(), key
    return got, hist


def test_sky_and_terminal(rtx_mod, orc, gpu, scene_dir):
    f = ssc.family("sky")
    assert ssc.sky_end(f["cases"]).all()
    got, _ = check(rtx_mod, orc, scene_dir, "table", "sky", f["cases"], f["lamb"])
    assert (got["cont"] == 0).all() and len(np.unique(got["L"], axis=0)) > 50


def test_lambertian(rtx_mod, orc, gpu, scene_dir):
    f = ssc.family("lambertian")
    got, hist = check(rtx_mod, orc, scene_dir, "table", "lambertian", f["cases"], f["lamb"])
    n = sum(hist.values())
    print(f"lambertian: matched at 0/0: {hist.get((0, 0), 0)} of {n} ({100.0 * hist.get((0, 0), 0) / n:.2f} %)")
    assert n > 1000 and (got["cont"] == 0).any()


def test_metal(rtx_mod, orc, gpu, scene_dir):
    f = ssc.family("metal")
    got, _ = check(rtx_mod, orc, scene_dir, "table", "metal", f["cases"], f["lamb"])
    go = got["cont"][f["fuzzed"] & (f["cases"]["depth"] < 5)] == 1
    assert 0.05 <= go.mean() <= 0.95


def test_dielectric(rtx_mod, orc, gpu, scene_dir):
    f = ssc.family("dielectric")
    got, _ = check(rtx_mod, orc, scene_dir, "table", "dielectric", f["cases"], f["lamb"])
    what = ssc.dielectric_outcomes(f["cases"], got)
    assert min((what == k).mean() for k in ("tir", "reflect", "refract")) >= 0.05


def test_emitter(rtx_mod, orc, gpu, scene_dir):
    f = ssc.family("emitter")
    got, _ = check(rtx_mod, orc, scene_dir, "table", "emitter", f["cases"], f["lamb"])
    assert (got["cont"] == 0).all() and (got["L"] != 0).any()


def test_scatter_api(rtx_mod, orc, gpu, scene_dir):
    dev, osc = scenes(rtx_mod, orc, scene_dir, "table")
    parts = [ssc.scatter_form(ssc.family(k)["cases"]) for k in ssc.FAMILIES] + [ssc.scatter_fallback_cases()]
    cases = np.concatenate(parts)
    got = rtx_mod.shade_steps(dev, cases, "scatter")
    ref = orc.shade_steps(osc, cases, scatter=True)
    bad = ~ssc.same(got, ref)
    print(f"scatter: {len(cases)} cases, {int(bad.sum())} mismatches, continue {float((ref['cont'] == 1).mean()):.2f}")
    assert not bad.any(), explain(cases, got, ref, bad)
    fb = got[-len(parts[-1]):]
    assert np.array_equal(fb["d"], parts[-1]["normal"]), "near_zero(direction): the normal"
    assert (ref["cont"] == 0).any() and (ref["L"] != 0).any()


def test_scene_flags(rtx_mod, orc, gpu, scene_dir):
    rtx = rtx_mod
    for scene, (cases, lamb) in (("lamb_notex", ssc.lamb_notex_cases()), ("mixed_notex", ssc.mixed_notex_cases())):
        assert len(variants_of(scene)) == {"lamb_notex": 9, "mixed_notex": 5}[scene]
        got, hist = check(rtx, orc, scene_dir, scene, scene, cases, lamb)
        assert sum(hist.values()) > 50 and (got["cont"] == 0).any()
    one = ssc.new_cases(4, 0, 0)  # hits of material 0, which every table has
    for scene, legal in (("table", ssc.CORE_FORMS["table"]), ("mixed_notex", ssc.CORE_FORMS["mixed_notex"])):
        dev, _ = scenes(rtx, orc, scene_dir, scene)
        for form in ssc.CORE_FORMS["lamb_notex"]:
            for v in (form, form + "_noorigin"):
                if form in legal:
                    rtx.shade_steps(dev, one, v)
                else:
                    with pytest.raises(rtx.RtxError, match="not all Lambertian|reads textures"):
                        rtx.shade_steps(dev, one, v)
    dev, _ = scenes(rtx, orc, scene_dir, "mixed_notex")
    for field, value in (("mat", 4), ("mat", -1), ("lazy_uv", 1), ("lazy_uv", -2)):
        c = ssc.new_cases(3, 0, 0)
        c[field][1] = value
        with pytest.raises(rtx.RtxError, match="out of range"):
            rtx.shade_steps(dev, c, "shade")


@pytest.mark.parametrize("precision", ("parity", "fast"))
@pytest.mark.parametrize("name,preset,width", [("three", "c1_three", 32), ("cornell", "cornell", 24)])
def test_the_hook_is_what_the_kernels_run(rtx_mod, gpu, name, preset, width, precision):
    """The hook chained over the device's own primary rays and closest hits at max_depth = 1 is
    the radiance query (k_radiance: the wavefront shade()) bit for bit."""
    rtx, seed = rtx_mod, 4242
    dev = rtx.DeviceScene(rtx.HostScene.load(scene_path(name)))
    cam = rtx.camera(rtx.camera_config(preset, width=width))
    R = rtx.camera_rays(dev, cam, 1, seed=seed)[:, 0]
    ids = np.arange(len(R), dtype=np.uint32)

    def cases_of(rays, pixel, depth, thr):
        h = dev.intersect(rays, precision=precision)
        c = ssc.orc.shade_cases(len(rays))
        for k, hk in (("hit", "hit"), ("p", "p"), ("normal", "normal"), ("u", "u"), ("v", "v"),
                      ("front_face", "front_face"), ("mat", "material")):
            c[k] = h[hk]
        c["o"], c["d"], c["thr"] = rays[:, :3], rays[:, 3:], thr
        c["seed"], c["pixel"], c["sample"], c["depth"], c["max_depth"] = seed, pixel, 0, depth, 1
        return c

    r0 = rtx.shade_steps(dev, cases_of(R, ids, 0, 1.0), "shade")
    go = r0["cont"] == 1
    r1 = rtx.shade_steps(dev, cases_of(np.concatenate([r0["o"][go], r0["d"][go]], 1), ids[go], 1, r0["thr"][go]), "shade")
    assert go.any() and (r1["cont"] == 0).all()
    L = r0["L"].copy()
    L[go] = r1["L"]
    rgb, segs = dev.radiance(R, 1, 1, seed=seed, ids=ids, precision=precision, segments=True)
    assert np.array_equal(L.view(np.uint64), rgb.view(np.uint64))
    assert np.array_equal(1 + go, segs)
    assert len(np.unique(rgb, axis=0)) > len(rgb) // 8


def test_power(rtx_mod, orc, gpu, scene_dir):
    """orc_set_perturb 1, 2 and 3 (the Lambertian BRDF scaled, the sky brightened, the eta^2 of a
    refraction dropped) must show as mismatches in the Lambertian, the sky and the refracting
    dielectric cases respectively and nowhere else.  The sky cases are every family's rows that end
    on the sky (the emitter family's light at the depth limit among them)."""
    dev, osc = scenes(rtx_mod, orc, scene_dir, "table")
    fams = {k: ssc.family(k) for k in ssc.FAMILIES}
    got = {k: device_records(rtx_mod, dev, k, f["cases"], variants_of("table")) for k, f in fams.items()}
    refracts = ssc.dielectric_outcomes(fams["dielectric"]["cases"], got["dielectric"]) == "refract"
    for perturb, target in ((1, "lambertian"), (2, "sky"), (3, "dielectric")):
        found = {}
        old = orc.set_perturb(perturb)
        try:
            assert old == 0
            for k, f in fams.items():
                bad, _ = ssc.mismatches(got[k], ssc.oracle_nudged(osc, f["cases"]), f["lamb"])
                end = ssc.sky_end(f["cases"])
                found["sky"] = found.get("sky", 0) + int((bad & end).sum())
                if k != "sky":
                    found[k] = int((bad & ~end).sum())
                if perturb == 3 and k == "dielectric":
                    assert not (bad & ~refracts).any()
                    assert bad[refracts & (f["cases"]["mat"] != ssc.GLASS[1])].all(), "every refraction with eta != 1"
        finally:
            orc.set_perturb(0)
        print("perturb", perturb, found)
        assert found[target] > 0 and all(n == 0 for k, n in found.items() if k != target), (perturb, found)
