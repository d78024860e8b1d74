"""Sampled films (rtx_film_create_sampled, csrc/rtx_film_sampled.h): the frames of
the light-sampling estimators kept as films, fixed spp or adaptive.

Pinned from outside.  A fixed film resolves to render_nee / render_mis at its budget bit for bit.
An adaptive film's saved state equals an independent replay: every sample's value and segment
count comes from the public query (radiance_mis / radiance_nee of the camera's own ray with spp = 1,
whose scale is exactly 1), and k_accumulate's recurrence is replayed in numpy float64 (division
and square roots as written, no contraction).  Group sizes, chunk caps, call splits, tiles and
stripes change nothing.  Without emitters, or at max_depth 1, the film is the plain wavefront film
byte for byte except the blob's sampler field.

All on the Cornell box at the 36-wide preset (36 x 24), depth 6, budgets <= 32.  ADAPT holds the
adaptive parameters, chosen on the replay so that the three classes of pixels (converged at
min_spp, converged later, unconverged at the budget) are all present."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import PKG, scene_path

pytestmark = pytest.mark.gpu
SEED = 4242
DEPTH = 6
PRECISIONS = ("parity", "fast")
ESTIMATORS = ("nee", "mis")
HEADER = "<8sII2ii4i3iQ4id2iq"  # FilmHeader, csrc/rtx_film.h
SAMPLER_AT = 76                 # the header's sampler field
ADAPT = dict(min_spp=4, rel_threshold=0.1)
BUDGET = 32
W, H = 36, 24
LUM = (0.2126, 0.7152, 0.0722)
FLOOR = 0.01
_cache = {}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def scene(rtx, name):
    if name not in _cache:
        host = rtx.HostScene.load(scene_path(name))
        _cache[name] = (rtx.DeviceScene(host), host)
    return _cache[name]


def camera(rtx):
    cam = rtx.camera(rtx.camera_config("cornell", width=W))
    assert (cam.image_width, cam.image_height) == (W, H)
    return cam


def tile_ids(x0, y0, w, h):
    return np.array([(y0 + r) * W + x0 + c for r in range(h) for c in range(w)])


def stripe_ids(rows, index, count):
    return np.array([y * W + x for y in range(H) if (y // rows) % count == index for x in range(W)])


def frame(dev, est, cam, spp, **kw):
    return (dev.render_mis if est == "mis" else dev.render_nee)(cam, spp, DEPTH, seed=SEED, **kw)


def table(rtx, est, precision, name="cornell", depth=DEPTH, seed=SEED, budget=BUDGET):
    """(X (npix, budget, 3), S (npix, budget)): every sample's value and segment count of the whole
    frame from the public query, sample k of pixel i from the camera's own ray of (i, k), keyed by
    the global pixel index.  Made once per key and left unchanged."""
    key = ("table", est, precision, name, depth, seed, budget)
    if key not in _cache:
        dev, _ = scene(rtx, name)
        cam = camera(rtx)
        query = dev.radiance_mis if est == "mis" else dev.radiance_nee
        ids = np.arange(W * H, dtype=np.uint32)
        X = np.zeros((W * H, budget, 3))
        S = np.zeros((W * H, budget), np.uint64)
        for k in range(budget):
            rays = rtx.camera_rays(dev, cam, 1, seed=seed, first_sample=k)[:, 0]
            X[:, k], S[:, k] = query(rays, 1, depth, seed=seed, ids=ids, first_sample=k, precision=precision,
                                     segments=True)
        X.setflags(write=False), S.setflags(write=False)
        _cache[key] = (X, S)
    return _cache[key]


def replay(X, S, min_spp, rel, budget, done=None):
    """k_accumulate's recurrence over each pixel's sample stream, in numpy float64: RecordSample,
    then IsConverged once the pixel holds min_spp samples; a pixel stops at its first converged
    sample or at the budget.  min_spp None: a fixed film (a plain sum, no test)."""
    n = len(X)
    sum_, mean, m2 = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
    cnt, conv, rec = np.zeros(n, np.int32), np.zeros(n, bool), np.zeros(n, np.uint64)
    for k in range(budget):
        act = ~conv
        a3 = act[:, None]
        x = X[:, k]
        nn = k + 1
        delta = x - mean
        mu = mean + delta / nn
        delta2 = x - mu
        mean = np.where(a3, mu, mean)
        m2 = np.where(a3, m2 + delta2 * delta, m2)
        sum_ = np.where(a3, sum_ + x, sum_)
        cnt[act] = nn
        rec[act] += S[act, k]
        if min_spp is not None and nn >= min_spp:
            var = m2 / (nn - 1) if nn > 1 else np.zeros_like(m2)
            mabs = np.maximum(np.abs(mean), 1e-3)
            err = np.sqrt(var) / np.sqrt(float(nn))
            ok = ~((err / mabs > rel).any(axis=1))
            conv = conv | (act & ok)
    return dict(sum=sum_, mean=mean, m2=m2, samples=cnt, conv=conv.astype(np.uint8), recorded=rec)


def state(blob, adaptive):
    """A saved film taken apart: the header's fields and the state arrays, pixel major."""
    h = struct.unpack(HEADER, blob[:104])
    npix = h[-1]
    body = np.frombuffer(blob, np.uint8)[104:]
    nf = 9 if adaptive else 3
    f = body[:nf * npix * 8].view(np.float64)
    out = dict(sampler=h[17], adaptive=h[15], done=h[19], npix=npix, sum=f[:3 * npix].reshape(3, npix).T)
    if adaptive:
        out["mean"], out["m2"] = f[3 * npix:6 * npix].reshape(3, npix).T, f[6 * npix:].reshape(3, npix).T
    out["samples"] = body[nf * npix * 8:nf * npix * 8 + 4 * npix].view(np.int32)
    if adaptive:
        out["conv"] = body[nf * npix * 8 + 4 * npix:]
        assert len(out["conv"]) == npix
    return out


def same_state(got, want, adaptive, ids=None):
    for k in ("sum", "mean", "m2") if adaptive else ("sum",):
        w = want[k] if ids is None else want[k][ids]
        assert np.array_equal(bits(got[k]), bits(w)), k
    for k in ("samples", "conv") if adaptive else ("samples",):
        w = want[k] if ids is None else want[k][ids]
        assert np.array_equal(got[k], w), k


def adaptive_film(dev, cam, est, precision="parity", **kw):
    return dev.film(cam, DEPTH, seed=SEED, adaptive=True, precision=precision, estimator=est, **dict(ADAPT, **kw))


# ---- fixed films --------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("est", ESTIMATORS)
def test_fixed_film_is_the_frame_at_its_budget(rtx_mod, gpu, est, precision):
    rtx = rtx_mod
    dev, _ = scene(rtx, "cornell")
    cam = camera(rtx)
    want = {b: frame(dev, est, cam, b, precision=precision) for b in (1, 3, 8)}
    for b in (1, 3, 8):  # in one call
        film = dev.film(cam, DEPTH, seed=SEED, adaptive=False, precision=precision, estimator=est)
        st = film.render(b)
        rgb, spp = film.resolve()
        assert np.array_equal(bits(rgb), bits(want[b][0])) and (spp == b).all() and film.samples == b
        total = int(want[b][1].sum(dtype=np.uint64))
        assert st["rays_total"] == total == st["rays_recorded"]
        assert st["paths"] == st["rays_primary"] == W * H * b and st["hot_launches"] >= 1
        assert st["kernel_ms"] > 0 and st["hot_kernel_ms"] > 0
        assert film.p3() == rtx.encode_p3(dev, want[b][0], W, H)
        film.close()
    film = dev.film(cam, DEPTH, seed=SEED, adaptive=False, precision=precision, estimator=est)
    seen = 0
    for b in (1, 3, 8):  # split 1 + 2 + 5
        st = film.render(b)
        rgb, _ = film.resolve()
        assert np.array_equal(bits(rgb), bits(want[b][0]))
        seen += st["rays_total"]
        assert seen == int(want[b][1].sum(dtype=np.uint64))
    assert film.render(8)["paths"] == 0 and film.render(5)["hot_launches"] == 0  # budget <= done: nothing
    assert np.array_equal(bits(film.resolve()[0]), bits(want[8][0]))
    # chunk seams: whole pixels per chunk, and one pixel's samples in runs
    for cap in (64, 1000, 5):
        rtx.radiance_chunk(cap)
        try:
            other = dev.film(cam, DEPTH, seed=SEED, adaptive=False, precision=precision, estimator=est)
            other.render(8)
            assert other.save() == film.save(), cap
            other.close()
        finally:
            rtx.radiance_chunk(0)
    # a tile under one wave, and stripes, against the whole frame's pixels
    for kw, ids in ((dict(tile=(7, 5, 5, 3)), tile_ids(7, 5, 5, 3)), (dict(stripes=(2, 1, 3)), stripe_ids(2, 1, 3))):
        part = dev.film(cam, DEPTH, seed=SEED, adaptive=False, precision=precision, estimator=est, **kw)
        part.render(3)
        part.render(8)
        assert part.npix == len(ids)
        assert np.array_equal(bits(part.resolve()[0]), bits(want[8][0][ids]))
        part.close()
    film.close()


# ---- adaptive films against the replay ----------------------------------------------------------
def test_the_replay_has_all_three_classes(rtx_mod, gpu):
    """ADAPT and BUDGET are chosen so that the replay alone (not the film) puts pixels in each class."""
    X, S = table(rtx_mod, "mis", "parity")
    r = replay(X, S, ADAPT["min_spp"], ADAPT["rel_threshold"], BUDGET)
    at_min = int(((r["conv"] == 1) & (r["samples"] == ADAPT["min_spp"])).sum())
    later = int(((r["conv"] == 1) & (r["samples"] > ADAPT["min_spp"])).sum())
    never = int((r["conv"] == 0).sum())
    print("classes (converged at min_spp, later, unconverged at the budget):", at_min, later, never)
    assert at_min > 0 and later > 0 and never > 0
    assert at_min + later + never == W * H and (r["samples"][r["conv"] == 0] == BUDGET).all()


@pytest.mark.parametrize("est,precision", [("mis", "parity"), ("mis", "fast"), ("nee", "parity")])
def test_adaptive_film_equals_the_replay(rtx_mod, gpu, est, precision):
    rtx = rtx_mod
    dev, _ = scene(rtx, "cornell")
    cam = camera(rtx)
    X, S = table(rtx, est, precision)
    want = replay(X, S, ADAPT["min_spp"], ADAPT["rel_threshold"], BUDGET)
    film = adaptive_film(dev, cam, est, precision)
    st = film.render(BUDGET)
    got = state(film.save(), True)
    assert (got["sampler"], got["adaptive"], got["done"]) == ({"nee": 2, "mis": 3}[est], 1, BUDGET)
    same_state(got, want, True)
    rgb, spp = film.resolve()
    n = want["samples"]
    scale = 1.0 / n.astype(np.float32).astype(np.float64)
    assert np.array_equal(bits(rgb), bits(want["sum"] * scale[:, None])) and np.array_equal(spp, n)
    assert st["rays_recorded"] == int(want["recorded"].sum(dtype=np.uint64))
    assert st["rays_total"] >= st["rays_recorded"] and st["paths"] == st["rays_primary"] >= int(n.sum())
    # the first group is min_spp samples of every pixel, later ones 4 of the pixels still sampling:
    # at most 3 discarded samples per pixel
    assert st["paths"] <= int(n.sum()) + 3 * W * H
    film.close()


def test_groups_chunks_splits_and_subsets_change_nothing(rtx_mod, gpu):
    rtx = rtx_mod
    dev, _ = scene(rtx, "cornell")
    cam = camera(rtx)
    X, S = table(rtx, "mis", "parity")
    want = replay(X, S, ADAPT["min_spp"], ADAPT["rel_threshold"], BUDGET)
    base = adaptive_film(dev, cam, "mis")
    base.render(BUDGET)
    blob = base.save()
    same_state(state(blob, True), want, True)
    base.close()

    def run(budgets=(BUDGET,), **kw):
        f = adaptive_film(dev, cam, "mis", **kw)
        stats = [f.render(b) for b in budgets]
        out = f.save()
        f.close()
        return out, stats

    try:
        for first, later in ((1, 1), (3, 7), (ADAPT["min_spp"], 4)):
            rtx.film_group(first, later)
            assert run()[0] == blob, (first, later)
        rtx.film_group()
        for cap in (64, 1000):
            rtx.radiance_chunk(cap)
            assert run()[0] == blob, cap
        rtx.radiance_chunk(64)
        rtx.film_group(3, 7)
        assert run((2, 9, BUDGET))[0] == blob
    finally:
        rtx.film_group()
        rtx.radiance_chunk(0)
    # budgets split over calls, one below min_spp; between calls every unconverged pixel holds `done`
    f = adaptive_film(dev, cam, "mis")
    for b in (2, 7, 20, BUDGET):
        f.render(b)
        s = state(f.save(), True)
        same_state(s, replay(X, S, ADAPT["min_spp"], ADAPT["rel_threshold"], b), True)
        assert (s["samples"][s["conv"] == 0] == b).all() and s["done"] == b
    assert f.save() == blob
    f.close()
    # a tile and stripes: the whole frame's pixels
    for kw, ids in ((dict(tile=(7, 5, 5, 3)), tile_ids(7, 5, 5, 3)), (dict(stripes=(2, 1, 3)), stripe_ids(2, 1, 3))):
        out, _ = run((5, BUDGET), **kw)
        same_state(state(out, True), want, True, ids)


def test_thresholds_at_the_ends(rtx_mod, gpu):
    rtx = rtx_mod
    dev, _ = scene(rtx, "cornell")
    cam = camera(rtx)
    X, S = table(rtx, "mis", "parity")
    m = ADAPT["min_spp"]
    # so loose that every pixel converges at min_spp: later calls launch nothing and change nothing
    loose = adaptive_film(dev, cam, "mis", rel_threshold=1e30)
    st = loose.render(m + 3)
    s = state(loose.save(), True)
    assert (s["conv"] == 1).all() and (s["samples"] == m).all() and st["paths"] == W * H * m
    same_state(s, replay(X, S, m, 1e30, m + 3), True)
    for b in (m + 3, 20, BUDGET):
        st = loose.render(b)
        assert st["paths"] == st["hot_launches"] == st["rays_total"] == 0 and st["kernel_ms"] == 0
        t = state(loose.save(), True)
        same_state(t, s, True)
    assert loose.samples == BUDGET and (loose.resolve()[1] == m).all()
    loose.close()
    # a threshold of 0: only a pixel whose samples are all equal (m2 == 0: it looks into the lamp)
    # passes IsConverged; every other pixel runs to the budget and holds the fixed film's sum
    want = replay(X, S, m, 0.0, BUDGET)
    flat = want["conv"] == 1
    assert (want["m2"][flat] == 0).all() and (~flat).sum() > W * H // 2
    zero = adaptive_film(dev, cam, "mis", rel_threshold=0.0)
    zero.render(BUDGET)
    z = state(zero.save(), True)
    same_state(z, want, True)
    fixed = dev.film(cam, DEPTH, seed=SEED, adaptive=False, estimator="mis")
    fixed.render(BUDGET)
    fsum = state(fixed.save(), False)["sum"]
    assert np.array_equal(bits(z["sum"][~flat]), bits(fsum[~flat])) and (z["samples"][~flat] == BUDGET).all()
    # ... and a flat pixel's 32 equal samples sum to 32 / min_spp times its min_spp samples
    assert np.allclose(z["sum"][flat] * (BUDGET // m), fsum[flat], rtol=1e-12, atol=0)
    zero.close(), fixed.close()


def test_an_active_list_of_one_pixel(rtx_mod, gpu):
    """A 2 x 1 tile picked from the replay: one pixel converges at min_spp, its neighbour goes on."""
    rtx = rtx_mod
    dev, _ = scene(rtx, "cornell")
    cam = camera(rtx)
    X, S = table(rtx, "mis", "parity")
    m = ADAPT["min_spp"]
    want = replay(X, S, m, ADAPT["rel_threshold"], BUDGET)
    stop = (want["conv"] == 1) & (want["samples"] == m)
    pairs = [i for i in range(W * H - 1) if i % W != W - 1 and stop[i] != stop[i + 1]
             and want["samples"][i] + want["samples"][i + 1] > 2 * m + 4]
    assert pairs
    i = pairs[0]
    ids = np.array([i, i + 1])
    f = adaptive_film(dev, cam, "mis", tile=(i % W, i // W, 2, 1))
    st = f.render(BUDGET)
    same_state(state(f.save(), True), want, True, ids)
    assert st["rays_recorded"] == int(want["recorded"][ids].sum(dtype=np.uint64))
    # min_spp samples of both pixels, then groups of 4 of the one that goes on
    more = int(want["samples"][ids].max()) - m
    assert st["paths"] == 2 * m + 4 * ((more + 3) // 4) - max(0, m + 4 * ((more + 3) // 4) - BUDGET)
    f.close()


# ---- the degenerate case: the plain wavefront film ----------------------------------------------
@pytest.mark.parametrize("name,depth", [("three", DEPTH), ("cornell", 1), ("cornell", 0)])
def test_without_a_term_it_is_the_plain_film(rtx_mod, gpu, name, depth):
    rtx = rtx_mod
    dev, _ = scene(rtx, name)
    cam = camera(rtx)
    if name == "three":
        assert dev.emitters()[0] == 0
    for precision in PRECISIONS:
        for adaptive in (False, True):
            kw = dict(seed=SEED, adaptive=adaptive, precision=precision, min_spp=4, rel_threshold=0.05)
            plain = dev.film(cam, depth, mode="wavefront", **kw)
            plain.render(3), plain.render(12)
            want = plain.save()
            assert want[SAMPLER_AT:SAMPLER_AT + 4] == bytes(4)
            for est, sampler in (("nee", 2), ("mis", 3)):
                f = dev.film(cam, depth, estimator=est, **kw)
                f.render(3), f.render(12)
                got = f.save()
                assert got[SAMPLER_AT:SAMPLER_AT + 4] == struct.pack("<i", sampler)
                assert got[:SAMPLER_AT] == want[:SAMPLER_AT] and got[SAMPLER_AT + 4:] == want[SAMPLER_AT + 4:]
                assert f.p3() == plain.p3()
                f.close()
            plain.close()


# ---- save, load, reset --------------------------------------------------------------------------
@pytest.mark.parametrize("adaptive", [False, True])
def test_save_load_and_the_sampler_field(rtx_mod, gpu, adaptive):
    rtx = rtx_mod
    dev, _ = scene(rtx, "cornell")
    cam = camera(rtx)
    kw = dict(seed=SEED, adaptive=adaptive, **ADAPT)
    whole = dev.film(cam, DEPTH, estimator="mis", **kw)
    whole.render(12)
    a = dev.film(cam, DEPTH, estimator="mis", **kw)
    a.render(6)
    blob = a.save()
    rtx.film_blob_check(blob)
    assert len(blob) == rtx.lib().rtx_film_state_bytes(a.h)
    b = dev.film(cam, DEPTH, estimator="mis", **kw)
    b.load(blob)
    assert b.samples == 6 and b.save() == blob
    b.render(12)
    assert b.save() == whole.save()
    for other in (dev.film(cam, DEPTH, mode="wavefront", **kw), dev.film(cam, DEPTH, estimator="nee", **kw)):
        with pytest.raises(rtx.RtxError, match="sampler .* differs from the film's"):
            other.load(blob)
        assert other.samples == 0
        other.render(2)
        with pytest.raises(rtx.RtxError, match="sampler .* differs from the film's"):
            b.load(other.save())
        other.close()
    assert b.save() == whole.save()
    for f in (whole, a, b):
        f.close()


def test_live_scene_and_reset(rtx_mod, gpu, tmp_path):
    """The light is moved in place (tests/test_gpu_mis.py test_live_scene's edit): the films refuse
    until reset(), then equal films on a scene made from the new file."""
    rtx = rtx_mod
    cam = camera(rtx)
    text = open(scene_path("cornell")).read()
    old = "rect xz 3 7 3 7 9.9900000000000002 3\n"
    assert old in text
    path = tmp_path / "cornell_moved.rtxs"
    path.write_text(text.replace(old, "rect xz 1 7 2 8 9.5 3\n"))
    fresh = rtx.DeviceScene(rtx.HostScene.load(str(path)))
    host = rtx.HostScene.load(scene_path("cornell"))
    dev = rtx.DeviceScene(host)
    films = {a: dev.film(cam, DEPTH, seed=SEED, adaptive=a, estimator="mis", **ADAPT) for a in (False, True)}
    before = {}
    for a, f in films.items():
        f.render(6)
        before[a] = f.save()
    prims = host.arrays()["prims"]
    li = int(rtx.emitter_table(dev)[0][0])
    moved = prims[li:li + 1].copy()
    moved[0]["g"][:5] = [1.0, 7.0, 2.0, 8.0, 9.5]
    dev.update_prims(moved, first=li)
    assert dev.emitters() == (1, 36.0)
    for a, f in films.items():
        with pytest.raises(rtx.RtxError, match="scene changed since the film was created"):
            f.render(8)
        with pytest.raises(rtx.RtxError, match="scene changed since the film was created"):
            f.save()
        f.reset()
        assert f.samples == 0
        f.render(2), f.render(8)
        want = fresh.film(cam, DEPTH, seed=SEED, adaptive=a, estimator="mis", **ADAPT)
        want.render(8)
        assert f.save() == want.save() and f.save() != before[a]
        want.close()
    for f in films.values():
        f.close()


# ---- the denoiser -------------------------------------------------------------------------------
def blob_variance(blob, npix, albedo):
    """tests/test_denoise.py's variance of an adaptive film's estimate from its saved state."""
    s = state(blob, True)
    m2, n = s["m2"].T, s["samples"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        vc = np.where(n >= 2, (m2 / (n - 1)) / n, 0.0)
    v = ((LUM[0] * LUM[0]) * vc[0] + (LUM[1] * LUM[1]) * vc[1]) + (LUM[2] * LUM[2]) * vc[2]
    a = np.maximum(albedo.astype(np.float32), np.float32(FLOOR)).astype(np.float64)
    lum = (LUM[0] * a[:, 0] + LUM[1] * a[:, 1]) + LUM[2] * a[:, 2]
    return v / (lum * lum)


@pytest.mark.parametrize("adaptive", [False, True])
def test_denoise_is_denoise_of_the_films_frame(rtx_mod, gpu, adaptive):
    rtx = rtx_mod
    dev, _ = scene(rtx, "cornell")
    cam = camera(rtx)
    aov = dev.aov(cam)
    film = dev.film(cam, DEPTH, seed=SEED, adaptive=adaptive, estimator="mis", **ADAPT)
    film.render(16)
    rgb, _ = film.resolve()
    blob = film.save()
    v = blob_variance(blob, W * H, aov[0]) if adaptive else None
    if adaptive:
        assert v.max() > 0
    want = rtx.denoise(dev, rgb, *aov, W, H, variance=v)
    got = film.denoise()
    assert np.array_equal(bits(got), bits(want)) and not np.array_equal(got, rgb)
    assert film.denoise_p3() == rtx.encode_p3(dev, got, W, H)
    assert film.save() == blob
    film.close()


# ---- adaptive sampling pays ---------------------------------------------------------------------
def test_adaptive_is_not_worse_than_fixed_at_equal_samples(rtx_mod, gpu):
    """The adaptive MIS film at ADAPT / BUDGET and a fixed MIS film with the same total of recorded
    samples (rounded up to whole spp), against a 1024-spp render_mis of a 12 x 8 tile, over 4 seeds.
    Asserted: the adaptive film's mean RMS is at most the fixed film's plus the seed-to-seed spread
    (max - min over the seeds) of the fixed film's RMS.  Both figures are printed."""
    rtx = rtx_mod
    dev, _ = scene(rtx, "cornell")
    cam = camera(rtx)
    tile = (12, 8, 12, 8)
    a_rms, f_rms, spps = [], [], []
    for seed in (11, 22, 33, 44):
        ref, _ = dev.render_mis(cam, 1024, DEPTH, seed=seed + 1000, tile=tile)
        fa = dev.film(cam, DEPTH, seed=seed, adaptive=True, estimator="mis", tile=tile, **ADAPT)
        fa.render(BUDGET)
        rgb, spp = fa.resolve()
        k = int(-(-int(spp.sum()) // len(spp)))
        ff = dev.film(cam, DEPTH, seed=seed, adaptive=False, estimator="mis", tile=tile)
        ff.render(k)
        a_rms.append(float(np.sqrt(np.mean((rgb - ref) ** 2))))
        f_rms.append(float(np.sqrt(np.mean((ff.resolve()[0] - ref) ** 2))))
        spps.append(k)
        fa.close(), ff.close()
    spread = max(f_rms) - min(f_rms)
    print("adaptive RMS %.5f, fixed RMS %.5f at %s spp, seed-to-seed spread %.5f" %
          (np.mean(a_rms), np.mean(f_rms), spps, spread))
    assert np.mean(a_rms) <= np.mean(f_rms) + spread


# ---- the command line ---------------------------------------------------------------------------
def command_line(rtx, tmp_path):
    exe = os.path.join(PKG, "raytracer")
    cams = json.load(open(os.path.join(os.path.dirname(PKG), "configs", "cameras.json")))
    small = dict(cams["cornell"], imageWidth=30, samplesPerPixel=20, maxDepth=6)
    path = tmp_path / "cameras.json"
    path.write_text(json.dumps({"default": cams["default"], "small": small}))
    base = [exe, "small", "--scene", scene_path("cornell"), "--cameras", str(path), "--seed", str(SEED)]

    def run(*args):
        r = subprocess.run(base + list(args), capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr.decode()
        return r

    dev, _ = scene(rtx, "cornell")
    cam = rtx.camera(rtx.camera_config("small", cameras=str(path)))
    assert (cam.image_width, cam.image_height) == (30, 20)
    return base, run, dev, cam


def test_command_line_fixed_film(rtx_mod, gpu, tmp_path):
    rtx = rtx_mod
    base, run, dev, cam = command_line(rtx, tmp_path)
    # --mis alone, and --nee --spp 2 alone, are what they were
    plain = run("--mis", "--spp", "6")
    rgb, segs = dev.render_mis(cam, 6, 6, seed=SEED)
    assert plain.stdout == rtx.encode_p3(dev, rgb, 30, 20)
    assert ("mis: 6 spp, 1 emitters, %d segments\n" % int(segs.sum(dtype=np.uint64))).encode() in plain.stderr
    assert b"film" not in plain.stderr
    nee = run("--nee", "--spp", "2")
    n_rgb, n_segs = dev.render_nee(cam, 2, 6, seed=SEED)
    assert nee.stdout == rtx.encode_p3(dev, n_rgb, 30, 20)
    assert ("nee: 2 spp, 1 emitters, %d segments\n" % int(n_segs.sum(dtype=np.uint64))).encode() in nee.stderr
    # chunks and a checkpoint, then a resume to more samples: the plain run's bytes
    ck = str(tmp_path / "film.ck")
    first = run("--mis", "--spp", "4", "--chunks", "3", "--checkpoint", ck, "--preview", str(tmp_path / "pv"))
    assert first.stdout == rtx.encode_p3(dev, dev.render_mis(cam, 4, 6, seed=SEED)[0], 30, 20)
    assert sorted(p.name for p in tmp_path.glob("pv_*.ppm")) == ["pv_2.ppm", "pv_3.ppm", "pv_4.ppm"]
    assert (tmp_path / "pv_2.ppm").read_bytes() == rtx.encode_p3(dev, dev.render_mis(cam, 2, 6, seed=SEED)[0], 30, 20)
    rtx.film_blob_check(open(ck, "rb").read())
    resumed = run("--mis", "--spp", "6", "--resume", ck)
    assert resumed.stdout == plain.stdout
    total = int(segs.sum(dtype=np.uint64)) - int(dev.render_mis(cam, 4, 6, seed=SEED)[1].sum(dtype=np.uint64))
    assert ("mis film: 6 spp, 1 emitters, %d segments traced, %d recorded\n" % (total, total)).encode() in resumed.stderr
    bad = subprocess.run(base + ["--nee", "--spp", "6", "--resume", ck], capture_output=True, timeout=120)
    assert bad.returncode == 1 and b"sampler" in bad.stderr and bad.stdout == b""


def test_command_line_adaptive_film(rtx_mod, gpu, tmp_path):
    """--adaptive: the Python adaptive film's P3 (min_spp 16, threshold 0.05f) and the log line."""
    rtx = rtx_mod
    base, run, dev, cam = command_line(rtx, tmp_path)
    film = dev.film(cam, 6, seed=SEED, adaptive=True, estimator="mis")
    st = film.render(20)
    ad = run("--mis", "--adaptive")
    assert ad.stdout == film.p3()
    line = "mis film: 20 spp, 1 emitters, %d segments traced, %d recorded\n" % (st["rays_total"], st["rays_recorded"])
    assert line.encode() in ad.stderr, ad.stderr.decode()
    film.close()
    alone = subprocess.run(base + ["--adaptive"], capture_output=True, timeout=120)
    assert alone.returncode == 2 and alone.stdout == b"" and b"--adaptive needs" in alone.stderr
