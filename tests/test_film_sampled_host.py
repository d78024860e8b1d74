"""Sampled films (rtx_film_create_sampled): the export, the argument checks and the
blob's sampler field (no GPU).

Every check of rtx_film_create_sampled is made before the library touches the scene or a device, so
the calls run without a GPU; where a non-NULL scene is needed to reach a later check the handle is
a dummy that must never be dereferenced.  The blob check is host only."""
import ctypes as C
import os
import re
import struct
import subprocess

import pytest

from conftest import ROOT

NEW = "rtx_film_create_sampled"
HOOK = "rtx_internal_film_group"
INVALID = -1
I32_MAX = 2 ** 31 - 1
DEPTH_CAP = 0x00FFFFFF
NEE, MIS = 1, 2
HEADER = "<8sII2ii4i3iQ4id2iq"  # FilmHeader, csrc/rtx_film.h
assert struct.calcsize(HEADER) == 104


def declared():
    """The functions include/rtx.h declares (comments stripped)."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtx.h")).read(), flags=re.S)
    return set(re.findall(r"\b(rtx_[a-z_0-9]+)\s*\(", text))


def test_the_export_the_header_and_exports_agree(rtx_mod):
    L = C.CDLL(rtx_mod.LIB_PATH)
    nm = subprocess.run(["nm", "-D", "--defined-only", rtx_mod.LIB_PATH], capture_output=True, text=True).stdout
    for name in (NEW, HOOK):
        assert hasattr(L, name), name
        assert re.search(rf"\bT {name}\b", nm), name
    assert NEW in declared() and NEW in rtx_mod.EXPORTS
    assert HOOK not in declared() and HOOK not in rtx_mod.EXPORTS  # a test hook, not part of rtx.h
    assert declared() == set(rtx_mod.EXPORTS)
    assert len(set(rtx_mod.EXPORTS)) == len(rtx_mod.EXPORTS)
    assert rtx_mod.lib().rtx_abi_version() == 9
    text = open(os.path.join(ROOT, "include", "rtx.h")).read()
    assert re.search(r"RTX_ESTIMATOR_NEE\s*=\s*1\s*,\s*RTX_ESTIMATOR_MIS\s*=\s*2", text)
    assert (rtx_mod.RTX_ESTIMATOR_NEE, rtx_mod.RTX_ESTIMATOR_MIS) == (NEE, MIS)
    assert rtx_mod.ESTIMATORS == {None: 0, "nee": NEE, "mis": MIS}


def test_film_group_exists(rtx_mod):
    assert callable(rtx_mod.film_group)
    rtx_mod.film_group(3, 7)
    rtx_mod.film_group()  # the defaults again
    f = rtx_mod.lib().rtx_internal_film_group
    assert f(-1, 0) == INVALID and f(0, -1) == INVALID
    assert b"film group" in rtx_mod.lib().rtx_last_error()


def invalid(rtx, rc, word):
    msg = rtx.lib().rtx_last_error().decode()
    assert rc == INVALID and word in msg, (rc, msg)


def render_params(rtx, max_depth=10, adaptive=0, precision=0, **tile):
    p = rtx.RenderParams()
    p.spp, p.max_depth, p.adaptive, p.precision, p.seed = 0, max_depth, adaptive, precision, 1
    p.min_spp, p.rel_threshold = 4, 0.1
    for k, v in tile.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("estimator,prefix", [(NEE, "nee"), (MIS, "mis")])
def test_argument_checks_in_order(rtx_mod, estimator, prefix):
    rtx = rtx_mod
    fn = rtx.lib().rtx_film_create_sampled
    cam = rtx.camera(rtx.camera_config("cornell", width=12))
    dummy = C.cast(C.create_string_buffer(64), C.c_void_p)  # never dereferenced: the checks below come first
    good = render_params(rtx)

    def call(scene=dummy, c=cam, p=good, est=estimator, out=True):
        h = C.c_void_p(0x1234)
        rc = fn(scene, None if c is None else C.byref(c), None if p is None else C.byref(p), est,
                C.byref(h) if out else None)
        if out and scene is not None and c is not None and p is not None:
            assert h.value is None  # *out is cleared once the arguments are there
        return rc

    # 1. NULL arguments, rtx_film_create's message
    invalid(rtx, call(scene=None), "NULL argument")
    invalid(rtx, call(c=None), "NULL argument")
    invalid(rtx, call(p=None), "NULL argument")
    invalid(rtx, call(out=False), "NULL argument")
    # 2. the estimator
    for est in (0, 3, -1, 77):
        invalid(rtx, call(est=est), "bad estimator")
    # 3. negative max_depth; 4. its cap, with the family's prefix
    invalid(rtx, call(p=render_params(rtx, max_depth=-1)), "negative max_depth")
    for md in (DEPTH_CAP + 1, I32_MAX):
        invalid(rtx, call(p=render_params(rtx, max_depth=md)), prefix + ": max_depth above")
    # 5. precision
    for precision in (-1, 2):
        invalid(rtx, call(p=render_params(rtx, precision=precision)), "bad precision")
    # 6. the pixel subset
    invalid(rtx, call(p=render_params(rtx, x0=4, y0=0, w=cam.image_width, h=2)), "tile outside the image")
    invalid(rtx, call(p=render_params(rtx, stripe_rows=2, stripe_index=3, stripe_count=3)), "bad stripe_index")
    # the documented order: each earlier failure wins over every later one
    worst = render_params(rtx, max_depth=-1, precision=9, x0=-1, w=1, h=1)
    invalid(rtx, call(scene=None, c=None, p=None, est=9), "NULL argument")
    invalid(rtx, call(p=worst, est=9), "bad estimator")
    invalid(rtx, call(p=worst), "negative max_depth")
    worst.max_depth = DEPTH_CAP + 1
    invalid(rtx, call(p=worst), prefix + ": max_depth above")
    worst.max_depth = DEPTH_CAP
    invalid(rtx, call(p=worst), "bad precision")
    worst.precision = 1
    invalid(rtx, call(p=worst), "tile outside the image")
    # spp, mode, flags and samples_per_group are ignored: values rtx_film_create rejects reach the
    # last check; adaptive films are allowed (the one-shot frames refuse them)
    odd = render_params(rtx, adaptive=1, x0=-1, w=1, h=1)
    odd.spp, odd.mode, odd.flags, odd.samples_per_group = -3, 77, -1, -9
    invalid(rtx, call(p=odd), "tile outside the image")


def test_the_plain_film_keeps_its_checks(rtx_mod):
    rtx = rtx_mod
    cam = rtx.camera(rtx.camera_config("cornell", width=12))
    dummy = C.cast(C.create_string_buffer(64), C.c_void_p)
    h = C.c_void_p()
    p = render_params(rtx)
    p.mode = 77
    invalid(rtx, rtx.lib().rtx_film_create(dummy, C.byref(cam), C.byref(p), C.byref(h)), "bad mode")
    p.mode, p.adaptive = 2, 1
    invalid(rtx, rtx.lib().rtx_film_create(dummy, C.byref(cam), C.byref(p), C.byref(h)), "megakernel films")


def blob(sampler, adaptive, npix_w=3, npix_h=2, extra=0, done=5):
    """A hand-packed film blob of a 3 x 2 image: the header and a zero body of the exact length."""
    npix = npix_w * npix_h
    head = struct.pack(HEADER, b"RTXFILM\0", 1, 104, npix_w, npix_h, 0, 0, 0, npix_w, npix_h, 0, 0, 0, 99, 6, adaptive,
                       4, sampler, 0.1, done, 0, npix)
    body = npix * (9 * 8 + 4 + 1 if adaptive else 3 * 8 + 4)
    return head + bytes(body + extra)


def test_blob_check_accepts_the_new_samplers(rtx_mod):
    rtx = rtx_mod
    assert len(blob(0, 0)) == 104 + 6 * 28 and len(blob(0, 1)) == 104 + 6 * 77
    for sampler in (0, 2, 3):
        for adaptive in (0, 1):
            rtx.film_blob_check(blob(sampler, adaptive))
    rtx.film_blob_check(blob(1, 0))
    for bad, word in ((blob(4, 0), "bad sampler"), (blob(4, 1), "bad sampler"), (blob(-1, 0), "bad sampler"),
                      (blob(1, 1), "megakernel films are not adaptive"),
                      (blob(2, 1, extra=1), "length %d above the %d bytes of its state" % (104 + 6 * 77 + 1, 104 + 6 * 77)),
                      (blob(3, 0, extra=-1), "truncated: %d bytes, %d expected" % (104 + 6 * 28 - 1, 104 + 6 * 28)),
                      (blob(2, 0)[:50], "truncated: shorter than the header")):
        with pytest.raises(rtx.RtxError) as e:
            rtx.film_blob_check(bad)
        assert "film blob: " + word in str(e.value), str(e.value)
