"""Occlusion queries and the AO pass: exports, argument checks and struct layout (no GPU).

Every check below is made before the library touches the scene or a device, so the calls run
without a GPU; where a non-NULL scene is needed to reach a later check, the handle is a dummy that
must never be dereferenced (the call returns RTX_ERR_INVALID first)."""
import ctypes as C
import re
import subprocess

import pytest

NEW = ["rtx_occluded", "rtx_occluded_device", "rtx_ao", "rtx_ao_device"]
INVALID = -1


def test_new_names_are_declared_and_exported(rtx_mod):
    L = C.CDLL(rtx_mod.LIB_PATH)
    nm = subprocess.run(["nm", "-D", "--defined-only", rtx_mod.LIB_PATH], capture_output=True, text=True).stdout
    for name in NEW + ["rtx_internal_ao_rays"]:
        assert hasattr(L, name), name
        assert re.search(rf"\bT {name}\b", nm), name
    for name in NEW:
        assert name in rtx_mod.EXPORTS, name
    assert "rtx_internal_ao_rays" not in rtx_mod.EXPORTS  # a test hook, not part of rtx.h


def test_ao_params_layout(rtx_mod):
    assert C.sizeof(rtx_mod.AoParams) == 24
    assert (rtx_mod.AoParams.samples.offset, rtx_mod.AoParams.radius.offset, rtx_mod.AoParams.seed.offset) == (0, 8, 16)


def invalid(rtx, rc, word):
    msg = rtx.lib().rtx_last_error().decode()
    assert rc == INVALID and word in msg, (rc, msg)


def test_occluded_argument_checks(rtx_mod):
    rtx, lib = rtx_mod, rtx_mod.lib()
    rays = (rtx.Ray * 2)()
    out = (C.c_uint8 * 2)()
    dummy = C.cast(C.create_string_buffer(64), C.c_void_p)  # never dereferenced: the checks below come first
    tmin = rtx.RTX_SEAM_TMIN
    invalid(rtx, lib.rtx_occluded(None, rays, 2, out, tmin, 1.0, 0), "scene is NULL")
    invalid(rtx, lib.rtx_occluded_device(None, rays, 2, out, tmin, 1.0, 0, None), "scene is NULL")
    for fn, tail in ((lib.rtx_occluded, ()), (lib.rtx_occluded_device, (None,))):
        invalid(rtx, fn(dummy, None, 2, out, tmin, 1.0, 0, *tail), "NULL buffer")
        invalid(rtx, fn(dummy, rays, 2, None, tmin, 1.0, 0, *tail), "NULL buffer")
        invalid(rtx, fn(dummy, rays, 2, out, 1.0, 1.0, 0, *tail), "tmin")
        invalid(rtx, fn(dummy, rays, 2, out, 2.0, 1.0, 0, *tail), "tmin")
        invalid(rtx, fn(dummy, rays, 2, out, float("nan"), 1.0, 0, *tail), "tmin")
        invalid(rtx, fn(dummy, rays, 0, out, 1.0, 1.0, 0, *tail), "tmin")  # the interval is checked even for n == 0


def test_ao_argument_checks(rtx_mod):
    rtx, lib = rtx_mod, rtx_mod.lib()
    cam = rtx.camera(rtx.camera_config("c1_three", width=16))
    prm = rtx.RenderParams()
    out = (C.c_double * (cam.image_width * cam.image_height))()
    dummy = C.cast(C.create_string_buffer(64), C.c_void_p)  # never dereferenced: the checks below come first

    def ao(samples, radius):
        a = rtx.AoParams()
        a.samples, a.radius, a.seed = samples, radius, 1
        return a

    hook = lib.rtx_internal_ao_rays
    hook.argtypes = [C.c_void_p, C.POINTER(rtx.Camera), C.POINTER(rtx.RenderParams), C.POINTER(rtx.AoParams), C.c_void_p]
    hook.restype = C.c_int
    calls = (lambda s, c, p, a, o: lib.rtx_ao(s, c, p, a, o), lambda s, c, p, a, o: lib.rtx_ao_device(s, c, p, a, o, None),
             lambda s, c, p, a, o: hook(s, c, p, a, o))
    good = ao(16, 1.0)
    for call in calls:
        invalid(rtx, call(None, C.byref(cam), C.byref(prm), C.byref(good), out), "scene is NULL")
        invalid(rtx, call(dummy, None, C.byref(prm), C.byref(good), out), "NULL argument")
        invalid(rtx, call(dummy, C.byref(cam), None, C.byref(good), out), "NULL argument")
        invalid(rtx, call(dummy, C.byref(cam), C.byref(prm), None, out), "NULL argument")
        invalid(rtx, call(dummy, C.byref(cam), C.byref(prm), C.byref(good), None), "NULL buffer")
        for samples in (0, 1025, -3):
            invalid(rtx, call(dummy, C.byref(cam), C.byref(prm), C.byref(ao(samples, 1.0)), out), "samples")
        for radius in (0.0, -1.0, float("nan")):
            invalid(rtx, call(dummy, C.byref(cam), C.byref(prm), C.byref(ao(16, radius)), out), "radius")
        bad = rtx.RenderParams()
        bad.x0, bad.w, bad.h = 10, 10, 2  # a tile outside the 16-pixel-wide image
        invalid(rtx, call(dummy, C.byref(cam), C.byref(bad), C.byref(good), out), "tile outside")
