"""Radiance queries: exports, struct layout and argument checks (no GPU).

Every check below is made before the library touches the scene or a device, so the calls run
without a GPU; where a non-NULL scene is needed to reach a later check, the handle is a dummy that
must never be dereferenced (the call returns RTX_ERR_INVALID first)."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

NEW = ["rtx_radiance", "rtx_radiance_device"]
HOOKS = ["rtx_internal_radiance_chunk", "rtx_internal_camera_rays"]
INVALID = -1
I32_MAX = 2 ** 31 - 1


def declared():
    """The functions include/rtx.h declares (comments stripped)."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtx.h")).read(), flags=re.S)
    return set(re.findall(r"\b(rtx_[a-z_0-9]+)\s*\(", text))


def test_new_names_are_declared_and_exported(rtx_mod):
    L = C.CDLL(rtx_mod.LIB_PATH)
    nm = subprocess.run(["nm", "-D", "--defined-only", rtx_mod.LIB_PATH], capture_output=True, text=True).stdout
    for name in NEW + HOOKS:
        assert hasattr(L, name), name
        assert re.search(rf"\bT {name}\b", nm), name
    for name in NEW:
        assert name in declared(), name
        assert name in rtx_mod.EXPORTS, name
    for name in HOOKS:  # test hooks, not part of rtx.h
        assert name not in declared(), name
        assert name not in rtx_mod.EXPORTS, name


def test_radiance_params_layout(rtx_mod):
    P = rtx_mod.RadianceParams
    assert C.sizeof(P) == 24
    assert (P.spp.offset, P.max_depth.offset, P.first_sample.offset, P.precision.offset, P.seed.offset) == (0, 4, 8, 12, 16)


def invalid(rtx, rc, word):
    msg = rtx.lib().rtx_last_error().decode()
    assert rc == INVALID and word in msg, (rc, msg)


def params(rtx, spp=4, max_depth=10, first_sample=0, precision=0):
    p = rtx.RadianceParams()
    p.spp, p.max_depth, p.first_sample, p.precision, p.seed = spp, max_depth, first_sample, precision, 1
    return p


def test_radiance_argument_checks(rtx_mod):
    rtx, lib = rtx_mod, rtx_mod.lib()
    rays = (rtx.Ray * 2)()
    ids = (C.c_uint32 * 2)()
    out = (C.c_double * 6)()
    segs = (C.c_uint32 * 2)()
    dummy = C.cast(C.create_string_buffer(64), C.c_void_p)  # never dereferenced: the checks below come first
    good = params(rtx)
    for fn, tail in ((lib.rtx_radiance, ()), (lib.rtx_radiance_device, (None,))):
        for n in (2, 0):  # the arguments are checked even for n == 0

            def call(scene=dummy, r=rays, p=good, o=out):
                return fn(scene, r, ids, n, None if p is None else C.byref(p), o, segs, *tail)

            invalid(rtx, call(scene=None), "scene is NULL")
            invalid(rtx, call(p=None), "NULL argument")
            invalid(rtx, call(r=None), "NULL buffer")
            invalid(rtx, call(o=None), "NULL buffer")
            for spp in (0, -1):
                invalid(rtx, call(p=params(rtx, spp=spp)), "spp")
            invalid(rtx, call(p=params(rtx, first_sample=-1)), "first_sample")
            invalid(rtx, call(p=params(rtx, spp=2, first_sample=I32_MAX - 1)), "first_sample")
            invalid(rtx, call(p=params(rtx, spp=I32_MAX, first_sample=1)), "first_sample")
            invalid(rtx, call(p=params(rtx, max_depth=-1)), "max_depth")
            for precision in (-1, 2):
                invalid(rtx, call(p=params(rtx, precision=precision)), "precision")
            # the documented order: each earlier failure wins over every later one
            worst = params(rtx, spp=0, first_sample=-1, max_depth=-1, precision=7)
            invalid(rtx, call(scene=None, p=None, r=None), "scene is NULL")
            invalid(rtx, call(p=None, r=None), "NULL argument")
            invalid(rtx, call(r=None, p=worst), "NULL buffer")
            invalid(rtx, call(p=worst), "radiance: spp")
            worst.spp = 1
            invalid(rtx, call(p=worst), "radiance: first_sample")
            worst.first_sample = 0
            invalid(rtx, call(p=worst), "max_depth")
            worst.max_depth = 0
            invalid(rtx, call(p=worst), "precision")
        # optional buffers may be NULL: with everything else in order and n == 0 the call is a no-op
        assert fn(dummy, rays, None, 0, C.byref(good), out, None, *tail) == 0
        assert fn(dummy, rays, ids, 0, C.byref(params(rtx, spp=1, first_sample=I32_MAX - 1, precision=1)), out, segs,
                  *tail) == 0


def test_radiance_chunk_hook_arguments(rtx_mod):
    f = rtx_mod.lib().rtx_internal_radiance_chunk
    f.argtypes, f.restype = [C.c_int64], C.c_int
    invalid(rtx_mod, f(-1), "radiance chunk")
    assert f(7) == 0 and f(0) == 0
    rtx_mod.radiance_chunk(5)
    rtx_mod.radiance_chunk()


def test_camera_rays_argument_checks(rtx_mod):
    rtx, lib = rtx_mod, rtx_mod.lib()
    cam = rtx.camera(rtx.camera_config("c1_three", width=16))
    prm = rtx.RenderParams()
    out = (C.c_double * (cam.image_width * cam.image_height * 2 * 6))()
    dummy = C.cast(C.create_string_buffer(64), C.c_void_p)  # never dereferenced: the checks below come first
    hook = lib.rtx_internal_camera_rays
    hook.argtypes = [C.c_void_p, C.POINTER(rtx.Camera), C.POINTER(rtx.RenderParams), C.c_int32, C.c_int32, C.c_void_p]
    hook.restype = C.c_int
    invalid(rtx, hook(None, C.byref(cam), C.byref(prm), 0, 2, out), "scene is NULL")
    invalid(rtx, hook(dummy, None, C.byref(prm), 0, 2, out), "NULL argument")
    invalid(rtx, hook(dummy, C.byref(cam), None, 0, 2, out), "NULL argument")
    invalid(rtx, hook(dummy, C.byref(cam), C.byref(prm), 0, 2, None), "NULL buffer")
    for spp in (0, -2):
        invalid(rtx, hook(dummy, C.byref(cam), C.byref(prm), 0, spp, out), "spp")
    invalid(rtx, hook(dummy, C.byref(cam), C.byref(prm), -1, 2, out), "first_sample")
    invalid(rtx, hook(dummy, C.byref(cam), C.byref(prm), I32_MAX - 1, 2, out), "first_sample")
    bad = rtx.RenderParams()
    bad.x0, bad.w, bad.h = 10, 10, 2  # a tile outside the 16-pixel-wide image
    invalid(rtx, hook(dummy, C.byref(cam), C.byref(bad), 0, 2, out), "tile outside")
    blank = rtx.Camera()  # never initialised
    invalid(rtx, hook(dummy, C.byref(blank), C.byref(prm), 0, 2, out), "camera not initialised")
