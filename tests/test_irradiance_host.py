"""Irradiance queries: exports and argument checks (no GPU).

Every check below is made before the library touches the scene or a device, so the calls run
without a GPU; where a non-NULL scene is needed to reach a later check, the handle is a dummy that
must never be dereferenced (the call returns RTX_ERR_INVALID first).  The checks, their order and
their messages are rtx_radiance's."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

NEW = ["rtx_irradiance", "rtx_irradiance_device"]
HOOKS = ["rtx_internal_irradiance_rays"]
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
    for name in HOOKS:  # a test hook, not part of rtx.h
        assert name not in declared(), name
        assert name not in rtx_mod.EXPORTS, name
    assert callable(rtx_mod.irradiance_rays)
    assert callable(rtx_mod.DeviceScene.irradiance) and callable(rtx_mod.DeviceScene.irradiance_device)


def invalid(rtx, rc, word):
    msg = rtx.lib().rtx_last_error().decode()
    assert rc == INVALID and word in msg, (rc, msg)


def params(rtx, spp=4, max_depth=10, first_sample=0, precision=0):
    p = rtx.RadianceParams()
    p.spp, p.max_depth, p.first_sample, p.precision, p.seed = spp, max_depth, first_sample, precision, 1
    return p


def entries(rtx):
    """(function, trailing arguments after the output buffers) of the two entry points and the hook,
    whose last buffer argument is its only output."""
    lib = rtx.lib()
    hook = lib.rtx_internal_irradiance_rays
    hook.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(rtx.RadianceParams), C.c_void_p]
    hook.restype = C.c_int
    return lib.rtx_irradiance, lib.rtx_irradiance_device, hook


def test_irradiance_argument_checks(rtx_mod):
    rtx = rtx_mod
    host, device, hook = entries(rtx)
    surfels = (rtx.Ray * 2)()
    ids = (C.c_uint32 * 2)()
    out = (C.c_double * (2 * 4 * 6))()  # (large enough for the hook's 6 doubles per ray)
    segs = (C.c_uint32 * 2)()
    dummy = C.cast(C.create_string_buffer(64), C.c_void_p)  # never dereferenced: the checks below come first
    good = params(rtx)

    def caller(fn, n):
        def call(scene=dummy, s=surfels, p=good, o=out):
            pp = None if p is None else C.byref(p)
            if fn is hook:
                return fn(scene, s, ids, n, pp, o)
            if fn is device:
                return fn(scene, s, ids, n, pp, o, segs, None)
            return fn(scene, s, ids, n, pp, o, segs)
        return call

    for fn in (host, device, hook):
        for n in (2, 0):  # the arguments are checked even for n == 0
            call = caller(fn, n)
            invalid(rtx, call(scene=None), "scene is NULL")
            invalid(rtx, call(p=None), "NULL argument")
            invalid(rtx, call(s=None), "NULL buffer")
            invalid(rtx, call(o=None), "NULL buffer")
            for spp in (0, -1):
                invalid(rtx, call(p=params(rtx, spp=spp)), "spp must be at least 1")
            invalid(rtx, call(p=params(rtx, first_sample=-1)), "first_sample must be >= 0")
            invalid(rtx, call(p=params(rtx, spp=2, first_sample=I32_MAX - 1)), "fit int32")
            invalid(rtx, call(p=params(rtx, spp=I32_MAX, first_sample=1)), "fit int32")
            invalid(rtx, call(p=params(rtx, max_depth=-1)), "negative max_depth")
            for precision in (-1, 2):
                invalid(rtx, call(p=params(rtx, precision=precision)), "bad precision")
            # the documented order: each earlier failure wins over every later one
            worst = params(rtx, spp=0, first_sample=-1, max_depth=-1, precision=7)
            invalid(rtx, call(scene=None, p=None, s=None), "scene is NULL")
            invalid(rtx, call(p=None, s=None), "NULL argument")
            invalid(rtx, call(s=None, p=worst), "NULL buffer")
            invalid(rtx, call(p=worst), "radiance: spp")
            worst.spp = 1
            invalid(rtx, call(p=worst), "radiance: first_sample")
            worst.first_sample = 0
            invalid(rtx, call(p=worst), "max_depth")
            worst.max_depth = 0
            invalid(rtx, call(p=worst), "precision")


def test_no_surfels_is_ok(rtx_mod):
    """After the checks n == 0 returns RTX_OK before the (dummy) scene is touched; the optional
    buffers may be NULL."""
    rtx = rtx_mod
    host, device, hook = entries(rtx)
    surfels = (rtx.Ray * 1)()
    ids = (C.c_uint32 * 1)()
    out = (C.c_double * 6)()
    segs = (C.c_uint32 * 1)()
    dummy = C.cast(C.create_string_buffer(64), C.c_void_p)
    good = params(rtx)
    edge = params(rtx, spp=1, first_sample=I32_MAX - 1, precision=1)
    assert host(dummy, surfels, None, 0, C.byref(good), out, None) == 0
    assert host(dummy, surfels, ids, 0, C.byref(edge), out, segs) == 0
    assert device(dummy, surfels, None, 0, C.byref(good), out, None, None) == 0
    assert device(dummy, surfels, ids, 0, C.byref(edge), out, segs, None) == 0
    assert hook(dummy, surfels, None, 0, C.byref(good), out) == 0
    assert hook(dummy, surfels, ids, 0, C.byref(edge), out) == 0
