"""Direct-lighting queries: exports and argument checks (no GPU).

Every check below is made before the library touches the scene or a device, so the calls run
without a GPU; where a non-NULL scene is needed to reach a later check, the handle is a dummy that
must never be dereferenced (the call returns RTX_ERR_INVALID first).  The checks, their order and
their messages are rtx_radiance's."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from conftest import ROOT

NEW = ["rtx_direct", "rtx_direct_device", "rtx_scene_emitters"]
HOOKS = ["rtx_internal_direct_samples", "rtx_internal_emitters"]
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
    assert callable(rtx_mod.direct_samples) and callable(rtx_mod.emitter_table)
    for method in ("direct", "direct_device", "emitters"):
        assert callable(getattr(rtx_mod.DeviceScene, method)), method
    # the shadow segment's end: the f32 nearest 0.9999, as the header's macro and the kernel have it
    assert rtx_mod.RTX_DIRECT_TMAX == float(np.float32(0.9999)) and rtx_mod.RTX_DIRECT_TMAX < 1.0
    header = open(os.path.join(ROOT, "include", "rtx.h")).read()
    assert re.search(r"#define RTX_DIRECT_TMAX \(\(double\)0\.9999f\)", header)


def test_abi_version_stays(rtx_mod):
    assert rtx_mod.lib().rtx_abi_version() == 9


def invalid(rtx, rc, word):
    msg = rtx.lib().rtx_last_error().decode()
    assert rc == INVALID and word in msg, (rc, msg)


def params(rtx, spp=4, max_depth=10, first_sample=0, precision=0):
    p = rtx.RadianceParams()
    p.spp, p.max_depth, p.first_sample, p.precision, p.seed = spp, max_depth, first_sample, precision, 1
    return p


def entries(rtx):
    """The two entry points and the sample hook, whose last buffer argument is its only output."""
    lib = rtx.lib()
    hook = lib.rtx_internal_direct_samples
    hook.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(rtx.RadianceParams), C.c_void_p]
    hook.restype = C.c_int
    return lib.rtx_direct, lib.rtx_direct_device, hook


def test_direct_argument_checks(rtx_mod):
    rtx = rtx_mod
    host, device, hook = entries(rtx)
    surfels = (rtx.Ray * 2)()
    ids = (C.c_uint32 * 2)()
    out = (C.c_double * (2 * 4 * 9))()  # (large enough for the hook's 9 doubles per sample)
    vis = (C.c_uint32 * 2)()
    dummy = C.cast(C.create_string_buffer(64), C.c_void_p)  # never dereferenced: the checks below come first
    good = params(rtx)

    def caller(fn, n):
        def call(scene=dummy, s=surfels, p=good, o=out):
            pp = None if p is None else C.byref(p)
            if fn is hook:
                return fn(scene, s, ids, n, pp, o)
            if fn is device:
                return fn(scene, s, ids, n, pp, o, vis, None)
            return fn(scene, s, ids, n, pp, o, vis)
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
            invalid(rtx, call(p=params(rtx, max_depth=-1)), "negative max_depth")  # checked, otherwise ignored
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
    out = (C.c_double * 9)()
    vis = (C.c_uint32 * 1)()
    dummy = C.cast(C.create_string_buffer(64), C.c_void_p)
    good = params(rtx)
    edge = params(rtx, spp=1, first_sample=I32_MAX - 1, precision=1)
    assert host(dummy, surfels, None, 0, C.byref(good), out, None) == 0
    assert host(dummy, surfels, ids, 0, C.byref(edge), out, vis) == 0
    assert device(dummy, surfels, None, 0, C.byref(good), out, None, None) == 0
    assert device(dummy, surfels, ids, 0, C.byref(edge), out, vis, None) == 0
    assert hook(dummy, surfels, None, 0, C.byref(good), out) == 0
    assert hook(dummy, surfels, ids, 0, C.byref(edge), out) == 0


def test_scene_emitters_argument_checks(rtx_mod):
    rtx = rtx_mod
    fn = rtx.lib().rtx_scene_emitters
    dummy = C.cast(C.create_string_buffer(64), C.c_void_p)
    n, a = C.c_int64(0), C.c_double(0.0)
    invalid(rtx, fn(None, C.byref(n), C.byref(a)), "scene is NULL")
    invalid(rtx, fn(None, None, None), "scene is NULL")
    invalid(rtx, fn(dummy, None, None), "NULL argument")
