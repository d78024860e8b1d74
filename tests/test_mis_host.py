"""Multiple importance sampling: exports and argument checks (no GPU).

The four entry points check as the next-event-estimation family does (tests/test_nee_host.py), in
its order, with "mis" where its messages say "nee"; every check is made before the library touches
the scene or a device, so the calls run without a GPU, and where a non-NULL scene is needed to
reach a later check the handle is a dummy that must never be dereferenced."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

NEW = ["rtx_radiance_mis", "rtx_radiance_mis_device", "rtx_render_mis", "rtx_render_mis_device"]
HOOK = "rtx_internal_mis_trace"
INVALID = -1
I32_MAX = 2 ** 31 - 1
DEPTH_CAP = 0x00FFFFFF


def declared():
    """The functions include/rtx.h declares (comments stripped)."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtx.h")).read(), flags=re.S)
    return set(re.findall(r"\b(rtx_[a-z_0-9]+)\s*\(", text))


def test_new_names_are_declared_and_exported(rtx_mod):
    L = C.CDLL(rtx_mod.LIB_PATH)
    nm = subprocess.run(["nm", "-D", "--defined-only", rtx_mod.LIB_PATH], capture_output=True, text=True).stdout
    for name in NEW + [HOOK]:
        assert hasattr(L, name), name
        assert re.search(rf"\bT {name}\b", nm), name
    for name in NEW:
        assert name in declared(), name
        assert name in rtx_mod.EXPORTS, name
    assert HOOK not in declared() and HOOK not in rtx_mod.EXPORTS  # a test hook, not part of rtx.h
    assert callable(rtx_mod.mis_trace)
    for method in ("radiance_mis", "radiance_mis_device", "render_mis", "render_mis_device"):
        assert callable(getattr(rtx_mod.DeviceScene, method)), method
    assert rtx_mod.MIS_WEIGHTED == 16
    assert (rtx_mod.NEE_ELIGIBLE, rtx_mod.NEE_TRACED, rtx_mod.NEE_VISIBLE, rtx_mod.NEE_SUPPRESSED) == (1, 2, 4, 8)


def test_header_and_exports_agree_and_the_abi_version_stays(rtx_mod):
    assert declared() == set(rtx_mod.EXPORTS)
    assert len(set(rtx_mod.EXPORTS)) == len(rtx_mod.EXPORTS)
    assert rtx_mod.lib().rtx_abi_version() == 9


def invalid(rtx, rc, word):
    msg = rtx.lib().rtx_last_error().decode()
    assert rc == INVALID and word in msg, (rc, msg)


def params(rtx, spp=4, max_depth=10, first_sample=0, precision=0):
    p = rtx.RadianceParams()
    p.spp, p.max_depth, p.first_sample, p.precision, p.seed = spp, max_depth, first_sample, precision, 1
    return p


def entries(rtx):
    lib = rtx.lib()
    trace = getattr(lib, HOOK)
    trace.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(rtx.RadianceParams), C.c_int32,
                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    trace.restype = C.c_int
    return lib.rtx_radiance_mis, lib.rtx_radiance_mis_device, trace


def test_ray_entry_argument_checks(rtx_mod):
    rtx = rtx_mod
    host, device, trace = entries(rtx)
    rays = (rtx.Ray * 2)()
    ids = (C.c_uint32 * 2)()
    out = (C.c_double * (2 * 4 * 11 * 2))()  # (large enough for the hook's doubles at cap 2)
    segs = (C.c_uint32 * (2 * 4 * 2))()
    ends = (C.c_double * (2 * 4 * 3))()
    dummy = C.cast(C.create_string_buffer(64), C.c_void_p)  # never dereferenced: the checks below come first
    good = params(rtx)

    def caller(fn, n):
        def call(scene=dummy, s=rays, p=good, o=out):
            pp = None if p is None else C.byref(p)
            if fn is trace:
                return fn(scene, s, ids, n, pp, 2, o, segs, ends, segs)
            if fn is device:
                return fn(scene, s, ids, n, pp, o, segs, None)
            return fn(scene, s, ids, n, pp, o, segs)
        return call

    for fn in (host, device, trace):
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
            worst.max_depth = DEPTH_CAP + 1
            invalid(rtx, call(p=worst), "precision")  # radiance_check's last check comes before the cap
            # the cap: after rtx_radiance's checks, with a message of its own, before n == 0 returns
            for md in (DEPTH_CAP + 1, I32_MAX):
                invalid(rtx, call(p=params(rtx, max_depth=md)), "mis: max_depth above")
    # the hook's own arguments, after the shared checks
    for n in (2, 0):
        for cap in (0, -3, 4097):
            invalid(rtx, trace(dummy, rays, ids, n, C.byref(good), cap, out, segs, ends, segs), "mis trace: cap")
        invalid(rtx, trace(dummy, rays, ids, n, C.byref(good), 2, out, None, ends, segs), "NULL buffer")
        invalid(rtx, trace(dummy, rays, ids, n, C.byref(good), 2, out, segs, None, segs), "NULL buffer")
        invalid(rtx, trace(dummy, rays, ids, n, C.byref(good), 2, out, segs, ends, None), "NULL buffer")
        # ... whose order: the cap of max_depth, then the buffers, then the record cap
        deep = params(rtx, max_depth=DEPTH_CAP + 1)
        invalid(rtx, trace(dummy, rays, ids, n, C.byref(deep), 0, out, None, ends, segs), "mis: max_depth above")
        invalid(rtx, trace(dummy, rays, ids, n, C.byref(good), 0, out, None, ends, segs), "NULL buffer")


def test_no_rays_is_ok(rtx_mod):
    """After the checks n == 0 returns RTX_OK before the (dummy) scene is touched; the optional
    buffers may be NULL; max_depth at the cap passes."""
    rtx = rtx_mod
    host, device, trace = entries(rtx)
    rays = (rtx.Ray * 1)()
    ids = (C.c_uint32 * 1)()
    out = (C.c_double * 22)()
    segs = (C.c_uint32 * 2)()
    dummy = C.cast(C.create_string_buffer(64), C.c_void_p)
    good = params(rtx)
    edge = params(rtx, spp=1, first_sample=I32_MAX - 1, precision=1, max_depth=DEPTH_CAP)
    assert host(dummy, rays, None, 0, C.byref(good), out, None) == 0
    assert host(dummy, rays, ids, 0, C.byref(edge), out, segs) == 0
    assert device(dummy, rays, None, 0, C.byref(good), out, None, None) == 0
    assert device(dummy, rays, ids, 0, C.byref(edge), out, segs, None) == 0
    assert trace(dummy, rays, ids, 0, C.byref(edge), 1, out, segs, out, segs) == 0
    assert trace(dummy, rays, None, 0, C.byref(good), 4096, out, segs, out, segs) == 0


def render_params(rtx, spp=4, max_depth=10, adaptive=0, precision=0, **tile):
    p = rtx.RenderParams()
    p.spp, p.max_depth, p.adaptive, p.precision, p.seed = spp, max_depth, adaptive, precision, 1
    for k, v in tile.items():
        setattr(p, k, v)
    return p


def test_frame_entry_argument_checks(rtx_mod):
    rtx = rtx_mod
    lib = rtx.lib()
    cam = rtx.camera(rtx.camera_config("cornell", width=12))
    out = (C.c_double * (3 * cam.image_width * cam.image_height))()
    segs = (C.c_uint32 * (cam.image_width * cam.image_height))()
    dummy = C.cast(C.create_string_buffer(64), C.c_void_p)
    good = render_params(rtx)

    def caller(fn):
        def call(scene=dummy, c=cam, p=good, o=out):
            cc = None if c is None else C.byref(c)
            pp = None if p is None else C.byref(p)
            if fn is lib.rtx_render_mis_device:
                return fn(scene, cc, pp, o, segs, None)
            return fn(scene, cc, pp, o, segs)
        return call

    for fn in (lib.rtx_render_mis, lib.rtx_render_mis_device):
        call = caller(fn)
        invalid(rtx, call(scene=None), "scene is NULL")
        invalid(rtx, call(c=None), "NULL argument")
        invalid(rtx, call(p=None), "NULL argument")
        for spp in (0, -1):
            invalid(rtx, call(p=render_params(rtx, spp=spp)), "render mis: spp must be at least 1")
        invalid(rtx, call(p=render_params(rtx, max_depth=-1)), "negative max_depth")
        for md in (DEPTH_CAP + 1, I32_MAX):
            invalid(rtx, call(p=render_params(rtx, max_depth=md)), "mis: max_depth above")
        for adaptive in (1, -1, 2):
            invalid(rtx, call(p=render_params(rtx, adaptive=adaptive)), "render mis: adaptive")
        for precision in (-1, 2):
            invalid(rtx, call(p=render_params(rtx, precision=precision)), "render mis: bad precision")
        invalid(rtx, call(p=render_params(rtx, x0=4, y0=0, w=cam.image_width, h=2)), "tile outside the image")
        invalid(rtx, call(p=render_params(rtx, stripe_rows=2, stripe_index=3, stripe_count=3)), "bad stripe_index")
        invalid(rtx, call(o=None), "NULL buffer")
        # the documented order
        worst = render_params(rtx, spp=0, max_depth=-1, adaptive=1, precision=9, x0=-1, w=1, h=1)
        invalid(rtx, call(scene=None, c=None, p=None, o=None), "scene is NULL")
        invalid(rtx, call(c=None, p=worst, o=None), "NULL argument")
        invalid(rtx, call(p=worst, o=None), "render mis: spp")
        worst.spp = 1
        invalid(rtx, call(p=worst, o=None), "negative max_depth")
        worst.max_depth = DEPTH_CAP + 1
        invalid(rtx, call(p=worst, o=None), "mis: max_depth above")
        worst.max_depth = DEPTH_CAP
        invalid(rtx, call(p=worst, o=None), "render mis: adaptive")
        worst.adaptive = 0
        invalid(rtx, call(p=worst, o=None), "render mis: bad precision")
        worst.precision = 1
        invalid(rtx, call(p=worst, o=None), "tile outside the image")
        worst.x0 = 0
        invalid(rtx, call(p=worst, o=None), "NULL buffer")
        # mode and flags are ignored: values rtx_render rejects reach the next check
        odd = render_params(rtx)
        odd.mode, odd.flags, odd.min_spp = 77, -1, -5
        invalid(rtx, call(p=odd, o=None), "NULL buffer")
        # an empty subset (stripes past the image's rows) is RTX_OK before the buffers are looked at
        none = render_params(rtx, stripe_rows=cam.image_height, stripe_index=1, stripe_count=2)
        assert lib.rtx_render_pixel_count(C.byref(cam), C.byref(none)) == 0
        assert call(p=none, o=None) == 0


def test_the_nee_family_keeps_its_messages(rtx_mod):
    """The shared checks say "nee" for the family they were written for."""
    rtx = rtx_mod
    lib = rtx.lib()
    rays = (rtx.Ray * 1)()
    out = (C.c_double * 3)()
    dummy = C.cast(C.create_string_buffer(64), C.c_void_p)
    deep = params(rtx, max_depth=DEPTH_CAP + 1)
    invalid(rtx, lib.rtx_radiance_nee(dummy, rays, None, 1, C.byref(deep), out, None), "nee: max_depth above")
    cam = rtx.camera(rtx.camera_config("cornell", width=12))
    invalid(rtx, lib.rtx_render_nee(dummy, C.byref(cam), C.byref(render_params(rtx, adaptive=1)), out, None),
            "render nee: adaptive")
