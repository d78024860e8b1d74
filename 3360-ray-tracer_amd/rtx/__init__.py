"""rtx — thin ctypes binding of librtx.so (include/rtx.h) for tests, bench and scripting.

The product is the C ABI + HIP kernels in librtx.so; this module only marshals arguments.
There is no CPU fallback: if librtx.so is missing or no GPU is present, calls raise.
"""
import ctypes as C
import os

import numpy as np

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPO = os.path.dirname(PKG_DIR)
LIB_PATH = os.environ.get("RTX_LIB") or os.path.join(PKG_DIR, "librtx.so")  # RTX_LIB: A/B variant builds
ASSETS = os.path.join(PKG_DIR, "assets")
CAMERAS = os.path.join(REPO, "configs", "cameras.json")

RTX_OK = 0
RTX_SEAM_TMIN = float(np.float32(0.001))
RTX_DIRECT_TMAX = float(np.float32(0.9999))  # where a direct-lighting shadow segment ends (rtx.h)
MODES = {"wavefront": 0, "persistent": 1, "megakernel": 2}
PRECISIONS = {"parity": 0, "fast": 1}
RTX_FLAG_COUNT, RTX_FLAG_PARK, RTX_FLAG_NO_PARK, RTX_FLAG_GENERIC, RTX_FLAG_LEAF_STEP = 1, 2, 4, 8, 16
# adaptive persistent renders: one launch per phase (the default; ADAPT_PHASES names it)
RTX_FLAG_ADAPT_PHASES = 32
ADAPT_SCHEDULE_FLAGS = {None: 0, "phases": RTX_FLAG_ADAPT_PHASES}
# "park": the PARK schedule with its default walk (speculative on trees of at most 65536 nodes);
# "park_step": the PARK schedule with the leaf-step walk on every tree
SCHEDULE_FLAGS = {None: 0, "auto": 0, "park": RTX_FLAG_PARK, "park_step": RTX_FLAG_PARK | RTX_FLAG_LEAF_STEP,
                  "plain": RTX_FLAG_NO_PARK}
BUILD_BITS = {"park": 1, "sphere_tree": 2, "triangle_tree": 4, "lambertian": 8, "no_textures": 16,
              "no_defocus": 32, "fast": 64, "count": 128, "scatter": 256, "speculative": 512}


def build_names(bits):
    """rtx_stats.build bits -> names of the persistent-kernel specialisations that ran."""
    return [k for k, b in BUILD_BITS.items() if bits & b]


class RtxError(RuntimeError):
    pass


class BvhNode(C.Structure):
    _fields_ = [("lo", C.c_double * 3), ("hi", C.c_double * 3), ("left_first", C.c_uint32),
                ("right_count", C.c_uint32), ("is_leaf", C.c_uint32), ("pad_", C.c_uint32)]


class Prim(C.Structure):
    _fields_ = [("kind", C.c_int32), ("material", C.c_int32), ("g", C.c_double * 9)]


class Texture(C.Structure):
    _fields_ = [("kind", C.c_int32), ("even", C.c_int32), ("odd", C.c_int32), ("image", C.c_int32),
                ("color", C.c_double * 3), ("inv_scale", C.c_double)]


class Image(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("texels", C.c_void_p)]


class Material(C.Structure):
    _fields_ = [("kind", C.c_int32), ("texture", C.c_int32), ("albedo", C.c_double * 3), ("fuzz", C.c_double),
                ("ref_idx", C.c_double)]


class SceneDesc(C.Structure):
    _fields_ = [("prims", C.POINTER(Prim)), ("n_prims", C.c_int64), ("nodes", C.POINTER(BvhNode)),
                ("n_nodes", C.c_int64), ("materials", C.POINTER(Material)), ("n_materials", C.c_int32),
                ("textures", C.POINTER(Texture)), ("n_textures", C.c_int32), ("images", C.POINTER(Image)),
                ("n_images", C.c_int32)]


class Ray(C.Structure):
    _fields_ = [("origin", C.c_double * 3), ("direction", C.c_double * 3)]


class Hit(C.Structure):
    _fields_ = [("hit", C.c_int32), ("front_face", C.c_int32), ("material", C.c_int32), ("pad_", C.c_int32),
                ("t", C.c_double), ("p", C.c_double * 3), ("normal", C.c_double * 3), ("u", C.c_double),
                ("v", C.c_double)]


class CameraConfig(C.Structure):
    _fields_ = [("aspect_ratio", C.c_double), ("image_width", C.c_int32), ("samples_per_pixel", C.c_int32),
                ("max_depth", C.c_int32), ("pad_", C.c_int32), ("vfov", C.c_double), ("lookfrom", C.c_double * 3),
                ("lookat", C.c_double * 3), ("vup", C.c_double * 3), ("defocus_angle", C.c_double),
                ("focus_dist", C.c_double)]


class Camera(C.Structure):
    _fields_ = [("center", C.c_double * 3), ("pixel00", C.c_double * 3), ("pixel_delta_u", C.c_double * 3),
                ("pixel_delta_v", C.c_double * 3), ("u", C.c_double * 3), ("v", C.c_double * 3),
                ("w", C.c_double * 3), ("defocus_disk_u", C.c_double * 3), ("defocus_disk_v", C.c_double * 3),
                ("defocus_angle", C.c_double), ("image_width", C.c_int32), ("image_height", C.c_int32)]


class RenderParams(C.Structure):
    _fields_ = [("spp", C.c_int32), ("max_depth", C.c_int32), ("adaptive", C.c_int32), ("min_spp", C.c_int32),
                ("rel_threshold", C.c_double), ("seed", C.c_uint64), ("mode", C.c_int32), ("precision", C.c_int32),
                ("stripe_rows", C.c_int32), ("stripe_index", C.c_int32), ("stripe_count", C.c_int32),
                ("x0", C.c_int32), ("y0", C.c_int32), ("w", C.c_int32), ("h", C.c_int32),
                ("samples_per_group", C.c_int32), ("flags", C.c_int32)]


class Stats(C.Structure):
    _fields_ = [("rays_primary", C.c_uint64), ("rays_total", C.c_uint64), ("paths", C.c_uint64),
                ("kernel_ms", C.c_double), ("hot_kernel_ms", C.c_double), ("hot_launches", C.c_uint64),
                ("node_visits", C.c_uint64), ("prim_tests", C.c_uint64),
                ("node_bytes", C.c_uint64), ("wave_node_iters", C.c_uint64), ("wave_prim_iters", C.c_uint64),
                ("tri_tests", C.c_uint64), ("sphere_tests", C.c_uint64), ("parked", C.c_uint64),
                ("build", C.c_uint64), ("rays_recorded", C.c_uint64), ("wave_rounds", C.c_uint64),
                ("wave_rounds_idle", C.c_uint64), ("wave_lanes_live", C.c_uint64)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


RTX_DENOISE_DEMODULATE = 1


class DenoiseParams(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("flags", C.c_int32), ("normal_power", C.c_double),
                ("sigma_depth", C.c_double), ("sigma_color", C.c_double)]


class AoParams(C.Structure):
    _fields_ = [("samples", C.c_int32), ("pad_", C.c_int32), ("radius", C.c_double), ("seed", C.c_uint64)]


class RadianceParams(C.Structure):
    _fields_ = [("spp", C.c_int32), ("max_depth", C.c_int32), ("first_sample", C.c_int32), ("precision", C.c_int32),
                ("seed", C.c_uint64)]


# Every entry point include/rtx.h declares (checked by tests/test_capi_exports.py).
EXPORTS = ["rtx_abi_version", "rtx_last_error", "rtx_device_count", "rtx_scene_create", "rtx_scene_destroy",
           "rtx_intersect", "rtx_intersect_device", "rtx_camera_init", "rtx_render", "rtx_render_pixel_count",
           "rtx_render_device", "rtx_host_scene_load", "rtx_host_scene_recipe", "rtx_host_scene_write",
           "rtx_host_scene_desc", "rtx_host_scene_prim_indices", "rtx_host_scene_destroy",
           "rtx_camera_config_load", "rtx_write_ppm", "rtx_p3_max_bytes", "rtx_render_p3", "rtx_encode_p3_device",
           "rtx_prim_bounds", "rtx_bvh_build", "rtx_bvh_build_host", "rtx_render_multi", "rtx_encode_p3", "rtx_image_load",
           "rtx_film_create", "rtx_film_destroy", "rtx_film_render", "rtx_film_samples", "rtx_film_resolve",
           "rtx_film_resolve_device", "rtx_film_p3", "rtx_film_state_bytes", "rtx_film_save", "rtx_film_load",
           "rtx_film_blob_check", "rtx_denoise_params_default", "rtx_aov", "rtx_aov_device", "rtx_denoise",
           "rtx_denoise_device", "rtx_film_denoise", "rtx_film_denoise_p3", "rtx_scene_update_prims",
           "rtx_scene_update_geometry_device", "rtx_scene_epoch", "rtx_bvh_refit_host", "rtx_film_reset",
           "rtx_occluded", "rtx_occluded_device", "rtx_ao", "rtx_ao_device", "rtx_radiance", "rtx_radiance_device",
           "rtx_irradiance", "rtx_irradiance_device", "rtx_direct", "rtx_direct_device", "rtx_scene_emitters",
           "rtx_radiance_nee", "rtx_radiance_nee_device", "rtx_render_nee", "rtx_render_nee_device",
           "rtx_radiance_mis", "rtx_radiance_mis_device", "rtx_render_mis", "rtx_render_mis_device",
           "rtx_film_create_sampled", "rtx_probe_sh", "rtx_probe_sh_device", "rtx_sh_eval"]

_lib = None


def lib():
    """Load librtx.so (built in-tree by `make -C 3360-ray-tracer_amd`); raise if absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RtxError(f"{LIB_PATH} is missing: run __graft_entry__.build() or make -C 3360-ray-tracer_amd")
        L = C.CDLL(LIB_PATH)
        vp, i32, i64, sz, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t, C.c_double
        sig = {
            "rtx_abi_version": ([], C.c_int),
            "rtx_last_error": ([], C.c_char_p),
            "rtx_device_count": ([C.POINTER(C.c_int)], C.c_int),
            "rtx_scene_create": ([C.c_int, C.POINTER(SceneDesc), C.POINTER(vp)], C.c_int),
            "rtx_scene_destroy": ([vp], C.c_int),
            "rtx_intersect": ([vp, vp, sz, vp, dbl, dbl, i32], C.c_int),
            "rtx_intersect_device": ([vp, vp, sz, vp, dbl, dbl, i32, vp], C.c_int),
            "rtx_camera_init": ([C.POINTER(CameraConfig), C.POINTER(Camera)], C.c_int),
            "rtx_render": ([vp, C.POINTER(Camera), C.POINTER(RenderParams), vp, vp, C.POINTER(Stats)], C.c_int),
            "rtx_render_pixel_count": ([C.POINTER(Camera), C.POINTER(RenderParams)], i64),
            "rtx_render_device": ([vp, C.POINTER(Camera), C.POINTER(RenderParams), vp, vp, C.POINTER(Stats), vp],
                                  C.c_int),
            "rtx_host_scene_load": ([C.c_char_p, C.c_char_p, C.POINTER(vp)], C.c_int),
            "rtx_host_scene_recipe": ([C.c_char_p, C.c_uint32, C.c_char_p, C.POINTER(vp)], C.c_int),
            "rtx_host_scene_write": ([vp, C.c_char_p], C.c_int),
            "rtx_host_scene_desc": ([vp, C.POINTER(SceneDesc)], C.c_int),
            "rtx_host_scene_prim_indices": ([vp, vp, i64], C.c_int),
            "rtx_host_scene_destroy": ([vp], C.c_int),
            "rtx_camera_config_load": ([C.c_char_p, C.c_char_p, C.POINTER(CameraConfig)], C.c_int),
            "rtx_write_ppm": ([C.c_char_p, vp, i32, i32], C.c_int),
            "rtx_p3_max_bytes": ([i32, i32], sz),
            "rtx_render_p3": ([vp, C.POINTER(Camera), C.POINTER(RenderParams), vp, sz, C.POINTER(sz), vp, vp,
                               C.POINTER(Stats)], C.c_int),
            "rtx_encode_p3_device": ([vp, vp, i32, i32, vp, sz, C.POINTER(sz), vp], C.c_int),
            "rtx_prim_bounds": ([vp, i64, vp], C.c_int),
            "rtx_bvh_build": ([C.c_int, vp, i64, vp, C.POINTER(i64), vp], C.c_int),
            "rtx_bvh_build_host": ([vp, i64, vp, C.POINTER(i64), vp], C.c_int),
            "rtx_render_multi": ([C.POINTER(vp), i32, C.POINTER(Camera), C.POINTER(RenderParams), vp, vp,
                                  C.POINTER(Stats), vp], C.c_int),
            "rtx_encode_p3": ([vp, vp, i32, i32, vp, sz, C.POINTER(sz)], C.c_int),
            "rtx_image_load": ([C.c_char_p, i32, C.POINTER(i32), C.POINTER(i32), vp, sz], C.c_int),
            "rtx_film_create": ([vp, C.POINTER(Camera), C.POINTER(RenderParams), C.POINTER(vp)], C.c_int),
            "rtx_film_create_sampled": ([vp, C.POINTER(Camera), C.POINTER(RenderParams), i32, C.POINTER(vp)], C.c_int),
            "rtx_film_destroy": ([vp], C.c_int),
            "rtx_film_render": ([vp, i32, C.POINTER(Stats)], C.c_int),
            "rtx_film_samples": ([vp, C.POINTER(i32)], C.c_int),
            "rtx_film_resolve": ([vp, vp, vp], C.c_int),
            "rtx_film_resolve_device": ([vp, vp, vp, vp], C.c_int),
            "rtx_film_p3": ([vp, vp, sz, C.POINTER(sz)], C.c_int),
            "rtx_film_state_bytes": ([vp], sz),
            "rtx_film_save": ([vp, vp, sz, C.POINTER(sz)], C.c_int),
            "rtx_film_load": ([vp, C.c_char_p, sz], C.c_int),
            "rtx_film_blob_check": ([C.c_char_p, sz], C.c_int),
            "rtx_denoise_params_default": ([C.POINTER(DenoiseParams)], C.c_int),
            "rtx_aov": ([vp, C.POINTER(Camera), C.POINTER(RenderParams), vp, vp, vp], C.c_int),
            "rtx_aov_device": ([vp, C.POINTER(Camera), C.POINTER(RenderParams), vp, vp, vp, vp], C.c_int),
            "rtx_denoise": ([vp, i32, i32, vp, vp, vp, vp, vp, C.POINTER(DenoiseParams), vp], C.c_int),
            "rtx_denoise_device": ([vp, i32, i32, vp, vp, vp, vp, vp, C.POINTER(DenoiseParams), vp, vp], C.c_int),
            "rtx_film_denoise": ([vp, C.POINTER(DenoiseParams), vp], C.c_int),
            "rtx_film_denoise_p3": ([vp, C.POINTER(DenoiseParams), vp, sz, C.POINTER(sz)], C.c_int),
            "rtx_scene_update_prims": ([vp, i64, i64, vp], C.c_int),
            "rtx_scene_update_geometry_device": ([vp, i64, i64, vp, vp], C.c_int),
            "rtx_scene_epoch": ([vp, C.POINTER(i64)], C.c_int),
            "rtx_bvh_refit_host": ([vp, i64, vp, i64], C.c_int),
            "rtx_film_reset": ([vp], C.c_int),
            "rtx_occluded": ([vp, vp, sz, vp, dbl, dbl, i32], C.c_int),
            "rtx_occluded_device": ([vp, vp, sz, vp, dbl, dbl, i32, vp], C.c_int),
            "rtx_ao": ([vp, C.POINTER(Camera), C.POINTER(RenderParams), C.POINTER(AoParams), vp], C.c_int),
            "rtx_ao_device": ([vp, C.POINTER(Camera), C.POINTER(RenderParams), C.POINTER(AoParams), vp, vp], C.c_int),
            "rtx_radiance": ([vp, vp, vp, sz, C.POINTER(RadianceParams), vp, vp], C.c_int),
            "rtx_radiance_device": ([vp, vp, vp, sz, C.POINTER(RadianceParams), vp, vp, vp], C.c_int),
            "rtx_irradiance": ([vp, vp, vp, sz, C.POINTER(RadianceParams), vp, vp], C.c_int),
            "rtx_irradiance_device": ([vp, vp, vp, sz, C.POINTER(RadianceParams), vp, vp, vp], C.c_int),
            "rtx_direct": ([vp, vp, vp, sz, C.POINTER(RadianceParams), vp, vp], C.c_int),
            "rtx_direct_device": ([vp, vp, vp, sz, C.POINTER(RadianceParams), vp, vp, vp], C.c_int),
            "rtx_scene_emitters": ([vp, C.POINTER(C.c_int64), C.POINTER(C.c_double)], C.c_int),
            "rtx_radiance_nee": ([vp, vp, vp, sz, C.POINTER(RadianceParams), vp, vp], C.c_int),
            "rtx_radiance_nee_device": ([vp, vp, vp, sz, C.POINTER(RadianceParams), vp, vp, vp], C.c_int),
            "rtx_render_nee": ([vp, C.POINTER(Camera), C.POINTER(RenderParams), vp, vp], C.c_int),
            "rtx_render_nee_device": ([vp, C.POINTER(Camera), C.POINTER(RenderParams), vp, vp, vp], C.c_int),
            "rtx_radiance_mis": ([vp, vp, vp, sz, C.POINTER(RadianceParams), vp, vp], C.c_int),
            "rtx_radiance_mis_device": ([vp, vp, vp, sz, C.POINTER(RadianceParams), vp, vp, vp], C.c_int),
            "rtx_render_mis": ([vp, C.POINTER(Camera), C.POINTER(RenderParams), vp, vp], C.c_int),
            "rtx_render_mis_device": ([vp, C.POINTER(Camera), C.POINTER(RenderParams), vp, vp, vp], C.c_int),
            "rtx_probe_sh": ([vp, vp, vp, sz, C.POINTER(RadianceParams), i32, vp, vp, vp], C.c_int),
            "rtx_probe_sh_device": ([vp, vp, vp, sz, C.POINTER(RadianceParams), i32, vp, vp, vp, vp], C.c_int),
            "rtx_sh_eval": ([vp, vp, sz, i32, vp], C.c_int),
        }
        for name, (args, res) in sig.items():
            f = getattr(L, name)
            f.argtypes, f.restype = args, res
        _lib = L
    return _lib


def _check(rc, what):
    if rc != RTX_OK:
        raise RtxError(f"{what} failed ({rc}): {lib().rtx_last_error().decode()}")


def _np(struct_ptr, n, dtype_fields):
    """View n C structs as a numpy structured array (copy)."""
    if n == 0:
        return np.zeros(0)
    buf = (C.c_char * (C.sizeof(struct_ptr._type_) * n)).from_address(C.addressof(struct_ptr.contents))
    return np.frombuffer(bytes(buf), dtype=dtype_fields).copy()


NODE_DTYPE = np.dtype([("lo", "<f8", 3), ("hi", "<f8", 3), ("left_first", "<u4"), ("right_count", "<u4"),
                       ("is_leaf", "<u4"), ("pad_", "<u4")])
PRIM_DTYPE = np.dtype([("kind", "<i4"), ("material", "<i4"), ("g", "<f8", 9)])
MAT_DTYPE = np.dtype([("kind", "<i4"), ("texture", "<i4"), ("albedo", "<f8", 3), ("fuzz", "<f8"), ("ref_idx", "<f8")])
TEX_DTYPE = np.dtype([("kind", "<i4"), ("even", "<i4"), ("odd", "<i4"), ("image", "<i4"), ("color", "<f8", 3),
                      ("inv_scale", "<f8")])
HIT_DTYPE = np.dtype([("hit", "<i4"), ("front_face", "<i4"), ("material", "<i4"), ("pad_", "<i4"), ("t", "<f8"),
                      ("p", "<f8", 3), ("normal", "<f8", 3), ("u", "<f8"), ("v", "<f8")])
assert NODE_DTYPE.itemsize == 64 and PRIM_DTYPE.itemsize == 80 and HIT_DTYPE.itemsize == 88


class HostScene:
    """Host-side scene (scene file or recipe) with its SAH BVH — no GPU needed."""

    def __init__(self, handle):
        self.h = handle

    @classmethod
    def load(cls, path, asset_dir=ASSETS):
        h = C.c_void_p()
        _check(lib().rtx_host_scene_load(path.encode(), asset_dir.encode(), C.byref(h)), "rtx_host_scene_load")
        return cls(h)

    @classmethod
    def recipe(cls, name, seed=1234, asset_dir=ASSETS):
        h = C.c_void_p()
        _check(lib().rtx_host_scene_recipe(name.encode(), seed, asset_dir.encode(), C.byref(h)),
               "rtx_host_scene_recipe")
        return cls(h)

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.rtx_host_scene_destroy(self.h)
            self.h = None

    def desc(self):
        d = SceneDesc()
        _check(lib().rtx_host_scene_desc(self.h, C.byref(d)), "rtx_host_scene_desc")
        return d

    def arrays(self):
        d = self.desc()
        return {
            "prims": _np(d.prims, d.n_prims, PRIM_DTYPE),
            "nodes": _np(d.nodes, d.n_nodes, NODE_DTYPE) if d.n_nodes else np.zeros(0, NODE_DTYPE),
            "materials": _np(d.materials, d.n_materials, MAT_DTYPE),
            "textures": _np(d.textures, d.n_textures, TEX_DTYPE),
            "n_images": d.n_images,
        }

    def prim_indices(self):
        d = self.desc()
        n = d.n_prims if d.n_nodes else 0
        out = np.zeros(n, np.int32)
        if n:
            _check(lib().rtx_host_scene_prim_indices(self.h, out.ctypes.data_as(C.c_void_p), n),
                   "rtx_host_scene_prim_indices")
        return out

    def write(self, path):
        _check(lib().rtx_host_scene_write(self.h, path.encode()), "rtx_host_scene_write")


def camera_config(preset, cameras=CAMERAS, **over):
    cfg = CameraConfig()
    _check(lib().rtx_camera_config_load(cameras.encode(), preset.encode(), C.byref(cfg)), "rtx_camera_config_load")
    keymap = {"width": "image_width", "vfov": "vfov", "defocus": "defocus_angle", "focus": "focus_dist",
              "aspect": "aspect_ratio", "spp": "samples_per_pixel", "depth": "max_depth"}
    for k, v in over.items():
        setattr(cfg, keymap.get(k, k), v)
    return cfg


def camera(cfg):
    cam = Camera()
    _check(lib().rtx_camera_init(C.byref(cfg), C.byref(cam)), "rtx_camera_init")
    return cam


def device_count():
    n = C.c_int(0)
    rc = lib().rtx_device_count(C.byref(n))
    return n.value if rc == RTX_OK else 0


class DeviceScene:
    """A scene resident on one GPU (rtx_scene_create)."""

    def __init__(self, host_scene, device=0):
        self.host = host_scene  # keeps host arrays alive during upload
        self.h = C.c_void_p()
        d = host_scene.desc()
        _check(lib().rtx_scene_create(device, C.byref(d), C.byref(self.h)), "rtx_scene_create")

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.rtx_scene_destroy(self.h)
            self.h = None

    def update_prims(self, prims, first=0):
        """Replace primitives [first, first + len(prims)) (PRIM_DTYPE, the scene's own order) and
        refit both trees on the device (rtx_scene_update_prims).  Kinds must stay as they are."""
        prims = np.ascontiguousarray(prims, dtype=PRIM_DTYPE)
        _check(lib().rtx_scene_update_prims(self.h, first, len(prims), prims.ctypes.data_as(C.c_void_p)),
               "rtx_scene_update_prims")

    def update_geometry_device(self, ptr, first, count, stream=0):
        """The same from device memory (rtx_scene_update_geometry_device): ptr names count x 9
        doubles (e.g. a torch tensor's data_ptr()); kinds and materials are kept.  Asynchronous."""
        _check(lib().rtx_scene_update_geometry_device(self.h, first, count, C.c_void_p(ptr),
                                                      C.c_void_p(stream) if stream else None),
               "rtx_scene_update_geometry_device")

    def epoch(self):
        """Updates applied to the scene so far (rtx_scene_epoch)."""
        n = C.c_int64()
        _check(lib().rtx_scene_epoch(self.h, C.byref(n)), "rtx_scene_epoch")
        return n.value

    def film(self, cam, max_depth, seed=1234, adaptive=True, mode="wavefront", precision="parity", tile=None,
             stripes=None, samples_per_group=0, min_spp=16, rel_threshold=float(np.float32(0.05)), schedule=None,
             generic=False, estimator=None):
        """A resumable frame on this scene (rtx_film_create): render(budget) advances it, and after
        each call it equals the one-shot render(...) of the same arguments at spp = budget.
        estimator "nee" / "mis": a sampled film (rtx_film_create_sampled), the frame of render_nee /
        render_mis kept as a film, fixed spp (adaptive=False) or with per-pixel adaptive sampling;
        mode, schedule, generic and samples_per_group are not read."""
        p = RenderParams()
        p.spp, p.max_depth, p.adaptive = 0, max_depth, int(bool(adaptive))
        p.min_spp, p.rel_threshold, p.seed = min_spp, rel_threshold, seed
        p.mode, p.precision = MODES[mode], PRECISIONS[precision]
        p.samples_per_group = samples_per_group
        p.flags = SCHEDULE_FLAGS[schedule] | (RTX_FLAG_GENERIC if generic else 0)
        if stripes is not None:
            p.stripe_rows, p.stripe_index, p.stripe_count = stripes
        elif tile is not None:
            p.x0, p.y0, p.w, p.h = tile
        return Film(self, cam, p, ESTIMATORS[estimator])

    def intersect(self, rays, tmin=RTX_SEAM_TMIN, tmax=float("inf"), precision="parity"):
        rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
        hits = np.zeros(len(rays), HIT_DTYPE)
        _check(lib().rtx_intersect(self.h, rays.ctypes.data_as(C.c_void_p), len(rays),
                                   hits.ctypes.data_as(C.c_void_p), tmin, tmax, PRECISIONS[precision]),
               "rtx_intersect")
        return hits

    def occluded(self, rays, tmin=RTX_SEAM_TMIN, tmax=float("inf"), precision="parity"):
        """Any-hit query (rtx_occluded): (n,) uint8, 1 where some primitive is hit on (tmin, tmax);
        equals intersect(...)["hit"] != 0 for the same arguments.  A segment a -> b is origin a,
        direction b - a, tmax 1."""
        rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
        out = np.zeros(len(rays), np.uint8)
        _check(lib().rtx_occluded(self.h, rays.ctypes.data_as(C.c_void_p), len(rays), out.ctypes.data_as(C.c_void_p),
                                  tmin, tmax, PRECISIONS[precision]), "rtx_occluded")
        return out

    def occluded_device(self, d_rays, n, d_out, tmin=RTX_SEAM_TMIN, tmax=float("inf"), precision="parity", stream=0):
        """The same on device buffers (rtx_occluded_device): d_rays names n x 6 doubles, d_out n
        bytes (e.g. torch tensors' data_ptr()).  Asynchronous."""
        _check(lib().rtx_occluded_device(self.h, C.c_void_p(d_rays), n, C.c_void_p(d_out), tmin, tmax,
                                         PRECISIONS[precision], C.c_void_p(stream) if stream else None),
               "rtx_occluded_device")

    @staticmethod
    def _radiance_params(spp, max_depth, seed, first_sample, precision):
        p = RadianceParams()
        p.spp, p.max_depth, p.first_sample, p.precision, p.seed = spp, max_depth, first_sample, PRECISIONS[precision], seed
        return p

    def radiance(self, rays, spp, max_depth, seed=1234, ids=None, first_sample=0, precision="parity", segments=False):
        """Radiance query (rtx_radiance): (n, 3), the mean of `spp` paths started from each ray as
        its depth-0 segment, traced and shaded as render(mode="wavefront", adaptive=False) does.
        Path i, k draws from (seed, pixel = ids[i] or i, sample = first_sample + k), so the primary
        rays of a pixel with its global index give that pixel's render value.  segments=True: also
        the (n,) uint32 segments traced per ray."""
        rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
        n = len(rays)
        if ids is not None:
            ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
            if len(ids) != n:
                raise ValueError("radiance: one id per ray")
        out = np.zeros((n, 3))
        segs = np.zeros(n, np.uint32) if segments else None
        p = self._radiance_params(spp, max_depth, seed, first_sample, precision)
        _check(lib().rtx_radiance(self.h, rays.ctypes.data_as(C.c_void_p),
                                  None if ids is None else ids.ctypes.data_as(C.c_void_p), n, C.byref(p),
                                  out.ctypes.data_as(C.c_void_p),
                                  None if segs is None else segs.ctypes.data_as(C.c_void_p)), "rtx_radiance")
        return (out, segs) if segments else out

    def radiance_device(self, d_rays, n, d_out, spp, max_depth, seed=1234, first_sample=0, precision="parity",
                        d_ids=0, d_segments=0, stream=0):
        """The same on device buffers (rtx_radiance_device): d_rays names n x 6 doubles, d_out
        n x 3 doubles, d_ids n uint32 (0: the ray's index), d_segments n uint32 (0: none), e.g.
        torch tensors' data_ptr().  Asynchronous."""
        p = self._radiance_params(spp, max_depth, seed, first_sample, precision)
        _check(lib().rtx_radiance_device(self.h, C.c_void_p(d_rays), C.c_void_p(d_ids) if d_ids else None, n,
                                         C.byref(p), C.c_void_p(d_out), C.c_void_p(d_segments) if d_segments else None,
                                         C.c_void_p(stream) if stream else None), "rtx_radiance_device")

    def irradiance(self, points, normals, samples, max_depth, seed=1234, ids=None, first_sample=0, precision="parity",
                   segments=False):
        """Irradiance query (rtx_irradiance): (n, 3), the cosine-weighted mean radiance arriving at
        each point over the hemisphere about its normal (any positive finite length), from
        `samples` paths per point traced and shaded as radiance() does; pi times it is the
        radiometric irradiance.  Sample k of point i draws from (seed, pixel = ids[i] or i,
        sample = first_sample + k) and equals radiance() of its ray (irradiance_rays) with that id,
        spp = 1 and first_sample + k.  A zero or non-finite normal gives 0 0 0 and 0 segments.
        segments=True: also the (n,) uint32 segments traced per point."""
        surfels = _surfels(points, normals)
        n = len(surfels)
        if ids is not None:
            ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
            if len(ids) != n:
                raise ValueError("irradiance: one id per point")
        out = np.zeros((n, 3))
        segs = np.zeros(n, np.uint32) if segments else None
        p = self._radiance_params(samples, max_depth, seed, first_sample, precision)
        _check(lib().rtx_irradiance(self.h, surfels.ctypes.data_as(C.c_void_p),
                                    None if ids is None else ids.ctypes.data_as(C.c_void_p), n, C.byref(p),
                                    out.ctypes.data_as(C.c_void_p),
                                    None if segs is None else segs.ctypes.data_as(C.c_void_p)), "rtx_irradiance")
        return (out, segs) if segments else out

    def irradiance_device(self, d_surfels, n, d_out, samples, max_depth, seed=1234, first_sample=0, precision="parity",
                          d_ids=0, d_segments=0, stream=0):
        """The same on device buffers (rtx_irradiance_device): d_surfels names n x 6 doubles (point,
        normal), d_out n x 3 doubles, d_ids n uint32 (0: the point's index), d_segments n uint32
        (0: none), e.g. torch tensors' data_ptr().  Asynchronous."""
        p = self._radiance_params(samples, max_depth, seed, first_sample, precision)
        _check(lib().rtx_irradiance_device(self.h, C.c_void_p(d_surfels), C.c_void_p(d_ids) if d_ids else None, n,
                                           C.byref(p), C.c_void_p(d_out),
                                           C.c_void_p(d_segments) if d_segments else None,
                                           C.c_void_p(stream) if stream else None), "rtx_irradiance_device")

    def direct(self, points, normals, samples, seed=1234, ids=None, first_sample=0, precision="parity", visible=False):
        """Direct-lighting query (rtx_direct): (n, 3), the light reaching each point straight from
        the scene's emitters, in irradiance()'s unit (the two add and compare directly), from
        `samples` points per surfel drawn uniformly over the emitting area, each weighted by the
        geometry term and by the visibility of its shadow segment (occluded() on (RTX_SEAM_TMIN,
        RTX_DIRECT_TMAX)).  Sample k of point i draws from (seed, pixel = ids[i] or i,
        sample = first_sample + k) and equals direct_samples()'s C times that visibility.  A zero
        or non-finite normal, and a scene without emitters, give 0 0 0.  visible=True: also the
        (n,) uint32 samples per point whose segment was traced and found unoccluded."""
        surfels = _surfels(points, normals)
        n = len(surfels)
        if ids is not None:
            ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
            if len(ids) != n:
                raise ValueError("direct: one id per point")
        out = np.zeros((n, 3))
        vis = np.zeros(n, np.uint32) if visible else None
        p = self._radiance_params(samples, 0, seed, first_sample, precision)
        _check(lib().rtx_direct(self.h, surfels.ctypes.data_as(C.c_void_p),
                                None if ids is None else ids.ctypes.data_as(C.c_void_p), n, C.byref(p),
                                out.ctypes.data_as(C.c_void_p),
                                None if vis is None else vis.ctypes.data_as(C.c_void_p)), "rtx_direct")
        return (out, vis) if visible else out

    def direct_device(self, d_surfels, n, d_out, samples, seed=1234, first_sample=0, precision="parity", d_ids=0,
                      d_visible=0, stream=0):
        """The same on device buffers (rtx_direct_device): d_surfels names n x 6 doubles (point,
        normal), d_out n x 3 doubles, d_ids n uint32 (0: the point's index), d_visible n uint32
        (0: none), e.g. torch tensors' data_ptr().  Asynchronous."""
        p = self._radiance_params(samples, 0, seed, first_sample, precision)
        _check(lib().rtx_direct_device(self.h, C.c_void_p(d_surfels), C.c_void_p(d_ids) if d_ids else None, n,
                                       C.byref(p), C.c_void_p(d_out), C.c_void_p(d_visible) if d_visible else None,
                                       C.c_void_p(stream) if stream else None), "rtx_direct_device")

    def emitters(self):
        """(count, area): the scene's emitters (primitives with a DiffuseLight material) and their
        total area in the live scene (rtx_scene_emitters); (0, 0.0) without emitters."""
        n, a = C.c_int64(0), C.c_double(0.0)
        _check(lib().rtx_scene_emitters(self.h, C.byref(n), C.byref(a)), "rtx_scene_emitters")
        return n.value, a.value

    def radiance_nee(self, rays, spp, max_depth, seed=1234, ids=None, first_sample=0, precision="parity",
                     segments=False):
        """Radiance query with next-event estimation (rtx_radiance_nee): radiance()'s arguments,
        paths and keys; at every vertex where a Lambertian scattered (and depth + 1 < max_depth) one
        emitter sample of direct() is added, weighted by the path's throughput and the surface's
        reflectance, and an emitter hit right after such a vertex counts 0.  The same expectation
        as radiance() with far less variance where lights are small; without emitters, or with
        max_depth <= 1, the same bits.  segments=True: also the (n,) uint32 closest-hit plus
        shadow segments traced per ray."""
        return self._radiance_sampled("nee", rays, spp, max_depth, seed, ids, first_sample, precision, segments)

    def _radiance_sampled(self, family, rays, spp, max_depth, seed, ids, first_sample, precision, segments):
        """radiance_nee() / radiance_mis(): rtx_radiance_<family> on host arrays."""
        rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
        n = len(rays)
        if ids is not None:
            ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
            if len(ids) != n:
                raise ValueError("radiance_%s: one id per ray" % family)
        out = np.zeros((n, 3))
        segs = np.zeros(n, np.uint32) if segments else None
        p = self._radiance_params(spp, max_depth, seed, first_sample, precision)
        name = "rtx_radiance_" + family
        _check(getattr(lib(), name)(self.h, rays.ctypes.data_as(C.c_void_p),
                                    None if ids is None else ids.ctypes.data_as(C.c_void_p), n, C.byref(p),
                                    out.ctypes.data_as(C.c_void_p),
                                    None if segs is None else segs.ctypes.data_as(C.c_void_p)), name)
        return (out, segs) if segments else out

    def radiance_nee_device(self, d_rays, n, d_out, spp, max_depth, seed=1234, first_sample=0, precision="parity",
                            d_ids=0, d_segments=0, stream=0):
        """The same on device buffers (rtx_radiance_nee_device), with radiance_device()'s
        arguments.  Asynchronous."""
        p = self._radiance_params(spp, max_depth, seed, first_sample, precision)
        _check(lib().rtx_radiance_nee_device(self.h, C.c_void_p(d_rays), C.c_void_p(d_ids) if d_ids else None, n,
                                             C.byref(p), C.c_void_p(d_out),
                                             C.c_void_p(d_segments) if d_segments else None,
                                             C.c_void_p(stream) if stream else None), "rtx_radiance_nee_device")

    def _nee_frame_args(self, cam, spp, max_depth, seed, precision, tile, stripes):
        p = RenderParams()
        p.spp, p.max_depth, p.seed, p.precision = spp, max_depth, seed, PRECISIONS[precision]
        if stripes is not None:
            p.stripe_rows, p.stripe_index, p.stripe_count = stripes
        elif tile is not None:
            p.x0, p.y0, p.w, p.h = tile
        n = lib().rtx_render_pixel_count(C.byref(cam), C.byref(p))
        if n < 0:
            _check(n, "rtx_render_pixel_count")
        return p, n

    def render_nee(self, cam, spp, max_depth, seed=1234, precision="parity", tile=None, stripes=None):
        """A frame with next-event estimation (rtx_render_nee): (rgb (n, 3), segments (n,) uint32)
        for the pixel subset in subset order, fixed spp; each pixel's samples are radiance_nee() of
        the camera's own rays keyed by the global pixel index.  Without emitters rgb equals
        render(adaptive=False, mode="wavefront")'s."""
        p, n = self._nee_frame_args(cam, spp, max_depth, seed, precision, tile, stripes)
        rgb = np.zeros((n, 3))
        segs = np.zeros(n, np.uint32)
        _check(lib().rtx_render_nee(self.h, C.byref(cam), C.byref(p), rgb.ctypes.data_as(C.c_void_p),
                                    segs.ctypes.data_as(C.c_void_p)), "rtx_render_nee")
        return rgb, segs

    def render_nee_device(self, cam, d_rgb, spp, max_depth, seed=1234, precision="parity", tile=None, stripes=None,
                          d_segments=0, stream=0):
        """The same into device buffers (rtx_render_nee_device): d_rgb names n x 3 doubles,
        d_segments n uint32 (0: none).  Asynchronous; returns the subset's pixel count."""
        p, n = self._nee_frame_args(cam, spp, max_depth, seed, precision, tile, stripes)
        _check(lib().rtx_render_nee_device(self.h, C.byref(cam), C.byref(p), C.c_void_p(d_rgb),
                                           C.c_void_p(d_segments) if d_segments else None,
                                           C.c_void_p(stream) if stream else None), "rtx_render_nee_device")
        return n

    def radiance_mis(self, rays, spp, max_depth, seed=1234, ids=None, first_sample=0, precision="parity",
                     segments=False):
        """Radiance query with multiple importance sampling (rtx_radiance_mis): radiance_nee()'s
        arguments, paths, emitter samples and segment counts; each emitter sample is weighted by
        the power heuristic's 1 / (1 + g^2) (g: the ratio of the BSDF's density to the light
        sampler's at that pair of points), and an emitter hit right after such a vertex counts with
        the complementary weight instead of 0 (with weight 1 for a light the emitter table does
        not hold).  The same expectation as radiance(), without radiance_nee()'s fireflies where a
        surface comes close to a light; without emitters, or with max_depth <= 1, the same bits."""
        return self._radiance_sampled("mis", rays, spp, max_depth, seed, ids, first_sample, precision, segments)

    def radiance_mis_device(self, d_rays, n, d_out, spp, max_depth, seed=1234, first_sample=0, precision="parity",
                            d_ids=0, d_segments=0, stream=0):
        """The same on device buffers (rtx_radiance_mis_device), with radiance_device()'s
        arguments.  Asynchronous."""
        p = self._radiance_params(spp, max_depth, seed, first_sample, precision)
        _check(lib().rtx_radiance_mis_device(self.h, C.c_void_p(d_rays), C.c_void_p(d_ids) if d_ids else None, n,
                                             C.byref(p), C.c_void_p(d_out),
                                             C.c_void_p(d_segments) if d_segments else None,
                                             C.c_void_p(stream) if stream else None), "rtx_radiance_mis_device")

    def render_mis(self, cam, spp, max_depth, seed=1234, precision="parity", tile=None, stripes=None):
        """A frame with multiple importance sampling (rtx_render_mis): render_nee()'s arguments and
        outputs; each pixel's samples are radiance_mis() of the camera's own rays keyed by the
        global pixel index."""
        p, n = self._nee_frame_args(cam, spp, max_depth, seed, precision, tile, stripes)
        rgb = np.zeros((n, 3))
        segs = np.zeros(n, np.uint32)
        _check(lib().rtx_render_mis(self.h, C.byref(cam), C.byref(p), rgb.ctypes.data_as(C.c_void_p),
                                    segs.ctypes.data_as(C.c_void_p)), "rtx_render_mis")
        return rgb, segs

    def render_mis_device(self, cam, d_rgb, spp, max_depth, seed=1234, precision="parity", tile=None, stripes=None,
                          d_segments=0, stream=0):
        """The same into device buffers (rtx_render_mis_device), with render_nee_device()'s
        arguments.  Asynchronous; returns the subset's pixel count."""
        p, n = self._nee_frame_args(cam, spp, max_depth, seed, precision, tile, stripes)
        _check(lib().rtx_render_mis_device(self.h, C.byref(cam), C.byref(p), C.c_void_p(d_rgb),
                                           C.c_void_p(d_segments) if d_segments else None,
                                           C.c_void_p(stream) if stream else None), "rtx_render_mis_device")
        return n

    def probe_sh(self, points, samples, max_depth, seed=1234, ids=None, first_sample=0, precision="parity",
                 estimator=None, segments=False, backfaces=False):
        """Light probes (rtx_probe_sh): (n, 9, 3), the radiance arriving at each point over the whole
        sphere projected onto the real SH basis to band 2 ([coefficient][r, g, b]), from `samples`
        paths per point in uniform directions, traced as radiance() does (estimator None), or as
        radiance_nee() / radiance_mis() ("nee", "mis").  Sample k of probe i draws from (seed,
        pixel = ids[i] or i, sample = first_sample + k) and equals that query of its ray
        (probe_rays) with that id, spp = 1 and first_sample + k.  A non-finite point gives zeros.
        segments=True: also the (n,) uint32 segments traced per probe; backfaces=True: also the
        (n,) uint32 samples whose depth-0 segment hit a primitive from inside."""
        points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        n = len(points)
        if ids is not None:
            ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
            if len(ids) != n:
                raise ValueError("probe_sh: one id per point")
        out = np.zeros((n, 9, 3))
        segs = np.zeros(n, np.uint32) if segments else None
        back = np.zeros(n, np.uint32) if backfaces else None
        p = self._radiance_params(samples, max_depth, seed, first_sample, precision)
        _check(lib().rtx_probe_sh(self.h, points.ctypes.data_as(C.c_void_p),
                                  None if ids is None else ids.ctypes.data_as(C.c_void_p), n, C.byref(p),
                                  ESTIMATORS[estimator], out.ctypes.data_as(C.c_void_p),
                                  None if segs is None else segs.ctypes.data_as(C.c_void_p),
                                  None if back is None else back.ctypes.data_as(C.c_void_p)), "rtx_probe_sh")
        extra = tuple(a for a in (segs, back) if a is not None)
        return (out,) + extra if extra else out

    def probe_sh_device(self, d_points, n, d_out, samples, max_depth, seed=1234, first_sample=0, precision="parity",
                        estimator=None, d_ids=0, d_segments=0, d_backfaces=0, stream=0):
        """The same on device buffers (rtx_probe_sh_device): d_points names n x 3 doubles, d_out
        n x 27 doubles, d_ids n uint32 (0: the point's index), d_segments and d_backfaces n uint32
        (0: none), e.g. torch tensors' data_ptr().  Asynchronous."""
        p = self._radiance_params(samples, max_depth, seed, first_sample, precision)
        _check(lib().rtx_probe_sh_device(self.h, C.c_void_p(d_points), C.c_void_p(d_ids) if d_ids else None, n,
                                         C.byref(p), ESTIMATORS[estimator], C.c_void_p(d_out),
                                         C.c_void_p(d_segments) if d_segments else None,
                                         C.c_void_p(d_backfaces) if d_backfaces else None,
                                         C.c_void_p(stream) if stream else None), "rtx_probe_sh_device")

    def _ao_args(self, cam, samples, radius, seed, tile, stripes, precision):
        p = RenderParams()
        p.precision = PRECISIONS[precision]
        if stripes is not None:
            p.stripe_rows, p.stripe_index, p.stripe_count = stripes
        elif tile is not None:
            p.x0, p.y0, p.w, p.h = tile
        n = lib().rtx_render_pixel_count(C.byref(cam), C.byref(p))
        if n < 0:
            _check(n, "rtx_render_pixel_count")
        a = AoParams()
        a.samples, a.radius, a.seed = samples, radius, seed
        return p, a, n

    def ao(self, cam, samples=16, radius=1.0, seed=1234, tile=None, stripes=None, precision="parity"):
        """Ambient occlusion of the pixel subset (rtx_ao), (n,) in subset order: the share of
        `samples` cosine-weighted rays from each pixel's first hit that reach `radius` unoccluded
        (1.0 where the pixel's ray misses)."""
        p, a, n = self._ao_args(cam, samples, radius, seed, tile, stripes, precision)
        out = np.zeros(n)
        _check(lib().rtx_ao(self.h, C.byref(cam), C.byref(p), C.byref(a), out.ctypes.data_as(C.c_void_p)), "rtx_ao")
        return out

    def aov(self, cam, tile=None, stripes=None, precision="parity"):
        """First-hit AOVs of the pixel subset (rtx_aov), in subset order: (albedo (n, 3), normal
        (n, 3), depth (n,)) from the ray through each pixel's centre."""
        p = RenderParams()
        p.precision = PRECISIONS[precision]
        if stripes is not None:
            p.stripe_rows, p.stripe_index, p.stripe_count = stripes
        elif tile is not None:
            p.x0, p.y0, p.w, p.h = tile
        n = lib().rtx_render_pixel_count(C.byref(cam), C.byref(p))
        if n < 0:
            _check(n, "rtx_render_pixel_count")
        albedo, normal, depth = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n)
        _check(lib().rtx_aov(self.h, C.byref(cam), C.byref(p), albedo.ctypes.data_as(C.c_void_p),
                             normal.ctypes.data_as(C.c_void_p), depth.ctypes.data_as(C.c_void_p)), "rtx_aov")
        return albedo, normal, depth

    def render(self, cam, spp, max_depth, seed=1234, adaptive=True, mode="wavefront", precision="parity",
               tile=None, stripes=None, samples_per_group=0, min_spp=16, rel_threshold=float(np.float32(0.05)),
               count=False, schedule=None, generic=False, adapt_schedule=None):
        p = RenderParams()
        p.spp, p.max_depth, p.adaptive = spp, max_depth, int(bool(adaptive))
        p.min_spp, p.rel_threshold, p.seed = min_spp, rel_threshold, seed
        p.mode, p.precision = MODES[mode], PRECISIONS[precision]
        p.samples_per_group = samples_per_group
        p.flags = ((1 if count else 0) | SCHEDULE_FLAGS[schedule] | (RTX_FLAG_GENERIC if generic else 0)
                   | ADAPT_SCHEDULE_FLAGS[adapt_schedule])
        if stripes is not None:
            p.stripe_rows, p.stripe_index, p.stripe_count = stripes
        elif tile is not None:
            p.x0, p.y0, p.w, p.h = tile
        n = lib().rtx_render_pixel_count(C.byref(cam), C.byref(p))
        if n < 0:
            _check(n, "rtx_render_pixel_count")
        rgb = np.zeros((n, 3))
        spp_out = np.zeros(n, np.int32)
        st = Stats()
        _check(lib().rtx_render(self.h, C.byref(cam), C.byref(p), rgb.ctypes.data_as(C.c_void_p),
                                spp_out.ctypes.data_as(C.c_void_p), C.byref(st)), "rtx_render")
        return rgb, spp_out, st.as_dict()

    def render_p3(self, cam, spp, max_depth, seed=1234, adaptive=True, mode="wavefront", precision="parity",
                  tile=None):
        """Render and return the P3 PPM file bytes, encoded on the device (rtx_render_p3)."""
        p = RenderParams()
        p.spp, p.max_depth, p.adaptive = spp, max_depth, int(bool(adaptive))
        p.min_spp, p.rel_threshold, p.seed = 16, float(np.float32(0.05)), seed
        p.mode, p.precision = MODES[mode], PRECISIONS[precision]
        if tile is not None:
            p.x0, p.y0, p.w, p.h = tile
        cap = lib().rtx_p3_max_bytes(cam.image_width, cam.image_height)
        buf = C.create_string_buffer(cap)
        n = C.c_size_t()
        st = Stats()
        _check(lib().rtx_render_p3(self.h, C.byref(cam), C.byref(p), buf, cap, C.byref(n), None, None,
                                   C.byref(st)), "rtx_render_p3")
        return buf.raw[:n.value], st.as_dict()

    def encode_p3_device(self, d_rgb, width, height, d_out, cap, stream=0):
        """P3 bytes of a device framebuffer into a device buffer; returns the byte count."""
        n = C.c_size_t()
        _check(lib().rtx_encode_p3_device(self.h, C.c_void_p(d_rgb), width, height, C.c_void_p(d_out), cap,
                                          C.byref(n), C.c_void_p(stream) if stream else None),
               "rtx_encode_p3_device")
        return n.value

    def render_device(self, cam, params, d_rgb, d_spp=0, stream=0, stats=True):
        """Device-resident render into caller buffers (e.g. torch tensors' data_ptr()).
        stats=False: no statistics, so the call returns without waiting for the render."""
        st = Stats()
        _check(lib().rtx_render_device(self.h, C.byref(cam), C.byref(params), C.c_void_p(d_rgb),
                                       C.c_void_p(d_spp) if d_spp else None, C.byref(st) if stats else None,
                                       C.c_void_p(stream) if stream else None), "rtx_render_device")
        return st.as_dict() if stats else None


RTX_ESTIMATOR_NEE, RTX_ESTIMATOR_MIS = 1, 2
ESTIMATORS = {None: 0, "nee": RTX_ESTIMATOR_NEE, "mis": RTX_ESTIMATOR_MIS}


class Film:
    """A frame rendered in steps (rtx_film_*): the per-pixel state stays on the scene's device
    between calls.  Made by DeviceScene.film(); it keeps its scene alive."""

    def __init__(self, scene, cam, params, estimator=0):
        self.scene = scene
        self.h = C.c_void_p()
        n = lib().rtx_render_pixel_count(C.byref(cam), C.byref(params))
        if n < 0:
            _check(n, "rtx_render_pixel_count")
        self.npix = n
        self._p3_cap = lib().rtx_p3_max_bytes(cam.image_width, cam.image_height)
        if estimator:
            _check(lib().rtx_film_create_sampled(scene.h, C.byref(cam), C.byref(params), estimator, C.byref(self.h)),
                   "rtx_film_create_sampled")
        else:
            _check(lib().rtx_film_create(scene.h, C.byref(cam), C.byref(params), C.byref(self.h)), "rtx_film_create")

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.rtx_film_destroy(self.h)
        self.h = None

    __del__ = close

    def _handle(self):
        if not self.h:
            raise RtxError("the film is closed")
        return self.h

    def render(self, budget):
        """Advance to `budget` samples per pixel; returns this call's statistics."""
        st = Stats()
        _check(lib().rtx_film_render(self._handle(), budget, C.byref(st)), "rtx_film_render")
        return st.as_dict()

    def reset(self):
        """Zero the film and bind it to its scene's current epoch (rtx_film_reset): the way to go
        on after the scene was updated."""
        _check(lib().rtx_film_reset(self._handle()), "rtx_film_reset")

    @property
    def samples(self):
        n = C.c_int32()
        _check(lib().rtx_film_samples(self._handle(), C.byref(n)), "rtx_film_samples")
        return n.value

    def resolve(self):
        """(rgb (npix, 3), spp (npix,)) at the current budget, in subset order."""
        rgb = np.zeros((self.npix, 3))
        spp = np.zeros(self.npix, np.int32)
        _check(lib().rtx_film_resolve(self._handle(), rgb.ctypes.data_as(C.c_void_p), spp.ctypes.data_as(C.c_void_p)),
               "rtx_film_resolve")
        return rgb, spp

    def p3(self):
        """The P3 PPM file bytes of the current output, encoded on the device."""
        buf = C.create_string_buffer(self._p3_cap)
        n = C.c_size_t()
        _check(lib().rtx_film_p3(self._handle(), buf, self._p3_cap, C.byref(n)), "rtx_film_p3")
        return buf.raw[:n.value]

    def denoise(self, **over):
        """The current output filtered with the film's own first-hit AOVs (rtx_film_denoise):
        (npix, 3) in subset order.  over: denoise_params fields.  The film is not changed."""
        rgb = np.zeros((self.npix, 3))
        _check(lib().rtx_film_denoise(self._handle(), C.byref(denoise_params(**over)), rgb.ctypes.data_as(C.c_void_p)),
               "rtx_film_denoise")
        return rgb

    def denoise_p3(self, **over):
        """The P3 PPM file bytes of denoise(**over), encoded on the device."""
        buf = C.create_string_buffer(self._p3_cap)
        n = C.c_size_t()
        _check(lib().rtx_film_denoise_p3(self._handle(), C.byref(denoise_params(**over)), buf, self._p3_cap,
                                         C.byref(n)), "rtx_film_denoise_p3")
        return buf.raw[:n.value]

    def save(self):
        cap = lib().rtx_film_state_bytes(self._handle())
        buf = C.create_string_buffer(cap)
        n = C.c_size_t()
        _check(lib().rtx_film_save(self.h, buf, cap, C.byref(n)), "rtx_film_save")
        return buf.raw[:n.value]

    def load(self, blob):
        blob = bytes(blob)
        _check(lib().rtx_film_load(self._handle(), blob, len(blob)), "rtx_film_load")


def film_blob_check(blob):
    """Header and length of a saved film (rtx_film_blob_check; no device needed): raises RtxError
    naming what is wrong."""
    blob = bytes(blob)
    _check(lib().rtx_film_blob_check(blob, len(blob)), "rtx_film_blob_check")


def denoise_params(**over):
    """The denoiser's defaults (rtx_denoise_params_default) with fields replaced: iterations, flags,
    normal_power, sigma_depth, sigma_color; demodulate=bool sets or clears RTX_DENOISE_DEMODULATE."""
    p = DenoiseParams()
    _check(lib().rtx_denoise_params_default(C.byref(p)), "rtx_denoise_params_default")
    if "demodulate" in over:
        on = over.pop("demodulate")
        p.flags = (p.flags | RTX_DENOISE_DEMODULATE) if on else (p.flags & ~RTX_DENOISE_DEMODULATE)
    for k, v in over.items():
        if k not in dict(DenoiseParams._fields_):
            raise TypeError(f"denoise_params: unknown field {k!r}")
        setattr(p, k, v)
    return p


def denoise(scene, rgb, albedo, normal, depth, width, height, variance=None, **over):
    """Edge-avoiding a-trous filter of a width x height host image on `scene`'s device
    (rtx_denoise): rgb, albedo, normal (n, 3), depth and the optional variance (n,), row-major;
    over: denoise_params fields.  Returns the filtered (n, 3) image."""
    n = width * height
    arr = [np.ascontiguousarray(a, dtype=np.float64).reshape(n, k)
           for a, k in ((rgb, 3), (albedo, 3), (normal, 3), (depth, 1))]
    var = None if variance is None else np.ascontiguousarray(variance, dtype=np.float64).reshape(n)
    out = np.zeros((n, 3))
    _check(lib().rtx_denoise(scene.h, width, height, *[a.ctypes.data_as(C.c_void_p) for a in arr],
                             None if var is None else var.ctypes.data_as(C.c_void_p),
                             C.byref(denoise_params(**over)), out.ctypes.data_as(C.c_void_p)), "rtx_denoise")
    return out


def ao_rays(scene, cam, samples=16, radius=1.0, seed=1234, tile=None, stripes=None, precision="parity"):
    """Test hook (rtx_internal_ao_rays, not in rtx.h): the sample rays DeviceScene.ao traces for
    the same arguments, (n, samples, 6), from the device function the AO kernel calls; all zero
    for a pixel whose ray misses."""
    p, a, n = scene._ao_args(cam, samples, radius, seed, tile, stripes, precision)
    f = lib().rtx_internal_ao_rays
    f.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderParams), C.POINTER(AoParams), C.c_void_p]
    f.restype = C.c_int
    out = np.zeros((n, samples, 6))
    _check(f(scene.h, C.byref(cam), C.byref(p), C.byref(a), out.ctypes.data_as(C.c_void_p)), "rtx_internal_ao_rays")
    return out


def camera_rays(scene, cam, spp, seed=1234, first_sample=0, tile=None, stripes=None):
    """Test hook (rtx_internal_camera_rays, not in rtx.h): the primary rays the render kernels
    generate for samples [first_sample, first_sample + spp) of the pixel subset, (n, spp, 6) in
    subset order, from the device function they call."""
    p = RenderParams()
    p.seed = seed
    if stripes is not None:
        p.stripe_rows, p.stripe_index, p.stripe_count = stripes
    elif tile is not None:
        p.x0, p.y0, p.w, p.h = tile
    n = lib().rtx_render_pixel_count(C.byref(cam), C.byref(p))
    if n < 0:
        _check(n, "rtx_render_pixel_count")
    f = lib().rtx_internal_camera_rays
    f.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderParams), C.c_int32, C.c_int32, C.c_void_p]
    f.restype = C.c_int
    out = np.zeros((n, spp, 6))
    _check(f(scene.h, C.byref(cam), C.byref(p), first_sample, spp, out.ctypes.data_as(C.c_void_p)),
           "rtx_internal_camera_rays")
    return out


# rtx_internal_shade_steps (csrc/rtx_shade_steps.h): a case (hit record, path state, Philox key)
# and the step's outcome
SHADE_CASE_DTYPE = np.dtype([("p", "<f8", 3), ("normal", "<f8", 3), ("u", "<f8"), ("v", "<f8"), ("o", "<f8", 3),
                             ("d", "<f8", 3), ("thr", "<f8", 3), ("seed", "<u8"), ("pixel", "<u4"), ("sample", "<u4"),
                             ("hit", "<i4"), ("front_face", "<i4"), ("mat", "<i4"), ("depth", "<i4"),
                             ("max_depth", "<i4"), ("lazy_uv", "<i4")])
SHADE_RECORD_DTYPE = np.dtype([("L", "<f8", 3), ("o", "<f8", 3), ("d", "<f8", 3), ("thr", "<f8", 3), ("next", "<f8"),
                               ("cont", "<i4"), ("depth", "<i4")])
assert SHADE_CASE_DTYPE.itemsize == 176 and SHADE_RECORD_DTYPE.itemsize == 112
# "core...": shade_core<LAMB, NOTEX, SET_ORIGIN> + shade_finish, the persistent kernel's form;
# "_noorigin": SET_ORIGIN = false (the hook sets the child's origin, as that kernel does)
SHADE_VARIANTS = {"shade": 0, "terminal": 1, "scatter": 2, "core": 8, "core_lamb": 9, "core_notex": 10,
                  "core_lamb_notex": 11, "core_noorigin": 12, "core_lamb_noorigin": 13, "core_notex_noorigin": 14,
                  "core_lamb_notex_noorigin": 15}


def shade_steps(scene, cases, variant="shade"):
    """Test hook (rtx_internal_shade_steps, not in rtx.h): one shading step per case
    (SHADE_CASE_DTYPE) through the device functions the render kernels call, on the scene's own
    material, texture and image tables; returns SHADE_RECORD_DTYPE.  variant: SHADE_VARIANTS.  A
    "lamb" / "notex" form of a scene whose flags do not allow it raises; "terminal" marks a case
    that does not end on the sky with cont = -1; "scatter" reads depth as the remaining depth."""
    cases = np.ascontiguousarray(cases, dtype=SHADE_CASE_DTYPE)
    out = np.zeros(len(cases), SHADE_RECORD_DTYPE)
    f = lib().rtx_internal_shade_steps
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, C.c_void_p]
    f.restype = C.c_int
    _check(f(scene.h, cases.ctypes.data_as(C.c_void_p), len(cases), SHADE_VARIANTS[variant],
             out.ctypes.data_as(C.c_void_p)), "rtx_internal_shade_steps")
    return out


def _surfels(points, normals):
    """(n, 6) doubles: point, normal (the rtx_ray layout of rtx_irradiance's surfels)."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    normals = np.asarray(normals, dtype=np.float64).reshape(-1, 3)
    if len(points) != len(normals):
        raise ValueError("irradiance: one normal per point")
    return np.ascontiguousarray(np.concatenate([points, normals], axis=1))


def irradiance_rays(scene, points, normals, samples, seed, ids=None, first_sample=0):
    """Test hook (rtx_internal_irradiance_rays, not in rtx.h): the depth-0 segments
    DeviceScene.irradiance traces for the same arguments, (n, samples, 6), from the device
    function the irradiance kernel calls; all zero for a point with a degenerate normal."""
    surfels = _surfels(points, normals)
    n = len(surfels)
    if ids is not None:
        ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        if len(ids) != n:
            raise ValueError("irradiance: one id per point")
    f = lib().rtx_internal_irradiance_rays
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(RadianceParams), C.c_void_p]
    f.restype = C.c_int
    p = DeviceScene._radiance_params(samples, 0, seed, first_sample, "parity")
    out = np.zeros((n, samples, 6))
    _check(f(scene.h, surfels.ctypes.data_as(C.c_void_p), None if ids is None else ids.ctypes.data_as(C.c_void_p), n,
             C.byref(p), out.ctypes.data_as(C.c_void_p)), "rtx_internal_irradiance_rays")
    return out


def probe_rays(scene, points, samples, seed, ids=None, first_sample=0):
    """Test hook (rtx_internal_probe_rays, not in rtx.h): the depth-0 segments DeviceScene.probe_sh
    traces for the same arguments, (n, samples, 6), from the device function the probe kernels
    call; all zero for a point with a non-finite coordinate."""
    points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    n = len(points)
    if ids is not None:
        ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        if len(ids) != n:
            raise ValueError("probe_rays: one id per point")
    f = lib().rtx_internal_probe_rays
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(RadianceParams), C.c_void_p]
    f.restype = C.c_int
    p = DeviceScene._radiance_params(samples, 0, seed, first_sample, "parity")
    out = np.zeros((n, samples, 6))
    _check(f(scene.h, points.ctypes.data_as(C.c_void_p), None if ids is None else ids.ctypes.data_as(C.c_void_p), n,
             C.byref(p), out.ctypes.data_as(C.c_void_p)), "rtx_internal_probe_rays")
    return out


# the constants of the real SH basis to band 2 (include/rtx.h, RTX_SH_K*)
SH_K0, SH_K1, SH_K4 = 0.28209479177387814, 0.48860251190291992, 1.0925484305920792
SH_K6, SH_K8 = 0.31539156525251999, 0.54627421529603959


def sh_eval(sh, dirs, cosine=False):
    """rtx_sh_eval: one probe's coefficients (9, 3) at unit directions (n, 3) -> (n, 3): the
    reconstruction, or with cosine=True the cosine-convolved value over pi about each direction as
    a normal (irradiance()'s unit).  Host only."""
    sh = np.ascontiguousarray(sh, dtype=np.float64)
    if sh.size != 27:
        raise ValueError("sh_eval: 9 x 3 coefficients")
    dirs = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
    out = np.zeros((len(dirs), 3))
    _check(lib().rtx_sh_eval(sh.ctypes.data_as(C.c_void_p), dirs.ctypes.data_as(C.c_void_p), len(dirs),
                             1 if cosine else 0, out.ctypes.data_as(C.c_void_p)), "rtx_sh_eval")
    return out


def direct_samples(scene, points, normals, samples, seed, ids=None, first_sample=0):
    """Test hook (rtx_internal_direct_samples, not in rtx.h): the samples DeviceScene.direct draws
    for the same arguments, (n, samples, 9): the shadow segment's origin, y - x, and the unshadowed
    contribution C, from the device function the kernel calls; all zero where nothing is traced."""
    surfels = _surfels(points, normals)
    n = len(surfels)
    if ids is not None:
        ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        if len(ids) != n:
            raise ValueError("direct: one id per point")
    f = lib().rtx_internal_direct_samples
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(RadianceParams), C.c_void_p]
    f.restype = C.c_int
    p = DeviceScene._radiance_params(samples, 0, seed, first_sample, "parity")
    out = np.zeros((n, samples, 9))
    _check(f(scene.h, surfels.ctypes.data_as(C.c_void_p), None if ids is None else ids.ctypes.data_as(C.c_void_p), n,
             C.byref(p), out.ctypes.data_as(C.c_void_p)), "rtx_internal_direct_samples")
    return out


def nee_samples(scene, points, normals, samples, seed, depth, ids=None, first_sample=0):
    """Test hook (rtx_internal_nee_samples, not in rtx.h): direct_samples() on the stream a path of
    DeviceScene.radiance_nee draws from at a vertex of `depth`, (n, samples, 9)."""
    surfels = _surfels(points, normals)
    n = len(surfels)
    if ids is not None:
        ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        if len(ids) != n:
            raise ValueError("nee_samples: one id per point")
    f = lib().rtx_internal_nee_samples
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(RadianceParams), C.c_int32, C.c_void_p]
    f.restype = C.c_int
    p = DeviceScene._radiance_params(samples, 0, seed, first_sample, "parity")
    out = np.zeros((n, samples, 9))
    _check(f(scene.h, surfels.ctypes.data_as(C.c_void_p), None if ids is None else ids.ctypes.data_as(C.c_void_p), n,
             C.byref(p), depth, out.ctypes.data_as(C.c_void_p)), "rtx_internal_nee_samples")
    return out


NEE_ELIGIBLE, NEE_TRACED, NEE_VISIBLE, NEE_SUPPRESSED = 1, 2, 4, 8  # rtx_internal_nee_trace's flag bits


def nee_trace(scene, rays, spp, max_depth, seed, cap, ids=None, first_sample=0, precision="parity"):
    """Test hook (rtx_internal_nee_trace, not in rtx.h): the paths DeviceScene.radiance_nee traces
    for the same arguments, from the device function its kernel runs.  Returns a dict: "p", "n",
    "w" (n, spp, cap, 3): each segment's vertex point, shading normal and w = throughput x
    reflectance (zero on a miss; w zero where no term is eligible); "flags" (n, spp, cap) uint32
    (NEE_* bits); "L_end" (n, spp, 3); "closest", "shadow" (n, spp) uint32 segment counts.
    Segments a path does not reach are zero."""
    rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
    n = len(rays)
    if ids is not None:
        ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        if len(ids) != n:
            raise ValueError("nee_trace: one id per ray")
    f = lib().rtx_internal_nee_trace
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(RadianceParams), C.c_int32, C.c_void_p,
                  C.c_void_p, C.c_void_p, C.c_void_p]
    f.restype = C.c_int
    p = DeviceScene._radiance_params(spp, max_depth, seed, first_sample, precision)
    verts = np.zeros((n, spp, cap, 9))
    flags = np.zeros((n, spp, cap), np.uint32)
    ends = np.zeros((n, spp, 3))
    counts = np.zeros((n, spp, 2), np.uint32)
    _check(f(scene.h, rays.ctypes.data_as(C.c_void_p), None if ids is None else ids.ctypes.data_as(C.c_void_p), n,
             C.byref(p), cap, verts.ctypes.data_as(C.c_void_p), flags.ctypes.data_as(C.c_void_p),
             ends.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p)), "rtx_internal_nee_trace")
    return {"p": verts[..., 0:3], "n": verts[..., 3:6], "w": verts[..., 6:9], "flags": flags, "L_end": ends,
            "closest": counts[..., 0], "shadow": counts[..., 1]}


MIS_WEIGHTED = 16  # rtx_internal_mis_trace's own flag bit (NEE_SUPPRESSED is never set there)


def mis_trace(scene, rays, spp, max_depth, seed, cap, ids=None, first_sample=0, precision="parity"):
    """Test hook (rtx_internal_mis_trace, not in rtx.h): nee_trace() for the paths of
    DeviceScene.radiance_mis.  The same dict with two more entries: "g" (n, spp, cap), the scalar of
    each vertex's light sample (0 where none was traceable), and "gb" (n, spp, cap), the gb applied
    to the emission of the segment that ended the path there (0 where none applied).  flags:
    NEE_ELIGIBLE / NEE_TRACED / NEE_VISIBLE and MIS_WEIGHTED."""
    rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
    n = len(rays)
    if ids is not None:
        ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        if len(ids) != n:
            raise ValueError("mis_trace: one id per ray")
    f = lib().rtx_internal_mis_trace
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(RadianceParams), C.c_int32, C.c_void_p,
                  C.c_void_p, C.c_void_p, C.c_void_p]
    f.restype = C.c_int
    p = DeviceScene._radiance_params(spp, max_depth, seed, first_sample, precision)
    verts = np.zeros((n, spp, cap, 11))
    flags = np.zeros((n, spp, cap), np.uint32)
    ends = np.zeros((n, spp, 3))
    counts = np.zeros((n, spp, 2), np.uint32)
    _check(f(scene.h, rays.ctypes.data_as(C.c_void_p), None if ids is None else ids.ctypes.data_as(C.c_void_p), n,
             C.byref(p), cap, verts.ctypes.data_as(C.c_void_p), flags.ctypes.data_as(C.c_void_p),
             ends.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p)), "rtx_internal_mis_trace")
    return {"p": verts[..., 0:3], "n": verts[..., 3:6], "w": verts[..., 6:9], "g": verts[..., 9], "gb": verts[..., 10],
            "flags": flags, "L_end": ends, "closest": counts[..., 0], "shadow": counts[..., 1]}


def emitter_table(scene):
    """Test hook (rtx_internal_emitters, not in rtx.h): the live emitter table, (prims, cum): each
    emitter's primitive index (int64, the scene's own order as update_prims counts it) and the
    inclusive cumulative areas (float64), whose last entry is emitters()'s area."""
    n = scene.emitters()[0]
    prims, cum = np.zeros(n, np.int64), np.zeros(n, np.float64)
    f = lib().rtx_internal_emitters
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    f.restype = C.c_int
    _check(f(scene.h, prims.ctypes.data_as(C.c_void_p), cum.ctypes.data_as(C.c_void_p), n), "rtx_internal_emitters")
    return prims, cum


def radiance_chunk(slots=0):
    """Test hook (rtx_internal_radiance_chunk, not in rtx.h): the slot cap (ray x sample) of the
    radiance calls that follow in this process; 0 restores the default.  Results never depend on
    it, only the chunking does."""
    f = lib().rtx_internal_radiance_chunk
    f.argtypes = [C.c_int64]
    f.restype = C.c_int
    _check(f(slots), "rtx_internal_radiance_chunk")


def film_group(first=0, later=0):
    """Test hook (rtx_internal_film_group, not in rtx.h): the samples per pixel of an adaptive sampled
    film's first group (on an empty film) and of its later groups, for the render calls that follow
    in this process; 0 restores the defaults (min_spp, 4).  Results never depend on them."""
    f = lib().rtx_internal_film_group
    f.argtypes = [C.c_int32, C.c_int32]
    f.restype = C.c_int
    _check(f(first, later), "rtx_internal_film_group")


def adapt_tune(phase_slots=0, phase_kcap=0, first_map=-1, phase_mstep=-1.0, margin1=-1.0, pool_w=-1.0):
    """Test / tuning hook (rtx_internal_adapt_tune, not in rtx.h): overrides of the adaptive
    phases' constants for the renders that follow in this process; no argument restores the
    defaults.  Results never depend on them, only the work and the phases do.  phase_slots: the
    smallest phase while pixels remain; phase_kcap: the largest batch of one pixel; first_map:
    the uniform first pass on the phase kernel (1, block-shared chunks) or on the uniform-group
    kernel (0); phase_mstep: the batch margin's growth per phase; margin1: the margin of the
    batches after the first phase; pool_w: the centre weight of the prediction pooled over each
    pixel's 3 x 3 neighbourhood (k_adapt_plan; 0: each pixel's own prediction)."""
    f = lib().rtx_internal_adapt_tune
    f.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double]
    f.restype = C.c_int
    _check(f(phase_slots, phase_kcap, first_map, phase_mstep, margin1, pool_w), "rtx_internal_adapt_tune")


def _pixel_outputs(npix):
    r = {k: np.zeros((npix, 3)) for k in ("sum", "mean", "m2", "rgb")}
    r["samples"], r["conv"], r["spp"] = np.zeros(npix, np.int32), np.zeros(npix, np.uint8), np.zeros(npix, np.int32)
    return r, [r[k].ctypes.data_as(C.c_void_p) for k in ("sum", "mean", "m2", "samples", "conv", "rgb", "spp")]


def adaptive_replay(scene, table, width, min_spp, rel):
    """Test hook (rtx_internal_adaptive_replay, not in rtx.h): the adaptive persistent render's own
    phase loop on a table of radiance samples [npix, budget, 3] instead of traced paths, the
    pixels a grid `width` columns wide (adapt_tune applies).  Returns the pixel statistics (sum,
    mean, m2 [npix, 3], samples, conv), k_resolve's output (rgb, spp) and asked [npix, budget]
    (uint8): how often the phases asked for each (pixel, sample)."""
    table = np.ascontiguousarray(table, dtype=np.float64)
    npix, budget = table.shape[:2]
    assert table.shape == (npix, budget, 3)
    r, ptrs = _pixel_outputs(npix)
    r["asked"] = np.zeros((npix, budget), np.uint8)
    f = lib().rtx_internal_adaptive_replay
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_double] + [C.c_void_p] * 8
    f.restype = C.c_int
    _check(f(scene.h, table.ctypes.data_as(C.c_void_p), npix, width, budget, min_spp, float(rel), *ptrs,
             r["asked"].ctypes.data_as(C.c_void_p)), "rtx_internal_adaptive_replay")
    return r


ACC_KINDS = {"record_adaptive": 0, "record": 1, "sum": 2, "mk_adaptive": 3}


def accumulate_groups(kind, table, groups, min_spp=16, rel=0.05, resolve=-1, bands=1, align=1, device=0):
    """Test hook (rtx_internal_accumulate_groups, not in rtx.h): a table of radiance samples [npix,
    budget, 3] fed in uniform groups of groups[i] samples through the renderer's own accumulate
    launches: "record_adaptive" / "record" k_accumulate with adaptive on / off, "sum"
    k_accumulate_sum (resolve -1: k_resolve afterwards; 0 / 1: the last group resolves, in `bands`
    bands aligned to `align` pixels), "mk_adaptive" AdaptiveSampler(min_spp, budget - 1, rel).
    Returns the pixel statistics as the kernels left them and the resolved output (rgb, spp)."""
    table = np.ascontiguousarray(table, dtype=np.float64)
    npix, budget = table.shape[:2]
    assert table.shape == (npix, budget, 3)
    g = np.ascontiguousarray(groups, dtype=np.int32)
    r, ptrs = _pixel_outputs(npix)
    f = lib().rtx_internal_accumulate_groups
    f.argtypes = [C.c_int, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int64,
                  C.c_int32, C.c_double, C.c_int32] + [C.c_void_p] * 7
    f.restype = C.c_int
    _check(f(device, ACC_KINDS[kind], table.ctypes.data_as(C.c_void_p), npix, budget, g.ctypes.data_as(C.c_void_p),
             len(g), bands, align, min_spp, float(rel), resolve, *ptrs), "rtx_internal_accumulate_groups")
    return r


def early_output_stats():
    """Test hook (rtx_internal_early_output_stats, not in rtx.h): (adaptive renders of this
    process whose output went to the host while phases still ran, pixels the device patched
    into the host framebuffer afterwards)."""
    f = lib().rtx_internal_early_output_stats
    f.argtypes = [C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    f.restype = C.c_int
    a, b = C.c_longlong(), C.c_longlong()
    _check(f(C.byref(a), C.byref(b)), "rtx_internal_early_output_stats")
    return a.value, b.value


def render_multi(scenes, cam, spp, max_depth, seed=1234, adaptive=True, mode="persistent", precision="fast",
                 stripe_rows=8, stripe_index=0, stripe_count=0, out=None, schedule=None, min_spp=16,
                 rel_threshold=float(np.float32(0.05)), samples_per_group=0):
    """One frame over several DeviceScenes (rtx_render_multi): returns the whole-frame
    (H*W, 3) framebuffer, (H*W,) sample counts, aggregate stats, per-scene stats."""
    p = RenderParams()
    p.spp, p.max_depth, p.adaptive = spp, max_depth, int(bool(adaptive))
    p.min_spp, p.rel_threshold, p.seed = min_spp, rel_threshold, seed
    p.mode, p.precision = MODES[mode], PRECISIONS[precision]
    p.flags = SCHEDULE_FLAGS[schedule]
    p.stripe_rows, p.stripe_index, p.stripe_count = stripe_rows, stripe_index, stripe_count
    p.samples_per_group = samples_per_group
    n = len(scenes)
    npix = cam.image_width * cam.image_height
    rgb = out if out is not None else np.zeros((npix, 3))
    sp = np.zeros(npix, np.int32)
    arr = (C.c_void_p * n)(*[s.h.value for s in scenes])
    st, per = Stats(), (Stats * n)()
    _check(lib().rtx_render_multi(arr, n, C.byref(cam), C.byref(p), rgb.ctypes.data_as(C.c_void_p),
                                  sp.ctypes.data_as(C.c_void_p), C.byref(st), per), "rtx_render_multi")
    return rgb, sp, st.as_dict(), [x.as_dict() for x in per]


def encode_p3(scene, rgb, width, height):
    """P3 file bytes of a host framebuffer, encoded on `scene`'s device (rtx_encode_p3)."""
    rgb = np.ascontiguousarray(rgb, dtype=np.float64)
    cap = lib().rtx_p3_max_bytes(width, height)
    buf = C.create_string_buffer(cap)
    n = C.c_size_t()
    _check(lib().rtx_encode_p3(scene.h, rgb.ctypes.data_as(C.c_void_p), width, height, buf, cap, C.byref(n)),
           "rtx_encode_p3")
    return buf.raw[:n.value]


def image_load(path, linear8=False):
    """Image::Load through rtx_image_load: (height, width, 3) uint8 texels (or the 8-bit decode)."""
    w, h = C.c_int32(), C.c_int32()
    _check(lib().rtx_image_load(path.encode(), int(linear8), C.byref(w), C.byref(h), None, 0), "rtx_image_load")
    out = np.zeros((h.value, w.value, 3), np.uint8)
    _check(lib().rtx_image_load(path.encode(), int(linear8), C.byref(w), C.byref(h),
                                out.ctypes.data_as(C.c_void_p), out.nbytes), "rtx_image_load")
    return out


def prim_bounds(prims):
    """Reference BoundingBox of each primitive record (PRIM_DTYPE array) -> (n, 6) float64."""
    prims = np.ascontiguousarray(prims)
    out = np.zeros((len(prims), 6))
    _check(lib().rtx_prim_bounds(prims.ctypes.data_as(C.c_void_p), len(prims), out.ctypes.data_as(C.c_void_p)),
           "rtx_prim_bounds")
    return out


def bvh_build(bounds, device=0, on="gpu"):
    """Binned-SAH BVH over (n, 6) primitive boxes: (nodes NODE_DTYPE, prim_indices uint32).
    on="gpu": rtx_bvh_build (device); on="host": rtx_bvh_build_host (the C++ builder)."""
    bounds = np.ascontiguousarray(bounds, dtype=np.float64).reshape(-1, 6)
    n = len(bounds)
    nodes = np.zeros(max(1, 2 * n), NODE_DTYPE)
    idx = np.zeros(max(1, n), np.uint32)
    nn = C.c_int64()
    bp, np_, ip = bounds.ctypes.data_as(C.c_void_p), nodes.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p)
    if on == "gpu":
        _check(lib().rtx_bvh_build(device, bp, n, np_, C.byref(nn), ip), "rtx_bvh_build")
    else:
        _check(lib().rtx_bvh_build_host(bp, n, np_, C.byref(nn), ip), "rtx_bvh_build_host")
    return nodes[:nn.value], idx[:n]


def bvh_refit(nodes, bounds):
    """Reference-layout nodes (NODE_DTYPE) refit bottom-up over (n, 6) primitive boxes in leaf
    order, topology unchanged (rtx_bvh_refit_host; no device needed).  Returns a new array."""
    nodes = np.ascontiguousarray(nodes, dtype=NODE_DTYPE).copy()
    bounds = np.ascontiguousarray(bounds, dtype=np.float64).reshape(-1, 6)
    _check(lib().rtx_bvh_refit_host(nodes.ctypes.data_as(C.c_void_p), len(nodes), bounds.ctypes.data_as(C.c_void_p),
                                    len(bounds)), "rtx_bvh_refit_host")
    return nodes


def stripe_rows_of(height, stripe_rows, index, count, width=1):
    """Rows owned by stripe `index` (interleaved row stripes), in output order: the library's own
    pixel map (rtx_internal_stripe_rows: subset_pixels + PixelMap::xy, host side, no device)."""
    f = lib().rtx_internal_stripe_rows
    f.argtypes = [C.c_int32] * 5 + [C.c_void_p, C.POINTER(C.c_int64)]
    f.restype = C.c_int
    rows = np.zeros(max(1, height), np.int32)
    n = C.c_int64()
    _check(f(width, height, stripe_rows, index, count, rows.ctypes.data_as(C.c_void_p), C.byref(n)),
           "rtx_internal_stripe_rows")
    return [int(y) for y in rows[:n.value]]


F4NODE_DTYPE = np.dtype([("lox", "<f4", 4), ("hix", "<f4", 4), ("loy", "<f4", 4), ("hiy", "<f4", 4),
                         ("loz", "<f4", 4), ("hiz", "<f4", 4), ("child", "<i4", 4), ("counts", "<u4", 2),
                         ("pad_", "<u4", 2)])
assert F4NODE_DTYPE.itemsize == 128
FAST_TREE_INFO = ("stack_parity", "depth", "fast_ok", "stack_fast", "fast_need", "n_f4", "n_global", "global0",
                  "global1", "tree_kind")


def fast_tree(scene):
    """Test hook (rtx_internal_fast_tree, not in rtx.h): the host-side traversal plan that
    rtx_scene_create makes for a scene, without a device.  scene: a SceneDesc, or anything with
    a .desc() method (a HostScene).  Returns (info dict, F4Node array): stack_parity (-1: deeper
    than 62 levels, rtx_scene_create refuses the scene), depth, fast_ok, stack_fast, fast_need,
    n_f4, n_global, global0, global1, tree_kind, and the fast tree's nodes (F4NODE_DTYPE; layout
    in csrc/rtx_device.h), which exist whenever the reference-layout root is internal."""
    d = scene if isinstance(scene, SceneDesc) else scene.desc()
    f = lib().rtx_internal_fast_tree
    f.argtypes = [C.POINTER(SceneDesc), C.c_void_p, C.c_void_p, C.c_int64]
    f.restype = C.c_int
    info = np.zeros(len(FAST_TREE_INFO), np.int32)
    _check(f(C.byref(d), info.ctypes.data_as(C.c_void_p), None, 0), "rtx_internal_fast_tree")
    nodes = np.zeros(int(info[5]), F4NODE_DTYPE)
    if len(nodes):
        _check(f(C.byref(d), info.ctypes.data_as(C.c_void_p), nodes.ctypes.data_as(C.c_void_p), len(nodes)),
               "rtx_internal_fast_tree")
    return {k: int(v) for k, v in zip(FAST_TREE_INFO, info)}, nodes


def scene_trees(scene):
    """Test hook (rtx_internal_scene_trees, not in rtx.h): the trees a DeviceScene holds on its
    device right now, copied back: (reference-layout nodes NODE_DTYPE, fast nodes F4NODE_DTYPE;
    the latter empty when the scene has no fast tree)."""
    info, _ = fast_tree(scene.host)
    f = lib().rtx_internal_scene_trees
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]
    f.restype = C.c_int
    nodes = np.zeros(int(scene.host.desc().n_nodes), NODE_DTYPE)
    f4 = np.zeros(info["n_f4"] if info["fast_ok"] else 0, F4NODE_DTYPE)
    _check(f(scene.h, nodes.ctypes.data_as(C.c_void_p), len(nodes), f4.ctypes.data_as(C.c_void_p), len(f4)),
           "rtx_internal_scene_trees")
    return nodes, f4


def write_ppm(path, rgb, width, height):
    rgb = np.ascontiguousarray(rgb, dtype=np.float64)
    _check(lib().rtx_write_ppm(path.encode(), rgb.ctypes.data_as(C.c_void_p), width, height), "rtx_write_ppm")
