/* include/rtx.h — C ABI of the MI355X-native path-tracing hot path (lib: librtx.so).
 *
 * This is the drop-in boundary for Luke-TS/3360-ray-tracer's per-pixel Monte Carlo path
 * tracer.  Plain C: POD structs, pointers and sizes, int status codes (RTX_OK == 0) and a
 * thread-local rtx_last_error() string.  No C++, no torch, no HIP types in the signatures.
 *
 * Reference interfaces each entry point replaces (paths under the reference's src/):
 *   rtx_intersect / rtx_intersect_device
 *       RayIntegrator::IntersectBatch(const vector<Ray>&, vector<HitRecord>&)
 *       integrator/ray_integrator.h:30-37; CPU version cpu_ray_integrator.h:18-46
 *       (interval fixed to [0.001f, +inf) there: pass tmin = RTX_SEAM_TMIN).
 *   rtx_render / rtx_render_device
 *       WavefrontRenderer(world, cam, integrator, max_depth, max_samples, batch).Render()
 *       renderer/wavefront.h:22-45, renderer/wavefront.cc:40-242 (mode RTX_MODE_WAVEFRONT);
 *       MegaKernel(scene, camera, DefaultSampler).Render()
 *       renderer/mega_kernel.h:10-59 + integrator/sampler.h:22-34 (mode RTX_MODE_MEGAKERNEL).
 *   rtx_film_* (no counterpart in the reference, whose Render() is one shot)
 *       the same renders in steps: WavefrontRenderer's per-pixel PixelState
 *       (renderer/pixel_state.h) kept between calls, resolved on demand, saved and loaded.
 *   rtx_scene_create
 *       the GPU hooks of the reference: Bvh::nodes()/prim_indices()/primitives() +
 *       BvhNodeGPU (geom/bvh.h:20-25,134-136), HittableType (geom/hittable.h:45-49).
 *   rtx_camera_init
 *       Camera::SetFromConfig + Camera::Initialize (scene/camera.h:84-131).
 *   rtx_host_scene_* (host-side scene assembly, no GPU work)
 *       scene::Scene::Add (scene/scene.h:26-33), geom::Bvh(Scene&) SAH build
 *       (geom/bvh.h:31-68,166-367), load_obj (load_obj.h:10-55), main.cc scene recipes.
 *
 * Ownership: the library copies everything it needs; it never retains caller pointers
 * past the call.  Output buffers are caller-allocated.
 * Threading: one rtx_scene per device; calls on different scenes (devices) may run
 * concurrently from different host threads; calls on one scene are serialised by the
 * caller.  Errors: every function returns RTX_OK or a negative RTX_ERR_*; the message is
 * in rtx_last_error() (thread-local).  HIP failures are reported, never swallowed; there
 * is no CPU fallback.
 */
#ifndef RTX_H_
#define RTX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTX_ABI_VERSION 9  /* 2: rtx_stats.node_bytes; 3: rtx_stats.parked, RTX_FLAG_PARK / NO_PARK;
                              4: rtx_stats.build, RTX_FLAG_GENERIC, rtx_render_multi;
                              5: RTX_FLAG_LEAF_STEP, RTX_BUILD_SPECULATIVE; 6: rtx_stats.rays_recorded;
                              7: RTX_FLAG_ADAPT_PHASES (the adaptive tile schedule is the default),
                              rtx_stats.wave_rounds / wave_rounds_idle;
                              8: RTX_FLAG_ADAPT_TILES (the phase schedule is the default again);
                              9: the tile schedule removed (flag bit 64 reserved, ignored) */

enum {
  RTX_OK = 0,
  RTX_ERR_INVALID = -1, /* bad argument / descriptor */
  RTX_ERR_HIP = -2,     /* HIP runtime or kernel failure */
  RTX_ERR_NODEVICE = -3,
  RTX_ERR_IO = -4,      /* file not found / parse error (host scene helpers) */
  RTX_ERR_NOMEM = -5
};

/* IntersectBatch's interval minimum: float(0.001) as a double (cpu_ray_integrator.h:21). */
#define RTX_SEAM_TMIN 0.0010000000474974513

/* ---- scene description (host memory, flattened) ---------------------------------- */

/* BvhNodeGPU (geom/bvh.h:20-25): bbox in double, pre-order layout (left child = idx+1). */
typedef struct {
  double lo[3], hi[3];
  uint32_t left_first;  /* internal: left child index; leaf: first primitive (leaf order) */
  uint32_t right_count; /* internal: right child index; leaf: primitive count */
  uint32_t is_leaf;
  uint32_t pad_;
} rtx_bvh_node; /* 64 bytes */

enum { /* HittableType (geom/hittable.h:45-49) split per rect axis */
  RTX_PRIM_SPHERE = 0,   /* g: center[3], radius                  (geom/sphere.h) */
  RTX_PRIM_TRIANGLE = 1, /* g: a[3], b[3], c[3]                   (geom/triangle.h) */
  RTX_PRIM_XY_RECT = 2,  /* g: x0 x1 y0 y1 k                      (geom/rect.h:9-47) */
  RTX_PRIM_XZ_RECT = 3,  /* g: x0 x1 z0 z1 k                      (geom/rect.h:53-91) */
  RTX_PRIM_YZ_RECT = 4   /* g: y0 y1 z0 z1 k                      (geom/rect.h:97-135) */
};
typedef struct {
  int32_t kind;
  int32_t material;
  double g[9];
} rtx_prim; /* 80 bytes */

enum { RTX_TEX_SOLID = 0, RTX_TEX_CHECKER = 1, RTX_TEX_IMAGE = 2 }; /* material/texture.h */
typedef struct {
  int32_t kind;
  int32_t even, odd; /* checker children (texture ids) */
  int32_t image;     /* image id for RTX_TEX_IMAGE; -1 = no data (cyan, texture.h:62) */
  double color[3];   /* solid */
  double inv_scale;  /* checker: 1/scale */
} rtx_texture;

typedef struct {
  int32_t width, height;
  const uint8_t* texels; /* RGB8 after Image::FloatToByte (scene/image.cc:43-73), rows top-down */
} rtx_image;

enum { /* material/material.h */
  RTX_MAT_LAMBERTIAN = 0,
  RTX_MAT_METAL = 1,
  RTX_MAT_DIELECTRIC = 2,
  RTX_MAT_DIFFUSE_LIGHT = 3
};
typedef struct {
  int32_t kind;
  int32_t texture;  /* lambertian albedo / diffuse-light emission */
  double albedo[3]; /* metal */
  double fuzz;      /* metal, already clamped to <= 1 (material.cc:78-80) */
  double ref_idx;   /* dielectric */
} rtx_material;

typedef struct {
  const rtx_prim* prims; /* in BVH leaf order when nodes != NULL, else list order */
  int64_t n_prims;
  const rtx_bvh_node* nodes; /* NULL: the root is a flat list (scene::Scene::Hit) */
  int64_t n_nodes;
  const rtx_material* materials;
  int32_t n_materials;
  const rtx_texture* textures;
  int32_t n_textures;
  const rtx_image* images;
  int32_t n_images;
} rtx_scene_desc;

typedef struct rtx_scene rtx_scene; /* device-resident scene, one per device */

/* ---- rays and hit records (IntersectBatch seam) ----------------------------------- */

typedef struct {
  double origin[3];
  double direction[3]; /* not normalised (ray.h) */
} rtx_ray;             /* 48 bytes, = core::Ray */

typedef struct {
  int32_t hit;
  int32_t front_face;
  int32_t material; /* replaces HitRecord::mat (shared_ptr): index into the material table */
  int32_t pad_;
  double t;
  double p[3];
  double normal[3]; /* faces against the ray (hittable.h:31-34) */
  double u, v;      /* triangles do not write u,v (triangle.h:77-84): 0 unless stale */
} rtx_hit;          /* 88 bytes, = geom::HitRecord */

/* ---- camera ------------------------------------------------------------------------ */

typedef struct { /* CameraConfig (scene/camera.h:25-38) */
  double aspect_ratio;
  int32_t image_width;
  int32_t samples_per_pixel;
  int32_t max_depth;
  int32_t pad_;
  double vfov;
  double lookfrom[3], lookat[3], vup[3];
  double defocus_angle;
  double focus_dist;
} rtx_camera_config;

typedef struct { /* Camera after Initialize() (scene/camera.h:100-131) */
  double center[3], pixel00[3], pixel_delta_u[3], pixel_delta_v[3];
  double u[3], v[3], w[3];
  double defocus_disk_u[3], defocus_disk_v[3];
  double defocus_angle;
  int32_t image_width, image_height;
} rtx_camera;

/* ---- rendering --------------------------------------------------------------------- */

enum {
  RTX_MODE_WAVEFRONT = 0,  /* WavefrontRenderer semantics, bounce-synchronous queues */
  RTX_MODE_PERSISTENT = 1, /* same semantics, persistent kernel with per-lane refill */
  RTX_MODE_MEGAKERNEL = 2  /* MegaKernel + DefaultSampler semantics (Scatter API) */
};
enum {
  RTX_PREC_PARITY = 0, /* f64 everywhere, reference traversal order (bvh.h:71-119) */
  RTX_PREC_FAST = 1    /* conservative f32 traversal, near-child first; f64 hit + shading */
};

typedef struct {
  int32_t spp;              /* max_samples (passes) */
  int32_t max_depth;
  int32_t adaptive;         /* 1: adaptive sampling.  WAVEFRONT/PERSISTENT: the renderer's
                               PixelState test (pixel_state.h:54-72); MEGAKERNEL:
                               AdaptiveSampler(min_spp, spp, rel_threshold) (sampler.h:44-82,
                               up to spp + 1 samples); 0: fixed spp / DefaultSampler */
  int32_t min_spp;          /* adaptive: kMinSamples (wavefront.cc:43) = 16 | min_samples_ */
  double rel_threshold;     /* adaptive: kRelThresh (float 0.05, wavefront.cc:42) | threshold_ */
  uint64_t seed;            /* Philox key: results depend on (seed, pixel, sample) only */
  int32_t mode;             /* RTX_MODE_* */
  int32_t precision;        /* RTX_PREC_* */
  /* pixel subset: interleaved row stripes (stripe_rows > 0) or a rectangle */
  int32_t stripe_rows, stripe_index, stripe_count;
  int32_t x0, y0, w, h;     /* rectangle (w == 0 -> whole image) */
  int32_t samples_per_group;/* samples in flight per pixel (0 = auto) */
  int32_t flags;            /* RTX_FLAG_* */
} rtx_render_params;

enum {
  RTX_FLAG_COUNT = 1,  /* count BVH node visits / primitive tests (diagnostic build of the kernel) */
  /* RTX_MODE_PERSISTENT + RTX_PREC_FAST schedule (results are identical either way): by
     default the first such render of a scene times both on a centre tile and keeps the
     faster for the scene; these flags force one */
  RTX_FLAG_PARK = 2,   /* park long traversals and resume them in the next segment round */
  RTX_FLAG_NO_PARK = 4, /* every traversal runs to completion within its round */
  /* RTX_MODE_PERSISTENT: run the generic kernel build, without the per-scene
     specialisations (same results; for measuring what the specialisations buy) */
  RTX_FLAG_GENERIC = 8,
  /* the PARK schedule's traversal: the speculative walk (queued leaf tests) by default on
     trees of at most 65536 BVH4 nodes, the leaf-step walk on larger ones; this flag asks for
     the leaf-step walk on every tree (same results) */
  RTX_FLAG_LEAF_STEP = 16,
  /* RTX_MODE_PERSISTENT adaptive renders (samples_per_group 0): one launch per phase over a
     device-wide slot map (the default; this flag names it explicitly) */
  RTX_FLAG_ADAPT_PHASES = 32
  /* 64: reserved (ABI <= 8: the adaptive tile schedule, removed; ignored) */
};

/* rtx_stats.build: which persistent-kernel build ran (the per-scene specialisations compile
   out code paths the scene cannot reach; every build gives identical results) */
enum {
  RTX_BUILD_PARK = 1,           /* parked-traversal schedule */
  RTX_BUILD_SPHERE_TREE = 2,    /* leaf tests for spheres only (every tree primitive a sphere) */
  RTX_BUILD_TRIANGLE_TREE = 4,  /* leaf tests for triangles only */
  RTX_BUILD_LAMBERTIAN = 8,     /* shading for Lambertian materials only */
  RTX_BUILD_NO_TEXTURES = 16,   /* no texture lookups (every colour in the material table) */
  RTX_BUILD_NO_DEFOCUS = 32,    /* no thin-lens camera sampling (defocus_angle <= 0) */
  RTX_BUILD_FAST = 64,          /* RTX_PREC_FAST traversal */
  RTX_BUILD_COUNT = 128,        /* diagnostic counting build */
  RTX_BUILD_SCATTER = 256,      /* MegaKernel (Scatter API) semantics */
  RTX_BUILD_SPECULATIVE = 512   /* PARK schedule with the speculative walk (else the leaf-step walk) */
};

typedef struct {
  uint64_t rays_primary;   /* segments at depth 0 */
  uint64_t rays_total;     /* all segments handed to closest-hit (= IntersectBatch count) */
  uint64_t paths;          /* samples recorded */
  double kernel_ms;        /* device time of the render (HIP events) */
  double hot_kernel_ms;    /* device time inside the dominant (trace) kernel */
  uint64_t hot_launches;
  uint64_t node_visits;    /* with RTX_FLAG_COUNT */
  uint64_t prim_tests;     /* with RTX_FLAG_COUNT */
  uint64_t node_bytes;     /* bytes of one BVH node visit in the traversal used (64 BVH2, 128 BVH4) */
  uint64_t wave_node_iters; /* with RTX_FLAG_COUNT, fast BVH4: node-loop iterations per wave (SIMD efficiency */
  uint64_t wave_prim_iters; /*   = node_visits / (64 * wave_node_iters)); primitive-loop iterations per wave */
  uint64_t tri_tests;       /* with RTX_FLAG_COUNT: triangle / sphere tests among prim_tests (rest: rects) */
  uint64_t sphere_tests;
  uint64_t parked;          /* 1: the persistent fast schedule that parks long traversals ran */
  uint64_t build;           /* RTX_BUILD_* bits of the persistent kernel build (0: wavefront mode) */
  uint64_t rays_recorded;   /* with RTX_FLAG_COUNT: segments of the samples the pixels recorded.  Fixed spp:
                               = rays_total.  Adaptive RTX_MODE_PERSISTENT renders with automatic grouping
                               (samples_per_group 0; the tile or phase schedule) trace some samples past a
                               pixel's convergence and discard them: counted per sample.  Other adaptive
                               renders (wavefront, megakernel, explicit samples_per_group): 0 (not
                               counted).  0 without RTX_FLAG_COUNT */
  uint64_t wave_rounds;      /* with RTX_FLAG_COUNT, persistent mode: rounds of the waves' loop (refill,
                                segment), and those in which a wave had no path to trace (waiting for work) */
  uint64_t wave_rounds_idle;
  uint64_t wave_lanes_live;  /* with RTX_FLAG_COUNT, persistent mode: lanes holding a path, summed over the
                                rounds that trace (/ (64 x tracing rounds) = the rounds' lane occupancy) */
} rtx_stats;

/* ---- entry points ------------------------------------------------------------------ */

int rtx_abi_version(void);
const char* rtx_last_error(void);
int rtx_device_count(int* n);

int rtx_scene_create(int device, const rtx_scene_desc* desc, rtx_scene** out);
int rtx_scene_destroy(rtx_scene* scene);

/* ---- in-place updates of a live scene (DESIGN.md "Scene updates") ---------------------------
 * Move or reshape primitives without re-creating the scene: the records are rewritten and both
 * trees refit bottom-up over their unchanged topology, on the device.  The refit trees hold the
 * bytes the host builders give for that topology, so hits and renders equal those of a scene
 * created from the new primitives (apart from exact t ties, which depend on the topology).
 * Primitive count, kinds, materials' table and textures stay; stack sizes and the persistent
 * fast schedule are kept.  Tree quality degrades as geometry drifts from what the build saw:
 * re-create the scene then. */
/* Replace primitives [first, first + count) of the scene, in the scene's own order (leaf order
 * when it has a BVH), and refit both trees over the unchanged topology.  prims[i].kind must equal
 * the kind the scene holds at first + i; material may change (range-checked); geometry must be
 * finite.  Checked on the host before any device work; on failure the scene is unchanged.
 * count == 0: RTX_OK, nothing happens; a range outside the scene: RTX_ERR_INVALID. */
int rtx_scene_update_prims(rtx_scene* scene, int64_t first, int64_t count, const rtx_prim* prims);
/* Geometry only, from device memory: count x 9 doubles (rtx_prim.g), kinds and materials kept.
 * Asynchronous on stream (NULL = the scene's stream).  Finite geometry is the caller's duty. */
int rtx_scene_update_geometry_device(rtx_scene* scene, int64_t first, int64_t count, const double* d_g, void* stream);
/* Updates applied to the scene so far (0 after rtx_scene_create). */
int rtx_scene_epoch(const rtx_scene* scene, int64_t* epoch);
/* Host-only: refit reference-layout nodes over n primitive boxes (n x 6 doubles, leaf order):
 * leaves take the union of their primitives' boxes, internal nodes of their children.  Nodes
 * must be pre-order (children after their parent) with leaf ranges inside n. */
int rtx_bvh_refit_host(rtx_bvh_node* nodes, int64_t n_nodes, const double* bounds, int64_t n);

/* Batch closest hit on [tmin, tmax); host buffers (PCIe round trip included).  tmin may be
 * negative (hits behind the origin are then reported, as the reference's Interval(tmin, tmax)
 * does); the fast walk clamps box entry distances at 0, so a query with tmin < 0 (or an empty
 * range, tmin >= tmax) runs the parity walk whatever precision it names.  In a fast query a single
 * ray takes the parity walk where the reference's f64 box test and the conservative f32 one part: a
 * direction component that is NaN or nonzero outside 2^-126 .. 2^126 in magnitude, an origin
 * component beyond 2^126 or NaN, or an axis-parallel ray that touches the primitive it hits in (or
 * outside) a face plane of that primitive's box, where the reference rejects the box (0 * inf).  The
 * query then reports what the reference does.  The same holds for rtx_occluded*. */
int rtx_intersect(rtx_scene* scene, const rtx_ray* rays, size_t n, rtx_hit* hits, double tmin, double tmax,
                  int32_t precision);
/* Same on device-resident buffers; stream is a hipStream_t (NULL = the scene's stream). */
int rtx_intersect_device(rtx_scene* scene, const rtx_ray* d_rays, size_t n, rtx_hit* d_hits, double tmin,
                         double tmax, int32_t precision, void* stream);

/* ---- occlusion (any-hit) queries (DESIGN.md "Occlusion queries and the AO pass") -------------
 * Shadow, visibility and line-of-sight rays need one bit: is anything in the way?  The walk stops
 * at the first primitive whose own test accepts the ray, keeps no closest distance, builds no
 * record and writes one byte per ray. */
/* 1 per ray if any primitive is hit on (tmin, tmax), else 0; equals rtx_intersect's hit flag for
   the same arguments.  Directions are not normalised, so a segment a->b is origin a, direction
   b - a, tmax 1.  tmin >= tmax (or a NaN) is RTX_ERR_INVALID.  Host buffers. */
int rtx_occluded(rtx_scene* scene, const rtx_ray* rays, size_t n, uint8_t* out, double tmin, double tmax,
                 int32_t precision);
/* Device buffers; asynchronous on stream (NULL = the scene's stream). */
int rtx_occluded_device(rtx_scene* scene, const rtx_ray* d_rays, size_t n, uint8_t* d_out, double tmin, double tmax,
                        int32_t precision, void* stream);

int rtx_camera_init(const rtx_camera_config* cfg, rtx_camera* out);

/* Render the pixel subset selected by params.  out_rgb: linear sum/(float)samples, double,
 * 3 per pixel, packed in subset order (rectangle row-major, or stripes in row order);
 * out_spp: samples per pixel (may be NULL).  Host buffers. */
int rtx_render(rtx_scene* scene, const rtx_camera* cam, const rtx_render_params* params, double* out_rgb,
               int32_t* out_spp, rtx_stats* stats);
/* Number of pixels rtx_render writes for these params. */
int64_t rtx_render_pixel_count(const rtx_camera* cam, const rtx_render_params* params);
/* Device-resident variant: out buffers are device pointers; asynchronous on stream. */
int rtx_render_device(rtx_scene* scene, const rtx_camera* cam, const rtx_render_params* params,
                      double* d_out_rgb, int32_t* d_out_spp, rtx_stats* stats, void* stream);

/* One frame over several devices: the image's rows are split into interleaved
 * stripes of params->stripe_rows rows (0: 8), and scenes[k] renders stripe
 * params->stripe_index + k of params->stripe_count (stripe_count <= 0: n stripes, from 0), each
 * from its own host thread on its scene's stream.  The stripes come back to the host and are
 * placed at their rows of out_rgb (W x H x 3, the whole frame; a pinned buffer receives them by
 * DMA, a pageable one through pinned staging) and out_spp (W x H, may be NULL); rows of other
 * stripes are not written, so several processes may fill one shared framebuffer.  Replaces
 * WavefrontRenderer::Render()'s one framebuffer (renderer/wavefront.cc:228-241) for G GPUs.
 * One scene per device is the intended use (rtx_scene_create on each; the same description);
 * a scene may not appear twice.  The RNG is keyed by the global pixel, so the image is
 * bit-identical for every n and split.  stats: counters summed, times = max over scenes;
 * per_scene (n entries) may be NULL. */
int rtx_render_multi(rtx_scene* const* scenes, int32_t n, const rtx_camera* cam, const rtx_render_params* params,
                     double* out_rgb, int32_t* out_spp, rtx_stats* stats, rtx_stats* per_scene);

/* ---- host-side scene assembly (C++ host library, no GPU) --------------------------- */

typedef struct rtx_host_scene rtx_host_scene;
/* Parse a .rtxs scene file (see DESIGN.md "Scene files"); image/obj paths relative to asset_dir. */
int rtx_host_scene_load(const char* path, const char* asset_dir, rtx_host_scene** out);
/* Build one of the reference's scene recipes: three, cornell, final, bunny, mixed (seeded). */
int rtx_host_scene_recipe(const char* name, uint32_t seed, const char* asset_dir, rtx_host_scene** out);
int rtx_host_scene_write(const rtx_host_scene* s, const char* path);
/* Flattened description; pointers stay valid until rtx_host_scene_destroy. */
int rtx_host_scene_desc(const rtx_host_scene* s, rtx_scene_desc* out);
/* prim_indices (Bvh::prim_indices, bvh.h:135) of the SAH build; n = n_prims. */
int rtx_host_scene_prim_indices(const rtx_host_scene* s, int32_t* out, int64_t n);
int rtx_host_scene_destroy(rtx_host_scene* s);

/* Image::Load (scene/image.cc:16-73; stb_image's stbi_loadf + FloatToByte): decode an image
   file — JPEG (sequential or progressive, 8-bit, 1/3/4 components) or binary PNM (P5/P6) — to
   the RGB8 texels image textures sample (width * height * 3 bytes, rows top-down).
   linear8 = 1: the 8-bit decode before the gamma-2.2 / FloatToByte step (stbi_load's bytes).
   texels == NULL: only *width / *height.  RTX_ERR_IO for an unreadable or unsupported file. */
int rtx_image_load(const char* path, int32_t linear8, int32_t* width, int32_t* height, uint8_t* texels,
                   size_t cap);

/* cameras.json preset -> config (parseCamera/loadCameras, scene/camera.h:40-67). */
int rtx_camera_config_load(const char* json_path, const char* preset, rtx_camera_config* out);

/* ---- BVH build (SURVEY §8f "GPU BVH build"; bvh.h:39-68,166-367) -------------------- */
/* Reference BoundingBox of each primitive (n x 6 doubles: lo xyz, hi xyz), host-side. */
int rtx_prim_bounds(const rtx_prim* prims, int64_t n, double* out_bounds);
/* Binned-SAH BVH over n primitive boxes (in the primitives' original order), built on the
   GPU.  Output is byte-identical to the host builder's (= the reference's Bvh::Build):
   out_nodes (capacity 2n) in pre-order, *out_n_nodes, out_prim_indices[n] (the permutation:
   leaf slot -> original primitive).  Host buffers; the device work is internal.
   All 6n bounds must be finite: a NaN or infinite bound is refused on the host, before any
   device call, with RTX_ERR_INVALID and a message naming the first such box (any finite value
   is fine, e.g. lo = -1.7e308, hi = 1.7e308).  lo <= hi is not required.  SAH bins are
   trunc((c - mn) / extent * 16) clamped to [0, 15]; where a centroid extent below 2^-1024 makes
   that product infinite or NaN, the bin is 0 (what the reference's x86 build computes). */
int rtx_bvh_build(int device, const double* bounds, int64_t n, rtx_bvh_node* out_nodes, int64_t* out_n_nodes,
                  uint32_t* out_prim_indices);
/* The same build on the host (the C++ builder scene assembly uses); identical outputs, and the
   same refusal of non-finite bounds. */
int rtx_bvh_build_host(const double* bounds, int64_t n, rtx_bvh_node* out_nodes, int64_t* out_n_nodes,
                       uint32_t* out_prim_indices);

/* ---- P3 PPM output encoded on the device (wavefront.cc:238-241 header + write_color,
 * core/color.h:18-33, per pixel; SURVEY §8f "on-GPU resolve + PPM output").  The bytes are
 * identical to rtx_write_ppm / the reference's Render() output. */
/* Upper bound of the P3 file size of a width x height image (header + 12 B per pixel). */
size_t rtx_p3_max_bytes(int32_t width, int32_t height);
/* Render like rtx_render and return the P3 file bytes of the rendered pixels (the tile /
   stripe subset: width x rows) in `out` (host, cap >= rtx_p3_max_bytes); *out_len = bytes.
   out_rgb (linear framebuffer) and out_spp are optional (NULL). */
int rtx_render_p3(rtx_scene* scene, const rtx_camera* cam, const rtx_render_params* params, char* out, size_t cap,
                  size_t* out_len, double* out_rgb, int32_t* out_spp, rtx_stats* stats);
/* P3 file bytes of a device-resident linear framebuffer (width x height x 3 doubles) into a
   device buffer d_out (cap >= rtx_p3_max_bytes); synchronizes `stream` to report *out_len. */
int rtx_encode_p3_device(rtx_scene* scene, const double* d_rgb, int32_t width, int32_t height, char* d_out,
                         size_t cap, size_t* out_len, void* stream);

/* P3 file bytes of a host linear framebuffer (width x height x 3 doubles), encoded on the
   scene's device (e.g. the gathered frame of rtx_render_multi); out: host, cap >=
   rtx_p3_max_bytes. */
int rtx_encode_p3(rtx_scene* scene, const double* rgb, int32_t width, int32_t height, char* out, size_t cap,
                  size_t* out_len);

/* ---- films: a frame rendered in steps (progressive preview, checkpoint / resume) ------------
 * A film is the per-pixel render state (sum, mean, M2, samples, converged) of one frame, kept on
 * the scene's device between calls.  rtx_render* starts that state, traces every sample and
 * throws it away; a film keeps it, so a frame can be shown after a few samples and refined,
 * stopped on a budget, extended later, or saved and continued in another process.  After
 * rtx_film_render(film, b) the film is bit for bit what the one-shot render of the same
 * parameters at spp = b holds, however the samples were split over calls (the RNG is keyed by
 * (seed, pixel, sample) and every pixel records its samples in order).
 * The scene lends its scratch (radiance slots, queues, the adaptive workspace); the film owns
 * only the pixel state.  Films of one scene and the scene's own renders may alternate freely;
 * like them, calls on one scene's films are serialised by the caller.  Destroying a scene
 * frees its films' device memory: they stay valid handles for rtx_film_samples and
 * rtx_film_destroy only, every other call returns RTX_ERR_INVALID. */
typedef struct rtx_film rtx_film;
/* A film over the pixel subset of params (rectangle or stripes) with its seed, max_depth, mode,
 * precision, flags, samples_per_group, adaptive, min_spp and rel_threshold; params->spp is
 * ignored.  RTX_MODE_MEGAKERNEL with adaptive is RTX_ERR_INVALID (AdaptiveSampler's spp + 1
 * budget does not compose across calls). */
int rtx_film_create(rtx_scene* scene, const rtx_camera* cam, const rtx_render_params* params, rtx_film** out);
/* A film of the light-sampling estimators (DESIGN.md "Sampled films"): estimator RTX_ESTIMATOR_NEE
 * is the frame of rtx_render_nee kept as a film, RTX_ESTIMATOR_MIS that of rtx_render_mis.  Of params
 * it reads max_depth, adaptive, min_spp, rel_threshold, seed, precision and the tile and stripe
 * fields; spp, mode, flags and samples_per_group are ignored.  adaptive 0: after
 * rtx_film_render(film, b) the film resolves to rtx_render_nee / rtx_render_mis at spp = b bit for
 * bit, however the budget was split over calls.  adaptive != 0: every pixel records its samples in
 * order with RecordSample / IsConverged (the renderer's adaptive sampling), tested after every sample
 * from min_spp on, and stops at its first converged sample or at the budget.  Checks, in this order:
 * NULL arguments, "bad estimator", negative max_depth, max_depth above 16777215 ("nee:" / "mis:"),
 * bad precision, the pixel subset.  Every other rtx_film_* call works on such a film as on a plain
 * one; its blob carries sampler 2 (NEE) or 3 (MIS) and loads only into a film of the same estimator.
 * rtx_stats of a render: paths = rays_primary = samples traced, rays_total = closest-hit plus
 * shadow segments traced, rays_recorded = those of the samples the pixels recorded (fixed:
 * = rays_total), kernel_ms, hot_kernel_ms / hot_launches of the path kernel; the rest 0. */
enum { RTX_ESTIMATOR_NEE = 1, RTX_ESTIMATOR_MIS = 2 };
int rtx_film_create_sampled(rtx_scene* scene, const rtx_camera* cam, const rtx_render_params* params,
                            int32_t estimator, rtx_film** out);
int rtx_film_destroy(rtx_film* film);
/* Advance the film to `budget` samples: fixed sampling traces samples [done, budget) of every
 * pixel; adaptive sampling continues every pixel that has not converged up to budget (the first
 * call in phases, later ones in uniform groups).  budget <= done: nothing, RTX_OK.  stats (may be
 * NULL: then the call does not wait for the device) covers this call only. */
int rtx_film_render(rtx_film* film, int32_t budget, rtx_stats* stats);
int rtx_film_samples(const rtx_film* film, int32_t* done);
/* A film remembers the scene's epoch (rtx_scene_epoch) it was created or last reset at; once the
 * scene was updated, every film call except rtx_film_samples, rtx_film_destroy and this one
 * returns RTX_ERR_INVALID ("scene changed since the film was created").
 * Zero a film's pixel state and bind it to the scene's current epoch (drops its cached AOVs). */
int rtx_film_reset(rtx_film* film);
/* The film's output at its current budget, as rtx_render gives it (out_rgb 3 doubles per pixel
 * in subset order, out_spp may be NULL).  Host buffers. */
int rtx_film_resolve(rtx_film* film, double* out_rgb, int32_t* out_spp);
/* Device buffers; stream is a hipStream_t (NULL = the scene's stream). */
int rtx_film_resolve_device(rtx_film* film, double* d_out_rgb, int32_t* d_out_spp, void* stream);
/* P3 file bytes of the film's output (device encoder, as rtx_render_p3); cap >= rtx_p3_max_bytes
 * of the subset's width x rows. */
int rtx_film_p3(rtx_film* film, char* out, size_t cap, size_t* out_len);
/* Save / load: a host blob of rtx_film_state_bytes bytes, a little-endian header and the state
 * arrays (layout: DESIGN.md "Film").  Load refuses (RTX_ERR_INVALID, the message names the
 * field; the film is unchanged) a blob that is truncated or whose image size, pixel map, seed,
 * max_depth, sampling parameters or sampler family differ from the film's. */
size_t rtx_film_state_bytes(const rtx_film* film);
int rtx_film_save(const rtx_film* film, void* blob, size_t cap, size_t* len);
int rtx_film_load(rtx_film* film, const void* blob, size_t len);
/* Header and length of a blob; host only, no device needed. */
int rtx_film_blob_check(const void* blob, size_t len);

/* ---- first-hit AOVs and the denoiser (DESIGN.md "AOVs and the denoiser") ----------------------
 * The geometry under each pixel, and an edge-avoiding a-trous wavelet filter guided by it, for
 * frames shown at a few samples per pixel.  Nothing here changes a render's own result. */
/* The AOVs of the pixel subset of params, in subset order like rtx_render, from the ray through
 * each pixel's centre (origin cam->center, no lens sampling, no jitter): albedo (3 doubles per
 * pixel: a Lambertian's texture value at the hit, a metal's albedo, 1 1 1 for dielectrics,
 * lights and misses), normal (3: the hit record's, facing against the ray; 0 0 0 on a miss) and
 * depth (1: t of the hit, 0 on a miss).  Only the pixel subset and `precision` of params are
 * read.  Specular paths are not followed to a diffuse hit.  Any output may be NULL. */
int rtx_aov(rtx_scene* scene, const rtx_camera* cam, const rtx_render_params* params, double* albedo,
            double* normal, double* depth);
/* Device buffers; stream is a hipStream_t (NULL = the scene's stream). */
int rtx_aov_device(rtx_scene* scene, const rtx_camera* cam, const rtx_render_params* params, double* d_albedo,
                   double* d_normal, double* d_depth, void* stream);

/* Ambient occlusion of the pixel subset of params (only the subset and `precision` are read), one
 * double per pixel in subset order: from the first hit of the ray through the pixel's centre (the
 * ray of rtx_aov), `samples` any-hit rays in unit cosine-weighted directions about the hit
 * record's normal, each on (RTX_SEAM_TMIN, radius); out = unoccluded / samples, 1.0 where the
 * pixel's ray misses.  One fused kernel: no ray goes through memory.  The directions come from a
 * Philox stream of their own keyed by (seed, global pixel, sample), so a pixel's value does not
 * depend on the subset.  samples outside 1..1024 or radius <= 0: RTX_ERR_INVALID. */
typedef struct {
  int32_t samples; /* 1..1024 */
  int32_t pad_;
  double radius;   /* > 0: the far end of every sample ray (directions are unit vectors) */
  uint64_t seed;
} rtx_ao_params;   /* 24 bytes */
int rtx_ao(rtx_scene* scene, const rtx_camera* cam, const rtx_render_params* params, const rtx_ao_params* ao,
           double* out);
/* Device buffer; asynchronous on stream (NULL = the scene's stream). */
int rtx_ao_device(rtx_scene* scene, const rtx_camera* cam, const rtx_render_params* params, const rtx_ao_params* ao,
                  double* d_out, void* stream);

/* ---- radiance queries (DESIGN.md "Radiance queries") -----------------------------------------
 * How much light arrives along these rays?  The bounce loop of rtx_render (RTX_MODE_WAVEFRONT
 * semantics, fixed sampling) started from rays the caller supplies instead of the built-in
 * camera: for ray i and sample k in [0, spp) a path starts with rays[i] as its depth-0 segment
 * and throughput 1; its random numbers are keyed by (seed, pixel = ids ? ids[i] : (uint32_t)i,
 * sample = first_sample + k), segment d shading from stream d + 1 (stream 0, the camera's, is
 * never opened).  Every segment takes the closest hit on (RTX_SEAM_TMIN, +inf), with the walk
 * rtx_intersect_device picks for `precision`; paths end as a render's do (sky on a miss, emitters,
 * absorption, max_depth, Russian roulette past depth 5).  So from the primary rays of a pixel, its
 * global index and the sample indices, the query returns exactly what rtx_render accumulates.
 * out_rgb: 3 doubles per ray, the in-order sum of the spp radiances times 1 / (double)(float)spp
 * (the fixed-spp resolve).  out_segments (may be NULL): segments traced for the ray over all its
 * samples.  The live scene is read (after rtx_scene_update_* the new geometry); no film is
 * involved.  Non-finite rays are the caller's duty.  One call at a time per scene. */
typedef struct {
  int32_t spp;          /* samples per ray, >= 1 */
  int32_t max_depth;    /* as rtx_render_params.max_depth (>= 0) */
  int32_t first_sample; /* RNG sample index of the first sample, >= 0; first_sample + spp must fit int32 */
  int32_t precision;    /* RTX_PREC_* */
  uint64_t seed;
} rtx_radiance_params;  /* 24 bytes */
/* Host buffers, staged through pinned memory; returns when out_rgb / out_segments are written. */
int rtx_radiance(rtx_scene* scene, const rtx_ray* rays, const uint32_t* ids, size_t n,
                 const rtx_radiance_params* params, double* out_rgb, uint32_t* out_segments);
/* Device buffers; asynchronous on stream (NULL = the scene's stream). */
int rtx_radiance_device(rtx_scene* scene, const rtx_ray* d_rays, const uint32_t* d_ids, size_t n,
                        const rtx_radiance_params* params, double* d_out_rgb, uint32_t* d_out_segments,
                        void* stream);

/* ---- irradiance queries (DESIGN.md "Irradiance queries") -------------------------------------
 * How much light arrives at these surface points?  The fused, ray-free consumer of the radiance
 * query, for light probes, lightmap texels and per-vertex irradiance.  A surfel is an rtx_ray:
 * `origin` is the point, `direction` the surface normal (any positive finite length: it is
 * normalised on the device).  rtx_radiance_params is read as by rtx_radiance, spp being the
 * samples per point.  For surfel i and sample k in [0, spp):
 *   direction: a unit cosine-weighted vector about normalize(normal), made by the operations of
 *     the AO pass's sample directions, from a Philox stream of its own keyed by (seed,
 *     pixel = ids ? ids[i] : (uint32_t)i, sample = first_sample + k);
 *   path: the ray (point, direction) is the depth-0 segment of a path with throughput 1, traced
 *     and shaded exactly as rtx_radiance does (closest hit on (RTX_SEAM_TMIN, +inf) with the walk
 *     of `precision`, segment d shading from stream d + 1 of the same key).
 * So sample k of surfel i is, bit for bit, rtx_radiance of that one ray with the same id,
 * spp = 1 and first_sample = first_sample + k.
 * out_rgb: 3 doubles per surfel, the in-order sum of the spp radiances (from 0) times
 * 1 / (double)(float)spp: the cosine-weighted mean incoming radiance, which is what a Lambertian
 * texel multiplies by its albedo.  Irradiance in the radiometric sense is pi times this value.
 * out_segments (may be NULL): segments traced for the surfel over all its samples.
 * A surfel whose normal has a squared length that is not > 0 or not finite (zero or NaN normals,
 * as in the padding texels of a lightmap) traces nothing: its output is 0 0 0 and its segment
 * count 0.  This is decided on the device; the device variant never reads caller memory on the
 * host.  Arguments are checked in rtx_radiance's order and with its messages (scene, params,
 * buffers, spp, first_sample, max_depth, precision) before the scene or a device is touched;
 * then n == 0 returns RTX_OK.  The live scene is read (after rtx_scene_update_* the new
 * geometry); no film is involved.  One call at a time per scene. */
/* Host buffers, staged through pinned memory in batches; returns when the outputs are written. */
int rtx_irradiance(rtx_scene* scene, const rtx_ray* surfels, const uint32_t* ids, size_t n,
                   const rtx_radiance_params* params, double* out_rgb, uint32_t* out_segments);
/* Device buffers; asynchronous on stream (NULL = the scene's stream). */
int rtx_irradiance_device(rtx_scene* scene, const rtx_ray* d_surfels, const uint32_t* d_ids, size_t n,
                          const rtx_radiance_params* params, double* d_out_rgb, uint32_t* d_out_segments,
                          void* stream);

/* ---- direct-lighting queries (DESIGN.md "Direct-lighting queries") ---------------------------
 * How much light reaches these surface points straight from the scene's emitters?  The radiance
 * and irradiance queries find a light only when a path runs into it; this one samples the lights.
 * An emitter is a primitive whose material is RTX_MAT_DIFFUSE_LIGHT (any primitive kind; emission
 * is two-sided).  The scene keeps a table of them with their cumulative areas, built on the
 * device at rtx_scene_create and again by every rtx_scene_update_*.
 * Surfels are rtx_irradiance's (origin x, direction the surface normal, any positive finite
 * length); rtx_radiance_params is read as there, spp being the samples per point, and max_depth
 * is checked and otherwise ignored.  For surfel i and sample k in [0, spp), three numbers u0, u1,
 * u2 from a Philox stream of its own keyed by (seed, pixel = ids ? ids[i] : (uint32_t)i,
 * sample = first_sample + k) give:
 *   the emitter: the first whose cumulative area exceeds u0 * A (A: the total emitting area), so
 *     the points are uniform over all emitting area (not weighted by power);
 *   the point y on it: rect: linear in u1, u2; triangle: s = sqrt(u1),
 *     y = (1 - s) a + s (1 - u2) b + s u2 c; sphere: z = 1 - 2 u1, phi = 2 pi u2 over the whole
 *     sphere (the far side is rejected by the sphere's own occlusion);
 *   the unshadowed contribution C = Le(y) max(0, n_x . w) |n_y . w| A / (pi |y - x|^2), w the unit
 *     vector from x to y, Le and n_y from the hit record a path reaching y would build (textured
 *     lights included);
 *   the visibility V: 1 iff rtx_occluded finds nothing on (RTX_SEAM_TMIN, RTX_DIRECT_TMAX) of the
 *     segment (x, y - x) with the walk of `precision`.  The margin below 1 keeps the emitter out of
 *     its own shadow ray; a blocker within 1e-4 of the segment's length from the light is ignored.
 * out_rgb: 3 doubles per surfel, the in-order sum of C V (from 0) times 1 / (double)(float)spp.
 * Its mean estimates (1 / pi) * the integral of the emitters' radiance times cos(theta) over the
 * hemisphere: rtx_irradiance's unit, so the two compare and add directly.
 * out_visible (may be NULL): per surfel, the samples whose shadow segment was traced and found
 * unoccluded.  A sample is 0 and traces nothing when the scene has no emitters or no emitting
 * area, the normal is degenerate (rtx_irradiance's rule), |y - x|^2 is not > 0 or not finite, or
 * C has no positive component (a light facing away or seen edge-on).
 * Arguments are checked in rtx_radiance's order and with its messages before the scene or a
 * device is touched; then n == 0 returns RTX_OK.  One call at a time per scene. */
#define RTX_DIRECT_TMAX ((double)0.9999f)
/* Host buffers, staged through pinned memory in batches; returns when the outputs are written. */
int rtx_direct(rtx_scene* scene, const rtx_ray* surfels, const uint32_t* ids, size_t n,
               const rtx_radiance_params* params, double* out_rgb, uint32_t* out_visible);
/* Device buffers; asynchronous on stream (NULL = the scene's stream). */
int rtx_direct_device(rtx_scene* scene, const rtx_ray* d_surfels, const uint32_t* d_ids, size_t n,
                      const rtx_radiance_params* params, double* d_out_rgb, uint32_t* d_out_visible,
                      void* stream);
/* The live emitter table: the number of emitters and their total area A (0 and 0.0 for a scene
 * without emitters), after everything queued on the scene's stream.  Either output may be NULL,
 * not both. */
int rtx_scene_emitters(const rtx_scene* scene, int64_t* count, double* area);

/* ---- next-event estimation (DESIGN.md "Next-event estimation") --------------------------------
 * rtx_radiance and rtx_render find a light only when a path runs into it.  These entry points
 * trace the same paths and sample the emitters at every diffuse vertex as well: a second, opt-in
 * estimator of the same radiance with far less variance where lights are small.  Nothing above
 * changes; results are deterministic in (seed, pixel, sample).
 * The path of (seed, pixel, sample) is rtx_radiance's path: same closest hits, shading steps,
 * throughput, Russian roulette and closest-hit segment count (segment d shades from stream d + 1).
 * On top of it, without multiple importance sampling:
 *   term: at the hit of segment d, when a Lambertian scattered there, d + 1 < max_depth and the
 *     emitter table is usable (emitters exist, their area A is finite and > 0), one sample of
 *     rtx_direct for the surfel (hit point, shading normal), drawn from a Philox stream of its own
 *     per depth (0xA3000000 + d of the same key), contributes w * (C V): C and V as rtx_direct
 *     defines them, w = (throughput on arrival at the vertex) * (the Lambertian's reflectance).
 *     The vertex's roulette does not apply to it.  d + 1 < max_depth mirrors rtx_render's rule that
 *     a segment at the depth limit returns sky whatever it hit: the plain estimator collects no
 *     emission there either.
 *   suppression: a path that ends on an emitter (a hit below the depth limit) right after a vertex
 *     where a term was eligible contributes 0 there: that light was already sampled.  Emission
 *     after a metal or dielectric vertex and at segment 0 is collected as before.
 * A sample's value is the terms added in depth order (from 0) plus the path's end; out_rgb is the
 * in-order sum of the spp values times 1 / (double)(float)spp, as rtx_radiance resolves.
 * out_segments (may be NULL): closest-hit segments plus the shadow segments actually traced.
 * Without emitters, or with max_depth <= 1, every output equals rtx_radiance's bit for bit.
 * Limit (as rtx_direct): a primitive turned into a light by rtx_scene_update_prims is not in the
 * emitter table; after a diffuse vertex it is neither sampled nor counted.
 * Arguments are checked in rtx_radiance's order and with its messages before the scene or a
 * device is touched, then max_depth > 0x00FFFFFF is RTX_ERR_INVALID (the per-depth streams stay
 * inside 0xA3000000 .. 0xA3FFFFFF); then n == 0 returns RTX_OK.  One call at a time per scene. */
/* Host buffers, staged through pinned memory in batches; returns when the outputs are written. */
int rtx_radiance_nee(rtx_scene* scene, const rtx_ray* rays, const uint32_t* ids, size_t n,
                     const rtx_radiance_params* params, double* out_rgb, uint32_t* out_segments);
/* Device buffers; asynchronous on stream (NULL = the scene's stream). */
int rtx_radiance_nee_device(rtx_scene* scene, const rtx_ray* d_rays, const uint32_t* d_ids, size_t n,
                            const rtx_radiance_params* params, double* d_out_rgb, uint32_t* d_out_segments,
                            void* stream);
/* A frame with that estimator: for every pixel of the subset of params and sample k in [0, spp)
 * the camera's own ray (the ray rtx_render generates: stream 0 of (seed, global pixel, k)) is the
 * depth-0 segment of such a path, keyed by the global pixel index.  Read from params: spp (>= 1),
 * max_depth, seed, precision and the tile / stripe fields; adaptive != 0 is RTX_ERR_INVALID; mode,
 * flags, min_spp, rel_threshold and samples_per_group are ignored.  out_rgb: 3 doubles per pixel
 * in subset order, as rtx_render writes them; out_segments (may be NULL): one uint32 per pixel,
 * all segments of its samples.  Without emitters the frame equals rtx_render's fixed-spp
 * RTX_MODE_WAVEFRONT frame bit for bit; it equals rtx_radiance_nee fed rtx_render's primary rays
 * with global pixel ids in every case.  Checks, in order: scene, cam / params, spp, max_depth
 * (negative, then above 0x00FFFFFF), adaptive, precision, the subset; an empty subset returns
 * RTX_OK; then out_rgb NULL is RTX_ERR_INVALID.  Host buffers. */
int rtx_render_nee(rtx_scene* scene, const rtx_camera* cam, const rtx_render_params* params, double* out_rgb,
                   uint32_t* out_segments);
/* Device buffers; asynchronous on stream (NULL = the scene's stream). */
int rtx_render_nee_device(rtx_scene* scene, const rtx_camera* cam, const rtx_render_params* params,
                          double* d_out_rgb, uint32_t* d_out_segments, void* stream);

/* ---- multiple importance sampling (DESIGN.md "Multiple importance sampling") -------------------
 * The light-sampling estimator above is noisy where a surface comes close to a light (its sample
 * value C = g Le, g = cos_x cos_y A / (pi |y - x|^2), is unbounded), exactly where the plain
 * estimator is good.  These entry points combine the two with the power heuristic: a third, opt-in
 * estimator of the same radiance.  The path of (seed, pixel, sample), the emitter sample at each
 * eligible vertex (same rule, same stream 0xA3000000 + d) and both segment counts are
 * rtx_radiance_nee's; two weights differ.
 *   light side: the term is (w * (C V)) * wl, wl = 1 / (1 + g^2), g the scalar of that sample: the
 *     ratio of the BSDF's solid-angle density cos_x / pi to the light sampler's |y - x|^2 /
 *     (A cos_y).  The term is at most w Le / 2.
 *   BSDF side: a path that ends on an emitter (a hit below the depth limit) right after a vertex
 *     where a term was eligible contributes wb * (throughput * Le) instead of 0, with
 *     wb = 1 - 1 / (1 + gb^2) and gb the same ratio for the parent vertex and the hit point; a hit
 *     primitive that is not in the emitter table (a light made by rtx_scene_update_prims: the light
 *     sampler cannot choose it) has wb = 1, so such scenes are estimated without bias.
 * The two weights sum to 1 at every pair of points, so the expectation is rtx_radiance's.  Emission
 * at segment 0 and after a metal or dielectric vertex is collected unweighted, as before.  Without
 * emitters, or with max_depth <= 1, every output equals rtx_radiance's bit for bit.
 * Arguments, checks, their order, the max_depth cap and the outputs are those of the four entry
 * points above; the messages say "mis" where those say "nee". */
int rtx_radiance_mis(rtx_scene* scene, const rtx_ray* rays, const uint32_t* ids, size_t n,
                     const rtx_radiance_params* params, double* out_rgb, uint32_t* out_segments);
int rtx_radiance_mis_device(rtx_scene* scene, const rtx_ray* d_rays, const uint32_t* d_ids, size_t n,
                            const rtx_radiance_params* params, double* d_out_rgb, uint32_t* d_out_segments,
                            void* stream);
int rtx_render_mis(rtx_scene* scene, const rtx_camera* cam, const rtx_render_params* params, double* out_rgb,
                   uint32_t* out_segments);
int rtx_render_mis_device(rtx_scene* scene, const rtx_camera* cam, const rtx_render_params* params,
                          double* d_out_rgb, uint32_t* d_out_segments, void* stream);

/* ---- light probes (DESIGN.md "Light probes") --------------------------------------------------
 * How much light arrives at these points from every direction?  The radiance over the whole sphere
 * about a point that need lie on no surface, projected onto real spherical harmonics to band 2:
 * nine coefficients per colour channel, for lighting moving objects and volumes.  No ray and no
 * per-sample value goes through caller memory.  A probe is three doubles.  rtx_radiance_params is
 * read as by rtx_radiance, spp being the samples per probe.  estimator: 0 (the plain path),
 * RTX_ESTIMATOR_NEE or RTX_ESTIMATOR_MIS.  For probe i and sample k in [0, spp):
 *   direction: two numbers u1, u2 from a Philox stream of its own (0xA4000000) keyed by (seed,
 *     pixel = ids ? ids[i] : (uint32_t)i, sample = first_sample + k) give z = 1 - 2 u1,
 *     phi = 2 pi u2, r = sqrt(max(0, 1 - z z)), d = (r cos phi, r sin phi, z): uniform over the
 *     sphere, |d| = 1 to rounding;
 *   path: the ray (point, d) is the depth-0 segment of a path with throughput 1.  With estimator 0
 *     its value L_k is, bit for bit, rtx_radiance of that one ray with the same id, spp = 1 and
 *     first_sample = first_sample + k; with RTX_ESTIMATOR_NEE / _MIS rtx_radiance_nee /
 *     rtx_radiance_mis of it, and its segment count likewise.  The probe is no vertex: an emitter
 *     seen directly at depth 0 counts in full, as for a camera ray.
 *   basis: with (x, y, z) = d, in this order and with these operations (no contraction):
 *     Y0 = K0, Y1 = K1*y, Y2 = K1*z, Y3 = K1*x, Y4 = K4*(x*y), Y5 = K4*(y*z),
 *     Y6 = K6*(3.0*(z*z) - 1.0), Y7 = K4*(x*z), Y8 = K8*(x*x - y*y),
 *     the constants below: the closed forms rounded to the nearest double.
 * out_sh: 27 doubles per probe, [coefficient j][r, g, b]: the products Y_j(d_k) * L_k[c] added in
 * sample order from 0, resolved as (4 pi) * ((1 / (double)(float)spp) * sum): the Monte-Carlo
 * estimate of the integral of L(w) Y_j(w) over the sphere.
 * out_segments (may be NULL): as rtx_irradiance's, all segments of the probe's samples.
 * out_backfaces (may be NULL): the samples whose depth-0 segment hit a primitive from inside
 * (front_face == 0 in the hit record): a probe buried in geometry reports spp, one in the open 0.
 * A probe with a non-finite coordinate traces nothing: 27 zeros and two zero counts, decided on the
 * device.  Checks: rtx_radiance's in its order and with its messages (scene, params, buffers: points
 * and out_sh, spp, first_sample, max_depth, precision), then the estimator ("probe: bad
 * estimator"), then for RTX_ESTIMATOR_NEE / _MIS the max_depth cap of rtx_radiance_nee /
 * rtx_radiance_mis; then n == 0 returns RTX_OK.  The live scene is read (after rtx_scene_update_*
 * the new geometry).  One call at a time per scene. */
#define RTX_SH_COEFFS 9
#define RTX_SH_K0 0.28209479177387814 /* 1 / (2 sqrt(pi)) */
#define RTX_SH_K1 0.48860251190291992 /* sqrt(3 / (4 pi)) */
#define RTX_SH_K4 1.0925484305920792  /* sqrt(15 / (4 pi)) */
#define RTX_SH_K6 0.31539156525251999 /* sqrt(5 / (16 pi)) */
#define RTX_SH_K8 0.54627421529603959 /* sqrt(15 / (16 pi)) */
/* Host buffers, staged through pinned memory in batches; returns when the outputs are written. */
int rtx_probe_sh(rtx_scene* scene, const double* points, const uint32_t* ids, size_t n,
                 const rtx_radiance_params* params, int32_t estimator, double* out_sh, uint32_t* out_segments,
                 uint32_t* out_backfaces);
/* Device buffers; asynchronous on stream (NULL = the scene's stream). */
int rtx_probe_sh_device(rtx_scene* scene, const double* d_points, const uint32_t* d_ids, size_t n,
                        const rtx_radiance_params* params, int32_t estimator, double* d_out_sh,
                        uint32_t* d_out_segments, uint32_t* d_out_backfaces, void* stream);
/* The coefficients of one probe (27 doubles, rtx_probe_sh's layout) evaluated at n unit directions
 * (3 doubles each; not normalised here), 3 doubles out per direction, the basis formed as above.
 * cosine == 0: the reconstruction, per channel ((..(c_0 Y_0 + c_1 Y_1) + ..) + c_8 Y_8).
 * cosine == 1: the cosine-convolved value over pi, with `dir` the surface normal:
 * c_0 Y_0 + (2/3) (c_1 Y_1 + c_2 Y_2 + c_3 Y_3) + (1/4) (c_4 Y_4 + .. + c_8 Y_8), each bracket added
 * left to right, the factors 2.0 / 3.0 and 0.25: rtx_irradiance's unit, so the two compare.
 * Host only, plain C++: NULL buffers with n > 0 or sh NULL ("NULL buffer") and cosine outside 0..1
 * ("sh eval: cosine must be 0 or 1") are RTX_ERR_INVALID; no device is touched. */
int rtx_sh_eval(const double* sh, const double* dirs, size_t n, int32_t cosine, double* out_rgb);

enum { RTX_DENOISE_DEMODULATE = 1 }; /* filter colour / max(albedo, 1e-3), multiply back at the end */
typedef struct {
  int32_t iterations; /* 0..8; iteration k filters 5 x 5 taps at step 2^k; 0 copies the input */
  int32_t flags;      /* RTX_DENOISE_* */
  double normal_power; /* w_n = max(0, n_p . n_q)^normal_power */
  double sigma_depth;  /* w_z = exp(-|z_p - z_q| / (sigma_depth max(z_p, z_q))) */
  double sigma_color;  /* w_l = exp(-|lum_p - lum_q| / (sigma_color g_p + 1e-6)) */
} rtx_denoise_params;
/* iterations 5, normal_power 64, sigma_depth 0.05, sigma_color 4, RTX_DENOISE_DEMODULATE.  Host only. */
int rtx_denoise_params_default(rtx_denoise_params* out);
/* Filter a width x height image on the scene's device: rgb, albedo and normal 3 doubles per
 * pixel, depth 1, row-major; variance (1 per pixel, may be NULL) is the variance of each pixel's
 * estimate in the filtered domain (of colour / albedo with RTX_DENOISE_DEMODULATE) and scales the
 * colour distance, g_p = sqrt of its 3 x 3 Gaussian; without it g_p = 1.  params NULL: the
 * defaults.  The working buffers are f32 and belong to the scene.  iterations outside 0..8, a
 * sigma or power that is not positive, and width * height >= 2^31 are RTX_ERR_INVALID.  out
 * (3 doubles per pixel) may be rgb.  Host buffers. */
int rtx_denoise(rtx_scene* scene, int32_t width, int32_t height, const double* rgb, const double* albedo,
                const double* normal, const double* depth, const double* variance, const rtx_denoise_params* params,
                double* out);
/* Device buffers; asynchronous on stream (NULL = the scene's stream). */
int rtx_denoise_device(rtx_scene* scene, int32_t width, int32_t height, const double* d_rgb, const double* d_albedo,
                       const double* d_normal, const double* d_depth, const double* d_variance,
                       const rtx_denoise_params* params, double* d_out, void* stream);
/* The film's output (rtx_film_resolve) filtered with the AOVs of its own camera and pixel
 * rectangle, computed on first use and kept with the film (not part of its saved state).  An
 * adaptive film passes the variance of its estimate: var_c = m2_c / (n - 1) / n for n >= 2 else
 * 0, var = sum_c lumweight_c^2 var_c, divided by lum(max(albedo, 1e-3))^2 when demodulating.
 * The film's state is not changed.  A stripe film is RTX_ERR_INVALID (stripes are not adjacent
 * rows).  out_rgb: host, subset order. */
int rtx_film_denoise(rtx_film* film, const rtx_denoise_params* params, double* out_rgb);
/* The same frame as P3 file bytes (as rtx_film_p3). */
int rtx_film_denoise_p3(rtx_film* film, const rtx_denoise_params* params, char* out, size_t cap, size_t* out_len);

/* write_color bytes (core/color.h:18-33) as a P3 PPM; rgb is a linear framebuffer (host). */
int rtx_write_ppm(const char* path, const double* rgb, int32_t width, int32_t height);

#ifdef __cplusplus
}
#endif
#endif /* RTX_H_ */
