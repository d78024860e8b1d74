// rtx_host.h — the host-side internals the C ABI's translation units share (rtx_capi.hip: scenes,
// films, renders; rtx_queries.hip: the ray-query entry points): error reporting, device and
// pinned buffers that free themselves (DevBuf, HostBuf: a scene's or a film's memory goes with
// its members, no list names them), the scene and film objects behind the opaque handles of include/rtx.h, the
// pixel subset of a render, and the one dispatch of a traversal kernel on a scene's walk
// (with_walk, launch_1d).  Host code only; no kernel is defined here.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <type_traits>
#include <vector>

#include "rtx.h"
#include "rtx_bounds.h"
#include "rtx_kernels.h"

using namespace rtxd;

// rtx_last_error()'s message, per thread: one definition, in rtx_capi.hip
extern "C" void rtx_internal_set_error(const char* msg);

inline int fail(int code, const std::string& msg) {
  rtx_internal_set_error(msg.c_str());
  return code;
}

#define HIPC(expr)                                                                                   \
  do {                                                                                               \
    hipError_t e_ = (expr);                                                                          \
    if (e_ != hipSuccess)                                                                            \
      return fail(RTX_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_) + " (" __FILE__ ":" + \
                                   std::to_string(__LINE__) + ")");                                  \
  } while (0)

// Device memory that frees itself (grow-only; move-only)
struct DevBuf {
  void* p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr, o.n = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) release(), p = o.p, n = o.n, o.p = nullptr, o.n = 0;
    return *this;
  }
  ~DevBuf() { release(); }
  int reserve(size_t bytes) {
    if (bytes <= n) return RTX_OK;
    if (p) (void)hipFree(p);
    p = nullptr, n = 0;
    if (bytes == 0) return RTX_OK;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) return fail(RTX_ERR_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
    n = bytes;
    return RTX_OK;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr, n = 0;
  }
  template <class T>
  T* as() const {
    return (T*)p;
  }
};

struct HostBuf {  // pinned host staging (grow-only; move-only, frees itself)
  void* p = nullptr;
  size_t n = 0;
  HostBuf() = default;
  HostBuf(HostBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr, o.n = 0; }
  HostBuf& operator=(HostBuf&& o) noexcept {
    if (this != &o) release(), p = o.p, n = o.n, o.p = nullptr, o.n = 0;
    return *this;
  }
  ~HostBuf() { release(); }
  int reserve(size_t bytes) {
    if (bytes <= n) return RTX_OK;
    if (p) (void)hipHostFree(p);
    p = nullptr, n = 0;
    if (bytes == 0) return RTX_OK;
    hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
    if (e != hipSuccess) return fail(RTX_ERR_NOMEM, std::string("hipHostMalloc: ") + hipGetErrorString(e));
    n = bytes;
    return RTX_OK;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr, n = 0;
  }
};

using rtxb::round_down;
using rtxb::round_up;

struct AdaptWs {
  // lst / kl / ol: the phases' pixel lists (ping-pong: sub-pixel, samples, first slot per entry);
  // knext: the next batch per entry of the phase just traced; pk: their packed prefix sums
  // rv: each pixel's predicted convergence count at its last record (k_adapt_plan's pooling)
  DevBuf lbuf, smap, lst[2], kl[2], ol[2], knext, pk, rv, scan_tmp, ctr;  // ctr: 8 region slot counters (128 B apart), then u64 slot count, pixel count, slot map address, ..., [132] segment buffer, then the spread pixel counts (kSpreadBase)
  DevBuf segs;                                  // counting renders: each slot's path segments (u16)
  HostBuf total_h;                              // pinned copy of the next phase's slot count
  hipEvent_t ev = nullptr;                      // total_h written
  ~AdaptWs() {
    if (ev) (void)hipEventDestroy(ev);
  }
};

// A film (rtx_film_*): its own pixel state on its scene's device; everything else a render needs
// (radiance slots, queues, counters, the adaptive workspace) stays the scene's scratch.
// Every buffer of a film lives here, so that release() below cannot miss one
struct FilmBufs {
  DevBuf sum, mean, m2, samples, conv;  // mean / m2: adaptive films only
  mutable DevBuf stage;     // save / load: the blob's body on the device
  // rtx_film_denoise*: the packed guide and albedo of the film's pixels (float4 each), made on
  // first use; not part of the saved state
  DevBuf dn_guide, dn_alb;
};
struct rtx_film : FilmBufs {
  rtx_scene* sc = nullptr;  // nullptr once the scene was destroyed (the film's memory went with it)
  int device = 0;
  rtx_camera cam{};
  rtx_render_params prm{};  // spp unused: every rtx_film_render names its budget
  PixelMap map{};
  int64_t npix = 0;
  int32_t done = 0;         // samples done: the film equals a one-shot render at spp = done
  // 0: a plain film (rtx_film_create); RTX_ESTIMATOR_NEE / RTX_ESTIMATOR_MIS: a sampled film
  // (rtx_film_create_sampled, rtx_film_sampled.h); active 0: its last render found every pixel
  // converged, so further renders have nothing to launch (-1: not known)
  int32_t estimator = 0;
  int64_t active = -1;
  int64_t epoch = 0;        // the scene's epoch the film was created or last reset at (rtx_film_reset)
  bool aov_ready = false;
  PixelSoA px() const {
    return PixelSoA{sum.as<double>(), mean.as<double>(), m2.as<double>(), samples.as<int32_t>(), conv.as<uint8_t>()};
  }
  void release() {  // an empty film: what is left of one that outlives its scene
    static_cast<FilmBufs&>(*this) = FilmBufs{};
    aov_ready = false;
  }
};

struct rtx_scene {
  int device = 0;
  std::vector<rtx_film*> films;  // live films of this scene (rtx_film_create / rtx_film_destroy)
  hipStream_t stream = nullptr;
  int cus = 0;
  DevBuf nodes, prims, mats, texs, images, fnodes, tri_n;
  // kept for rtx_scene_update_* (DESIGN.md §4c), scenes with nodes: each primitive's reference
  // box (6 doubles, rtx_prim_bounds) and conservative fast box (6 floats, prim_box rounded
  // outward), and both trees' node indices grouped by height (a node without child nodes has
  // height 0); *_lvl: where each height starts in its index array, and the end
  DevBuf ref_box, fast_box, node_order, f4_order, upd_stage;
  std::vector<int64_t> node_lvl, f4_lvl;
  HostBuf upd_host;            // rtx_scene_update_prims: pinned staging of the caller's records
  std::vector<int8_t> kinds;   // each primitive's kind (an update may not change it)
  int32_t n_materials = 0;
  int64_t epoch = 0;           // updates applied so far
  DevBuf segs1;  // counting adaptive renders: the first phase's per-slot path segments (u16)
  std::vector<DevBuf> texels;
  DScene S{};
  int stack_parity = 32, stack_fast = 32;
  int fast_need = 0;     // exact worst-case stack depth of the lean BVH4 walk (build_fast4)
  size_t n_f4 = 0;       // F4Node count of the fast tree
  bool fast_ok = false;  // RTX_PREC_FAST available (BVH with an internal root)
  int park = -1;         // persistent fast schedule: -1 not yet timed, 0 plain kernel, 1 PARK kernel
  DevBuf calib_rgb;      // output of the schedule-timing renders
  int64_t n_nodes = 0;
  // render workspace (grow-only)
  DevBuf px_sum, px_mean, px_m2, px_samples, px_conv, lbuf, queue[2], counters, out_rgb, out_spp, rays, hits;
  DevBuf p3_scratch, p3_body;  // device P3 encoding (rtx_p3.h)
  DevBuf occ;                  // rtx_occluded: the rays' bytes (the rays themselves stage through `rays`)
  // rtx_radiance: the slot scratch (radiance and segments per slot, the carry of a ray summed
  // across chunks), and the host entry point's staging (pinned on the host; ids, output and
  // segment totals on the device, the rays through `rays`)
  DevBuf rad_L, rad_segs, rad_carry, rad_ids, rad_out, rad_oseg;
  HostBuf rad_host;
  // rtx_direct (rtx_direct.h): the emitters' primitive indices, fixed at create (kept on the host
  // too), and their cumulative areas, rebuilt on the device after every update; none: no buffers
  std::vector<uint32_t> emit_idx;
  DevBuf emit_prim, emit_cum;
  DevBuf patch_q;              // adaptive early output: the pixels still sampling when it went
  // AOVs and the denoiser (rtx_denoise.h): the f64 AOVs of rtx_aov / a film's first denoise, the
  // host entry points' staged inputs, an adaptive film's variance, and the filter's f32 working
  // set: colour + variance ping-pong, guide, albedo
  DevBuf aov_f64, dn_in, dn_var, dn_work[2], dn_guide, dn_alb;
  HostBuf stage_rgb, stage_spp;  // rtx_render_multi: pinned D2H staging of this device's stripes
  HostBuf counters_h;            // timed renders: pinned copy of the statistics counters (read after the end event)
  // ev[0] / ev[1]: a timed render's start and end (rtx_stats.kernel_ms), ev[2] / ev[3]: the
  // adaptive debug timing, ev[4]: the frame and its output copy done (the host's wait)
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  // the hot launches' timing events of a timed call: a grow-only pool, used in pairs
  std::vector<hipEvent_t> evpool;
  hipEvent_t pool_event(size_t i) {  // event i, created on demand; nullptr: hipEventCreate failed
    while (evpool.size() <= i) {
      hipEvent_t e = nullptr;
      if (hipEventCreate(&e) != hipSuccess) return nullptr;
      evpool.push_back(e);
    }
    return evpool[i];
  }
  int pool_pairs_ms(size_t n, double& ms) const {  // the sum of the first n / 2 pairs, in ms, added to `ms`
    for (size_t e = 0; e + 1 < n; e += 2) {
      float pair_ms = 0;
      HIPC(hipEventElapsedTime(&pair_ms, evpool[e], evpool[e + 1]));
      ms += pair_ms;
    }
    return RTX_OK;
  }
  // banded output copies (BandSink): a copy stream and its ordering events
  hipStream_t copy_stream = nullptr;
  std::vector<hipEvent_t> band_ev;
  AdaptWs aw;  // adaptive phases' workspace
  // sampled films (rtx_film_sampled.h): the spread segment counters, their totals and the active
  // lists' counts; the pinned copy of the totals and of the next list's count
  DevBuf fs_ctr;
  HostBuf fs_host;
  double slot_mem = -1.0;  // bytes the slot buffers may take (slot_target; -1: not yet queried)
  ~rtx_scene() {
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
    // films outlive their scene as empty shells: their device memory goes here, and every call
    // on them but rtx_film_destroy fails from now on
    for (rtx_film* f : films) f->release(), f->sc = nullptr;
    for (auto e : evpool) (void)hipEventDestroy(e);
    for (auto e : band_ev) (void)hipEventDestroy(e);
    if (copy_stream) (void)hipStreamDestroy(copy_stream);
    for (auto& e : ev)
      if (e) (void)hipEventDestroy(e);
    if (stream) (void)hipStreamDestroy(stream);
    // the buffers (DevBuf, HostBuf) and the adaptive workspace free themselves after this
  }
};

template <class T>
int upload(DevBuf& b, const T* src, size_t n, hipStream_t s) {
  int rc = b.reserve(std::max<size_t>(n * sizeof(T), 16));
  if (rc) return rc;
  if (n) HIPC(hipMemcpyAsync(b.p, src, n * sizeof(T), hipMemcpyHostToDevice, s));
  return RTX_OK;
}

inline int64_t subset_pixels(const rtx_camera* cam, const rtx_render_params* p, PixelMap& m, std::string& err) {
  m.W = cam->image_width, m.H = cam->image_height;
  if (m.W <= 0 || m.H <= 0) {
    err = "camera not initialised (image size <= 0)";
    return -1;
  }
  if ((int64_t)m.W * m.H > 0x7FFFFFFFll) {  // pixel indices are 32-bit on the device
    err = "image larger than 2^31 pixels";
    return -1;
  }
  if (p->stripe_rows > 0) {
    if (p->stripe_count <= 0 || p->stripe_index < 0 || p->stripe_index >= p->stripe_count) {
      err = "bad stripe_index/stripe_count";
      return -1;
    }
    m.stripes = 1, m.srows = p->stripe_rows, m.sidx = p->stripe_index, m.scount = p->stripe_count;
    int64_t rows = 0;
    for (int y = 0; y < m.H; y++)
      if ((y / m.srows) % m.scount == m.sidx) rows++;
    m.x0 = m.y0 = 0, m.w = m.W, m.h = (int)rows;
    set_map_div(m);
    return rows * (int64_t)m.W;
  }
  m.stripes = 0;
  m.x0 = p->x0, m.y0 = p->y0, m.w = p->w, m.h = p->h;
  if (m.w == 0 && m.h == 0) m.x0 = 0, m.y0 = 0, m.w = m.W, m.h = m.H;
  if (m.x0 < 0 || m.y0 < 0 || m.w < 0 || m.h < 0 || m.x0 + m.w > m.W || m.y0 + m.h > m.H) {
    err = "tile outside the image";
    return -1;
  }
  m.srows = 1, m.sidx = 0, m.scount = 1;
  set_map_div(m);
  return (int64_t)m.w * m.h;
}

// ---- the walk of a traversal kernel: its <STACK, FAST> template pair ----
template <int STACK, bool FAST>
struct Walk {
  static constexpr int stack = STACK;
  static constexpr bool fast = FAST;
};
// f(Walk<STACK, FAST>{}) for a stack size and a tree: any stack other than 32 means 64
template <class F>
int with_walk(int stack, bool fast, F&& f) {
  if (fast) return stack == 32 ? f(Walk<32, true>{}) : f(Walk<64, true>{});
  return stack == 32 ? f(Walk<32, false>{}) : f(Walk<64, false>{});
}
// ... for the walk a query of `precision` runs on a scene: fast only with a fast tree, and that
// tree's stack size
template <class F>
int with_walk(const rtx_scene* sc, int32_t precision, F&& f) {
  const bool fast = precision == RTX_PREC_FAST && sc->fast_ok;
  return with_walk(fast ? sc->stack_fast : sc->stack_parity, fast, f);
}
// f(std::bool_constant<b>{}): a run-time flag as a kernel's template argument
template <class F>
int with_flag(bool b, F&& f) {
  return b ? f(std::true_type{}) : f(std::false_type{});
}
// One lane per item, blocks of kBlock, on `s`
template <class K, class... Args>
int launch_1d(K kernel, int64_t items, size_t lds, hipStream_t s, const Args&... args) {
  hipLaunchKernelGGL(kernel, dim3((unsigned)((items + kBlock - 1) / kBlock)), dim3(kBlock), lds, s, args...);
  HIPC(hipGetLastError());
  return RTX_OK;
}

// ---- what crosses the units ----
// rtx_queries.hip: k_aov over a pixel map with the walk of `precision` (film_denoise_on), and the
// emitters' areas and their running sum from the live primitives (scene create, in-place updates)
int aov_on(rtx_scene* sc, const rtx_camera* cam, const PixelMap& map, int64_t npix, int32_t precision, double* d_albedo,
           double* d_normal, double* d_depth, hipStream_t s);
int emitters_rebuild(rtx_scene* sc, hipStream_t s);
// rtx_queries.hip: a sampled film (f->estimator != 0, alive, budget > f->done) advanced to `budget`
// on its scene's stream (rtx_film_sampled.h); the caller sets f->done
int film_sampled_render(rtx_film* f, int32_t budget, rtx_stats* stats);
// next-event estimation: the vertex of segment d draws from stream kRngStreamNee + d, d < max_depth
inline int nee_depth_check(int32_t max_depth, bool mis = false) {
  if (max_depth > 0x00FFFFFF)
    return fail(RTX_ERR_INVALID, mis ? "mis: max_depth above 16777215 (0x00FFFFFF)"
                                     : "nee: max_depth above 16777215 (0x00FFFFFF)");
  return RTX_OK;
}
// A call's slot scratch of the radiance queries: at most kRadianceSlots slots (448 MB), which
// rtx_internal_radiance_chunk may raise to kRadianceSlotsMax (the test hooks' limit per call too)
constexpr int64_t kRadianceSlots = (int64_t)1 << 24;
constexpr int64_t kRadianceSlotsMax = (int64_t)1 << 30;
