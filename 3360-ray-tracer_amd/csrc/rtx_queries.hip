// rtx_queries.hip — the ray-query entry points of the C ABI (include/rtx.h) and their kernels:
// closest hit (rtx_intersect*), any hit and the AO pass (rtx_occluded*, rtx_ao*), first-hit AOVs
// (rtx_aov*), radiance, irradiance and direct lighting on caller-supplied rays and surfels
// (rtx_radiance*, rtx_irradiance*, rtx_direct*, rtx_scene_emitters), the light-sampling estimator
// on rays and on the camera's own frame (rtx_radiance_nee*, rtx_render_nee*) and its power-heuristic
// form (rtx_radiance_mis*, rtx_render_mis*), light probes (rtx_probe_sh*), with their test hooks, and the render of a sampled film
// (film_sampled_render: the frames of those two estimators kept as a film, rtx_film_sampled.h).
// Scenes, films and the frame renderer are rtx_capi.hip's; the two share rtx_host.h.  Every query
// picks its walk with with_walk (fast only with a fast tree, the scene's stack size).
#include <atomic>
#include <cstring>

#include "rtx_host.h"
#include "rtx_occlusion.h"
#include "rtx_radiance.h"
#include "rtx_irradiance.h"
#include "rtx_direct.h"
#include "rtx_nee.h"
#include "rtx_probe.h"
#include "rtx_film_sampled.h"
#include "rtx_scan.h"
#include "rtx_shade_steps.h"
#define RTX_DENOISE_AOV_KERNELS  // this translation unit holds k_aov (it needs the trace kernels)
#include "rtx_denoise.h"

// k_aov over a pixel map, with the walk rtx_intersect_device picks for `precision`
int aov_on(rtx_scene* sc, const rtx_camera* cam, const PixelMap& map, int64_t npix, int32_t precision, double* d_albedo,
           double* d_normal, double* d_depth, hipStream_t s) {
  if (npix == 0) return RTX_OK;
  return with_walk(sc, precision, [&](auto w) {
    return launch_1d(k_aov<w.stack, w.fast>, npix, stack_lds_bytes(w.stack), s, sc->S, *cam, map, npix,
                     (double)RTX_SEAM_TMIN, d_albedo, d_normal, d_depth);
  });
}

namespace {
// ---- direct-lighting queries (rtx_direct.h) ----
EmitterTable emitter_table(const rtx_scene* sc) {
  return EmitterTable{sc->emit_prim.as<uint32_t>(), sc->emit_cum.as<double>(), (int64_t)sc->emit_idx.size()};
}
}  // namespace
// The emitters' areas and their running sum from the live primitives, on `s`: at create, and at
// the end of every in-place update.  A scene without emitters launches nothing.
int emitters_rebuild(rtx_scene* sc, hipStream_t s) {
  const EmitterTable E = emitter_table(sc);
  if (E.n <= 0) return RTX_OK;
  int rc;
  if ((rc = launch_1d(k_emitter_area, E.n, 0, s, sc->prims.as<rtx_prim>(), E))) return rc;
  return launch_1d(k_emitter_scan, 1, 0, s, E);
}

namespace {
// ---- occlusion queries and the AO pass (rtx_occlusion.h) ----
// rays == nullptr: k_ao into d_out; else k_ao_rays (the test hook's sample rays)
int ao_on(rtx_scene* sc, const rtx_camera* cam, const PixelMap& map, int64_t npix, int32_t precision,
          const rtx_ao_params* ao, double* d_out, rtx_ray* d_rays, hipStream_t s) {
  if (npix == 0) return RTX_OK;
  return with_walk(sc, precision, [&](auto w) {
    if (d_rays)
      return launch_1d(k_ao_rays<w.stack, w.fast>, npix, stack_lds_bytes(w.stack), s, sc->S, *cam, map, npix, ao->seed,
                       ao->samples, d_rays);
    return launch_1d(k_ao<w.stack, w.fast>, npix, stack_lds_bytes(w.stack), s, sc->S, *cam, map, npix, ao->seed,
                     ao->samples, ao->radius, d_out);
  });
}
// the checks rtx_ao, rtx_ao_device and rtx_internal_ao_rays share; *npix: pixels of the subset
int ao_check(const rtx_scene* sc, const rtx_camera* cam, const rtx_render_params* prm, const rtx_ao_params* ao,
             PixelMap& map, int64_t* npix) {
  if (!sc) return fail(RTX_ERR_INVALID, "scene is NULL");
  if (!cam || !prm || !ao) return fail(RTX_ERR_INVALID, "NULL argument");
  if (ao->samples < 1 || ao->samples > 1024) return fail(RTX_ERR_INVALID, "ao: samples outside 1..1024");
  if (!(ao->radius > 0)) return fail(RTX_ERR_INVALID, "ao: radius must be positive");
  std::string err;
  *npix = subset_pixels(cam, prm, map, err);
  if (*npix < 0) return fail(RTX_ERR_INVALID, err);
  return RTX_OK;
}
// ---- radiance queries (rtx_radiance.h) ----
// the slot cap of the calls that follow (rtx_internal_radiance_chunk; 0: kRadianceSlots)
std::atomic<int64_t> g_radiance_chunk{0};
int64_t slot_cap() {
  const int64_t tuned = g_radiance_chunk.load();
  return std::min<int64_t>(tuned > 0 ? tuned : kRadianceSlots, kRadianceSlotsMax);
}
// what a chunk's slots hold (radiance_on): a path from a caller's ray, a path from a surfel's
// hemisphere sample, a surfel's emitter sample, or a path with next-event estimation (from a
// caller's ray, or from the camera when radiance_on is given one), plain or with MIS weights
enum SlotKind { kSlotRadiance = 0, kSlotIrradiance = 1, kSlotDirect = 2, kSlotNee = 3, kSlotMis = 4 };
// the checks rtx_radiance*, rtx_irradiance*, rtx_direct* and their test hooks share, in the documented order
int radiance_check(const rtx_scene* sc, const rtx_radiance_params* prm, const void* rays, const void* out) {
  if (!sc) return fail(RTX_ERR_INVALID, "scene is NULL");
  if (!prm) return fail(RTX_ERR_INVALID, "NULL argument");
  if (!rays || !out) return fail(RTX_ERR_INVALID, "NULL buffer");
  if (prm->spp < 1) return fail(RTX_ERR_INVALID, "radiance: spp must be at least 1");
  if (prm->first_sample < 0 || prm->first_sample > 0x7FFFFFFF - prm->spp)
    return fail(RTX_ERR_INVALID, "radiance: first_sample must be >= 0 and first_sample + spp fit int32");
  if (prm->max_depth < 0) return fail(RTX_ERR_INVALID, "negative max_depth");
  if (prm->precision != RTX_PREC_PARITY && prm->precision != RTX_PREC_FAST)
    return fail(RTX_ERR_INVALID, "radiance: bad precision");
  return RTX_OK;
}
// n > 0 rays on device buffers, in chunks of at most `cap` slots (ray x sample): whole rays per
// chunk, or, when one ray's samples exceed the cap, one ray at a time in runs of `cap` samples
// whose partial sum k_radiance_sum carries.  id_base: the pixel key of d_rays[0] when d_ids is
// null (the host entry point's batches).  what: for kSlotIrradiance and kSlotDirect d_rays are
// surfels and the slots are k_irradiance's (rtx_irradiance*) or k_direct's (rtx_direct*: a
// slot's "segments" are its visibility, 0 or 1); the chunking, the scratch and the sum are the same.
// kSlotNee, kSlotMis: k_sampled's slots, from the caller's rays or with `cam` from the camera: the
// "rays" are then the n pixels of the camera's subset in subset order (d_rays and d_ids are not
// read).
int radiance_on(rtx_scene* sc, const rtx_ray* d_rays, const uint32_t* d_ids, uint64_t id_base, int64_t n,
                const rtx_radiance_params* prm, double* d_out, uint32_t* d_segs, hipStream_t s,
                SlotKind what = kSlotRadiance, const NeeCamera* cam = nullptr) {
  const int64_t cap = slot_cap();
  const int64_t spp = prm->spp;
  const int64_t rays_per = std::max<int64_t>(1, cap / spp);  // rays per chunk
  const int64_t k_per = std::min<int64_t>(spp, cap);         // samples of a ray per chunk
  const int64_t most = std::min<int64_t>(n, rays_per) * k_per;  // slots of the largest chunk (<= cap)
  int rc;
  if ((rc = sc->rad_L.reserve((size_t)most * 3 * sizeof(double)))) return rc;
  if ((rc = sc->rad_segs.reserve((size_t)most * sizeof(uint32_t)))) return rc;
  if (k_per < spp) {  // (one ray per chunk)
    if ((rc = sc->rad_carry.reserve(4 * sizeof(double)))) return rc;
  }
  double* const carry = k_per < spp ? sc->rad_carry.as<double>() : nullptr;
  const EmitterTable E = emitter_table(sc);
  const NeeCamera nc = cam ? *cam : NeeCamera{};  // (k_sampled's ray form takes one and does not read it)
  return with_walk(sc, prm->precision, [&](auto w) {
    using W = decltype(w);
    constexpr size_t lds = stack_lds_bytes(W::stack);
    for (int64_t r0 = 0; r0 < n; r0 += rays_per) {
      const int64_t nr = std::min<int64_t>(rays_per, n - r0);
      for (int64_t k0 = 0; k0 < spp; k0 += k_per) {
        const int64_t K = std::min<int64_t>(k_per, spp - k0);
        RadianceChunk A;
        A.rays = d_rays, A.ids = d_ids, A.ray0 = r0, A.id_base = id_base;
        A.slots = (uint32_t)(nr * K), A.K = (uint32_t)K;
        A.s0 = (int32_t)(prm->first_sample + k0), A.max_depth = prm->max_depth, A.seed = prm->seed;
        A.L = sc->rad_L.as<double>(), A.segs = sc->rad_segs.as<uint32_t>();
        if (what == kSlotRadiance) rc = launch_1d(k_radiance<W::stack, W::fast>, A.slots, lds, s, sc->S, A);
        else if (what == kSlotIrradiance) rc = launch_1d(k_irradiance<W::stack, W::fast>, A.slots, lds, s, sc->S, A);
        else if (what == kSlotDirect) rc = launch_1d(k_direct<W::stack, W::fast>, A.slots, lds, s, sc->S, E, A);
        else
          rc = with_flag(cam != nullptr, [&](auto camera) {
            return with_flag(what == kSlotMis, [&](auto mis) {
              return launch_1d(k_sampled<W::stack, W::fast, decltype(camera)::value, decltype(mis)::value>, A.slots,
                               lds, s, sc->S, E, A, nc);
            });
          });
        if (rc) return rc;
        if ((rc = launch_1d(k_radiance_sum, nr, 0, s, sc->rad_L.as<double>(), sc->rad_segs.as<uint32_t>(), nr,
                            (uint32_t)K, k0 == 0 ? 1 : 0, k0 + K == spp ? 1 : 0, prm->spp, carry,
                            carry ? (uint32_t*)(carry + 3) : nullptr, d_out + 3 * r0, d_segs ? d_segs + r0 : nullptr)))
          return rc;
      }
    }
    return (int)RTX_OK;
  });
}
// The host entry point works in batches of kRadianceHostRays rays: the caller's rays and ids are
// copied into pinned memory, traced, and the results copied back out of it.
constexpr size_t kRadianceHostRays = (size_t)1 << 20;
// (shared with rtx_irradiance and rtx_direct, whose rays are surfels)
int radiance_host(rtx_scene* sc, const rtx_ray* rays, const uint32_t* ids, size_t n, const rtx_radiance_params* prm,
                  double* out_rgb, uint32_t* out_segments, SlotKind what) {
  int rc;
  if ((rc = radiance_check(sc, prm, rays, out_rgb))) return rc;
  if ((what == kSlotNee || what == kSlotMis) && (rc = nee_depth_check(prm->max_depth, what == kSlotMis))) return rc;
  if (n == 0) return RTX_OK;
  HIPC(hipSetDevice(sc->device));
  const size_t m = std::min(n, kRadianceHostRays);
  // pinned: rays | rgb | ids | segments (8-byte items first)
  const size_t off_rgb = m * sizeof(rtx_ray), off_ids = off_rgb + m * 3 * sizeof(double),
               off_seg = off_ids + m * sizeof(uint32_t);
  if ((rc = sc->rad_host.reserve(off_seg + m * sizeof(uint32_t)))) return rc;
  if ((rc = sc->rays.reserve(m * sizeof(rtx_ray)))) return rc;
  if ((rc = sc->rad_out.reserve(m * 3 * sizeof(double)))) return rc;
  if ((rc = sc->rad_oseg.reserve(m * sizeof(uint32_t)))) return rc;
  if (ids && (rc = sc->rad_ids.reserve(m * sizeof(uint32_t)))) return rc;
  char* const pin = (char*)sc->rad_host.p;
  for (size_t b0 = 0; b0 < n; b0 += m) {
    const size_t nb = std::min(m, n - b0);
    std::memcpy(pin, rays + b0, nb * sizeof(rtx_ray));
    HIPC(hipMemcpyAsync(sc->rays.p, pin, nb * sizeof(rtx_ray), hipMemcpyHostToDevice, sc->stream));
    if (ids) {
      std::memcpy(pin + off_ids, ids + b0, nb * sizeof(uint32_t));
      HIPC(hipMemcpyAsync(sc->rad_ids.p, pin + off_ids, nb * sizeof(uint32_t), hipMemcpyHostToDevice, sc->stream));
    }
    if ((rc = radiance_on(sc, sc->rays.as<rtx_ray>(), ids ? sc->rad_ids.as<uint32_t>() : nullptr, (uint64_t)b0,
                          (int64_t)nb, prm, sc->rad_out.as<double>(), sc->rad_oseg.as<uint32_t>(), sc->stream, what)))
      return rc;
    HIPC(hipMemcpyAsync(pin + off_rgb, sc->rad_out.p, nb * 3 * sizeof(double), hipMemcpyDeviceToHost, sc->stream));
    if (out_segments)
      HIPC(hipMemcpyAsync(pin + off_seg, sc->rad_oseg.p, nb * sizeof(uint32_t), hipMemcpyDeviceToHost, sc->stream));
    HIPC(hipStreamSynchronize(sc->stream));
    std::memcpy(out_rgb + 3 * b0, pin + off_rgb, nb * 3 * sizeof(double));
    if (out_segments) std::memcpy(out_segments + b0, pin + off_seg, nb * sizeof(uint32_t));
  }
  return RTX_OK;
}
// the device entry points of the three families: the checks, then the chunks on the caller's stream
int radiance_device(rtx_scene* sc, const rtx_ray* d_rays, const uint32_t* d_ids, size_t n,
                    const rtx_radiance_params* prm, double* d_out_rgb, uint32_t* d_out_segments, void* stream,
                    SlotKind what) {
  int rc;
  if ((rc = radiance_check(sc, prm, d_rays, d_out_rgb))) return rc;
  if ((what == kSlotNee || what == kSlotMis) && (rc = nee_depth_check(prm->max_depth, what == kSlotMis))) return rc;
  if (n == 0) return RTX_OK;
  HIPC(hipSetDevice(sc->device));
  return radiance_on(sc, d_rays, d_ids, 0, (int64_t)n, prm, d_out_rgb, d_out_segments,
                     stream ? (hipStream_t)stream : sc->stream, what);
}
// What rtx_internal_irradiance_rays and rtx_internal_direct_samples share: the checks, the
// surfels and ids staged to the device, `launch(nslots, d_surfels, d_ids, d_out)` into the slot
// scratch (`per_slot` doubles per slot) and the copy back to the host.
template <class Launch>
int surfel_samples(rtx_scene* sc, const rtx_ray* surfels, const uint32_t* ids, size_t n, const rtx_radiance_params* prm,
                   double* out, size_t per_slot, const char* too_many, Launch launch, const char* bad_extra = nullptr) {
  int rc;
  if ((rc = radiance_check(sc, prm, surfels, out))) return rc;
  if (bad_extra) return fail(RTX_ERR_INVALID, bad_extra);  // (a hook's own argument, after the shared checks)
  if (n == 0) return RTX_OK;
  if (n > (size_t)kRadianceSlotsMax || (int64_t)n * prm->spp > kRadianceSlotsMax) return fail(RTX_ERR_INVALID, too_many);
  HIPC(hipSetDevice(sc->device));
  const uint32_t nslots = (uint32_t)(n * (size_t)prm->spp);
  const size_t bytes = (size_t)nslots * per_slot * sizeof(double);
  if ((rc = sc->rays.reserve(n * sizeof(rtx_ray)))) return rc;
  if ((rc = sc->rad_L.reserve(bytes))) return rc;
  if (ids && (rc = sc->rad_ids.reserve(n * sizeof(uint32_t)))) return rc;
  HIPC(hipMemcpyAsync(sc->rays.p, surfels, n * sizeof(rtx_ray), hipMemcpyHostToDevice, sc->stream));
  if (ids) HIPC(hipMemcpyAsync(sc->rad_ids.p, ids, n * sizeof(uint32_t), hipMemcpyHostToDevice, sc->stream));
  if ((rc = launch(nslots, sc->rays.as<rtx_ray>(), ids ? sc->rad_ids.as<uint32_t>() : nullptr, sc->rad_L.as<double>())))
    return rc;
  HIPC(hipMemcpyAsync(out, sc->rad_L.p, bytes, hipMemcpyDeviceToHost, sc->stream));
  HIPC(hipStreamSynchronize(sc->stream));
  return RTX_OK;
}
// ---- frames with next-event estimation (rtx_nee.h) ----
// What rtx_render_nee / rtx_render_mis and their _device forms do first: the checks in the
// documented order, then the empty subset (*npix == 0: the caller returns RTX_OK), then the output
// buffer, then the device.  rp: the render params read as the radiance family reads its own; the
// messages say "mis" where the NEE family's say "nee" (what: kSlotNee or kSlotMis).
int render_nee_begin(const rtx_scene* sc, const rtx_camera* cam, const rtx_render_params* prm, const void* out,
                     SlotKind what, NeeCamera& nc, int64_t* npix, rtx_radiance_params& rp) {
  const bool mis = what == kSlotMis;
  *npix = 0;
  if (!sc) return fail(RTX_ERR_INVALID, "scene is NULL");
  if (!cam || !prm) return fail(RTX_ERR_INVALID, "NULL argument");
  if (prm->spp < 1)
    return fail(RTX_ERR_INVALID, mis ? "render mis: spp must be at least 1" : "render nee: spp must be at least 1");
  if (prm->max_depth < 0) return fail(RTX_ERR_INVALID, "negative max_depth");
  int rc;
  if ((rc = nee_depth_check(prm->max_depth, mis))) return rc;
  if (prm->adaptive != 0)
    return fail(RTX_ERR_INVALID, mis ? "render mis: adaptive sampling is not supported (fixed spp only)"
                                     : "render nee: adaptive sampling is not supported (fixed spp only)");
  if (prm->precision != RTX_PREC_PARITY && prm->precision != RTX_PREC_FAST)
    return fail(RTX_ERR_INVALID, mis ? "render mis: bad precision" : "render nee: bad precision");
  std::string err;
  *npix = subset_pixels(cam, prm, nc.map, err);
  if (*npix < 0) return fail(RTX_ERR_INVALID, err);
  if (*npix == 0) return RTX_OK;
  if (!out) return fail(RTX_ERR_INVALID, "NULL buffer");
  HIPC(hipSetDevice(sc->device));
  nc.cam = *cam;
  rp.spp = prm->spp, rp.max_depth = prm->max_depth, rp.first_sample = 0, rp.precision = prm->precision;
  rp.seed = prm->seed;
  return RTX_OK;
}
// the frame entry points of the two families (what: kSlotNee or kSlotMis)
int render_nee_device(rtx_scene* sc, const rtx_camera* cam, const rtx_render_params* prm, double* d_out_rgb,
                      uint32_t* d_out_segments, void* stream, SlotKind what) {
  NeeCamera nc;
  int64_t npix;
  rtx_radiance_params rp{};
  int rc;
  if ((rc = render_nee_begin(sc, cam, prm, d_out_rgb, what, nc, &npix, rp)) || npix == 0) return rc;
  return radiance_on(sc, nullptr, nullptr, 0, npix, &rp, d_out_rgb, d_out_segments,
                     stream ? (hipStream_t)stream : sc->stream, what, &nc);
}
int render_nee_host(rtx_scene* sc, const rtx_camera* cam, const rtx_render_params* prm, double* out_rgb,
                    uint32_t* out_segments, SlotKind what) {
  NeeCamera nc;
  int64_t npix;
  rtx_radiance_params rp{};
  int rc;
  if ((rc = render_nee_begin(sc, cam, prm, out_rgb, what, nc, &npix, rp)) || npix == 0) return rc;
  if ((rc = sc->rad_out.reserve((size_t)npix * 3 * sizeof(double)))) return rc;
  if ((rc = sc->rad_oseg.reserve((size_t)npix * sizeof(uint32_t)))) return rc;
  if ((rc = radiance_on(sc, nullptr, nullptr, 0, npix, &rp, sc->rad_out.as<double>(), sc->rad_oseg.as<uint32_t>(),
                        sc->stream, what, &nc)))
    return rc;
  HIPC(hipMemcpyAsync(out_rgb, sc->rad_out.p, (size_t)npix * 3 * sizeof(double), hipMemcpyDeviceToHost, sc->stream));
  if (out_segments)
    HIPC(hipMemcpyAsync(out_segments, sc->rad_oseg.p, (size_t)npix * sizeof(uint32_t), hipMemcpyDeviceToHost, sc->stream));
  HIPC(hipStreamSynchronize(sc->stream));
  return RTX_OK;
}
// What rtx_internal_nee_trace and rtx_internal_mis_trace share (per: doubles per recorded segment,
// 9 or 11; the MIS form launches k_path_trace<.., true> and says "mis" in its messages).
int path_trace_hook(rtx_scene* sc, const rtx_ray* rays, const uint32_t* ids, size_t n, const rtx_radiance_params* prm,
                    int32_t cap, double* verts, uint32_t* flags, double* ends, uint32_t* counts, bool mis) {
  const size_t per = mis ? 11 : 9;
  int rc;
  if ((rc = radiance_check(sc, prm, rays, verts))) return rc;
  if ((rc = nee_depth_check(prm->max_depth, mis))) return rc;
  if (!flags || !ends || !counts) return fail(RTX_ERR_INVALID, "NULL buffer");
  if (cap < 1 || cap > 4096)
    return fail(RTX_ERR_INVALID, mis ? "mis trace: cap outside 1..4096" : "nee trace: cap outside 1..4096");
  if (n == 0) return RTX_OK;
  if (n > ((size_t)1 << 20) || (int64_t)n * prm->spp * cap > ((int64_t)1 << 22))
    return fail(RTX_ERR_INVALID,
                mis ? "mis trace: too many records for one call" : "nee trace: too many records for one call");
  HIPC(hipSetDevice(sc->device));
  const size_t nslots = n * (size_t)prm->spp, nrec = nslots * (size_t)cap;
  // doubles: verts | ends (rad_L); words: flags | counts (rad_segs)
  const size_t b_verts = nrec * per * sizeof(double), b_ends = nslots * 3 * sizeof(double);
  const size_t b_flags = nrec * sizeof(uint32_t), b_counts = nslots * 2 * sizeof(uint32_t);
  if ((rc = sc->rays.reserve(n * sizeof(rtx_ray)))) return rc;
  if ((rc = sc->rad_L.reserve(b_verts + b_ends))) return rc;
  if ((rc = sc->rad_segs.reserve(b_flags + b_counts))) return rc;
  if (ids && (rc = sc->rad_ids.reserve(n * sizeof(uint32_t)))) return rc;
  hipStream_t s = sc->stream;
  HIPC(hipMemcpyAsync(sc->rays.p, rays, n * sizeof(rtx_ray), hipMemcpyHostToDevice, s));
  if (ids) HIPC(hipMemcpyAsync(sc->rad_ids.p, ids, n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  HIPC(hipMemsetAsync(sc->rad_L.p, 0, b_verts + b_ends, s));
  HIPC(hipMemsetAsync(sc->rad_segs.p, 0, b_flags + b_counts, s));
  double* const d_verts = sc->rad_L.as<double>();
  double* const d_ends = d_verts + nrec * per;
  uint32_t* const d_flags = sc->rad_segs.as<uint32_t>();
  uint32_t* const d_counts = d_flags + nrec;
  RadianceChunk A;
  A.rays = sc->rays.as<rtx_ray>(), A.ids = ids ? sc->rad_ids.as<uint32_t>() : nullptr, A.ray0 = 0, A.id_base = 0;
  A.slots = (uint32_t)nslots, A.K = (uint32_t)prm->spp;
  A.s0 = prm->first_sample, A.max_depth = prm->max_depth, A.seed = prm->seed;
  A.L = nullptr, A.segs = nullptr;  // (not written by k_path_trace)
  if ((rc = with_walk(sc, prm->precision, [&](auto w) {
         using W = decltype(w);
         return with_flag(mis, [&](auto m) {
           return launch_1d(k_path_trace<W::stack, W::fast, decltype(m)::value>, (int64_t)nslots,
                            stack_lds_bytes(W::stack), s, sc->S, emitter_table(sc), A, cap, d_verts, d_flags, d_ends,
                            d_counts);
         });
       })))
    return rc;
  HIPC(hipMemcpyAsync(verts, d_verts, b_verts, hipMemcpyDeviceToHost, s));
  HIPC(hipMemcpyAsync(ends, d_ends, b_ends, hipMemcpyDeviceToHost, s));
  HIPC(hipMemcpyAsync(flags, d_flags, b_flags, hipMemcpyDeviceToHost, s));
  HIPC(hipMemcpyAsync(counts, d_counts, b_counts, hipMemcpyDeviceToHost, s));
  HIPC(hipStreamSynchronize(s));
  return RTX_OK;
}
// ---- light probes (rtx_probe.h) ----
// the checks rtx_probe_sh*, and up to the estimator rtx_internal_probe_rays, share, in the documented order
int probe_check(const rtx_scene* sc, const rtx_radiance_params* prm, const void* points, const void* out,
                int32_t estimator) {
  int rc;
  if ((rc = radiance_check(sc, prm, points, out))) return rc;
  if (estimator != 0 && estimator != RTX_ESTIMATOR_NEE && estimator != RTX_ESTIMATOR_MIS)
    return fail(RTX_ERR_INVALID, "probe: bad estimator");
  if (estimator != 0) return nee_depth_check(prm->max_depth, estimator == RTX_ESTIMATOR_MIS);
  return RTX_OK;
}
// n > 0 probes on device buffers, in radiance_on's chunks (whole probes per chunk, or, when one
// probe's samples exceed the cap, one probe at a time in runs of `cap` samples whose 27 partial
// sums and two counts k_probe_sum carries): k_probe into the slot scratch, then k_probe_sum.
int probe_on(rtx_scene* sc, const double* d_points, const uint32_t* d_ids, uint64_t id_base, int64_t n,
             const rtx_radiance_params* prm, int32_t estimator, double* d_sh, uint32_t* d_segs, uint32_t* d_back,
             hipStream_t s) {
  const int64_t cap = slot_cap();
  const int64_t spp = prm->spp;
  const int64_t probes_per = std::max<int64_t>(1, cap / spp);     // probes per chunk
  const int64_t k_per = std::min<int64_t>(spp, cap);              // samples of a probe per chunk
  const int64_t most = std::min<int64_t>(n, probes_per) * k_per;  // slots of the largest chunk (<= cap)
  int rc;
  if ((rc = sc->rad_L.reserve((size_t)most * 3 * sizeof(double)))) return rc;
  if ((rc = sc->rad_segs.reserve((size_t)most * sizeof(uint32_t)))) return rc;
  if (k_per < spp) {  // (one probe per chunk)
    if ((rc = sc->rad_carry.reserve(kProbeCarry * sizeof(double)))) return rc;
  }
  double* const carry = k_per < spp ? sc->rad_carry.as<double>() : nullptr;
  const EmitterTable E = emitter_table(sc);
  return with_walk(sc, prm->precision, [&](auto w) {
    using W = decltype(w);
    constexpr size_t lds = stack_lds_bytes(W::stack);
    for (int64_t r0 = 0; r0 < n; r0 += probes_per) {
      const int64_t nr = std::min<int64_t>(probes_per, n - r0);
      for (int64_t k0 = 0; k0 < spp; k0 += k_per) {
        const int64_t K = std::min<int64_t>(k_per, spp - k0);
        RadianceChunk A;
        A.rays = nullptr, A.ids = d_ids, A.ray0 = r0, A.id_base = id_base;  // (the points travel beside the chunk)
        A.slots = (uint32_t)(nr * K), A.K = (uint32_t)K;
        A.s0 = (int32_t)(prm->first_sample + k0), A.max_depth = prm->max_depth, A.seed = prm->seed;
        A.L = sc->rad_L.as<double>(), A.segs = sc->rad_segs.as<uint32_t>();
        if (estimator == 0) rc = launch_1d(k_probe<W::stack, W::fast, 0>, A.slots, lds, s, sc->S, E, A, d_points);
        else if (estimator == RTX_ESTIMATOR_NEE)
          rc = launch_1d(k_probe<W::stack, W::fast, RTX_ESTIMATOR_NEE>, A.slots, lds, s, sc->S, E, A, d_points);
        else rc = launch_1d(k_probe<W::stack, W::fast, RTX_ESTIMATOR_MIS>, A.slots, lds, s, sc->S, E, A, d_points);
        if (rc) return rc;
        if ((rc = launch_1d(k_probe_sum, nr, 0, s, A, d_points, nr, k0 == 0 ? 1 : 0, k0 + K == spp ? 1 : 0, prm->spp,
                            carry, d_sh + 3 * RTX_SH_COEFFS * r0, d_segs ? d_segs + r0 : nullptr,
                            d_back ? d_back + r0 : nullptr)))
          return rc;
      }
    }
    return (int)RTX_OK;
  });
}
// The host entry point works in batches of kProbeHostBatch probes, staged through pinned memory as
// radiance_host stages its rays (the points through `rays`, the coefficients through rad_out, the
// two counts through rad_oseg).
constexpr size_t kProbeHostBatch = (size_t)1 << 18;
int probe_host(rtx_scene* sc, const double* points, const uint32_t* ids, size_t n, const rtx_radiance_params* prm,
               int32_t estimator, double* out_sh, uint32_t* out_segments, uint32_t* out_backfaces) {
  int rc;
  if ((rc = probe_check(sc, prm, points, out_sh, estimator))) return rc;
  if (n == 0) return RTX_OK;
  HIPC(hipSetDevice(sc->device));
  constexpr size_t kSh = 3 * RTX_SH_COEFFS;
  const size_t m = std::min(n, kProbeHostBatch);
  // pinned: points | coefficients | ids | segments | back-faces (8-byte items first)
  const size_t off_sh = m * 3 * sizeof(double), off_ids = off_sh + m * kSh * sizeof(double),
               off_seg = off_ids + m * sizeof(uint32_t), off_back = off_seg + m * sizeof(uint32_t);
  if ((rc = sc->rad_host.reserve(off_back + m * sizeof(uint32_t)))) return rc;
  if ((rc = sc->rays.reserve(m * 3 * sizeof(double)))) return rc;
  if ((rc = sc->rad_out.reserve(m * kSh * sizeof(double)))) return rc;
  if ((rc = sc->rad_oseg.reserve(2 * m * sizeof(uint32_t)))) return rc;
  if (ids && (rc = sc->rad_ids.reserve(m * sizeof(uint32_t)))) return rc;
  char* const pin = (char*)sc->rad_host.p;
  uint32_t* const d_seg = sc->rad_oseg.as<uint32_t>();
  uint32_t* const d_back = d_seg + m;
  for (size_t b0 = 0; b0 < n; b0 += m) {
    const size_t nb = std::min(m, n - b0);
    std::memcpy(pin, points + 3 * b0, nb * 3 * sizeof(double));
    HIPC(hipMemcpyAsync(sc->rays.p, pin, nb * 3 * sizeof(double), hipMemcpyHostToDevice, sc->stream));
    if (ids) {
      std::memcpy(pin + off_ids, ids + b0, nb * sizeof(uint32_t));
      HIPC(hipMemcpyAsync(sc->rad_ids.p, pin + off_ids, nb * sizeof(uint32_t), hipMemcpyHostToDevice, sc->stream));
    }
    if ((rc = probe_on(sc, sc->rays.as<double>(), ids ? sc->rad_ids.as<uint32_t>() : nullptr, (uint64_t)b0, (int64_t)nb,
                       prm, estimator, sc->rad_out.as<double>(), d_seg, d_back, sc->stream)))
      return rc;
    HIPC(hipMemcpyAsync(pin + off_sh, sc->rad_out.p, nb * kSh * sizeof(double), hipMemcpyDeviceToHost, sc->stream));
    if (out_segments)
      HIPC(hipMemcpyAsync(pin + off_seg, d_seg, nb * sizeof(uint32_t), hipMemcpyDeviceToHost, sc->stream));
    if (out_backfaces)
      HIPC(hipMemcpyAsync(pin + off_back, d_back, nb * sizeof(uint32_t), hipMemcpyDeviceToHost, sc->stream));
    HIPC(hipStreamSynchronize(sc->stream));
    std::memcpy(out_sh + kSh * b0, pin + off_sh, nb * kSh * sizeof(double));
    if (out_segments) std::memcpy(out_segments + b0, pin + off_seg, nb * sizeof(uint32_t));
    if (out_backfaces) std::memcpy(out_backfaces + b0, pin + off_back, nb * sizeof(uint32_t));
  }
  return RTX_OK;
}
// ---- sampled films (rtx_film_sampled.h) ----
// the group sizes of the calls that follow (rtx_internal_film_group; 0: the defaults)
std::atomic<int32_t> g_film_group_first{0}, g_film_group_later{0};
// Samples per entry of an adaptive film's groups after the first: the reference tests after every
// sample, so at most kFilmGroup - 1 traced samples of a pixel are discarded.
constexpr int32_t kFilmGroup = 4;
}  // namespace

// A sampled film advanced to `budget`.  Fixed: samples [done, budget) of every pixel, in chunks
// under the slot cap (whole pixels per chunk, or one pixel's samples in runs), each traced and
// added in sample order.  Adaptive: every pixel still sampling holds the same count, so a group is
// G samples of every entry of the active list; an empty film starts with min(min_spp, budget)
// samples of every pixel (nothing can converge earlier), a film that holds samples with a pass of
// no samples that lists its unconverged pixels.  After each group the next list's count comes back
// through a pinned word (the next launch is sized by it), and the call ends when it is 0 or the
// budget is reached.
int film_sampled_render(rtx_film* f, int32_t budget, rtx_stats* stats) {
  rtx_scene* sc = f->sc;
  const int64_t npix = f->npix;
  const bool adaptive = f->prm.adaptive != 0;
  if (npix == 0 || (adaptive && f->active == 0)) return RTX_OK;
  HIPC(hipSetDevice(sc->device));
  hipStream_t s = sc->stream;
  const bool mis = f->estimator == RTX_ESTIMATOR_MIS;
  const int64_t cap = slot_cap();
  int rc;
  if ((rc = sc->fs_ctr.reserve(kFilmCtrWords * sizeof(unsigned long long)))) return rc;
  if ((rc = sc->fs_host.reserve(4 * sizeof(unsigned long long)))) return rc;
  unsigned long long* const ctr = sc->fs_ctr.as<unsigned long long>();
  uint32_t* const counts = (uint32_t*)(ctr + kFilmCtrTotals + 2);  // the two lists' counts
  volatile unsigned long long* const pin = (volatile unsigned long long*)sc->fs_host.p;
  HIPC(hipMemsetAsync(ctr, 0, kFilmCtrWords * sizeof(unsigned long long), s));
  AdaptWs& w = sc->aw;
  if (adaptive) {
    for (DevBuf* b : {&w.lst[0], &w.lst[1], &w.knext})
      if ((rc = b->reserve((size_t)npix * sizeof(uint32_t)))) return rc;
    if ((rc = w.pk.reserve((size_t)npix * sizeof(uint64_t)))) return rc;
    if ((rc = w.scan_tmp.reserve(rtxscan::temp_bytes_packed(npix)))) return rc;
  }
  const NeeCamera nc{f->cam, f->map};
  const EmitterTable E = emitter_table(sc);
  const PixelSoA px = f->px();
  // timing: the call between ev[0] and ev[1], each path launch between a pair of the pool
  const bool timed = stats != nullptr;
  size_t evi = 0;
  uint64_t slots_traced = 0, hot_launches = 0;
  if (timed) HIPC(hipEventRecord(sc->ev[0], s));
  FilmGroup A{};
  A.max_depth = f->prm.max_depth, A.seed = f->prm.seed, A.npix = (uint32_t)npix;
  FilmRecord R{};
  R.min_spp = f->prm.min_spp, R.budget = budget, R.rel = f->prm.rel_threshold;
  R.keep = adaptive ? w.knext.as<uint32_t>() : nullptr, R.ctr = ctr;
  // entries [A.e0, A.e0 + A.ne) of the group in A: traced into the slot scratch, then recorded
  auto launch = [&]() -> int {
    const int64_t slots = (int64_t)A.ne * A.G;
    if (slots > 0) {
      int r;
      if ((r = sc->rad_L.reserve((size_t)slots * 3 * sizeof(double)))) return r;
      if ((r = sc->rad_segs.reserve((size_t)slots * sizeof(uint32_t)))) return r;
      A.L = sc->rad_L.as<double>(), A.segs = sc->rad_segs.as<uint32_t>();
      hipEvent_t e0 = nullptr, e1 = nullptr;
      if (timed) {
        e0 = sc->pool_event(evi), e1 = sc->pool_event(evi + 1);
        if (!e0 || !e1) return fail(RTX_ERR_HIP, "hipEventCreate failed");
        evi += 2;
        HIPC(hipEventRecord(e0, s));
      }
      if ((r = with_walk(sc, f->prm.precision, [&](auto wk) {
             using W = decltype(wk);
             return with_flag(mis, [&](auto m) {
               return launch_1d(k_film_paths<W::stack, W::fast, decltype(m)::value>, slots, stack_lds_bytes(W::stack), s,
                                sc->S, E, nc, A);
             });
           })))
        return r;
      if (timed) HIPC(hipEventRecord(e1, s));
      slots_traced += (uint64_t)slots, hot_launches++;
    }
    if (adaptive) return launch_1d(k_film_record<true>, A.ne, 0, s, px, A, R);
    return launch_1d(k_film_record<false>, A.ne, 0, s, px, A, R);
  };
  if (!adaptive) {
    const int64_t todo = (int64_t)budget - f->done;
    const int64_t k_per = std::min<int64_t>(todo, cap), pix_per = std::max<int64_t>(1, cap / todo);
    A.list = nullptr, A.count = nullptr, A.bound = (uint32_t)npix;
    for (int64_t r0 = 0; r0 < npix; r0 += pix_per)
      for (int64_t k0 = 0; k0 < todo; k0 += k_per) {
        A.e0 = (uint32_t)r0, A.ne = (uint32_t)std::min<int64_t>(pix_per, npix - r0);
        A.G = (uint32_t)std::min<int64_t>(k_per, todo - k0), A.s0 = (int32_t)(f->done + k0);
        if ((rc = launch())) return rc;
      }
  } else {
    const int32_t g_first = g_film_group_first.load(), g_later = g_film_group_later.load();
    int cur = -1;                 // the list in use: w.lst[cur], or none yet (every pixel)
    int64_t n_active = npix;      // its entries, as the host knows them
    int32_t have = f->done;       // samples every entry of the list holds
    bool first = f->done == 0;
    // the group in A recorded over all its entries; then the next list and its count
    auto group = [&](int32_t G) -> int {
      const int64_t per = G > 0 ? std::max<int64_t>(1, cap / G) : n_active;
      A.list = cur < 0 ? nullptr : w.lst[cur].as<uint32_t>(), A.count = cur < 0 ? nullptr : counts + cur;
      A.bound = (uint32_t)n_active, A.G = (uint32_t)G, A.s0 = have;
      for (int64_t e0 = 0; e0 < n_active; e0 += per) {
        A.e0 = (uint32_t)e0, A.ne = (uint32_t)std::min<int64_t>(per, n_active - e0);
        int r;
        if ((r = launch())) return r;
      }
      const int nxt = cur == 0 ? 1 : 0;
      HIPC(rtxscan::exclusive_scan_packed(R.keep, w.pk.as<uint64_t>(), n_active, w.scan_tmp.p, w.scan_tmp.n, s));
      int r;
      if ((r = launch_1d(k_film_emit, n_active, 0, s, A.list, (const uint32_t*)R.keep, (const uint64_t*)w.pk.as<uint64_t>(),
                         (uint32_t)n_active, (uint32_t)npix, w.lst[nxt].as<uint32_t>(), counts + nxt)))
        return r;
      HIPC(hipMemcpyAsync((void*)(pin + 2), counts + nxt, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
      HIPC(hipStreamSynchronize(s));
      n_active = std::min<int64_t>((int64_t)(uint32_t)pin[2], n_active);  // (a list only shrinks)
      cur = nxt, have += G;
      return RTX_OK;
    };
    if (!first && (rc = group(0))) return rc;  // who is still sampling
    while (n_active > 0 && have < budget) {
      int32_t G = first ? (g_first > 0 ? g_first : std::max(1, f->prm.min_spp)) : (g_later > 0 ? g_later : kFilmGroup);
      G = (int32_t)std::min<int64_t>(std::min<int64_t>(G, budget - have), cap);
      if ((rc = group(G))) return rc;
      first = false;
    }
    // an empty list below the budget: every pixel has converged (at the budget the list is empty
    // either way, and who has converged is not known here)
    f->active = have < budget ? n_active : -1;
  }
  if (timed) {
    HIPC(hipEventRecord(sc->ev[1], s));
    hipLaunchKernelGGL(k_film_totals, dim3(1), dim3(64), 0, s, ctr);
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync((void*)pin, ctr + kFilmCtrTotals, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    float ms = 0;
    HIPC(hipEventElapsedTime(&ms, sc->ev[0], sc->ev[1]));
    double hot_ms = 0;
    if ((rc = sc->pool_pairs_ms(evi, hot_ms))) return rc;
    stats->paths = stats->rays_primary = slots_traced;
    stats->rays_total = pin[0], stats->rays_recorded = pin[1];
    stats->kernel_ms = ms, stats->hot_kernel_ms = hot_ms, stats->hot_launches = hot_launches;
  }
  return RTX_OK;
}

// The walk of rtx_intersect* / rtx_occluded*.  The fast walk clamps a box's entry distance at 0
// (visit_slabs), so it culls geometry behind the origin that a negative tmin asks for, and the f64
// slab test rejects every box on an empty range: such a query runs the parity walk, whatever
// precision it names (include/rtx.h).  A fast query's kernel sends single rays to the parity walk
// too (fast_query_domain, rtx_kernels.h), so its lanes get the deeper of the two stacks.
template <class F>
static int query_walk(const rtx_scene* sc, int32_t precision, double tmin, double tmax, F&& f) {
  const bool fast = precision == RTX_PREC_FAST && sc->fast_ok && tmin >= 0.0 && tmin < tmax;
  return with_walk(fast ? std::max(sc->stack_fast, sc->stack_parity) : sc->stack_parity, fast, f);
}

extern "C" {

int rtx_intersect_device(rtx_scene* sc, const rtx_ray* d_rays, size_t n, rtx_hit* d_hits, double tmin, double tmax,
                         int32_t precision, void* stream) {
  if (!sc) return fail(RTX_ERR_INVALID, "scene is NULL");
  if (n == 0) return RTX_OK;
  if (!d_rays || !d_hits) return fail(RTX_ERR_INVALID, "NULL buffer");
  HIPC(hipSetDevice(sc->device));
  hipStream_t s = stream ? (hipStream_t)stream : sc->stream;
  return query_walk(sc, precision, tmin, tmax, [&](auto w) {
    return launch_1d(k_intersect<w.stack, w.fast>, (int64_t)n, stack_lds_bytes(w.stack), s, sc->S, d_rays, (int64_t)n,
                     d_hits, tmin, tmax);
  });
}

int rtx_intersect(rtx_scene* sc, const rtx_ray* rays, size_t n, rtx_hit* hits, double tmin, double tmax,
                  int32_t precision) {
  if (!sc) return fail(RTX_ERR_INVALID, "scene is NULL");
  if (n == 0) return RTX_OK;
  if (!rays || !hits) return fail(RTX_ERR_INVALID, "NULL buffer");
  HIPC(hipSetDevice(sc->device));
  int rc;
  if ((rc = sc->rays.reserve(n * sizeof(rtx_ray)))) return rc;
  if ((rc = sc->hits.reserve(n * sizeof(rtx_hit)))) return rc;
  HIPC(hipMemcpyAsync(sc->rays.p, rays, n * sizeof(rtx_ray), hipMemcpyHostToDevice, sc->stream));
  if ((rc = rtx_intersect_device(sc, sc->rays.as<rtx_ray>(), n, sc->hits.as<rtx_hit>(), tmin, tmax, precision,
                                 sc->stream)))
    return rc;
  HIPC(hipMemcpyAsync(hits, sc->hits.p, n * sizeof(rtx_hit), hipMemcpyDeviceToHost, sc->stream));
  HIPC(hipStreamSynchronize(sc->stream));
  return RTX_OK;
}

int rtx_occluded_device(rtx_scene* sc, const rtx_ray* d_rays, size_t n, uint8_t* d_out, double tmin, double tmax,
                        int32_t precision, void* stream) {
  if (!sc) return fail(RTX_ERR_INVALID, "scene is NULL");
  if (!(tmin < tmax)) return fail(RTX_ERR_INVALID, "occluded: tmin must be below tmax");
  if (n == 0) return RTX_OK;
  if (!d_rays || !d_out) return fail(RTX_ERR_INVALID, "NULL buffer");
  HIPC(hipSetDevice(sc->device));
  hipStream_t s = stream ? (hipStream_t)stream : sc->stream;
  return query_walk(sc, precision, tmin, tmax, [&](auto w) {
    return launch_1d(k_occluded<w.stack, w.fast>, (int64_t)n, stack_lds_bytes(w.stack), s, sc->S, d_rays, (int64_t)n,
                     d_out, tmin, tmax);
  });
}

int rtx_occluded(rtx_scene* sc, const rtx_ray* rays, size_t n, uint8_t* out, double tmin, double tmax,
                 int32_t precision) {
  if (!sc) return fail(RTX_ERR_INVALID, "scene is NULL");
  if (!(tmin < tmax)) return fail(RTX_ERR_INVALID, "occluded: tmin must be below tmax");
  if (n == 0) return RTX_OK;
  if (!rays || !out) return fail(RTX_ERR_INVALID, "NULL buffer");
  HIPC(hipSetDevice(sc->device));
  int rc;
  if ((rc = sc->rays.reserve(n * sizeof(rtx_ray)))) return rc;
  if ((rc = sc->occ.reserve(n))) return rc;
  HIPC(hipMemcpyAsync(sc->rays.p, rays, n * sizeof(rtx_ray), hipMemcpyHostToDevice, sc->stream));
  if ((rc = rtx_occluded_device(sc, sc->rays.as<rtx_ray>(), n, sc->occ.as<uint8_t>(), tmin, tmax, precision, sc->stream)))
    return rc;
  HIPC(hipMemcpyAsync(out, sc->occ.p, n, hipMemcpyDeviceToHost, sc->stream));
  HIPC(hipStreamSynchronize(sc->stream));
  return RTX_OK;
}

int rtx_ao_device(rtx_scene* sc, const rtx_camera* cam, const rtx_render_params* prm, const rtx_ao_params* ao,
                  double* d_out, void* stream) {
  PixelMap map;
  int64_t npix;
  int rc;
  if ((rc = ao_check(sc, cam, prm, ao, map, &npix))) return rc;
  if (npix == 0) return RTX_OK;
  if (!d_out) return fail(RTX_ERR_INVALID, "NULL buffer");
  HIPC(hipSetDevice(sc->device));
  return ao_on(sc, cam, map, npix, prm->precision, ao, d_out, nullptr, stream ? (hipStream_t)stream : sc->stream);
}

int rtx_ao(rtx_scene* sc, const rtx_camera* cam, const rtx_render_params* prm, const rtx_ao_params* ao, double* out) {
  PixelMap map;
  int64_t npix;
  int rc;
  if ((rc = ao_check(sc, cam, prm, ao, map, &npix))) return rc;
  if (npix == 0) return RTX_OK;
  if (!out) return fail(RTX_ERR_INVALID, "NULL buffer");
  HIPC(hipSetDevice(sc->device));
  if ((rc = sc->aov_f64.reserve((size_t)npix * sizeof(double)))) return rc;  // (the AOV staging: one double per pixel)
  if ((rc = ao_on(sc, cam, map, npix, prm->precision, ao, sc->aov_f64.as<double>(), nullptr, sc->stream))) return rc;
  HIPC(hipMemcpyAsync(out, sc->aov_f64.p, (size_t)npix * sizeof(double), hipMemcpyDeviceToHost, sc->stream));
  HIPC(hipStreamSynchronize(sc->stream));
  return RTX_OK;
}

// Test hook (not in rtx.h): the sample rays of rtx_ao for the same arguments, npix * samples of
// them, pixel major, made by the device function k_ao calls (ao_direction after ao_first_hit,
// rtx_occlusion.h) and copied to the host; a pixel that misses has all-zero rays.
int rtx_internal_ao_rays(rtx_scene* sc, const rtx_camera* cam, const rtx_render_params* prm, const rtx_ao_params* ao,
                         rtx_ray* out) {
  PixelMap map;
  int64_t npix;
  int rc;
  if ((rc = ao_check(sc, cam, prm, ao, map, &npix))) return rc;
  if (npix == 0) return RTX_OK;
  if (!out) return fail(RTX_ERR_INVALID, "NULL buffer");
  HIPC(hipSetDevice(sc->device));
  const size_t bytes = (size_t)npix * (size_t)ao->samples * sizeof(rtx_ray);
  if ((rc = sc->rays.reserve(bytes))) return rc;
  if ((rc = ao_on(sc, cam, map, npix, prm->precision, ao, nullptr, sc->rays.as<rtx_ray>(), sc->stream))) return rc;
  HIPC(hipMemcpyAsync(out, sc->rays.p, bytes, hipMemcpyDeviceToHost, sc->stream));
  HIPC(hipStreamSynchronize(sc->stream));
  return RTX_OK;
}

int rtx_aov_device(rtx_scene* sc, const rtx_camera* cam, const rtx_render_params* prm, double* d_albedo,
                   double* d_normal, double* d_depth, void* stream) {
  if (!sc) return fail(RTX_ERR_INVALID, "scene is NULL");
  if (!cam || !prm) return fail(RTX_ERR_INVALID, "NULL argument");
  PixelMap map;
  std::string err;
  const int64_t npix = subset_pixels(cam, prm, map, err);
  if (npix < 0) return fail(RTX_ERR_INVALID, err);
  HIPC(hipSetDevice(sc->device));
  return aov_on(sc, cam, map, npix, prm->precision, d_albedo, d_normal, d_depth, stream ? (hipStream_t)stream : sc->stream);
}

int rtx_aov(rtx_scene* sc, const rtx_camera* cam, const rtx_render_params* prm, double* albedo, double* normal,
            double* depth) {
  if (!sc) return fail(RTX_ERR_INVALID, "scene is NULL");
  if (!cam || !prm) return fail(RTX_ERR_INVALID, "NULL argument");
  PixelMap map;
  std::string err;
  const int64_t npix = subset_pixels(cam, prm, map, err);
  if (npix < 0) return fail(RTX_ERR_INVALID, err);
  if (npix == 0) return RTX_OK;
  HIPC(hipSetDevice(sc->device));
  int rc;
  if ((rc = sc->aov_f64.reserve((size_t)npix * 7 * sizeof(double)))) return rc;
  double* a = sc->aov_f64.as<double>();  // albedo 3 n, normal 3 n, depth n
  double *n = a + 3 * npix, *d = a + 6 * npix;
  hipStream_t s = sc->stream;
  if ((rc = aov_on(sc, cam, map, npix, prm->precision, albedo ? a : nullptr, normal ? n : nullptr, depth ? d : nullptr, s)))
    return rc;
  if (albedo) HIPC(hipMemcpyAsync(albedo, a, (size_t)npix * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
  if (normal) HIPC(hipMemcpyAsync(normal, n, (size_t)npix * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
  if (depth) HIPC(hipMemcpyAsync(depth, d, (size_t)npix * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPC(hipStreamSynchronize(s));
  return RTX_OK;
}

int rtx_radiance_device(rtx_scene* sc, const rtx_ray* d_rays, const uint32_t* d_ids, size_t n,
                        const rtx_radiance_params* prm, double* d_out_rgb, uint32_t* d_out_segments, void* stream) {
  return radiance_device(sc, d_rays, d_ids, n, prm, d_out_rgb, d_out_segments, stream, kSlotRadiance);
}
int rtx_radiance(rtx_scene* sc, const rtx_ray* rays, const uint32_t* ids, size_t n, const rtx_radiance_params* prm,
                 double* out_rgb, uint32_t* out_segments) {
  return radiance_host(sc, rays, ids, n, prm, out_rgb, out_segments, kSlotRadiance);
}

// ---- irradiance queries (rtx_irradiance.h): rtx_radiance's checks, chunks and staging ----
int rtx_irradiance_device(rtx_scene* sc, const rtx_ray* d_surfels, const uint32_t* d_ids, size_t n,
                          const rtx_radiance_params* prm, double* d_out_rgb, uint32_t* d_out_segments, void* stream) {
  return radiance_device(sc, d_surfels, d_ids, n, prm, d_out_rgb, d_out_segments, stream, kSlotIrradiance);
}
int rtx_irradiance(rtx_scene* sc, const rtx_ray* surfels, const uint32_t* ids, size_t n,
                   const rtx_radiance_params* prm, double* out_rgb, uint32_t* out_segments) {
  return radiance_host(sc, surfels, ids, n, prm, out_rgb, out_segments, kSlotIrradiance);
}

// Test hook (not in rtx.h): the depth-0 segments rtx_irradiance traces for the same arguments
// (seed, first_sample and spp of prm are read; the rest is checked as there), n x spp x 6
// doubles (origin, direction), surfel major, made by the device function k_irradiance calls
// (irradiance_ray, rtx_irradiance.h); all zero for a surfel with a degenerate normal.  Host
// buffers.
int rtx_internal_irradiance_rays(rtx_scene* sc, const rtx_ray* surfels, const uint32_t* ids, size_t n,
                                 const rtx_radiance_params* prm, double* out) {
  return surfel_samples(sc, surfels, ids, n, prm, out, 6, "irradiance rays: too many rays for one call",
                        [&](uint32_t nslots, const rtx_ray* d_surfels, const uint32_t* d_ids, double* d_out) {
                          return launch_1d(k_irradiance_rays, nslots, 0, sc->stream, d_surfels, d_ids, nslots,
                                           (uint32_t)prm->spp, prm->seed, prm->first_sample, d_out);
                        });
}

// ---- direct-lighting queries (rtx_direct.h): rtx_radiance's checks, chunks and staging ----
int rtx_direct_device(rtx_scene* sc, const rtx_ray* d_surfels, const uint32_t* d_ids, size_t n,
                      const rtx_radiance_params* prm, double* d_out_rgb, uint32_t* d_out_visible, void* stream) {
  return radiance_device(sc, d_surfels, d_ids, n, prm, d_out_rgb, d_out_visible, stream, kSlotDirect);
}
int rtx_direct(rtx_scene* sc, const rtx_ray* surfels, const uint32_t* ids, size_t n, const rtx_radiance_params* prm,
               double* out_rgb, uint32_t* out_visible) {
  return radiance_host(sc, surfels, ids, n, prm, out_rgb, out_visible, kSlotDirect);
}

int rtx_scene_emitters(const rtx_scene* sc, int64_t* count, double* area) {
  if (!sc) return fail(RTX_ERR_INVALID, "scene is NULL");
  if (!count && !area) return fail(RTX_ERR_INVALID, "NULL argument");
  const int64_t n = (int64_t)sc->emit_idx.size();
  if (count) *count = n;
  if (area) {
    *area = 0.0;
    if (n > 0) {
      HIPC(hipSetDevice(sc->device));
      HIPC(hipStreamSynchronize(sc->stream));
      HIPC(hipMemcpy(area, sc->emit_cum.as<double>() + (n - 1), sizeof(double), hipMemcpyDeviceToHost));
    }
  }
  return RTX_OK;
}

// Test hook (not in rtx.h): the samples rtx_direct draws for the same arguments (seed,
// first_sample and spp of prm are read; the rest is checked as there), n x spp x 9 doubles
// (segment origin, y - x, the unshadowed contribution C), surfel major, made by the device
// function k_direct calls (direct_sample, through k_emitter_samples, rtx_direct.h); all zero where nothing is traced.  Host
// buffers.
int rtx_internal_direct_samples(rtx_scene* sc, const rtx_ray* surfels, const uint32_t* ids, size_t n,
                                const rtx_radiance_params* prm, double* out) {
  return surfel_samples(sc, surfels, ids, n, prm, out, 9, "direct samples: too many samples for one call",
                        [&](uint32_t nslots, const rtx_ray* d_surfels, const uint32_t* d_ids, double* d_out) {
                          return launch_1d(k_emitter_samples, nslots, 0, sc->stream, sc->S, emitter_table(sc), d_surfels,
                                           d_ids, nslots, (uint32_t)prm->spp, prm->seed, prm->first_sample,
                                           kRngStreamDirect, d_out);
                        });
}

// Test hook (not in rtx.h): the live emitter table copied back after everything queued on the
// scene's stream, at most `cap` entries: each emitter's primitive index (the caller's own order,
// as rtx_scene_update_prims counts it) and the inclusive cumulative areas.  Either may be NULL.
int rtx_internal_emitters(rtx_scene* sc, int64_t* prims_out, double* cum_out, int64_t cap) {
  if (!sc) return fail(RTX_ERR_INVALID, "scene is NULL");
  const int64_t n = std::min<int64_t>(std::max<int64_t>(0, cap), (int64_t)sc->emit_idx.size());
  if (n == 0) return RTX_OK;
  if (prims_out)
    for (int64_t i = 0; i < n; i++) prims_out[i] = (int64_t)sc->emit_idx[(size_t)i];
  if (cum_out) {
    HIPC(hipSetDevice(sc->device));
    HIPC(hipStreamSynchronize(sc->stream));
    HIPC(hipMemcpy(cum_out, sc->emit_cum.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  }
  return RTX_OK;
}

// ---- next-event estimation (rtx_nee.h): rtx_radiance's checks, chunks and staging ----
int rtx_radiance_nee_device(rtx_scene* sc, const rtx_ray* d_rays, const uint32_t* d_ids, size_t n,
                            const rtx_radiance_params* prm, double* d_out_rgb, uint32_t* d_out_segments,
                            void* stream) {
  return radiance_device(sc, d_rays, d_ids, n, prm, d_out_rgb, d_out_segments, stream, kSlotNee);
}
int rtx_radiance_nee(rtx_scene* sc, const rtx_ray* rays, const uint32_t* ids, size_t n, const rtx_radiance_params* prm,
                     double* out_rgb, uint32_t* out_segments) {
  return radiance_host(sc, rays, ids, n, prm, out_rgb, out_segments, kSlotNee);
}

int rtx_render_nee_device(rtx_scene* sc, const rtx_camera* cam, const rtx_render_params* prm, double* d_out_rgb,
                          uint32_t* d_out_segments, void* stream) {
  return render_nee_device(sc, cam, prm, d_out_rgb, d_out_segments, stream, kSlotNee);
}
int rtx_render_nee(rtx_scene* sc, const rtx_camera* cam, const rtx_render_params* prm, double* out_rgb,
                   uint32_t* out_segments) {
  return render_nee_host(sc, cam, prm, out_rgb, out_segments, kSlotNee);
}

// ---- the power-heuristic form (rtx_nee.h, MIS): the NEE family's checks, chunks and staging ----
int rtx_radiance_mis_device(rtx_scene* sc, const rtx_ray* d_rays, const uint32_t* d_ids, size_t n,
                            const rtx_radiance_params* prm, double* d_out_rgb, uint32_t* d_out_segments,
                            void* stream) {
  return radiance_device(sc, d_rays, d_ids, n, prm, d_out_rgb, d_out_segments, stream, kSlotMis);
}
int rtx_radiance_mis(rtx_scene* sc, const rtx_ray* rays, const uint32_t* ids, size_t n, const rtx_radiance_params* prm,
                     double* out_rgb, uint32_t* out_segments) {
  return radiance_host(sc, rays, ids, n, prm, out_rgb, out_segments, kSlotMis);
}
int rtx_render_mis_device(rtx_scene* sc, const rtx_camera* cam, const rtx_render_params* prm, double* d_out_rgb,
                          uint32_t* d_out_segments, void* stream) {
  return render_nee_device(sc, cam, prm, d_out_rgb, d_out_segments, stream, kSlotMis);
}
int rtx_render_mis(rtx_scene* sc, const rtx_camera* cam, const rtx_render_params* prm, double* out_rgb,
                   uint32_t* out_segments) {
  return render_nee_host(sc, cam, prm, out_rgb, out_segments, kSlotMis);
}

// ---- light probes (rtx_probe.h): rtx_radiance's checks, then the estimator's; its chunks and staging ----
int rtx_probe_sh_device(rtx_scene* sc, const double* d_points, const uint32_t* d_ids, size_t n,
                        const rtx_radiance_params* prm, int32_t estimator, double* d_out_sh, uint32_t* d_out_segments,
                        uint32_t* d_out_backfaces, void* stream) {
  int rc;
  if ((rc = probe_check(sc, prm, d_points, d_out_sh, estimator))) return rc;
  if (n == 0) return RTX_OK;
  HIPC(hipSetDevice(sc->device));
  return probe_on(sc, d_points, d_ids, 0, (int64_t)n, prm, estimator, d_out_sh, d_out_segments, d_out_backfaces,
                  stream ? (hipStream_t)stream : sc->stream);
}
int rtx_probe_sh(rtx_scene* sc, const double* points, const uint32_t* ids, size_t n, const rtx_radiance_params* prm,
                 int32_t estimator, double* out_sh, uint32_t* out_segments, uint32_t* out_backfaces) {
  return probe_host(sc, points, ids, n, prm, estimator, out_sh, out_segments, out_backfaces);
}

// Test hook (not in rtx.h): the depth-0 segments rtx_probe_sh traces for the same arguments (seed,
// first_sample and spp of prm are read; the rest is checked as rtx_radiance's), n x spp x 6
// doubles (origin, direction), probe major, made by the device function k_probe and k_probe_sum
// call (probe_ray, rtx_probe.h); all zero for a probe with a non-finite coordinate.  Host buffers.
int rtx_internal_probe_rays(rtx_scene* sc, const double* points, const uint32_t* ids, size_t n,
                            const rtx_radiance_params* prm, double* out) {
  int rc;
  if ((rc = radiance_check(sc, prm, points, out))) return rc;
  if (n == 0) return RTX_OK;
  if (n > (size_t)kRadianceSlotsMax || (int64_t)n * prm->spp > kRadianceSlotsMax)
    return fail(RTX_ERR_INVALID, "probe rays: too many rays for one call");
  HIPC(hipSetDevice(sc->device));
  const uint32_t nslots = (uint32_t)(n * (size_t)prm->spp);
  const size_t bytes = (size_t)nslots * 6 * sizeof(double);
  if ((rc = sc->rays.reserve(n * 3 * sizeof(double)))) return rc;
  if ((rc = sc->rad_L.reserve(bytes))) return rc;
  if (ids && (rc = sc->rad_ids.reserve(n * sizeof(uint32_t)))) return rc;
  HIPC(hipMemcpyAsync(sc->rays.p, points, n * 3 * sizeof(double), hipMemcpyHostToDevice, sc->stream));
  if (ids) HIPC(hipMemcpyAsync(sc->rad_ids.p, ids, n * sizeof(uint32_t), hipMemcpyHostToDevice, sc->stream));
  if ((rc = launch_1d(k_probe_rays, nslots, 0, sc->stream, (const double*)sc->rays.as<double>(),
                      (const uint32_t*)(ids ? sc->rad_ids.as<uint32_t>() : nullptr), nslots, (uint32_t)prm->spp,
                      prm->seed, prm->first_sample, sc->rad_L.as<double>())))
    return rc;
  HIPC(hipMemcpyAsync(out, sc->rad_L.p, bytes, hipMemcpyDeviceToHost, sc->stream));
  HIPC(hipStreamSynchronize(sc->stream));
  return RTX_OK;
}

// Test hook (not in rtx.h): rtx_internal_direct_samples on stream kRngStreamNee + depth, the
// samples a path of rtx_radiance_nee draws at a vertex of that depth (k_emitter_samples, rtx_direct.h);
// depth outside 0 .. 0x00FFFFFE is RTX_ERR_INVALID after the shared checks.  Host buffers.
int rtx_internal_nee_samples(rtx_scene* sc, const rtx_ray* surfels, const uint32_t* ids, size_t n,
                             const rtx_radiance_params* prm, int32_t depth, double* out) {
  return surfel_samples(
      sc, surfels, ids, n, prm, out, 9, "nee samples: too many samples for one call",
      [&](uint32_t nslots, const rtx_ray* d_surfels, const uint32_t* d_ids, double* d_out) {
        return launch_1d(k_emitter_samples, nslots, 0, sc->stream, sc->S, emitter_table(sc), d_surfels, d_ids, nslots,
                         (uint32_t)prm->spp, prm->seed, prm->first_sample, kRngStreamNee + (uint32_t)depth, d_out);
      },
      depth < 0 || depth >= 0x00FFFFFF ? "nee samples: depth outside 0..16777214" : nullptr);
}

// Test hook (not in rtx.h): the paths of rtx_radiance_nee for the same rays, keys and params, one
// slot per (ray, sample), ray major, from the device function its kernel runs (nee_path through
// k_path_trace, rtx_nee.h).  Per slot and segment d < cap: verts 9 doubles (vertex point, shading
// normal, w = thr * rho; zero on a miss, w zero where no term is eligible) and one flag word
// (1 term eligible, 2 sample traced, 4 visible, 8 the path ended here on an emitter whose emission
// is suppressed); segments a path does not reach stay zero.  Per slot: ends 3 doubles (L_end) and
// counts 2 uint32 (closest-hit segments, shadow segments traced).  cap in 1..4096.  Host buffers.
int rtx_internal_nee_trace(rtx_scene* sc, const rtx_ray* rays, const uint32_t* ids, size_t n,
                           const rtx_radiance_params* prm, int32_t cap, double* verts, uint32_t* flags, double* ends,
                           uint32_t* counts) {
  return path_trace_hook(sc, rays, ids, n, prm, cap, verts, flags, ends, counts, false);
}

// Test hook (not in rtx.h): rtx_internal_nee_trace for the paths of rtx_radiance_mis (k_path_trace's MIS
// form, rtx_nee.h).  verts holds 11 doubles per slot and segment: the nine of rtx_internal_nee_trace,
// then g of the vertex's light sample (0 where none was traceable) and the gb applied to the
// segment's emission (0 where none applied).  Flag 8 is never set; 16: the path ended here on an
// emitter of the table and its emission was weighted with gb.  Messages say "mis".
int rtx_internal_mis_trace(rtx_scene* sc, const rtx_ray* rays, const uint32_t* ids, size_t n,
                           const rtx_radiance_params* prm, int32_t cap, double* verts, uint32_t* flags, double* ends,
                           uint32_t* counts) {
  return path_trace_hook(sc, rays, ids, n, prm, cap, verts, flags, ends, counts, true);
}

// Test hook (not in rtx.h): one shading step per case (rtx_shade_steps.h), n ShadeCase in and n
// ShadeRecord out, host buffers.  variant: 0 shade(); 1 shade_terminal (a case that does not end
// on the sky gets cont = -1); 2 the scatter-API branch; 8 + bits: shade_core + shade_finish with
// bit 0 LAMB, bit 1 NOTEX, bit 2 SET_ORIGIN = false (the hook sets the origin, as k_persistent
// does).  A LAMB / NOTEX form on a scene whose flags do not allow it, and a material or primitive
// index outside the scene's tables, are RTX_ERR_INVALID: nothing is launched.
int rtx_internal_shade_steps(rtx_scene* sc, const void* cases, size_t n, int32_t variant, void* out) {
  if (!sc) return fail(RTX_ERR_INVALID, "scene is NULL");
  if (!cases || !out) return fail(RTX_ERR_INVALID, "NULL buffer");
  if (!((variant >= 0 && variant <= 2) || (variant >= 8 && variant <= 15)))
    return fail(RTX_ERR_INVALID, "shade steps: unknown variant");
  if (n == 0) return RTX_OK;
  if (n > (size_t)kRadianceSlots) return fail(RTX_ERR_INVALID, "shade steps: too many cases for one call");
  const bool lamb = variant >= 8 && (variant & 1), notex = variant >= 8 && (variant & 2);
  if (lamb && !sc->S.all_lambertian) return fail(RTX_ERR_INVALID, "shade steps: the scene is not all Lambertian");
  if (notex && !sc->S.no_textures) return fail(RTX_ERR_INVALID, "shade steps: the scene reads textures");
  const ShadeCase* cs = (const ShadeCase*)cases;
  for (size_t i = 0; i < n; i++) {
    if (cs[i].hit && (cs[i].mat < 0 || cs[i].mat >= sc->n_materials))
      return fail(RTX_ERR_INVALID, "shade steps: material index out of range");
    if (cs[i].lazy_uv < -1 || cs[i].lazy_uv >= sc->S.n_prims)
      return fail(RTX_ERR_INVALID, "shade steps: primitive index out of range");
  }
  HIPC(hipSetDevice(sc->device));
  int rc;
  if ((rc = sc->rays.reserve(n * sizeof(ShadeCase)))) return rc;
  if ((rc = sc->hits.reserve(n * sizeof(ShadeRecord)))) return rc;
  HIPC(hipMemcpyAsync(sc->rays.p, cases, n * sizeof(ShadeCase), hipMemcpyHostToDevice, sc->stream));
  const ShadeCase* d_in = sc->rays.as<ShadeCase>();
  ShadeRecord* d_out = sc->hits.as<ShadeRecord>();
  auto run = [&](auto kernel) { return launch_1d(kernel, (int64_t)n, 0, sc->stream, sc->S, d_in, (int64_t)n, d_out); };
  switch (variant) {
    case 0: rc = run(k_shade_steps<kShadeFormShade>); break;
    case 1: rc = run(k_shade_steps<kShadeFormTerminal>); break;
    case 2: rc = run(k_shade_steps<kShadeFormScatter>); break;
    case 8: rc = run(k_shade_steps<kShadeFormCore, false, false, true>); break;
    case 9: rc = run(k_shade_steps<kShadeFormCore, true, false, true>); break;
    case 10: rc = run(k_shade_steps<kShadeFormCore, false, true, true>); break;
    case 11: rc = run(k_shade_steps<kShadeFormCore, true, true, true>); break;
    case 12: rc = run(k_shade_steps<kShadeFormCore, false, false, false>); break;
    case 13: rc = run(k_shade_steps<kShadeFormCore, true, false, false>); break;
    case 14: rc = run(k_shade_steps<kShadeFormCore, false, true, false>); break;
    default: rc = run(k_shade_steps<kShadeFormCore, true, true, false>);
  }
  if (rc) return rc;
  HIPC(hipMemcpyAsync(out, sc->hits.p, n * sizeof(ShadeRecord), hipMemcpyDeviceToHost, sc->stream));
  HIPC(hipStreamSynchronize(sc->stream));
  return RTX_OK;
}

// Test hook (not in rtx.h): the slot cap of the radiance calls that follow in this process
// (0 restores kRadianceSlots), so chunk seams are reached at small shapes.  Results never
// depend on it.
int rtx_internal_radiance_chunk(int64_t slots) {
  if (slots < 0) return fail(RTX_ERR_INVALID, "radiance chunk: negative slot count");
  g_radiance_chunk.store(slots);
  return RTX_OK;
}

// Test hook (not in rtx.h): the samples per entry of an adaptive sampled film's first group (on
// an empty film) and of its later groups, for the rtx_film_render calls that follow in this
// process (0 restores min_spp and kFilmGroup).  Results never depend on them.
int rtx_internal_film_group(int32_t first, int32_t later) {
  if (first < 0 || later < 0) return fail(RTX_ERR_INVALID, "film group: negative group size");
  g_film_group_first.store(first), g_film_group_later.store(later);
  return RTX_OK;
}

}  // extern "C"
