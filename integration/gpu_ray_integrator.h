// gpu_ray_integrator.h — reference-side file (add as src/integrator/gpu_ray_integrator.h of
// Luke-TS/3360-ray-tracer): a drop-in for CPURayIntegrator (cpu_ray_integrator.h:13-50) whose
// IntersectBatch runs on the MI355X through the C ABI (include/rtx.h).  With it, main.cc:190
// becomes `integrator::GpuRayIntegrator integrator(&world);` and the reference's own
// WavefrontRenderer::Render keeps its CPU shading loop (hybrid mode).
#pragma once

#include <stdexcept>
#include <string>
#include <vector>

#include "core/interval.h"
#include "integrator/ray_integrator.h"
#include "rtx.h"
#include "rtx_flatten.h"

namespace rt::integrator {

class GpuRayIntegrator : public RayIntegrator {
 public:
  explicit GpuRayIntegrator(const scene::Scene* world, int device = 0, int precision = RTX_PREC_PARITY)
      : flat_(Flatten(*world)), precision_(precision) {
    const rtx_scene_desc d = flat_.desc();
    if (rtx_scene_create(device, &d, &dev_) != RTX_OK)
      throw std::runtime_error(std::string("rtx_scene_create: ") + rtx_last_error());
  }
  ~GpuRayIntegrator() { rtx_scene_destroy(dev_); }  // RayIntegrator has no virtual destructor
  GpuRayIntegrator(const GpuRayIntegrator&) = delete;
  GpuRayIntegrator& operator=(const GpuRayIntegrator&) = delete;

  // cpu_ray_integrator.h:18-46: hits resized to rays.size(), interval [0.001f, +inf), rec.hit
  // set for every ray, HitRecord::mat re-attached from the material id
  void IntersectBatch(const std::vector<core::Ray>& rays, std::vector<geom::HitRecord>& hits) const override {
    hits.resize(rays.size());
    if (rays.empty()) return;
    std::vector<rtx_ray> r(rays.size());
    for (size_t i = 0; i < rays.size(); i++)
      for (int k = 0; k < 3; k++) r[i].origin[k] = rays[i].origin()[k], r[i].direction[k] = rays[i].direction()[k];
    std::vector<rtx_hit> h(rays.size());
    if (rtx_intersect(dev_, r.data(), r.size(), h.data(), RTX_SEAM_TMIN, core::kInfinity, precision_) != RTX_OK)
      throw std::runtime_error(std::string("rtx_intersect: ") + rtx_last_error());
    for (size_t i = 0; i < rays.size(); i++) {
      geom::HitRecord& o = hits[i];
      o.hit = h[i].hit != 0;
      if (!o.hit) continue;
      o.t = h[i].t;
      o.p = core::Point3(h[i].p[0], h[i].p[1], h[i].p[2]);
      o.normal = core::Vec3(h[i].normal[0], h[i].normal[1], h[i].normal[2]);
      o.front_face = h[i].front_face != 0;
      o.u = h[i].u, o.v = h[i].v;
      o.mat = flat_.mat_ptrs[h[i].material];
    }
  }

  // Occlusion (any-hit) query on the same fixed tmin: out[i] = 1 iff some primitive is hit on
  // (0.001f, tmax), i.e. iff IntersectBatch with that far end would set hits[i].hit
  // (rtx_occluded: stops at the first primitive hit, one byte per ray).  A segment a -> b is
  // Ray(a, b - a) with tmax 1.  Not virtual: the reference's interface has no such call.
  void OccludedBatch(const std::vector<core::Ray>& rays, std::vector<uint8_t>& out,
                     double tmax = core::kInfinity) const {
    out.resize(rays.size());
    if (rays.empty()) return;
    std::vector<rtx_ray> r(rays.size());
    for (size_t i = 0; i < rays.size(); i++)
      for (int k = 0; k < 3; k++) r[i].origin[k] = rays[i].origin()[k], r[i].direction[k] = rays[i].direction()[k];
    if (rtx_occluded(dev_, r.data(), r.size(), out.data(), RTX_SEAM_TMIN, tmax, precision_) != RTX_OK)
      throw std::runtime_error(std::string("rtx_occluded: ") + rtx_last_error());
  }

  // Radiance query: out[i] = the mean of spp paths started from rays[i] as their depth-0 segment
  // and traced and shaded on the device as WavefrontRenderer does (rtx_radiance: fixed sampling,
  // random numbers keyed by (seed, ids ? ids[i] : i, first_sample + k)); segments, if given, the
  // segments traced per ray.  Not virtual: the reference's interface has no such call.
  void RadianceBatch(const std::vector<core::Ray>& rays, std::vector<core::Vec3>& out, int spp, int max_depth,
                     uint64_t seed, const std::vector<uint32_t>* ids = nullptr, int first_sample = 0,
                     std::vector<uint32_t>* segments = nullptr) const {
    out.resize(rays.size());
    if (segments) segments->resize(rays.size());
    if (rays.empty()) return;
    if (ids && ids->size() != rays.size()) throw std::invalid_argument("RadianceBatch: one id per ray");
    std::vector<rtx_ray> r(rays.size());
    for (size_t i = 0; i < rays.size(); i++)
      for (int k = 0; k < 3; k++) r[i].origin[k] = rays[i].origin()[k], r[i].direction[k] = rays[i].direction()[k];
    rtx_radiance_params p{};
    p.spp = spp, p.max_depth = max_depth, p.first_sample = first_sample, p.precision = precision_, p.seed = seed;
    std::vector<double> rgb(3 * rays.size());
    if (rtx_radiance(dev_, r.data(), ids ? ids->data() : nullptr, r.size(), &p, rgb.data(),
                     segments ? segments->data() : nullptr) != RTX_OK)
      throw std::runtime_error(std::string("rtx_radiance: ") + rtx_last_error());
    for (size_t i = 0; i < rays.size(); i++) out[i] = core::Vec3(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]);
  }

  // Radiance query with next-event estimation: RadianceBatch's arguments, paths and keys, with one
  // emitter sample (DirectBatch's) added at every vertex where a Lambertian scattered, and no
  // emission collected right after such a vertex (rtx_radiance_nee).  The same expectation with
  // far less variance where lights are small; without emitters the same values.  segments, if
  // given: closest-hit plus shadow segments per ray.  max_depth above 0x00FFFFFF throws.  Not
  // virtual: the reference's interface has no such call.
  void RadianceNeeBatch(const std::vector<core::Ray>& rays, std::vector<core::Vec3>& out, int spp, int max_depth,
                        uint64_t seed, const std::vector<uint32_t>* ids = nullptr, int first_sample = 0,
                        std::vector<uint32_t>* segments = nullptr) const {
    out.resize(rays.size());
    if (segments) segments->resize(rays.size());
    if (rays.empty()) return;
    if (ids && ids->size() != rays.size()) throw std::invalid_argument("RadianceNeeBatch: one id per ray");
    std::vector<rtx_ray> r(rays.size());
    for (size_t i = 0; i < rays.size(); i++)
      for (int k = 0; k < 3; k++) r[i].origin[k] = rays[i].origin()[k], r[i].direction[k] = rays[i].direction()[k];
    rtx_radiance_params p{};
    p.spp = spp, p.max_depth = max_depth, p.first_sample = first_sample, p.precision = precision_, p.seed = seed;
    std::vector<double> rgb(3 * rays.size());
    if (rtx_radiance_nee(dev_, r.data(), ids ? ids->data() : nullptr, r.size(), &p, rgb.data(),
                         segments ? segments->data() : nullptr) != RTX_OK)
      throw std::runtime_error(std::string("rtx_radiance_nee: ") + rtx_last_error());
    for (size_t i = 0; i < rays.size(); i++) out[i] = core::Vec3(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]);
  }

  // Radiance query with multiple importance sampling: RadianceNeeBatch's arguments, paths, emitter
  // samples and segment counts, with the power heuristic's weights on both strategies
  // (rtx_radiance_mis): each emitter sample counts 1 / (1 + g^2) of its value, and an emitter hit
  // right after a diffuse vertex the complementary share instead of nothing (all of it for a light
  // the emitter table does not hold).  The same expectation, without RadianceNeeBatch's fireflies
  // where a surface comes close to a light.  Not virtual: the reference's interface has no such call.
  void RadianceMisBatch(const std::vector<core::Ray>& rays, std::vector<core::Vec3>& out, int spp, int max_depth,
                        uint64_t seed, const std::vector<uint32_t>* ids = nullptr, int first_sample = 0,
                        std::vector<uint32_t>* segments = nullptr) const {
    out.resize(rays.size());
    if (segments) segments->resize(rays.size());
    if (rays.empty()) return;
    if (ids && ids->size() != rays.size()) throw std::invalid_argument("RadianceMisBatch: one id per ray");
    std::vector<rtx_ray> r(rays.size());
    for (size_t i = 0; i < rays.size(); i++)
      for (int k = 0; k < 3; k++) r[i].origin[k] = rays[i].origin()[k], r[i].direction[k] = rays[i].direction()[k];
    rtx_radiance_params p{};
    p.spp = spp, p.max_depth = max_depth, p.first_sample = first_sample, p.precision = precision_, p.seed = seed;
    std::vector<double> rgb(3 * rays.size());
    if (rtx_radiance_mis(dev_, r.data(), ids ? ids->data() : nullptr, r.size(), &p, rgb.data(),
                         segments ? segments->data() : nullptr) != RTX_OK)
      throw std::runtime_error(std::string("rtx_radiance_mis: ") + rtx_last_error());
    for (size_t i = 0; i < rays.size(); i++) out[i] = core::Vec3(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]);
  }

  // Irradiance query: out[i] = the cosine-weighted mean radiance arriving at points[i] over the
  // hemisphere about normals[i] (any positive finite length), from `samples` paths per point
  // traced and shaded as RadianceBatch does (rtx_irradiance: directions keyed by (seed,
  // ids ? ids[i] : i, first_sample + k)); pi times it is the radiometric irradiance, and a
  // Lambertian texel multiplies it by its albedo.  A zero or non-finite normal gives 0 0 0.
  // Not virtual: the reference's interface has no such call.
  void IrradianceBatch(const std::vector<core::Point3>& points, const std::vector<core::Vec3>& normals,
                       std::vector<core::Vec3>& out, int samples, int max_depth, uint64_t seed,
                       const std::vector<uint32_t>* ids = nullptr, int first_sample = 0,
                       std::vector<uint32_t>* segments = nullptr) const {
    if (normals.size() != points.size()) throw std::invalid_argument("IrradianceBatch: one normal per point");
    out.resize(points.size());
    if (segments) segments->resize(points.size());
    if (points.empty()) return;
    if (ids && ids->size() != points.size()) throw std::invalid_argument("IrradianceBatch: one id per point");
    std::vector<rtx_ray> s(points.size());
    for (size_t i = 0; i < points.size(); i++)
      for (int k = 0; k < 3; k++) s[i].origin[k] = points[i][k], s[i].direction[k] = normals[i][k];
    rtx_radiance_params p{};
    p.spp = samples, p.max_depth = max_depth, p.first_sample = first_sample, p.precision = precision_, p.seed = seed;
    std::vector<double> rgb(3 * points.size());
    if (rtx_irradiance(dev_, s.data(), ids ? ids->data() : nullptr, s.size(), &p, rgb.data(),
                       segments ? segments->data() : nullptr) != RTX_OK)
      throw std::runtime_error(std::string("rtx_irradiance: ") + rtx_last_error());
    for (size_t i = 0; i < points.size(); i++) out[i] = core::Vec3(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]);
  }

  // Direct-lighting query: out[i] = the light reaching points[i] straight from the scene's
  // emitters, in IrradianceBatch's unit (the two add), from `samples` points per surfel drawn
  // uniformly over the emitting area and weighted by the geometry term and the visibility of the
  // shadow segment (rtx_direct: keyed by (seed, ids ? ids[i] : i, first_sample + k)).  A zero or
  // non-finite normal, and a scene without emitters, give 0 0 0.  visible, if given: the
  // unoccluded samples per point.  Not virtual: the reference's interface has no such call.
  void DirectBatch(const std::vector<core::Point3>& points, const std::vector<core::Vec3>& normals,
                   std::vector<core::Vec3>& out, int samples, uint64_t seed,
                   const std::vector<uint32_t>* ids = nullptr, int first_sample = 0,
                   std::vector<uint32_t>* visible = nullptr) const {
    if (normals.size() != points.size()) throw std::invalid_argument("DirectBatch: one normal per point");
    out.resize(points.size());
    if (visible) visible->resize(points.size());
    if (points.empty()) return;
    if (ids && ids->size() != points.size()) throw std::invalid_argument("DirectBatch: one id per point");
    std::vector<rtx_ray> s(points.size());
    for (size_t i = 0; i < points.size(); i++)
      for (int k = 0; k < 3; k++) s[i].origin[k] = points[i][k], s[i].direction[k] = normals[i][k];
    rtx_radiance_params p{};
    p.spp = samples, p.max_depth = 0, p.first_sample = first_sample, p.precision = precision_, p.seed = seed;
    std::vector<double> rgb(3 * points.size());
    if (rtx_direct(dev_, s.data(), ids ? ids->data() : nullptr, s.size(), &p, rgb.data(),
                   visible ? visible->data() : nullptr) != RTX_OK)
      throw std::runtime_error(std::string("rtx_direct: ") + rtx_last_error());
    for (size_t i = 0; i < points.size(); i++) out[i] = core::Vec3(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]);
  }

  rtx_scene* device_scene() const { return dev_; }
  const RtxScene& flat() const { return flat_; }

 private:
  RtxScene flat_;
  int precision_;
  rtx_scene* dev_ = nullptr;
};

}  // namespace rt::integrator
