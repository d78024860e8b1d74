// rt/integrator.h — the batch closest-hit seam (mirrors the reference's
// src/integrator/ray_integrator.h:30-37, ray_state.h, pixel_state.h, sampler.h).
#pragma once

#include <memory>
#include <vector>

#include "rt/core.h"
#include "rt/geom.h"
#include "rt/scene.h"
#include "rtx.h"

namespace rt::integrator {

struct RayState {  // ray_state.h:8-13
  core::Ray r;
  int pixel_index = 0;
  int depth = 0;
  core::Color throughput = core::Color(1, 1, 1);
};

struct PixelState {  // pixel_state.h:13-19 (the GPU keeps the same fields per pixel)
  core::Color sum, mean, m2;
  int samples = 0;
  bool converged = false;
};

class RayIntegrator {  // ray_integrator.h:30-37
 public:
  virtual ~RayIntegrator() = default;
  virtual void IntersectBatch(const std::vector<core::Ray>& rays, std::vector<geom::HitRecord>& hits) const = 0;
};

// Drop-in replacement for CPURayIntegrator (cpu_ray_integrator.h:13-50): same contract
// (hits resized to rays.size(), interval [0.001f, +inf), HitRecord::mat re-attached from
// the material id) computed by rtx_intersect on the MI355X.  Holds a non-owning pointer to
// the world like the reference; the device copy is made on construction.
class GpuRayIntegrator : public RayIntegrator {
 public:
  explicit GpuRayIntegrator(const scene::Scene* world, int device = 0, int precision = RTX_PREC_PARITY);
  ~GpuRayIntegrator() override;
  GpuRayIntegrator(const GpuRayIntegrator&) = delete;
  GpuRayIntegrator& operator=(const GpuRayIntegrator&) = delete;
  void IntersectBatch(const std::vector<core::Ray>& rays, std::vector<geom::HitRecord>& hits) const override;
  // Occlusion (any-hit) query beside IntersectBatch, on the same fixed tmin: out[i] = 1 iff some
  // primitive is hit on (0.001f, tmax), i.e. iff IntersectBatch with that far end reports a hit
  // (rtx_occluded: stops at the first primitive hit, one byte per ray).  Not part of the
  // reference's RayIntegrator interface.
  void OccludedBatch(const std::vector<core::Ray>& rays, std::vector<uint8_t>& out,
                     double tmax = core::kInfinity) const;
  // Irradiance query: out[i] = the cosine-weighted mean radiance arriving at points[i] over the
  // hemisphere about normals[i] (any positive finite length), from `samples` paths per point
  // traced and shaded on the device (rtx_irradiance: directions keyed by (seed, ids ? ids[i] : i,
  // first_sample + k)); pi times it is the radiometric irradiance.  A zero or non-finite normal
  // gives 0 0 0.  segments, if given: the segments traced per point.  Not part of the reference's
  // RayIntegrator interface.
  void IrradianceBatch(const std::vector<core::Point3>& points, const std::vector<core::Vec3>& normals,
                       std::vector<core::Vec3>& out, int samples, int max_depth, uint64_t seed,
                       const std::vector<uint32_t>* ids = nullptr, int first_sample = 0,
                       std::vector<uint32_t>* segments = nullptr) const;
  // Direct-lighting query: out[i] = the light reaching points[i] straight from the scene's
  // emitters, in IrradianceBatch's unit, from `samples` points per surfel drawn uniformly over the
  // emitting area and weighted by the geometry term and the shadow segment's visibility
  // (rtx_direct: keyed by (seed, ids ? ids[i] : i, first_sample + k)).  A zero or non-finite
  // normal, and a scene without emitters, give 0 0 0.  visible, if given: the unoccluded samples
  // per point.  Not part of the reference's RayIntegrator interface.
  void DirectBatch(const std::vector<core::Point3>& points, const std::vector<core::Vec3>& normals,
                   std::vector<core::Vec3>& out, int samples, uint64_t seed,
                   const std::vector<uint32_t>* ids = nullptr, int first_sample = 0,
                   std::vector<uint32_t>* visible = nullptr) const;
  // Light probes: sh[27 * i + 3 * j + c] = coefficient j, channel c of the radiance arriving at
  // points[i] over the whole sphere, projected onto the real SH basis to band 2, from `samples`
  // paths per point in uniform directions (rtx_probe_sh: keyed by (seed, ids ? ids[i] : i,
  // first_sample + k); estimator 0, RTX_ESTIMATOR_NEE or RTX_ESTIMATOR_MIS).  A non-finite point
  // gives zeros.  segments / backfaces, if given: per point the segments traced and the samples
  // whose first segment hit a primitive from inside.  rtx_sh_eval evaluates a probe's 27 doubles.
  // Not part of the reference's RayIntegrator interface.
  void ProbeBatch(const std::vector<core::Point3>& points, std::vector<double>& sh, int samples, int max_depth,
                  uint64_t seed, int estimator = 0, const std::vector<uint32_t>* ids = nullptr, int first_sample = 0,
                  std::vector<uint32_t>* segments = nullptr, std::vector<uint32_t>* backfaces = nullptr) const;
  rtx_scene* device_scene() const { return dev_; }
  // Replace primitives [first, first + prims.size()) of the device copy, in its own order (leaf
  // order for a BVH world), and refit its trees in place (rtx_scene_update_prims): kinds stay,
  // geometry must be finite.  flat() stays the description the copy was created from.  Throws std::runtime_error on a refused update.
  void UpdatePrims(int64_t first, const std::vector<rtx_prim>& prims);
  const scene::FlatScene& flat() const { return flat_; }
  int device() const { return device_; }
  int precision() const { return precision_; }

 private:
  const scene::Scene* world_;
  scene::FlatScene flat_;
  rtx_scene* dev_ = nullptr;
  int device_, precision_;
};

// Samplers (sampler.h): configuration of the MegaKernel renderer on the GPU.
class Sampler {
 public:
  virtual ~Sampler() = default;
  virtual int num_samples() const = 0;
};
class DefaultSampler : public Sampler {  // sampler.h:22-37
 public:
  explicit DefaultSampler(int n) : n_(n) {}
  int num_samples() const override { return n_; }

 private:
  int n_;
};
// sampler.h:44-82: per pixel until the relative error of the running sums drops below
// `threshold` (after min_samples), at most max_samples + 1 samples.
class AdaptiveSampler : public Sampler {
 public:
  AdaptiveSampler(int min_samples, int max_samples, float threshold)
      : min_samples_(min_samples), max_samples_(max_samples), threshold_(threshold) {}
  int num_samples() const override { return max_samples_; }
  int min_samples() const { return min_samples_; }
  float threshold() const { return threshold_; }

 private:
  int min_samples_, max_samples_;
  float threshold_;
};

}  // namespace rt::integrator
