// renderer.cc — GpuRayIntegrator, WavefrontRenderer and MegaKernel over the C ABI.
#include <fstream>
#include <iterator>
#include <stdexcept>

#include "rt/material.h"
#include "rt/renderer.h"

namespace rt::integrator {

namespace {
void check(int rc, const char* what) {
  if (rc != RTX_OK) throw std::runtime_error(std::string(what) + ": " + rtx_last_error());
}
}  // namespace

GpuRayIntegrator::GpuRayIntegrator(const scene::Scene* world, int device, int precision)
    : world_(world), device_(device), precision_(precision) {
  if (!world_) throw std::invalid_argument("GpuRayIntegrator: world is null");
  flat_ = scene::Flatten(*world_);
  const rtx_scene_desc d = flat_.desc();
  check(rtx_scene_create(device_, &d, &dev_), "rtx_scene_create");
}

GpuRayIntegrator::~GpuRayIntegrator() { rtx_scene_destroy(dev_); }

void GpuRayIntegrator::UpdatePrims(int64_t first, const std::vector<rtx_prim>& prims) {
  check(rtx_scene_update_prims(dev_, first, (int64_t)prims.size(), prims.data()), "rtx_scene_update_prims");
}

// cpu_ray_integrator.h:18-46 contract on the GPU: [0.001f, +inf), hit flag per record,
// HitRecord::mat re-attached from the material id.
void GpuRayIntegrator::IntersectBatch(const std::vector<core::Ray>& rays, std::vector<geom::HitRecord>& hits) const {
  hits.resize(rays.size());
  if (rays.empty()) return;
  std::vector<rtx_ray> r(rays.size());
  for (size_t i = 0; i < rays.size(); i++)
    for (int k = 0; k < 3; k++) r[i].origin[k] = rays[i].origin()[k], r[i].direction[k] = rays[i].direction()[k];
  std::vector<rtx_hit> h(rays.size());
  check(rtx_intersect(dev_, r.data(), r.size(), h.data(), RTX_SEAM_TMIN, core::kInfinity, precision_),
        "rtx_intersect");
  for (size_t i = 0; i < rays.size(); i++) {
    geom::HitRecord& o = hits[i];
    o.hit = h[i].hit != 0;
    if (!o.hit) {
      o.mat.reset();
      continue;
    }
    o.t = h[i].t;
    o.p = core::Point3(h[i].p[0], h[i].p[1], h[i].p[2]);
    o.normal = core::Vec3(h[i].normal[0], h[i].normal[1], h[i].normal[2]);
    o.front_face = h[i].front_face != 0;
    o.u = h[i].u, o.v = h[i].v;
    o.mat = flat_.material_ptrs.at(h[i].material);
  }
}

// Any-hit on (0.001f, tmax): out[i] = 1 iff IntersectBatch would set hits[i].hit with that far
// end (rtx_occluded).  A segment a -> b: Ray(a, b - a), tmax 1.
void GpuRayIntegrator::OccludedBatch(const std::vector<core::Ray>& rays, std::vector<uint8_t>& out, double tmax) const {
  out.resize(rays.size());
  if (rays.empty()) return;
  std::vector<rtx_ray> r(rays.size());
  for (size_t i = 0; i < rays.size(); i++)
    for (int k = 0; k < 3; k++) r[i].origin[k] = rays[i].origin()[k], r[i].direction[k] = rays[i].direction()[k];
  check(rtx_occluded(dev_, r.data(), r.size(), out.data(), RTX_SEAM_TMIN, tmax, precision_), "rtx_occluded");
}

// The cosine-weighted mean radiance arriving at each point about its normal (rtx_irradiance).
void GpuRayIntegrator::IrradianceBatch(const std::vector<core::Point3>& points, const std::vector<core::Vec3>& normals,
                                       std::vector<core::Vec3>& out, int samples, int max_depth, uint64_t seed,
                                       const std::vector<uint32_t>* ids, int first_sample,
                                       std::vector<uint32_t>* segments) const {
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
  check(rtx_irradiance(dev_, s.data(), ids ? ids->data() : nullptr, s.size(), &p, rgb.data(),
                       segments ? segments->data() : nullptr),
        "rtx_irradiance");
  for (size_t i = 0; i < points.size(); i++) out[i] = core::Vec3(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]);
}

// The radiance about each point as 9 x 3 SH coefficients (rtx_probe_sh).
void GpuRayIntegrator::ProbeBatch(const std::vector<core::Point3>& points, std::vector<double>& sh, int samples,
                                  int max_depth, uint64_t seed, int estimator, const std::vector<uint32_t>* ids,
                                  int first_sample, std::vector<uint32_t>* segments,
                                  std::vector<uint32_t>* backfaces) const {
  sh.assign(3 * RTX_SH_COEFFS * points.size(), 0.0);
  if (segments) segments->resize(points.size());
  if (backfaces) backfaces->resize(points.size());
  if (points.empty()) return;
  if (ids && ids->size() != points.size()) throw std::invalid_argument("ProbeBatch: one id per point");
  std::vector<double> p3(3 * points.size());
  for (size_t i = 0; i < points.size(); i++)
    for (int k = 0; k < 3; k++) p3[3 * i + k] = points[i][k];
  rtx_radiance_params p{};
  p.spp = samples, p.max_depth = max_depth, p.first_sample = first_sample, p.precision = precision_, p.seed = seed;
  check(rtx_probe_sh(dev_, p3.data(), ids ? ids->data() : nullptr, points.size(), &p, estimator, sh.data(),
                     segments ? segments->data() : nullptr, backfaces ? backfaces->data() : nullptr),
        "rtx_probe_sh");
}

// The light reaching each point straight from the scene's emitters (rtx_direct).
void GpuRayIntegrator::DirectBatch(const std::vector<core::Point3>& points, const std::vector<core::Vec3>& normals,
                                   std::vector<core::Vec3>& out, int samples, uint64_t seed,
                                   const std::vector<uint32_t>* ids, int first_sample,
                                   std::vector<uint32_t>* visible) const {
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
  check(rtx_direct(dev_, s.data(), ids ? ids->data() : nullptr, s.size(), &p, rgb.data(),
                   visible ? visible->data() : nullptr),
        "rtx_direct");
  for (size_t i = 0; i < points.size(); i++) out[i] = core::Vec3(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]);
}

}  // namespace rt::integrator

namespace rt::renderer {

rtx_render_params DefaultParams(int spp, int max_depth) {
  rtx_render_params p{};
  p.spp = spp;
  p.max_depth = max_depth;
  p.adaptive = 1;
  p.min_spp = 16;                        // wavefront.cc:43
  p.rel_threshold = (double)0.05f;       // wavefront.cc:42 (const float)
  p.seed = 1234;
  // the persistent schedule gives the same pixels as the bounce-synchronous wavefront one
  // (same per-path RNG streams, same per-pixel accumulation order) and is the fast kernel
  p.mode = RTX_MODE_PERSISTENT;
  p.precision = RTX_PREC_PARITY;
  return p;
}

WavefrontRenderer::WavefrontRenderer(const scene::Scene& w, const scene::Camera& c, integrator::RayIntegrator& i,
                                     int max_depth, int max_samples, int /*batch_size*/)
    : world(w), cam(c), integrator(i), params_(DefaultParams(max_samples, max_depth)) {}

WavefrontRenderer::~WavefrontRenderer() {
  for (rtx_scene* s : extra_) rtx_scene_destroy(s);
}

void WavefrontRenderer::set_devices(const std::vector<int>& devices, int stripe_rows) {
  // devices[0] renders through the integrator's own scene: it must be the integrator's device
  // (a list without it would leave a listed device unused).  A device may appear more than
  // once: each entry gets its own scene copy, thread and stream (rtx_render_multi).
  auto* gpu = dynamic_cast<integrator::GpuRayIntegrator*>(&integrator);
  const int own = gpu ? gpu->device() : 0;
  if (!devices.empty() && devices[0] != own)
    throw std::invalid_argument("WavefrontRenderer::set_devices: the first device must be the integrator's (device " +
                                std::to_string(own) + ")");
  for (rtx_scene* s : extra_) rtx_scene_destroy(s);
  extra_.clear();
  devices_ = devices;
  stripe_rows_ = stripe_rows > 0 ? stripe_rows : 8;
}

void WavefrontRenderer::set_gpus(int n) {
  int count = 0;
  if (rtx_device_count(&count) != RTX_OK) throw std::runtime_error(std::string("rtx_device_count: ") + rtx_last_error());
  if (n < 1 || n > count) throw std::invalid_argument("WavefrontRenderer::set_gpus: " + std::to_string(n) +
                                                      " GPUs requested, " + std::to_string(count) + " present");
  auto* gpu = dynamic_cast<integrator::GpuRayIntegrator*>(&integrator);
  const int first = gpu ? gpu->device() : 0;
  std::vector<int> d{first};
  for (int k = 0; (int)d.size() < n; k++)
    if (k != first) d.push_back(k);
  set_devices(d, stripe_rows_);
}

void WavefrontRenderer::Render() { Render(std::cout); }

void WavefrontRenderer::Render(std::ostream& out) {
  auto* gpu = dynamic_cast<integrator::GpuRayIntegrator*>(&integrator);
  if (!gpu)
    throw std::invalid_argument(
        "WavefrontRenderer (MI355X): the integrator must be a GpuRayIntegrator; shading runs on the device");
  const rtx_camera& dc = cam.device();
  if (dc.image_width <= 0) throw std::invalid_argument("WavefrontRenderer: camera not initialised");
  rtx_render_params p = params_;
  p.x0 = p.y0 = p.w = p.h = 0;
  p.stripe_rows = 0;
  const int64_t n = (int64_t)dc.image_width * dc.image_height;
  rgb_.assign(3 * n, 0.0);
  spp_.assign(n, 0);
  // wavefront.cc:238-241: the P3 text is formatted on the device (rtx_render_p3)
  if (chunks_ > 0 || !checkpoint_.empty() || !resume_.empty() || estimator_ != 0) {
    if (devices_.size() > 1)
      throw std::invalid_argument(
          "WavefrontRenderer: set_progressive / set_checkpoint / set_resume / set_estimator render through one film "
          "on one device; not with set_devices / set_gpus");
    RenderFilm(gpu, p, out);
    return;
  }
  if (denoise_ && devices_.size() <= 1) {  // the film keeps the variance an adaptive frame is filtered with
    RenderFilm(gpu, p, out);
    return;
  }
  std::string bytes(rtx_p3_max_bytes(dc.image_width, dc.image_height), '\0');
  size_t len = 0;
  if (devices_.size() > 1) {  // one frame over several devices, gathered on the host
    if (extra_.empty()) {
      const rtx_scene_desc d = gpu->flat().desc();
      for (size_t k = 1; k < devices_.size(); k++) {
        rtx_scene* s = nullptr;
        if (rtx_scene_create(devices_[k], &d, &s) != RTX_OK)
          throw std::runtime_error(std::string("rtx_scene_create: ") + rtx_last_error());
        extra_.push_back(s);
      }
    }
    std::vector<rtx_scene*> all{gpu->device_scene()};
    all.insert(all.end(), extra_.begin(), extra_.end());
    p.stripe_rows = stripe_rows_, p.stripe_index = 0, p.stripe_count = 0;
    if (rtx_render_multi(all.data(), (int32_t)all.size(), &dc, &p, rgb_.data(), spp_.data(), &stats_, nullptr) != RTX_OK)
      throw std::runtime_error(std::string("rtx_render_multi: ") + rtx_last_error());
    const double* frame = rgb_.data();
    std::vector<double> clean;
    if (denoise_) {  // the gathered frame, with the whole image's AOVs from the first device
      rtx_render_params whole = p;
      whole.stripe_rows = 0;
      std::vector<double> alb(3 * n), nrm(3 * n), dep(n);
      clean.resize(3 * n);
      if (rtx_aov(all[0], &dc, &whole, alb.data(), nrm.data(), dep.data()) != RTX_OK ||
          rtx_denoise(all[0], dc.image_width, dc.image_height, rgb_.data(), alb.data(), nrm.data(), dep.data(), nullptr,
                      nullptr, clean.data()) != RTX_OK)
        throw std::runtime_error(std::string("rtx_denoise: ") + rtx_last_error());
      frame = clean.data();
    }
    if (rtx_encode_p3(all[0], frame, dc.image_width, dc.image_height, bytes.data(), bytes.size(), &len) != RTX_OK)
      throw std::runtime_error(std::string("rtx_encode_p3: ") + rtx_last_error());
    out.write(bytes.data(), (std::streamsize)len);
    return;
  }
  if (rtx_render_p3(gpu->device_scene(), &dc, &p, bytes.data(), bytes.size(), &len, rgb_.data(), spp_.data(), &stats_) != RTX_OK)
    throw std::runtime_error(std::string("rtx_render_p3: ") + rtx_last_error());
  out.write(bytes.data(), (std::streamsize)len);
}

// The frame through a film: optionally from a saved state, in chunks with a preview after each,
// the state saved at the end.  The output equals the one-shot frame's (rtx_film_render).
void WavefrontRenderer::RenderFilm(integrator::GpuRayIntegrator* gpu, const rtx_render_params& p, std::ostream& out) {
  const rtx_camera& dc = cam.device();
  struct Owner {
    rtx_film* f = nullptr;
    ~Owner() { rtx_film_destroy(f); }
  } film;
  if (estimator_ != 0) {
    if (rtx_film_create_sampled(gpu->device_scene(), &dc, &p, estimator_, &film.f) != RTX_OK)
      throw std::runtime_error(std::string("rtx_film_create_sampled: ") + rtx_last_error());
  } else if (rtx_film_create(gpu->device_scene(), &dc, &p, &film.f) != RTX_OK)
    throw std::runtime_error(std::string("rtx_film_create: ") + rtx_last_error());
  if (!resume_.empty()) {
    std::ifstream in(resume_, std::ios::binary);
    if (!in) throw std::runtime_error("cannot read " + resume_);
    const std::string blob((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    if (rtx_film_load(film.f, blob.data(), blob.size()) != RTX_OK)
      throw std::runtime_error(resume_ + ": " + rtx_last_error());
  }
  std::string bytes(rtx_p3_max_bytes(dc.image_width, dc.image_height), '\0');
  size_t len = 0;
  auto p3 = [&] {
    const int rc = denoise_ ? rtx_film_denoise_p3(film.f, nullptr, bytes.data(), bytes.size(), &len)
                            : rtx_film_p3(film.f, bytes.data(), bytes.size(), &len);
    if (rc != RTX_OK) throw std::runtime_error(std::string(denoise_ ? "rtx_film_denoise_p3: " : "rtx_film_p3: ") + rtx_last_error());
  };
  const int chunks = chunks_ > 0 ? chunks_ : 1;
  stats_ = rtx_stats{};
  for (int k = 1; k <= chunks; k++) {
    const int budget = (int)(((int64_t)k * p.spp + chunks - 1) / chunks);  // ceil(k spp / chunks)
    rtx_stats st{};
    if (rtx_film_render(film.f, budget, &st) != RTX_OK)
      throw std::runtime_error(std::string("rtx_film_render: ") + rtx_last_error());
    stats_.rays_primary += st.rays_primary, stats_.rays_total += st.rays_total, stats_.paths += st.paths;
    stats_.kernel_ms += st.kernel_ms, stats_.hot_kernel_ms += st.hot_kernel_ms, stats_.hot_launches += st.hot_launches;
    stats_.rays_recorded += st.rays_recorded;
    if (st.hot_launches) stats_.build = st.build, stats_.parked = st.parked, stats_.node_bytes = st.node_bytes;
    if (preview_ && k < chunks) {
      p3();
      preview_(budget, bytes.substr(0, len));
    }
  }
  if (rtx_film_resolve(film.f, rgb_.data(), spp_.data()) != RTX_OK)
    throw std::runtime_error(std::string("rtx_film_resolve: ") + rtx_last_error());
  p3();
  if (preview_) preview_(p.spp, bytes.substr(0, len));
  if (!checkpoint_.empty()) {
    std::string blob(rtx_film_state_bytes(film.f), '\0');
    size_t n = 0;
    if (rtx_film_save(film.f, blob.data(), blob.size(), &n) != RTX_OK)
      throw std::runtime_error(std::string("rtx_film_save: ") + rtx_last_error());
    std::ofstream o(checkpoint_, std::ios::binary);
    o.write(blob.data(), (std::streamsize)n);
    if (!o) throw std::runtime_error("cannot write " + checkpoint_);
  }
  out.write(bytes.data(), (std::streamsize)len);
}

MegaKernel::MegaKernel(scene::Scene& scene, scene::Camera& camera, integrator::Sampler& sampler, int device)
    : sampler_(sampler), world_(scene), cam_(camera), device_(device) {}

void MegaKernel::Render() { Render(std::cout); }

void MegaKernel::Render(std::ostream& out) {
  cam_.Initialize();  // mega_kernel.h:16
  integrator::GpuRayIntegrator gpu(&world_, device_);
  const rtx_camera& dc = cam_.device();
  rtx_render_params p = DefaultParams(sampler_.num_samples(), cam_.max_depth_);
  p.adaptive = 0;
  if (auto* a = dynamic_cast<const integrator::AdaptiveSampler*>(&sampler_)) {
    p.adaptive = 1;
    p.min_spp = a->min_samples();
    p.rel_threshold = (double)a->threshold();
  }
  p.mode = RTX_MODE_MEGAKERNEL;
  p.seed = seed_;
  rtx_stats st{};
  rgb_.assign(3 * (size_t)dc.image_width * dc.image_height, 0.0);
  std::string bytes(rtx_p3_max_bytes(dc.image_width, dc.image_height), '\0');
  size_t len = 0;
  if (rtx_render_p3(gpu.device_scene(), &dc, &p, bytes.data(), bytes.size(), &len, rgb_.data(), nullptr, &st) != RTX_OK)
    throw std::runtime_error(std::string("rtx_render_p3: ") + rtx_last_error());
  out.write(bytes.data(), (std::streamsize)len);
}

}  // namespace rt::renderer
