// raytracer — CLI drop-in for the reference binary (main.cc:158-197):
//   raytracer [camera-preset] [--scene cornell|three|final|bunny|mixed|<file.rtxs>]
//             [--cameras cameras.json] [--spp N] [--depth N] [--seed S] [--fixed]
//             [--mode wavefront|persistent|megakernel] [--precision parity|fast]
//             [--mk-adaptive MIN:THRESHOLD] [--gpus N]
//             [--chunks N] [--preview PREFIX] [--checkpoint FILE] [--resume FILE] [--denoise]
//             [--ao N[,RADIUS]] [--irradiance N[,DEPTH]] [--direct N] [--nee | --mis] [--adaptive] > out.ppm
//             [--probes NX,NY,NZ[,SPP]] > probes.txt
// --gpus N renders one frame over N GPUs (interleaved row stripes, one host thread per GPU,
// one gathered framebuffer and P3 output; identical pixels for every N); --devices 0,2,3
// names the devices (a device may repeat: several streams on one GPU).
// --chunks N renders the frame in N steps (budgets ceil(k * spp / N)) through a film;
// --preview PREFIX writes PREFIX_<budget>.ppm after each step; --checkpoint FILE saves the
// film's state at the end and --resume FILE continues from a saved state (same scene, camera,
// seed, depth and sampling).  The PPM on stdout is byte-identical to the plain run at the same
// spp.  One GPU, wavefront / persistent modes.
// --denoise filters the PPM on stdout and every preview with the edge-avoiding denoiser at its
// default parameters (first-hit albedo / normal / depth guides; an adaptive frame's own variance);
// without it the bytes are those of the plain run.  Wavefront / persistent modes.
// --ao N[,RADIUS] writes the ambient-occlusion pass instead of a render (rtx_ao: N cosine-weighted
// any-hit rays of length RADIUS from each pixel's first hit; default RADIUS a quarter of the
// scene's bounding-box diagonal) as a grey P3 PPM, AO replicated into R, G and B, through the
// device encoder; --seed and --precision apply.  Without the flag no output changes.
// --irradiance N[,DEPTH] writes the irradiance pass instead of a render (rtx_irradiance: at each
// pixel's first hit, the cosine-weighted mean of the radiance of N paths of at most DEPTH bounces
// over the hemisphere about the hit's normal, keyed by the global pixel; default DEPTH the
// preset's max depth, or --depth; black where the pixel's ray misses) as a P3 PPM through the
// device encoder; --seed and --precision apply.
// --direct N writes the direct-lighting pass instead of a render (rtx_direct: at each pixel's
// first hit, the light arriving straight from the scene's emitters, from N points sampled on the
// emitters and their shadow segments, keyed by the global pixel; black where the pixel's ray
// misses) as a P3 PPM through the device encoder; --seed and --precision apply.
// --nee writes the frame of the light-sampling estimator instead of the plain render
// (rtx_render_nee: the renderer's own paths with one emitter sample at every diffuse vertex, fixed
// spp) as a P3 PPM through the device encoder, at the preset's samples and depth (or --spp,
// --depth); --seed and --precision apply.  Without the flag no output changes.
// --mis writes the frame of the combined estimator in the same way (rtx_render_mis: the same paths
// and emitter samples, the two strategies weighted with the power heuristic, so a lamp close to a
// wall leaves no fireflies); --nee and --mis together is an error.
// --nee / --mis with any of --chunks, --preview, --checkpoint, --resume, --denoise or --adaptive render
// the estimator's frame through a sampled film (rtx_film_create_sampled): those options then work as
// they do for the plain render, and without --adaptive the bytes on stdout are those of the plain
// --nee / --mis run at the same spp.  --adaptive samples every pixel until it converges (the
// renderer's own test, 16 samples at least, threshold 0.05f) or reaches the spp.  The run logs
// "mis film: <budget> spp, <emitters> emitters, <traced> segments traced, <recorded> recorded".
// --probes NX,NY,NZ[,SPP] writes light probes as text instead of a PPM (rtx_probe_sh): the probes sit
// at the cell centres of an NX x NY x NZ grid over the scene's bounding box, x fastest, keyed by
// their index; one line per probe, "x y z" and the 27 SH coefficients ([coefficient][r, g, b]), each
// number with %.17g.  SPP samples per probe (default 256); depth and seed are the preset's (or
// --depth, --seed), --precision applies, --nee / --mis choose the estimator.
// --mk-adaptive selects the AdaptiveSampler (sampler.h:44-82) for --mode megakernel,
// with max_samples = the preset's (or --spp) samples.
// Defaults follow main.cc: preset "default" (fallback when unknown), the Cornell box
// scene (switch(4), main.cc:178-183), WavefrontRenderer with the preset's maxDepth and
// samplesPerPixel, adaptive sampling on; "Runtime: Xs" on stderr.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <string>
#include <vector>

#include "rt/renderer.h"

using namespace rt;

int main(int argc, char** argv) {
  core::Timer clock;
  std::string preset = "default", scene_name = "cornell", cameras = "cameras.json", mode = "persistent",
              precision = "parity";
  int spp = -1, depth = -1;
  uint64_t seed = 1234;
  bool fixed = false, denoise = false;
  bool adaptive = false;  // --adaptive (with --nee / --mis)
  std::vector<int> devices;
  int mk_min = -1, gpus = 1, chunks = 0, ao_samples = 0;
  int irr_samples = 0, irr_depth = -1;  // --irradiance (depth -1: the preset's)
  bool irr = false;
  int direct_samples = 0;  // --direct
  bool direct = false;
  int probes[4] = {0, 0, 0, 256};  // --probes NX,NY,NZ[,SPP]
  bool probe = false;
  bool nee = false;  // --nee
  bool mis = false;  // --mis
  double ao_radius = 0.0;  // 0: a quarter of the scene's bounding-box diagonal
  std::string preview, checkpoint, resume;
  float mk_thr = 0.0f;
  for (int i = 1; i < argc; i++) {
    std::string a = argv[i];
    auto next = [&]() -> std::string {
      if (i + 1 >= argc) {
        std::cerr << "missing value for " << a << "\n";
        std::exit(2);
      }
      return argv[++i];
    };
    if (a == "--scene") scene_name = next();
    else if (a == "--cameras") cameras = next();
    else if (a == "--spp") spp = std::atoi(next().c_str());
    else if (a == "--depth") depth = std::atoi(next().c_str());
    else if (a == "--seed") seed = std::strtoull(next().c_str(), nullptr, 10);
    else if (a == "--mode") mode = next();
    else if (a == "--precision") precision = next();
    else if (a == "--fixed") fixed = true;
    else if (a == "--gpus") gpus = std::atoi(next().c_str());
    else if (a == "--chunks") chunks = std::atoi(next().c_str());
    else if (a == "--preview") preview = next();
    else if (a == "--checkpoint") checkpoint = next();
    else if (a == "--resume") resume = next();
    else if (a == "--denoise") denoise = true;
    else if (a == "--adaptive") adaptive = true;
    else if (a == "--ao") {
      const std::string v = next();
      const size_t c = v.find(',');
      ao_samples = std::atoi(v.substr(0, c).c_str());
      if (c != std::string::npos) ao_radius = std::strtod(v.substr(c + 1).c_str(), nullptr);
      if (ao_samples < 1 || ao_samples > 1024 || (c != std::string::npos && !(ao_radius > 0))) {
        std::cerr << "--ao expects N[,RADIUS] with N in 1..1024 and RADIUS > 0\n";
        return 2;
      }
    }
    else if (a == "--irradiance") {
      const std::string v = next();
      const size_t c = v.find(',');
      irr = true;
      irr_samples = std::atoi(v.substr(0, c).c_str());
      if (c != std::string::npos) irr_depth = std::atoi(v.substr(c + 1).c_str());
      if (irr_samples < 1 || (c != std::string::npos && irr_depth < 0)) {
        std::cerr << "--irradiance expects N[,DEPTH] with N >= 1 and DEPTH >= 0\n";
        return 2;
      }
    }
    else if (a == "--direct") {
      direct = true;
      direct_samples = std::atoi(next().c_str());
      if (direct_samples < 1) {
        std::cerr << "--direct expects N >= 1\n";
        return 2;
      }
    }
    else if (a == "--probes") {
      const std::string v = next();
      probe = true;
      int fields = 0;
      bool ok = !v.empty();
      for (size_t p = 0; ok && p <= v.size();) {
        size_t q = v.find(',', p);
        if (q == std::string::npos) q = v.size();
        const std::string f = v.substr(p, q - p);
        char* end = nullptr;
        const long val = std::strtol(f.c_str(), &end, 10);
        ok = fields < 4 && !f.empty() && *end == '\0' && val >= 1 && val <= 0x7FFFFFFF;
        if (ok) probes[fields++] = (int)val;
        p = q + 1;
      }
      if (!ok || fields < 3 || (int64_t)probes[0] * probes[1] * probes[2] > ((int64_t)1 << 24)) {
        std::cerr << "--probes expects NX,NY,NZ[,SPP], each >= 1, at most 2^24 probes\n";
        return 2;
      }
    }
    else if (a == "--nee") nee = true;
    else if (a == "--mis") mis = true;
    else if (a == "--devices") {
      const std::string v = next();
      for (size_t p = 0; p < v.size();) {
        size_t q = v.find(',', p);
        if (q == std::string::npos) q = v.size();
        devices.push_back(std::atoi(v.substr(p, q - p).c_str()));
        p = q + 1;
      }
    }
    else if (a == "--mk-adaptive") {
      const std::string v = next();
      const size_t c = v.find(':');
      if (c == std::string::npos) {
        std::cerr << "--mk-adaptive expects MIN:THRESHOLD\n";
        return 2;
      }
      mk_min = std::atoi(v.substr(0, c).c_str());
      mk_thr = std::strtof(v.substr(c + 1).c_str(), nullptr);
    }
    else if (!a.empty() && a[0] != '-') preset = a;
    else {
      std::cerr << "unknown option " << a << "\n";
      return 2;
    }
  }
  if (nee && mis) {
    std::cerr << "--nee and --mis exclude each other\n";
    return 2;
  }
  if (adaptive && !nee && !mis) {
    std::cerr << "--adaptive needs --nee or --mis (the plain render is adaptive unless --fixed)\n";
    return 2;
  }
  try {
    if (!std::ifstream(cameras)) {
      const std::string alt = scene::ResolveAsset("../../configs/cameras.json");
      if (!alt.empty()) cameras = alt;
    }
    auto cams = scene::loadCameras(cameras);
    if (!cams.count(preset)) {  // main.cc:169-172
      std::cerr << "Camera '" << preset << "' not found. Using default.\n";
      preset = "default";
    }
    scene::ColorCamera cam;
    cam.SetFromConfig(cams[preset]);
    cam.Initialize();
    std::shared_ptr<scene::Scene> world;
    if (scene_name.size() > 5 && scene_name.substr(scene_name.size() - 5) == ".rtxs")
      world = scene::LoadSceneFile(scene_name, "");
    else
      world = scene::BuildRecipe(scene_name, 1234, "");
    const int ns = spp > 0 ? spp : cam.samples_per_pixel_;
    const int md = depth >= 0 ? depth : cam.max_depth_;
    const bool film = chunks > 0 || !preview.empty() || !checkpoint.empty() || !resume.empty();
    if (film && mode == "megakernel") {
      std::cerr << "--chunks / --preview / --checkpoint / --resume need --mode wavefront or persistent\n";
      return 2;
    }
    if (denoise && mode == "megakernel") {
      std::cerr << "--denoise needs --mode wavefront or persistent\n";
      return 2;
    }
    if (probe) {
      integrator::GpuRayIntegrator integ(world.get(), devices.empty() ? 0 : devices[0],
                                         precision == "fast" ? RTX_PREC_FAST : RTX_PREC_PARITY);
      const geom::Aabb b = world->BoundingBox();
      const double lo[3] = {b.x.min_, b.y.min_, b.z.min_}, hi[3] = {b.x.max_, b.y.max_, b.z.max_};
      std::vector<core::Point3> pts;
      for (int iz = 0; iz < probes[2]; iz++)
        for (int iy = 0; iy < probes[1]; iy++)
          for (int ix = 0; ix < probes[0]; ix++) {
            const int at[3] = {ix, iy, iz};
            double c[3];
            for (int k = 0; k < 3; k++) c[k] = lo[k] + (hi[k] - lo[k]) * (((double)at[k] + 0.5) / (double)probes[k]);
            pts.push_back(core::Point3(c[0], c[1], c[2]));
          }
      std::vector<double> sh;
      integ.ProbeBatch(pts, sh, probes[3], md, seed, mis ? RTX_ESTIMATOR_MIS : (nee ? RTX_ESTIMATOR_NEE : 0));
      std::string out;
      char num[40];
      for (size_t i = 0; i < pts.size(); i++) {
        for (int k = 0; k < 3; k++) {
          std::snprintf(num, sizeof num, k ? " %.17g" : "%.17g", pts[i][k]);
          out += num;
        }
        for (int q = 0; q < 3 * RTX_SH_COEFFS; q++) {
          std::snprintf(num, sizeof num, " %.17g", sh[3 * RTX_SH_COEFFS * i + q]);
          out += num;
        }
        out += "\n";
      }
      std::cout.write(out.data(), (std::streamsize)out.size());
      std::clog << "probes: " << pts.size() << " probes, " << probes[3] << " samples, depth " << md << "\n";
    } else if (ao_samples > 0) {
      integrator::GpuRayIntegrator integ(world.get(), devices.empty() ? 0 : devices[0],
                                         precision == "fast" ? RTX_PREC_FAST : RTX_PREC_PARITY);
      if (!(ao_radius > 0)) {
        const geom::Aabb b = world->BoundingBox();
        const double dx = b.x.max_ - b.x.min_, dy = b.y.max_ - b.y.min_, dz = b.z.max_ - b.z.min_;
        ao_radius = 0.25 * std::sqrt(dx * dx + dy * dy + dz * dz);
      }
      const rtx_camera& dc = cam.device();
      rtx_render_params whole{};
      whole.precision = integ.precision();
      const rtx_ao_params ap{ao_samples, 0, ao_radius, seed};
      const size_t npix = (size_t)dc.image_width * (size_t)dc.image_height;
      std::vector<double> ao(npix), rgb(3 * npix);
      if (rtx_ao(integ.device_scene(), &dc, &whole, &ap, ao.data()) != RTX_OK)
        throw std::runtime_error(std::string("rtx_ao: ") + rtx_last_error());
      for (size_t i = 0; i < npix; i++) rgb[3 * i] = rgb[3 * i + 1] = rgb[3 * i + 2] = ao[i];
      std::string bytes(rtx_p3_max_bytes(dc.image_width, dc.image_height), '\0');
      size_t len = 0;
      if (rtx_encode_p3(integ.device_scene(), rgb.data(), dc.image_width, dc.image_height, bytes.data(), bytes.size(),
                        &len) != RTX_OK)
        throw std::runtime_error(std::string("rtx_encode_p3: ") + rtx_last_error());
      std::cout.write(bytes.data(), (std::streamsize)len);
      std::clog << "AO: " << ao_samples << " samples, radius " << ao_radius << "\n";
    } else if (irr || direct) {
      integrator::GpuRayIntegrator integ(world.get(), devices.empty() ? 0 : devices[0],
                                         precision == "fast" ? RTX_PREC_FAST : RTX_PREC_PARITY);
      const rtx_camera& dc = cam.device();
      const int W = dc.image_width, H = dc.image_height;
      const size_t npix = (size_t)W * (size_t)H;
      // each pixel's centre ray (the ray of rtx_aov) and its first hit
      std::vector<rtx_ray> rays(npix);
      for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
          rtx_ray& r = rays[(size_t)y * W + x];
          for (int k = 0; k < 3; k++) {
            r.origin[k] = dc.center[k];
            r.direction[k] =
                ((dc.pixel00[k] + ((double)x * dc.pixel_delta_u[k])) + ((double)y * dc.pixel_delta_v[k])) - dc.center[k];
          }
        }
      std::vector<rtx_hit> hits(npix);
      if (rtx_intersect(integ.device_scene(), rays.data(), npix, hits.data(), RTX_SEAM_TMIN, core::kInfinity,
                        integ.precision()) != RTX_OK)
        throw std::runtime_error(std::string("rtx_intersect: ") + rtx_last_error());
      // surfels: the hit point and the record's normal; a zero normal (black) where the ray misses
      std::vector<uint32_t> ids(npix);
      for (size_t i = 0; i < npix; i++) {
        ids[i] = (uint32_t)i;
        for (int k = 0; k < 3; k++)
          rays[i].origin[k] = hits[i].hit ? hits[i].p[k] : 0.0, rays[i].direction[k] = hits[i].hit ? hits[i].normal[k] : 0.0;
      }
      rtx_radiance_params rp{};
      rp.spp = direct ? direct_samples : irr_samples, rp.max_depth = irr_depth >= 0 ? irr_depth : md, rp.first_sample = 0;
      rp.precision = integ.precision(), rp.seed = seed;
      std::vector<double> rgb(3 * npix);
      int64_t n_emitters = 0;
      if (direct) {
        if (rtx_direct(integ.device_scene(), rays.data(), ids.data(), npix, &rp, rgb.data(), nullptr) != RTX_OK)
          throw std::runtime_error(std::string("rtx_direct: ") + rtx_last_error());
        if (rtx_scene_emitters(integ.device_scene(), &n_emitters, nullptr) != RTX_OK)
          throw std::runtime_error(std::string("rtx_scene_emitters: ") + rtx_last_error());
      } else if (rtx_irradiance(integ.device_scene(), rays.data(), ids.data(), npix, &rp, rgb.data(), nullptr) != RTX_OK)
        throw std::runtime_error(std::string("rtx_irradiance: ") + rtx_last_error());
      std::string bytes(rtx_p3_max_bytes(W, H), '\0');
      size_t len = 0;
      if (rtx_encode_p3(integ.device_scene(), rgb.data(), W, H, bytes.data(), bytes.size(), &len) != RTX_OK)
        throw std::runtime_error(std::string("rtx_encode_p3: ") + rtx_last_error());
      std::cout.write(bytes.data(), (std::streamsize)len);
      if (direct) std::clog << "direct: " << direct_samples << " samples, " << n_emitters << " emitters\n";
      else std::clog << "irradiance: " << irr_samples << " samples, depth " << rp.max_depth << "\n";
    } else if ((nee || mis) && (film || denoise || adaptive)) {  // the estimator's frame through a sampled film
      integrator::GpuRayIntegrator integ(world.get(), devices.empty() ? 0 : devices[0],
                                         precision == "fast" ? RTX_PREC_FAST : RTX_PREC_PARITY);
      renderer::WavefrontRenderer r(*world, cam, integ, md, ns, 2 * 8192);
      r.set_seed(seed);
      r.set_adaptive(adaptive);
      r.set_precision(precision == "fast" ? RTX_PREC_FAST : RTX_PREC_PARITY);
      r.set_estimator(mis ? RTX_ESTIMATOR_MIS : RTX_ESTIMATOR_NEE);
      if (film) r.set_progressive(chunks > 0 ? chunks : 1);
      if (!checkpoint.empty()) r.set_checkpoint(checkpoint);
      if (!resume.empty()) r.set_resume(resume);
      r.set_denoise(denoise);
      if (!preview.empty())
        r.set_preview([&](int budget, const std::string& p3) {
          const std::string path = preview + "_" + std::to_string(budget) + ".ppm";
          std::ofstream o(path, std::ios::binary);
          o.write(p3.data(), (std::streamsize)p3.size());
          if (!o) throw std::runtime_error("cannot write " + path);
        });
      r.Render();
      int64_t n_emitters = 0;
      if (rtx_scene_emitters(integ.device_scene(), &n_emitters, nullptr) != RTX_OK)
        throw std::runtime_error(std::string("rtx_scene_emitters: ") + rtx_last_error());
      std::clog << (mis ? "mis film: " : "nee film: ") << ns << " spp, " << n_emitters << " emitters, "
                << r.stats().rays_total << " segments traced, " << r.stats().rays_recorded << " recorded\n";
    } else if (nee || mis) {
      integrator::GpuRayIntegrator integ(world.get(), devices.empty() ? 0 : devices[0],
                                         precision == "fast" ? RTX_PREC_FAST : RTX_PREC_PARITY);
      const rtx_camera& dc = cam.device();
      const int W = dc.image_width, H = dc.image_height;
      const size_t npix = (size_t)W * (size_t)H;
      rtx_render_params rp{};
      rp.spp = ns, rp.max_depth = md, rp.seed = seed, rp.precision = integ.precision();
      std::vector<double> rgb(3 * npix);
      std::vector<uint32_t> segs(npix);
      if ((mis ? rtx_render_mis : rtx_render_nee)(integ.device_scene(), &dc, &rp, rgb.data(), segs.data()) != RTX_OK)
        throw std::runtime_error(std::string(mis ? "rtx_render_mis: " : "rtx_render_nee: ") + rtx_last_error());
      int64_t n_emitters = 0;
      if (rtx_scene_emitters(integ.device_scene(), &n_emitters, nullptr) != RTX_OK)
        throw std::runtime_error(std::string("rtx_scene_emitters: ") + rtx_last_error());
      std::string bytes(rtx_p3_max_bytes(W, H), '\0');
      size_t len = 0;
      if (rtx_encode_p3(integ.device_scene(), rgb.data(), W, H, bytes.data(), bytes.size(), &len) != RTX_OK)
        throw std::runtime_error(std::string("rtx_encode_p3: ") + rtx_last_error());
      std::cout.write(bytes.data(), (std::streamsize)len);
      uint64_t total = 0;
      for (uint32_t v : segs) total += v;
      std::clog << (mis ? "mis: " : "nee: ") << ns << " spp, " << n_emitters << " emitters, " << total << " segments\n";
    } else if (mode == "megakernel") {
      integrator::DefaultSampler fixed_sampler(ns);
      integrator::AdaptiveSampler adaptive_sampler(mk_min, ns, mk_thr);
      integrator::Sampler& sampler = mk_min >= 0 ? (integrator::Sampler&)adaptive_sampler : fixed_sampler;
      cam.max_depth_ = md;
      renderer::MegaKernel r(*world, cam, sampler);
      r.set_seed(seed);
      r.Render();
    } else {
      integrator::GpuRayIntegrator integ(world.get(), devices.empty() ? 0 : devices[0],
                                         precision == "fast" ? RTX_PREC_FAST : RTX_PREC_PARITY);
      renderer::WavefrontRenderer r(*world, cam, integ, md, ns, 2 * 8192);
      r.set_seed(seed);
      r.set_adaptive(!fixed);
      r.set_precision(precision == "fast" ? RTX_PREC_FAST : RTX_PREC_PARITY);
      r.set_mode(mode == "persistent" ? RTX_MODE_PERSISTENT : RTX_MODE_WAVEFRONT);
      if (!devices.empty()) r.set_devices(devices);
      else if (gpus > 1) r.set_gpus(gpus);
      if (film) r.set_progressive(chunks > 0 ? chunks : 1);
      if (!checkpoint.empty()) r.set_checkpoint(checkpoint);
      if (!resume.empty()) r.set_resume(resume);
      r.set_denoise(denoise);
      if (!preview.empty())
        r.set_preview([&](int budget, const std::string& p3) {
          const std::string path = preview + "_" + std::to_string(budget) + ".ppm";
          std::ofstream o(path, std::ios::binary);
          o.write(p3.data(), (std::streamsize)p3.size());
          if (!o) throw std::runtime_error("cannot write " + path);
        });
      r.Render();
      std::clog << "Rays: " << r.stats().rays_total << " (" << r.stats().rays_total / (r.stats().kernel_ms * 1e3)
                << " Mrays/s device)\n";
    }
  } catch (const std::exception& e) {
    std::cerr << "error: " << e.what() << "\n";
    return 1;
  }
  std::clog << "Runtime: " << std::setprecision(2) << clock.elapsed() << "s" << std::flush;
  return 0;
}
