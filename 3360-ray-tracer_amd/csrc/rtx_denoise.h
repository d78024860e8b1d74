// rtx_denoise.h — first-hit AOVs and the edge-avoiding a-trous denoiser (rtx_aov*, rtx_denoise*,
// rtx_film_denoise*, include/rtx.h; DESIGN.md §4b "AOVs and the denoiser").
// Here: the filter's launch interface (its kernels are their own translation unit,
// rtx_denoise.hip) and, for the translation unit that holds the trace kernels
// (RTX_DENOISE_AOV_KERNELS, rtx_queries.hip), k_aov.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace rtxdn {

constexpr int kMaxIterations = 8;
constexpr int kDemodulate = 1;      // RTX_DENOISE_DEMODULATE
constexpr float kAlbedoFloor = 1e-3f;  // demodulation divides by max(albedo, kAlbedoFloor)

struct FilterParams {  // rtx_denoise_params as the kernels take it (validated by the caller)
  int iterations, flags;
  float normal_power, sigma_depth, sigma_color;
};

// The f64 AOVs as the filter reads them: guide {nx, ny, nz, depth} and albedo {r, g, b, 0}, one
// float4 each per pixel.  A pixel is a hit where its f32 depth is > 0.
hipError_t pack_guides(const double* d_normal, const double* d_depth, const double* d_albedo, int64_t npix,
                       float4* guide, float4* albedo, hipStream_t s);

// d_rgb (w x h x 3 doubles; d_var: w x h doubles or nullptr) filtered into d_out.  work0 / work1:
// w x h float4 each.  iterations == 0 copies d_rgb to d_out (no f32 round trip).  Enqueues on `s`.
hipError_t filter(int32_t w, int32_t h, const double* d_rgb, const double* d_var, const float4* guide,
                  const float4* albedo, float4* work0, float4* work1, const FilterParams& p, double* d_out,
                  hipStream_t s);

}  // namespace rtxdn

#if defined(__HIPCC__) && defined(RTX_DENOISE_AOV_KERNELS)
#include "rtx_kernels.h"

namespace rtxd {

// First-hit AOVs: one lane per pixel of the subset, in subset order.  The ray is the pixel
// centre's: origin cam.center, direction ((pixel00 + i du) + j dv) - center, no lens and no
// jitter.  Written as doubles (a null output is skipped): depth = t of the closest hit on
// [tmin, inf) or 0 on a miss; normal = the record's (against the ray) or 0; albedo = the
// Lambertian's texture value at the hit, the metal's albedo, and 1 for dielectrics, lights and
// misses (where demodulating by it changes nothing).
template <int STACK, bool FAST>
__global__ __launch_bounds__(kBlock, kTraceWaves) void k_aov(DScene S, rtx_camera cam, PixelMap map, int64_t npix,
                                                                 double tmin, double* __restrict__ albedo,
                                                                 double* __restrict__ normal,
                                                                 double* __restrict__ depth) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  uint32_t* stk = lds + threadIdx.x;
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= npix) return;
  int x, y;
  map.xy((uint32_t)p, x, y);
  const V3 c = v3(cam.center[0], cam.center[1], cam.center[2]);
  const V3 p00 = v3(cam.pixel00[0], cam.pixel00[1], cam.pixel00[2]);
  const V3 du = v3(cam.pixel_delta_u[0], cam.pixel_delta_u[1], cam.pixel_delta_u[2]);
  const V3 dv = v3(cam.pixel_delta_v[0], cam.pixel_delta_v[1], cam.pixel_delta_v[2]);
  const V3 d = ((p00 + ((double)x * du)) + ((double)y * dv)) - c;
  Counters cnt{};
  double tb;
  const int64_t best = trace<STACK, FAST, false>(S, c, d, tmin, kInf, stk, cnt, tb);
  V3 a = v3(1, 1, 1), n = v3(0, 0, 0);
  double t = 0.0;
  if (best >= 0) {
    Hit h;
    finish_hit_at(S, best, tb, c, d, h);
    t = h.t, n = h.normal;
    const rtx_material m = S.mats[h.mat];
    if (m.kind == RTX_MAT_LAMBERTIAN) a = mat_tex(S, m, h);
    else if (m.kind == RTX_MAT_METAL) a = v3(m.albedo[0], m.albedo[1], m.albedo[2]);
  }
  if (albedo) albedo[3 * p] = a.x, albedo[3 * p + 1] = a.y, albedo[3 * p + 2] = a.z;
  if (normal) normal[3 * p] = n.x, normal[3 * p + 1] = n.y, normal[3 * p + 2] = n.z;
  if (depth) depth[p] = t;
}

}  // namespace rtxd
#endif
