// rtx_irradiance.h — irradiance queries: the cosine-weighted gather of radiance over the
// hemisphere at caller-supplied surface points (rtx_irradiance*, include/rtx.h; DESIGN.md §4f
// "Irradiance queries").  Included once, by rtx_queries.hip, after rtx_radiance.h.  Nothing here is
// used by a render kernel, and k_radiance, k_radiance_sum, k_ao and trace<>() are as they were:
// the kernels below call the same device functions.
//
// Contract: a surfel is an rtx_ray whose origin is the point and whose direction is the surface
// normal (any positive finite length).  Sample k of surfel i starts a path at the point along
// irradiance_ray()'s direction: cosine_direction (rtx_occlusion.h, the operations of the AO
// pass's ao_direction) from stream kRngStreamIrr of (seed, pixel, first_sample + k).  From there
// the lane runs k_radiance's loop on k_radiance's operands, so the slot value is, bit for bit,
// rtx_radiance of that one ray with the same pixel key, spp = 1 and first_sample + k: the ray
// is a pure function of (seed, pixel, sample, surfel), both kernels below get it from the one
// function, no contraction is allowed (-ffp-contract=off), and a double survives the trip
// through memory unchanged.  The slots are summed by k_radiance_sum as it is.
#pragma once

#include "rtx_occlusion.h"
#include "rtx_radiance.h"

namespace rtxd {

// The depth-0 segment of sample `smp` of a surfel.  false: a degenerate normal (squared length
// not > 0 or not finite: zero, NaN, overflow), for which nothing is traced.
__device__ __forceinline__ bool irradiance_ray(uint64_t seed, uint32_t pix, uint32_t smp, const rtx_ray& s, V3& o,
                                               V3& d) {
  const V3 n = v3(s.direction[0], s.direction[1], s.direction[2]);
  const double l2 = len2(n);
  if (!(l2 > 0.0) || !(l2 < kInf)) return false;
  o = v3(s.origin[0], s.origin[1], s.origin[2]);
  d = cosine_direction(seed, pix, smp, kRngStreamIrr, n);
  return true;
}

// One lane per slot of the chunk (RadianceChunk: `rays` are the surfels): slot j is sample
// s0 + j % K of surfel ray0 + j / K, so a wave's 64 paths start at 64 / K neighbouring points.
// The whole path per lane, the traversal stack in the lane's LDS column, as in k_radiance (the
// same loop text, the same chunk_slot and slot_write); a degenerate surfel's lanes write 0 and leave.
template <int STACK, bool FAST>
__global__ __launch_bounds__(kBlock, kTraceWaves) void k_irradiance(DScene S, RadianceChunk A) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  uint32_t* stk = lds + threadIdx.x;
  const uint32_t j = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  if (j >= A.slots) return;
  rtx_ray surfel;
  uint32_t pix, smp;
  chunk_slot(A, j, surfel, pix, smp);
  Path P;
  if (!irradiance_ray(A.seed, pix, smp, surfel, P.o, P.d)) {
    slot_write(A.L, A.segs, j, v3(0.0, 0.0, 0.0), 0u);
    return;
  }
  P.thr = v3(1.0, 1.0, 1.0);
  P.depth = 0;
  Counters c{};
  uint32_t segs = 0;
  V3 L;
  while (true) {
    double tb;
    const int64_t best = trace<STACK, FAST, false>(S, P.o, P.d, (double)0.001f, kInf, stk, c, tb);
    segs++;
    Hit h;
    if (best >= 0) finish_hit<false>(S, best, P.o, P.d, (double)0.001f, h);
    Rng g = make_rng(A.seed, pix, smp, (uint32_t)P.depth + 1u);
    if (!shade(S, A.max_depth, P, h, best >= 0, g, L)) break;
  }
  slot_write(A.L, A.segs, j, L, segs);
}

// Test hook (rtx_internal_irradiance_rays): the depth-0 segments k_irradiance traces, one lane
// per (surfel, sample), surfel major, from irradiance_ray(); 6 doubles per ray (origin,
// direction), all zero for a degenerate surfel.
__global__ __launch_bounds__(kBlock) void k_irradiance_rays(const rtx_ray* __restrict__ surfels,
                                                            const uint32_t* __restrict__ ids, uint32_t nslots,
                                                            uint32_t K, uint64_t seed, int32_t s0,
                                                            double* __restrict__ out) {
  const uint32_t j = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  if (j >= nslots) return;
  const uint32_t i = j / K, k = j - i * K;
  const rtx_ray surfel = surfels[i];
  V3 o = v3(0, 0, 0), d = v3(0, 0, 0);  // (kept where irradiance_ray() returns false)
  irradiance_ray(seed, ids ? ids[i] : i, (uint32_t)s0 + k, surfel, o, d);
  double* q = out + 6 * (uint64_t)j;
  q[0] = o.x, q[1] = o.y, q[2] = o.z, q[3] = d.x, q[4] = d.y, q[5] = d.z;
}

}  // namespace rtxd
