// rtx_direct.h — direct-lighting queries: the scene's emitters sampled from caller-supplied
// surface points (rtx_direct*, rtx_scene_emitters, include/rtx.h; DESIGN.md §4g "Direct-lighting
// queries").  Included once, by rtx_queries.hip, after rtx_irradiance.h.  Nothing here is used by a
// render kernel, and trace<>(), shade*, k_radiance*, k_irradiance, k_ao and k_occluded are as
// they were: the kernels below call the same device functions, and k_direct decodes and writes its
// slot with rtx_radiance.h's chunk_slot and slot_write.
//
// Contract: a surfel is an rtx_ray whose origin is the point x and whose direction is the surface
// normal (any positive finite length).  Sample k of surfel i is direct_sample() of (seed, pixel,
// first_sample + k, surfel): a point y uniform over the scene's emitting area A (the emitter
// table below), the segment (x, y - x) and the unshadowed contribution
//   C = Le(y) max(0, n_x . w) |n_y . w| A / (pi |y - x|^2),  w = (y - x) / |y - x|,
// with Le and n_y from the hit record a path reaching y along the segment would build
// (finish_hit_at<true> at t = 1, mat_emitted).  The slot value is C V, V = 1 iff the any-hit walk
// of rtx_occluded accepts nothing on (RTX_SEAM_TMIN, kDirectTmax) of the segment.  Both kernels
// below get the sample from the one function, no contraction is allowed (-ffp-contract=off) and a
// double survives the trip through memory unchanged, so the kernel's slot equals C of the hook
// times the public rtx_occluded of the hook's segment, bit for bit.  The slots are summed by
// k_radiance_sum as it is.
#pragma once

#include "rtx_irradiance.h"
#include "rtx_occlusion.h"
#include "rtx_radiance.h"

namespace rtxd {

// The shadow segment ends short of the emitter: the chosen primitive is itself hit at t = 1 up to
// the rounding of the f32 islands in the primitive tests, and must not shadow its own sample.  A
// blocker within 1e-4 of the segment's length from the light is ignored.
constexpr double kDirectTmax = (double)0.9999f;

// The emitters of a scene (primitives whose material is a DiffuseLight), in the order of the
// device primitive array, and their inclusive cumulative areas: cum[n - 1] is the total area A.
// prim is fixed for the scene's life; cum is rebuilt after every in-place update.
struct EmitterTable {
  const uint32_t* prim;
  double* cum;
  int64_t n;
};

// One lane per emitter: its area into cum[] (k_emitter_scan then sums in place).  Sphere
// 4 pi r^2 (r = fmax(0, radius), the radius the primitive tests use), triangle
// |e1 x e2| / 2 (the device record holds A, B - A, C - A), rect (a1 - a0)(b1 - b0).  A
// non-finite or negative area counts as 0.
__global__ __launch_bounds__(kBlock) void k_emitter_area(const rtx_prim* __restrict__ prims, EmitterTable E) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= E.n) return;
  const rtx_prim* __restrict__ P = prims + E.prim[i];
  const int kind = P->kind;
  double a;
  if (kind == RTX_PRIM_SPHERE) {
    const double r = fmax(0.0, P->g[3]);
    a = (4.0 * kPi) * (r * r);
  } else if (kind == RTX_PRIM_TRIANGLE) {
    a = 0.5 * sqrt(len2(cross(tri_e1(P->g), tri_e2(P->g))));
  } else {
    a = (P->g[1] - P->g[0]) * (P->g[3] - P->g[2]);
  }
  E.cum[i] = (a >= 0.0 && a < kInf) ? a : 0.0;
}

// One block: the inclusive running sum of cum[0 .. n), in place.  Lane t owns the contiguous
// entries [t * per, (t + 1) * per), per = ceil(n / kBlock): it adds them up from 0, lane 0 turns
// the kBlock partial sums into each lane's starting offset (a left-to-right sum), and every lane
// walks its entries again from its offset.  The partition and therefore the order of every
// addition depend on n only: the same areas give the same bits on every run.
__global__ __launch_bounds__(kBlock) void k_emitter_scan(EmitterTable E) {
  __shared__ double part[kBlock];
  const int64_t per = (E.n + kBlock - 1) / kBlock;
  const int64_t b0 = (int64_t)threadIdx.x * per;
  const int64_t i0 = b0 < E.n ? b0 : E.n, i1 = i0 + per < E.n ? i0 + per : E.n;
  double s = 0.0;
  for (int64_t i = i0; i < i1; i++) s += E.cum[i];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double run = 0.0;
    for (int t = 0; t < kBlock; t++) {
      const double p = part[t];
      part[t] = run;
      run += p;
    }
  }
  __syncthreads();
  s = part[threadIdx.x];
  for (int64_t i = i0; i < i1; i++) {
    s += E.cum[i];
    E.cum[i] = s;
  }
}

// Sample `smp` of a surfel: the segment (o, d) = (x, y - x) to a point y uniform over the
// emitting area, and its unshadowed contribution C.  u0, u1, u2 are drawn in that order from
// stream kRngStreamDirect of (seed, pix, smp): u0 selects the emitter in proportion to its area
// (the first table entry whose cumulative area exceeds u0 A), u1, u2 place y on it (rect: linear;
// triangle: s = sqrt(u1), y = (1 - s) a + s (1 - u2) b + s u2 c, formed from the record's edges as
// a + s (1 - u2)(b - a) + s u2 (c - a); sphere: z = 1 - 2 u1, phi = 2 pi u2 over the whole
// sphere, whose far side its own occlusion rejects).
// false, with o, d and C zero: nothing to trace.  No emitters, A not > 0 or not finite; a
// degenerate normal (irradiance_ray's test); |y - x|^2 not > 0 or not finite; or no component of
// C > 0 (a light that faces away or is seen edge-on, a black light, a NaN).
// direct_sample_from: the same from `stream` of the key (next-event estimation draws a path
// vertex's sample from a stream of its own, rtx_nee.h).
// direct_sample_g: direct_sample_from that also gives g, the scalar Le is multiplied by (C = g Le):
// the ratio of the two solid-angle densities at (x, y), p_bsdf / p_light, which the
// power-heuristic weights of rtx_nee.h's MIS form are made of.  0 where nothing is traced.
__device__ __forceinline__ bool direct_sample_g(const DScene& S, const EmitterTable& E, uint64_t seed, uint32_t pix,
                                                uint32_t smp, uint32_t stream, const rtx_ray& s, V3& o, V3& d, V3& C,
                                                double& g_out) {
  o = v3(0, 0, 0), d = v3(0, 0, 0), C = v3(0, 0, 0);
  g_out = 0.0;
  if (E.n <= 0) return false;
  const double A = E.cum[E.n - 1];
  if (!(A > 0.0) || !(A < kInf)) return false;
  const V3 n = v3(s.direction[0], s.direction[1], s.direction[2]);
  const double l2 = len2(n);
  if (!(l2 > 0.0) || !(l2 < kInf)) return false;
  const V3 x = v3(s.origin[0], s.origin[1], s.origin[2]);
  Rng g = make_rng(seed, pix, smp, stream);
  const double u0 = g.next(), u1 = g.next(), u2 = g.next();
  // the first entry above u0 * A; the last one when the product rounds up to A
  const double target = u0 * A;
  int64_t lo = 0, hi = E.n - 1;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (E.cum[mid] > target) hi = mid;
    else lo = mid + 1;
  }
  // cum[lo - 1] <= target < cum[lo]: the entry's own area is positive, except at that last one,
  // from which the walk steps back over entries of zero area (A > 0: it ends at index >= 0)
  if (!(E.cum[lo] > target))
    while (lo > 0 && E.cum[lo - 1] == E.cum[lo]) lo--;
  const int64_t e = (int64_t)E.prim[lo];
  const rtx_prim* __restrict__ P = S.prims + e;
  const int kind = P->kind;
  V3 y;
  if (kind == RTX_PRIM_SPHERE) {
    const V3 c{P->g[0], P->g[1], P->g[2]};
    const double radius = fmax(0.0, P->g[3]);
    const double z = 1.0 - 2.0 * u1;
    const double rxy = sqrt(fmax(0.0, 1.0 - z * z));
    const double phi = 2.0 * kPi * u2;
    double cph, sph;
    cos_sin(phi, cph, sph);
    y = c + radius * v3(rxy * cph, rxy * sph, z);
  } else if (kind == RTX_PRIM_TRIANGLE) {
    const V3 a{P->g[0], P->g[1], P->g[2]};
    const double sq = sqrt(u1);
    y = (a + (sq * (1.0 - u2)) * tri_e1(P->g)) + (sq * u2) * tri_e2(P->g);
  } else {
    const double p = P->g[0] + u1 * (P->g[1] - P->g[0]);
    const double q = P->g[2] + u2 * (P->g[3] - P->g[2]);
    const double k = P->g[4];
    if (kind == RTX_PRIM_XY_RECT) y = v3(p, q, k);
    else if (kind == RTX_PRIM_XZ_RECT) y = v3(p, k, q);
    else y = v3(k, p, q);
  }
  const V3 seg = y - x;
  const double d2 = len2(seg);
  if (!(d2 > 0.0) || !(d2 < kInf)) return false;
  Hit h;
  finish_hit_at<true>(S, e, 1.0, x, seg, h);
  const V3 Le = mat_emitted(S, S.mats[h.mat], h);
  const V3 w = (1.0 / sqrt(d2)) * seg;
  const double cx = fmax(0.0, dot(normalize(n), w));
  const double cy = fabs(dot(h.normal, w));
  const double gs = ((cx * cy) * A) / (kPi * d2);
  const V3 c = gs * Le;
  if (!(c.x > 0.0 || c.y > 0.0 || c.z > 0.0)) return false;
  o = x, d = seg, C = c, g_out = gs;
  return true;
}
__device__ __forceinline__ bool direct_sample_from(const DScene& S, const EmitterTable& E, uint64_t seed, uint32_t pix,
                                                   uint32_t smp, uint32_t stream, const rtx_ray& s, V3& o, V3& d,
                                                   V3& C) {
  double gs;
  return direct_sample_g(S, E, seed, pix, smp, stream, s, o, d, C, gs);
}
__device__ __forceinline__ bool direct_sample(const DScene& S, const EmitterTable& E, uint64_t seed, uint32_t pix,
                                              uint32_t smp, const rtx_ray& s, V3& o, V3& d, V3& C) {
  return direct_sample_from(S, E, seed, pix, smp, kRngStreamDirect, s, o, d, C);
}

// One lane per slot of the chunk (RadianceChunk: `rays` are the surfels; max_depth is not read):
// slot j is sample s0 + j % K of surfel ray0 + j / K.  The lane writes C V to L and V (0 or 1)
// to segs, 0 where nothing is traced; the walk's stack sits in the lane's LDS column, as in
// k_occluded.
template <int STACK, bool FAST>
__global__ __launch_bounds__(kBlock, kTraceWaves) void k_direct(DScene S, EmitterTable E, RadianceChunk A) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  uint32_t* stk = lds + threadIdx.x;
  const uint32_t j = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  if (j >= A.slots) return;
  rtx_ray surfel;
  uint32_t pix, smp;
  chunk_slot(A, j, surfel, pix, smp);
  V3 o, d, C;
  uint32_t vis = 0u;
  if (direct_sample(S, E, A.seed, pix, smp, surfel, o, d, C))
    vis = occluded<STACK, FAST>(S, o, d, (double)RTX_SEAM_TMIN, kDirectTmax, stk) ? 0u : 1u;
  if (!vis) C = v3(0.0, 0.0, 0.0);
  slot_write(A.L, A.segs, j, C, vis);
}

// Test hook (rtx_internal_direct_samples, rtx_internal_nee_samples): the samples of `stream`, one
// lane per (surfel, sample), surfel major, from direct_sample_from(): with kRngStreamDirect the
// samples k_direct draws, with kRngStreamNee + depth those nee_path (rtx_nee.h) draws at a vertex
// of that depth.  9 doubles per sample (segment origin, y - x, C), all zero where nothing is traced.
__global__ __launch_bounds__(kBlock) void k_emitter_samples(DScene S, EmitterTable E,
                                                            const rtx_ray* __restrict__ surfels,
                                                            const uint32_t* __restrict__ ids, uint32_t nslots,
                                                            uint32_t K, uint64_t seed, int32_t s0, uint32_t stream,
                                                            double* __restrict__ out) {
  const uint32_t j = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  if (j >= nslots) return;
  const uint32_t i = j / K, k = j - i * K;
  const rtx_ray surfel = surfels[i];
  V3 o, d, C;
  direct_sample_from(S, E, seed, ids ? ids[i] : i, (uint32_t)s0 + k, stream, surfel, o, d, C);
  double* q = out + 9 * (uint64_t)j;
  q[0] = o.x, q[1] = o.y, q[2] = o.z, q[3] = d.x, q[4] = d.y, q[5] = d.z, q[6] = C.x, q[7] = C.y, q[8] = C.z;
}

}  // namespace rtxd
