// rtx_occlusion.h — occlusion (any-hit) ray queries and the ambient-occlusion pass
// (rtx_occluded*, rtx_ao*, include/rtx.h; DESIGN.md §4d "Occlusion queries and the AO pass").
// Included once, by rtx_queries.hip, after the trace kernels.  Nothing here is used by a render
// kernel: k_persistent, k_wf_extend, k_intersect and trace<>() are as they were.
//
// Contract: occluded(ray) == 1 iff some primitive's own test (prim_t: the sphere, triangle and
// rect routines of rtx_device.h, float islands included) accepts the ray on (tmin, tmax).  The
// walk returns at the first acceptance: no near-to-far order, no `closest`, no hit record.
//
// For the same scene, ray, interval and precision, occluded == (rtx_intersect's hit != 0), for
// every ray, with no tolerated exceptions and no tie cases:
//   hit => occluded.  The closest-hit walk culls with a bound (`closest`, in f32 tmax_f) that
//     starts at tmax and only shrinks, and both box tests are monotone in that bound, so every
//     node and leaf it visits the any-hit walk (whose bound stays at tmax) visits too, unless it
//     has returned 1 already; and a root the closest-hit walk accepts in (tmin, closest) lies in
//     (tmin, tmax), where the same arithmetic accepts it here.
//   occluded => hit.  The any-hit walk accepted some primitive P on (tmin, tmax).  The
//     closest-hit walk skips a leaf either by the same tmax bound (then this walk skips it as
//     well) or by a bound a hit found earlier has shrunk: a hit exists.  If it tests P, it
//     accepts P's root unless the root lies beyond `closest` < tmax: again a hit exists.
//     (A sphere's far root is tried only when the near one is out of range, in both walks; a
//     near root beyond `closest` but inside tmax is the case above.)
// The order in which children are visited plays no part in either direction.
#pragma once

#include "rtx_kernels.h"

namespace rtxd {

// one primitive's accept / reject on (tmin, tmax)
template <int KIND = -1>
__device__ __forceinline__ bool occl_prim(const DScene& S, uint32_t i, V3 o, V3 d, double tmin, double tmax) {
  double t;
  int32_t m;
  return prim_t<KIND>(S.prims + i, S.has_tris, o, d, tmin, tmax, t, m);
}

// The flat list (a scene without nodes), or the fast BVH's single-leaf root: trace_flat's
// counterpart.
// (who, here and below: where given, it receives the primitive that was accepted)
__device__ __forceinline__ bool occluded_flat(const DScene& S, V3 o, V3 d, double tmin, double tmax,
                                              int64_t* who = nullptr) {
  const int64_t n = S.use_bvh ? S.froot_count : S.n_prims;
  for (int64_t i = 0; i < n; i++)
    if (occl_prim(S, (uint32_t)i, o, d, tmin, tmax)) {
      if (who) *who = i;
      return true;
    }
  return false;
}

// Parity: the reference-layout tree with the f64 slab test on [tmin, tmax], the stack in the
// lane's LDS column as in trace_parity (entry i of lane t at stk[i * stride + t]).
template <int STACK>
__device__ __forceinline__ bool occluded_parity(const DScene& S, V3 o, V3 d, double tmin, double tmax, uint32_t* stk,
                                                int stride) {
  if (!S.use_bvh) {
    for (int64_t i = 0; i < S.n_prims; i++)
      if (occl_prim(S, (uint32_t)i, o, d, tmin, tmax)) return true;
    return false;
  }
  int sp = 1;
  stk[0] = 0u;
  while (sp > 0) {
    const uint32_t ni = stk[(--sp) * stride];
    const rtx_bvh_node* __restrict__ nd = S.nodes + ni;
    double lo[3] = {nd->lo[0], nd->lo[1], nd->lo[2]};
    double hi[3] = {nd->hi[0], nd->hi[1], nd->hi[2]};
    const uint32_t a = nd->left_first, b = nd->right_count, leaf = nd->is_leaf;
    if (!box_hit(lo, hi, o, o, d, tmin, tmax)) continue;
    if (leaf) {
      for (uint32_t i = 0; i < b; i++)
        if (occl_prim(S, a + i, o, d, tmin, tmax)) return true;
    } else {
      if (sp + 2 > STACK) __builtin_trap();  // host sizes STACK >= tree depth + 1
      stk[(sp++) * stride] = b;
      stk[(sp++) * stride] = a;
    }
  }
  return false;
}

// The global primitives (kept out of the fast tree), tested first, in the converged start of the
// walk, as trav_globals does: plain spheres (kGlobalSpheres) from uniform loads of the record
// with g[4] = radius * radius and sphere_root's one division, else the generic test.
__device__ __forceinline__ bool occluded_globals(const DScene& S, V3 o, V3 d, double tmin, double tmax,
                                                 int64_t* who = nullptr) {
  bool occ = false;
  if (S.n_global & kGlobalSpheres) {
    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    typedef double d2 __attribute__((ext_vector_type(2)));
    typedef const __attribute__((address_space(4))) u4 cu4;
    typedef const __attribute__((address_space(4))) d2 cd2;
    for (int i = 0; i < (S.n_global & 3); i++) {
      const uintptr_t P = (uintptr_t)(S.prims + (uint32_t)S.global[i]);
      const u4 w0 = *(cu4*)P;  // kind, material, g[0]
      const d2 w1 = *((cd2*)P + 1), w2 = *((cd2*)P + 2);
      const V3 oc = V3{__hiloint2double((int)w0.w, (int)w0.z), w1.x, w1.y} - o;
      const double a = len2(d);
      const double h = dot(d, oc);
      const double cc = len2(oc) - w2.y;
      const double disc = h * h - a * cc;
      double t;
      if (!(disc < 0) && sphere_root(a, h, sqrt(disc), tmin, tmax, t)) {
        occ = true;
        if (who) *who = S.global[i];
      }
    }
    return occ;
  }
  for (int i = 0; i < S.n_global; i++)
    if (occl_prim(S, (uint32_t)S.global[i], o, d, tmin, tmax)) {
      occ = true;
      if (who) *who = S.global[i];
    }
  return occ;
}

// Fast: the BVH4 tree with visit_slabs' conservative f32 slabs.  tmax_x is formed once and
// never shrinks.  Leaf tests run inline (the trace4_run shape).  The lean walk's push
// discipline is kept: the walk continues into one entered child (the nearest: a blocker is
// likelier there, and it costs three v_min and a select chain instead of the five-swap sort) and
// pushes the other entered ones, at most three per visit — exactly the pushes build_fast4's
// worst case counts for a node (internal slots - 1, whichever child is continued into), so its
// bound on sp holds for this walk and the kernel's STACK + 1 slots per lane suffice: the stores
// below are unconditional at sp, one slot above the deepest entry at most, as in visit_next.
template <int STACK>
__device__ __forceinline__ bool occluded_fast4(const DScene& S, V3 o, V3 d, double tmin, double tmax, uint32_t* stk,
                                               int stride, int64_t* who = nullptr) {
  if (!S.use_bvh || S.froot_leaf) return occluded_flat(S, o, d, tmin, tmax, who);
  if (occluded_globals(S, o, d, tmin, tmax, who)) return true;
  const FRay4L r = make_fray4l(o, d);
  const char* __restrict__ nbase = (const char*)S.f4nodes;
  const float tmax_x = f32_round_up(tmax) * 1.00001f;  // exit-side clamp with the slack folded in
  int sp = 0;
  uint32_t node = 0;
  while (true) {
    float tt[4];
    int32_t cc[4];
    uint32_t lmask = visit_slabs(nbase, node, r, tmax_x, tt, cc);
    while (lmask) {  // the visit's leaf slots
      const uint32_t cur = leaf_prim(cc, __builtin_ctz(lmask));
      lmask &= lmask - 1u;
      if (occl_prim(S, cur, o, d, tmin, tmax)) {
        if (who) *who = cur;
        return true;
      }
    }
    const float tn = fminf(fminf(tt[0], tt[1]), fminf(tt[2], tt[3]));
    if (tn != __builtin_inff()) {
      const int k = tt[0] == tn ? 0 : (tt[1] == tn ? 1 : (tt[2] == tn ? 2 : 3));
#pragma unroll
      for (int c = 0; c < 4; c++) {
        stk[sp * stride] = (uint32_t)cc[c];
        sp += (c != k && tt[c] != __builtin_inff()) ? 1 : 0;
      }
      node = (uint32_t)(k == 0 ? cc[0] : (k == 1 ? cc[1] : (k == 2 ? cc[2] : cc[3])));
      continue;
    }
    if (sp == 0) return false;
    node = stk[(--sp) * stride];
  }
}

template <int STACK, bool FAST>
__device__ __forceinline__ bool occluded(const DScene& S, V3 o, V3 d, double tmin, double tmax, uint32_t* stk) {
  if (FAST) return occluded_fast4<STACK>(S, o, d, tmin, tmax, stk, kBlock);
  return occluded_parity<STACK>(S, o, d, tmin, tmax, stk, kBlock);
}

// One ray per lane; out[i] = 0 or 1.
template <int STACK, bool FAST>
__global__ __launch_bounds__(kBlock, kTraceWaves) void k_occluded(DScene S, const rtx_ray* __restrict__ rays, int64_t n,
                                                                      uint8_t* __restrict__ out, double tmin,
                                                                      double tmax) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  uint32_t* stk = lds + threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const rtx_ray r = rays[i];
  const V3 o{r.origin[0], r.origin[1], r.origin[2]}, d{r.direction[0], r.direction[1], r.direction[2]};
  // (the parity walk where the two box tests part, as in k_intersect: fast_query_domain, and an
  // accepted primitive that a face-plane ray touches, face_plane_hit)
  bool occ;
  if (FAST && !fast_query_domain(o, d)) {
    occ = occluded<STACK, false>(S, o, d, tmin, tmax, stk);
  } else if (FAST) {
    int64_t who = -1;
    occ = occluded_fast4<STACK>(S, o, d, tmin, tmax, stk, kBlock, &who);
    if (occ && face_plane_hit(S, who, o, d)) occ = occluded<STACK, false>(S, o, d, tmin, tmax, stk);
  } else {
    occ = occluded<STACK, false>(S, o, d, tmin, tmax, stk);
  }
  out[i] = occ ? (uint8_t)1 : (uint8_t)0;
}

// ---------------------------------------------------------------------------------------
// Ambient occlusion
// ---------------------------------------------------------------------------------------
// The first hit under a pixel of the subset: the ray through the pixel's centre, exactly the ray
// k_aov traces (origin cam.center, no lens, no jitter).  pix: the global pixel index.
struct AoHit {
  V3 p, n;
  bool hit;
  uint32_t pix;
};
template <int STACK, bool FAST>
__device__ __forceinline__ AoHit ao_first_hit(const DScene& S, const rtx_camera& cam, const PixelMap& map, uint32_t local,
                                              uint32_t* stk) {
  int x, y;
  map.xy(local, x, y);
  const V3 c = v3(cam.center[0], cam.center[1], cam.center[2]);
  const V3 p00 = v3(cam.pixel00[0], cam.pixel00[1], cam.pixel00[2]);
  const V3 du = v3(cam.pixel_delta_u[0], cam.pixel_delta_u[1], cam.pixel_delta_u[2]);
  const V3 dv = v3(cam.pixel_delta_v[0], cam.pixel_delta_v[1], cam.pixel_delta_v[2]);
  const V3 d = ((p00 + ((double)x * du)) + ((double)y * dv)) - c;
  Counters cnt{};
  double tb;
  const int64_t best = trace<STACK, FAST, false>(S, c, d, (double)RTX_SEAM_TMIN, kInf, stk, cnt, tb);
  AoHit a;
  a.hit = best >= 0;
  a.pix = (uint32_t)(y * map.W + x);
  a.p = v3(0, 0, 0), a.n = v3(0, 0, 0);
  if (a.hit) {
    Hit h;
    finish_hit_at<false>(S, best, tb, c, d, h);
    a.p = h.p, a.n = h.normal;
  }
  return a;
}

// Sample `sample` of pixel `pix`: a unit cosine-weighted direction about the normal n
// (RandomCosineDirection over an ONB about n, the operations of the Lambertian chain in
// shade_core: r1, r2 drawn in that order, phi = 2 pi r1, (sqrt(r2) cos phi, sqrt(r2) sin phi,
// sqrt(1 - r2)) in the basis u = v x w, v = normalize(w x a), w = normalize(n)), from stream
// `stream` of (seed, pix, sample): kRngStreamAo for the AO pass (ao_direction: both k_ao and
// k_ao_rays call it), kRngStreamIrr for the irradiance queries (rtx_irradiance.h).
__device__ __forceinline__ V3 cosine_direction(uint64_t seed, uint32_t pix, uint32_t sample, uint32_t stream, V3 n) {
  Rng g = make_rng(seed, pix, sample, stream);
  const double r1 = g.next(), r2 = g.next();
  const V3 w = normalize(n);
  const V3 a = (fabs(w.x) > 0.9) ? v3(0, 1, 0) : v3(1, 0, 0);
  const V3 v = normalize(cross(w, a));
  const V3 u = cross(v, w);
  const double phi = 2.0 * kPi * r1;
  double cph, sph;
  cos_sin(phi, cph, sph);
  const double s = sqrt(r2);
  const double x = s * cph, y = s * sph, z = sqrt(1.0 - r2);
  return normalize(x * u + y * v + z * w);
}
__device__ __forceinline__ V3 ao_direction(uint64_t seed, uint32_t pix, uint32_t sample, V3 n) {
  return cosine_direction(seed, pix, sample, kRngStreamAo, n);
}

// One lane per pixel of the subset, in subset order: the first hit, then `samples` any-hit rays
// from the hit point on (RTX_SEAM_TMIN, radius); out = unoccluded / samples, 1 on a miss.  No ray
// goes through memory.  A pixel's value depends on its global index only, not on the subset or
// the launch shape.
template <int STACK, bool FAST>
__global__ __launch_bounds__(kBlock, kTraceWaves) void k_ao(DScene S, rtx_camera cam, PixelMap map, int64_t npix,
                                                                uint64_t seed, int32_t samples, double radius,
                                                                double* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  uint32_t* stk = lds + threadIdx.x;
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= npix) return;
  const AoHit a = ao_first_hit<STACK, FAST>(S, cam, map, (uint32_t)p, stk);
  if (!a.hit) {
    out[p] = 1.0;
    return;
  }
  int32_t open = 0;
  for (int32_t s = 0; s < samples; s++) {
    const V3 d = ao_direction(seed, a.pix, (uint32_t)s, a.n);
    open += occluded<STACK, FAST>(S, a.p, d, (double)RTX_SEAM_TMIN, radius, stk) ? 0 : 1;
  }
  out[p] = (double)open / (double)samples;
}

// Test hook (rtx_internal_ao_rays): the sample rays k_ao traces, npix * samples of them, pixel
// major; all zero for a pixel that misses.
template <int STACK, bool FAST>
__global__ __launch_bounds__(kBlock, kTraceWaves) void k_ao_rays(DScene S, rtx_camera cam, PixelMap map, int64_t npix,
                                                                     uint64_t seed, int32_t samples,
                                                                     rtx_ray* __restrict__ rays) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  uint32_t* stk = lds + threadIdx.x;
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= npix) return;
  const AoHit a = ao_first_hit<STACK, FAST>(S, cam, map, (uint32_t)p, stk);
  for (int32_t s = 0; s < samples; s++) {
    rtx_ray r{};
    if (a.hit) {
      const V3 d = ao_direction(seed, a.pix, (uint32_t)s, a.n);
      r.origin[0] = a.p.x, r.origin[1] = a.p.y, r.origin[2] = a.p.z;
      r.direction[0] = d.x, r.direction[1] = d.y, r.direction[2] = d.z;
    }
    rays[p * samples + s] = r;
  }
}

}  // namespace rtxd
