// rtx_nee.h — next-event estimation: radiance queries and frames that sample the lights
// (rtx_radiance_nee*, rtx_render_nee*, include/rtx.h; DESIGN.md §4h "Next-event estimation").
// Included once, by rtx_queries.hip, after rtx_direct.h.  Nothing here is used by a render kernel,
// and trace<>(), shade*, occluded<>(), k_radiance*, k_direct* are as they were: the kernels below
// call the same device functions.
//
// Contract: the path of (seed, pixel, sample) is k_radiance's path: per segment trace<> on
// ((double)0.001f, +inf), finish_hit<false>, then shade_core / shade_finish (the two halves of
// shade()) with stream depth + 1.  The emitter samples come from streams of their own
// (kRngStreamNee + depth), so the path's geometry, throughput, roulette decisions and closest-hit
// segment count are rtx_radiance's for the same key.  On top of that path:
//   term: at the hit of segment d, when the step's outcome is kShadeDiffuse (a Lambertian that
//     scattered), d + 1 < max_depth and the emitter table is usable (E.n > 0, A finite and > 0),
//     one direct_sample_from() of the surfel (rec.p, rec.normal) on stream kRngStreamNee + d; when
//     it is traceable V = !occluded<>() on (RTX_SEAM_TMIN, kDirectTmax) of its segment, with the
//     walk's own LDS stack column.  The term is w * (C V), w = thr * rho with thr the throughput on
//     arrival at the vertex and rho = mat_tex(S, m, rec); this vertex's roulette does not touch it.
//   suppression: a segment that ends the path with kShadeEmit on a hit below the depth limit (an
//     emitter's emission) contributes 0 when a term was eligible at the parent vertex (whether or
//     not its sample was traced or visible); emission after a specular parent and at segment 0 is
//     collected as before.
//   slot: (the terms added in depth order from 0) + L_end, plain f64; its segment count is the
//     closest-hit segments plus the shadow segments actually traced.
// With an unusable table or max_depth <= 1 no term is eligible and nothing is suppressed: the slot
// and its count are k_radiance's bit for bit.  k_radiance_sum resolves the slots as they are.
// A primitive that became a light through rtx_scene_update_prims is not in the emitter table
// (DESIGN.md §4g): after a diffuse vertex it is neither sampled nor counted.
//
// The same path with multiple importance sampling (rtx_radiance_mis*, rtx_render_mis*)
// is nee_path<.., MIS = true>: its contract stands at nee_path below.  Every kernel that existed is
// the MIS = false path.
#pragma once

#include "rtx_direct.h"

namespace rtxd {

// A vertex's flag word in the test hook's records (rtx_internal_nee_trace)
enum : uint32_t {
  kNeeEligible = 1u,    // a term was eligible at this vertex
  kNeeTraced = 2u,      // its sample was traceable: the shadow segment was traced
  kNeeVisible = 4u,     // ... and found unoccluded
  kNeeSuppressed = 8u,  // this segment ended the path on an emitter whose emission was suppressed
  kMisWeighted = 16u    // (rtx_internal_mis_trace) ... whose emission was weighted with a table member's gb
};

// What a path gives: the slot value's two parts and the two segment counts.
struct NeePath {
  V3 sum;    // the terms, added in depth order from 0
  V3 L_end;  // what the path's last segment contributed
  uint32_t closest, shadow;
};

// The kernels' recorder: nothing is kept per vertex.
struct NeeNoRecord {
  __device__ __forceinline__ void operator()(int32_t, const Hit&, bool, V3, uint32_t) const {}
  __device__ __forceinline__ void operator()(int32_t, const Hit&, bool, V3, uint32_t, double, double) const {}  // (MIS)
};

// Is `prim` (an index of the device primitive array) in the emitter table?  E.prim is ascending
// (rtx_scene_create fills it in the order of that array): a binary search.  E.n > 0.
__device__ __forceinline__ bool emitter_member(const EmitterTable& E, uint32_t prim) {
  int64_t lo = 0, hi = E.n - 1;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (E.prim[mid] < prim) lo = mid + 1;
    else hi = mid;
  }
  return E.prim[lo] == prim;
}

// The whole path of (seed, pix, smp) from the depth-0 segment (o, d).  rec(depth, hit record,
// hit?, w, flags) is called once per segment, after its step.
// MIS: the power-heuristic form (rtx_radiance_mis*, rtx_render_mis*; DESIGN.md §4i "Multiple
// importance sampling").  The same path, the same kRngStreamNee + d sample at each eligible
// vertex, the same two segment counts; only two weights differ.
//   light side: the term is (w * (C V)) * wl, wl = 1.0 / (1.0 + g * g), g the scalar of that sample
//     (direct_sample_g: C = g Le; g = p_bsdf / p_light at the pair, so wl is the power heuristic's
//     light weight; an infinite g gives 0).
//   BSDF side: the segment that ends the path with kShadeEmit on a hit below the depth limit after
//     a vertex where a term was eligible contributes wb * (thr * Le) instead of 0.  For a hit
//     primitive in the emitter table wb = 1.0 - 1.0 / (1.0 + gb * gb), with gb formed in
//     direct_sample_g's order: seg = tb * d (the segment from the parent vertex to the hit),
//     d2 = len2(seg), w = (1 / sqrt(d2)) seg, cy = |n_hit . w|, A the table's total area,
//     gb = ((cx * cy) * A) / (pi * d2), and cx = max(0, normalize(n_parent) . w') the one double
//     carried from the parent, formed there from the direction w' = (1 / sqrt(len2(d'))) d' that
//     shade_core chose (d' and tb d' point the same way).  A primitive outside the table (a light
//     made by rtx_scene_update_prims) and a NaN gb give wb = 1: the emission is kept.
//   kNeeSuppressed is never set.  rec gets two more doubles: g of the vertex's sample (0 where none
//   was traceable) and the gb applied to the segment's emission (0 where none applied).
// The two weights sum to 1 at every pair (x, y), so the expectation is the plain estimator's.
template <int STACK, bool FAST, bool MIS = false, class Rec>
__device__ __forceinline__ NeePath nee_path(const DScene& S, const EmitterTable& E, uint64_t seed, uint32_t pix,
                                            uint32_t smp, int32_t max_depth, V3 o, V3 d, uint32_t* stk, Rec&& rec) {
  bool usable = false;
  if (E.n > 0) {
    const double A = E.cum[E.n - 1];
    usable = A > 0.0 && A < kInf;
  }
  Path P;
  P.o = o, P.d = d;
  P.thr = v3(1.0, 1.0, 1.0);
  P.depth = 0;
  Counters c{};
  NeePath out;
  out.sum = v3(0.0, 0.0, 0.0);
  out.closest = 0, out.shadow = 0;
  bool parent = false;  // a term was eligible at the vertex this segment left
  double pcx = 0.0;     // MIS: that vertex's cosine toward this segment
  while (true) {
    double tb;
    const int64_t best = trace<STACK, FAST, false>(S, P.o, P.d, (double)0.001f, kInf, stk, c, tb);
    out.closest++;
    const bool hit = best >= 0;
    Hit h;
    if (hit) finish_hit<false>(S, best, P.o, P.d, (double)0.001f, h);
    const int32_t depth = P.depth;
    const V3 thr = P.thr;
    Rng g = make_rng(seed, pix, smp, (uint32_t)depth + 1u);
    rtx_material m;
    if (hit) m = S.mats[h.mat];
    ShadeOut so;
    shade_core<false, false>(S, max_depth, P, h, hit, g, m, so);  // (shade()'s two halves)
    V3 L;
    const bool cont = shade_finish(so, P.thr, P.depth, g, L);
    uint32_t flags = 0u;
    double gl = 0.0, gb = 0.0;  // MIS: what the recorder is told
    if (so.what == kShadeEmit && hit && depth < max_depth && parent) {
      if constexpr (MIS) {
        if (emitter_member(E, (uint32_t)best)) {  // (parent: the table is usable, E.n > 0)
          const V3 seg = tb * P.d;                // (shade_core left P.d alone: the step ended the path)
          const double d2 = len2(seg);
          const V3 wv = (1.0 / sqrt(d2)) * seg;
          const double cy = fabs(dot(h.normal, wv));
          const double A = E.cum[E.n - 1];
          const double gg = ((pcx * cy) * A) / (kPi * d2);
          if (gg == gg) {
            gb = gg;
            L = (1.0 - 1.0 / (1.0 + gg * gg)) * L;
            flags |= kMisWeighted;
          }
        }
      } else {
        L = v3(0.0, 0.0, 0.0);
        flags |= kNeeSuppressed;
      }
    }
    const bool eligible = so.what == kShadeDiffuse && depth + 1 < max_depth && usable;
    V3 w = v3(0.0, 0.0, 0.0);
    if (eligible) {
      flags |= kNeeEligible;
      w = thr * mat_tex(S, m, h);
      rtx_ray surfel;
      surfel.origin[0] = h.p.x, surfel.origin[1] = h.p.y, surfel.origin[2] = h.p.z;
      surfel.direction[0] = h.normal.x, surfel.direction[1] = h.normal.y, surfel.direction[2] = h.normal.z;
      V3 so_, sd, C;
      if constexpr (MIS) {
        // the one double the next segment's BSDF weight needs from this vertex, formed before the
        // shadow walk so that the normal need not live across it
        pcx = fmax(0.0, dot(normalize(h.normal), (1.0 / sqrt(len2(P.d))) * P.d));
      }
      if (direct_sample_g(S, E, seed, pix, smp, kRngStreamNee + (uint32_t)depth, surfel, so_, sd, C, gl)) {
        flags |= kNeeTraced;
        out.shadow++;
        if (occluded<STACK, FAST>(S, so_, sd, (double)RTX_SEAM_TMIN, kDirectTmax, stk)) C = v3(0.0, 0.0, 0.0);
        else flags |= kNeeVisible;
      }
      if constexpr (MIS) out.sum = out.sum + (1.0 / (1.0 + gl * gl)) * (w * C);
      else out.sum = out.sum + w * C;
    }
    if constexpr (MIS) rec(depth, h, hit, w, flags, gl, gb);
    else rec(depth, h, hit, w, flags);
    parent = eligible;
    if (!cont) {
      out.L_end = L;
      break;
    }
  }
  return out;
}

// The camera of the frame form: slot j's depth-0 segment is get_ray on stream 0 for sample
// s0 + j % K of pixel ray0 + j / K of the subset (k_ao's mapping), keyed by the global pixel
// index: the ray k_wf_generate makes and rtx_internal_camera_rays reports.
struct NeeCamera {
  rtx_camera cam;
  PixelMap map;
};

template <int STACK, bool FAST, bool CAMERA, bool MIS = false>
__device__ __forceinline__ void nee_slot(const DScene& S, const EmitterTable& E, const RadianceChunk& A,
                                         const NeeCamera* cam, uint32_t* stk) {
  const uint32_t j = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  if (j >= A.slots) return;
  const uint32_t r = j / A.K, k = j - r * A.K;
  const int64_t i = A.ray0 + (int64_t)r;
  const uint32_t smp = (uint32_t)A.s0 + k;
  uint32_t pix;
  V3 o, d;
  if (CAMERA) {
    int x, y;
    cam->map.xy((uint32_t)i, x, y);
    pix = (uint32_t)(y * cam->map.W + x);
    Rng g = make_rng(A.seed, pix, smp, 0u);
    get_ray(cam->cam, x, y, g, o, d);
  } else {
    const rtx_ray ray = A.rays[i];
    pix = A.ids ? A.ids[i] : (uint32_t)(A.id_base + (uint64_t)i);
    o = v3(ray.origin[0], ray.origin[1], ray.origin[2]);
    d = v3(ray.direction[0], ray.direction[1], ray.direction[2]);
  }
  const NeePath p = nee_path<STACK, FAST, MIS>(S, E, A.seed, pix, smp, A.max_depth, o, d, stk, NeeNoRecord{});
  const V3 L = p.sum + p.L_end;
  double* Lp = A.L + 3 * (uint64_t)j;
  Lp[0] = L.x, Lp[1] = L.y, Lp[2] = L.z;
  A.segs[j] = p.closest + p.shadow;
}

// One lane per slot, k_radiance's launch shape: the whole path with its emitter samples, the
// traversal stack (of the closest-hit walk and, between two of them, of the any-hit walk) in the
// lane's LDS column.
template <int STACK, bool FAST>
__global__ __launch_bounds__(kBlock, kTraceWaves) void k_radiance_nee(DScene S, EmitterTable E, RadianceChunk A) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  nee_slot<STACK, FAST, false>(S, E, A, nullptr, lds + threadIdx.x);
}
// The frame form: the same body from the camera's own depth-0 segments (A.rays and A.ids are not
// read; A.ray0 counts pixels of the subset).
template <int STACK, bool FAST>
__global__ __launch_bounds__(kBlock, kTraceWaves) void k_render_nee(DScene S, EmitterTable E, RadianceChunk A,
                                                                    NeeCamera cam) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  nee_slot<STACK, FAST, true>(S, E, A, &cam, lds + threadIdx.x);
}

// The MIS forms of the two (nee_path<.., MIS = true>): the same launch shape, arguments and slots.
template <int STACK, bool FAST>
__global__ __launch_bounds__(kBlock, kTraceWaves) void k_radiance_mis(DScene S, EmitterTable E, RadianceChunk A) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  nee_slot<STACK, FAST, false, true>(S, E, A, nullptr, lds + threadIdx.x);
}
template <int STACK, bool FAST>
__global__ __launch_bounds__(kBlock, kTraceWaves) void k_render_mis(DScene S, EmitterTable E, RadianceChunk A,
                                                                    NeeCamera cam) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  nee_slot<STACK, FAST, true, true>(S, E, A, &cam, lds + threadIdx.x);
}

// Test hook (rtx_internal_nee_samples): k_direct_samples on stream kRngStreamNee + depth, the
// samples nee_path draws at a vertex of that depth, from direct_sample_from(); 9 doubles per
// sample (segment origin, y - x, C), all zero where nothing is traced.
__global__ __launch_bounds__(kBlock) void k_nee_samples(DScene S, EmitterTable E, const rtx_ray* __restrict__ surfels,
                                                        const uint32_t* __restrict__ ids, uint32_t nslots, uint32_t K,
                                                        uint64_t seed, int32_t s0, uint32_t depth,
                                                        double* __restrict__ out) {
  const uint32_t j = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  if (j >= nslots) return;
  const uint32_t i = j / K, k = j - i * K;
  const rtx_ray surfel = surfels[i];
  V3 o, d, C;
  direct_sample_from(S, E, seed, ids ? ids[i] : i, (uint32_t)s0 + k, kRngStreamNee + depth, surfel, o, d, C);
  double* q = out + 9 * (uint64_t)j;
  q[0] = o.x, q[1] = o.y, q[2] = o.z, q[3] = d.x, q[4] = d.y, q[5] = d.z, q[6] = C.x, q[7] = C.y, q[8] = C.z;
}

// Test hook (rtx_internal_nee_trace): nee_path with a recorder.  Per slot and per segment below
// `cap`, 9 doubles (the vertex point, the shading normal, w; zero on a miss, w zero where no term
// is eligible) into verts and the flag word into flags; per slot L_end (3 doubles) into ends and
// the closest-hit and shadow segment counts into counts.  Records past the path's end are not
// written (the host zeroes the buffers).
struct NeeRecorder {
  double* verts;
  uint32_t* flags;
  int32_t cap;
  __device__ __forceinline__ void operator()(int32_t depth, const Hit& h, bool hit, V3 w, uint32_t f) const {
    if (depth >= cap) return;
    double* q = verts + 9 * depth;
    if (hit) q[0] = h.p.x, q[1] = h.p.y, q[2] = h.p.z, q[3] = h.normal.x, q[4] = h.normal.y, q[5] = h.normal.z;
    q[6] = w.x, q[7] = w.y, q[8] = w.z;
    flags[depth] = f;
  }
};
template <int STACK, bool FAST>
__global__ __launch_bounds__(kBlock, kTraceWaves) void k_nee_trace(DScene S, EmitterTable E, RadianceChunk A,
                                                                   int32_t cap, double* __restrict__ verts,
                                                                   uint32_t* __restrict__ flags,
                                                                   double* __restrict__ ends,
                                                                   uint32_t* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  uint32_t* stk = lds + threadIdx.x;
  const uint32_t j = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  if (j >= A.slots) return;
  const uint32_t r = j / A.K, k = j - r * A.K;
  const int64_t i = A.ray0 + (int64_t)r;
  const rtx_ray ray = A.rays[i];
  const uint32_t pix = A.ids ? A.ids[i] : (uint32_t)(A.id_base + (uint64_t)i);
  const NeeRecorder rec{verts + 9 * (uint64_t)j * (uint64_t)cap, flags + (uint64_t)j * (uint64_t)cap, cap};
  const NeePath p = nee_path<STACK, FAST>(S, E, A.seed, pix, (uint32_t)A.s0 + k, A.max_depth,
                                          v3(ray.origin[0], ray.origin[1], ray.origin[2]),
                                          v3(ray.direction[0], ray.direction[1], ray.direction[2]), stk, rec);
  double* e = ends + 3 * (uint64_t)j;
  e[0] = p.L_end.x, e[1] = p.L_end.y, e[2] = p.L_end.z;
  counts[2 * (uint64_t)j] = p.closest, counts[2 * (uint64_t)j + 1] = p.shadow;
}


// Test hook (rtx_internal_mis_trace): k_nee_trace for the MIS form.  11 doubles per segment: the
// nine of NeeRecorder, then g of the vertex's light sample (0 where none was traceable) and the gb
// applied to the segment's emission (0 where none applied).
struct MisRecorder {
  double* verts;
  uint32_t* flags;
  int32_t cap;
  __device__ __forceinline__ void operator()(int32_t depth, const Hit& h, bool hit, V3 w, uint32_t f, double g,
                                             double gb) const {
    if (depth >= cap) return;
    double* q = verts + 11 * depth;
    if (hit) q[0] = h.p.x, q[1] = h.p.y, q[2] = h.p.z, q[3] = h.normal.x, q[4] = h.normal.y, q[5] = h.normal.z;
    q[6] = w.x, q[7] = w.y, q[8] = w.z;
    q[9] = g, q[10] = gb;
    flags[depth] = f;
  }
};
template <int STACK, bool FAST>
__global__ __launch_bounds__(kBlock, kTraceWaves) void k_mis_trace(DScene S, EmitterTable E, RadianceChunk A,
                                                                   int32_t cap, double* __restrict__ verts,
                                                                   uint32_t* __restrict__ flags,
                                                                   double* __restrict__ ends,
                                                                   uint32_t* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  uint32_t* stk = lds + threadIdx.x;
  const uint32_t j = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  if (j >= A.slots) return;
  const uint32_t r = j / A.K, k = j - r * A.K;
  const int64_t i = A.ray0 + (int64_t)r;
  const rtx_ray ray = A.rays[i];
  const uint32_t pix = A.ids ? A.ids[i] : (uint32_t)(A.id_base + (uint64_t)i);
  const MisRecorder rec{verts + 11 * (uint64_t)j * (uint64_t)cap, flags + (uint64_t)j * (uint64_t)cap, cap};
  const NeePath p = nee_path<STACK, FAST, true>(S, E, A.seed, pix, (uint32_t)A.s0 + k, A.max_depth,
                                                v3(ray.origin[0], ray.origin[1], ray.origin[2]),
                                                v3(ray.direction[0], ray.direction[1], ray.direction[2]), stk, rec);
  double* e = ends + 3 * (uint64_t)j;
  e[0] = p.L_end.x, e[1] = p.L_end.y, e[2] = p.L_end.z;
  counts[2 * (uint64_t)j] = p.closest, counts[2 * (uint64_t)j + 1] = p.shadow;
}

}  // namespace rtxd
