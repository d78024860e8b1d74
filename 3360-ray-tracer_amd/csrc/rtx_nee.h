// rtx_nee.h — next-event estimation: radiance queries and frames that sample the lights
// (rtx_radiance_nee*, rtx_render_nee*, include/rtx.h; DESIGN.md §4h "Next-event estimation").
// Included once, by rtx_queries.hip, after rtx_direct.h.  Nothing here is used by a render kernel,
// and trace<>(), shade*, occluded<>(), k_radiance*, k_direct* are as they were: the kernels below
// call the same device functions, and decode and write their slots with rtx_radiance.h's
// chunk_slot / chunk_index and slot_write.
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
// is nee_path<.., MIS = true>: its contract stands at nee_path below.  One kernel, k_sampled, runs
// the path for both estimators, on rays and on the camera's frame.
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

// The kernels' recorder: nothing is kept per vertex (the last two arguments are the MIS form's).
struct NeeNoRecord {
  __device__ __forceinline__ void operator()(int32_t, const Hit&, bool, V3, uint32_t, double = 0.0, double = 0.0) const {}
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
// Sample smp of subset pixel i: the global pixel key and the depth-0 segment (the one definition of
// the camera form, k_sampled<.., CAMERA = true> and k_film_paths).
__device__ __forceinline__ void camera_slot(const NeeCamera& C, uint64_t seed, uint32_t i, uint32_t smp, uint32_t& pix,
                                            V3& o, V3& d) {
  int x, y;
  C.map.xy(i, x, y);
  pix = (uint32_t)(y * C.map.W + x);
  Rng g = make_rng(seed, pix, smp, 0u);
  get_ray(C.cam, x, y, g, o, d);
}

// The sampled path's one query kernel: one lane per slot, k_radiance's launch shape, the whole path
// with its emitter samples, the traversal stack (of the closest-hit walk and, between two of them,
// of the any-hit walk) in the lane's LDS column.  CAMERA = false: the caller's rays
// (rtx_radiance_nee*, rtx_radiance_mis*; `cam` is not read).  CAMERA = true: the frame form, the
// same body from the camera's own depth-0 segments (rtx_render_nee*, rtx_render_mis*; A.rays and
// A.ids are not read, A.ray0 counts pixels of the subset).  MIS: nee_path's power-heuristic form.
template <int STACK, bool FAST, bool CAMERA, bool MIS>
__global__ __launch_bounds__(kBlock, kTraceWaves) void k_sampled(DScene S, EmitterTable E, RadianceChunk A,
                                                                 NeeCamera cam) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  uint32_t* stk = lds + threadIdx.x;
  const uint32_t j = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  if (j >= A.slots) return;
  uint32_t pix, smp;
  V3 o, d;
  if (CAMERA) {
    int64_t i;
    uint32_t k;
    chunk_index(A, j, i, k);
    smp = (uint32_t)A.s0 + k;
    camera_slot(cam, A.seed, (uint32_t)i, smp, pix, o, d);
  } else {
    rtx_ray ray;
    chunk_slot(A, j, ray, pix, smp);
    o = v3(ray.origin[0], ray.origin[1], ray.origin[2]);
    d = v3(ray.direction[0], ray.direction[1], ray.direction[2]);
  }
  const NeePath p = nee_path<STACK, FAST, MIS>(S, E, A.seed, pix, smp, A.max_depth, o, d, stk, NeeNoRecord{});
  slot_write(A.L, A.segs, j, p.sum + p.L_end, p.closest + p.shadow);
}

// Test hook (rtx_internal_nee_trace, rtx_internal_mis_trace): nee_path with a recorder.  Per slot
// and per segment below `cap`, kDoubles doubles into verts and the flag word into flags: the vertex
// point, the shading normal, w (zero on a miss, w zero where no term is eligible), and with MIS g of
// the vertex's light sample (0 where none was traceable) and the gb applied to the segment's
// emission (0 where none applied): 9 or 11.  Per slot L_end (3 doubles) into ends and the
// closest-hit and shadow segment counts into counts.  Records past the path's end are not written
// (the host zeroes the buffers).
template <bool MIS>
struct NeeRecorder {
  static constexpr int kDoubles = MIS ? 11 : 9;
  double* verts;
  uint32_t* flags;
  int32_t cap;
  __device__ __forceinline__ void operator()(int32_t depth, const Hit& h, bool hit, V3 w, uint32_t f, double g = 0.0,
                                             double gb = 0.0) const {
    if (depth >= cap) return;
    double* q = verts + kDoubles * depth;
    if (hit) q[0] = h.p.x, q[1] = h.p.y, q[2] = h.p.z, q[3] = h.normal.x, q[4] = h.normal.y, q[5] = h.normal.z;
    q[6] = w.x, q[7] = w.y, q[8] = w.z;
    if (MIS) q[9] = g, q[10] = gb;
    flags[depth] = f;
  }
};
template <int STACK, bool FAST, bool MIS>
__global__ __launch_bounds__(kBlock, kTraceWaves) void k_path_trace(DScene S, EmitterTable E, RadianceChunk A,
                                                                    int32_t cap, double* __restrict__ verts,
                                                                    uint32_t* __restrict__ flags,
                                                                    double* __restrict__ ends,
                                                                    uint32_t* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  uint32_t* stk = lds + threadIdx.x;
  const uint32_t j = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  if (j >= A.slots) return;
  rtx_ray ray;
  uint32_t pix, smp;
  chunk_slot(A, j, ray, pix, smp);
  using Rec = NeeRecorder<MIS>;
  const Rec rec{verts + Rec::kDoubles * (uint64_t)j * (uint64_t)cap, flags + (uint64_t)j * (uint64_t)cap, cap};
  const NeePath p = nee_path<STACK, FAST, MIS>(S, E, A.seed, pix, smp, A.max_depth,
                                               v3(ray.origin[0], ray.origin[1], ray.origin[2]),
                                               v3(ray.direction[0], ray.direction[1], ray.direction[2]), stk, rec);
  double* e = ends + 3 * (uint64_t)j;
  e[0] = p.L_end.x, e[1] = p.L_end.y, e[2] = p.L_end.z;
  counts[2 * (uint64_t)j] = p.closest, counts[2 * (uint64_t)j + 1] = p.shadow;
}

}  // namespace rtxd
