// rtx_shade_steps.h — test hook (rtx_internal_shade_steps, rtx_queries.hip; not in rtx.h): one
// shading step per case, one lane per case, through the device functions the render kernels call
// (csrc/rtx_device.h), on a real rtx_scene: the uploaded material table, the texture and image
// tables and the all_lambertian / no_textures flags are the renderer's own.  Each case supplies a
// hit record, a path state and the Philox key of its path; the record it gets back is the step's
// whole outcome, compared bit for bit with the CPU oracle's (orc_shade_steps,
// oracle/rtx_oracle.cc; tests/test_gpu_shade_steps.py).  No timed kernel includes this header.
#pragma once

#include "rtx_device.h"
#include "rtx_kernels.h"

namespace rtxd {

struct ShadeCase {
  double p[3], normal[3], u, v;  // the hit record (read on a hit)
  double o[3], d[3], thr[3];     // the path state
  uint64_t seed;                 // make_rng(seed, pixel, sample, the segment's stream)
  uint32_t pixel, sample;
  int32_t hit, front_face, mat;
  int32_t depth, max_depth;  // kShadeFormScatter: depth is the remaining depth, as k_persistent has it
  int32_t lazy_uv;           // Hit::lazy_uv: the primitive whose u, v are derived from p, or -1
};
struct ShadeRecord {
  double L[3];                // the radiance of a path that ended (0 0 0 of one that continues)
  double o[3], d[3], thr[3];  // the child (all zero when the path ended)
  double next;                // the next draw of the segment's stream: stands for the draws consumed
  int32_t cont, depth;        // cont -1: kShadeFormTerminal asked of a case that does not end on the sky
};
static_assert(sizeof(ShadeCase) == 176 && sizeof(ShadeRecord) == 112, "shade step layouts");

enum : int {
  kShadeFormShade = 0,     // shade(), as k_wf_shade, k_radiance and k_irradiance call it
  kShadeFormCore = 1,      // shade_core<LAMB, NOTEX, SET_ORIGIN> then shade_finish, as k_persistent's shade_segment
  kShadeFormTerminal = 2,  // shade_terminal, as k_persistent ends a miss or a segment at the depth limit
  kShadeFormScatter = 3    // the scatter-API branch of k_persistent: sky / mat_scatter / mat_emitted
};

template <int FORM, bool LAMB = false, bool NOTEX = false, bool SET_ORIGIN = true>
__global__ __launch_bounds__(kBlock) void k_shade_steps(DScene S, const ShadeCase* __restrict__ cases, int64_t n,
                                                        ShadeRecord* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const ShadeCase c = cases[i];
  Hit h;
  h.p = v3(c.p[0], c.p[1], c.p[2]), h.normal = v3(c.normal[0], c.normal[1], c.normal[2]);
  h.t = 0.0, h.u = c.u, h.v = c.v, h.mat = c.mat, h.front_face = c.front_face, h.lazy_uv = c.lazy_uv;
  const bool hit = c.hit != 0;
  Path P;
  P.o = v3(c.o[0], c.o[1], c.o[2]), P.d = v3(c.d[0], c.d[1], c.d[2]), P.thr = v3(c.thr[0], c.thr[1], c.thr[2]);
  P.depth = c.depth;
  Rng g = make_rng(c.seed, c.pixel, c.sample,
                   FORM == kShadeFormScatter ? (uint32_t)(c.max_depth - P.depth) + 1u : (uint32_t)P.depth + 1u);
  V3 L = v3(0, 0, 0);
  int32_t cont = 0;
  if constexpr (FORM == kShadeFormShade) {
    cont = shade(S, c.max_depth, P, h, hit, g, L);
  } else if constexpr (FORM == kShadeFormCore) {
    ShadeOut so;
    const rtx_material& mr = *opaque(S.mats + (hit ? h.mat : 0));
    shade_core<LAMB, NOTEX, SET_ORIGIN>(S, c.max_depth, P, h, hit, g, mr, so);
    V3 thr = P.thr;
    cont = shade_finish(so, thr, P.depth, g, L, hit ? S.mats + h.mat : S.mats);
    if (cont) P.thr = thr;
    if (!SET_ORIGIN && cont) P.o = h.p;  // the caller's part (k_persistent: the hit point parked in LDS)
  } else if constexpr (FORM == kShadeFormTerminal) {
    if (!hit || P.depth >= c.max_depth) L = shade_terminal(P.d, P.thr);
    else cont = -1;
  } else {
    if (!hit) {
      L = P.thr * sky(P.d);
    } else {
      const rtx_material m = S.mats[h.mat];
      V3 att, sd;
      if (mat_scatter(S, m, P.d, h, att, sd, g)) {
        P.thr = P.thr * att;
        P.o = h.p, P.d = sd;
        P.depth--;
        cont = 1;
      } else {
        L = P.thr * mat_emitted(S, m, h);
      }
    }
  }
  ShadeRecord r;
  const bool on = cont == 1;
  const V3 z = v3(0, 0, 0), ro = on ? P.o : z, rd = on ? P.d : z, rt = on ? P.thr : z;
  r.L[0] = L.x, r.L[1] = L.y, r.L[2] = L.z;
  r.o[0] = ro.x, r.o[1] = ro.y, r.o[2] = ro.z;
  r.d[0] = rd.x, r.d[1] = rd.y, r.d[2] = rd.z;
  r.thr[0] = rt.x, r.thr[1] = rt.y, r.thr[2] = rt.z;
  r.next = g.next();
  r.cont = cont, r.depth = on ? P.depth : 0;
  out[i] = r;
}

}  // namespace rtxd
