// rtx_radiance.h — radiance queries: the bounce loop on caller-supplied rays (rtx_radiance*,
// include/rtx.h; DESIGN.md §4e "Radiance queries").  Included once, by rtx_queries.hip, after the
// trace kernels.  Nothing here is used by a render kernel: k_persistent, k_wf_*, k_intersect and
// trace<>() are as they were; the kernels below call the same device functions.  The slot decode
// (chunk_slot) and the slot write (slot_write) defined here are the one definition every query
// kernel that takes a RadianceChunk shares.  The bounce loop stands three times, here, in
// k_irradiance and in k_probe (rtx_probe.h), token for token: as a function of its own it costs the kernels registers (the
// parity walk: 48 -> 64 B of scratch, 28 -> 40 spilled VGPRs), so it stays written out.
//
// Contract: for ray i and sample k the lane traces the path the wavefront renderer traces from
// the same depth-0 segment: per segment the closest hit of k_wf_extend (trace<> on
// ((double)0.001f, +inf)), then k_wf_shade's finish_hit<false> and shade() with the stream
// depth + 1 of (seed, pixel, sample), until shade() returns false.  Stream 0 (the camera ray's)
// is never opened.  Every operation that forms the radiance is one of those device functions on
// the same operands, so the value equals the renderer's slot value bit for bit.
#pragma once

#include "rtx_kernels.h"

namespace rtxd {

// One chunk of a call: rays [ray0, ray0 + slots / K) of the caller's arrays, samples
// [s0, s0 + K) of each; slot j is sample s0 + j % K of ray ray0 + j / K (a ray's slots are
// adjacent, rays in caller order).
struct RadianceChunk {
  const rtx_ray* rays;
  const uint32_t* ids;  // may be null: the pixel key is id_base + the ray's index
  int64_t ray0;
  uint64_t id_base;
  uint32_t slots;       // <= kRadianceSlotsMax
  uint32_t K;
  int32_t s0;
  int32_t max_depth;
  uint64_t seed;
  double* L;            // 3 doubles per slot
  uint32_t* segs;       // segments per slot
};

// Slot j of a chunk: the index i of its ray in the caller's arrays and its sample's place k in the
// chunk (sample s0 + k) ...
__device__ __forceinline__ void chunk_index(const RadianceChunk& A, uint32_t j, int64_t& i, uint32_t& k) {
  const uint32_t r = j / A.K;
  k = j - r * A.K;
  i = A.ray0 + (int64_t)r;
}
// ... and the caller's ray (or surfel), pixel key and sample number: the one decode of every kernel
// that takes a RadianceChunk of caller-supplied rays
__device__ __forceinline__ void chunk_slot(const RadianceChunk& A, uint32_t j, rtx_ray& ray, uint32_t& pix,
                                           uint32_t& smp) {
  int64_t i;
  uint32_t k;
  chunk_index(A, j, i, k);
  ray = A.rays[i];
  pix = A.ids ? A.ids[i] : (uint32_t)(A.id_base + (uint64_t)i);
  smp = (uint32_t)A.s0 + k;
}
// Slot j's result: three doubles and a count
__device__ __forceinline__ void slot_write(double* L, uint32_t* segs, uint32_t j, V3 v, uint32_t n) {
  double* Lp = L + 3 * (uint64_t)j;
  Lp[0] = v.x, Lp[1] = v.y, Lp[2] = v.z;
  segs[j] = n;
}

// One lane per slot: the whole path, the traversal stack in the lane's LDS column as in
// k_intersect.  A lane whose path has ended idles until its wave's longest path ends (no refill).
// (From `P.thr` to the loop's end the text is k_irradiance's too, and k_probe<.., 0>'s in
// rtx_probe.h but for its back-face line: change all or none.)
template <int STACK, bool FAST>
__global__ __launch_bounds__(kBlock, kTraceWaves) void k_radiance(DScene S, RadianceChunk A) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  uint32_t* stk = lds + threadIdx.x;
  const uint32_t j = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  if (j >= A.slots) return;
  rtx_ray ray;
  uint32_t pix, smp;
  chunk_slot(A, j, ray, pix, smp);
  Path P;
  P.o = v3(ray.origin[0], ray.origin[1], ray.origin[2]);
  P.d = v3(ray.direction[0], ray.direction[1], ray.direction[2]);
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

// One lane per ray of the chunk: the ray's K slot radiances added in sample order (plain f64
// adds, from 0 as k_accumulate_sum starts a pixel's sum) and its segment total.  A ray whose
// samples span several chunks carries both through `carry` / `carry_segs` (first: this chunk
// starts the ray; last: it ends it), so the additions and their order do not depend on the
// chunking.  The last chunk writes k_accumulate_sum's resolve: (1 / (double)(float)spp) * sum.
__global__ __launch_bounds__(kBlock) void k_radiance_sum(const double* __restrict__ L,
                                                         const uint32_t* __restrict__ segs, int64_t nrays, uint32_t K,
                                                         int first, int last, int32_t spp, double* carry,
                                                         uint32_t* carry_segs, double* __restrict__ out_rgb,
                                                         uint32_t* __restrict__ out_segs) {
  const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (r >= nrays) return;
  double sum[3] = {0, 0, 0};
  uint32_t ns = 0;
  if (!first) {
    for (int c = 0; c < 3; c++) sum[c] = carry[3 * r + c];
    ns = carry_segs[r];
  }
  const double* x = L + 3 * (uint64_t)r * K;
  for (uint32_t k = 0; k < K; k++)
    for (int c = 0; c < 3; c++) sum[c] += x[3 * (uint64_t)k + c];
  for (uint32_t k = 0; k < K; k++) ns += segs[(uint64_t)r * K + k];
  if (last) {
    const double sc = 1.0 / (double)(float)spp;
    for (int c = 0; c < 3; c++) out_rgb[3 * r + c] = sc * sum[c];
    if (out_segs) out_segs[r] = ns;
  } else {
    for (int c = 0; c < 3; c++) carry[3 * r + c] = sum[c];
    carry_segs[r] = ns;
  }
}

}  // namespace rtxd
