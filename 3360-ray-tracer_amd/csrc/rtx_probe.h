// rtx_probe.h — light probes: the radiance over the whole sphere about caller-supplied points,
// projected onto real spherical harmonics to band 2 (rtx_probe_sh*, include/rtx.h; DESIGN.md §4k
// "Light probes").  Included once, by rtx_queries.hip, after rtx_nee.h.  Nothing here is used by a
// render kernel, and k_radiance, k_irradiance, k_sampled, k_radiance_sum, nee_path and trace<>() are
// as they were: the kernels below call the same device functions.
//
// Contract: a probe is three doubles.  Sample k of probe i starts a path at the point along
// probe_ray()'s direction: z = 1 - 2 u1, phi = 2 pi u2, r = sqrt(max(0, 1 - z z)),
// d = (r cos phi, r sin phi, z) with u1, u2 the first two draws of stream kRngStreamProbe of
// (seed, pixel, first_sample + k): uniform over the sphere.  From there the lane runs k_radiance's
// loop (EST == 0) or nee_path (RTX_ESTIMATOR_NEE, _MIS) on their operands, so the slot value and
// its segment count are, bit for bit, rtx_radiance / rtx_radiance_nee / rtx_radiance_mis of that
// one ray with the same pixel key, spp = 1 and first_sample + k.  The probe is no vertex: nee_path
// collects emission at segment 0 in full.  k_probe_sum makes the direction again from the one
// function, forms the nine basis values (sh_basis: the operations rtx.h lists, no contraction) and
// adds the 27 products Y_j * L[c] in sample order from 0; the last chunk resolves
// kFourPi * ((1.0 / (double)(float)spp) * sum).
//
// The points: the chunk does not stage them as rtx_ray.  The kernels take the caller's points
// pointer (3 doubles per probe) next to the RadianceChunk, whose `rays` stays null and unread;
// ray0, ids, id_base, K, s0 and the slot layout are read as every query kernel reads them
// (chunk_index).  So the device entry point traces the caller's buffer as it is, 24 bytes per probe.
//
// The back-face bit: a slot's count word holds its segments in the low 31 bits and, in bit 31,
// whether the depth-0 segment hit a primitive with front_face == 0.  A path's segments stay below
// 2^31: with RTX_ESTIMATOR_NEE / _MIS at most 2 * (0x00FFFFFF + 1) (the entry points' depth cap,
// closest-hit plus shadow segments); with the plain path at most max_depth + 1 <= 2^31, and 2^31
// itself would need Russian roulette (survival at most 0.95 per bounce past depth 5) to pass
// 2^31 - 6 times.
#pragma once

#include "rtx_nee.h"

namespace rtxd {

constexpr double kFourPi = 4.0 * kPi;  // (exact: a power of two times kPi)
constexpr uint32_t kProbeBackBit = 0x80000000u;

// The depth-0 segment of sample `smp` of a probe at `point`: the one definition, called by
// k_probe, k_probe_sum and k_probe_rays.  false: a non-finite coordinate, for which nothing is
// traced (o and d are left alone).
__device__ __forceinline__ bool probe_ray(uint64_t seed, uint32_t pix, uint32_t smp, V3 point, V3& o, V3& d) {
  if (!(fabs(point.x) < kInf) || !(fabs(point.y) < kInf) || !(fabs(point.z) < kInf)) return false;
  Rng g = make_rng(seed, pix, smp, kRngStreamProbe);
  const double u1 = g.next(), u2 = g.next();
  const double z = 1.0 - 2.0 * u1;
  const double phi = 2.0 * kPi * u2;
  const double r = sqrt(fmax(0.0, 1.0 - z * z));
  double cph, sph;
  cos_sin(phi, cph, sph);
  o = point;
  d = v3(r * cph, r * sph, z);
  return true;
}

// The nine real orthonormal SH basis values of bands 0..2 at d (include/rtx.h: this order, these
// operations)
__device__ __forceinline__ void sh_basis(V3 d, double Y[RTX_SH_COEFFS]) {
  const double x = d.x, y = d.y, z = d.z;
  Y[0] = RTX_SH_K0;
  Y[1] = RTX_SH_K1 * y;
  Y[2] = RTX_SH_K1 * z;
  Y[3] = RTX_SH_K1 * x;
  Y[4] = RTX_SH_K4 * (x * y);
  Y[5] = RTX_SH_K4 * (y * z);
  Y[6] = RTX_SH_K6 * (3.0 * (z * z) - 1.0);
  Y[7] = RTX_SH_K4 * (x * z);
  Y[8] = RTX_SH_K8 * (x * x - y * y);
}

// Slot j of a probe chunk: the probe's point, pixel key and sample number (chunk_index's layout;
// A.rays is not read)
__device__ __forceinline__ void probe_slot(const RadianceChunk& A, const double* __restrict__ points, uint32_t j,
                                           V3& point, uint32_t& pix, uint32_t& smp) {
  int64_t i;
  uint32_t k;
  chunk_index(A, j, i, k);
  const double* p = points + 3 * i;
  point = v3(p[0], p[1], p[2]);
  pix = A.ids ? A.ids[i] : (uint32_t)(A.id_base + (uint64_t)i);
  smp = (uint32_t)A.s0 + k;
}

// nee_path's recorder of k_probe: only the depth-0 segment's front_face is kept.
struct ProbeRecorder {
  uint32_t back = 0u;
  __device__ __forceinline__ void operator()(int32_t depth, const Hit& h, bool hit, V3, uint32_t, double = 0.0,
                                             double = 0.0) {
    if (depth == 0 && hit && !h.front_face) back = kProbeBackBit;
  }
};

// One lane per slot of the chunk, k_radiance's launch shape, kTraceWaves and LDS stack column: slot
// j is sample s0 + j % K of probe ray0 + j / K.  EST == 0: the whole path per lane with
// k_radiance's loop (from `P.thr` to the loop's end the text is k_radiance's and k_irradiance's,
// but for the back-face line: change all or none).  EST == RTX_ESTIMATOR_NEE / _MIS: nee_path, as
// k_sampled calls it.  A non-finite probe's lanes write 0 and leave.
template <int STACK, bool FAST, int EST>
__global__ __launch_bounds__(kBlock, kTraceWaves) void k_probe(DScene S, EmitterTable E, RadianceChunk A,
                                                               const double* __restrict__ points) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  uint32_t* stk = lds + threadIdx.x;
  const uint32_t j = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  if (j >= A.slots) return;
  V3 point;
  uint32_t pix, smp;
  probe_slot(A, points, j, point, pix, smp);
  Path P;
  if (!probe_ray(A.seed, pix, smp, point, P.o, P.d)) {
    slot_write(A.L, A.segs, j, v3(0.0, 0.0, 0.0), 0u);
    return;
  }
  if constexpr (EST == 0) {
    P.thr = v3(1.0, 1.0, 1.0);
    P.depth = 0;
    Counters c{};
    uint32_t segs = 0;  // (bit 31: the back-face bit)
    V3 L;
    while (true) {
      double tb;
      const int64_t best = trace<STACK, FAST, false>(S, P.o, P.d, (double)0.001f, kInf, stk, c, tb);
      segs++;
      Hit h;
      if (best >= 0) finish_hit<false>(S, best, P.o, P.d, (double)0.001f, h);
      if (P.depth == 0 && best >= 0 && !h.front_face) segs |= kProbeBackBit;
      Rng g = make_rng(A.seed, pix, smp, (uint32_t)P.depth + 1u);
      if (!shade(S, A.max_depth, P, h, best >= 0, g, L)) break;
    }
    slot_write(A.L, A.segs, j, L, segs);
  } else {
    ProbeRecorder rec;
    const NeePath p =
        nee_path<STACK, FAST, EST == RTX_ESTIMATOR_MIS>(S, E, A.seed, pix, smp, A.max_depth, P.o, P.d, stk, rec);
    slot_write(A.L, A.segs, j, p.sum + p.L_end, (p.closest + p.shadow) | rec.back);
  }
}

// One lane per probe of the chunk: for each of its K slots in order the direction again from
// probe_ray(), the nine basis values, and the 27 products added to the running sums (plain f64,
// from 0); the segment and back-face totals from the slots' count words.  A probe whose samples
// span several chunks carries the 27 sums and the two counts through `carry` (28 doubles per
// probe: the sums, then the two counts in the last double's bytes; first: this chunk starts the
// probe, last: it ends it), so the additions and their order do not depend on the chunking.  The
// last chunk resolves kFourPi * ((1.0 / (double)(float)spp) * sum).  A non-finite probe adds
// nothing: its slots are zero and its sums stay +0.
constexpr int kProbeCarry = 3 * RTX_SH_COEFFS + 1;
__global__ __launch_bounds__(kBlock) void k_probe_sum(RadianceChunk A, const double* __restrict__ points, int64_t nprobes,
                                                      int first, int last, int32_t spp, double* carry,
                                                      double* __restrict__ out_sh, uint32_t* __restrict__ out_segs,
                                                      uint32_t* __restrict__ out_back) {
  const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (r >= nprobes) return;
  double sum[3 * RTX_SH_COEFFS];
  uint32_t ns = 0, nb = 0;
  if (first) {
#pragma unroll
    for (int q = 0; q < 3 * RTX_SH_COEFFS; q++) sum[q] = 0.0;
  } else {
    const double* cr = carry + (int64_t)kProbeCarry * r;
#pragma unroll
    for (int q = 0; q < 3 * RTX_SH_COEFFS; q++) sum[q] = cr[q];
    const uint32_t* cw = (const uint32_t*)(cr + 3 * RTX_SH_COEFFS);
    ns = cw[0], nb = cw[1];
  }
  const uint32_t j0 = (uint32_t)r * A.K;  // (the probe's first slot: nprobes * K = A.slots fits 32 bits)
  V3 point;
  uint32_t pix, smp;
  probe_slot(A, points, j0, point, pix, smp);
  for (uint32_t k = 0; k < A.K; k++) {
    V3 o, d;
    if (!probe_ray(A.seed, pix, smp + k, point, o, d)) break;
    double Y[RTX_SH_COEFFS];
    sh_basis(d, Y);
    const double* x = A.L + 3 * (uint64_t)(j0 + k);
    const double L0 = x[0], L1 = x[1], L2 = x[2];
#pragma unroll
    for (int q = 0; q < RTX_SH_COEFFS; q++) {
      sum[3 * q] += Y[q] * L0;
      sum[3 * q + 1] += Y[q] * L1;
      sum[3 * q + 2] += Y[q] * L2;
    }
    const uint32_t w = A.segs[j0 + k];
    ns += w & ~kProbeBackBit, nb += w >> 31;
  }
  if (last) {
    const double sc = 1.0 / (double)(float)spp;
    double* o = out_sh + 3 * RTX_SH_COEFFS * r;
#pragma unroll
    for (int q = 0; q < 3 * RTX_SH_COEFFS; q++) o[q] = kFourPi * (sc * sum[q]);
    if (out_segs) out_segs[r] = ns;
    if (out_back) out_back[r] = nb;
  } else {
    double* cr = carry + (int64_t)kProbeCarry * r;
#pragma unroll
    for (int q = 0; q < 3 * RTX_SH_COEFFS; q++) cr[q] = sum[q];
    uint32_t* cw = (uint32_t*)(cr + 3 * RTX_SH_COEFFS);
    cw[0] = ns, cw[1] = nb;
  }
}

// Test hook (rtx_internal_probe_rays): the depth-0 segments k_probe traces, one lane per (probe,
// sample), probe major, from probe_ray(); 6 doubles per ray (origin, direction), all zero for a
// non-finite probe.
__global__ __launch_bounds__(kBlock) void k_probe_rays(const double* __restrict__ points,
                                                       const uint32_t* __restrict__ ids, uint32_t nslots, uint32_t K,
                                                       uint64_t seed, int32_t s0, double* __restrict__ out) {
  const uint32_t j = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  if (j >= nslots) return;
  const uint32_t i = j / K, k = j - i * K;
  const double* p = points + 3 * (uint64_t)i;
  V3 o = v3(0, 0, 0), d = v3(0, 0, 0);  // (kept where probe_ray() returns false)
  probe_ray(seed, ids ? ids[i] : i, (uint32_t)s0 + k, v3(p[0], p[1], p[2]), o, d);
  double* q = out + 6 * (uint64_t)j;
  q[0] = o.x, q[1] = o.y, q[2] = o.z, q[3] = d.x, q[4] = d.y, q[5] = d.z;
}

}  // namespace rtxd
