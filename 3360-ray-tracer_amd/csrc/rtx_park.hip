// PARK instantiations of the persistent kernel (k_persistent<STACK, true, COUNT, SCATTER,
// PARK = 1 or 2>), compiled apart from rtx_capi.hip so this translation unit can have its own
// per-TU choices (RTX_PARK_TU: see the top of rtx_device.h) and scheduler options (Makefile
// PARKFLAGS).  k_persistent refuses to be instantiated with PARK > 0 anywhere else.
#define RTX_PARK_TU 1
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "rtx.h"
#include "rtx_host.h"  // (the test hooks at the end: error reporting, device buffers, the scene)
#include "rtx_kernels.h"

namespace rtxd {
#define RTX_PARK_DEFINE(ST, CO, SC, MP, PK)                                                                     \
  template __global__ void k_persistent<ST, true, CO, SC, PK, -1, false, false, false, MP>(RenderArgs,          \
                                                                                          unsigned long long*);
RTX_PARK_INSTANCES(RTX_PARK_DEFINE)
#undef RTX_PARK_DEFINE
#define RTX_PARK_TRI_DEFINE(ST, MP, PK)                                                                              \
  template __global__ void k_persistent<ST, true, false, false, PK, RTX_PRIM_TRIANGLE, false, false, false, MP>(    \
      RenderArgs, unsigned long long*);                                                                              \
  template __global__ void k_persistent<ST, true, false, false, PK, RTX_PRIM_TRIANGLE, true, false, false, MP>(     \
      RenderArgs, unsigned long long*);                                                                              \
  template __global__ void k_persistent<ST, true, false, false, PK, RTX_PRIM_TRIANGLE, true, true, false, MP>(      \
      RenderArgs, unsigned long long*);
RTX_PARK_TRI_INSTANCES(RTX_PARK_TRI_DEFINE)
#undef RTX_PARK_TRI_DEFINE

// The three forms of the Lambertian cos/sin (cos_sin, rtx_device.h) side by side, compiled here
// with the flags of the kernels that select among them: one lane per angle, phi[i] for i < n, then
// n_draws angles 2*pi*r1 with r1 the first draw of a segment's stream, made as shade_core makes it
// (angle j: pixel j >> 5, sample (j >> 3) & 3, depth j & 7).  Each form gets its own opaque copy
// of the angle, so none is folded into another.  bad: the angles at which the forms' bits differ;
// cs (or null): the library form's cos and sin of phi[i].
__global__ void k_cos_sin_forms(const double* __restrict__ phi, int64_t n, uint64_t seed, int64_t n_draws,
                                unsigned long long* bad, double* first_bad, double* __restrict__ cs) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n + n_draws;
       i += (int64_t)gridDim.x * blockDim.x) {
    double x;
    if (i < n) {
      x = phi[i];
    } else {
      const uint64_t j = (uint64_t)(i - n);
      Rng g = make_rng(seed, (uint32_t)(j >> 5), (uint32_t)(j >> 3) & 3u, ((uint32_t)j & 7u) + 1u);
      const double r1 = g.next();
      x = 2.0 * kPi * r1;
    }
    double xa = x, xb = x, xc = x;
    asm volatile("" : "+v"(xa));
    asm volatile("" : "+v"(xb));
    asm volatile("" : "+v"(xc));
    double c0, s0, c1, s1, c2, s2;
    cos_sin<kCosSinLib>(xa, c0, s0);
    cos_sin<kCosSinEach>(xb, c1, s1);
    cos_sin<kCosSinShared>(xc, c2, s2);
    const long long bc = __double_as_longlong(c0), bs = __double_as_longlong(s0);
    if (__double_as_longlong(c1) != bc || __double_as_longlong(c2) != bc || __double_as_longlong(s1) != bs ||
        __double_as_longlong(s2) != bs) {
      if (atomicAdd(bad, 1ull) == 0) *first_bad = x;
    }
    if (cs && i < n) cs[2 * i] = c0, cs[2 * i + 1] = s0;
  }
}

// One wave per block walks `lanes` rays (1..64, one per lane, the other lanes idle) through the
// fast tree with the speculative walk of k_persistent's PARK 2 builds (no parking, the tree
// alone: no global primitives, closest starts at +inf), each lane logging its node visits and
// primitive tests (CountersSeq).  It is the counting, generic-kind instantiation of
// trace4_run_spec (COUNT on, KIND -1), not the flagship's (COUNT off, triangles only): the
// queueing, sort and push are the same template text, so the order is the flagship's by
// construction, not by the same instructions.  fray: the lane's 15 slab constants (make_fray4l) as words.
template <int STACK>
__global__ void __launch_bounds__(64) k_visit_order(DScene S, const double* __restrict__ rays, int64_t n, int lanes,
                                                    double tmin, int32_t* seq, double* tseq, int32_t* len,
                                                    uint32_t* fray) {
  __shared__ uint16_t stk[(STACK + 1) * 64];
  __shared__ uint32_t lq[kLeafQueue * 64];
  const int lane = (int)threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * lanes + lane;
  if (lane >= lanes || i >= n) return;
  const V3 o{rays[6 * i], rays[6 * i + 1], rays[6 * i + 2]}, d{rays[6 * i + 3], rays[6 * i + 4], rays[6 * i + 5]};
  const FRay4L r = make_fray4l(o, d);
  const float rf[12] = {r.iex, r.iey, r.iez, r.nex, r.ney, r.nez, r.ixx, r.ixy, r.ixz, r.nxx, r.nxy, r.nxz};
  for (int k = 0; k < 12; k++) fray[15 * i + k] = __float_as_uint(rf[k]);
  fray[15 * i + 12] = r.ox, fray[15 * i + 13] = r.oy, fray[15 * i + 14] = r.oz;
  CountersSeq c{};
  c.seq = seq + kSeqCap * i, c.tseq = tseq + kSeqCap * i, c.n = 0;
  TravState ts;
  trav_init(ts, kInf);
  trace4_run_spec<STACK, true, -1>(S, o, d, tmin, stk + lane, lq + lane, 64, c, ts, -1);
  len[i] = (int32_t)c.n;
}
}  // namespace rtxd

// Test hook (not in rtx.h; tests/test_gpu_cos_sin_forms.py): the forms of cos_sin on n caller
// angles (0 <= phi < 2^30) and n_draws sampler angles.  mismatches: the angles at which any two
// forms differ in a bit of cos or sin, first_bad one of them; cs (or null): 2 * n doubles, the
// library's cos and sin of each caller angle.
extern "C" int rtx_internal_cos_sin_forms(int device, const double* phi, int64_t n, uint64_t seed, int64_t n_draws,
                                          int64_t* mismatches, double* first_bad, double* cs) {
  if (n < 0 || n_draws < 0 || n + n_draws > ((int64_t)1 << 32) || (n > 0 && !phi) || !mismatches)
    return fail(RTX_ERR_INVALID, "bad argument");
  HIPC(hipSetDevice(device));
  DevBuf res, in, out;
  int rc;
  if ((rc = res.reserve(2 * sizeof(unsigned long long)))) return rc;
  if ((rc = in.reserve((size_t)n * sizeof(double)))) return rc;
  if (cs && (rc = out.reserve((size_t)n * 2 * sizeof(double)))) return rc;
  HIPC(hipMemset(res.p, 0, 2 * sizeof(unsigned long long)));
  if (n) HIPC(hipMemcpy(in.p, phi, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
  const int64_t total = n + n_draws;
  if (total > 0) {
    const unsigned blocks = (unsigned)std::min<int64_t>(1024, (total + 255) / 256);
    unsigned long long* bad = res.as<unsigned long long>();
    hipLaunchKernelGGL(rtxd::k_cos_sin_forms, dim3(blocks), dim3(256), 0, nullptr, in.as<double>(), n, seed, n_draws,
                       bad, (double*)(bad + 1), cs ? out.as<double>() : nullptr);
    HIPC(hipGetLastError());
  }
  unsigned long long h[2];
  HIPC(hipMemcpy(h, res.p, sizeof(h), hipMemcpyDeviceToHost));
  if (cs && n) HIPC(hipMemcpy(cs, out.p, (size_t)n * 2 * sizeof(double), hipMemcpyDeviceToHost));
  *mismatches = (int64_t)h[0];
  if (first_bad) std::memcpy(first_bad, &h[1], sizeof(double));
  return RTX_OK;
}

// Test hook (not in rtx.h; tests/test_gpu_visit_order.py): the speculative walk's order.  n rays
// (6 doubles each), `lanes` of them per wave; seq / tseq: 64 entries per ray, the node visited
// (>= 0) or ~primitive tested (< 0) and the closest distance after it; len: each ray's entries,
// those past 64 counted but not kept; fray: 15 words per ray, the slab constants the walk used.
// The scene must have a fast tree of fewer than 2^16 nodes (the speculative walk's condition).
extern "C" int rtx_internal_visit_order(rtx_scene* sc, const double* rays, int64_t n, int lanes, double tmin,
                                        int32_t* seq, double* tseq, int32_t* len, uint32_t* fray) {
  if (!sc || n <= 0 || n > (1 << 20) || !rays || lanes < 1 || lanes > 64 || !seq || !tseq || !len || !fray)
    return fail(RTX_ERR_INVALID, "bad argument");
  if (!sc->fast_ok || sc->n_f4 == 0 || sc->n_f4 >= 65536 || (sc->stack_fast != 32 && sc->stack_fast != 64))
    return fail(RTX_ERR_INVALID, "the scene has no fast tree the speculative walk runs on");
  HIPC(hipSetDevice(sc->device));
  DevBuf in, oseq, ot, olen, ofr;
  int rc;
  const size_t un = (size_t)n;
  if ((rc = in.reserve(un * 6 * sizeof(double)))) return rc;
  if ((rc = oseq.reserve(un * rtxd::kSeqCap * sizeof(int32_t)))) return rc;
  if ((rc = ot.reserve(un * rtxd::kSeqCap * sizeof(double)))) return rc;
  if ((rc = olen.reserve(un * sizeof(int32_t)))) return rc;
  if ((rc = ofr.reserve(un * 15 * sizeof(uint32_t)))) return rc;
  HIPC(hipMemcpy(in.p, rays, un * 6 * sizeof(double), hipMemcpyHostToDevice));
  HIPC(hipMemset(oseq.p, 0, un * rtxd::kSeqCap * sizeof(int32_t)));
  HIPC(hipMemset(ot.p, 0, un * rtxd::kSeqCap * sizeof(double)));
  HIPC(hipMemset(olen.p, 0, un * sizeof(int32_t)));
  HIPC(hipStreamSynchronize(sc->stream));
  const unsigned blocks = (unsigned)((n + lanes - 1) / lanes);
  if (sc->stack_fast == 32)
    hipLaunchKernelGGL(rtxd::k_visit_order<32>, dim3(blocks), dim3(64), 0, nullptr, sc->S, in.as<double>(), n, lanes, tmin,
                       oseq.as<int32_t>(), ot.as<double>(), olen.as<int32_t>(), ofr.as<uint32_t>());
  else
    hipLaunchKernelGGL(rtxd::k_visit_order<64>, dim3(blocks), dim3(64), 0, nullptr, sc->S, in.as<double>(), n, lanes, tmin,
                       oseq.as<int32_t>(), ot.as<double>(), olen.as<int32_t>(), ofr.as<uint32_t>());
  HIPC(hipGetLastError());
  HIPC(hipMemcpy(seq, oseq.p, un * rtxd::kSeqCap * sizeof(int32_t), hipMemcpyDeviceToHost));
  HIPC(hipMemcpy(tseq, ot.p, un * rtxd::kSeqCap * sizeof(double), hipMemcpyDeviceToHost));
  HIPC(hipMemcpy(len, olen.p, un * sizeof(int32_t), hipMemcpyDeviceToHost));
  HIPC(hipMemcpy(fray, ofr.p, un * 15 * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return RTX_OK;
}
