// PARK instantiations of the persistent kernel (k_persistent<STACK, true, COUNT, SCATTER,
// PARK = 1 or 2>), compiled apart from rtx_capi.hip so this translation unit can have its own
// per-TU choices (RTX_PARK_TU: see the top of rtx_device.h) and scheduler options (Makefile
// PARKFLAGS).  k_persistent refuses to be instantiated with PARK > 0 anywhere else.
#define RTX_PARK_TU 1
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "rtx.h"
#include "rtx_host.h"  // (the test hook at the end: error reporting, device buffers)
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
  struct Owned : DevBuf {
    ~Owned() { release(); }
  } res, in, out;
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
