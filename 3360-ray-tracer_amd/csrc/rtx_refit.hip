// rtx_refit.hip — the kernels of in-place scene updates (rtx_refit.h).  gfx950.
#include "rtx_refit.h"

#include "rtx_bounds.h"
#include "rtx_device.h"

namespace rtxrefit {
namespace {

constexpr int kBlock = 256;

// One thread per updated primitive: the device record (triangles in edge form), the triangle's
// unit normal and the primitive's two boxes.
__global__ __launch_bounds__(kBlock) void k_update_prims(UpdateArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.count) return;
  const int64_t p = a.first + i;
  rtx_prim& dst = a.prims[p];
  int32_t kind, material;
  double g[9];
  if (a.src) {
    kind = a.src[i].kind, material = a.src[i].material;
    for (int k = 0; k < 9; k++) g[k] = a.src[i].g[k];
  } else {
    kind = dst.kind, material = dst.material;
    for (int k = 0; k < 9; k++) g[k] = a.src_g[9 * i + k];
  }
  if (a.ref_box) rtxb::ref_bounds(kind, g, a.ref_box + 6 * p);
  if (a.fast_box) rtxb::fast_box(kind, g, a.fast_box + 6 * p);
  if (kind == RTX_PRIM_TRIANGLE) {
    if (a.tri_n) {
      double n[3];
      rtxb::tri_unit_normal(g, n);
      for (int k = 0; k < 3; k++) a.tri_n[4 * p + k] = n[k];
    }
    for (int k = 0; k < 3; k++) g[3 + k] = g[3 + k] - g[k], g[6 + k] = g[6 + k] - g[k];
  }
  dst.kind = kind, dst.material = material;
  for (int k = 0; k < 9; k++) dst.g[k] = g[k];
}

__global__ __launch_bounds__(kBlock) void k_refit_nodes(rtx_bvh_node* nodes, const double* ref_box,
                                                        const uint32_t* idx, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  rtx_bvh_node& me = nodes[idx[i]];
  if (me.is_leaf) rtxb::refit_leaf(me, ref_box);
  else rtxb::refit_inner(me, nodes[me.left_first], nodes[me.right_count]);
}

// One thread per slot (four per node).
__global__ __launch_bounds__(kBlock) void k_refit_f4(rtxd::F4Node* nodes, const float* fast_box, const uint32_t* idx,
                                                     int64_t n) {
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= 4 * n) return;
  rtxd::F4Node& me = nodes[idx[t >> 2]];
  const int c = (int)(t & 3);
  const int32_t child = me.child[c];
  float b[6];
  if (child >= 0) {
    const rtxd::F4Node& ch = nodes[child];
    b[0] = ch.lox[0], b[1] = ch.loy[0], b[2] = ch.loz[0], b[3] = ch.hix[0], b[4] = ch.hiy[0], b[5] = ch.hiz[0];
    for (int k = 1; k < 4; k++) {
      b[0] = rtxb::fmin32(b[0], ch.lox[k]), b[1] = rtxb::fmin32(b[1], ch.loy[k]), b[2] = rtxb::fmin32(b[2], ch.loz[k]);
      b[3] = rtxb::fmax32(b[3], ch.hix[k]), b[4] = rtxb::fmax32(b[4], ch.hiy[k]), b[5] = rtxb::fmax32(b[5], ch.hiz[k]);
    }
  } else if ((me.counts[c >> 1] >> (16 * (c & 1))) & 0xFFFFu) {  // a leaf slot: ~child is its primitive
    const float* f = fast_box + 6 * (size_t)(uint32_t)~child;
    for (int k = 0; k < 6; k++) b[k] = f[k];
  } else {
    return;  // empty: stays inverted
  }
  me.lox[c] = b[0], me.loy[c] = b[1], me.loz[c] = b[2];
  me.hix[c] = b[3], me.hiy[c] = b[4], me.hiz[c] = b[5];
}

unsigned blocks_of(int64_t threads) { return (unsigned)((threads + kBlock - 1) / kBlock); }

}  // namespace

hipError_t update_prims(const UpdateArgs& a, hipStream_t s) {
  if (a.count <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_update_prims, dim3(blocks_of(a.count)), dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

hipError_t refit_nodes(rtx_bvh_node* nodes, const double* ref_box, const uint32_t* idx, int64_t n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_refit_nodes, dim3(blocks_of(n)), dim3(kBlock), 0, s, nodes, ref_box, idx, n);
  return hipGetLastError();
}

hipError_t refit_f4(rtxd::F4Node* nodes, const float* fast_box, const uint32_t* idx, int64_t n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_refit_f4, dim3(blocks_of(4 * n)), dim3(kBlock), 0, s, nodes, fast_box, idx, n);
  return hipGetLastError();
}

}  // namespace rtxrefit
