// rtx_bounds.h — the box arithmetic of a primitive and of a tree node, written once for the host
// builders (rtx_prim_bounds, build_fast4, rtx_bvh_refit_host) and the refit kernels
// (rtx_refit.hip).  Host and device run the same IEEE operations in the same order (the build
// uses -ffp-contract=off), so a device refit reproduces the host's bytes.  min / max are the
// comparisons of std::min / std::max (first argument kept on equality).
#ifndef RTX_BOUNDS_H_
#define RTX_BOUNDS_H_

#include <math.h>
#include <stdint.h>

#include "rtx.h"

#if defined(__HIPCC__)
#define RTX_HD __host__ __device__
#else
#define RTX_HD
#endif

namespace rtxb {

RTX_HD inline double dmin(double a, double b) { return b < a ? b : a; }
RTX_HD inline double dmax(double a, double b) { return a < b ? b : a; }
RTX_HD inline float fmin32(float a, float b) { return b < a ? b : a; }
RTX_HD inline float fmax32(float a, float b) { return a < b ? b : a; }

// Outward rounding to f32 (monotone: the rounded union is the union of the rounded boxes).
RTX_HD inline float round_down(double x) {
  float f = (float)x;
  if ((double)f > x) f = nextafterf(f, -INFINITY);
  return f;
}
RTX_HD inline float round_up(double x) {
  float f = (float)x;
  if ((double)f < x) f = nextafterf(f, INFINITY);
  return f;
}

// Aabb(Point3 a, Point3 b) of the host classes, one axis: the interval in order.
RTX_HD inline void ordered(double a, double b, double& lo, double& hi) {
  if (a <= b) lo = a, hi = b;
  else lo = b, hi = a;
}

// Hittable::BoundingBox of a primitive record as the host classes compute it (sphere.h,
// triangle.h:18-38, rect.h:42-45,87-89,132-134): out = lo xyz, hi xyz.  The kind must be valid;
// a triangle's g is A, B, C (not the device table's edge form).
RTX_HD inline void ref_bounds(int32_t kind, const double* g, double* out) {
  if (kind == RTX_PRIM_SPHERE) {
    for (int a = 0; a < 3; a++) ordered(g[a] + g[3], g[a] - g[3], out[a], out[3 + a]);
    return;
  }
  if (kind == RTX_PRIM_TRIANGLE) {
    const double eps = 1e-6f;
    for (int a = 0; a < 3; a++) {
      double mn = fmin(g[a], fmin(g[3 + a], g[6 + a]));
      double mx = fmax(g[a], fmax(g[3 + a], g[6 + a]));
      mn += -eps;
      mx += eps;
      ordered(mn, mx, out[a], out[3 + a]);
    }
    return;
  }
  int ax, a0, a1;  // rect.h: XY (z = k), XZ (y = k), YZ (x = k)
  if (kind == RTX_PRIM_XY_RECT) ax = 2, a0 = 0, a1 = 1;
  else if (kind == RTX_PRIM_XZ_RECT) ax = 1, a0 = 0, a1 = 2;
  else ax = 0, a0 = 1, a1 = 2;
  ordered(g[0], g[1], out[a0], out[3 + a0]);
  ordered(g[2], g[3], out[a1], out[3 + a1]);
  ordered(g[4] - 0.0001, g[4] + 0.0001, out[ax], out[3 + ax]);
}

// SAH bin (of 16) of a centroid coordinate c in a node whose centroids start at mn, inv =
// 1 / extent (bvh.h:230-236): trunc((c - mn) * inv * 16), clamped to [0, 15].  An extent below
// 2^-1024 makes inv +inf and the product +inf (c > mn) or NaN (c == mn); converting those to
// int is undefined in C++ and differs by machine (x86 cvttsd2si gives INT_MIN, gfx950
// saturates +inf to INT_MAX).  The rule here is what the reference's x86 build does: a product
// that is NaN or not below 2^31 goes to bin 0.  Every other value converts as the bare cast.
RTX_HD inline int sah_bin(double c, double mn, double inv) {
  const double v = (c - mn) * inv * 16;
  if (!(v < 2147483648.0) || v < 0.0) return 0;
  const int b = (int)v;
  return b > 15 ? 15 : b;
}

// Index of the first of n boxes (6 doubles each) with a NaN or infinite bound, -1 if all are
// finite.  The raw-box builders refuse such input: a NaN bound or centroid compares equal to
// nothing, which the device build's "first position holding the extreme" search relies on.
inline int64_t first_nonfinite_box(const double* bounds, int64_t n) {
  for (int64_t i = 0; i < n; i++)
    for (int c = 0; c < 6; c++)
      if (!isfinite(bounds[6 * i + c])) return i;
  return -1;
}

// Conservative f64 box of one primitive (fast-path leaf splitting).  Spheres: centre +-
// |r|; rects: the rectangle on its plane; triangles: the vertex box padded by 2^-19 of its
// largest extent, which covers the points the reference's float-rounded barycentric test
// accepts just outside the exact triangle (u, v, u + v within 2^-23 of the edges).
RTX_HD inline void prim_box(int32_t kind, const double* g, double lo[3], double hi[3]) {
  if (kind == RTX_PRIM_SPHERE) {
    const double r = fabs(g[3]);
    for (int a = 0; a < 3; a++) lo[a] = g[a] - r, hi[a] = g[a] + r;
    return;
  }
  if (kind == RTX_PRIM_TRIANGLE) {
    double ext = 0;
    for (int a = 0; a < 3; a++) {
      lo[a] = dmin(g[a], dmin(g[3 + a], g[6 + a]));
      hi[a] = dmax(g[a], dmax(g[3 + a], g[6 + a]));
      ext = dmax(ext, hi[a] - lo[a]);
    }
    const double pad = ldexp(ext, -19);
    for (int a = 0; a < 3; a++) lo[a] -= pad, hi[a] += pad;
    return;
  }
  int ax, a0, a1;
  if (kind == RTX_PRIM_XY_RECT) ax = 2, a0 = 0, a1 = 1;
  else if (kind == RTX_PRIM_XZ_RECT) ax = 1, a0 = 0, a1 = 2;
  else ax = 0, a0 = 1, a1 = 2;
  lo[a0] = dmin(g[0], g[1]), hi[a0] = dmax(g[0], g[1]);
  lo[a1] = dmin(g[2], g[3]), hi[a1] = dmax(g[2], g[3]);
  lo[ax] = hi[ax] = g[4];
}

// prim_box rounded outward: the box a one-primitive slot of the fast tree holds (lo xyz, hi xyz).
RTX_HD inline void fast_box(int32_t kind, const double* g, float* out) {
  double lo[3], hi[3];
  prim_box(kind, g, lo, hi);
  for (int a = 0; a < 3; a++) out[a] = round_down(lo[a]), out[3 + a] = round_up(hi[a]);
}

// Triangle::Hit's Normalize(Cross(edge1, edge2)) (triangle.h:80-82) of A, B, C in g: cross,
// length squared, sqrt, 1 / l, products; (0, 0, 0) for a zero length.
RTX_HD inline void tri_unit_normal(const double* g, double n[3]) {
  double e1[3], e2[3];
  for (int a = 0; a < 3; a++) e1[a] = g[3 + a] - g[a], e2[a] = g[6 + a] - g[a];
  const double c[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
  const double l = sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
  n[0] = n[1] = n[2] = 0.0;
  if (l == 0.0) return;
  const double inv = 1.0 / l;
  for (int a = 0; a < 3; a++) n[a] = inv * c[a];
}

// Refit of a reference-layout node: a leaf takes the union of its primitives' boxes (bounds:
// 6 doubles per primitive, leaf order; an empty leaf keeps its box), an internal node the union
// of its two children.
RTX_HD inline void refit_leaf(rtx_bvh_node& n, const double* bounds) {
  if (n.right_count == 0) return;
  const double* b = bounds + 6 * (size_t)n.left_first;
  double lo[3] = {b[0], b[1], b[2]}, hi[3] = {b[3], b[4], b[5]};
  for (uint32_t i = 1; i < n.right_count; i++) {
    b += 6;
    for (int a = 0; a < 3; a++) lo[a] = dmin(lo[a], b[a]), hi[a] = dmax(hi[a], b[3 + a]);
  }
  for (int a = 0; a < 3; a++) n.lo[a] = lo[a], n.hi[a] = hi[a];
}
RTX_HD inline void refit_inner(rtx_bvh_node& n, const rtx_bvh_node& l, const rtx_bvh_node& r) {
  for (int a = 0; a < 3; a++) n.lo[a] = dmin(l.lo[a], r.lo[a]), n.hi[a] = dmax(l.hi[a], r.hi[a]);
}

}  // namespace rtxb

#endif  // RTX_BOUNDS_H_
