// rtx_refit.h — in-place scene updates (rtx_scene_update_*): rewrite primitive
// records and refit both trees bottom-up over their unchanged topology, one launch per height so
// that a node reads its children's boxes across a kernel boundary.  The callers (rtx_capi.hip)
// validate every range and index on the host; the kernels trust them.
#ifndef RTX_REFIT_H_
#define RTX_REFIT_H_

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "rtx.h"
#include "rtx_f4node.h"

namespace rtxrefit {

// Primitives [first, first + count) of the scene's tables.  Exactly one source is set: src
// (count whole records: kind, material, geometry) or src_g (count x 9 doubles, the records keep
// their kind and material).  Triangles arrive as A, B, C and are stored as A, B - A, C - A.
struct UpdateArgs {
  rtx_prim* prims;
  double* tri_n;     // 4 doubles per primitive, or nullptr (a scene without triangles)
  double* ref_box;   // 6 doubles per primitive (rtx_prim_bounds), or nullptr (a flat list)
  float* fast_box;   // 6 floats per primitive (prim_box rounded outward), or nullptr
  int64_t first, count;
  const rtx_prim* src;
  const double* src_g;
};
hipError_t update_prims(const UpdateArgs& a, hipStream_t s);

// One height of the reference-layout tree: idx[0..n) are its nodes.  Leaves union their
// primitives' ref_box, internal nodes their two children (refit at lower heights).
hipError_t refit_nodes(rtx_bvh_node* nodes, const double* ref_box, const uint32_t* idx, int64_t n, hipStream_t s);
// One height of the fast tree: every slot of idx[0..n) that holds a primitive takes its
// fast_box, every slot that holds a child node the f32 union of the child's four slots; empty
// slots keep their inverted box.
hipError_t refit_f4(rtxd::F4Node* nodes, const float* fast_box, const uint32_t* idx, int64_t n, hipStream_t s);

}  // namespace rtxrefit

#endif  // RTX_REFIT_H_
