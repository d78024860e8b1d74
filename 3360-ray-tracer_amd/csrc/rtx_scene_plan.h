// rtx_scene_plan.h — everything rtx_scene_create decides and tabulates on the host before it
// touches a device: the description checks, the fast tree and its stacks, the tables it uploads
// and the flags of the device scene.  Plain C++ (rtx_scene_plan.cc), no HIP header: the unit
// builds into a stand-alone program too (tools/plan_check.cc).  Errors are reported the way
// bad_nodes does: a message, or nullptr; the C ABI's units turn it into fail() (rtx_host.h).
#ifndef RTX_SCENE_PLAN_H_
#define RTX_SCENE_PLAN_H_

#include <stdint.h>

#include <vector>

#include "rtx.h"
#include "rtx_f4node.h"

namespace rtxplan {

// The reference-layout nodes' indices, checked so that neither the host routines nor the
// kernels read out of bounds: nullptr, or what is wrong.
const char* bad_nodes(const rtx_scene_desc* d);

// What rtx_scene_create decides on the host about a scene's traversal, and the fast tree it
// uploads: one routine, shared with the test hook rtx_internal_fast_tree, so the hook reports
// the product's own tree.  No HIP call.
struct FastPlan {
  int depth = 0;                    // levels of the reference-layout tree (bvh_depth)
  int stack_parity = 32;            // pick_stack(depth), -1: deeper than the parity walk's largest stack
  int stack_fast = 32, fast_need = 0;
  bool fast_ok = false;             // RTX_PREC_FAST has a tree and a stack for it
  std::vector<rtxd::F4Node> f4;     // built whenever the root is internal, also when fast_ok is false
  int32_t global[2] = {0, 0};
  int n_global = 0;                 // globals the tree was built without (the scene uses them only with fast_ok)
  int tree_kind = -1;               // the one kind of the tree's primitives with fast_ok, else -1
};
void plan_fast_tree(const rtx_scene_desc* d, FastPlan& p);

// A checked description's host side, whole: plan_scene fills it, rtx_scene_create uploads from it
// and keeps what an update needs.  The tables live as long as the plan, so the uploads need no
// synchronisation of their own.
struct ScenePlan {
  FastPlan fast;
  std::vector<double> tri_n;      // (x, y, z, 0) per primitive, a triangle's unit normal; empty: no triangles
  std::vector<rtx_prim> prims;    // the device table: triangles as A, B - A, C - A; a plain global sphere's r * r in g[4]
  std::vector<rtx_material> mats; // the device table: solid colours and the dielectric's 1 / ri, r0 resolved
  // scenes with nodes (rtx_scene_update_*): each primitive's reference box (6 doubles) and fast box
  // (6 floats), both trees' node indices grouped by height and where each height starts
  std::vector<double> ref_box;
  std::vector<float> fast_box;
  std::vector<uint32_t> node_order, f4_order;
  std::vector<int64_t> node_lvl, f4_lvl;
  std::vector<int8_t> kinds;      // each primitive's kind
  std::vector<uint32_t> emit_idx; // the primitives whose material is a DiffuseLight, in order
  // DScene's fields that are no pointers (rtx_device.h), under their names there
  int64_t n_prims = 0;
  int32_t use_bvh = 0, froot_leaf = 0, froot_count = 0, has_tris = 0, tree_kind = -1;
  int32_t all_lambertian = 0, no_textures = 1;
  int32_t n_global = 0;           // with bit 2 (kGlobalSpheres) when every global is a plain sphere
  int32_t global[2] = {0, 0};
};
constexpr int32_t kPlainGlobalSpheres = 4;  // rtxd::kGlobalSpheres of rtx_device.h (rtx_capi.hip asserts that the two agree)

// The checks of a description in rtx_scene_create's order, then its whole plan: nullptr, or why
// the description is refused (p is then unspecified).
const char* plan_scene(const rtx_scene_desc* d, ScenePlan& p);

}  // namespace rtxplan

#endif  // RTX_SCENE_PLAN_H_
