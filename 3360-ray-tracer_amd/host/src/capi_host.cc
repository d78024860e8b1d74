// capi_host.cc — the host-side part of include/rtx.h: scene assembly helpers and
// cameras.json presets, implemented with the C++ host API (rt::scene / rt::geom).
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <string>

#include "rt/image.h"
#include "rt/scene.h"
#include "rtx.h"
#include "rtx_bounds.h"

struct rtx_host_scene {
  std::shared_ptr<rt::scene::Scene> root;
  rt::scene::FlatScene flat;
  bool bvh = false;
};

// rtx_last_error() is defined with the device part; host helpers report through it too.
extern "C" void rtx_internal_set_error(const char* msg);

namespace {
int host_fail(int code, const std::string& m) {
  rtx_internal_set_error(m.c_str());
  return code;
}
}  // namespace

namespace {
int finish(std::shared_ptr<rt::scene::Scene> root, rtx_host_scene** out) {
  auto* s = new rtx_host_scene;
  s->root = std::move(root);
  s->flat = rt::scene::Flatten(*s->root);
  s->bvh = !s->flat.nodes.empty() || (s->root->Objects().size() == 1 &&
                                       dynamic_cast<const rt::geom::Bvh*>(s->root->Objects()[0].get()));
  *out = s;
  return RTX_OK;
}
}  // namespace

extern "C" {

int rtx_host_scene_load(const char* path, const char* asset_dir, rtx_host_scene** out) {
  if (!path || !out) return host_fail(RTX_ERR_INVALID, "NULL argument");
  try {
    return finish(rt::scene::LoadSceneFile(path, asset_dir ? asset_dir : ""), out);
  } catch (const std::exception& e) {
    return host_fail(RTX_ERR_IO, e.what());
  }
}

int rtx_host_scene_recipe(const char* name, uint32_t seed, const char* asset_dir, rtx_host_scene** out) {
  if (!name || !out) return host_fail(RTX_ERR_INVALID, "NULL argument");
  try {
    return finish(rt::scene::BuildRecipe(name, seed, asset_dir ? asset_dir : ""), out);
  } catch (const std::exception& e) {
    return host_fail(RTX_ERR_IO, e.what());
  }
}

int rtx_host_scene_write(const rtx_host_scene* s, const char* path) {
  if (!s || !path) return host_fail(RTX_ERR_INVALID, "NULL argument");
  try {
    rt::scene::WriteSceneFile(s->flat, s->bvh, path);
  } catch (const std::exception& e) {
    return host_fail(RTX_ERR_IO, e.what());
  }
  return RTX_OK;
}

int rtx_host_scene_desc(const rtx_host_scene* s, rtx_scene_desc* out) {
  if (!s || !out) return host_fail(RTX_ERR_INVALID, "NULL argument");
  *out = s->flat.desc();
  return RTX_OK;
}

int rtx_host_scene_prim_indices(const rtx_host_scene* s, int32_t* out, int64_t n) {
  if (!s || !out) return host_fail(RTX_ERR_INVALID, "NULL argument");
  if (n != (int64_t)s->flat.prim_indices.size()) return host_fail(RTX_ERR_INVALID, "n != number of prim indices");
  std::memcpy(out, s->flat.prim_indices.data(), n * sizeof(int32_t));
  return RTX_OK;
}

// Hittable::BoundingBox of each primitive record, as the host classes compute it
// (sphere.h, triangle.h:18-38, rect.h:42-45,87-89,132-134): the SAH builder's input.
int rtx_prim_bounds(const rtx_prim* prims, int64_t n, double* out) {
  if ((!prims || !out) && n > 0) return host_fail(RTX_ERR_INVALID, "NULL argument");
  for (int64_t i = 0; i < n; i++) {
    const rtx_prim& p = prims[i];
    if (p.kind < RTX_PRIM_SPHERE || p.kind > RTX_PRIM_YZ_RECT) return host_fail(RTX_ERR_INVALID, "unknown primitive kind");
    rtxb::ref_bounds(p.kind, p.g, out + 6 * i);  // rtx_bounds.h: the arithmetic the update kernel runs too
  }
  return RTX_OK;
}

// Bottom-up refit of reference-layout nodes over new primitive boxes, topology unchanged: what
// rtx_scene_update_* does on the device (rtx_refit.hip), with the same routines (rtx_bounds.h).
int rtx_bvh_refit_host(rtx_bvh_node* nodes, int64_t n_nodes, const double* bounds, int64_t n) {
  if (n_nodes < 0 || n < 0) return host_fail(RTX_ERR_INVALID, "negative count");
  if ((!nodes && n_nodes > 0) || (!bounds && n > 0)) return host_fail(RTX_ERR_INVALID, "NULL argument");
  for (int64_t i = 0; i < n_nodes; i++) {
    const rtx_bvh_node& q = nodes[i];
    if (q.is_leaf) {
      if ((int64_t)q.left_first + q.right_count > n) return host_fail(RTX_ERR_INVALID, "leaf range out of bounds");
    } else if (q.left_first >= n_nodes || q.right_count >= n_nodes || q.left_first <= i || q.right_count <= i) {
      return host_fail(RTX_ERR_INVALID, "child index out of bounds (nodes must be pre-order)");
    }
  }
  for (int64_t i = n_nodes - 1; i >= 0; i--) {  // children come after their parent
    rtx_bvh_node& q = nodes[i];
    if (q.is_leaf) rtxb::refit_leaf(q, bounds);
    else rtxb::refit_inner(q, nodes[q.left_first], nodes[q.right_count]);
  }
  return RTX_OK;
}

int rtx_bvh_build_host(const double* bounds, int64_t n, rtx_bvh_node* out_nodes, int64_t* out_n_nodes,
                       uint32_t* out_prim_indices) {
  if ((!bounds && n > 0) || !out_nodes || !out_n_nodes || !out_prim_indices)
    return host_fail(RTX_ERR_INVALID, "NULL argument");
  if (n < 0 || n > 0x3FFFFFFF) return host_fail(RTX_ERR_INVALID, "primitive count out of range");
  if (const int64_t bad = rtxb::first_nonfinite_box(bounds, n); bad >= 0)
    return host_fail(RTX_ERR_INVALID, "rtx_bvh_build_host: box " + std::to_string(bad) + " has a NaN or infinite bound");
  std::vector<rt::geom::Aabb> b(n);
  for (int64_t i = 0; i < n; i++) {
    const double* q = bounds + 6 * i;
    b[i] = rt::geom::Aabb(rt::core::Interval(q[0], q[3]), rt::core::Interval(q[1], q[4]),
                          rt::core::Interval(q[2], q[5]));
  }
  std::vector<int> idx;
  std::vector<rt::geom::BvhNodeGPU> nodes;
  rt::geom::BuildSah(b, idx, nodes);
  for (size_t i = 0; i < nodes.size(); i++) {
    rtx_bvh_node& o = out_nodes[i];
    const rt::geom::Aabb& a = nodes[i].bbox;
    o.lo[0] = a.x.min_, o.lo[1] = a.y.min_, o.lo[2] = a.z.min_;
    o.hi[0] = a.x.max_, o.hi[1] = a.y.max_, o.hi[2] = a.z.max_;
    o.left_first = nodes[i].left_pIdx, o.right_count = nodes[i].right_pCnt, o.is_leaf = nodes[i].isLeaf, o.pad_ = 0;
  }
  for (int64_t i = 0; i < n; i++) out_prim_indices[i] = (uint32_t)idx[i];
  *out_n_nodes = (int64_t)nodes.size();
  return RTX_OK;
}

int rtx_host_scene_destroy(rtx_host_scene* s) {
  delete s;
  return RTX_OK;
}

int rtx_camera_config_load(const char* json_path, const char* preset, rtx_camera_config* out) {
  if (!json_path || !preset || !out) return host_fail(RTX_ERR_INVALID, "NULL argument");
  try {
    auto cams = rt::scene::loadCameras(json_path);
    auto it = cams.find(preset);
    if (it == cams.end()) return host_fail(RTX_ERR_INVALID, std::string("camera preset not found: ") + preset);
    const auto& c = it->second;
    std::memset(out, 0, sizeof *out);
    out->aspect_ratio = c.aspect_ratio, out->image_width = c.image_width;
    out->samples_per_pixel = c.samples_per_pixel, out->max_depth = c.max_depth, out->vfov = c.vfov;
    for (int i = 0; i < 3; i++) out->lookfrom[i] = c.lookfrom[i], out->lookat[i] = c.lookat[i], out->vup[i] = c.vup[i];
    out->defocus_angle = c.defocus_angle, out->focus_dist = c.focus_dist;
  } catch (const std::exception& e) {
    return host_fail(RTX_ERR_IO, e.what());
  }
  return RTX_OK;
}

}  // extern "C"

// Image::Load (scene/image.cc:16-73) as a C entry point: the texels the renderer samples, or
// (linear8) the 8-bit decode before stb's gamma step.  texels == NULL: size query.
int rtx_image_load(const char* path, int32_t linear8, int32_t* width, int32_t* height, uint8_t* texels,
                   size_t cap) {
  if (!path || !width || !height) return host_fail(RTX_ERR_INVALID, "NULL argument");
  int w = 0, h = 0;
  std::vector<uint8_t> px;
  std::string err;
  if (!rt::scene::LoadTexels(path, w, h, px, err, linear8 != 0)) return host_fail(RTX_ERR_IO, err);
  *width = w, *height = h;
  if (texels) {
    if (cap < px.size()) return host_fail(RTX_ERR_INVALID, "texel buffer too small");
    std::memcpy(texels, px.data(), px.size());
  }
  return RTX_OK;
}

// A probe's SH coefficients (rtx_probe_sh's layout) at n directions: the reconstruction, or the
// cosine-convolved value over pi (include/rtx.h).  The basis in rtx.h's order and operations, as
// the device's sh_basis (csrc/rtx_probe.h) forms it; this unit is built with -ffp-contract=off.
int rtx_sh_eval(const double* sh, const double* dirs, size_t n, int32_t cosine, double* out_rgb) {
  if (!sh || ((!dirs || !out_rgb) && n > 0)) return host_fail(RTX_ERR_INVALID, "NULL buffer");
  if (cosine != 0 && cosine != 1) return host_fail(RTX_ERR_INVALID, "sh eval: cosine must be 0 or 1");
  for (size_t i = 0; i < n; i++) {
    const double x = dirs[3 * i], y = dirs[3 * i + 1], z = dirs[3 * i + 2];
    double Y[RTX_SH_COEFFS];
    Y[0] = RTX_SH_K0;
    Y[1] = RTX_SH_K1 * y;
    Y[2] = RTX_SH_K1 * z;
    Y[3] = RTX_SH_K1 * x;
    Y[4] = RTX_SH_K4 * (x * y);
    Y[5] = RTX_SH_K4 * (y * z);
    Y[6] = RTX_SH_K6 * (3.0 * (z * z) - 1.0);
    Y[7] = RTX_SH_K4 * (x * z);
    Y[8] = RTX_SH_K8 * (x * x - y * y);
    for (int c = 0; c < 3; c++) {
      const double* s = sh + c;  // coefficient j of this channel: s[3 * j]
      if (cosine) {
        const double b1 = (s[3] * Y[1] + s[6] * Y[2]) + s[9] * Y[3];
        const double b2 = (((s[12] * Y[4] + s[15] * Y[5]) + s[18] * Y[6]) + s[21] * Y[7]) + s[24] * Y[8];
        out_rgb[3 * i + c] = (s[0] * Y[0] + (2.0 / 3.0) * b1) + 0.25 * b2;
      } else {
        double v = s[0] * Y[0];
        for (int j = 1; j < RTX_SH_COEFFS; j++) v = v + s[3 * j] * Y[j];
        out_rgb[3 * i + c] = v;
      }
    }
  }
  return RTX_OK;
}
