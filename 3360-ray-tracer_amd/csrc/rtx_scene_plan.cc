// rtx_scene_plan.cc — the host side of rtx_scene_create (rtx_scene_plan.h): the description
// checks, the fast path's tree (global primitives, binned SAH, BVH4 collapse), the traversal
// stacks, and every table and flag the device scene is made of.  Plain C++ with the host flags
// (-ffp-contract=off): no HIP header, no device.
#include "rtx_scene_plan.h"

#include <algorithm>
#include <cmath>

#include "rtx_bounds.h"

using rtxb::round_down;
using rtxb::round_up;
using rtxd::F4Node;

namespace {

// Tree depth of the reference-layout BVH (pre-order, left = idx+1).
int bvh_depth(const rtx_bvh_node* n, int64_t count) {
  if (count == 0) return 0;
  std::vector<int> d(count, 0);
  int m = 1;
  for (int64_t i = 0; i < count; i++) {
    m = std::max(m, d[i] + 1);
    if (!n[i].is_leaf) {
      d[n[i].left_first] = d[i] + 1;
      d[n[i].right_count] = d[i] + 1;
    }
  }
  return m;
}

// Conservative f64 box of one primitive (fast-path leaf splitting): rtx_bounds.h, shared with
// the refit kernels.
void prim_box(const rtx_prim& p, double lo[3], double hi[3]) { rtxb::prim_box(p.kind, p.g, lo, hi); }

// BVH4 fast layout: the binary tree collapsed top-down.  Each F4Node starts from the binary
// node's two children and repeatedly opens the slot with the largest surface area until it
// holds four slots or nothing fits: an internal binary node opens into its two children, a
// leaf of 2-4 primitives into its primitives.  Every leaf slot of the result holds exactly
// ONE primitive with its own conservative box (prim_box), so the f32 slab test culls
// primitives before their f64 test and the kernel needs no per-slot counts: a leaf of
// several primitives left in a slot becomes a child F4Node of one-primitive slots (and a leaf
// of more than four, a small tree of them).  Empty slots carry an inverted box (lo = +inf,
// hi = -inf) that no ray enters.  Every slot keeps a box that contains all hits its
// primitives can report, rounded outward, so the candidate set is unchanged.
// Returns the exact worst-case traversal stack depth (trace_fast4 pushes at most
// `internal slots - 1` entries per visited node).
int build_fast4(const rtx_bvh_node* n, const rtx_prim* prims, std::vector<F4Node>& out) {
  out.clear();
  struct Slot {
    int kind;  // 0 binary node, 1 one primitive, 2 a primitive range emitted as a child node
    uint32_t id, count;  // kind 0: node; kind 1: primitive; kind 2: first primitive, count
    double lo[3], hi[3];
  };
  auto node_slot = [&](uint32_t b) {
    Slot s{0, b, 0, {}, {}};
    for (int a = 0; a < 3; a++) s.lo[a] = n[b].lo[a], s.hi[a] = n[b].hi[a];
    if (n[b].is_leaf && n[b].right_count >= 2) s.kind = 2, s.id = n[b].left_first, s.count = n[b].right_count;
    return s;
  };
  auto prim_slot = [&](uint32_t id) {
    Slot s{1, id, 1, {}, {}};
    prim_box(prims[id], s.lo, s.hi);
    return s;
  };
  auto area = [](const Slot& s) {
    const double dx = s.hi[0] - s.lo[0], dy = s.hi[1] - s.lo[1], dz = s.hi[2] - s.lo[2];
    return dx * dy + dy * dz + dz * dx;
  };
  // the slots of the child node a kind-2 range becomes: its primitives (<= 4), else four
  // contiguous sub-ranges with the union of their primitive boxes
  auto range_slots = [&](uint32_t first, uint32_t count) {
    std::vector<Slot> r;
    if (count <= 4) {
      for (uint32_t q = 0; q < count; q++) r.push_back(prim_slot(first + q));
      return r;
    }
    const uint32_t per = (count + 3) / 4;
    for (uint32_t g = first; g < first + count; g += per) {
      const uint32_t k = std::min(per, first + count - g);
      Slot sl{k == 1 ? 1 : 2, g, k, {INFINITY, INFINITY, INFINITY}, {-INFINITY, -INFINITY, -INFINITY}};
      for (uint32_t q = 0; q < k; q++) {
        double lo[3], hi[3];
        prim_box(prims[g + q], lo, hi);
        for (int a = 0; a < 3; a++) sl.lo[a] = std::min(sl.lo[a], lo[a]), sl.hi[a] = std::max(sl.hi[a], hi[a]);
      }
      r.push_back(sl);
    }
    return r;
  };
  // number of slots a slot opens into inside the current node (0: cannot open)
  auto fan = [&](const Slot& s) -> uint32_t {
    if (s.kind == 0) return n[s.id].is_leaf ? 0 : 2;
    if (s.kind == 2) return s.count <= 4 ? s.count : 0;
    return 0;
  };
  int need = 0;
  struct Item {
    std::vector<Slot> slots;
    int64_t parent_slot;
    int depth;
  };
  std::vector<Item> work;
  if (n[0].is_leaf) work.push_back({range_slots(n[0].left_first, n[0].right_count), -1, 0});
  else work.push_back({{node_slot(n[0].left_first), node_slot(n[0].right_count)}, -1, 0});
  while (!work.empty()) {
    Item it = std::move(work.back());
    work.pop_back();
    const int32_t me = (int32_t)out.size();
    if (it.parent_slot >= 0) out[it.parent_slot >> 2].child[it.parent_slot & 3] = me;
    out.push_back(F4Node{});
    std::vector<Slot>& slots = it.slots;
    while (slots.size() < 4) {
      int pick = -1;
      double best = -1.0;
      for (size_t k = 0; k < slots.size(); k++) {
        const uint32_t f = fan(slots[k]);
        if (f && slots.size() - 1 + f <= 4 && area(slots[k]) > best) best = area(slots[k]), pick = (int)k;
      }
      if (pick < 0) break;
      const Slot b = slots[pick];
      std::vector<Slot> rep;
      if (b.kind == 0) rep = {node_slot(n[b.id].left_first), node_slot(n[b.id].right_count)};
      else rep = range_slots(b.id, b.count);
      slots.erase(slots.begin() + pick);
      slots.insert(slots.begin() + pick, rep.begin(), rep.end());
    }
    int internal = 0;
    for (const Slot& sl : slots) internal += (sl.kind == 2 || (sl.kind == 0 && !n[sl.id].is_leaf)) ? 1 : 0;
    const int child_depth = it.depth + std::max(0, internal - 1);
    need = std::max(need, child_depth);
    F4Node& f = out[me];
    for (int c = 0; c < 4; c++) {
      if (c >= (int)slots.size() || (slots[c].kind == 0 && n[slots[c].id].is_leaf && n[slots[c].id].right_count == 0)) {
        f.child[c] = -1;  // empty slot: inverted box, never entered
        f.lox[c] = f.loy[c] = f.loz[c] = INFINITY;
        f.hix[c] = f.hiy[c] = f.hiz[c] = -INFINITY;
        continue;
      }
      const Slot& sl = slots[c];
      f.lox[c] = round_down(sl.lo[0]), f.loy[c] = round_down(sl.lo[1]), f.loz[c] = round_down(sl.lo[2]);
      f.hix[c] = round_up(sl.hi[0]), f.hiy[c] = round_up(sl.hi[1]), f.hiz[c] = round_up(sl.hi[2]);
      uint32_t first;
      if (sl.kind == 1) first = sl.id;
      else if (sl.kind == 0 && n[sl.id].is_leaf) first = n[sl.id].left_first;  // one-primitive binary leaf
      else continue;  // internal: patched when the child is emitted
      f.child[c] = ~(int32_t)first;
      f.counts[c >> 1] |= 1u << (16 * (c & 1));
    }
    // push in reverse so children are laid out in slot order (pre-order)
    for (int c = (int)slots.size() - 1; c >= 0; c--) {
      const Slot& sl = slots[c];
      if (sl.kind == 2) {
        work.push_back({range_slots(sl.id, sl.count), (int64_t)me * 4 + c, child_depth});
      } else if (sl.kind == 0 && !n[sl.id].is_leaf) {
        work.push_back({{node_slot(n[sl.id].left_first), node_slot(n[sl.id].right_count)}, (int64_t)me * 4 + c,
                        child_depth});
      }
    }
  }
  return need;
}

// Fast-path tree of our own: binned SAH on all three axes (32 bins)
// over the conservative primitive boxes (prim_box), split down to one primitive per leaf;
// the result uses the reference node layout (pre-order, leaf = one primitive by its index
// in the scene's prim array) so build_fast4 collapses it like the reference tree.  The
// fast path only needs the closest hit among the same primitives, which any conservative
// tree over them yields (up to exact ties), so the tree itself is free to differ.
struct SahItem {
  double lo[3], hi[3], c[3];
  uint32_t prim;
};
static double half_area(const double lo[3], const double hi[3]) {
  const double dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
  return dx * dy + dy * dz + dz * dx;
}
static int own_sah_node(std::vector<SahItem>& it, int b, int e, std::vector<rtx_bvh_node>& out) {
  const int me = (int)out.size();
  out.push_back(rtx_bvh_node{});
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  double clo[3] = {INFINITY, INFINITY, INFINITY}, chi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int i = b; i < e; i++)
    for (int a = 0; a < 3; a++) {
      lo[a] = std::min(lo[a], it[i].lo[a]), hi[a] = std::max(hi[a], it[i].hi[a]);
      clo[a] = std::min(clo[a], it[i].c[a]), chi[a] = std::max(chi[a], it[i].c[a]);
    }
  for (int a = 0; a < 3; a++) out[me].lo[a] = lo[a], out[me].hi[a] = hi[a];
  if (e - b == 1) {
    out[me].is_leaf = 1, out[me].left_first = it[b].prim, out[me].right_count = 1;
    return me;
  }
  constexpr int kB = 32;
  int best_axis = -1, best_plane = -1;
  double best = INFINITY;
  for (int a = 0; a < 3; a++) {
    const double ext = chi[a] - clo[a];
    if (!(ext > 0)) continue;
    int cnt[kB] = {0};
    double blo[kB][3], bhi[kB][3];
    for (int k = 0; k < kB; k++)
      for (int q = 0; q < 3; q++) blo[k][q] = INFINITY, bhi[k][q] = -INFINITY;
    const double sc = kB / ext;
    for (int i = b; i < e; i++) {
      const int k = std::min(kB - 1, std::max(0, (int)((it[i].c[a] - clo[a]) * sc)));
      cnt[k]++;
      for (int q = 0; q < 3; q++) blo[k][q] = std::min(blo[k][q], it[i].lo[q]), bhi[k][q] = std::max(bhi[k][q], it[i].hi[q]);
    }
    double rarea[kB];
    int rcnt[kB];
    double alo[3] = {INFINITY, INFINITY, INFINITY}, ahi[3] = {-INFINITY, -INFINITY, -INFINITY};
    int n = 0;
    for (int k = kB - 1; k >= 1; k--) {
      n += cnt[k];
      for (int q = 0; q < 3; q++) alo[q] = std::min(alo[q], blo[k][q]), ahi[q] = std::max(ahi[q], bhi[k][q]);
      rcnt[k] = n, rarea[k] = n ? half_area(alo, ahi) : 0.0;
    }
    for (int q = 0; q < 3; q++) alo[q] = INFINITY, ahi[q] = -INFINITY;
    n = 0;
    for (int k = 0; k < kB - 1; k++) {
      n += cnt[k];
      for (int q = 0; q < 3; q++) alo[q] = std::min(alo[q], blo[k][q]), ahi[q] = std::max(ahi[q], bhi[k][q]);
      if (n == 0 || rcnt[k + 1] == 0) continue;
      const double cost = half_area(alo, ahi) * n + rarea[k + 1] * rcnt[k + 1];
      if (cost < best) best = cost, best_axis = a, best_plane = k;
    }
  }
  int mid;
  if (best_axis >= 0) {
    const double ext = chi[best_axis] - clo[best_axis], sc = kB / ext, c0 = clo[best_axis];
    auto m = std::partition(it.begin() + b, it.begin() + e, [&](const SahItem& x) {
      return std::min(kB - 1, std::max(0, (int)((x.c[best_axis] - c0) * sc))) <= best_plane;
    });
    mid = (int)(m - it.begin());
  } else {
    mid = (b + e) / 2;  // coincident centroids: split the list
  }
  if (mid == b || mid == e) mid = (b + e) / 2;
  const int l = own_sah_node(it, b, mid, out);
  const int r = own_sah_node(it, mid, e, out);
  out[me].is_leaf = 0, out[me].left_first = (uint32_t)l, out[me].right_count = (uint32_t)r;
  return me;
}
static void build_own_sah(const rtx_prim* prims, int64_t n, const int32_t* skip, int n_skip,
                          std::vector<rtx_bvh_node>& out) {
  std::vector<SahItem> it;
  it.reserve((size_t)n);
  for (int64_t i = 0; i < n; i++) {
    if (std::find(skip, skip + n_skip, (int32_t)i) != skip + n_skip) continue;
    SahItem x;
    prim_box(prims[i], x.lo, x.hi);
    for (int a = 0; a < 3; a++) x.c[a] = 0.5 * (x.lo[a] + x.hi[a]);
    x.prim = (uint32_t)i;
    it.push_back(x);
  }
  out.clear();
  out.reserve(2 * it.size());
  if (!it.empty()) own_sah_node(it, 0, (int)it.size(), out);
}

// Primitives the fast path tests outside its tree (DScene::global, trav_globals): up to two
// whose conservative box has at least the surface area of the union of all other
// primitives' boxes, i.e. a box that nearly every ray's walk would enter at the root anyway
// (the ground spheres of the final, bunny and mixed scenes: r = 1000 against a scene a few
// tens of units wide).  At least two primitives stay in the tree so its root is internal.
static int build_global_prims(const rtx_prim* prims, int64_t n, int32_t out[2]) {
  int k = 0;
  while (k < 2 && n - k > 2) {
    // largest remaining box, and the union of the others
    int64_t big = -1;
    double big_area = -1.0;
    for (int64_t i = 0; i < n; i++) {
      if (std::find(out, out + k, (int32_t)i) != out + k) continue;
      double lo[3], hi[3];
      prim_box(prims[i], lo, hi);
      const double a = half_area(lo, hi);
      if (a > big_area) big_area = a, big = i;
    }
    double ulo[3] = {INFINITY, INFINITY, INFINITY}, uhi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t i = 0; i < n; i++) {
      if (i == big || std::find(out, out + k, (int32_t)i) != out + k) continue;
      double lo[3], hi[3];
      prim_box(prims[i], lo, hi);
      for (int a = 0; a < 3; a++) ulo[a] = std::min(ulo[a], lo[a]), uhi[a] = std::max(uhi[a], hi[a]);
    }
    if (!(big >= 0 && std::isfinite(big_area) && big_area >= half_area(ulo, uhi))) break;
    out[k++] = (int32_t)big;
  }
  return k;
}

int pick_stack(int depth) {
  if (depth + 2 <= 32) return 32;
  if (depth + 2 <= 64) return 64;
  return -1;
}

// Node indices sorted by height (stable), and where each height starts: lvl[k] .. lvl[k + 1] are
// the nodes of height k in `order`.
void group_by_height(const std::vector<int>& h, std::vector<uint32_t>& order, std::vector<int64_t>& lvl) {
  int top = 0;
  for (int v : h) top = std::max(top, v);
  lvl.assign((size_t)top + 2, 0);
  for (int v : h) lvl[(size_t)v + 1]++;
  for (size_t k = 1; k < lvl.size(); k++) lvl[k] += lvl[k - 1];
  order.resize(h.size());
  std::vector<int64_t> at(lvl.begin(), lvl.end() - 1);
  for (size_t i = 0; i < h.size(); i++) order[(size_t)at[h[i]]++] = (uint32_t)i;
}

}  // namespace

namespace rtxplan {

const char* bad_nodes(const rtx_scene_desc* d) {
  for (int64_t i = 0; i < d->n_nodes; i++) {
    const rtx_bvh_node& n = d->nodes[i];
    if (n.is_leaf) {
      if ((int64_t)n.left_first + n.right_count > d->n_prims) return "leaf range out of bounds";
    } else if (n.left_first >= d->n_nodes || n.right_count >= d->n_nodes || n.left_first <= i || n.right_count <= i) {
      return "child index out of bounds (nodes must be pre-order)";
    }
  }
  return nullptr;
}

void plan_fast_tree(const rtx_scene_desc* d, FastPlan& p) {
  p = FastPlan{};
  if (!(d->nodes && d->n_nodes > 0)) return;
  p.depth = bvh_depth(d->nodes, d->n_nodes);
  p.stack_parity = pick_stack(p.depth);
  p.stack_fast = p.stack_parity;
  if (p.stack_parity < 0) return;
  if (!d->nodes[0].is_leaf) {
    // the fast path's tree: our own binned SAH tree over the primitives (without the global
    // ones), collapsed to BVH4 (r01: +2 % C2 / bunny, +6 % C5 over collapsing the reference's)
    std::vector<rtx_bvh_node> own;
    p.n_global = build_global_prims(d->prims, d->n_prims, p.global);
    build_own_sah(d->prims, d->n_prims, p.global, p.n_global, own);
    const int need = build_fast4(own.data(), d->prims, p.f4);
    p.stack_fast = need < 0 ? -1 : (need <= 32 ? 32 : (need <= 64 ? 64 : -1));
    p.fast_need = need;
    p.fast_ok = p.stack_fast > 0;
  }
  if (p.fast_ok && d->n_prims > 0) {  // the one kind of the tree's primitives (globals excluded)
    int k = -2;
    for (int64_t i = 0; i < d->n_prims && k != -1; i++) {
      if ((p.n_global > 0 && p.global[0] == i) || (p.n_global > 1 && p.global[1] == i)) continue;
      k = k == -2 ? d->prims[i].kind : (k == d->prims[i].kind ? k : -1);
    }
    p.tree_kind = k < 0 ? -1 : k;
  }
}

const char* plan_scene(const rtx_scene_desc* d, ScenePlan& p) {
  p = ScenePlan{};
  if (d->n_prims < 0 || d->n_nodes < 0 || d->n_materials < 0 || d->n_textures < 0 || d->n_images < 0)
    return "negative counts";
  if (d->n_prims > 0 && !d->prims) return "prims is NULL";
  if (d->n_materials > 0 && !d->materials) return "materials is NULL";
  if (d->n_textures > 0 && !d->textures) return "textures is NULL";
  if (d->n_images > 0 && !d->images) return "images is NULL";
  if (d->n_nodes > 0 && !d->nodes) return "nodes is NULL";
  if (d->n_prims > 0x7FFFFFFFll) return "more than 2^31-1 primitives";
  // validate indices so kernels never read out of bounds
  for (int64_t i = 0; i < d->n_prims; i++) {
    const rtx_prim& q = d->prims[i];
    if (q.kind < RTX_PRIM_SPHERE || q.kind > RTX_PRIM_YZ_RECT) return "bad primitive kind";
    if (q.material < 0 || q.material >= d->n_materials) return "primitive material out of range";
  }
  for (int32_t i = 0; i < d->n_materials; i++) {
    const rtx_material& m = d->materials[i];
    if (m.kind < 0 || m.kind > RTX_MAT_DIFFUSE_LIGHT) return "bad material kind";
    if ((m.kind == RTX_MAT_LAMBERTIAN || m.kind == RTX_MAT_DIFFUSE_LIGHT) && (m.texture < 0 || m.texture >= d->n_textures))
      return "material texture out of range";
  }
  for (int32_t i = 0; i < d->n_textures; i++) {
    const rtx_texture& t = d->textures[i];
    // the device treats every kind other than solid / checker as an image lookup
    if (t.kind < RTX_TEX_SOLID || t.kind > RTX_TEX_IMAGE) return "bad texture kind";
    if (t.kind == RTX_TEX_CHECKER && (t.even < 0 || t.even >= d->n_textures || t.odd < 0 || t.odd >= d->n_textures))
      return "checker child out of range";
    if (t.kind == RTX_TEX_IMAGE && t.image >= d->n_images) return "image index out of range";
  }
  for (int32_t i = 0; i < d->n_images; i++) {
    const rtx_image& im = d->images[i];
    if (im.width < 0 || im.height < 0) return "negative image size";
    if ((int64_t)im.width * im.height > (1ll << 31)) return "image above 2^31 texels";
  }
  if (const char* why = bad_nodes(d)) return why;
  plan_fast_tree(d, p.fast);
  if (p.fast.stack_parity < 0) return "BVH deeper than 62 levels";
  const FastPlan& fp = p.fast;
  const std::vector<F4Node>& f4 = fp.f4;
  // Triangle normals for the hit records (Triangle::Hit, triangle.h:80-82: Normalize(Cross(
  // edge1, edge2))), formed here in the device's double operations and order (cross, len2,
  // sqrt, 1 / l, products; no contraction), so the table holds the very bits finish_hit_at
  // would compute per hit.
  for (int64_t i = 0; i < d->n_prims && !p.has_tris; i++) p.has_tris = d->prims[i].kind == RTX_PRIM_TRIANGLE;
  if (p.has_tris) {
    p.tri_n.assign((size_t)d->n_prims * 4, 0.0);
    for (int64_t i = 0; i < d->n_prims; i++) {
      const rtx_prim& q = d->prims[i];
      if (q.kind != RTX_PRIM_TRIANGLE) continue;
      double nrm[3];
      rtxb::tri_unit_normal(q.g, nrm);  // (0, 0, 0) for a zero length, as normalize() returns
      for (int a = 0; a < 3; a++) p.tri_n[4 * (size_t)i + a] = nrm[a];
    }
  }
  // device table: triangles carry A, B - A, C - A (tri_e1 / tri_e2)
  p.prims.assign(d->prims, d->prims + d->n_prims);
  for (rtx_prim& q : p.prims)
    if (q.kind == RTX_PRIM_TRIANGLE)
      for (int a = 0; a < 3; a++) q.g[3 + a] = q.g[3 + a] - q.g[a], q.g[6 + a] = q.g[6 + a] - q.g[a];
  // Device copy of the material table: a Lambertian / DiffuseLight whose texture is a
  // SolidColor carries the colour itself (texture = -1, colour in the unused albedo field),
  // so shading skips the dependent texture-table load (mat_tex, rtx_device.h).
  p.mats.assign(d->materials, d->materials + d->n_materials);
  for (rtx_material& m : p.mats) {
    if ((m.kind == RTX_MAT_LAMBERTIAN || m.kind == RTX_MAT_DIFFUSE_LIGHT) && m.texture >= 0 &&
        d->textures[m.texture].kind == RTX_TEX_SOLID) {
      for (int c = 0; c < 3; c++) m.albedo[c] = d->textures[m.texture].color[c];
      m.texture = -1;
    }
  }
  // Dielectric: eta on a front-face hit (eta_i / eta_t = 1 / ri) and Schlick's r0 for
  // reflectance(c, ri) (material.cc:226-262) in the unused albedo field, computed with the same
  // IEEE double operations the kernel would perform (shade_merged, rtx_device.h).
  for (rtx_material& m : p.mats) {
    if (m.kind != RTX_MAT_DIELECTRIC) continue;
    const double ri = m.ref_idx;
    double r0 = (1.0 - ri) / (1.0 + ri);
    r0 = r0 * r0;
    m.albedo[0] = 1.0 / ri;
    m.albedo[1] = r0;
  }
  // what an in-place update needs (rtx_scene_update_*): the primitives' boxes as the builders saw
  // them, and both trees' nodes by height
  p.kinds.resize((size_t)d->n_prims);
  for (int64_t i = 0; i < d->n_prims; i++) p.kinds[i] = (int8_t)d->prims[i].kind;
  if (d->n_nodes > 0) {
    p.ref_box.resize((size_t)d->n_prims * 6), p.fast_box.resize((size_t)d->n_prims * 6);
    for (int64_t i = 0; i < d->n_prims; i++) {
      rtxb::ref_bounds(d->prims[i].kind, d->prims[i].g, &p.ref_box[6 * (size_t)i]);
      rtxb::fast_box(d->prims[i].kind, d->prims[i].g, &p.fast_box[6 * (size_t)i]);
    }
    std::vector<int> h((size_t)d->n_nodes, 0);
    for (int64_t i = d->n_nodes - 1; i >= 0; i--)  // pre-order (bad_nodes): children come later
      if (!d->nodes[i].is_leaf) h[i] = 1 + std::max(h[d->nodes[i].left_first], h[d->nodes[i].right_count]);
    group_by_height(h, p.node_order, p.node_lvl);
    if (fp.fast_ok) {
      h.assign(f4.size(), 0);
      for (int64_t i = (int64_t)f4.size() - 1; i >= 0; i--)  // build_fast4 emits children after their parent
        for (int c = 0; c < 4; c++)
          if (f4[i].child[c] >= 0) h[i] = std::max(h[i], 1 + h[f4[i].child[c]]);
      group_by_height(h, p.f4_order, p.f4_lvl);
    }
  }
  // the emitter table (rtx_direct.h): the primitives whose material is a DiffuseLight, in the
  // order of the primitive array; kinds and materials stay (an update changes geometry), so the
  // list is final and only the areas are rebuilt
  for (int64_t i = 0; i < d->n_prims; i++)
    if (d->materials[d->prims[i].material].kind == RTX_MAT_DIFFUSE_LIGHT) p.emit_idx.push_back((uint32_t)i);
  p.use_bvh = d->n_nodes > 0 ? 1 : 0;
  p.n_prims = d->n_prims;
  if (p.use_bvh && d->nodes[0].is_leaf) p.froot_leaf = 1, p.froot_count = (int32_t)d->nodes[0].right_count;
  p.n_global = fp.fast_ok ? fp.n_global : 0;
  p.all_lambertian = d->n_materials > 0 ? 1 : 0;
  for (int32_t i = 0; i < d->n_materials && p.all_lambertian; i++)
    p.all_lambertian = d->materials[i].kind == RTX_MAT_LAMBERTIAN;
  for (const rtx_material& m : p.mats)
    if ((m.kind == RTX_MAT_LAMBERTIAN || m.kind == RTX_MAT_DIFFUSE_LIGHT) && m.texture >= 0) p.no_textures = 0;
  p.tree_kind = fp.tree_kind;  // the one kind of the tree's primitives (globals excluded)
  p.global[0] = fp.global[0], p.global[1] = fp.global[1];
  // Plain global spheres (kGlobalSpheres, rtx_device.h): when every global is a sphere with
  // radius > 0, fmax(0, radius) is the radius itself and radius * radius, the one product the
  // test forms from the record alone, goes into the record's unused g[4], in the device's IEEE
  // double multiplication.  An in-place update that reaches a global withdraws the flag
  // (update_and_refit): the test then reads the record as any primitive's.
  bool plain = p.n_global > 0;
  for (int k = 0; k < p.n_global; k++) {
    const rtx_prim& q = d->prims[p.global[k]];
    plain = plain && q.kind == RTX_PRIM_SPHERE && q.g[3] > 0.0;
  }
  for (int k = 0; k < p.n_global && plain; k++) {
    const double r = d->prims[p.global[k]].g[3], r2 = r * r;
    p.prims[p.global[k]].g[4] = r2;
  }
  if (plain) p.n_global |= kPlainGlobalSpheres;
  return nullptr;
}

}  // namespace rtxplan
