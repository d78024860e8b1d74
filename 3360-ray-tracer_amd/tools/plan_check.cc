// plan_check — the scene planner (csrc/rtx_scene_plan.cc) on hand-made descriptions, built with
// -fsanitize=address,undefined (make plan_check): every description runs through plan_scene,
// the accepted ones are checked for the invariants tests/test_fast_tree.py states (every
// primitive outside the globals in exactly one leaf slot, children after parents, fast_need
// within stack_fast, the height orders permutations), the rejected ones for their message.
// Exit status 0: every check held and the sanitizers stayed silent.  Needs no device.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "rtx_bounds.h"
#include "rtx_scene_plan.h"

using rtxd::F4Node;
using rtxplan::ScenePlan;

static int g_failed = 0;
static const char* g_case = "";
#define CHECK(cond)                                                            \
  do {                                                                         \
    if (!(cond)) {                                                             \
      std::printf("  FAILED %s: %s (line %d)\n", g_case, #cond, __LINE__);     \
      g_failed++;                                                              \
      return;                                                                  \
    }                                                                          \
  } while (0)

// A description that owns its arrays: two solid textures, Lambertians 0 and 1, a metal, a
// dielectric and a light (materials 2, 3, 4)
struct Scene {
  std::vector<rtx_prim> prims;
  std::vector<rtx_bvh_node> nodes;
  std::vector<rtx_material> mats;
  std::vector<rtx_texture> texs;
  Scene() {
    texs.resize(2), mats.resize(5);
    const double col[2][3] = {{0.5, 0.5, 0.5}, {0.9, 0.2, 0.1}};
    for (int t = 0; t < 2; t++) {
      texs[t] = rtx_texture{};
      texs[t].kind = RTX_TEX_SOLID, texs[t].even = texs[t].odd = texs[t].image = -1;
      for (int c = 0; c < 3; c++) texs[t].color[c] = col[t][c];
    }
    const int kind[5] = {RTX_MAT_LAMBERTIAN, RTX_MAT_LAMBERTIAN, RTX_MAT_METAL, RTX_MAT_DIELECTRIC, RTX_MAT_DIFFUSE_LIGHT};
    for (int m = 0; m < 5; m++) {
      mats[m] = rtx_material{};
      mats[m].kind = kind[m], mats[m].texture = m < 2 ? m : (m == 4 ? 1 : -1), mats[m].ref_idx = 1.5;
      for (int c = 0; c < 3; c++) mats[m].albedo[c] = 0.8;
    }
  }
  void sphere(double x, double y, double z, double r, int m = 0) {
    rtx_prim p{};
    p.kind = RTX_PRIM_SPHERE, p.material = m;
    p.g[0] = x, p.g[1] = y, p.g[2] = z, p.g[3] = r;
    prims.push_back(p);
  }
  void tri(const double (&v)[9], int m = 0) {
    rtx_prim p{};
    p.kind = RTX_PRIM_TRIANGLE, p.material = m;
    for (int k = 0; k < 9; k++) p.g[k] = v[k];
    prims.push_back(p);
  }
  void rect(int kind, double a0, double a1, double b0, double b1, double k, int m = 0) {
    rtx_prim p{};
    p.kind = kind, p.material = m;
    p.g[0] = a0, p.g[1] = a1, p.g[2] = b0, p.g[3] = b1, p.g[4] = k;
    prims.push_back(p);
  }
  // one node over primitives [first, first + count): the union of their reference boxes
  rtx_bvh_node leaf(uint32_t first, uint32_t count) const {
    rtx_bvh_node n{};
    n.is_leaf = 1, n.left_first = first, n.right_count = count;
    for (int a = 0; a < 3; a++) n.lo[a] = INFINITY, n.hi[a] = -INFINITY;
    for (uint32_t i = first; i < first + count; i++) {
      double b[6];
      rtxb::ref_bounds(prims[i].kind, prims[i].g, b);
      for (int a = 0; a < 3; a++) n.lo[a] = std::fmin(n.lo[a], b[a]), n.hi[a] = std::fmax(n.hi[a], b[3 + a]);
    }
    return n;
  }
  // pre-order tree over [first, first + count) split in the middle, leaves of at most `per`
  uint32_t split(uint32_t first, uint32_t count, uint32_t per) {
    const uint32_t me = (uint32_t)nodes.size();
    nodes.push_back(leaf(first, count));
    if (count <= per) return me;
    const uint32_t l = split(first, count / 2, per), r = split(first + count / 2, count - count / 2, per);
    nodes[me].is_leaf = 0, nodes[me].left_first = l, nodes[me].right_count = r;
    return me;
  }
  // a caterpillar of `levels` levels over primitives 0 .. levels - 1: every internal node has one
  // one-primitive leaf and the rest of the chain as its left (side 0) or right child
  uint32_t chain(uint32_t k, uint32_t levels, int side) {
    const uint32_t me = (uint32_t)nodes.size();
    if (k + 1 == levels) {
      nodes.push_back(leaf(k, 1));
      return me;
    }
    nodes.push_back(leaf(k, levels - k));
    uint32_t l, r;
    if (side == 0) l = chain(k + 1, levels, side), r = (uint32_t)nodes.size(), nodes.push_back(leaf(k, 1));
    else l = (uint32_t)nodes.size(), nodes.push_back(leaf(k, 1)), r = chain(k + 1, levels, side);
    nodes[me].is_leaf = 0, nodes[me].left_first = l, nodes[me].right_count = r;
    return me;
  }
  rtx_scene_desc desc() const {
    rtx_scene_desc d{};
    d.prims = prims.empty() ? nullptr : prims.data(), d.n_prims = (int64_t)prims.size();
    d.nodes = nodes.empty() ? nullptr : nodes.data(), d.n_nodes = (int64_t)nodes.size();
    d.materials = mats.data(), d.n_materials = (int32_t)mats.size();
    d.textures = texs.data(), d.n_textures = (int32_t)texs.size();
    return d;
  }
};

// order: a permutation of 0 .. n - 1 in runs lvl[k] .. lvl[k + 1] of equal height, every child
// (kids(i, out)) at a lower height than its parent
static bool heights_ok(const std::vector<uint32_t>& order, const std::vector<int64_t>& lvl, size_t n,
                       const std::function<void(size_t, std::vector<size_t>&)>& kids) {
  if (order.size() != n || lvl.size() < 2 || lvl.front() != 0 || lvl.back() != (int64_t)n) return false;
  std::vector<int> height(n, -1);
  for (size_t k = 0; k + 1 < lvl.size(); k++) {
    if (lvl[k] > lvl[k + 1]) return false;
    for (int64_t j = lvl[k]; j < lvl[k + 1]; j++) {
      if (order[(size_t)j] >= n || height[order[(size_t)j]] != -1) return false;
      height[order[(size_t)j]] = (int)k;
    }
  }
  std::vector<size_t> c;
  for (size_t i = 0; i < n; i++) {
    c.clear(), kids(i, c);
    int top = -1;
    for (size_t q : c) top = std::max(top, height[q]);
    if (height[i] != top + 1) return false;
  }
  return true;
}

static void check_plan(const Scene& sc, const ScenePlan& p) {
  const size_t n = sc.prims.size(), nn = sc.nodes.size();
  const rtxplan::FastPlan& fp = p.fast;
  const int ng = p.n_global & 3;
  // the tables
  CHECK(p.prims.size() == n && p.kinds.size() == n && p.mats.size() == sc.mats.size() && p.n_prims == (int64_t)n);
  CHECK(p.use_bvh == (nn > 0));
  CHECK(p.tri_n.size() == (p.has_tris ? 4 * n : 0));
  CHECK(p.ref_box.size() == (nn ? 6 * n : 0) && p.fast_box.size() == (nn ? 6 * n : 0));
  bool tris = false;
  for (size_t i = 0; i < n; i++) {
    CHECK(p.kinds[i] == sc.prims[i].kind && p.prims[i].kind == sc.prims[i].kind);
    tris = tris || sc.prims[i].kind == RTX_PRIM_TRIANGLE;
    if (sc.prims[i].kind == RTX_PRIM_TRIANGLE) {
      for (int a = 0; a < 3; a++) CHECK(p.prims[i].g[3 + a] == sc.prims[i].g[3 + a] - sc.prims[i].g[a]);
      const double* t = &p.tri_n[4 * i];
      const double l2 = t[0] * t[0] + t[1] * t[1] + t[2] * t[2];
      CHECK(t[3] == 0.0 && (l2 == 0.0 || std::fabs(l2 - 1.0) < 1e-12));
    }
    if (nn) {
      for (int a = 0; a < 3; a++) CHECK(p.ref_box[6 * i + a] <= p.ref_box[6 * i + 3 + a]);
      for (int a = 0; a < 3; a++) CHECK(p.fast_box[6 * i + a] <= p.fast_box[6 * i + 3 + a]);
    }
  }
  CHECK((p.has_tris != 0) == tris);
  for (const rtx_material& m : p.mats) CHECK(m.texture == -1);  // (the textures here are solid colours)
  CHECK(p.no_textures == 1 && p.all_lambertian == 0);
  size_t lights = 0;
  for (size_t i = 0; i < n; i++) lights += sc.mats[sc.prims[i].material].kind == RTX_MAT_DIFFUSE_LIGHT;
  CHECK(p.emit_idx.size() == lights);
  for (uint32_t e : p.emit_idx) CHECK(e < n && sc.mats[sc.prims[e].material].kind == RTX_MAT_DIFFUSE_LIGHT);
  // the stacks
  CHECK(fp.stack_parity == 32 || fp.stack_parity == 64);
  if (nn == 0 || sc.nodes[0].is_leaf) {  // flat list / one-leaf root: no fast tree
    CHECK(!fp.fast_ok && fp.f4.empty() && ng == 0 && p.tree_kind == -1 && p.f4_order.empty());
    CHECK(p.froot_leaf == (nn > 0) && p.froot_count == (nn ? (int32_t)sc.nodes[0].right_count : 0));
    if (nn) CHECK(heights_ok(p.node_order, p.node_lvl, nn, [&](size_t, std::vector<size_t>&) {}));
    else CHECK(p.node_order.empty() && p.node_lvl.empty());
    return;
  }
  CHECK(p.froot_leaf == 0);
  CHECK(fp.fast_ok ? (fp.stack_fast == 32 || fp.stack_fast == 64) && fp.fast_need <= fp.stack_fast
                   : fp.stack_fast == -1 && fp.fast_need > 64);
  CHECK(ng == (fp.fast_ok ? fp.n_global : 0) && fp.n_global <= 2 && (int64_t)n - fp.n_global >= 2);
  // every primitive outside the globals in exactly one leaf slot; children after their parent,
  // every node but the root referenced once
  const std::vector<F4Node>& f4 = fp.f4;
  CHECK(!f4.empty());
  std::vector<int> seen(n, 0), refs(f4.size(), 0);
  for (size_t i = 0; i < f4.size(); i++)
    for (int c = 0; c < 4; c++) {
      const int32_t ch = f4[i].child[c];
      const bool empty = f4[i].lox[c] == INFINITY && f4[i].hix[c] == -INFINITY;
      if (empty) {
        CHECK(ch == -1 && c >= 2);
      } else if (ch >= 0) {
        CHECK((size_t)ch > i && (size_t)ch < f4.size());
        refs[(size_t)ch]++;
      } else {
        CHECK((size_t)~ch < n);
        seen[(size_t)~ch]++;
        CHECK(f4[i].lox[c] <= f4[i].hix[c] && f4[i].loy[c] <= f4[i].hiy[c] && f4[i].loz[c] <= f4[i].hiz[c]);
      }
    }
  for (size_t i = 0; i < f4.size(); i++) CHECK(refs[i] == (i ? 1 : 0));
  for (size_t i = 0; i < n; i++) {
    const bool global = (fp.n_global > 0 && fp.global[0] == (int32_t)i) || (fp.n_global > 1 && fp.global[1] == (int32_t)i);
    CHECK(seen[i] == (global ? 0 : 1));
  }
  // plain global spheres carry r * r
  if (p.n_global & rtxplan::kPlainGlobalSpheres)
    for (int k = 0; k < ng; k++) {
      const rtx_prim& q = sc.prims[(size_t)p.global[k]];
      CHECK(q.kind == RTX_PRIM_SPHERE && q.g[3] > 0.0 && p.prims[(size_t)p.global[k]].g[4] == q.g[3] * q.g[3]);
    }
  // the height orders
  CHECK(heights_ok(p.node_order, p.node_lvl, nn, [&](size_t i, std::vector<size_t>& out) {
    if (!sc.nodes[i].is_leaf) out.push_back(sc.nodes[i].left_first), out.push_back(sc.nodes[i].right_count);
  }));
  if (fp.fast_ok)
    CHECK(heights_ok(p.f4_order, p.f4_lvl, f4.size(), [&](size_t i, std::vector<size_t>& out) {
      for (int c = 0; c < 4; c++)
        if (f4[i].child[c] >= 0) out.push_back((size_t)f4[i].child[c]);
    }));
  else CHECK(p.f4_order.empty());
}

// plan_scene on `sc`: accepted and checked (want == nullptr), or refused with `want`
static void run(const char* name, const Scene& sc, const char* want = nullptr) {
  g_case = name;
  const rtx_scene_desc d = sc.desc();
  ScenePlan p;
  const char* why = rtxplan::plan_scene(&d, p);
  const int before = g_failed;
  if (want) {
    if (!why || std::strcmp(why, want)) std::printf("  FAILED %s: refused with \"%s\"\n", name, why ? why : "(accepted)"), g_failed++;
  } else if (why) {
    std::printf("  FAILED %s: refused: %s\n", name, why), g_failed++;
  } else {
    check_plan(sc, p);
  }
  if (g_failed == before)
    std::printf("ok  %-28s %s%s  prims %zu nodes %zu f4 %zu need %d stacks %d/%d globals %d\n", name, want ? "refused: " : "",
                want ? want : "", sc.prims.size(), sc.nodes.size(), p.fast.f4.size(), p.fast.fast_need, p.fast.stack_parity,
                p.fast.stack_fast, p.n_global);
}

static Scene spheres(int n) {
  Scene s;
  for (int k = 0; k < n; k++) s.sphere(3.0 * k, 0.25 * k, -0.5 * k, 1.0 + 0.125 * k, k % 3);
  return s;
}
// n spheres at x = 1.25^k with radius proportional to x (tests/test_fast_tree.py line_prims)
static Scene line(int n) {
  Scene s;
  const double ratio = 1.25, rf = 0.5 * (ratio - 1) / (ratio + 1);
  for (int k = 0; k < n; k++) s.sphere(std::pow(ratio, k), 0, 0, rf * std::pow(ratio, k), k % 3);
  s.split(0, (uint32_t)n, 1);
  return s;
}
static Scene chain(int levels, int side) {
  Scene s;
  for (int k = 0; k < levels; k++) s.sphere(3.0 * k, 0, 0, 1.0, k % 3);
  s.chain(0, (uint32_t)levels, side);
  return s;
}
static Scene mixed() {
  Scene s;
  s.sphere(0, 1, 0, 1, 3);
  s.sphere(2, 0.5, 1, -0.5, 2);  // a negative radius
  s.tri({0, 0, 0, 1, 0, 0, 0, 1, 0}, 0);
  s.tri({0.1, 1.0 / 3, 1000.3, 0.1, 1.0 / 3, 1000.3, 0.1, 1.0 / 3, 1000.3}, 1);  // a point: zero area
  s.tri({0, 0, 0, 1, 1, 1, 2, 2, 2}, 1);                                       // collinear: zero area
  s.tri({-1e-3, 2.7, -5.3, 7.1, 1e-40, -0.0, 2.7, 2.7, 0.1}, 2);
  s.rect(RTX_PRIM_XY_RECT, 0, 2, 0, 2, -1, 4);
  s.rect(RTX_PRIM_XZ_RECT, 3, 1, 0, 2, 5, 4);  // reversed interval
  s.rect(RTX_PRIM_YZ_RECT, 0, 2, 0, 2, 3, 0);
  s.split(0, (uint32_t)s.prims.size(), 2);
  return s;
}

int main() {
  run("empty", Scene());
  run("list of 3, no nodes", spheres(3));
  for (int n : {1, 4, 5}) {
    Scene s = spheres(n);
    s.nodes.push_back(s.leaf(0, (uint32_t)n));
    run(("leaf root of " + std::to_string(n)).c_str(), s);
  }
  {
    Scene s = spheres(2);
    s.split(0, 2, 1);
    run("two primitives", s);
  }
  for (int side = 0; side < 2; side++) {
    const std::string w = side ? "right" : "left";
    run(("chain " + w + " 62").c_str(), chain(62, side));
    run(("chain " + w + " 63").c_str(), chain(63, side), "BVH deeper than 62 levels");
  }
  run("line of 64", line(64));
  run("line of 65", line(65));
  run("line, need 64 (295)", line(295));  // the largest stack the fast walk has
  run("line, need 65 (300)", line(300));  // one more: no fast tree
  {
    Scene s;
    s.sphere(0, -1000, 0, 1000, 0), s.sphere(0, 1, 0, 1, 1), s.sphere(3, 0.5, 1, 0.5, 4), s.sphere(-3, 0.5, 1, 0.5, 3);
    s.split(0, 4, 1);
    run("ground sphere", s);
  }
  run("mixed kinds", mixed());
  {
    Scene s = spheres(4);
    s.split(0, 4, 1);
    Scene a = s, b = s, c = s, e = s;
    a.prims[2].kind = 7, run("bad kind", a, "bad primitive kind");
    b.prims[3].material = 5, run("material out of range", b, "primitive material out of range");
    c.nodes[0].left_first = 0, run("child not pre-order", c, "child index out of bounds (nodes must be pre-order)");
    e.nodes.back().right_count = 2, run("leaf range out of bounds", e, "leaf range out of bounds");
  }
  std::printf(g_failed ? "plan_check: %d FAILED\n" : "plan_check: all passed\n", g_failed);
  return g_failed ? 1 : 0;
}
