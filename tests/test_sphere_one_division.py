"""The global spheres' root selection (rtx_device.h sphere_root): Sphere::Hit tries root1 =
(h - sq) / a and then root2 = (h + sq) / a against (tmin, tmax); the kernel divides once where
h - sq <= 0 decides that root1 fails (a positive and finite, tmin >= 0).  A small C++ program
(g++, -ffp-contract=off like the oracle) restates both sequences on the host and requires the same
decision and the same t, bit for bit, on 10^6 seeded rays against the bunny scene's ground sphere
(centre (0, -1003.9, 0), radius 1000) and on the edge cases: origins on, just above and just inside
the surface, directions through the horizon, tmax finite and infinite, and the guarded inputs
(a == 0, a NaN direction, tmin < 0), which take the original sequence."""
import shutil
import subprocess

import pytest

SRC = r"""
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
static uint64_t s = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
static double uni() { return (double)(rnd() >> 11) * 0x1p-53; }
static double uni(double a, double b) { return a + (b - a) * uni(); }
struct V3 { double x, y, z; };
static V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
static double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static double len2(V3 a) { return a.x * a.x + a.y * a.y + a.z * a.z; }
static const V3 C = {0.0, -1003.9, 0.0};
static const double R = 1000.0;

// the original sequence (Sphere::Hit up to the accepted root)
static bool ref_t(V3 o, V3 d, double tmin, double tmax, double& t) {
  const double radius = std::fmax(0.0, R);
  const V3 oc = sub(C, o);
  const double a = len2(d), h = dot(d, oc), cc = len2(oc) - radius * radius;
  const double disc = h * h - a * cc;
  if (disc < 0) return false;
  const double sq = std::sqrt(disc);
  double root = (h - sq) / a;
  if (!(tmin < root && root < tmax)) {
    root = (h + sq) / a;
    if (!(tmin < root && root < tmax)) return false;
  }
  t = root;
  return true;
}
// the kernel's: radius * radius formed once by the host, one division where h - sq <= 0
static int guarded = 0, second = 0;
static bool sphere_root(double a, double h, double sq, double tmin, double tmax, double& root) {
  const double n1 = h - sq;
  const bool orig = !(a > 0.0 && a < INFINITY && tmin >= 0.0);
  const bool near_first = orig || n1 > 0.0;
  guarded += orig;
  root = (near_first ? n1 : h + sq) / a;
  bool ok = tmin < root && root < tmax;
  if (!ok && near_first) {
    second++;
    root = (h + sq) / a;
    ok = tmin < root && root < tmax;
  }
  return ok;
}
static const double R2 = R * R;
static bool new_t(V3 o, V3 d, double tmin, double tmax, double& t) {
  const V3 oc = sub(C, o);
  const double a = len2(d), h = dot(d, oc), cc = len2(oc) - R2;
  const double disc = h * h - a * cc;
  return !(disc < 0) && sphere_root(a, h, std::sqrt(disc), tmin, tmax, t);
}
static long bad = 0, tot = 0, hits = 0;
static void check(V3 o, V3 d, double tmin, double tmax) {
  double t0 = 0, t1 = 0;
  const bool r0 = ref_t(o, d, tmin, tmax, t0), r1 = new_t(o, d, tmin, tmax, t1);
  tot++, hits += r0;
  if (r0 != r1 || (r0 && std::memcmp(&t0, &t1, 8) != 0)) {
    if (bad < 5) std::printf("o=(%a %a %a) d=(%a %a %a) tmin=%a tmax=%a: %d %a vs %d %a\n", o.x, o.y, o.z, d.x, d.y, d.z,
                             tmin, tmax, (int)r0, t0, (int)r1, t1);
    bad++;
  }
}
static V3 rand_dir() { return {uni(-1, 1), uni(-1, 1), uni(-1, 1)}; }
// a point of the sphere near its top (where the bunny scene's rays meet it), moved by `off` along the radius
static V3 surface(double off) {
  const double x = uni(-30, 30), z = uni(-30, 30);
  const double y = std::sqrt(R * R - x * x - z * z);
  const double k = (R + off) / R;
  return {C.x + x * k, C.y + y * k, C.z + z * k};
}
int main() {
  const double tmins[] = {0.001, (double)0.001f, 0.0};
  // seeded rays as a render sends them: from above the ground, in any direction
  for (int i = 0; i < 1000000; i++) {
    const V3 o = {uni(-20, 20), uni(-3.9, 12), uni(-20, 20)};
    check(o, rand_dir(), tmins[i % 3], (i & 1) ? INFINITY : uni(0.0, 60.0));
  }
  // origins on, just above and just inside the surface (a scattered ray starts at a hit point)
  const double offs[] = {0.0, 1e-13, -1e-13, 1e-9, -1e-9, 1e-4, -1e-4, 0.00099, 0.0011, -0.0011};
  for (int i = 0; i < 400000; i++) {
    const V3 o = surface(offs[i % 10]);
    check(o, rand_dir(), tmins[i % 3], (i & 1) ? INFINITY : uni(0.0, 2500.0));
  }
  // directions through the horizon: tangent to the sphere at the origin, tilted by a few ulps and more
  for (int i = 0; i < 400000; i++) {
    const V3 o = surface(offs[i % 10]);
    const V3 n = sub(o, C);
    V3 d = rand_dir();
    const double k = dot(d, n) / len2(n);
    const double tilt = (i % 4 == 0) ? 0.0 : uni(-1, 1) * std::ldexp(1.0, -(int)(rnd() % 60));
    d = {d.x - (k - tilt) * n.x, d.y - (k - tilt) * n.y, d.z - (k - tilt) * n.z};
    check(o, d, tmins[i % 3], (i & 1) ? INFINITY : uni(0.0, 2500.0));
  }
  const long before = guarded;
  // the guarded inputs: a == 0, NaN and infinite directions, tmin < 0
  for (int i = 0; i < 100000; i++) {
    const V3 o = (i & 1) ? surface(offs[i % 10]) : V3{uni(-20, 20), uni(-3.9, 12), uni(-20, 20)};
    V3 d = rand_dir();
    double tmin = 0.001;
    switch (i % 5) {
      case 0: d = {0.0, 0.0, 0.0}; break;
      case 1: d.y = NAN; break;
      case 2: d.x = INFINITY; break;
      case 3: tmin = -uni(0.0, 3000.0); break;
      default: d = {d.x * 0x1p-540, d.y * 0x1p-540, d.z * 0x1p-540};  // a underflows to 0 or a denormal
    }
    check(o, d, tmin, (i & 2) ? INFINITY : uni(0.0, 2500.0));
  }
  std::printf("checked %ld hits %ld guarded %ld second %d mismatches %ld\n", tot, hits, guarded - before, second, bad);
  // the cases must reach every branch: accepted roots, the original sequence, the second division
  return bad != 0 || hits < tot / 10 || guarded - before < 60000 || second < 1000;
}
"""


def test_one_division_root_equals_the_two_division_sequence(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ unavailable")
    src, exe = tmp_path / "sphere_root.cc", tmp_path / "sphere_root"
    src.write_text(SRC)
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-o", str(exe), str(src)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout
    assert "mismatches 0" in r.stdout
