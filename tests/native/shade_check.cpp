// shade_check.cpp -- CPU check of maniskill_amd/csrc/mssim_raycast_shade.h: the normal, albedo and light routines of the
// flat-shaded view (namespace rc, the code k_raycast_shade runs per pixel) on a table of rays with closed-form answers,
// the one walk (rc::trace) into the depth kernel's hit record and into the shaded view's, ray for ray, and what
// mssim_raycast_set_colours / mssim_raycast_shade refuse (namespace mssim_shade), with every table exactly as long as its
// counts say. Stand-alone (tests/test_shade.py builds it with ASan + UBSan and expects exit status 0).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/mssim.h"
#include "../../include/mssim_hip_tasks.h"
#include "../../maniskill_amd/csrc/mssim_raycast_shade.h"

static int g_failed = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::printf("%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond);   \
      g_failed++;                                                            \
    }                                                                        \
  } while (0)

namespace {

using rc::mk;
using rc::v3;

bool close(float a, float b, float tol = 2e-6f) { return std::fabs(a - b) <= tol; }
bool close3(v3 a, float x, float y, float z, float tol = 2e-6f) { return close(a.x, x, tol) && close(a.y, y, tol) && close(a.z, z, tol); }

struct Entry { float t; v3 n; };
Entry enter(int type, std::vector<float> p, v3 o, v3 d, const std::vector<float>& planes = {}) {
  p.resize(3);
  Entry e{0.f, mk(9.f, 9.f, 9.f)};
  e.t = rc::enter_normal(type, p.data(), o, d, planes.data(), 0, (int)(planes.size() / 4), &e.n);
  return e;
}

unsigned byte_of(unsigned px, int k) { return (px >> (8 * k)) & 0xffu; }

void normals() {
  // plane: +x, from wherever the ray comes; from behind it misses
  Entry e = enter(MSSIM_SHAPE_PLANE, {}, mk(2, 1, -3), mk(-1, 0.3f, 0.2f));
  CHECK(close(e.t, 2.f) && close3(e.n, 1, 0, 0));
  CHECK(std::isinf(enter(MSSIM_SHAPE_PLANE, {}, mk(2, 0, 0), mk(1, 0, 0)).t));
  // box (0.3, 0.2, 0.1): each of the six faces, the sign against d on the axis
  const float h[3] = {0.3f, 0.2f, 0.1f};
  for (int axis = 0; axis < 3; axis++)
    for (int s = -1; s <= 1; s += 2) {
      float o[3] = {0.01f, -0.02f, 0.015f}, d[3] = {0.01f, 0.02f, -0.01f};
      o[axis] = 2.f * s; d[axis] = -1.f * s;
      e = enter(MSSIM_SHAPE_BOX, {h[0], h[1], h[2]}, mk(o[0], o[1], o[2]), mk(d[0], d[1], d[2]));
      CHECK(close(e.t, 2.f - h[axis], 1e-5f));
      CHECK(close3(e.n, axis == 0 ? (float)s : 0.f, axis == 1 ? (float)s : 0.f, axis == 2 ? (float)s : 0.f));
    }
  // a ray down the box's diagonal enters through three slabs at once (a cube, exactly): the lowest axis wins
  e = enter(MSSIM_SHAPE_BOX, {0.5f, 0.5f, 0.5f}, mk(2, 2, 2), mk(-1, -1, -1));
  CHECK(close(e.t, 1.5f) && close3(e.n, 1, 0, 0));
  // a ray parallel to two axes: only the third slab can set the entry
  e = enter(MSSIM_SHAPE_BOX, {0.5f, 0.5f, 0.5f}, mk(0.1f, 0.2f, 3), mk(0, 0, -1));
  CHECK(close(e.t, 2.5f) && close3(e.n, 0, 0, 1));
  // sphere: p / |p|
  e = enter(MSSIM_SHAPE_SPHERE, {0.5f}, mk(0, 0, 2), mk(0, 0, -1));
  CHECK(close(e.t, 1.5f) && close3(e.n, 0, 0, 1));
  e = enter(MSSIM_SHAPE_SPHERE, {0.5f}, mk(0.3f, 0, 2), mk(0, 0, -1));
  CHECK(close(e.t, 1.6f, 1e-5f) && close3(e.n, 0.6f, 0, 0.8f, 1e-5f));
  // cylinder r 0.2, half length 0.4 about x: the cap, then the side
  e = enter(MSSIM_SHAPE_CYLINDER, {0.2f, 0.4f}, mk(2, 0.05f, 0.05f), mk(-1, 0, 0));
  CHECK(close(e.t, 1.6f) && close3(e.n, 1, 0, 0));
  e = enter(MSSIM_SHAPE_CYLINDER, {0.2f, 0.4f}, mk(-2, 0.05f, 0.05f), mk(1, 0, 0));
  CHECK(close(e.t, 1.6f) && close3(e.n, -1, 0, 0));
  e = enter(MSSIM_SHAPE_CYLINDER, {0.2f, 0.4f}, mk(0.1f, 0.12f, 2), mk(0, 0, -1));
  CHECK(close(e.t, 1.84f, 1e-5f) && close3(e.n, 0, 0.6f, 0.8f, 1e-5f));
  // capsule r 0.2, half length 0.4: tube, the ball at -x, the ball at +x
  e = enter(MSSIM_SHAPE_CAPSULE, {0.2f, 0.4f}, mk(0.1f, 0, 2), mk(0, 0, -1));
  CHECK(close(e.t, 1.8f) && close3(e.n, 0, 0, 1));
  e = enter(MSSIM_SHAPE_CAPSULE, {0.2f, 0.4f}, mk(-2, 0, 0), mk(1, 0, 0));
  CHECK(close(e.t, 1.4f) && close3(e.n, -1, 0, 0));
  e = enter(MSSIM_SHAPE_CAPSULE, {0.2f, 0.4f}, mk(0.52f, 0, 2), mk(0, 0, -1));
  CHECK(close(e.t, 1.84f, 1e-5f) && close3(e.n, 0.6f, 0, 0.8f, 1e-5f));
  // a hull made of a box's six planes gives the box's entry and normal, ray for ray
  const std::vector<float> planes = {1, 0, 0, 0.3f, -1, 0, 0, 0.3f, 0, 1, 0, 0.2f, 0, -1, 0, 0.2f, 0, 0, 1, 0.1f, 0, 0, -1, 0.1f};
  for (int k = 0; k < 40; k++) {
    const float a = 0.7f * k, b = 0.37f * k + 0.2f;
    const v3 o = mk(2.f * std::cos(a) * std::cos(b), 2.f * std::sin(a) * std::cos(b), 2.f * std::sin(b));
    const v3 d = mk(-o.x + 0.05f * std::sin(3.f * k), -o.y + 0.04f * std::cos(5.f * k), -o.z + 0.03f);
    const Entry bx = enter(MSSIM_SHAPE_BOX, {0.3f, 0.2f, 0.1f}, o, d), hl = enter(MSSIM_SHAPE_CONVEX, {}, o, d, planes);
    CHECK(std::isfinite(bx.t) && close(bx.t, hl.t) && close3(hl.n, bx.n.x, bx.n.y, bx.n.z));
  }
  // two planes that set tin at the same parameter: the first in index order keeps it
  const std::vector<float> wedge = {0, 0, 1, 0.5f, 0, 0, 1, 0.5f, 1, 0, 0, 1, -1, 0, 0, 1, 0, 1, 0, 1, 0, -1, 0, 1, 0, 0, -1, 1};
  e = enter(MSSIM_SHAPE_CONVEX, {}, mk(0, 0, 2), mk(0, 0, -1), wedge);
  CHECK(close(e.t, 1.5f) && close3(e.n, 0, 0, 1));
}

// one triangle in the plane z = 0.25 about its centroid, and one BVH node whose child 0 is that leaf
struct OneTriangle {
  const float soup[12] = {0.f, 0.f, 0.25f, 1.f, -0.5f, 0.f, -0.5f, 1.f, 0.f, -0.5f, -0.5f, 0.f};
  std::vector<float> node = std::vector<float>(112, 0.f);
  OneTriangle() {
    for (int c = 0; c < 16; c++) { node[6 * c] = 1.f; node[6 * c + 3] = -1.f; }  // min > max: no child
    const float box[6] = {-0.5f, -0.5f, 0.25f, 1.f, 1.f, 0.25f};
    for (int k = 0; k < 6; k++) node[k] = box[k];
    const int32_t leaf = ~0;
    std::memcpy(&node[96], &leaf, 4);
  }
};

void triangles() {
  // seen from above and from below the triangle turns its normal to the ray
  const OneTriangle m;
  rc::MeshLevel stack[MSSIM_RAYCAST_MESH_DEPTH];
  for (int s = -1; s <= 1; s += 2) {
    const v3 o = mk(0.1f, 0.1f, 0.25f + 2.f * s), d = mk(0, 0, -1.f * s);
    int tri = -1;
    const float t = rc::mesh_hit(m.node.data(), m.soup, 0, o, d, 0.01f, 30.f, rc::kInf, stack, 1, &tri);
    CHECK(close(t, 2.f) && tri == 0);
    CHECK(close3(rc::triangle_normal(m.soup, tri, d), 0, 0, (float)s));
  }
  int tri = -7;
  CHECK(std::isinf(rc::mesh_hit(m.node.data(), m.soup, 0, mk(3, 3, 2), mk(0, 0, -1), 0.01f, 30.f, rc::kInf, stack, 1, &tri)) && tri == -7);
}

void light_and_colour() {
  // a camera at the env's origin looking along env +x (identity pose, SAPIEN axes): OpenCV x = -env y, y = -env z, z = env x
  float L[6];
  rc::lights(rc::xf{rc::p3{0, 0, 0}, rc::q4{1, 0, 0, 0}}, L);
  const float s = 1.f / std::sqrt(3.f);
  CHECK(close(L[0], -s) && close(L[1], s) && close(L[2], s) && close(L[3], 0) && close(L[4], 1) && close(L[5], 0));
  // the six faces of an axis-aligned box under the two lights, from the two direction vectors: with n = +-e_k the first
  // light gives max(0, -+l_k) = 1/sqrt 3 on -x, -y, +z, the second 1 on +z
  struct { float n[3]; float k; } faces[6] = {{{1, 0, 0}, 0.3f}, {{-1, 0, 0}, 0.3f + s}, {{0, 1, 0}, 0.3f}, {{0, -1, 0}, 0.3f + s}, {{0, 0, 1}, 1.f}, {{0, 0, -1}, 0.3f}};
  for (auto& f : faces) {
    const v3 n_cv = mk(-f.n[1], -f.n[2], f.n[0]);
    const unsigned px = rc::shade(n_cv, mk(1.f, 0.5f, 0.25f), L);
    CHECK(byte_of(px, 3) == 255u);
    CHECK(byte_of(px, 0) == (unsigned)std::floor(255.0 * f.k + 0.5) && byte_of(px, 1) == (unsigned)std::floor(255.0 * 0.5 * f.k + 0.5) &&
          byte_of(px, 2) == (unsigned)std::floor(255.0 * 0.25 * f.k + 0.5));
  }
  // an albedo above 1 saturates, it does not wrap
  CHECK(byte_of(rc::shade(mk(0, -1, 0), mk(3.f, 1.f, 0.f), L), 0) == 255u && byte_of(rc::shade(mk(0, -1, 0), mk(3.f, 1.f, 0.f), L), 2) == 0u);
  // a rotated camera: the rotated lights against a normal rotated the same way give the same byte
  const rc::q4 q = rc::qnorm(rc::q4{0.7, 0.2, -0.5, 0.3});
  float Lr[6];
  rc::lights(rc::xf{rc::p3{1, 2, 3}, q}, Lr);
  const rc::p3 up = rc::qrot(rc::qconj(q), rc::p3{0, 0, 1});  // env +z in the camera's SAPIEN axes
  CHECK(rc::shade(mk((float)-up.y, (float)-up.z, (float)up.x), mk(1, 1, 1), Lr) == (0xffffffffu));
  // checker: 1 m cells on the ground (the plane's frame: x is the normal), 0.8 where the cell sum is odd; a point a rounding
  // above or below the plane is in the same cell
  const float c[4] = {1.f, 0.5f, 0.25f, 1.f};
  CHECK(rc::albedo(c, mk(1e-7f, 0.5f, 0.5f), MSSIM_SHAPE_PLANE).x == 1.f && rc::albedo(c, mk(-1e-7f, 0.5f, 0.5f), MSSIM_SHAPE_PLANE).x == 1.f);
  CHECK(rc::albedo(c, mk(0.f, 1.5f, 0.5f), MSSIM_SHAPE_PLANE).x == 0.8f && rc::albedo(c, mk(0.f, 1.5f, 1.5f), MSSIM_SHAPE_PLANE).x == 1.f);
  CHECK(rc::albedo(c, mk(0.f, -0.5f, 0.5f), MSSIM_SHAPE_PLANE).y == 0.4f && rc::albedo(c, mk(0.f, -0.5f, -0.5f), MSSIM_SHAPE_PLANE).y == 0.5f);
  CHECK(rc::albedo(c, mk(0.5f, 0.5f, 0.5f), MSSIM_SHAPE_BOX).x == 1.f && rc::albedo(c, mk(-0.5f, 0.5f, 0.5f), MSSIM_SHAPE_BOX).x == 0.8f);
  const float plain[4] = {0.2f, 0.4f, 0.6f, 0.f};
  CHECK(rc::albedo(plain, mk(1.5f, 0.5f, 0.5f), MSSIM_SHAPE_BOX).z == 0.6f);
  CHECK(byte_of(rc::kBackground, 3) == 255u);
}

// rc::trace into a Lit over a staged list on the host: a hit in the first of two calls keeps its normal and colour while a
// second list (the next chunk) is walked, and a nearer shape of the second list replaces all three
void trace() {
  const rc::xf cam{rc::p3{0, 0, 0}, rc::q4{1, 0, 0, 0}};  // looks along env +x
  const float r[3] = {0.5f, 0, 0};
  const rc::Staged far_ball = rc::stage(cam, rc::xf{rc::p3{5, 0, 0}, rc::q4{1, 0, 0, 0}}, rc::p3{5, 0, 0}, 0.5f, MSSIM_SHAPE_SPHERE, r, 0, 0, 0);
  const rc::Staged near_ball = rc::stage(cam, rc::xf{rc::p3{3, 0, 0}, rc::q4{1, 0, 0, 0}}, rc::p3{3, 0, 0}, 0.5f, MSSIM_SHAPE_SPHERE, r, 0, 0, 0);
  const rc::Staged off_ball = rc::stage(cam, rc::xf{rc::p3{3, 4, 0}, rc::q4{1, 0, 0, 0}}, rc::p3{3, 4, 0}, 0.5f, MSSIM_SHAPE_SPHERE, r, 0, 0, 0);
  const float red[4] = {1, 0, 0, 0}, green[4] = {0, 1, 0, 0};
  rc::Lit hit{rc::kInf, mk(0, 0, 0), mk(0, 0, 0), red};
  rc::trace<false>(&far_ball, 1, nullptr, 0.f, 0.f, 0.01f, 30.f, true, &hit);
  CHECK(close(hit.t, 4.5f) && close3(hit.n, 0, 0, -1) && hit.a.x == 1.f && hit.a.y == 0.f);
  hit.col = green;
  rc::trace<false>(&off_ball, 1, nullptr, 0.f, 0.f, 0.01f, 30.f, true, &hit);  // missed: everything kept
  CHECK(close(hit.t, 4.5f) && close3(hit.n, 0, 0, -1) && hit.a.x == 1.f && hit.a.y == 0.f);
  rc::trace<false>(&near_ball, 1, nullptr, 0.f, 0.f, 0.01f, 30.f, true, &hit);
  CHECK(close(hit.t, 2.5f) && close3(hit.n, 0, 0, -1) && hit.a.x == 0.f && hit.a.y == 1.f);
  hit.col = red;
  rc::trace<false>(&far_ball, 1, nullptr, 0.f, 0.f, 0.01f, 30.f, true, &hit);  // farther: everything kept
  CHECK(close(hit.t, 2.5f) && hit.a.y == 1.f);
}

// The shaded view and the depth image agree on what is in front, bit for bit: one staged list walked twice by rc::trace,
// once into the depth kernel's record and once into the shaded view's, over a grid of rays. Returns how many rays hit
// each id (index 0: nothing).
template <bool MESH>
std::vector<int> walk_twice(const std::vector<rc::Staged>& list, const std::vector<float>& planes, const float* bvh, const float* soup) {
  const int n = (int)list.size();
  const std::vector<float> col(4 * list.size(), 0.5f);
  std::vector<int> seen(list.size() + 1, 0);
  rc::MeshLevel stack[MSSIM_RAYCAST_MESH_DEPTH];
  for (int v = 0; v < 41; v++)
    for (int u = 0; u < 41; u++) {
      const float xcv = 0.3f * (u - 20) / 20.f, ycv = 0.3f * (v - 20) / 20.f;
      rc::Hit hit{rc::kInf, 0};
      rc::Lit lit{rc::kInf, mk(0, 0, 0), mk(0, 0, 0), col.data()};
      rc::trace<MESH>(list.data(), n, planes.data(), xcv, ycv, 0.01f, 30.f, true, &hit, bvh, soup, stack, 1);
      rc::trace<MESH>(list.data(), n, planes.data(), xcv, ycv, 0.01f, 30.f, true, &lit, bvh, soup, stack, 1);
      CHECK(std::memcmp(&hit.t, &lit.t, 4) == 0);
      CHECK(std::isinf(hit.t) || close(rc::dot(lit.n, lit.n), 1.f, 1e-5f));
      seen[hit.seg]++;
    }
  return seen;
}

void one_walk() {
  const rc::xf cam{rc::p3{0, 0, 0}, rc::q4{1, 0, 0, 0}};  // looks along env +x
  auto at = [&](double x, double y, double z, rc::q4 q) { return rc::xf{rc::p3{x, y, z}, rc::qnorm(q)}; };
  auto staged = [&](rc::xf pose, float br, int type, std::vector<float> p, int seg, int pl0 = 0, int pln = 0) {
    p.resize(3);
    return rc::stage(cam, pose, pose.p, br, type, p.data(), seg, pl0, pln);
  };
  // a box, a capsule, a hull (a box's six planes) and a sphere, all tilted; the sphere stands in front of part of the box
  const std::vector<float> planes = {1, 0, 0, 0.3f, -1, 0, 0, 0.3f, 0, 1, 0, 0.2f, 0, -1, 0, 0.2f, 0, 0, 1, 0.1f, 0, 0, -1, 0.1f};
  const std::vector<rc::Staged> list = {
      staged(at(4.0, 0.6, 0.3, {0.9, 0.1, -0.3, 0.2}), 0.45f, MSSIM_SHAPE_BOX, {0.3f, 0.2f, 0.25f}, 1),
      staged(at(3.0, -0.5, -0.2, {0.8, -0.2, 0.4, 0.3}), 0.55f, MSSIM_SHAPE_CAPSULE, {0.15f, 0.4f}, 2),
      staged(at(5.0, 0.1, -0.6, {0.7, 0.5, 0.1, -0.4}), 0.38f, MSSIM_SHAPE_CONVEX, {}, 3, 0, 6),
      staged(at(3.5, 0.3, 0.25, {1, 0, 0, 0}), 0.2f, MSSIM_SHAPE_SPHERE, {0.2f}, 4),
  };
  const std::vector<int> seen = walk_twice<false>(list, planes, nullptr, nullptr);
  for (int k = 0; k <= 4; k++) CHECK(seen[k] > 10);  // every shape and the background are in the picture
  // the ray at the sphere's centre enters it at z-depth 3.5 (1 - r / |c|); the ray at the box's centre passes beside the
  // sphere; a ray between the two meets both, and the sphere is in front
  rc::Hit centre{rc::kInf, 0}, beside{rc::kInf, 0}, both{rc::kInf, 0}, box_alone{rc::kInf, 0};
  rc::trace<false>(list.data(), 4, planes.data(), -0.3f / 3.5f, -0.25f / 3.5f, 0.01f, 30.f, true, &centre);
  rc::trace<false>(list.data(), 4, planes.data(), -0.6f / 4.f, -0.3f / 4.f, 0.01f, 30.f, true, &beside);
  rc::trace<false>(list.data(), 4, planes.data(), -0.12f, -0.073f, 0.01f, 30.f, true, &both);
  rc::trace<false>(list.data(), 1, planes.data(), -0.12f, -0.073f, 0.01f, 30.f, true, &box_alone);
  CHECK(centre.seg == 4 && close(centre.t, 3.5f * (1.f - 0.2f / std::sqrt(12.4025f)), 1e-5f) && beside.seg == 1);
  CHECK(both.seg == 4 && box_alone.seg == 1 && both.t < box_alone.t && box_alone.t < 30.f);
  // the one-triangle mesh, turned to face the camera (its z along env -x), and a sphere in front of its middle
  const OneTriangle m;
  const std::vector<rc::Staged> with_mesh = {
      staged(at(4.0, 0.0, 0.0, {0.7071067811865476, 0, -0.7071067811865476, 0}), 2.f, MSSIM_SHAPE_TRIMESH, {}, 1, 0, 1),
      staged(at(3.0, 0.1, 0.1, {1, 0, 0, 0}), 0.2f, MSSIM_SHAPE_SPHERE, {0.2f}, 2),
  };
  const std::vector<int> seen_mesh = walk_twice<true>(with_mesh, {}, m.node.data(), m.soup);
  for (int k = 0; k <= 2; k++) CHECK(seen_mesh[k] > 10);
}

void refusals() {
  constexpr int S = 3, SLOTS = 2, N = 4;
  std::vector<float> rgba(4 * S, 0.5f), env(4 * SLOTS * N, 0.25f);
  std::string err;
  CHECK(mssim_shade::validate_colours(rgba.data(), S, nullptr, 0, N, &err) == 0);
  CHECK(mssim_shade::validate_colours(rgba.data(), S, nullptr, SLOTS, N, &err) == 0);
  CHECK(mssim_shade::validate_colours(rgba.data(), S, env.data(), SLOTS, N, &err) == 0);
  CHECK(mssim_shade::validate_colours(nullptr, 0, nullptr, 0, N, &err) == 0);
  CHECK(mssim_shade::validate_colours(nullptr, S, nullptr, 0, N, &err) == 1 && err.find("raycast_set_colours") == 0);
  CHECK(mssim_shade::validate_colours(rgba.data(), S, env.data(), 0, N, &err) == 3 && err.find("without per-env") != std::string::npos);
  const float bad[4] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -0.1f, -1e-30f};
  for (float b : bad)
    for (size_t at : {(size_t)0, (size_t)(4 * S - 1)}) {  // a colour of the first shape, the cell size of the last
      std::vector<float> c = rgba;
      c[at] = b;
      err.clear();
      CHECK(mssim_shade::validate_colours(c.data(), S, nullptr, 0, N, &err) == 2 && err.find("shape " + std::to_string(at / 4)) != std::string::npos);
    }
  std::vector<float> e2 = env;
  e2.back() = bad[0];
  CHECK(mssim_shade::validate_colours(rgba.data(), S, e2.data(), SLOTS, N, &err) == 2 && err.find("slot 1, env 3") != std::string::npos);
  CHECK(mssim_shade::validate_colours(rgba.data(), S, e2.data(), SLOTS, N, nullptr) == 2);  // (no message asked for)
  alignas(8) unsigned char out[16];
  CHECK(mssim_shade::validate_shade(true, out, &err) == 0 && mssim_shade::validate_shade(true, out + 4, &err) == 0);
  for (int k = 1; k < 4; k++) CHECK(mssim_shade::validate_shade(true, out + k, &err) == 1 && err.find("4-byte aligned") != std::string::npos);
  CHECK(mssim_shade::validate_shade(false, out, &err) == 3 && err.find("mssim_raycast_set_colours") != std::string::npos);
  CHECK(mssim_shade::validate_shade(true, nullptr, &err) == 1);
}

}  // namespace

int main() {
  normals();
  triangles();
  light_and_colour();
  trace();
  one_walk();
  refusals();
  if (g_failed) {
    std::printf("shade_check: %d checks failed\n", g_failed);
    return 1;
  }
  std::printf("shade_check: ok\n");
  return 0;
}
