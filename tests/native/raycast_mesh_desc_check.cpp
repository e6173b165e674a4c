// raycast_mesh_desc_check.cpp -- CPU check of maniskill_amd/csrc/mssim_raycast_desc.h for scenes with triangle meshes,
// per-env hulls and per-env ids: a valid scene with every table exactly as long as its counts say (a read past an end is
// an AddressSanitizer report), then one defect at a time -- a triangle range, a node reference, a child reference cycle,
// the depth bound, a per-env range in one env only, a per-env plane range --, each refused with its return code and
// message. Stand-alone (tests/test_raycast_mesh.py builds it with ASan + UBSan and expects exit status 0).
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../maniskill_amd/csrc/mssim_raycast_desc.h"

static int g_failed = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::printf("%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond);   \
      g_failed++;                                                            \
    }                                                                        \
  } while (0)

namespace {

constexpr int N = 3, ROWS = 4;
constexpr int NODES = MSSIM_RAYCAST_MESH_DEPTH + 3;  // node 0: a two-level mesh's root, node 1 its child; nodes 2..: a chain of DEPTH + 1

// Shapes: 0 a mesh (triangles 0..3 under node 0 -> node 1), 1 a per-env mesh slot (env 0 the shared mesh, env 1 its own:
// triangles 4..5 under node 2, env 2 nothing), 2 a per-env hull slot (planes 0..4, 5..9, nothing), 3 a sphere with
// per-env ids. Nodes 2 .. NODES-1 are a chain (node k's child 1 is node k + 1) that is cut after node 2 in the valid
// scene: linking it up gives a mesh of up to NODES - 2 = MSSIM_RAYCAST_MESH_DEPTH + 1 levels under node 2.
struct Scene {
  std::vector<int32_t> type{MSSIM_SHAPE_TRIMESH, MSSIM_SHAPE_TRIMESH, MSSIM_SHAPE_CONVEX, MSSIM_SHAPE_SPHERE};
  std::vector<int32_t> row{-1, 3, 0, 2};
  std::vector<float> frame, param, bound;
  std::vector<int16_t> seg{1, 2, 3, 4};
  std::vector<int32_t> planes2{0, 0, 0, 0, 0, 5, 0, 0};
  std::vector<float> planes;
  std::vector<int32_t> slot{-1, 0, 1, 2};
  std::vector<float> env_frame, env_param, env_bound;
  std::vector<float> soup, bvh;
  std::vector<int32_t> env_planes2;
  std::vector<int16_t> env_seg;
  mssim_raycast_scene d{};

  void set_child(int node, int c, int32_t ref) {
    float* b = &bvh[(size_t)node * 112 + 6 * c];
    b[0] = b[1] = b[2] = -1.f; b[3] = b[4] = b[5] = 1.f;
    std::memcpy(&bvh[(size_t)node * 112 + 96 + c], &ref, 4);
  }
  void clear_child(int node, int c) {
    float* b = &bvh[(size_t)node * 112 + 6 * c];
    b[0] = b[1] = b[2] = 1.f; b[3] = b[4] = b[5] = -1.f;
  }
  Scene() {
    for (int i = 0; i < 4; i++) {
      const float f[7] = {0.1f * i, 0, 0, 1, 0, 0, 0};
      frame.insert(frame.end(), f, f + 7);
      const float b[4] = {0, 0, 0, 2.f};
      bound.insert(bound.end(), b, b + 4);
    }
    param = {0, 4, 0, 0, /* shape 1: the same mesh */ 0, 4, 0, 0, 0, 0, 0, 0, 0.1f, 0, 0, 0};
    for (int k = 0; k < 10; k++) {
      const float pl[4] = {k % 5 == 0 ? 1.f : 0.f, k % 5 == 1 ? 1.f : 0.f, k % 5 >= 2 ? 1.f : 0.f, 0.1f};
      planes.insert(planes.end(), pl, pl + 4);
    }
    for (int t = 0; t < 6; t++) {
      const float q[12] = {0.1f * t, 0, 0, -0.1f, -0.1f, 0, 0.1f, -0.1f, 0, 0, 0.2f, 0};
      soup.insert(soup.end(), q, q + 12);
    }
    bvh.assign((size_t)NODES * 112, 0.f);
    for (int nd = 0; nd < NODES; nd++)
      for (int c = 0; c < 16; c++) clear_child(nd, c);
    set_child(0, 0, ~0); set_child(0, 1, 1); set_child(1, 0, ~1); set_child(1, 1, ~2); set_child(1, 15, ~3);
    for (int nd = 2; nd < NODES; nd++) set_child(nd, 0, nd % 2 ? ~5 : ~4);
    env_frame.assign(3 * 7 * N, 0.f);
    for (int s = 0; s < 3; s++)
      for (int e = 0; e < N; e++) env_frame[(s * 7 + 3) * N + e] = 1.f;
    env_param.assign(3 * 4 * N, 0.f);
    // slot 0: env 0 the shared mesh (type code 0), env 1 its own (first 4, count 2, root 2), env 2 nothing
    env_param[0 * N + 1] = 4.f; env_param[1 * N + 1] = 2.f; env_param[2 * N + 1] = 2.f;
    env_param[3 * N + 1] = (float)(MSSIM_SHAPE_TRIMESH + 1); env_param[3 * N + 2] = (float)(MSSIM_SHAPE_NONE + 1);
    // slot 1: hulls in envs 0 and 1, nothing in env 2
    env_param[(4 + 3) * N + 0] = (float)(MSSIM_SHAPE_CONVEX + 1); env_param[(4 + 3) * N + 1] = 0.f; env_param[(4 + 3) * N + 2] = (float)(MSSIM_SHAPE_NONE + 1);
    // slot 2: a sphere everywhere
    for (int e = 0; e < N; e++) { env_param[8 * N + e] = 0.1f; env_param[(8 + 3) * N + e] = (float)(MSSIM_SHAPE_SPHERE + 1); }
    env_bound.assign(3 * 4 * N, 0.1f);
    env_planes2.assign(3 * 2 * N, 0);
    env_planes2[(2 + 0) * N + 0] = 0; env_planes2[(2 + 1) * N + 0] = 5;   // slot 1, env 0: planes 0..4
    env_planes2[(2 + 0) * N + 1] = 5; env_planes2[(2 + 1) * N + 1] = 5;   // env 1: planes 5..9 (the last of the table)
    env_seg = {2, 2, 2, 3, 3, 3, 7, 8, 9};
    link();
  }
  void link() {
    d.n_shape = (int32_t)type.size();
    d.shape_type = type.data(); d.shape_row = row.data(); d.shape_frame = frame.data(); d.shape_param = param.data();
    d.shape_bound = bound.data(); d.shape_seg = seg.data(); d.shape_planes = planes2.data();
    d.n_plane = (int32_t)planes.size() / 4; d.planes = planes.data();
    d.n_env_shape = 3; d.shape_env_slot = slot.data();
    d.env_shape_frame = env_frame.data(); d.env_shape_param = env_param.data(); d.env_shape_bound = env_bound.data();
    d.n_tri = (int32_t)soup.size() / 12; d.tri_soup = soup.empty() ? nullptr : soup.data();
    d.n_tri_node = (int32_t)bvh.size() / 112; d.tri_bvh = bvh.empty() ? nullptr : bvh.data();
    d.env_shape_planes = env_planes2.empty() ? nullptr : env_planes2.data(); d.env_shape_seg = env_seg.empty() ? nullptr : env_seg.data();
  }
  // nodes 2 .. 2 + levels - 1 become one chain under node 2
  void chain(int levels) {
    for (int nd = 2; nd < 2 + levels - 1; nd++) set_child(nd, 1, nd + 1);
  }
};

mssim_camera_desc good_camera() {
  mssim_camera_desc c{};
  c.width = 32; c.height = 24; c.fx = c.fy = 20.f; c.cx = 16.f; c.cy = 12.f; c.near = 0.01f; c.far = 100.f; c.mount_row = -1;
  c.pose[3] = 1.f;
  return c;
}

int verdict(const Scene& s, std::string* err) {
  const mssim_camera_desc cam = good_camera();
  return mssim_raycast::validate(&s.d, &cam, 1, N, ROWS, err);
}

template <class Break>
void accepted(Break brk) {
  Scene s;
  brk(s);
  s.link();
  std::string err = "untouched";
  const int got = verdict(s, &err);
  if (got != 0) std::printf("expected acceptance, got rc %d: %s\n", got, err.c_str());
  CHECK(got == 0);
  CHECK(err == "untouched");
}

template <class Break>
void refused(int rc, const char* word, Break brk) {
  Scene s;
  brk(s);
  s.link();
  std::string err;
  const int got = verdict(s, &err);
  if (got != rc || err.find(word) == std::string::npos) std::printf("expected rc %d with '%s', got rc %d: %s\n", rc, word, got, err.c_str());
  CHECK(got == rc);
  CHECK(err.find("raycast_create: ") == 0);
  CHECK(err.find(word) != std::string::npos);
}

}  // namespace

int main() {
  accepted([](Scene&) {});
  accepted([](Scene& s) { s.chain(MSSIM_RAYCAST_MESH_DEPTH); });  // exactly as deep as the stack
  // the optional tables may be absent: the hull slot then renders its shared range, the ids are the shared ones
  accepted([](Scene& s) { s.env_planes2.clear(); s.env_seg.clear(); });
  // ---- a triangle range
  refused(2, "triangle range", [](Scene& s) { s.param[1] = 7.f; });             // shared: count past the soup
  refused(2, "triangle range", [](Scene& s) { s.param[0] = -1.f; });
  refused(2, "triangle range", [](Scene& s) { s.param[0] = 0.5f; });            // not an integer
  refused(2, "root node", [](Scene& s) { s.param[2] = (float)NODES; });
  // ---- a node reference
  refused(2, "child reference", [](Scene& s) { s.set_child(1, 2, NODES); });    // a node past the table
  refused(2, "child reference", [](Scene& s) { s.set_child(1, 2, ~6); });       // a triangle past the soup
  refused(2, "child reference", [](Scene& s) { s.set_child(NODES - 1, 3, ~6); });  // in a node no shape names: still refused (the table is uploaded whole)
  // ---- a child reference cycle
  refused(2, "cycle", [](Scene& s) { s.set_child(1, 2, 0); });                  // node 1 back to its parent
  refused(2, "cycle", [](Scene& s) { s.set_child(1, 2, 1); });                  // to itself
  refused(2, "cycle", [](Scene& s) { s.chain(NODES - 2); s.set_child(NODES - 1, 1, 2); });  // a long one
  // ---- the depth bound: one level more than the stack holds, under a root that a shape (env 1 of slot 0) names
  refused(3, "levels deep", [](Scene& s) { s.chain(MSSIM_RAYCAST_MESH_DEPTH + 1); });
  accepted([](Scene& s) { s.chain(MSSIM_RAYCAST_MESH_DEPTH + 1); s.env_param[2 * N + 1] = 3.f; });  // (the same chain entered one node down)
  // ---- a per-env range in one env only
  refused(2, "in env 1: triangle range", [](Scene& s) { s.env_param[1 * N + 1] = 3.f; });   // triangles 4..6 of 6
  refused(2, "in env 1: triangle range", [](Scene& s) { s.env_param[2 * N + 1] = (float)NODES; });
  accepted([](Scene& s) { s.env_param[1 * N + 2] = 99.f; s.env_param[2 * N + 0] = 99.f; });  // envs that do not read the rows (NONE, shared)
  // ---- a per-env plane range
  refused(2, "in env 1: per-env plane range", [](Scene& s) { s.env_planes2[(2 + 1) * N + 1] = 6; });   // one past the table
  refused(2, "in env 0: per-env plane range", [](Scene& s) { s.env_planes2[(2 + 0) * N + 0] = -1; });
  refused(2, "in env 0: per-env plane range", [](Scene& s) { s.env_planes2[(2 + 1) * N + 0] = 3; });   // fewer than a tetrahedron's
  accepted([](Scene& s) { s.env_planes2[(2 + 1) * N + 2] = 99; });                                      // env 2 has nothing in the slot
  // ---- what stays refused
  refused(3, "triangle mesh", [](Scene& s) { s.soup.clear(); s.bvh.clear(); });                          // a mesh shape, no triangle table
  refused(3, "triangle mesh", [](Scene& s) { s.env_param[(8 + 3) * N + 1] = (float)(MSSIM_SHAPE_TRIMESH + 1); });   // in a sphere's slot
  refused(3, "per-env hulls", [](Scene& s) { s.env_param[(8 + 3) * N + 1] = (float)(MSSIM_SHAPE_CONVEX + 1); });
  refused(1, "not finite", [](Scene& s) { s.soup[13] = std::numeric_limits<float>::quiet_NaN(); });
  {  // counts without tables
    Scene s;
    s.d.tri_bvh = nullptr;
    std::string err;
    CHECK(verdict(s, &err) == 1 && err.find("triangle table is missing") != std::string::npos);
  }
  if (g_failed) {
    std::printf("raycast_mesh_desc_check: %d failed\n", g_failed);
    return 1;
  }
  std::printf("raycast_mesh_desc_check: ok\n");
  return 0;
}
