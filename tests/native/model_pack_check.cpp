// model_pack_check.cpp -- CPU check of maniskill_amd/csrc/mssim_model_pack.h: every rejection mssim_create documents (by
// return code and message) and the layout of the tables it packs, on the smallest hand-written models that reach each
// branch. Stand-alone (tests/test_model_pack.py builds it with ASan + UBSan and expects exit status 0).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../maniskill_amd/csrc/mssim_model_pack.h"

static int g_failed = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::printf("%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond);   \
      g_failed++;                                                            \
    }                                                                        \
  } while (0)

using VI = std::vector<int32_t>;
using VF = std::vector<float>;
template <class T, class U>
static void push(std::vector<T>& v, std::initializer_list<U> x) { for (U a : x) v.push_back((T)a); }

// a model description whose arrays live in vectors; desc() points an mssim_model_desc at them
struct Model {
  VI dof_parent, dof_type, body_gravity, free_gravity, shape_type, shape_kind, shape_index, shape_row, shape_hull, pair_shape, shape_env_slot, free_env_slot;
  VF dof_frame, dof_axis, dof_limit, dof_drive, dof_armature, body_inertial, free_inertial, free_damping;
  VF shape_frame, shape_param, shape_material, shape_bound, hull_verts, env_shape_frame, env_shape_param, env_shape_bound, env_free_inertial, tri_soup, tri_bvh;
  int n_kin = 0, num_envs = 0, n_env_shape = 0, n_env_free = 0, abi = MSSIM_ABI_VERSION;

  int add_shape(int type, int kind, int index, float p0 = 0, float p1 = 0, float p2 = 0, int hull_start = 0, int hull_count = 0) {
    push(shape_type, {type}); push(shape_kind, {kind}); push(shape_index, {index}); push(shape_row, {-1});
    push(shape_frame, {0, 0, 0, 1, 0, 0, 0}); push(shape_param, {p0, p1, p2, 0.f}); push(shape_material, {0.5f, 0.5f, 0.f, 0.f});
    push(shape_bound, {0, 0, 0, 1}); push(shape_hull, {hull_start, hull_count}); push(shape_env_slot, {-1});
    return (int)shape_type.size() - 1;
  }
  void add_free() {
    push(free_inertial, {1, 0, 0, 0, 1, 1, 1, 0, 0, 0}); push(free_damping, {0, 0}); push(free_gravity, {1}); push(free_env_slot, {-1});
  }
  void add_joint(int parent, int type) {
    push(dof_parent, {parent}); push(dof_type, {type}); push(body_gravity, {0}); push(dof_frame, {0.f, 0.f, 0.1f, 1.f, 0.f, 0.f, 0.f}); push(dof_axis, {0, 0, 1});
    push(dof_limit, {-1, 1}); push(dof_drive, {100, 10, 50, 0}); push(dof_armature, {0.01f}); push(body_inertial, {1, 0, 0, 0, 1, 1, 1, 0, 0, 0});
  }
  void add_pair(int a, int b) { push(pair_shape, {a, b}); }
  mssim_model_desc desc() const {
    mssim_model_desc d;
    std::memset(&d, 0, sizeof d);
    d.abi_version = abi;
    d.n_dof = (int)dof_parent.size(); d.dof_parent = dof_parent.data(); d.dof_type = dof_type.data(); d.dof_frame = dof_frame.data(); d.dof_axis = dof_axis.data();
    d.dof_limit = dof_limit.data(); d.dof_drive = dof_drive.data(); d.dof_armature = dof_armature.data(); d.body_inertial = body_inertial.data(); d.body_gravity = body_gravity.data();
    d.n_free = (int)free_gravity.size(); d.free_inertial = free_inertial.data(); d.free_damping = free_damping.data(); d.free_gravity = free_gravity.data();
    d.n_kin = n_kin;
    d.n_shape = (int)shape_type.size(); d.shape_type = shape_type.data(); d.shape_body_kind = shape_kind.data(); d.shape_body_index = shape_index.data(); d.shape_row = shape_row.data();
    d.shape_frame = shape_frame.data(); d.shape_param = shape_param.data(); d.shape_material = shape_material.data(); d.shape_hull = shape_hull.data(); d.shape_bound = shape_bound.data();
    d.n_hull_verts = (int)hull_verts.size() / 3; d.hull_verts = hull_verts.data();
    d.n_pair = (int)pair_shape.size() / 2; d.pair_shape = pair_shape.data();
    d.num_envs = num_envs; d.n_env_shape = n_env_shape; d.shape_env_slot = shape_env_slot.data(); d.env_shape_frame = env_shape_frame.data();
    d.env_shape_param = env_shape_param.data(); d.env_shape_bound = env_shape_bound.data();
    d.n_env_free = n_env_free; d.free_env_slot = free_env_slot.data(); d.env_free_inertial = env_free_inertial.data();
    d.n_tri = (int)tri_soup.size() / 12; d.tri_soup = tri_soup.data(); d.n_tri_node = (int)tri_bvh.size() / 112; d.tri_bvh = tri_bvh.data();
    return d;
  }
};

// a fixed plane, and a box and a 5-vertex hull on one free body; pairs (plane, box), (plane, hull). The hull is vertices
// 2..6 of a 7-vertex table. Shapes: 0 plane, 1 box, 2 hull
static Model base_model() {
  Model m;
  m.add_free();
  push(m.hull_verts, {9.f, 9.f, 9.f, 8.f, 8.f, 8.f,                                        // (vertices 0, 1: of no hull)
                      0.1f, 0.2f, -0.05f, -0.1f, 0.2f, -0.05f, 0.f, -0.3f, -0.05f, 0.f, 0.f, 0.4f, 0.05f, 0.05f, -0.06f});
  m.add_shape(MSSIM_SHAPE_PLANE, MSSIM_BODY_WORLD, 0);
  m.add_shape(MSSIM_SHAPE_BOX, MSSIM_BODY_FREE, 0, 0.1f, 0.2f, 0.3f);
  m.add_shape(MSSIM_SHAPE_CONVEX, MSSIM_BODY_FREE, 0, 0, 0, 0, 2, 5);
  m.add_pair(0, 1);
  m.add_pair(0, 2);
  return m;
}
// the same with the hull in per-env slot 0 at N = 3: env 0 the shared hull, env 1 the hull of vertices 0..3, env 2 no shape
static Model per_env_model() {
  Model m = base_model();
  const int N = 3;
  m.num_envs = N; m.n_env_shape = 1; m.shape_env_slot[2] = 0;
  m.env_shape_frame.assign(7 * N, 0.f);
  for (int e = 0; e < N; e++) m.env_shape_frame[3 * N + e] = 1.f;  // identity frames
  m.env_shape_bound.assign(4 * N, 0.f);
  for (int e = 0; e < N; e++) m.env_shape_bound[3 * N + e] = 1.f;
  m.env_shape_param = {2, 0, 0,                                                   // first vertex
                       5, 4, 0,                                                   // vertex count
                       0, 0, 0,
                       0, MSSIM_SHAPE_CONVEX + 1, MSSIM_SHAPE_NONE + 1};          // type + 1, 0 = shared
  return m;
}
// a 2-triangle mesh with a one-node BVH on a kinematic body, a sphere on a free body, the pair (sphere, mesh). Shapes: 0 sphere, 1 mesh
static Model mesh_model() {
  Model m;
  m.add_free();
  m.n_kin = 1;
  m.tri_soup = {1.f, 1.f, 0.f, -1.f, -1.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.5f,         // corners (0,0,0) (2,1,0) (1,2,.5)
                -1.f, 0.f, 0.f, -1.f, 0.f, 0.f, 1.f, -1.f, 0.f, 0.f, 1.f, 0.f};       // corners (-2,0,0) (0,-1,0) (-1,1,0)
  m.tri_bvh.assign(112, 0.f);
  for (int c = 0; c < 16; c++) { m.tri_bvh[6 * c] = 1.f; m.tri_bvh[6 * c + 3] = -1.f; }  // min > max: no child
  const float boxes[2][6] = {{0, 0, 0, 2, 2, 0.5f}, {-2, -1, 0, 0, 1, 0}};
  for (int c = 0; c < 2; c++) {
    std::memcpy(&m.tri_bvh[6 * c], boxes[c], sizeof boxes[c]);
    const int32_t ref = ~c;
    std::memcpy(&m.tri_bvh[96 + c], &ref, 4);
  }
  m.add_shape(MSSIM_SHAPE_SPHERE, MSSIM_BODY_FREE, 0, 0.05f);
  m.add_shape(MSSIM_SHAPE_TRIMESH, MSSIM_BODY_KIN, 0, /* first triangle */ 0, /* count */ 2, 0, /* root node */ 0, 0);
  m.add_pair(0, 1);
  return m;
}
// a 9-joint chain with the Panda's parents and types, and n_free free bodies
static Model panda_chain(int n_free) {
  Model m;
  for (int j = 0; j < 9; j++) m.add_joint(kPandaParent[j], kPandaType[j]);
  for (int b = 0; b < n_free; b++) m.add_free();
  return m;
}

static void expect_reject(const char* what, const Model& m, int num_envs, int rc_want, const char* msg_part) {
  const mssim_model_desc d = m.desc();
  std::string err;
  const int rc = validate_model(&d, num_envs, &err);
  if (rc != rc_want || err.find(msg_part) == std::string::npos) {
    std::printf("%s: rc %d (want %d), message \"%s\" (want \"%s\" in it)\n", what, rc, rc_want, err.c_str(), msg_part);
    g_failed++;
  }
}
static PackedModel expect_pack(const char* what, const Model& m, int num_envs) {
  const mssim_model_desc d = m.desc();
  std::string err;
  PackedModel P;
  int rc = validate_model(&d, num_envs, &err);
  if (!rc) rc = pack_model(&d, num_envs, &P, &err);
  if (rc) {
    std::printf("%s: a good model was turned down, rc %d: %s\n", what, rc, err.c_str());
    g_failed++;
  }
  return P;
}
static int32_t bits(float f) { int32_t v; std::memcpy(&v, &f, 4); return v; }
static bool close(float a, float b) { return std::fabs(a - b) <= 1e-6f; }

static void check_rejections() {
  { Model m = base_model(); m.abi = 99; expect_reject("ABI", m, 4, 2, "ABI version mismatch"); }
  { std::string err; CHECK(validate_model(nullptr, 4, &err) == 1 && err == "bad arguments"); }
  expect_reject("num_envs = 0", base_model(), 0, 1, "bad arguments");
  expect_reject("num_envs < 0", base_model(), -3, 1, "bad arguments");
  { Model m = base_model(); for (int b = 1; b < 7; b++) m.add_free(); expect_reject("7 free bodies", m, 4, 9, "7 free bodies (max 6)"); }
  { Model m; for (int j = 0; j < 17; j++) m.add_joint(j - 1, 0); expect_reject("17 joints", m, 4, 3, "MSSIM_MAX_DOF"); }
  { Model m = base_model(); while (m.pair_shape.size() < 2 * 897) m.add_pair(0, 1); expect_reject("897 pairs", m, 4, 9, "897 candidate pairs (max 896)"); }
  { Model m = base_model(); while (m.pair_shape.size() < 2 * 896) m.add_pair(0, 1); expect_pack("896 pairs", m, 4); }
  { Model m = panda_chain(1); m.dof_parent[3] = 5; expect_reject("unsorted dof_parent", m, 4, 4, "topologically sorted"); }
  { Model m = base_model(); m.pair_shape[1] = 99; expect_reject("pair names shape 99", m, 4, 4, "pair_shape names a shape that does not exist"); }
  { Model m = base_model(); m.pair_shape[2] = -1; expect_reject("pair names shape -1", m, 4, 4, "pair_shape"); }
  { Model m = base_model(); m.shape_hull[5] = 3; expect_reject("hull of 3 vertices", m, 4, 5, "convex hull vertex count out of range"); }
  { Model m = base_model(); m.shape_hull[5] = MSSIM_MAX_HULL_VERTS + 1; expect_reject("hull of 65 vertices", m, 4, 5, "convex hull vertex count out of range"); }
  { Model m = base_model(); m.shape_hull[4] = 3; expect_reject("hull range past hull_verts", m, 4, 5, "vertex range outside hull_verts"); }
  { Model m = base_model(); m.shape_hull[4] = -1; expect_reject("hull range before hull_verts", m, 4, 5, "vertex range outside hull_verts"); }
  { Model m = per_env_model(); m.env_shape_param[1 * 3 + 2] = 99.f; m.env_shape_param[3 * 3 + 2] = 0.f; expect_reject("per-env hull count 99", m, 3, 8, "per-env hull reference out of range"); }
  { Model m = per_env_model(); m.env_shape_param[3 * 3 + 1] = MSSIM_SHAPE_PLANE + 1; expect_reject("per-env plane", m, 3, 8, "planes cannot be per-env shapes"); }
  { Model m = per_env_model(); m.env_shape_param[3 * 3 + 1] = MSSIM_SHAPE_TRIMESH + 1; expect_reject("per-env mesh in a hull slot", m, 3, 8, "a triangle mesh only in a slot that is a triangle mesh"); }
  { Model m = per_env_model(); m.shape_env_slot[2] = 77; expect_reject("shape_env_slot 77", m, 3, 5, "shape_env_slot names a slot beyond n_env_shape"); }
  {
    Model m = per_env_model();
    m.n_env_free = 1; m.free_env_slot[0] = 5; m.env_free_inertial.assign(10 * 3, 1.f);
    expect_reject("free_env_slot 5", m, 3, 5, "free_env_slot names a slot beyond n_env_free");
    m.free_env_slot[0] = 0;
    expect_pack("free_env_slot 0", m, 3);
  }
  { Model m = mesh_model(); const int32_t ref = ~2; std::memcpy(&m.tri_bvh[96 + 1], &ref, 4); expect_reject("BVH leaf outside tri_soup", m, 2, 5, "tri_bvh: a child reference points outside"); }
  { Model m = mesh_model(); const int32_t ref = 1; std::memcpy(&m.tri_bvh[96 + 1], &ref, 4); expect_reject("BVH child outside the nodes", m, 2, 5, "tri_bvh: a child reference points outside"); }
  { Model m = mesh_model(); m.shape_kind[1] = MSSIM_BODY_FREE; expect_reject("mesh on a free body", m, 2, 8, "the mesh belongs to a moving body"); }
  { Model m = mesh_model(); m.shape_hull[2] = 1; expect_reject("mesh root outside the nodes", m, 2, 8, "BVH root out of range"); }
  { Model m = mesh_model(); m.shape_param[4 + 1] = 3.f; expect_reject("triangle range past tri_soup", m, 2, 8, "triangle range out of tri_soup"); }
  expect_reject("per-env arrays of another num_envs", per_env_model(), 4, 7, "per-env arrays were built for a different num_envs");
}

static void check_hulls_and_shapes() {
  // shapes 2, 3 share the hull (2, 5); shape 4 has its own (0, 4). The box sits off its bound centre, in a frame turned by
  // 90 degrees about z and given as a quaternion of length 2
  Model m = base_model();
  const float frame[7] = {1.f, 2.f, 3.f, std::sqrt(2.f), 0.f, 0.f, std::sqrt(2.f)}, bound[4] = {0.01f, -0.02f, 0.03f, 0.5f};
  std::copy(frame, frame + 7, &m.shape_frame[7 * 1]);
  std::copy(bound, bound + 4, &m.shape_bound[4 * 1]);
  m.add_shape(MSSIM_SHAPE_CONVEX, MSSIM_BODY_FREE, 0, 0, 0, 0, 2, 5);
  m.add_shape(MSSIM_SHAPE_CONVEX, MSSIM_BODY_FREE, 0, 0, 0, 0, 0, 4);
  const PackedModel P = expect_pack("hulls", m, 4);
  CHECK(P.shape_hull.size() == 2 * 5 && P.hull_verts.size() == 3 * 16);
  CHECK(P.shape_hull[0] == 0 && P.shape_hull[1] == 0 && P.shape_hull[3] == 0);  // plane, box: no hull
  CHECK(P.shape_hull[2 * 2] == P.shape_hull[2 * 3] && P.shape_hull[2 * 2 + 1] == 5 && P.shape_hull[2 * 3 + 1] == 5);
  CHECK(P.shape_hull[2 * 4] != P.shape_hull[2 * 2] && P.shape_hull[2 * 4 + 1] == 4);
  for (int s = 2; s < 5 && P.shape_hull.size() == 10 && P.hull_verts.size() == 48; s++) {
    const int st = P.shape_hull[2 * s], cnt = P.shape_hull[2 * s + 1], src = m.shape_hull[2 * s];
    CHECK(st % 8 == 0 && st >= 0 && st + 8 <= 16);
    for (int i = 0; i < 8; i++)
      for (int k = 0; k < 3; k++) CHECK(P.hull_verts[3 * (st + i) + k] == m.hull_verts[3 * (src + (i < cnt ? i : 0)) + k]);
  }
  // box: half extents = its parameters + |bound offset|; centre = frame position + R * offset (x -> y, y -> -x)
  CHECK(P.shape_half.size() == 15 && P.shape_center.size() == 15 && P.shape_pack.size() == 24 * 5);
  CHECK(P.shape_half[3] == 0.1f + 0.01f && P.shape_half[4] == 0.2f + 0.02f && P.shape_half[5] == 0.3f + 0.03f);
  CHECK(close(P.shape_center[3], 1.f + 0.02f) && close(P.shape_center[4], 2.f + 0.01f) && close(P.shape_center[5], 3.f + 0.03f));
  CHECK(P.shape_half[0] == 3e30f);  // plane
  // hull: extents of its vertices about the bound centre
  CHECK(P.shape_half[6] == 0.1f && P.shape_half[7] == 0.3f && P.shape_half[8] == 0.4f);
  const float* r = &P.shape_pack[24 * 1];
  CHECK(std::equal(frame, frame + 7, r) && r[7] == 0.1f && r[8] == 0.2f && r[9] == 0.3f && r[13] == 0.5f && r[17] == 0.5f);
  CHECK(std::equal(&P.shape_center[3], &P.shape_center[6], r + 10) && std::equal(&P.shape_half[3], &P.shape_half[6], r + 14));
  CHECK(bits(r[18]) == MSSIM_SHAPE_BOX && bits(r[19]) == MSSIM_BODY_FREE && bits(r[20]) == 0 && bits(r[21]) == -1);
  // no per-env arrays: every slot shared; no mesh
  CHECK(P.shape_env_slot == VI(5, -1) && P.free_env_slot == VI(1, -1) && P.env_shape_param.empty());
  CHECK(!P.has_tri && !P.panda && P.rows_per_env == 1 && P.n_mesh_pair == 0 && P.pair_mesh_slot == VI(2, -1));
  // pair table: 128 words per started chunk + 128, -1 behind the last pair
  CHECK(P.pair_packed.size() == 256 && P.pair_packed[0] == (0 | 1 << 8) && P.pair_packed[1] == (0 | 2 << 8));
  for (size_t i = 2; i < P.pair_packed.size(); i++) CHECK(P.pair_packed[i] == -1);
  while (m.pair_shape.size() < 2 * 129) m.add_pair(0, 4);
  const PackedModel Q = expect_pack("129 pairs", m, 4);
  CHECK(Q.pair_packed.size() == 256 + 128 && Q.pair_packed[128] == (0 | 4 << 8) && Q.pair_packed[129] == -1 && Q.pair_packed.back() == -1);
  m.pair_shape.resize(2 * 128);
  CHECK(expect_pack("128 pairs", m, 4).pair_packed.size() == 256);
}

static void check_per_env_rows() {
  const Model m = per_env_model();
  const int N = 3;
  const PackedModel P = expect_pack("per-env hull", m, N);
  CHECK(P.env_shape_param.size() == 4 * N && P.hull_verts.size() == 3 * 16);
  CHECK(P.shape_env_slot == (VI{-1, -1, 0}) && P.free_env_slot == VI(1, -1));
  if (P.env_shape_param.size() != 4 * N || P.shape_hull.size() != 6) return;
  // env 0: the shared hull, through the range the shared shape already has; env 1: a hull of its own; env 2: nothing
  const int st0 = P.shape_hull[2 * 2], st1 = 8 - st0;
  CHECK(st0 == 0);
  CHECK(bits(P.env_shape_param[0]) == (MSSIM_SHAPE_CONVEX | 5 << 3 | st0 << 10));
  CHECK(bits(P.env_shape_param[1]) == (MSSIM_SHAPE_CONVEX | 4 << 3 | st1 << 10));
  CHECK(bits(P.env_shape_param[2]) == MSSIM_SHAPE_NONE);
  for (int k = 0; k < 3; k++) CHECK(P.hull_verts[3 * st1 + k] == 9.f && P.hull_verts[3 * (st1 + 4) + k] == 9.f && P.hull_verts[3 * (st1 + 1) + k] == 8.f);
  // rows 1..3: half extents of the hull about its bound centre (here the shape frame's origin)
  const float want[3][3] = {{0.1f, 0.3f, 0.4f}, {9.f, 9.f, 9.f}, {0.f, 0.f, 0.f}};
  for (int e = 0; e < N; e++)
    for (int k = 0; k < 3; k++) CHECK(P.env_shape_param[(1 + k) * N + e] == want[e][k]);
  CHECK(bits(P.shape_pack[24 * 2 + 21]) == 0 && bits(P.shape_pack[24 * 1 + 21]) == -1);  // env slot of the hull / of the box
  // a bound centre off the frame origin, in a frame turned by 90 degrees about z: x extent about -0.05 - (centre y in the shape frame)
  Model t = per_env_model();
  for (int e = 0; e < N; e++) { t.env_shape_frame[3 * N + e] = t.env_shape_frame[6 * N + e] = std::sqrt(0.5f); t.env_shape_frame[0 * N + e] = 1.f; t.env_shape_bound[0 * N + e] = 1.f; t.env_shape_bound[1 * N + e] = 0.1f; }
  const PackedModel T = expect_pack("per-env hull, turned frame", t, N);
  // body-frame offset (0, 0.1, 0) is (0.1, 0, 0) in the shape frame: |x - 0.1| over the hull's x in {0.1, -0.1, 0, 0, 0.05}
  if (T.env_shape_param.size() == 4 * N) CHECK(close(T.env_shape_param[1 * N + 0], 0.2f) && close(T.env_shape_param[2 * N + 0], 0.3f) && close(T.env_shape_param[3 * N + 0], 0.4f));
}

static void check_mesh() {
  const Model m = mesh_model();
  const PackedModel P = expect_pack("mesh", m, 2);
  CHECK(P.has_tri && P.n_mesh_pair == 1 && P.pair_mesh_slot == VI(1, 0) && P.hull_verts.empty());
  CHECK(P.shape_hull == (VI{0, 0, 0, 0}) && P.rows_per_env == 1);
  CHECK(P.shape_half.size() == 6 && P.shape_half[0] == 0.05f && P.shape_half[3] == 2.f && P.shape_half[4] == 2.f && P.shape_half[5] == 0.5f);
  // a second mesh pair gets the next slot; a pair whose second shape is no mesh gets none
  Model m2 = mesh_model();
  m2.add_shape(MSSIM_SHAPE_BOX, MSSIM_BODY_FREE, 0, 0.1f, 0.1f, 0.1f);
  m2.add_pair(2, 0);
  m2.add_pair(2, 1);
  const PackedModel Q = expect_pack("two mesh pairs", m2, 2);
  CHECK(Q.n_mesh_pair == 2 && Q.pair_mesh_slot == (VI{0, -1, 1}));
  // per-env meshes in the mesh's slot: env 0 triangle 1 alone, env 1 no shape
  Model e = mesh_model();
  e.num_envs = 2; e.n_env_shape = 1; e.shape_env_slot[1] = 0;
  e.env_shape_frame = {0, 0, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0};
  e.env_shape_bound = {0, 0, 0, 0, 0, 0, 1, 1};
  e.env_shape_param = {1, 0, 1, 0, 0, 0, 0, MSSIM_SHAPE_NONE + 1};
  const PackedModel E = expect_pack("per-env mesh", e, 2);
  if (E.env_shape_param.size() == 8) {
    CHECK(bits(E.env_shape_param[0]) == (MSSIM_SHAPE_TRIMESH | 0 << 10) && bits(E.env_shape_param[1]) == MSSIM_SHAPE_NONE);
    CHECK(E.env_shape_param[2] == 2.f && E.env_shape_param[4] == 1.f && E.env_shape_param[6] == 0.f && E.env_shape_param[3] == 0.f);
  } else {
    CHECK(false);
  }
  e.env_shape_param[2] = 2;  // 2 triangles from triangle 1
  expect_reject("per-env mesh range", e, 2, 8, "per-env triangle mesh: triangle range / root node out of range");
}

static void check_topology() {
  // TopoPanda::anc (mssim_kernels.hip): the strict ancestors of each joint of the Panda chain
  const uint32_t anc[9] = {0x00, 0x01, 0x03, 0x07, 0x0F, 0x1F, 0x3F, 0x7F, 0x7F};
  for (int n_free = 1; n_free <= 3; n_free++) {
    const PackedModel P = expect_pack("panda chain", panda_chain(n_free), 4);
    CHECK(P.panda && P.dof_anc == std::vector<uint32_t>(anc, anc + 9));
    CHECK(P.rows_per_env == (n_free == 1 ? 1 : (n_free == 2 ? 2 : 4)));  // 15, 21, 27 velocity components
    CHECK(P.dof_pack.size() == 32 * 9 && P.shape_pack.size() == 24 && P.shape_hull == VI(2, 0) && P.pair_packed == VI(128, -1));
    for (int j = 0; j < 9 && P.dof_pack.size() == 32 * 9; j++) {
      const float* r = &P.dof_pack[32 * j];
      CHECK(r[2] == 0.1f && r[3] == 1.f && r[9] == 1.f && bits(r[10]) == kPandaParent[j] && bits(r[11]) == kPandaType[j] && (uint32_t)bits(r[12]) == anc[j]);
      CHECK(r[13] == 100.f && r[14] == 10.f && r[15] == 50.f && r[16] == 0.f && r[17] == 0.01f && r[18] == -1.f && r[19] == 1.f && r[20] == 1.f && r[24] == 1.f && bits(r[30]) == 0);
    }
  }
  Model m = panda_chain(1);
  m.dof_parent[8] = 7;  // the second finger on the first
  const PackedModel P = expect_pack("other parent", m, 4);
  CHECK(!P.panda && P.dof_anc[8] == 0xFFu);
  Model t = panda_chain(1);
  t.dof_type[6] = MSSIM_JOINT_PRISMATIC;
  CHECK(!expect_pack("other type", t, 4).panda);
  Model none;
  const PackedModel Z = expect_pack("empty model", none, 1);
  CHECK(!Z.panda && Z.dof_anc == std::vector<uint32_t>(1, 0u) && Z.dof_pack == VF(32, 0.f) && Z.rows_per_env == 1);
}

int main() {
  check_rejections();
  check_hulls_and_shapes();
  check_per_env_rows();
  check_mesh();
  check_topology();
  if (g_failed) std::printf("%d check(s) failed\n", g_failed);
  else std::printf("model_pack_check: ok\n");
  return g_failed ? 1 : 0;
}
