// mssim_model_pack.h -- the part of mssim_create that needs no device: validate_model() holds every check a model has
// to pass (a malformed model gets a return code and an error string, not an out-of-bounds read on the host or on the
// device), pack_model() derives every table the kernels read from it. Plain C++17, no HIP: tests/native/model_pack_check.cpp
// runs both on a CPU.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mssim.h"
#include "mssim_limits.h"

// what the Panda kernels (TopoPanda: the 9-DoF tree unrolled at compile time) stand for: panda_v2/v3, a chain of 7
// revolute joints and 2 prismatic fingers on body 6
static const int kPandaParent[9] = {-1, 0, 1, 2, 3, 4, 5, 6, 6};
static const int kPandaType[9] = {0, 0, 0, 0, 0, 0, 0, 1, 1};

// Everything mssim_create uploads that is not a verbatim copy of a model array. Tables of a model without joints /
// shapes / pairs keep one (unused) element, as the device copies do.
struct PackedModel {
  // hull vertices repacked so that every hull starts on a multiple of 8 vertices and is padded to a multiple of 8 with
  // copies of its vertex 0: `support()` reads whole 8-vertex batches as six aligned 16-byte loads, and a copy of vertex 0
  // can never win its strict first-maximum scan. Ranges that share (start, count) share one repacked range.
  std::vector<int32_t> shape_hull;     // [n_shape][2] first repacked vertex, count (a triangle mesh: root node of its BVH, 0)
  std::vector<float> hull_verts;       // [..][3]
  // device rows of every per-env shape ([n_env_shape*4][N]; empty without per-env shapes): row 0 = type | vertex count << 3 |
  // first repacked vertex << 10 (a mesh: root node << 10) as a bit pattern, rows 1..3 = the three parameters of a primitive,
  // or the half extents of a hull's / mesh's box about its bound centre (shape frame) for the cull
  std::vector<float> env_shape_param;
  std::vector<float> shape_center;     // [n_shape][3] bounding-sphere centre in the BODY frame (shape_frame applied)
  std::vector<float> shape_half;       // [n_shape][3] half extents of a box in the SHAPE frame, centred at the bound centre, that contains the shape
  std::vector<float> shape_pack;       // [n_shape][24] all per-shape constants of the narrowphase in one 96-byte record
  std::vector<float> dof_pack;         // [n_dof][32]   all per-joint constants of the control-step kernel in one 128-byte record
  std::vector<uint32_t> dof_anc;       // [n_dof] bitmask of strict ancestors of each dof
  std::vector<int32_t> shape_env_slot, free_env_slot;  // the model's, or -1 (shared) throughout when it has no such env arrays (a shape's goes into its shape_pack record)
  std::vector<int32_t> pair_mesh_slot; // [n_pair] ordinal of the pair among those whose second shape is a triangle mesh, else -1
  int n_mesh_pair = 0;
  std::vector<int32_t> pair_packed;    // [n_pair rounded up to 128, + 128] shape a | shape b << 8, -1 behind the last pair
  bool has_tri = false;                // the model has triangle-mesh shapes
  bool panda = false;                  // joints have the Panda's parents and types
  int rows_per_env = 1;                // 16-lane rows an env takes in the control-step kernel (its template parameter NR)
};

namespace mssim_pack {

// the control-step kernel keeps an env on 16-lane rows, one velocity component per lane: 1 row while joints and free
// bodies fit 16 lanes together; else the joints in row 0 and two free bodies per further row
inline int rows_per_env(const mssim_model_desc* d) { return d->n_dof + 6 * d->n_free <= S16_LANES ? 1 : (d->n_free <= 2 ? 2 : 4); }

// rotation matrix of a (w, x, y, z) quaternion of any length
inline void rot_from_quat(const float* q, float R[3][3]) {
  const float nq = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const float qw = q[0] / nq, qx = q[1] / nq, qy = q[2] / nq, qz = q[3] / nq;
  const float r[3][3] = {{1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qw * qz), 2 * (qx * qz + qw * qy)},
                         {2 * (qx * qy + qw * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qw * qx)},
                         {2 * (qx * qz - qw * qy), 2 * (qy * qz + qw * qx), 1 - 2 * (qx * qx + qy * qy)}};
  std::memcpy(R, r, sizeof r);
}

// h[k] = max |p[k] - c[k]| over `count` hull vertices (3 floats each) or, `tri`, over the corners of `count` triangles
// of tri_soup (12 floats each: centroid, three corners relative to it)
inline void extent_about(const float* c, const float* pts, int count, bool tri, float* h) {
  h[0] = h[1] = h[2] = 0.f;
  for (int i = 0; i < count; i++) {
    const float* p = pts + (size_t)(tri ? 12 : 3) * i;
    for (int c3 = 0; c3 < (tri ? 3 : 1); c3++)
      for (int k = 0; k < 3; k++) h[k] = std::max(h[k], std::fabs((tri ? p[k] + p[3 + 3 * c3 + k] : p[k]) - c[k]));
  }
}

// element (row, e) of a per-env array [rows][N]
inline float env_at(const float* a, int row, int num_envs, int e) { return a[(size_t)row * num_envs + e]; }
// shape type of per-env slot `slot` of shape s in env e (row 3 of env_shape_param: type + 1, 0 = the shared type)
inline int env_shape_type(const mssim_model_desc* d, int s, int slot, int num_envs, int e) {
  const int tcode = (int)env_at(d->env_shape_param, 4 * slot + 3, num_envs, e);
  return tcode > 0 ? tcode - 1 : d->shape_type[s];
}

}  // namespace mssim_pack

// Every check mssim_create makes on a model, before anything touches the device. 0, or the return code of mssim_create
// with its message in *err.
inline int validate_model(const mssim_model_desc* d, int num_envs, std::string* err) {
  using namespace mssim_pack;
  auto fail = [&](int rc, const char* msg) { *err = msg; return rc; };
  if (!d || num_envs <= 0) return fail(1, "bad arguments");
  if (d->abi_version != MSSIM_ABI_VERSION) return fail(2, "ABI version mismatch");
  if (d->n_dof > MSSIM_MAX_DOF || d->n_free > MSSIM_MAX_FREE) return fail(3, "model exceeds MSSIM_MAX_DOF / MSSIM_MAX_FREE");
  const int nr = rows_per_env(d), ns = d->n_shape;
  if (d->n_dof > S16_LANES || d->n_free > S16_MAX_FREE_(4) || d->n_kin > S16_MAX_KIN || ns > S16_MAX_SHAPE_(nr) || d->n_pair > S16_MAX_PAIR) {
    char msg[320];
    snprintf(msg, sizeof msg, "model exceeds the control-step kernel's tables: %d joints (max %d), %d free bodies (max %d), %d kinematic bodies (max %d), "
             "%d shapes (max %d with %d velocity components), %d candidate pairs (max %d)", d->n_dof, S16_LANES, d->n_free, S16_MAX_FREE_(4), d->n_kin, S16_MAX_KIN, ns,
             S16_MAX_SHAPE_(nr), d->n_dof + 6 * d->n_free, d->n_pair, S16_MAX_PAIR);
    return fail(9, msg);
  }
  for (int j = 0; j < d->n_dof; j++)
    if (d->dof_parent[j] >= j) return fail(4, "dof_parent must be topologically sorted");
  for (int i = 0; i < 2 * d->n_pair; i++)
    if (d->pair_shape[i] < 0 || d->pair_shape[i] >= ns) return fail(4, "pair_shape names a shape that does not exist");
  for (int s = 0; s < ns; s++)
    if (d->shape_type[s] == MSSIM_SHAPE_CONVEX && (d->shape_hull[2 * s + 1] < 4 || d->shape_hull[2 * s + 1] > MSSIM_MAX_HULL_VERTS))
      return fail(5, "convex hull vertex count out of range");
  // tables the kernels index without checks
  if (d->n_tri_node >= (1 << 17) || d->n_tri >= (1 << 24))
    return fail(5, "triangle meshes: more than 131071 BVH nodes or 16777215 triangles (the shape word packs the root node into 17 bits)");
  for (int nd = 0; nd < d->n_tri_node; nd++)
    for (int c = 0; c < 16; c++) {
      const float* nb = d->tri_bvh + (size_t)nd * 112;
      if (!(nb[6 * c] <= nb[6 * c + 3])) continue;  // (min > max: no child)
      int32_t ref;
      std::memcpy(&ref, nb + 96 + c, 4);
      if (ref >= 0 ? ref >= d->n_tri_node : ~ref >= d->n_tri) return fail(5, "tri_bvh: a child reference points outside the node / triangle tables");
    }
  const bool has_es = d->n_env_shape > 0, has_ef = d->n_env_free > 0;
  for (int s = 0; has_es && s < ns; s++)
    if (d->shape_env_slot[s] >= d->n_env_shape) return fail(5, "shape_env_slot names a slot beyond n_env_shape");
  for (int b = 0; has_ef && b < d->n_free; b++)
    if (d->free_env_slot[b] >= d->n_env_free) return fail(5, "free_env_slot names a slot beyond n_env_free");
  for (int s = 0; s < ns; s++)
    if (d->shape_type[s] == MSSIM_SHAPE_CONVEX && (d->shape_hull[2 * s] < 0 || d->shape_hull[2 * s] + d->shape_hull[2 * s + 1] > d->n_hull_verts))
      return fail(5, "convex hull: vertex range outside hull_verts");
  for (int s = 0; s < ns; s++) {
    if (d->shape_type[s] != MSSIM_SHAPE_TRIMESH) continue;
    const int root = d->shape_hull[2 * s], kind = d->shape_body_kind[s];
    if (root < 0 || root >= d->n_tri_node || kind == MSSIM_BODY_FREE || kind == MSSIM_BODY_ART)
      return fail(8, "triangle mesh: BVH root out of range, or the mesh belongs to a moving body (fixed / kinematic bodies only)");
    const int first = (int)d->shape_param[4 * s], count = (int)d->shape_param[4 * s + 1];
    if (first < 0 || count < 0 || first + count > d->n_tri) return fail(8, "triangle mesh: triangle range out of tri_soup");
  }
  if ((has_es || has_ef) && d->num_envs != num_envs) return fail(7, "per-env arrays were built for a different num_envs");
  for (int s = 0; has_es && s < ns; s++) {
    const int slot = d->shape_env_slot[s];
    if (slot < 0) continue;
    for (int e = 0; e < num_envs; e++) {
      const int type = env_shape_type(d, s, slot, num_envs, e);
      const int p0 = (int)env_at(d->env_shape_param, 4 * slot, num_envs, e), p1 = (int)env_at(d->env_shape_param, 4 * slot + 1, num_envs, e);
      // (a triangle mesh only in a slot whose own type is TRIMESH: the mesh variant of the kernel is chosen by the shared types)
      const bool env_mesh = type == MSSIM_SHAPE_TRIMESH && d->shape_type[s] == MSSIM_SHAPE_TRIMESH;
      if ((type < MSSIM_SHAPE_BOX || type > MSSIM_SHAPE_NONE) && !env_mesh)
        return fail(8, "per-env shape type out of range (planes cannot be per-env shapes; a triangle mesh only in a slot that is a triangle mesh)");
      if (env_mesh) {  // first triangle, triangle count, root node of this env's mesh
        const int root = (int)env_at(d->env_shape_param, 4 * slot + 2, num_envs, e);
        if (p0 < 0 || p1 < 0 || p0 + p1 > d->n_tri || root < 0 || root >= d->n_tri_node) return fail(8, "per-env triangle mesh: triangle range / root node out of range");
      }
      if (type == MSSIM_SHAPE_CONVEX && (p1 < 1 || p1 > MSSIM_MAX_HULL_VERTS || p0 < 0 || p0 + p1 > d->n_hull_verts))  // first vertex, vertex count
        return fail(8, "per-env hull reference out of range");
    }
  }
  return 0;
}

// The tables of a model that passed validate_model. Fails only on what is known after the hulls are repacked: more
// vertices than a shape word can address.
inline int pack_model(const mssim_model_desc* d, int num_envs, PackedModel* P, std::string* err) {
  using namespace mssim_pack;
  const int n = d->n_dof, ns = d->n_shape, np = d->n_pair;
  const size_t n1 = n > 0 ? n : 1, ns1 = ns > 0 ? ns : 1, np1 = np > 0 ? np : 1;
  const bool has_es = d->n_env_shape > 0, has_ef = d->n_env_free > 0;
  auto fbits = [](int32_t v) { float f; std::memcpy(&f, &v, 4); return f; };
  P->rows_per_env = rows_per_env(d);
  P->panda = n == 9 && std::equal(kPandaParent, kPandaParent + 9, d->dof_parent) && std::equal(kPandaType, kPandaType + 9, d->dof_type);
  P->dof_anc.assign(n1, 0u);
  for (int j = 0; j < n; j++)
    for (int i = d->dof_parent[j]; i >= 0; i = d->dof_parent[i]) P->dof_anc[j] |= 1u << i;

  // hulls of the shared shapes, then of the per-env shapes, each (start, count) once
  std::vector<int> seen;  // start, count, repacked start
  auto repacked = [&](int st, int cnt) {
    for (size_t i = 0; i < seen.size(); i += 3)
      if (seen[i] == st && seen[i + 1] == cnt) return seen[i + 2];
    const int found = (int)(P->hull_verts.size() / 3);
    for (int i = 0; i < (cnt + 7) / 8 * 8; i++) {
      const float* v = d->hull_verts + 3 * (size_t)(st + (i < cnt ? i : 0));
      P->hull_verts.insert(P->hull_verts.end(), v, v + 3);
    }
    seen.insert(seen.end(), {st, cnt, found});
    return found;
  };
  P->shape_hull.assign(2 * ns1, 0);
  for (int s = 0; s < ns; s++) {
    const int st = d->shape_hull[2 * s], cnt = d->shape_hull[2 * s + 1];
    if (d->shape_type[s] == MSSIM_SHAPE_TRIMESH) {  // (root node of its BVH, no hull vertices)
      P->shape_hull[2 * s] = st;
      P->has_tri = true;
      continue;
    }
    P->shape_hull[2 * s + 1] = cnt;
    if (cnt > 0) P->shape_hull[2 * s] = repacked(st, cnt);
  }
  if (has_es) P->env_shape_param.assign(d->env_shape_param, d->env_shape_param + (size_t)4 * d->n_env_shape * num_envs);
  for (int s = 0; has_es && s < ns; s++) {
    const int slot = d->shape_env_slot[s];
    if (slot < 0) continue;
    for (int e = 0; e < num_envs; e++) {
      const int type = env_shape_type(d, s, slot, num_envs, e);
      int32_t word = type;
      float rows[3];
      for (int k = 0; k < 3; k++) rows[k] = type == MSSIM_SHAPE_NONE ? 0.f : env_at(d->env_shape_param, 4 * slot + k, num_envs, e);
      const bool env_mesh = type == MSSIM_SHAPE_TRIMESH && d->shape_type[s] == MSSIM_SHAPE_TRIMESH;
      if (env_mesh || type == MSSIM_SHAPE_CONVEX) {
        // rows = (first triangle, triangle count, root node) of this env's mesh, or (first vertex, vertex count) of its hull.
        // The device rows get the half extents about the bound centre: body frame -> shape frame first
        const int first = (int)rows[0], count = (int)rows[1], root = (int)rows[2];
        float fr[7], cb[3], cs[3], R[3][3];
        for (int k = 0; k < 7; k++) fr[k] = env_at(d->env_shape_frame, 7 * slot + k, num_envs, e);
        for (int k = 0; k < 3; k++) cb[k] = env_at(d->env_shape_bound, 4 * slot + k, num_envs, e) - fr[k];
        rot_from_quat(fr + 3, R);
        for (int k = 0; k < 3; k++) cs[k] = R[0][k] * cb[0] + R[1][k] * cb[1] + R[2][k] * cb[2];
        extent_about(cs, env_mesh ? d->tri_soup + 12 * (size_t)first : d->hull_verts + 3 * (size_t)first, count, env_mesh, rows);
        word |= env_mesh ? root << 10 : (count << 3) | (repacked(first, count) << 10);
      }
      P->env_shape_param[(size_t)(4 * slot) * num_envs + e] = fbits(word);
      for (int k = 0; k < 3; k++) P->env_shape_param[(size_t)(4 * slot + 1 + k) * num_envs + e] = rows[k];
    }
  }
  if (P->hull_verts.size() / 3 >= (1u << 17)) { *err = "too many hull vertices"; return 8; }

  // bound centres in the body frame; oriented bounding boxes for the cull (shape frame axes, centred at the bound centre)
  P->shape_center.assign(3 * ns1, 0.f);
  P->shape_half.assign(3 * ns1, 0.f);
  for (int s = 0; s < ns; s++) {
    const float *f = d->shape_frame + 7 * s, *b = d->shape_bound + 4 * s, *pp = d->shape_param + 4 * s;
    float R[3][3], *h = &P->shape_half[3 * s];
    rot_from_quat(f + 3, R);
    for (int i = 0; i < 3; i++) P->shape_center[3 * s + i] = f[i] + R[i][0] * b[0] + R[i][1] * b[1] + R[i][2] * b[2];
    switch (d->shape_type[s]) {
      case MSSIM_SHAPE_BOX: h[0] = pp[0]; h[1] = pp[1]; h[2] = pp[2]; break;
      case MSSIM_SHAPE_SPHERE: h[0] = h[1] = h[2] = pp[0]; break;
      case MSSIM_SHAPE_CAPSULE: h[0] = pp[1] + pp[0]; h[1] = h[2] = pp[0]; break;
      case MSSIM_SHAPE_CYLINDER: h[0] = pp[1]; h[1] = h[2] = pp[0]; break;
      case MSSIM_SHAPE_CONVEX: extent_about(b, d->hull_verts + 3 * (size_t)d->shape_hull[2 * s], d->shape_hull[2 * s + 1], false, h); continue;
      case MSSIM_SHAPE_TRIMESH: extent_about(b, d->tri_soup + 12 * (size_t)(int)pp[0], (int)pp[1], true, h); continue;
      default: h[0] = h[1] = h[2] = 3e30f; continue;  // plane: never used
    }
    // primitive shapes are centred on their frame; keep the box valid if the bound centre is offset
    for (int k = 0; k < 3; k++) h[k] += std::fabs(b[k]);
  }

  P->shape_env_slot.assign(ns1, -1);
  P->free_env_slot.assign(d->n_free > 0 ? d->n_free : 1, -1);
  if (has_es) std::copy(d->shape_env_slot, d->shape_env_slot + ns, P->shape_env_slot.begin());
  if (has_ef) std::copy(d->free_env_slot, d->free_env_slot + d->n_free, P->free_env_slot.begin());

  // packed constant records (one or two cache lines per joint / shape instead of ~10 arrays)
  P->shape_pack.assign(24 * ns1, 0.f);
  for (int s = 0; s < ns; s++) {
    float* r = &P->shape_pack[24 * (size_t)s];
    for (int k = 0; k < 7; k++) r[k] = d->shape_frame[7 * s + k];
    for (int k = 0; k < 3; k++) { r[7 + k] = d->shape_param[4 * s + k]; r[10 + k] = P->shape_center[3 * s + k]; r[14 + k] = P->shape_half[3 * s + k]; }
    r[13] = d->shape_bound[4 * s + 3];
    r[17] = d->shape_material[4 * s + 1];
    r[18] = fbits(d->shape_type[s]);
    r[19] = fbits(d->shape_body_kind[s]);
    r[20] = fbits(d->shape_body_index[s]);
    r[21] = fbits(P->shape_env_slot[s]);
    r[22] = d->shape_material[4 * s + 3];  // torsional patch radius
  }
  P->dof_pack.assign(32 * n1, 0.f);
  for (int j = 0; j < n; j++) {
    float* r = &P->dof_pack[32 * (size_t)j];
    for (int k = 0; k < 7; k++) r[k] = d->dof_frame[7 * j + k];
    for (int k = 0; k < 3; k++) r[7 + k] = d->dof_axis[3 * j + k];
    r[10] = fbits(d->dof_parent[j]); r[11] = fbits(d->dof_type[j]); r[12] = fbits((int32_t)P->dof_anc[j]);
    for (int k = 0; k < 4; k++) r[13 + k] = d->dof_drive[4 * j + k];
    r[17] = d->dof_armature[j]; r[18] = d->dof_limit[2 * j]; r[19] = d->dof_limit[2 * j + 1];
    for (int k = 0; k < 10; k++) r[20 + k] = d->body_inertial[10 * j + k];
    r[30] = fbits(d->body_gravity[j]);
  }

  P->pair_mesh_slot.assign(np1, -1);
  P->pair_packed.assign((size_t)((np + 127) / 128 * 128 + 128), -1);  // (read in chunks of 8 rounds of 16)
  P->n_mesh_pair = 0;
  for (int p = 0; p < np; p++) {
    if (d->shape_type[d->pair_shape[2 * p + 1]] == MSSIM_SHAPE_TRIMESH) P->pair_mesh_slot[p] = P->n_mesh_pair++;
    P->pair_packed[p] = d->pair_shape[2 * p] | (d->pair_shape[2 * p + 1] << 8);
  }
  return 0;
}
