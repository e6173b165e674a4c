// mssim_raycast_desc.h -- what mssim_raycast_create accepts (include/mssim_hip_tasks.h): index ranges, plane ranges,
// triangle ranges and the BVH's references (range, cycles, depth), override slots and their per-env ranges. Plain C++17,
// no HIP: a malformed scene is turned down before the device is touched, and tests/native/raycast_desc_check.cpp and
// raycast_mesh_desc_check.cpp check the rules on a CPU.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mssim_hip_tasks.h"

namespace mssim_raycast {

constexpr int kMaxImageSide = 4096;

inline int refuse(std::string* err, int rc, const std::string& msg) {
  if (err) *err = "raycast_create: " + msg;
  return rc;
}

inline bool finite_all(const float* p, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (!std::isfinite(p[i])) return false;
  return true;
}

// first triangle, triangle count, root node of a mesh (three float-valued integers) against the tables
inline bool mesh_words_ok(const mssim_raycast_scene* s, float first, float count, float root) {
  if (!(first >= 0.f) || !(count >= 0.f) || !(root >= 0.f)) return false;
  return (double)first + (double)count <= (double)s->n_tri && root < (float)s->n_tri_node && first == std::floor(first) && count == std::floor(count) &&
         root == std::floor(root);
}

// height[node] = levels of nodes below and with it, for every node of the table. Refuses (2) a child reference that points
// outside the tables and references that form a cycle (an explicit stack: a chain of 100000 nodes is walked, not recursed into)
inline int bvh_heights(const mssim_raycast_scene* s, std::vector<int>* height, std::string* err) {
  const int n = s->n_tri_node;
  height->assign((size_t)n, 0);
  std::vector<signed char> state((size_t)n, 0);  // 0 new, 1 on the path, 2 done
  std::vector<int> path, next;
  auto ref_of = [&](int node, int c) { int32_t r; std::memcpy(&r, s->tri_bvh + (size_t)node * 112 + 96 + c, 4); return r; };
  auto has = [&](int node, int c) { const float* b = s->tri_bvh + (size_t)node * 112 + 6 * c; return b[0] <= b[3]; };  // (min > max or NaN: no child)
  for (int start = 0; start < n; start++) {
    if (state[(size_t)start]) continue;
    path.assign(1, start); next.assign(1, 0);
    state[(size_t)start] = 1; (*height)[(size_t)start] = 1;
    while (!path.empty()) {
      const int node = path.back();
      int& c = next.back();
      if (c == 16) {
        state[(size_t)node] = 2;
        const int h = (*height)[(size_t)node];
        path.pop_back(); next.pop_back();
        if (!path.empty()) (*height)[(size_t)path.back()] = std::max((*height)[(size_t)path.back()], h + 1);
        continue;
      }
      const int k = c++;
      if (!has(node, k)) continue;
      const int32_t ref = ref_of(node, k);
      if (ref < 0 ? ~ref >= s->n_tri : ref >= n)
        return refuse(err, 2, "tri_bvh node " + std::to_string(node) + ": child reference " + std::to_string(ref) + " points outside the node / triangle tables");
      if (ref < 0) continue;
      if (state[(size_t)ref] == 1) return refuse(err, 2, "tri_bvh node " + std::to_string(node) + ": the child references form a cycle through node " + std::to_string(ref));
      if (state[(size_t)ref] == 2) { (*height)[(size_t)node] = std::max((*height)[(size_t)node], (*height)[(size_t)ref] + 1); continue; }
      state[(size_t)ref] = 1; (*height)[(size_t)ref] = 1;
      path.push_back(ref); next.push_back(0);
    }
  }
  return 0;
}

// 0 = accepted. `N` envs, `n_rows` body rows of rigid_body_data. Return codes: 1 bad arguments, 2 index out of range
// (a BVH reference cycle included), 3 out of scope (a triangle mesh without a triangle table or in a slot that is not a
// mesh's, a per-env hull in a slot that is not a hull's, a BVH deeper than the kernel's stack), 4 bad camera.
inline int validate(const mssim_raycast_scene* s, const mssim_camera_desc* cams, int n_cameras, int N, int n_rows, std::string* err) {
  if (!s || !cams) return refuse(err, 1, "no scene / cameras");
  if (N <= 0) return refuse(err, 1, "no envs");
  if (n_cameras <= 0) return refuse(err, 1, "no cameras");
  if (s->n_shape < 0 || s->n_plane < 0 || s->n_env_shape < 0 || s->n_tri < 0 || s->n_tri_node < 0) return refuse(err, 1, "negative count");
  if (s->n_shape > 0 && (!s->shape_type || !s->shape_row || !s->shape_frame || !s->shape_param || !s->shape_bound || !s->shape_seg || !s->shape_planes))
    return refuse(err, 1, "a shape table is missing");
  if (s->n_plane > 0 && !s->planes) return refuse(err, 1, "no plane table");
  if (s->n_env_shape > 0 && (!s->shape_env_slot || !s->env_shape_frame || !s->env_shape_param || !s->env_shape_bound))
    return refuse(err, 1, "a per-env table is missing");
  if (s->n_plane > 0 && !finite_all(s->planes, 4 * (size_t)s->n_plane)) return refuse(err, 1, "a plane is not finite");
  if ((s->n_tri > 0 && !s->tri_soup) || (s->n_tri_node > 0 && !s->tri_bvh)) return refuse(err, 1, "a triangle table is missing");
  if (s->n_tri >= (1 << 24) || s->n_tri_node >= (1 << 24)) return refuse(err, 1, "more than 16777215 triangles or BVH nodes (counts are carried as floats)");
  const bool has_mesh = s->n_tri > 0 && s->n_tri_node > 0;
  if (s->n_tri > 0 && !finite_all(s->tri_soup, 12 * (size_t)s->n_tri)) return refuse(err, 1, "a triangle is not finite");
  std::vector<int> height;
  if (has_mesh)
    if (int rc = bvh_heights(s, &height, err)) return rc;
  // a mesh named by (first triangle, count, root node): in range, and no deeper than the traversal stack
  auto mesh_ok = [&](const std::string& who, float first, float count, float root) {
    if (!mesh_words_ok(s, first, count, root))
      return refuse(err, 2, who + ": triangle range [" + std::to_string(first) + ", +" + std::to_string(count) + ") / root node " + std::to_string(root) +
                                " outside the tables of " + std::to_string(s->n_tri) + " triangles, " + std::to_string(s->n_tri_node) + " nodes");
    if (height[(size_t)root] > MSSIM_RAYCAST_MESH_DEPTH)
      return refuse(err, 3, who + ": its BVH is " + std::to_string(height[(size_t)root]) + " levels deep, the ray caster's traversal stack holds " + std::to_string(MSSIM_RAYCAST_MESH_DEPTH));
    return 0;
  };
  for (int i = 0; i < s->n_shape; i++) {
    const std::string who = "shape " + std::to_string(i);
    const int type = s->shape_type[i];
    if (type == MSSIM_SHAPE_TRIMESH && !has_mesh) return refuse(err, 3, who + " is a triangle mesh in a scene that carries no triangle table");
    if (type < MSSIM_SHAPE_PLANE || type > MSSIM_SHAPE_TRIMESH) return refuse(err, 2, who + ": unknown type " + std::to_string(type));
    if (s->shape_row[i] < -1 || s->shape_row[i] >= n_rows) return refuse(err, 2, who + ": body row " + std::to_string(s->shape_row[i]) + " out of range");
    if (!finite_all(s->shape_frame + 7 * (size_t)i, 7) || !finite_all(s->shape_param + 4 * (size_t)i, 4) || !finite_all(s->shape_bound + 4 * (size_t)i, 4))
      return refuse(err, 1, who + ": frame / param / bound not finite");
    if (type == MSSIM_SHAPE_CONVEX) {
      const long long first = s->shape_planes[2 * i], count = s->shape_planes[2 * i + 1];
      if (first < 0 || count < 4 || first + count > s->n_plane)
        return refuse(err, 2, who + ": plane range [" + std::to_string(first) + ", +" + std::to_string(count) + ") outside the table of " + std::to_string(s->n_plane));
    }
    if (type == MSSIM_SHAPE_TRIMESH)
      if (int rc = mesh_ok(who, s->shape_param[4 * (size_t)i], s->shape_param[4 * (size_t)i + 1], s->shape_param[4 * (size_t)i + 2])) return rc;
    const int slot = s->n_env_shape > 0 ? s->shape_env_slot[i] : -1;
    if (slot < -1 || slot >= s->n_env_shape) return refuse(err, 2, who + ": override slot " + std::to_string(slot) + " out of range");
    if (slot < 0) continue;
    if (type == MSSIM_SHAPE_PLANE) return refuse(err, 1, who + ": a plane cannot be a per-env shape");
    const float* ptype = s->env_shape_param + ((size_t)slot * 4 + 3) * (size_t)N;
    for (int e = 0; e < N; e++) {
      const float t1 = ptype[e];
      if (!(t1 >= 0.f && t1 <= (float)(MSSIM_SHAPE_TRIMESH + 1)) || t1 != std::floor(t1))
        return refuse(err, 2, who + ": per-env type of env " + std::to_string(e) + " is not a shape type");
      const int te = t1 == 0.f ? type : (int)t1 - 1;
      if (te == MSSIM_SHAPE_TRIMESH && type != MSSIM_SHAPE_TRIMESH)
        return refuse(err, 3, who + " is a triangle mesh in env " + std::to_string(e) + ", in a slot whose shared type is not a triangle mesh");
      if (te == MSSIM_SHAPE_PLANE) return refuse(err, 1, who + ": a plane cannot be a per-env shape");
      if (te == MSSIM_SHAPE_CONVEX && type != MSSIM_SHAPE_CONVEX)
        return refuse(err, 3, who + " is a hull of its own in env " + std::to_string(e) + " (per-env hulls only in a slot whose shared type is a hull)");
      const std::string where = who + " in env " + std::to_string(e);
      if (te == MSSIM_SHAPE_TRIMESH && t1 != 0.f) {  // (the env's own mesh; 0 = the shared one, checked above)
        const float* ep = s->env_shape_param + (size_t)slot * 4 * N + e;
        if (!std::isfinite(ep[0]) || !std::isfinite(ep[(size_t)N]) || !std::isfinite(ep[2 * (size_t)N])) return refuse(err, 1, who + ": per-env frame / param / bound not finite");
        if (int rc = mesh_ok(where, ep[0], ep[(size_t)N], ep[2 * (size_t)N])) return rc;
      }
      if (te == MSSIM_SHAPE_CONVEX && s->env_shape_planes) {
        const long long first = s->env_shape_planes[(size_t)slot * 2 * N + e], count = s->env_shape_planes[((size_t)slot * 2 + 1) * N + e];
        if (first < 0 || count < 4 || first + count > s->n_plane)
          return refuse(err, 2, where + ": per-env plane range [" + std::to_string(first) + ", +" + std::to_string(count) + ") outside the table of " + std::to_string(s->n_plane));
      }
    }
    if (!finite_all(s->env_shape_frame + (size_t)slot * 7 * N, 7 * (size_t)N) || !finite_all(s->env_shape_param + (size_t)slot * 4 * N, 4 * (size_t)N) ||
        !finite_all(s->env_shape_bound + (size_t)slot * 4 * N, 4 * (size_t)N))
      return refuse(err, 1, who + ": per-env frame / param / bound not finite");
  }
  for (int c = 0; c < n_cameras; c++) {
    const mssim_camera_desc& k = cams[c];
    const std::string who = "camera " + std::to_string(c);
    if (k.width <= 0 || k.height <= 0 || k.width > kMaxImageSide || k.height > kMaxImageSide) return refuse(err, 4, who + ": image size out of range");
    if (!(k.fx > 0.f) || !(k.fy > 0.f) || !std::isfinite(k.fx) || !std::isfinite(k.fy) || !std::isfinite(k.cx) || !std::isfinite(k.cy))
      return refuse(err, 4, who + ": bad intrinsics");
    if (!(k.near > 0.f) || !(k.far > k.near) || !std::isfinite(k.far)) return refuse(err, 4, who + ": needs 0 < near < far");
    if (k.mount_row < -1 || k.mount_row >= n_rows) return refuse(err, 2, who + ": mount row " + std::to_string(k.mount_row) + " out of range");
    if (!k.env_pose && !finite_all(k.pose, 7)) return refuse(err, 4, who + ": pose not finite");
    // (blocks of one launch: tiles x envs, counted in 32 bits)
    const long long tiles = (long long)((k.width + 15) / 16) * ((k.height + 15) / 16);
    if (tiles * N > 0x7fffffffLL) return refuse(err, 4, who + ": too many tiles for one launch");
  }
  return 0;
}

}  // namespace mssim_raycast
