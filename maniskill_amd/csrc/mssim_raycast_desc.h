// mssim_raycast_desc.h -- what mssim_raycast_create accepts (include/mssim_hip_tasks.h): index ranges, plane ranges,
// override slots, and the two refusals (triangle meshes, per-env hulls). Plain C++17, no HIP: a malformed scene is
// turned down before the device is touched, and tests/native/raycast_desc_check.cpp checks the rules on a CPU.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

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

// What it cannot see: a scene holds no hull identity per env, so where a slot's shared type and an env's type are both
// CONVEX the env renders the SHARED plane range. A caller of the C entry point whose hulls differ from env to env must
// refuse such a model itself (model/compile.py: raycast_scene does); the header only turns down a per-env CONVEX type in a
// slot whose shared type is not CONVEX.
// 0 = accepted. `N` envs, `n_rows` body rows of rigid_body_data. Return codes: 1 bad arguments, 2 index out of range,
// 3 out of scope (triangle mesh, per-env hull), 4 bad camera.
inline int validate(const mssim_raycast_scene* s, const mssim_camera_desc* cams, int n_cameras, int N, int n_rows, std::string* err) {
  if (!s || !cams) return refuse(err, 1, "no scene / cameras");
  if (N <= 0) return refuse(err, 1, "no envs");
  if (n_cameras <= 0) return refuse(err, 1, "no cameras");
  if (s->n_shape < 0 || s->n_plane < 0 || s->n_env_shape < 0) return refuse(err, 1, "negative count");
  if (s->n_shape > 0 && (!s->shape_type || !s->shape_row || !s->shape_frame || !s->shape_param || !s->shape_bound || !s->shape_seg || !s->shape_planes))
    return refuse(err, 1, "a shape table is missing");
  if (s->n_plane > 0 && !s->planes) return refuse(err, 1, "no plane table");
  if (s->n_env_shape > 0 && (!s->shape_env_slot || !s->env_shape_frame || !s->env_shape_param || !s->env_shape_bound))
    return refuse(err, 1, "a per-env table is missing");
  if (s->n_plane > 0 && !finite_all(s->planes, 4 * (size_t)s->n_plane)) return refuse(err, 1, "a plane is not finite");
  for (int i = 0; i < s->n_shape; i++) {
    const std::string who = "shape " + std::to_string(i);
    const int type = s->shape_type[i];
    if (type == MSSIM_SHAPE_TRIMESH) return refuse(err, 3, who + " is a triangle mesh (out of scope of the ray caster)");
    if (type < MSSIM_SHAPE_PLANE || type > MSSIM_SHAPE_NONE) return refuse(err, 2, who + ": unknown type " + std::to_string(type));
    if (s->shape_row[i] < -1 || s->shape_row[i] >= n_rows) return refuse(err, 2, who + ": body row " + std::to_string(s->shape_row[i]) + " out of range");
    if (!finite_all(s->shape_frame + 7 * (size_t)i, 7) || !finite_all(s->shape_param + 4 * (size_t)i, 4) || !finite_all(s->shape_bound + 4 * (size_t)i, 4))
      return refuse(err, 1, who + ": frame / param / bound not finite");
    if (type == MSSIM_SHAPE_CONVEX) {
      const long long first = s->shape_planes[2 * i], count = s->shape_planes[2 * i + 1];
      if (first < 0 || count < 4 || first + count > s->n_plane)
        return refuse(err, 2, who + ": plane range [" + std::to_string(first) + ", +" + std::to_string(count) + ") outside the table of " + std::to_string(s->n_plane));
    }
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
      if (te == MSSIM_SHAPE_TRIMESH) return refuse(err, 3, who + " is a triangle mesh in env " + std::to_string(e) + " (out of scope of the ray caster)");
      if (te == MSSIM_SHAPE_PLANE) return refuse(err, 1, who + ": a plane cannot be a per-env shape");
      if (te == MSSIM_SHAPE_CONVEX && type != MSSIM_SHAPE_CONVEX)
        return refuse(err, 3, who + " is a hull of its own in env " + std::to_string(e) + " (per-env hulls are out of scope of the ray caster)");
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
