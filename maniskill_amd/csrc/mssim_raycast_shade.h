// mssim_raycast_shade.h -- the flat-shaded view behind render() and the episode videos (include/mssim_hip_tasks.h,
// mssim_raycast_set_colours / mssim_raycast_shade). Included by mssim_kernels.hip after mssim_raycast.h. It shows what the
// depth camera sees by construction: k_raycast_shade stages the shapes with k_raycast's rc_stage_shape and walks them with
// k_raycast's rc::trace -- one reject, one wave-wide skip, one rc::enter, one BVH walk -- and differs in the hit record alone
// (rc::Lit here, rc::Hit there).
//
// k_raycast_shade has k_raycast's shape: one block per 16 x 16 tile, one lane per pixel, the env's shapes staged in LDS a
// chunk at a time, beside them one float4 per shape (colour, checker cell) and, once per block, the two light directions
// in the camera's frame (rotated in double by one lane of wave 1 while wave 0 stages). rc::enter and rc::mesh_hit name the
// FACE a ray entered through, one integer. A later chunk overwrites the staged entries, so a lane whose nearest hit
// improves works out right then (rc::Lit::take) what it will need at the end: the unit normal at the entry point, from the
// face (rc::face_normal, rc::triangle_normal), rotated into the camera frame with the transpose of the staged rows, and the
// albedo with its checker. What a lane carries across chunks is t, the normal and the albedo: seven registers. One 4-byte
// store per pixel, no atomics.
//
// Where a ray enters (shape frame, p = o + t d):
//   plane     +x (and p.x is taken as exactly 0: the checker must not flicker on the roundings of a point ON the plane)
//   box       the axis whose slab set the entry parameter, signed against d on that axis; on a tie the lowest axis
//   sphere    p / |p|
//   cylinder  (+-1, 0, 0) where the cap slab set the entry, else (0, p_y, p_z) / r
//   capsule   the normal of whichever of the cylinder and the two balls gave the earliest entry (cylinder first on a tie)
//   hull      the normal of the first plane, in index order, that set tin
//   triangle  (e1 x e2) / |e1 x e2|, turned to face the ray: surfaces are two-sided, as they are for depth
// Light: ambient 0.3 and two white directional lights along (1, 1, -1) / sqrt 3 and (0, 0, -1) in the env frame, no
// shadows, no specular term: c = albedo min(1, 0.3 + sum_i max(0, -l_i . n)), channel = floor(255 min(c, 1) + 0.5).
// Albedo: rgb of the shape's float4; with a cell size w > 0 scaled by 0.8 where floor(p.x / w) + floor(p.y / w) +
// floor(p.z / w) is odd (a 3-D checker in the shape frame).
//
// The arithmetic (namespace rc) is under RC_HD and the refusals (namespace mssim_shade) are plain C++:
// tests/native/shade_check.cpp runs both on a CPU.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

#include "mssim_raycast.h"

namespace rc {

constexpr float kAmbient = 0.3f;
constexpr float kCheckerDim = 0.8f;
constexpr unsigned kBackgroundR = 44u, kBackgroundG = 52u, kBackgroundB = 66u;  // a pixel that hits nothing
constexpr unsigned kBackground = kBackgroundR | (kBackgroundG << 8) | (kBackgroundB << 16) | 0xff000000u;

RC_HD float against(float d) { return d > 0.f ? -1.f : 1.f; }

RC_HD v3 unit(v3 a) { return (1.f / sqrtf(dot(a, a))) * a; }

// outward unit normal (shape frame) where the ray o + t d enters the shape through `face`, t and face from rc::enter
RC_HD v3 face_normal(int type, const float* p, v3 o, v3 d, float t, int face, const float* __restrict__ planes, int pl0) {
  switch (type) {
    case MSSIM_SHAPE_BOX:
      return mk(face == 0 ? against(d.x) : 0.f, face == 1 ? against(d.y) : 0.f, face == 2 ? against(d.z) : 0.f);
    case MSSIM_SHAPE_SPHERE:
      return unit(o + t * d);
    case MSSIM_SHAPE_CYLINDER:
    case MSSIM_SHAPE_CAPSULE: {
      if (face == 1) return mk(against(d.x), 0.f, 0.f);
      if (face >= 2) return unit(mk(o.x - (face == 3 ? p[1] : -p[1]), o.y, o.z) + t * d);
      const float ir = 1.f / p[0];
      return mk(0.f, (o.y + t * d.y) * ir, (o.z + t * d.z) * ir);
    }
    case MSSIM_SHAPE_CONVEX: {
      const float* pl = planes + 4 * (size_t)(pl0 + face);
      return mk(pl[0], pl[1], pl[2]);
    }
    default:  // the plane
      return mk(1.f, 0.f, 0.f);
  }
}

// entry parameter and normal in one call (what tests/native/shade_check.cpp pins); *n is untouched where the line misses
RC_HD float enter_normal(int type, const float* p, v3 o, v3 d, const float* __restrict__ planes, int pl0, int pln, v3* n) {
  int face;
  const float t = enter(type, p, o, d, planes, pl0, pln, &face);
  if (t < kInf) *n = face_normal(type, p, o, d, t, face, planes, pl0);
  return t;
}

// unit normal of triangle `tri` of the soup, turned against the ray's direction d
RC_HD v3 triangle_normal(const float* __restrict__ soup, int tri, v3 d) {
  const float* q = soup + (size_t)tri * 12;
  const v3 e1 = mk(q[6] - q[3], q[7] - q[4], q[8] - q[5]), e2 = mk(q[9] - q[3], q[10] - q[4], q[11] - q[5]);
  const v3 n = unit(mk(e1.y * e2.z - e1.z * e2.y, e1.z * e2.x - e1.x * e2.z, e1.x * e2.y - e1.y * e2.x));
  return dot(n, d) > 0.f ? -1.f * n : n;
}

// the albedo at the point p of a shape (shape frame): `c` = r, g, b, checker cell size (0: none)
RC_HD v3 albedo(const float* c, v3 p, int type) {
  const v3 a = mk(c[0], c[1], c[2]);
  const float w = c[3];
  if (!(w > 0.f)) return a;
  if (type == MSSIM_SHAPE_PLANE) p.x = 0.f;
  const float k = floorf(p.x / w) + floorf(p.y / w) + floorf(p.z / w);
  return k - 2.f * floorf(0.5f * k) == 1.f ? kCheckerDim * a : a;
}

// the two light directions in the camera's OpenCV frame, L[0..2] and L[3..5], for the camera `cam` (env frame <- camera,
// SAPIEN axes): once per block, in double
RC_HD void lights(xf cam, float* L) {
  const real s = 1.0 / sqrt(3.0);
  const q4 ci = qconj(cam.q);
  const p3 a = qrot(ci, p3{s, s, -s}), b = qrot(ci, p3{0.0, 0.0, -1.0});
  L[0] = (float)-a.y; L[1] = (float)-a.z; L[2] = (float)a.x;
  L[3] = (float)-b.y; L[4] = (float)-b.z; L[5] = (float)b.x;
}

RC_HD unsigned channel(float c) { return (unsigned)floorf(255.f * fminf(c, 1.f) + 0.5f); }

// r | g << 8 | b << 16 | 255 << 24 of a surface with unit normal n and albedo a under the lights L (one frame for n and L)
RC_HD unsigned shade(v3 n, v3 a, const float* L) {
  const float l0 = fmaxf(0.f, -(L[0] * n.x + L[1] * n.y + L[2] * n.z)), l1 = fmaxf(0.f, -(L[3] * n.x + L[4] * n.y + L[5] * n.z));
  const float k = fminf(1.f, kAmbient + l0 + l1);
  return channel(a.x * k) | (channel(a.y * k) << 8) | (channel(a.z * k) << 16) | 0xff000000u;
}

// the nearest hit so far as the shaded view keeps it (rc::Hit's counterpart for rc::trace): parameter, unit normal in the
// camera frame, albedo -- a later chunk could no longer work the last two out. `col` holds four floats per shape of the
// staged chunk being walked.
struct Lit {
  float t; v3 n, a; const float* col;
  RC_HD void take(const Staged& s, int i, v3 o, v3 d, float t_, int face, bool mesh, const float* __restrict__ planes, const float* __restrict__ soup) {
    const v3 ns = mesh ? triangle_normal(soup, face, d) : face_normal(s.type, s.p, o, d, t_, face, planes, s.pl0);
    t = t_;
    // p_shape = R p_cv: a shape-frame direction goes back with the transpose
    n = mk(s.r0[0] * ns.x + s.r1[0] * ns.y + s.r2[0] * ns.z, s.r0[1] * ns.x + s.r1[1] * ns.y + s.r2[1] * ns.z,
           s.r0[2] * ns.x + s.r1[2] * ns.y + s.r2[2] * ns.z);
    a = albedo(col + 4 * i, o + t_ * d, s.type);
  }
};

}  // namespace rc

// ---- what mssim_raycast_set_colours and mssim_raycast_shade turn down (plain C++: no device is touched) ----
namespace mssim_shade {

inline int refuse(std::string* err, const char* who, int rc, const std::string& msg) {
  if (err) *err = std::string(who) + ": " + msg;
  return rc;
}

// 0 = accepted. shape_rgba [n_shape][4], env_shape_rgba [n_env_shape][N][4] or null. Return codes: 1 bad arguments,
// 2 a value out of range, 3 a table the scene has no use for.
inline int validate_colours(const float* shape_rgba, int n_shape, const float* env_shape_rgba, int n_env_shape, int N, std::string* err) {
  const char* who = "raycast_set_colours";
  if (n_shape > 0 && !shape_rgba) return refuse(err, who, 1, "no colour table");
  if (env_shape_rgba && n_env_shape <= 0) return refuse(err, who, 3, "a per-env colour table for a scene without per-env shape slots");
  auto bad = [](const float* c) {
    for (int k = 0; k < 4; k++)
      if (!std::isfinite(c[k]) || c[k] < 0.f) return true;
    return false;
  };
  for (int i = 0; i < n_shape; i++)
    if (bad(shape_rgba + 4 * (size_t)i))
      return refuse(err, who, 2, "shape " + std::to_string(i) + ": a colour or checker cell size that is negative or not finite");
  if (env_shape_rgba)
    for (size_t k = 0; k < (size_t)n_env_shape * (size_t)N; k++)
      if (bad(env_shape_rgba + 4 * k))
        return refuse(err, who, 2, "slot " + std::to_string(k / (size_t)N) + ", env " + std::to_string(k % (size_t)N) +
                                       ": a colour or checker cell size that is negative or not finite");
  return 0;
}

inline int validate_shade(bool have_colours, const void* rgba_u8, std::string* err) {
  const char* who = "raycast_shade";
  if (!have_colours) return refuse(err, who, 3, "no colours were set for this scene (mssim_raycast_set_colours comes first)");
  if (!rgba_u8) return refuse(err, who, 1, "no output");
  if ((uintptr_t)rgba_u8 & 3u) return refuse(err, who, 1, "the output must be 4-byte aligned (one store per pixel)");
  return 0;
}

}  // namespace mssim_shade

#ifdef __HIPCC__

// MESH as in k_raycast; it is also the variant that reads the per-env colours. rgba: [n_shape] float4, env_rgba:
// [slots][N] float4, env fastest (null: the shared colour in every env). out: [N][H][W] r | g << 8 | b << 16 | 255 << 24.
template <bool MESH>
__global__ __launch_bounds__(256) void k_raycast_shade(RcTables T, RcCamera C, const float* __restrict__ rigid, const float4* __restrict__ rgba,
                                                       const float4* __restrict__ env_rgba, int N, int tiles_x, int tiles, unsigned* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) rc::Staged sh[MSSIM_RAYCAST_CHUNK];
  __shared__ __attribute__((aligned(16))) float col[4 * MSSIM_RAYCAST_CHUNK];
  __shared__ float light[6];
  __shared__ __attribute__((aligned(8))) rc::MeshLevel levels[MESH ? MSSIM_RAYCAST_MESH_DEPTH * 256 : 1];  // [level][lane]
  const int env = blockIdx.x / tiles;  // block = (env, tile)
  if (env >= N) return;  // (never: the grid is N * tiles)
  const RcPixel px = rc_pixel(C, tiles_x, blockIdx.x - env * tiles);
  rc::Lit hit{rc::kInf, rc::mk(0.f, 0.f, 0.f), rc::mk(0.f, 0.f, 0.f), col};

  for (int base = 0; base < T.n_shape; base += MSSIM_RAYCAST_CHUNK) {
    const int n = min(MSSIM_RAYCAST_CHUNK, T.n_shape - base);
    if (base) __syncthreads();  // the previous chunk has been walked by every wave
    const bool stages = (int)threadIdx.x < n, lights = base == 0 && threadIdx.x == 64;
    if (stages || lights) {
      const rc::xf cam = rc_camera(C, rigid, N, env);
      if (lights) {
        rc::lights(cam, light);
      } else {
        const int i = base + threadIdx.x;
        int slot;
        sh[threadIdx.x] = rc_stage_shape<MESH>(T, cam, rigid, N, env, i, &slot);
        float4 c = rgba[i];
        if (MESH && slot >= 0 && env_rgba) c = env_rgba[(size_t)slot * N + env];
        *reinterpret_cast<float4*>(col + 4 * threadIdx.x) = c;
      }
    }
    __syncthreads();
    rc::trace<MESH>(sh, n, T.plane, px.xcv, px.ycv, C.near, C.tmax, px.live, &hit, T.tri_bvh, T.tri_soup, levels + (MESH ? threadIdx.x : 0), 256);
  }
  if (!px.live) return;
  out[((size_t)env * C.height + px.v) * C.width + px.u] = hit.t < rc::kInf ? rc::shade(hit.n, hit.a, light) : rc::kBackground;
}

extern "C" {

int mssim_raycast_set_colours(mssim_handle h, int32_t id, const float* shape_rgba, const float* env_shape_rgba) {
  if (!h) return 1;
  if (id < 0 || id >= (int)h->raycasts.size() || !h->raycasts[id]) { h->err = "raycast_set_colours: bad id"; return 1; }
  RcObject& o = *h->raycasts[id];
  if (int rc = mssim_shade::validate_colours(shape_rgba, o.T.n_shape, env_shape_rgba, o.n_env_shape, h->N, &h->err)) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  const size_t n = 4 * (size_t)o.T.n_shape, ne = 4 * (size_t)o.n_env_shape * (size_t)h->N;
  // a launch that reads the tables of an earlier call may still be under way
  HIPCHK(h, hipDeviceSynchronize());
  if (!o.rgba)
    if (int rc = rc_upload(h, &o, shape_rgba, n, &o.rgba)) return rc;
  if (n > 0) HIPCHK(h, hipMemcpy((void*)o.rgba, shape_rgba, n * sizeof(float), hipMemcpyHostToDevice));
  if (env_shape_rgba) {
    if (!o.env_rgba_store)
      if (int rc = rc_upload(h, &o, env_shape_rgba, ne, &o.env_rgba_store)) return rc;
    HIPCHK(h, hipMemcpy((void*)o.env_rgba_store, env_shape_rgba, ne * sizeof(float), hipMemcpyHostToDevice));
  }
  o.env_rgba = env_shape_rgba ? o.env_rgba_store : nullptr;
  return 0;
}

int mssim_raycast_shade(mssim_handle h, int32_t id, int32_t camera, uint8_t* rgba_u8, void* stream) {
  if (!h) return 1;
  settle(h, (hipStream_t)stream);
  RcTarget at;
  if (int rc = rc_target(h, "raycast_shade", id, camera, &at)) return rc;
  const RcObject& o = *at.o;
  if (int rc = mssim_shade::validate_shade(o.rgba != nullptr, rgba_u8, &h->err)) return rc;
  const auto kernel = (o.mesh || o.env_rgba) ? k_raycast_shade<true> : k_raycast_shade<false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)(at.tiles * h->N)), dim3(256), 0, (hipStream_t)stream, o.T, *at.C, h->buf.rigid_body_data,
                     (const float4*)o.rgba, (const float4*)o.env_rgba, h->N, at.tiles_x, at.tiles, (unsigned*)rgba_u8);
  HIPCHK(h, hipGetLastError());
  return 0;
}

}  // extern "C"

#endif  // __HIPCC__
