// mssim_raycast_dots.h -- a dot layer composited over the shaded view (include/mssim_hip_tasks.h, mssim_raycast_draw_dots):
// the drawing of DrawTriangle-style tasks. Included by mssim_kernels.hip after mssim_raycast_shade.h. The dots are not
// shapes of the scene -- up to 300 per env, a table the task epilogue appends to -- so k_raycast and k_raycast_shade are
// not touched: this is a launch of its own over the picture k_raycast_shade wrote, with the float depth k_raycast wrote for
// the same scene, camera and state deciding what hides a dot.
//
// k_raycast_dots has their shape: one block per 16 x 16 tile of one env, one lane per pixel (rc_pixel). Lane 0 stages the
// plane z = D.z as a shape frame (rc::stage: the camera's pose composed in double, rounded once), the block copies the
// env's drawn dots into LDS (a dot that is not drawn becomes a NaN, which no comparison passes), then every lane meets its
// ray with the plane and tests the point against the dots. A pixel is painted where the point lies on a disc and the scene
// has nothing more than a millimetre nearer; every other pixel keeps what it had. One 4-byte store per painted pixel.
#pragma once

#include <cstdint>
#include <string>

#include "mssim_raycast_shade.h"

#define MSSIM_DOT_LAYER_MAX 1024  // dots per env the kernel's LDS table holds

namespace mssim_dots {

constexpr float kOcclusionMargin = 1e-3f;  // metres of z-depth: the canvas under a dot is not "in front of" it

// 0 = accepted (plain C++: no device is touched)
inline int validate(const mssim_dot_layer* layer, const float* depth_f32, const void* rgba_u8, std::string* err) {
  const char* who = "raycast_draw_dots";
  if (!layer || !layer->dots || !layer->dot_near || !layer->count) return mssim_shade::refuse(err, who, 1, "no dot tables");
  if (layer->max_dots < 1 || layer->max_dots > MSSIM_DOT_LAYER_MAX) return mssim_shade::refuse(err, who, 2, "max_dots outside [1, " + std::to_string(MSSIM_DOT_LAYER_MAX) + "]");
  if (!(layer->radius > 0.f)) return mssim_shade::refuse(err, who, 2, "the radius must be positive");
  if (!depth_f32) return mssim_shade::refuse(err, who, 1, "no depth (mssim_raycast_render's depth_f32 of the same camera)");
  if (!rgba_u8) return mssim_shade::refuse(err, who, 1, "no picture");
  if ((uintptr_t)rgba_u8 & 3u) return mssim_shade::refuse(err, who, 1, "the picture must be 4-byte aligned (one store per pixel)");
  return 0;
}

}  // namespace mssim_dots

#ifdef __HIPCC__

__global__ __launch_bounds__(256) void k_raycast_dots(RcCamera C, const float* __restrict__ rigid, mssim_dot_layer D, const float* __restrict__ depth, int N,
                                                      int tiles_x, int tiles, unsigned* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) rc::Staged plane;
  __shared__ float2 dots[MSSIM_DOT_LAYER_MAX];
  const int env = blockIdx.x / tiles;  // block = (env, tile)
  if (env >= N) return;  // (never: the grid is N * tiles)
  const int n = min(max(D.count[env], 0), D.max_dots);
  if (n == 0) return;  // (the whole block: nothing was drawn in this env)
  const RcPixel px = rc_pixel(C, tiles_x, blockIdx.x - env * tiles);
  if (threadIdx.x == 0) {
    const float none[3] = {0.f, 0.f, 0.f};
    const rc::p3 at{0.0, 0.0, (double)D.z};
    plane = rc::stage(rc_camera(C, rigid, N, env), rc::xf{at, rc::q4{1.0, 0.0, 0.0, 0.0}}, at, -1.f, MSSIM_SHAPE_NONE, none, 0, 0, 0);
  }
  for (int i = threadIdx.x; i < n; i += 256) {
    const size_t at = (size_t)env * D.max_dots + i;
    dots[i] = D.dot_near[at] >= 0 ? make_float2(D.dots[2 * at], D.dots[2 * at + 1]) : make_float2(NAN, NAN);
  }
  __syncthreads();
  if (!px.live) return;
  // the ray in the plane's frame (the env's axes, the origin at height z): it has to come down from above
  const float dz = plane.r2[0] * px.xcv + plane.r2[1] * px.ycv + plane.r2[2];
  if (!(plane.oz > 0.f && dz < 0.f)) return;
  const float t = -plane.oz / dz;
  if (!(t >= C.near && t <= C.tmax)) return;
  const size_t pix = ((size_t)env * C.height + px.v) * C.width + px.u;
  const float seen = depth[pix];
  if (seen != 0.f && !(t <= seen + mssim_dots::kOcclusionMargin)) return;
  const float x = plane.ox + t * (plane.r0[0] * px.xcv + plane.r0[1] * px.ycv + plane.r0[2]);
  const float y = plane.oy + t * (plane.r1[0] * px.xcv + plane.r1[1] * px.ycv + plane.r1[2]);
  const float r2 = D.radius * D.radius;
  bool on = false;
  for (int i = 0; i < n; i++) {
    const float ex = x - dots[i].x, ey = y - dots[i].y;  // (one address per wave: a broadcast)
    on = on || ex * ex + ey * ey <= r2;
  }
  if (on) out[pix] = D.rgba;
}

extern "C" {

int mssim_raycast_draw_dots(mssim_handle h, int32_t id, int32_t camera, const mssim_dot_layer* layer, const float* depth_f32, uint8_t* rgba_u8, void* stream) {
  if (!h) return 1;
  settle(h, (hipStream_t)stream);
  RcTarget at;
  if (int rc = rc_target(h, "raycast_draw_dots", id, camera, &at)) return rc;
  if (int rc = mssim_dots::validate(layer, depth_f32, rgba_u8, &h->err)) return rc;
  hipLaunchKernelGGL(k_raycast_dots, dim3((unsigned)(at.tiles * h->N)), dim3(256), 0, (hipStream_t)stream, *at.C, h->buf.rigid_body_data, *layer, depth_f32, h->N,
                     at.tiles_x, at.tiles, (unsigned*)rgba_u8);
  HIPCHK(h, hipGetLastError());
  return 0;
}

}  // extern "C"

#endif  // __HIPCC__
