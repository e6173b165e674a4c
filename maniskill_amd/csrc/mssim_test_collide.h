// mssim_test_collide.h -- test hook (not part of the mssim ABI, not in include/mssim.h): the manifold generators of the
// control-step kernel on a batch of explicit shape pairs, one routine and one pair at a time.
//
// k_test_collide calls the device functions that k_solve16 calls -- collide_plane, collide_box_box<16>, collide_box_box_coop,
// collide_plane_hull_coop, collide_mpr_t with SupDirect and with SupCoop16 -- with the lane and scratch layout of the stage
// that uses them, and writes what they return. It is the counterpart of the oracle's mssim_ref_test_collide.
//
//   path 0  one pair per lane (stage A): collide_plane (a hull has no routine here), collide_box_box<16> with its clip scratch
//           as one column per lane of a 16-lane group, otherwise collide_mpr (SupDirect)
//   path 1  one pair per 16-lane group (stages B and C), the four groups of a wave loop over the batch: collide_box_box_coop,
//           collide_plane_hull_coop, otherwise collide_mpr_t with SupCoop16 (a plane against a primitive has no routine here)
//   path 2  collide_mpr (SupDirect) per lane for every pair: the oracle's `force_mpr`
//
// Out of scope: the triangle stage, the persistent-manifold cache and its growth queries, the patch reduction.
#pragma once

MS_DEV shape_t tc_shape(int type, const float* __restrict__ pose, const float* __restrict__ prm, int first, int count, const float* __restrict__ verts) {
  shape_t s;
  s.type = type;
  s.c = f3{pose[0], pose[1], pose[2]};
  s.rot = qmat(qnormalized(q4{pose[3], pose[4], pose[5], pose[6]}));
  s.p0 = prm[0]; s.p1 = prm[1]; s.p2 = prm[2];
  s.verts = verts + 3 * (size_t)first;
  s.nverts = count;
  return s;
}
MS_DEV void tc_store(float* __restrict__ o, const manifold_t& m) {
  o[0] = (float)m.count;
  o[1] = m.n.x; o[2] = m.n.y; o[3] = m.n.z;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const bool g = k < m.count;
    o[4 + 4 * k] = g ? m.x[k].x : 0.f; o[5 + 4 * k] = g ? m.x[k].y : 0.f; o[6 + 4 * k] = g ? m.x[k].z : 0.f; o[7 + 4 * k] = g ? m.sep[k] : 0.f;
  }
}

// type [n][2], pose [n][2][7], param [n][2][4], hull [n][2][2] (first vertex, count), out [n][20]
__global__ __launch_bounds__(64) void k_test_collide(int n, const int* __restrict__ type, const float* __restrict__ pose, const float* __restrict__ param,
                                                     const int* __restrict__ hull, const float* __restrict__ verts, float offset, int path, float* __restrict__ out) {
  __shared__ float clip[4][CLIP_SLOTS * 16];  // path 0: the clip scratch of a group's lanes, [slot][16 lanes]
  __shared__ float bscr[4][24];               // path 1: polygon scatter / gather words of the group
  __shared__ float bout[4][20];               // path 1: the group's manifold
  const int lane = threadIdx.x, g = lane >> 4, c = lane & 15;
  auto shapes = [&](int i, shape_t& A, shape_t& B) __attribute__((always_inline)) {
    A = tc_shape(type[2 * i], pose + 14 * (size_t)i, param + 8 * (size_t)i, hull[4 * i], hull[4 * i + 1], verts);
    B = tc_shape(type[2 * i + 1], pose + 14 * (size_t)i + 7, param + 8 * (size_t)i + 4, hull[4 * i + 2], hull[4 * i + 3], verts);
  };
  if (path != 1) {
    const int i = blockIdx.x * 64 + lane;
    if (i >= n) return;
    shape_t A, B;
    shapes(i, A, B);
    manifold_t m;
    manifold_clear(m);
    if (path == 2) collide_mpr(A, B, offset, m);
    else if (A.type == SH_PLANE) collide_plane(A, B, offset, m);
    else if (A.type == SH_BOX && B.type == SH_BOX) collide_box_box<16>(A, B, offset, m, clip[g] + c);
    else collide_mpr(A, B, offset, m);
    tc_store(out + 20 * (size_t)i, m);
    return;
  }
  for (int i = blockIdx.x * 4 + g; i < n; i += gridDim.x * 4) {  // (group-uniform: the 16 lanes stay converged)
    shape_t A, B;
    shapes(i, A, B);
    float* o = out + 20 * (size_t)i;
    const bool ph = A.type == SH_PLANE, bb = A.type == SH_BOX && B.type == SH_BOX;
    if (ph || bb) {
      float* og = bout[g];
      og[c] = 0.f;
      if (c < 4) og[16 + c] = 0.f;
      WSYNC();
      if (ph) collide_plane_hull_coop(A, B, offset, og, c, g);
      else collide_box_box_coop(A, B, offset, bscr[g], og, c, g);
      WSYNC();
      const int cnt = __float_as_int(og[0]);
      o[c] = c == 0 ? (float)cnt : ((c < 4 || c < 4 + 4 * cnt) ? og[c] : 0.f);
      if (c < 4) o[16 + c] = 16 + c < 4 + 4 * cnt ? og[16 + c] : 0.f;
      WSYNC();
    } else {
      SupCoop16 sup;
      sup.c = c;
      SupCoop16::load_one(sup.va, A, c);
      SupCoop16::load_one(sup.vb, B, c);
      manifold_t m;
      collide_mpr_t(A, B, offset, m, sup);
      if (c == 0) tc_store(o, m);
    }
  }
}

// Validates the whole batch on the host (the type and hull tables are copied back) before anything is launched: no launch can
// read outside the arrays it is given. Returns 0, or non-zero with the reason in mssim_last_error(NULL).
// `verts`: [n_verts][3], every hull starting on a multiple of 8 vertices and padded to a multiple of 8 with copies of its
// vertex 0, as the model packer lays them out (support() reads them as float4).
extern "C" int mssim_test_collide(int32_t n, const int32_t* type, const float* pose, const float* param, const int32_t* hull, const float* verts,
                                  int32_t n_verts, float offset, int32_t path, float* out, void* stream) {
  auto fail = [](const std::string& why) { g_create_error = "mssim_test_collide: " + why; return 1; };
  if (n < 0 || n > (1 << 20)) return fail("batch size out of range");
  if (path < 0 || path > 2) return fail("unknown path");
  if (!(offset >= 0.f) || !std::isfinite(offset)) return fail("contact offset must be finite and >= 0");
  if (n == 0) return 0;
  if (!type || !pose || !param || !hull || !out) return fail("null array");
  if (n_verts < 0 || (n_verts > 0 && !verts)) return fail("bad vertex buffer");
  if (reinterpret_cast<uintptr_t>(verts) % 16 != 0) return fail("vertex buffer not 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  std::vector<int32_t> ht(2 * (size_t)n), hh(4 * (size_t)n);
  if (hipStreamSynchronize(st) != hipSuccess || hipMemcpy(ht.data(), type, sizeof(int32_t) * ht.size(), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(hh.data(), hull, sizeof(int32_t) * hh.size(), hipMemcpyDeviceToHost) != hipSuccess)
    return fail("cannot read the type / hull tables back");
  for (int i = 0; i < n; i++) {
    const int ta = ht[2 * i], tb = ht[2 * i + 1];
    const std::string at = " (pair " + std::to_string(i) + ")";
    if (ta < SH_PLANE || ta > SH_CONVEX || tb <= SH_PLANE || tb > SH_CONVEX) return fail("shape type out of range" + at);
    for (int k = 0; k < 2; k++) {
      if (ht[2 * i + k] != SH_CONVEX) continue;
      const long long first = hh[4 * i + 2 * k], cnt = hh[4 * i + 2 * k + 1];
      if (cnt < 1 || cnt > MSSIM_MAX_HULL_VERTS) return fail("hull vertex count out of range" + at);
      if (first < 0 || first % 8 != 0) return fail("hull does not start on a multiple of 8 vertices" + at);
      if (first + (cnt + 7) / 8 * 8 > n_verts) return fail("hull runs past the vertex buffer" + at);
    }
    const bool plane = ta == SH_PLANE, hullb = tb == SH_CONVEX;
    if (path == 0 && plane && hullb) return fail("(plane, hull) has no per-lane routine" + at);
    if (path == 1 && plane && !hullb) return fail("(plane, primitive) has no 16-lane routine" + at);
    if (path == 2 && plane) return fail("a plane cannot go through MPR" + at);
  }
  const unsigned blocks = path == 1 ? (unsigned)std::min((n + 3) / 4, 1024) : (unsigned)((n + 63) / 64);
  hipLaunchKernelGGL(k_test_collide, dim3(blocks), dim3(64), 0, st, (int)n, type, pose, param, hull, verts, offset, (int)path, out);
  if (hipGetLastError() != hipSuccess) return fail("launch failed");
  return 0;
}
