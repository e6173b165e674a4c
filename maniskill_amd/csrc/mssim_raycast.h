// mssim_raycast.h -- the ray caster behind the depth / segmentation / position camera observations
// (include/mssim_hip_tasks.h, mssim_raycast_*). Included by mssim_kernels.hip after mssim_sim is defined.
//
// One block of 256 lanes renders a 16 x 16 tile of one (env, camera); each wave owns an 8 x 8 quadrant, each lane one
// pixel. The block first stages the env's shapes in LDS in the CAMERA's frame, MSSIM_RAYCAST_CHUNK at a time (one lane per
// shape: body pose from rigid_body_data, per-env overrides, the camera's pose -- read once per block, not once per ray):
// 6 x 16 B per shape, read back with one address per wave (a broadcast). Every lane then walks the staged list; a
// shape is skipped by its bounding sphere, by the whole wave when no lane's ray meets the sphere. A hull's planes are
// read from global memory at addresses that are the same in every lane. No atomics: one lane writes each pixel, with one
// 8-byte store (and one 4-byte store for the float depth), so a render is deterministic. The shaded view
// (mssim_raycast_shade.h, k_raycast_shade) stages and walks with the routines of this file -- rc_stage_shape, rc::trace -- and
// keeps another hit record: what either kernel has in front of a pixel is decided here, once.
//
// Triangle meshes (k_raycast<true>, chosen at create for a scene that holds one, or per-env plane ranges or ids, which
// that instance alone reads while staging; k_raycast<false> is the kernel without any of them, register for register): a staged mesh passes the same bounding-sphere reject, then each lane walks the mesh's 16-wide BVH for its own ray,
// depth first: at a node it tests the 16 child boxes (slabs, against [near, nearest hit so far]) into a 16-bit mask and
// takes the children in index order; a leaf child is one triangle, intersected two-sided from its centroid and relative
// corners (rc::triangle). A level's (node, children still to visit) waits in LDS while the lane is below it -- one 8-byte
// word per lane and level, [level][lane] so that a wave's access is one contiguous 512 B --: no per-lane array, no
// scratch. Node and triangle data are read from global memory; the rays of a wave are neighbours and mostly ask for the
// same nodes, which the caches serve. mssim_raycast::validate bounds a mesh's depth by MSSIM_RAYCAST_MESH_DEPTH.
//
// The arithmetic (namespace rc) is plain C++ under RC_HD, so that a host build can run it too.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#ifdef __HIPCC__
#define RC_HD __host__ __device__ __forceinline__
#else
#define RC_HD inline
#endif

namespace rc {

template <class T> struct V3 { T x, y, z; };
template <class T> RC_HD V3<T> operator+(V3<T> a, V3<T> b) { return V3<T>{a.x + b.x, a.y + b.y, a.z + b.z}; }
template <class T> RC_HD V3<T> operator-(V3<T> a, V3<T> b) { return V3<T>{a.x - b.x, a.y - b.y, a.z - b.z}; }
template <class T> RC_HD V3<T> operator*(T s, V3<T> a) { return V3<T>{s * a.x, s * a.y, s * a.z}; }
template <class T> RC_HD T dot(V3<T> a, V3<T> b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
using v3 = V3<float>;  // the per-ray arithmetic is float
RC_HD v3 mk(float x, float y, float z) { return v3{x, y, z}; }

// Poses are composed in double while the shapes are staged (once per block and shape, a few hundred operations), so that
// what the rays see -- one rotation matrix and one origin per shape -- is rounded to float once, not once per link of the
// chain camera <- mount <- env <- body <- shape.
using real = double;
using p3 = V3<real>;
struct q4 { real w, x, y, z; };
struct xf { p3 p; q4 q; };  // pose: x_parent = p + rot(q) x

RC_HD q4 qnorm(q4 q) {
  const real n = sqrt(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);
  if (!(n > 0.0)) return q4{1.0, 0.0, 0.0, 0.0};
  const real s = 1.0 / n;
  return q4{q.w * s, q.x * s, q.y * s, q.z * s};
}
RC_HD q4 qmul(q4 a, q4 b) {
  return q4{a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z, a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
            a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x, a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w};
}
RC_HD q4 qconj(q4 q) { return q4{q.w, -q.x, -q.y, -q.z}; }
RC_HD p3 qrot(q4 q, p3 v) {  // v + 2 w (u x v) + 2 u x (u x v)
  const p3 u{q.x, q.y, q.z};
  const p3 c{u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x};
  const p3 cc{u.y * c.z - u.z * c.y, u.z * c.x - u.x * c.z, u.x * c.y - u.y * c.x};
  return v + real(2) * (q.w * c + cc);
}
RC_HD xf compose(xf a, xf b) { return xf{a.p + qrot(a.q, b.p), qmul(a.q, b.q)}; }  // a o b
RC_HD xf inverse(xf a) { const q4 c = qconj(a.q); return xf{real(-1) * qrot(c, a.p), c}; }
RC_HD xf load_xf(const float* p, size_t stride) {
  return xf{p3{p[0], p[stride], p[2 * stride]}, qnorm(q4{p[3 * stride], p[4 * stride], p[5 * stride], p[6 * stride]})};
}

// a staged shape: the map camera (OpenCV axes) -> shape frame as rows of a matrix plus the camera's origin in the
// shape frame, the bounding sphere in the camera frame, type, parameters, id, plane range. 6 x 16 B.
struct Staged {
  float r0[3], ox, r1[3], oy, r2[3], oz;  // p_shape = (r0 . p_cv + ox, r1 . p_cv + oy, r2 . p_cv + oz)
  float bc[3], br;                        // bounding sphere, camera (OpenCV) frame; br < 0: unbounded
  float p[3]; int type;
  int seg, pl0, pln, pad;
};
static_assert(sizeof(Staged) == 96, "Staged is six 16-byte words");

// rows of the rotation matrix of q
RC_HD void qrows(q4 q, p3* r0, p3* r1, p3* r2) {
  const real xx = q.x * q.x, yy = q.y * q.y, zz = q.z * q.z, xy = q.x * q.y, xz = q.x * q.z, yz = q.y * q.z, wx = q.w * q.x, wy = q.w * q.y, wz = q.w * q.z;
  *r0 = p3{1.0 - 2.0 * (yy + zz), 2.0 * (xy - wz), 2.0 * (xz + wy)};
  *r1 = p3{2.0 * (xy + wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz - wx)};
  *r2 = p3{2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (xx + yy)};
}

// stage one shape: `cam` = env frame <- camera (SAPIEN axes), `shape` = env frame <- shape frame, bound centre `bc_env`
// in the env frame. A SAPIEN-axes point is (z_cv, -x_cv, -y_cv) of its OpenCV coordinates.
RC_HD Staged stage(xf cam, xf shape, p3 bc_env, float br, int type, const float* param, int seg, int pl0, int pln) {
  const xf sc = compose(inverse(shape), cam);  // shape <- camera (SAPIEN axes)
  p3 a0, a1, a2;
  qrows(sc.q, &a0, &a1, &a2);
  Staged s;
  // columns: x_cv -> -(SAPIEN y), y_cv -> -(SAPIEN z), z_cv -> SAPIEN x
  s.r0[0] = (float)-a0.y; s.r0[1] = (float)-a0.z; s.r0[2] = (float)a0.x; s.ox = (float)sc.p.x;
  s.r1[0] = (float)-a1.y; s.r1[1] = (float)-a1.z; s.r1[2] = (float)a1.x; s.oy = (float)sc.p.y;
  s.r2[0] = (float)-a2.y; s.r2[1] = (float)-a2.z; s.r2[2] = (float)a2.x; s.oz = (float)sc.p.z;
  const xf ci = inverse(cam);
  const p3 b = ci.p + qrot(ci.q, bc_env);  // camera, SAPIEN axes
  s.bc[0] = (float)-b.y; s.bc[1] = (float)-b.z; s.bc[2] = (float)b.x; s.br = br;
  s.p[0] = param[0]; s.p[1] = param[1]; s.p[2] = param[2];
  s.type = type; s.seg = seg; s.pl0 = pl0; s.pln = pln; s.pad = 0;
  return s;
}

constexpr float kInf = INFINITY;

// the slab |x| <= h along one axis: narrows [*tin, *tout]; true where it raised *tin (strictly: on a tie the earlier slab
// keeps the entry)
RC_HD bool slab(float o, float d, float h, float* tin, float* tout) {
  if (d == 0.f) {
    if (fabsf(o) > h) { *tin = kInf; *tout = -kInf; }
    return false;
  }
  const float inv = 1.f / d;
  const float t1 = (-h - o) * inv, t2 = (h - o) * inv;
  const float lo = fminf(t1, t2);
  const bool sets = lo > *tin;
  *tin = fmaxf(*tin, lo);
  *tout = fminf(*tout, fmaxf(t1, t2));
  return sets;
}

// the ball of radius r about the origin (`oc`: the ray's start relative to the centre): interval of the line oc + t d
// inside it, from the foot of the perpendicular (well conditioned where the line passes close to the centre). With the
// x components zeroed this is the side of a cylinder about +x.
RC_HD void ball(v3 oc, v3 d, float r, float* tin, float* tout) {
  const float a = dot(d, d);
  if (a == 0.f) {  // (a ray along the axis of a cylinder: inside the side for all t, or never)
    if (dot(oc, oc) > r * r) { *tin = kInf; *tout = -kInf; } else { *tin = -kInf; *tout = kInf; }
    return;
  }
  const float tm = -dot(oc, d) / a;  // parameter of the closest point
  const v3 l = oc + tm * d;         // closest point, relative to the centre
  const float h2 = r * r - dot(l, l);
  if (h2 < 0.f) { *tin = kInf; *tout = -kInf; return; }
  const float half = sqrtf(h2 / a);
  *tin = tm - half;
  *tout = tm + half;
}

// [tin, tout] of a cylinder of radius r and half length h about +x; *face = 1 where the cap slab set the entry, else 0 (the side)
RC_HD void cylinder(v3 o, v3 d, float r, float h, float* tin, float* tout, int* face) {
  ball(mk(0.f, o.y, o.z), mk(0.f, d.y, d.z), r, tin, tout);
  *face = slab(o.x, d.x, h, tin, tout) ? 1 : 0;
}

// entry parameter of the ray (o, d) into the shape, in the shape's frame; +inf: the line misses it. An entry < 0 means
// the start is inside or the shape lies behind: the caller's `near` test drops both. *face names the FACE entered, one
// integer from which the shaded view works out a normal where it needs one (the depth kernel never reads it, and it folds
// away there):
//   box 0 / 1 / 2: the axis whose slab set the entry, the lowest on a tie; cylinder 0 side, 1 cap; capsule 0 / 1 its
//   cylinder's side / cap, 2 the ball at -x, 3 at +x, whichever gave the earliest entry (cylinder first on a tie); hull: the
//   first plane, by index in its range, that set tin; plane, sphere: 0
RC_HD float enter(int type, const float* p, v3 o, v3 d, const float* __restrict__ planes, int pl0, int pln, int* face) {
  float tin = -kInf, tout = kInf;
  *face = 0;
  switch (type) {
    case MSSIM_SHAPE_PLANE:  // solid: x <= 0
      if (!(d.x < 0.f)) return kInf;
      return -o.x / d.x;
    case MSSIM_SHAPE_BOX:
      slab(o.x, d.x, p[0], &tin, &tout);
      if (slab(o.y, d.y, p[1], &tin, &tout)) *face = 1;
      if (slab(o.z, d.z, p[2], &tin, &tout)) *face = 2;
      break;
    case MSSIM_SHAPE_SPHERE:
      ball(o, d, p[0], &tin, &tout);
      break;
    case MSSIM_SHAPE_CYLINDER:
      cylinder(o, d, p[0], p[1], &tin, &tout, face);
      break;
    case MSSIM_SHAPE_CAPSULE: {  // the union of a cylinder and two balls, itself convex: the earliest entry of the three
      float best = kInf;
      int f = 0;
      cylinder(o, d, p[0], p[1], &tin, &tout, &f);
      if (tin <= tout) { best = tin; *face = f; }
      for (int k = 0; k < 2; k++) {
        const float cx = k ? p[1] : -p[1];
        ball(mk(o.x - cx, o.y, o.z), d, p[0], &tin, &tout);
        // (fminf(best, tin) but for the sign of a zero, and a zero entry is below every `near`)
        if (tin <= tout && tin < best) { best = tin; *face = 2 + k; }
      }
      return best;
    }
    case MSSIM_SHAPE_CONVEX:
      for (int k = 0; k < pln; k++) {
        const float* pl = planes + 4 * (size_t)(pl0 + k);
        const v3 n = mk(pl[0], pl[1], pl[2]);
        const float nd = dot(n, d), dist = pl[3] - dot(n, o);  // dist >= 0: the start is on the inner side
        if (nd == 0.f) {
          if (dist < 0.f) return kInf;
          continue;
        }
        const float t = dist / nd;
        if (nd < 0.f) {
          if (t > tin) *face = k;  // (strictly: the first plane in index order keeps the entry)
          tin = fmaxf(tin, t);
        } else {
          tout = fminf(tout, t);
        }
      }
      break;
    default:
      return kInf;
  }
  return tin <= tout ? tin : kInf;
}


// ---- triangle meshes (include/mssim_hip_tasks.h: a surface of two-sided triangles, inclusive edges) ----
// Barycentric slack of the edge tests: a triangle counts as hit up to this far (in units of its own edges) outside it, so
// that the float roundings of two triangles that share an edge cannot open a crack between them. 1e-5 of an edge -- 10
// micrometres on a metre -- is a hundred float roundings and far less than a pixel anywhere.
constexpr float kTriSlack = 1e-5f;

// parameter of the ray (oc + t d, oc relative to the centroid) where it meets the triangle with corners a, b, c relative
// to the centroid, from either side; +inf: no hit (outside, or the ray lies in the triangle's plane)
RC_HD float triangle(v3 oc, v3 d, v3 a, v3 b, v3 c) {
  const v3 e1 = b - a, e2 = c - a, s = oc - a;
  const v3 p = mk(d.y * e2.z - d.z * e2.y, d.z * e2.x - d.x * e2.z, d.x * e2.y - d.y * e2.x);  // d x e2
  const float det = dot(e1, p);
  if (det == 0.f) return kInf;
  const float inv = 1.f / det;
  const float u = dot(s, p) * inv;
  const v3 q = mk(s.y * e1.z - s.z * e1.y, s.z * e1.x - s.x * e1.z, s.x * e1.y - s.y * e1.x);  // s x e1
  const float v = dot(d, q) * inv;
  if (!(u >= -kTriSlack && v >= -kTriSlack && u + v <= 1.f + kTriSlack)) return kInf;
  return dot(e2, q) * inv;
}

// which of a node's 16 child boxes the ray meets within [lo, hi]: bit c = child c. The boxes bound the corners exactly
// (model/mesh.py builds them from the float corners), the slab arithmetic rounds: a relative slack on the interval keeps
// a flat box -- an axis-aligned triangle's -- from slipping between two roundings. `inv` = 1 / d per axis (+-inf where
// d is 0: a NaN from 0 x inf is dropped by fminf / fmaxf, which reads as "inside the slab", the safe side).
RC_HD unsigned node_mask(const float* __restrict__ node, v3 o, v3 inv, float lo, float hi) {
  unsigned mask = 0u;
  for (int c = 0; c < 16; c++) {
    const float* b = node + 6 * c;
    if (!(b[0] <= b[3])) continue;  // no child
    const float x1 = (b[0] - o.x) * inv.x, x2 = (b[3] - o.x) * inv.x;
    const float y1 = (b[1] - o.y) * inv.y, y2 = (b[4] - o.y) * inv.y;
    const float z1 = (b[2] - o.z) * inv.z, z2 = (b[5] - o.z) * inv.z;
    const float tin = fmaxf(fmaxf(fminf(x1, x2), fminf(y1, y2)), fmaxf(fminf(z1, z2), lo));
    const float tout = fminf(fminf(fmaxf(x1, x2), fmaxf(y1, y2)), fminf(fmaxf(z1, z2), hi));
    if (tin <= tout + 4e-6f * (fabsf(tin) + fabsf(tout)) + 1e-7f) mask |= 1u << c;
  }
  return mask;
}

struct MeshLevel { int node; unsigned mask; };  // a level of the walk: the node and its children still to visit

// smallest t in [near, tmax] below `best` over the triangles of the mesh under `root` (shape frame: o, d); +inf where
// there is none. *tri = index in `soup` of the triangle that gave the returned t (untouched on a miss). `stack` holds
// MSSIM_RAYCAST_MESH_DEPTH levels, `stride` elements apart.
RC_HD float mesh_hit(const float* __restrict__ bvh, const float* __restrict__ soup, int root, v3 o, v3 d, float near, float tmax, float best,
                     MeshLevel* stack, int stride, int* tri) {
  const v3 inv = mk(1.f / d.x, 1.f / d.y, 1.f / d.z);
  best = fminf(best, tmax);
  bool found = false;
  int sp = 0, node = root;
  unsigned mask = node_mask(bvh + (size_t)node * 112, o, inv, near, best);
  for (;;) {
    if (mask == 0u) {
      if (sp == 0) break;
      sp--;
      node = stack[sp * stride].node; mask = stack[sp * stride].mask;
      continue;
    }
    const int c = __builtin_ctz(mask);
    mask &= mask - 1u;
    const float* nd = bvh + (size_t)node * 112;
    int ref;
#ifdef __HIP_DEVICE_COMPILE__
    ref = __float_as_int(nd[96 + c]);
#else
    memcpy(&ref, nd + 96 + c, 4);
#endif
    if (ref < 0) {
      const float* q = soup + (size_t)(~ref) * 12;
      const float t = triangle(mk(o.x - q[0], o.y - q[1], o.z - q[2]), d, mk(q[3], q[4], q[5]), mk(q[6], q[7], q[8]), mk(q[9], q[10], q[11]));
      if (t >= near && t <= tmax && (found ? t < best : t <= best)) { best = t; found = true; *tri = ~ref; }
      continue;
    }
    if (mask != 0u) {
      if (sp == MSSIM_RAYCAST_MESH_DEPTH) continue;  // (never: validate bounds the depth; a deeper branch is left out, not overrun)
      stack[sp * stride].node = node; stack[sp * stride].mask = mask;
      sp++;
    }
    node = ref;
    mask = node_mask(bvh + (size_t)node * 112, o, inv, near, best);
  }
  return found ? best : kInf;
}

// the nearest hit so far, as the depth kernel keeps it: parameter and id. A hit record has `t` and take(), which trace
// calls on an improving hit with all it knows about it (rc::Lit of the shaded view keeps a normal and a colour instead).
struct Hit {
  float t; int seg;
  RC_HD void take(const Staged& s, int, v3, v3, float t_, int, bool, const float*, const float*) { t = t_; seg = s.seg; }
};

// one pixel's ray (x_cv, y_cv, 1) against staged shapes [0, n): improves `hit` (strictly smaller t only) through
// hit->take(shape, its index in sh, o, d, t, face -- of a mesh: the triangle --, whether it is a mesh, planes, soup). MESH: a
// staged TRIMESH shape (pl0 = its root node) is walked through `bvh` / `soup` with the lane's `stack`; without it such a
// shape is never staged (validate turns a mesh down for a scene without triangle tables, and those choose MESH).
template <bool MESH, class H>
RC_HD void trace(const Staged* __restrict__ sh, int n, const float* __restrict__ planes, float xcv, float ycv, float near, float tmax, bool live, H* hit,
                 const float* __restrict__ bvh = nullptr, const float* __restrict__ soup = nullptr, MeshLevel* stack = nullptr, int stride = 0) {
  const float dd = xcv * xcv + ycv * ycv + 1.f;
  for (int i = 0; i < n; i++) {
    const Staged& s = sh[i];
    if (s.type == MSSIM_SHAPE_NONE) continue;
    bool need = live;
    if (s.br >= 0.f) {  // |c x d|^2 <= r^2 |d|^2: the line passes within r of the centre
      const float cd = s.bc[0] * xcv + s.bc[1] * ycv + s.bc[2];
      const float cc = s.bc[0] * s.bc[0] + s.bc[1] * s.bc[1] + s.bc[2] * s.bc[2];
      // The exact test decides, this one only saves it, so it must never reject a ray that hits: a margin of a hundredth of
      // the radius and a millimetre, plus the float cancellation error of the left side, which grows with the distance -- a
      // few roundings of 6e-8 on terms of size |c|^2 |d|^2, covered 30 times over by 2e-6 |c|^2 |d|^2 (at 30 m that widens
      // a small shape's sphere by 4 cm: a few exact tests more, no hit lost).
      const float r = 1.01f * s.br + 1e-3f;
      need = need && (cc * dd - cd * cd <= (r * r + 2e-6f * cc) * dd);
    }
#ifdef __HIP_DEVICE_COMPILE__
    if (__ballot(need) == 0ull) continue;  // the whole wave skips the shape
#endif
    if (need) {
      const v3 o = mk(s.ox, s.oy, s.oz);
      const v3 d = mk(s.r0[0] * xcv + s.r0[1] * ycv + s.r0[2], s.r1[0] * xcv + s.r1[1] * ycv + s.r1[2], s.r2[0] * xcv + s.r2[1] * ycv + s.r2[2]);
      float t;
      int face = -1;
      const bool mesh = MESH && s.type == MSSIM_SHAPE_TRIMESH;
      if (mesh) t = mesh_hit(bvh, soup, s.pl0, o, d, near, tmax, hit->t, stack, stride, &face);
      else t = enter(s.type, s.p, o, d, planes, s.pl0, s.pln, &face);
      if (t >= near && t <= tmax && t < hit->t) hit->take(s, i, o, d, t, face, mesh, planes, soup);
    }
  }
}

RC_HD int mm(float metres) {  // truncated toward zero, saturated to int16
  const float v = fminf(fmaxf(1000.f * metres, -32768.f), 32767.f);
  return (int)v;
}

}  // namespace rc

#ifdef __HIPCC__

// device tables of one scene (uploaded by mssim_raycast_create)
struct RcTables {
  int n_shape;
  const int* type; const int* row; const float* frame; const float* param; const float* bound; const int* seg; const int* planes2;
  const float* plane;
  const int* env_slot; const float* env_frame; const float* env_param; const float* env_bound;  // env_slot null: no overrides
  const int* env_planes2; const int* env_seg;  // [slots * 2][N], [slots][N]; null: the shared plane range / id in every env
  const float* tri_soup; const float* tri_bvh;  // null without meshes
};

struct RcCamera {
  int width, height; float fx, fy, cx, cy, near, tmax; int mount_row; float pose[7]; const float* env_pose;
};

struct RcObject {
  RcTables T{};
  std::vector<RcCamera> cams;
  std::vector<void*> allocs;
  bool needs_rows = false;  // some shape or camera rides on a body row
  bool mesh = false;        // the scene holds a triangle mesh, per-env plane ranges or per-env ids: k_raycast<true>
  // the shaded view (mssim_raycast_shade.h): colour tables once mssim_raycast_set_colours was called, the slot count they are checked against
  int n_env_shape = 0;
  const float* rgba = nullptr; const float* env_rgba_store = nullptr; const float* env_rgba = nullptr;
  ~RcObject() { for (void* p : allocs) (void)hipFree(p); }
};

constexpr int RC_TILE = 16;

// the camera in the env frame: its pose, composed with its mount row's (the body row, read here)
__device__ __forceinline__ rc::xf rc_camera(const RcCamera& C, const float* __restrict__ rigid, int N, int env) {
  rc::xf cam = C.env_pose ? rc::load_xf(C.env_pose + 7 * (size_t)env, 1) : rc::load_xf(C.pose, 1);
  if (C.mount_row >= 0) cam = rc::compose(rc::load_xf(rigid + ((size_t)C.mount_row * N + env) * 13, 1), cam);
  return cam;
}

// shape i of the scene staged for env `env`: the shared tables, the env's own rows where the shape has a slot (*slot, -1:
// none), the body row. MESH: the env's own hull and id too (tables that only this variant reads: see RcObject::mesh)
template <bool MESH>
__device__ __forceinline__ rc::Staged rc_stage_shape(const RcTables& T, const rc::xf cam, const float* __restrict__ rigid, int N, int env, int i, int* slot_out) {
  int type = T.type[i];
  rc::xf frame = rc::load_xf(T.frame + 7 * (size_t)i, 1);
  float param[3] = {T.param[4 * i], T.param[4 * i + 1], T.param[4 * i + 2]};
  rc::p3 bc{T.bound[4 * i], T.bound[4 * i + 1], T.bound[4 * i + 2]};
  float br = T.bound[4 * i + 3];
  const int slot = T.env_slot ? T.env_slot[i] : -1;
  if (slot >= 0) {  // [items][N], env fastest
    frame = rc::load_xf(T.env_frame + (size_t)slot * 7 * N + env, (size_t)N);
    const float* ep = T.env_param + (size_t)slot * 4 * N + env;
    const float* eb = T.env_bound + (size_t)slot * 4 * N + env;
    const int t1 = (int)ep[3 * (size_t)N];
    if (t1 > 0) type = t1 - 1;
    if (type != MSSIM_SHAPE_CONVEX && !(MESH && type == MSSIM_SHAPE_TRIMESH && t1 == 0)) { param[0] = ep[0]; param[1] = ep[(size_t)N]; param[2] = ep[2 * (size_t)N]; }
    bc = rc::p3{eb[0], eb[(size_t)N], eb[2 * (size_t)N]};
    br = eb[3 * (size_t)N];
  }
  const int row = T.row[i];
  if (row >= 0) {
    const rc::xf body = rc::load_xf(rigid + ((size_t)row * N + env) * 13, 1);
    frame = rc::compose(body, frame);
    bc = body.p + rc::qrot(body.q, bc);
  }
  int seg = T.seg[i], pl0 = T.planes2[2 * i], pln = T.planes2[2 * i + 1];
  if (MESH && slot >= 0) {
    if (T.env_planes2 && type == MSSIM_SHAPE_CONVEX) { pl0 = T.env_planes2[(size_t)slot * 2 * N + env]; pln = T.env_planes2[((size_t)slot * 2 + 1) * N + env]; }
    if (T.env_seg) seg = T.env_seg[(size_t)slot * N + env];
  }
  if (MESH && type == MSSIM_SHAPE_TRIMESH) { pl0 = (int)param[2]; pln = (int)param[1]; }  // root node, triangle count
  *slot_out = slot;
  return rc::stage(cam, frame, bc, br, type, param, seg, pl0, pln);
}

// which pixel of tile `tile` a lane renders: wave w owns quadrant (w & 1, w >> 1) of the tile, lane l pixel (l & 7, l >> 3)
// of the quadrant. live: the pixel lies in the image; (xcv, ycv, 1) is its ray.
struct RcPixel { int u, v; bool live; float xcv, ycv; };
__device__ __forceinline__ RcPixel rc_pixel(const RcCamera& C, int tiles_x, int tile) {
  const int tx = tile % tiles_x, ty = tile / tiles_x;
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int u = tx * RC_TILE + (w & 1) * 8 + (l & 7), v = ty * RC_TILE + (w >> 1) * 8 + (l >> 3);
  return RcPixel{u, v, u < C.width && v < C.height, ((float)u + 0.5f - C.cx) / C.fx, ((float)v + 0.5f - C.cy) / C.fy};
}

// MESH: the scene holds triangle meshes, per-env hulls or per-env ids (see the head of this file); false is the kernel as
// it is without them
template <bool MESH>
__global__ __launch_bounds__(256) void k_raycast(RcTables T, RcCamera C, const float* __restrict__ rigid, int N, int tiles_x, int tiles,
                                                 short* __restrict__ pos_seg, float* __restrict__ depth) {
  __shared__ __attribute__((aligned(16))) rc::Staged sh[MSSIM_RAYCAST_CHUNK];
  __shared__ __attribute__((aligned(8))) rc::MeshLevel levels[MESH ? MSSIM_RAYCAST_MESH_DEPTH * 256 : 1];  // [level][lane]
  const int env = blockIdx.x / tiles;  // block = (env, tile)
  if (env >= N) return;  // (never: the grid is N * tiles)
  const RcPixel px = rc_pixel(C, tiles_x, blockIdx.x - env * tiles);
  rc::Hit hit{rc::kInf, 0};

  for (int base = 0; base < T.n_shape; base += MSSIM_RAYCAST_CHUNK) {
    const int n = min(MSSIM_RAYCAST_CHUNK, T.n_shape - base);
    if (base) __syncthreads();  // the previous chunk has been walked by every wave
    if ((int)threadIdx.x < n) {
      int slot;
      sh[threadIdx.x] = rc_stage_shape<MESH>(T, rc_camera(C, rigid, N, env), rigid, N, env, base + threadIdx.x, &slot);
    }
    __syncthreads();
    rc::trace<MESH>(sh, n, T.plane, px.xcv, px.ycv, C.near, C.tmax, px.live, &hit, T.tri_bvh, T.tri_soup, levels + (MESH ? threadIdx.x : 0), 256);
  }
  if (!px.live) return;
  const bool any = hit.t < rc::kInf;
  const float t = any ? hit.t : 0.f;
  const size_t pix = ((size_t)env * C.height + px.v) * C.width + px.u;
  const int x = rc::mm(px.xcv * t), y = rc::mm(-(px.ycv * t)), z = rc::mm(-t);
  uint2 out;
  out.x = any ? ((unsigned)x & 0xffffu) | ((unsigned)y << 16) : 0u;
  out.y = any ? ((unsigned)z & 0xffffu) | ((unsigned)hit.seg << 16) : 0u;
  *reinterpret_cast<uint2*>(pos_seg + 4 * pix) = out;  // (hipMalloc'd / torch tensors: [N][H][W][4] int16 is 8-byte aligned per pixel)
  if (depth) depth[pix] = t;
}

template <typename Tt>
static int rc_upload(mssim_handle h, RcObject* o, const Tt* src, size_t count, const Tt** dst) {
  void* d = nullptr;
  HIPCHK(h, hipMalloc(&d, (count > 0 ? count : 1) * sizeof(Tt)));
  o->allocs.push_back(d);
  if (count > 0) HIPCHK(h, hipMemcpy(d, src, count * sizeof(Tt), hipMemcpyHostToDevice));
  *dst = (const Tt*)d;
  return 0;
}

// what a render or shade call names: the scene, its camera and the camera's tile grid. Refusals carry the caller's name.
struct RcTarget { const RcObject* o; const RcCamera* C; int tiles_x, tiles; };
static int rc_target(mssim_handle h, const char* who, int32_t id, int32_t camera, RcTarget* at) {
  const auto refuse = [&](const char* msg) { h->err = std::string(who) + ": " + msg; return 1; };
  if (id < 0 || id >= (int)h->raycasts.size() || !h->raycasts[id]) return refuse("bad id");
  const RcObject& o = *h->raycasts[id];
  if (camera < 0 || camera >= (int)o.cams.size()) return refuse("bad camera index");
  if (o.needs_rows && !h->buf.rigid_body_data) return refuse("no rigid_body_data bound");
  const RcCamera& C = o.cams[camera];
  const int tiles_x = (C.width + RC_TILE - 1) / RC_TILE;
  *at = RcTarget{&o, &C, tiles_x, tiles_x * ((C.height + RC_TILE - 1) / RC_TILE)};
  return 0;
}

extern "C" {

int mssim_raycast_create(mssim_handle h, const mssim_raycast_scene* s, const mssim_camera_desc* cameras, int32_t n_cameras, int32_t* id) {
  if (!h) return 1;
  if (!id) { h->err = "raycast_create: no id"; return 1; }
  const int N = h->N, n_rows = h->M.n_link + h->M.n_free + h->M.n_kin;
  if (int rc = mssim_raycast::validate(s, cameras, n_cameras, N, n_rows, &h->err)) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  auto o = std::make_shared<RcObject>();
  const size_t n = (size_t)s->n_shape;
  std::vector<int> seg(n);
  for (size_t i = 0; i < n; i++) {
    seg[i] = (int)(uint16_t)s->shape_seg[i];
    o->needs_rows = o->needs_rows || s->shape_row[i] >= 0;
    o->mesh = o->mesh || s->shape_type[i] == MSSIM_SHAPE_TRIMESH;  // (a per-env mesh lives in a slot whose shared type is one)
  }
  RcTables& T = o->T;
  T.n_shape = s->n_shape;
  o->n_env_shape = s->n_env_shape;
  if (int rc = rc_upload(h, o.get(), s->shape_type, n, &T.type)) return rc;
  if (int rc = rc_upload(h, o.get(), s->shape_row, n, &T.row)) return rc;
  if (int rc = rc_upload(h, o.get(), s->shape_frame, 7 * n, &T.frame)) return rc;
  if (int rc = rc_upload(h, o.get(), s->shape_param, 4 * n, &T.param)) return rc;
  if (int rc = rc_upload(h, o.get(), s->shape_bound, 4 * n, &T.bound)) return rc;
  if (int rc = rc_upload(h, o.get(), seg.data(), n, &T.seg)) return rc;
  if (int rc = rc_upload(h, o.get(), s->shape_planes, 2 * n, &T.planes2)) return rc;
  if (int rc = rc_upload(h, o.get(), s->planes, 4 * (size_t)s->n_plane, &T.plane)) return rc;
  if (s->n_env_shape > 0) {
    const size_t ne = (size_t)s->n_env_shape * (size_t)N;
    if (int rc = rc_upload(h, o.get(), s->shape_env_slot, n, &T.env_slot)) return rc;
    if (int rc = rc_upload(h, o.get(), s->env_shape_frame, 7 * ne, &T.env_frame)) return rc;
    if (int rc = rc_upload(h, o.get(), s->env_shape_param, 4 * ne, &T.env_param)) return rc;
    if (int rc = rc_upload(h, o.get(), s->env_shape_bound, 4 * ne, &T.env_bound)) return rc;
    if (s->env_shape_planes)
      if (int rc = rc_upload(h, o.get(), s->env_shape_planes, 2 * ne, &T.env_planes2)) return rc;
    if (s->env_shape_seg) {
      std::vector<int> eseg(ne);
      for (size_t k = 0; k < ne; k++) eseg[k] = (int)(uint16_t)s->env_shape_seg[k];
      if (int rc = rc_upload(h, o.get(), eseg.data(), ne, &T.env_seg)) return rc;
    }
  }
  o->mesh = o->mesh || T.env_planes2 || T.env_seg;  // (k_raycast<false> stays the kernel it was: it reads neither table)
  if (s->n_tri > 0 && s->n_tri_node > 0 && o->mesh) {
    if (int rc = rc_upload(h, o.get(), s->tri_soup, 12 * (size_t)s->n_tri, &T.tri_soup)) return rc;
    if (int rc = rc_upload(h, o.get(), s->tri_bvh, 112 * (size_t)s->n_tri_node, &T.tri_bvh)) return rc;
  }
  for (int c = 0; c < n_cameras; c++) {
    const mssim_camera_desc& k = cameras[c];
    RcCamera cam{k.width, k.height, k.fx, k.fy, k.cx, k.cy, k.near, fminf(k.far, 0.001f * (float)MSSIM_RAYCAST_MAX_MM), k.mount_row, {}, k.env_pose};
    for (int j = 0; j < 7; j++) cam.pose[j] = k.pose[j];
    o->needs_rows = o->needs_rows || k.mount_row >= 0;
    o->cams.push_back(cam);
  }
  h->raycasts.push_back(o);
  *id = (int)h->raycasts.size() - 1;
  return 0;
}

int mssim_raycast_destroy(mssim_handle h, int32_t id) {
  if (!h) return 1;
  if (id < 0 || id >= (int)h->raycasts.size() || !h->raycasts[id]) { h->err = "raycast_destroy: bad id"; return 1; }
  (void)hipSetDevice(h->device);
  h->raycasts[id].reset();
  return 0;
}

int mssim_raycast_render(mssim_handle h, int32_t id, int32_t camera, int16_t* pos_seg, float* depth_f32, void* stream) {
  if (!h) return 1;
  settle(h, (hipStream_t)stream);
  RcTarget at;
  if (int rc = rc_target(h, "raycast_render", id, camera, &at)) return rc;
  if (!pos_seg) { h->err = "raycast_render: no pos_seg output"; return 1; }
  if (((uintptr_t)pos_seg & 7u) || ((uintptr_t)depth_f32 & 3u)) { h->err = "raycast_render: pos_seg must be 8-byte aligned, depth_f32 4-byte"; return 1; }
  const auto kernel = at.o->mesh ? k_raycast<true> : k_raycast<false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)(at.tiles * h->N)), dim3(256), 0, (hipStream_t)stream, at.o->T, *at.C, h->buf.rigid_body_data,
                     h->N, at.tiles_x, at.tiles, (short*)pos_seg, depth_f32);
  HIPCHK(h, hipGetLastError());
  return 0;
}

}  // extern "C"

#endif  // __HIPCC__
