// mssim_kernels.hip -- gfx950 kernels + C ABI (include/mssim.h) of the batched rigid-body step.
//
// Replaces `px.step()` and the px.gpu_apply_* / px.gpu_fetch_* / contact-query calls of
// ManiSkill's GPU path (mani_skill/envs/scene.py:374-375, 736-796, 941-977).
//
// Data layout in HBM: every per-env quantity is struct-of-arrays `[item][N]` with the env index
// fastest, so lane e of a wave touches address base + e*4: one 256-B coalesced request per
// wave-instruction. Constant model tables are env-shared and wave-uniform (scalar loads, L2
// resident).
//
// One kernel advances the simulation: k_solve16 (mssim_solve16.h), 16 lanes per env, a whole control step per
// launch (narrowphase, dynamics, solver, integration, FK for every substep; optionally the action map at its head and
// the copy-out + task epilogue at its tail). All launches go to the caller's stream, no host sync.
// `Topo` (FK-only kernel) selects compile-time (Panda: 9-DoF tree unrolled into VGPRs) or run-time topology.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <memory>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/mssim.h"
#include "../../include/mssim_hip_tasks.h"
#include "mssim_collide.h"

// the control-step kernel carries the task structs in one union (DevState::tail_task): a new one must not widen it,
// or the kernel arguments of every instance change
static_assert(sizeof(mssim_stack_task) <= sizeof(mssim_peg_task) && alignof(mssim_stack_task) <= alignof(mssim_peg_task), "tail_task union would grow");
static_assert(sizeof(mssim_pusht_task) <= sizeof(mssim_peg_task) && alignof(mssim_pusht_task) <= alignof(mssim_peg_task), "tail_task union would grow");

#include "mssim_limits.h"  // MAXC and the other capacities the host shares with the control-step kernel

struct DevModel {
  int n_dof, n_tendon, n_link, n_free, n_kin, n_shape, n_pair;
  const int *dof_parent, *dof_type, *body_gravity, *tendon_dof, *link_body, *free_gravity;
  const unsigned* dof_anc;  // bitmask of strict ancestors of each dof
  const float *dof_frame, *dof_axis, *dof_limit, *dof_drive, *dof_armature, *body_inertial, *tendon_param, *link_frame;
  const float *free_inertial, *free_damping;
  const int *shape_type, *shape_kind, *shape_index, *shape_row, *shape_hull, *pair_shape;
  const int* pair_packed;  // [n_pair rounded up to 128, + 128] shape a | shape b << 8 (-1 behind the last pair): what the control-step kernel's cull reads, one word per pair
  const float *shape_frame, *shape_param, *shape_material, *shape_bound, *hull_verts;
  const float* shape_center;  // [n_shape][3] bounding-sphere centre in the BODY frame (shape_frame applied)
  const float* dof_pack;      // [n_dof][32]  all per-joint constants of the cooperative kernel in one 128-byte record
  const float* shape_pack;    // [n_shape][24] all per-shape constants of its narrowphase in one 96-byte record
  const float* shape_half;    // [n_shape][3] half extents of a box in the SHAPE frame, centred at the bound centre, that contains the shape
  const float* tri_soup;      // [n_tri][12] triangle meshes: centroid, three corners relative to it (include/mssim.h)
  const float* tri_bvh;       // [n_tri_node][112] their 16-wide BVH
  const int* pair_mesh_slot;  // [n_pair] ordinal of the pair among those whose second shape is a triangle mesh, else -1 (rows of DevState::tri_clear)
  // per-env overrides ([items][N], env fastest); slot < 0 = shared value
  const int *shape_env_slot, *free_env_slot;
  const float *env_shape_frame, *env_shape_param, *env_shape_bound, *env_free_inertial;
  float gx, gy, gz, dt, contact_offset, rest_offset, erp, max_depen, sleep_threshold;
  int pos_iters, vel_iters;
};

struct DevState {
  int N;
  float *root, *q, *qd, *qt, *qdt, *qf, *qacc;  // [7][N], [n_dof][N] ...
  float *free_s, *free_force, *kin;             // [n_free*13][N], [n_free*3][N], [n_kin*7][N]
  float* free_wake;                             // [n_free][N] seconds of low energy left before the body sleeps; <= 0: asleep
  float* pcm;                                   // [N][MSSIM_PCM_SLOTS][48] persistent contact manifolds (mssim_limits.h S16_PCM_LEN)
  int* pcm_tick;                                // [N] substep counter of the cache
  float* warm;                                  // [4 n_pair][N][4] contact multipliers (n, t1, t2) + substep stamp per (pair, manifold slot)
  float* tri_clear;                             // [4 n_mesh_pair][N] per (convex shape, mesh) pair: the shape's bounding-sphere centre in the mesh frame at its last
                                                // full BVH traversal and how far it may move from there before a triangle can be in range (<= 0: traverse)
  float *bodypose, *bodyvel;                    // [n_dof*7][N], [n_dof*6][N] (velocity about O = root position)
  float* bodyaux;                               // [n_dof*6][N] world joint axis (3) + joint anchor (3)
  int* pair_cnt;                                // [n_pair][N] contact points of the pair in the last substep (after the patch reduction)
  float* pair_imp;                              // [n_pair*3][N]
  int* hit_list;                                // [1 + MAXC][N]: count, then the pairs in contact after the last fused step
  float* rows;                                  // [N][S16_ROWS_GLB][32] J | W rows of the contacts beyond the register / LDS resident ones
  int* overflow;                                // [N]
  // action of this control step, mapped to drive targets at the head of the fused launch (mssim_step_action);
  // null = targets were set before the launch
  const float* act;                             // [N][act_dim]
  int act_dim;
  const int* act_col;                           // [n_dof] action column, < 0: joint untouched
  const float *act_lo, *act_hi;                 // [n_dof]
  const int* act_flags;                         // [n_dof] 1: delta on the current position, 2: clip + affine map
  const float* act_qpos;                        // user-visible qpos buffer (what the controller reads) or null
  float* act_target;                            // user-visible target_qpos buffer or null
  float* act_target_vel;                        // user-visible target_qvel buffer or null
  // copy-out + task epilogue at the tail of the fused launch (whole control step = one launch); 0 = none
  unsigned tail_fetch;                          // mssim_fetch mask
  mssim_buffers tail_buf;
  union { mssim_pick_task pick; mssim_push_task push; mssim_peg_task peg; mssim_stack_task stack; mssim_pusht_task pusht; } tail_task;  // kind = template TASK
  const int* tail_pairs; int tail_npairs;       // finger <-> object candidate pairs
  float *tail_obs, *tail_reward, *tail_head;  // tail_head: PegInsertionSide's head_at_hole, PushT's intersection
  uint8_t* tail_flags;
};

// ------------------------------------------------------------------------------------------------
// topology policies
struct TopoDyn {
  static constexpr int MAXD = MSSIM_MAX_DOF;
  static constexpr bool STATIC = false;
  static constexpr int UNROLL = 1;
  int nd;
  const int* par;
  const int* typ;
  const unsigned* ancm;
  MS_DEV TopoDyn(const DevModel& M) : nd(M.n_dof), par(M.dof_parent), typ(M.dof_type), ancm(M.dof_anc) {}
  MS_DEV int n() const { return nd; }
  MS_DEV int parent(int j) const { return par[j]; }
  MS_DEV bool revolute(int j) const { return typ[j] == MSSIM_JOINT_REVOLUTE; }
  MS_DEV unsigned anc(int j) const { return ancm[j]; }
};
struct TopoPanda {  // panda_v2/v3: 7 revolute chain + 2 prismatic fingers on body 6
  static constexpr int MAXD = 9;
  static constexpr bool STATIC = true;
  static constexpr int UNROLL = 9;
  MS_DEV TopoPanda(const DevModel&) {}
  MS_DEV constexpr int n() const { return 9; }
  MS_DEV constexpr int parent(int j) const { return j == 0 ? -1 : (j <= 7 ? j - 1 : 6); }
  MS_DEV constexpr bool revolute(int j) const { return j < 7; }
  MS_DEV constexpr unsigned anc(int j) const { return j <= 7 ? ((1u << j) - 1u) : 0x7Fu; }
};

// spatial helpers (world frame, about the origin O = articulation root position)
struct sv6 { f3 w, v; };                    // motion
struct sf6 { f3 n, f; };                    // force
struct si10 { float m; f3 h; s3 I; };       // inertia
MS_DEV sv6 crossm(sv6 a, sv6 b) { return sv6{cross(a.w, b.w), cross(a.w, b.v) + cross(a.v, b.w)}; }
MS_DEV sf6 crossf(sv6 a, sf6 b) { return sf6{cross(a.w, b.n) + cross(a.v, b.f), cross(a.w, b.f)}; }
MS_DEV sf6 imul(const si10& I, sv6 a) { return sf6{smulv(I.I, a.w) + cross(I.h, a.v), a.v * I.m - cross(I.h, a.w)}; }
MS_DEV float sdot(sv6 s, sf6 f) { return dot(s.w, f.n) + dot(s.v, f.f); }

#define SOA(ptr, item) ((ptr)[(size_t)(item) * N + e])

// XCD-aware block -> env-chunk mapping. Workgroups are dealt round-robin to the 8 XCDs (each with its
// own L2), so with the identity mapping every XCD touches a 1/8 slice of every cache line of the
// [item][N] arrays (false sharing across the 8 L2s, 8x fetch amplification). Grids are padded to a
// multiple of 8 blocks and block b works on chunk (b % 8) * (grid / 8) + b / 8: XCD x owns one
// contiguous range of envs in every kernel, so the state a kernel writes is re-read from the same L2.
MS_DEV int xcd_chunk(int b, int grid) { return (b & 7) * (grid >> 3) + (b >> 3); }

template <class T>
MS_DEV void fk_bodies(const T& topo, const DevModel& M, pose_t root, const float* q, pose_t* bp, f3* aw, f3* anchor) {
#pragma unroll T::UNROLL
  for (int j = 0; j < T::MAXD; j++) {
    if (j >= topo.n()) break;
    int p = topo.parent(j);
    pose_t P = root;
    if (T::STATIC) {
#pragma unroll
      for (int k = 0; k < T::MAXD; k++)
        if (k == p) P = bp[k];
    } else if (p >= 0) {
      P = bp[p];
    }
    pose_t J = pmul(P, pose_from(M.dof_frame + 7 * j));
    f3 al = f3{M.dof_axis[3 * j], M.dof_axis[3 * j + 1], M.dof_axis[3 * j + 2]};
    f3 a = qrot(J.q, al);
    pose_t B = J;
    if (topo.revolute(j)) B.q = qnormalized(qmul(J.q, qaxis_angle(al, q[j])));
    else B.p = J.p + a * q[j];
    bp[j] = B;
    aw[j] = a;
    anchor[j] = J.p;
  }
}

template <class T>
MS_DEV sv6 subspace(const T& topo, int j, f3 a, f3 r) {  // r = anchor - O
  if (topo.revolute(j)) return sv6{a, cross(r, a)};
  return sv6{f3{0.f, 0.f, 0.f}, a};
}

// body spatial velocities about O from qd; writes bodypose / bodyvel SoA
template <class T>
MS_DEV void write_kinematics(const T& topo, const DevModel& M, const DevState& S, int e, pose_t root, const float* qd,
                             const pose_t* bp, const f3* aw, const f3* anchor) {
  const int N = S.N;
  sv6 V[T::MAXD];
#pragma unroll T::UNROLL
  for (int j = 0; j < T::MAXD; j++) {
    if (j >= topo.n()) break;
    int p = topo.parent(j);
    sv6 Vp = sv6{f3{0, 0, 0}, f3{0, 0, 0}};
    if (T::STATIC) {
#pragma unroll
      for (int k = 0; k < T::MAXD; k++)
        if (k == p) Vp = V[k];
    } else if (p >= 0) {
      Vp = V[p];
    }
    sv6 Sj = subspace(topo, j, aw[j], anchor[j] - root.p);
    V[j] = sv6{Vp.w + Sj.w * qd[j], Vp.v + Sj.v * qd[j]};
    pose_store_soa(S.bodypose, 7 * j, N, e, bp[j]);
    float* o = S.bodyvel + (size_t)(6 * j) * N + e;
    o[0] = V[j].w.x; o[(size_t)N] = V[j].w.y; o[2 * (size_t)N] = V[j].w.z;
    o[3 * (size_t)N] = V[j].v.x; o[4 * (size_t)N] = V[j].v.y; o[5 * (size_t)N] = V[j].v.z;
    float* a = S.bodyaux + (size_t)(6 * j) * N + e;
    a[0] = aw[j].x; a[(size_t)N] = aw[j].y; a[2 * (size_t)N] = aw[j].z;
    a[3 * (size_t)N] = anchor[j].x; a[4 * (size_t)N] = anchor[j].y; a[5 * (size_t)N] = anchor[j].z;
  }
}

// ------------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(64) void k_fk(DevModel M, DevState S) {
  const int N = S.N;
  int e = xcd_chunk(blockIdx.x, gridDim.x) * 64 + threadIdx.x;
  if (e >= N) return;
  T topo(M);
  pose_t root = pose_soa(S.root, 0, N, e);
  float q[T::MAXD], qd[T::MAXD];
#pragma unroll T::UNROLL
  for (int j = 0; j < T::MAXD; j++) {
    if (j >= topo.n()) break;
    q[j] = SOA(S.q, j);
    qd[j] = SOA(S.qd, j);
  }
  pose_t bp[T::MAXD];
  f3 aw[T::MAXD], anchor[T::MAXD];
  fk_bodies(topo, M, root, q, bp, aw, anchor);
  write_kinematics(topo, M, S, e, root, qd, bp, aw, anchor);
}

// ------------------------------------------------------------------------------------------------
// the 10 inertial parameters of free body b in env e (per-env override or shared table)
MS_DEV void free_inertial_of(const DevModel& M, int N, int b, int e, float* out) {
  const int slot = M.free_env_slot[b];
#pragma unroll
  for (int k = 0; k < 10; k++) out[k] = slot < 0 ? M.free_inertial[10 * b + k] : M.env_free_inertial[(size_t)(10 * slot + k) * N + e];
}

// ------------------------------------------------------------------------------------------------
// apply / fetch: transposes between the user-visible AoS buffers and the SoA state
__global__ void k_apply(DevModel M, DevState S, mssim_buffers B, unsigned what) {
  const int N = S.N;
  int e = xcd_chunk(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x;
  if (e >= N) return;
  const int n = M.n_dof;
  if ((what & MSSIM_RIGID_DATA) && B.rigid_body_data) {
    for (int b = 0; b < M.n_free; b++) {
      const float* r = B.rigid_body_data + 13 * ((size_t)(M.n_link + b) * N + e);
      // a row that differs from what the last fetch wrote wakes the body (include/mssim.h sleep_threshold)
      bool changed = false;
      for (int c = 0; c < 13; c++) changed = changed || r[c] != SOA(S.free_s, 13 * b + c);
      if (!changed) continue;
      for (int c = 0; c < 13; c++) SOA(S.free_s, 13 * b + c) = r[c];
      SOA(S.free_wake, b) = MSSIM_WAKE_TIME;
    }
    // a kinematic body given a different pose wakes the env's free bodies (include/mssim.h sleep_threshold): it may have been
    // moved into a sleeping body, or away from under one
    bool kin_moved = false;
    for (int k = 0; k < M.n_kin; k++) {
      const float* r = B.rigid_body_data + 13 * ((size_t)(M.n_link + M.n_free + k) * N + e);
      for (int c = 0; c < 7; c++) {
        kin_moved = kin_moved || r[c] != SOA(S.kin, 7 * k + c);
        SOA(S.kin, 7 * k + c) = r[c];
      }
    }
    if (kin_moved)
      for (int b = 0; b < M.n_free; b++) SOA(S.free_wake, b) = MSSIM_WAKE_TIME;
  }
  if ((what & MSSIM_ART_ROOT_POSE) && B.rigid_body_data && M.n_link > 0) {
    const float* r = B.rigid_body_data + 13 * (size_t)e;
    for (int c = 0; c < 7; c++) SOA(S.root, c) = r[c];
  }
  if ((what & MSSIM_ART_QPOS) && B.art_qpos) for (int j = 0; j < n; j++) SOA(S.q, j) = B.art_qpos[(size_t)e * n + j];
  if ((what & MSSIM_ART_QVEL) && B.art_qvel) for (int j = 0; j < n; j++) SOA(S.qd, j) = B.art_qvel[(size_t)e * n + j];
  if ((what & MSSIM_ART_QF) && B.art_qf) for (int j = 0; j < n; j++) SOA(S.qf, j) = B.art_qf[(size_t)e * n + j];
  if ((what & MSSIM_ART_TARGET_POS) && B.art_target_qpos) for (int j = 0; j < n; j++) SOA(S.qt, j) = B.art_target_qpos[(size_t)e * n + j];
  if ((what & MSSIM_ART_TARGET_VEL) && B.art_target_qvel) for (int j = 0; j < n; j++) SOA(S.qdt, j) = B.art_target_qvel[(size_t)e * n + j];
  if ((what & MSSIM_RIGID_FORCE) && B.rigid_body_force)
    for (int b = 0; b < M.n_free; b++) {
      const float* f = B.rigid_body_force + 4 * ((size_t)(M.n_link + b) * N + e);
      for (int c = 0; c < 3; c++) SOA(S.free_force, 3 * b + c) = f[c];
      if (f[0] != 0.f || f[1] != 0.f || f[2] != 0.f) SOA(S.free_wake, b) = MSSIM_WAKE_TIME;
    }
}

// fetch: grid (N/64, n_rows + 1). blockIdx.y < n_rows: one (body row, env) per lane -> consecutive
// lanes write consecutive 52-byte records (coalesced); blockIdx.y == n_rows: the articulation arrays
// (device functions: k_fetch runs them one (row, env) per lane, the fetch + task-epilogue launches run the
// rows of an env over 4 lanes of one block)
MS_DEV void fetch_row(const DevModel& M, const DevState& S, const mssim_buffers& B, unsigned what, int e, int row) {
  const int N = S.N;
  if (!B.rigid_body_data) return;
  float* r = B.rigid_body_data + 13 * ((size_t)row * N + e);
  if (row < M.n_link) {
    if (!(what & (MSSIM_LINK_POSE | MSSIM_LINK_VEL))) return;
    const pose_t root = pose_soa(S.root, 0, N, e);
    const int b = M.link_body[row];
    const pose_t P = pmul(b < 0 ? root : pose_soa(S.bodypose, 7 * b, N, e), pose_from(M.link_frame + 7 * row));
    if (what & MSSIM_LINK_POSE) { r[0] = P.p.x; r[1] = P.p.y; r[2] = P.p.z; r[3] = P.q.w; r[4] = P.q.x; r[5] = P.q.y; r[6] = P.q.z; }
    if (what & MSSIM_LINK_VEL) {
      f3 w = f3{0, 0, 0}, vv = f3{0, 0, 0};
      if (b >= 0) {
        w = f3{SOA(S.bodyvel, 6 * b), SOA(S.bodyvel, 6 * b + 1), SOA(S.bodyvel, 6 * b + 2)};
        vv = f3{SOA(S.bodyvel, 6 * b + 3), SOA(S.bodyvel, 6 * b + 4), SOA(S.bodyvel, 6 * b + 5)} + cross(w, P.p - root.p);
      }
      r[7] = vv.x; r[8] = vv.y; r[9] = vv.z; r[10] = w.x; r[11] = w.y; r[12] = w.z;
    }
  } else if (what & MSSIM_RIGID_DATA) {
    if (row < M.n_link + M.n_free) {
      const int b = row - M.n_link;
      for (int c = 0; c < 13; c++) r[c] = SOA(S.free_s, 13 * b + c);
    } else {
      const int k = row - M.n_link - M.n_free;
      const pose_t P = pose_soa(S.kin, 7 * k, N, e);
      r[0] = P.p.x; r[1] = P.p.y; r[2] = P.p.z; r[3] = P.q.w; r[4] = P.q.x; r[5] = P.q.y; r[6] = P.q.z;
      for (int c = 7; c < 13; c++) r[c] = 0.f;
    }
  }
}
// one joint per lane (the control-step kernel's tail)
MS_DEV void fetch_art_joint(const DevModel& M, const DevState& S, const mssim_buffers& B, unsigned what, int e, int j) {
  const int N = S.N;
  const int n = M.n_dof;
  if ((what & MSSIM_ART_QPOS) && B.art_qpos) B.art_qpos[(size_t)e * n + j] = SOA(S.q, j);
  if ((what & MSSIM_ART_QVEL) && B.art_qvel) B.art_qvel[(size_t)e * n + j] = SOA(S.qd, j);
  if ((what & MSSIM_ART_QACC) && B.art_qacc) B.art_qacc[(size_t)e * n + j] = SOA(S.qacc, j);
  if ((what & MSSIM_ART_TARGET_POS) && B.art_target_qpos) B.art_target_qpos[(size_t)e * n + j] = SOA(S.qt, j);
  if ((what & MSSIM_ART_TARGET_VEL) && B.art_target_qvel) B.art_target_qvel[(size_t)e * n + j] = SOA(S.qdt, j);
}
MS_DEV void fetch_art(const DevModel& M, const DevState& S, const mssim_buffers& B, unsigned what, int e) {
  const int N = S.N;
  const int n = M.n_dof;
  if ((what & MSSIM_ART_QPOS) && B.art_qpos) for (int j = 0; j < n; j++) B.art_qpos[(size_t)e * n + j] = SOA(S.q, j);
  if ((what & MSSIM_ART_QVEL) && B.art_qvel) for (int j = 0; j < n; j++) B.art_qvel[(size_t)e * n + j] = SOA(S.qd, j);
  if ((what & MSSIM_ART_QACC) && B.art_qacc) for (int j = 0; j < n; j++) B.art_qacc[(size_t)e * n + j] = SOA(S.qacc, j);
  if ((what & MSSIM_ART_TARGET_POS) && B.art_target_qpos) for (int j = 0; j < n; j++) B.art_target_qpos[(size_t)e * n + j] = SOA(S.qt, j);
  if ((what & MSSIM_ART_TARGET_VEL) && B.art_target_qvel) for (int j = 0; j < n; j++) B.art_target_qvel[(size_t)e * n + j] = SOA(S.qdt, j);
}
__global__ __launch_bounds__(64) void k_fetch(DevModel M, DevState S, mssim_buffers B, unsigned what) {
  const int e = xcd_chunk(blockIdx.x, gridDim.x) * 64 + threadIdx.x;
  if (e >= S.N) return;
  const int R = M.n_link + M.n_free + M.n_kin;
  if ((int)blockIdx.y < R) fetch_row(M, S, B, what, e, blockIdx.y);
  else fetch_art(M, S, B, what, e);
}
// fetch inside a task-epilogue launch (256 threads = 64 envs x 4 lanes): the 4 lanes of an env share its
// rows, then one of them runs the epilogue on what the block just wrote (same CU, same L1)
MS_DEV int fetch_in_block(const DevModel& M, const DevState& S, const mssim_buffers& B, unsigned what) {
  const int e = xcd_chunk(blockIdx.x, gridDim.x) * 64 + (threadIdx.x & 63);
  const int ty = threadIdx.x >> 6;
  if (e < S.N) {
    const int R = M.n_link + M.n_free + M.n_kin;
    for (int row = ty; row < R; row += 4) fetch_row(M, S, B, what, e, row);
    if (ty == 3) fetch_art(M, S, B, what, e);
  }
  __threadfence_block();
  __syncthreads();
  return (ty == 0 && e < S.N) ? e : -1;
}

// contact impulse queries: q = [nq][2] body rows (pair query) or [nq] rows (body query)
__global__ void k_query(DevModel M, DevState S, const int* q, int nq, int body_query, float* out) {
  const int N = S.N;
  int e = blockIdx.x * blockDim.x + threadIdx.x;
  int k = blockIdx.y;
  if (e >= N || k >= nq) return;
  f3 s = f3{0, 0, 0};
  int qa = body_query ? q[k] : q[2 * k], qb = body_query ? -2 : q[2 * k + 1];
  for (int p = 0; p < M.n_pair; p++) {
    int ra = M.shape_row[M.pair_shape[2 * p]], rb = M.shape_row[M.pair_shape[2 * p + 1]];
    float sign = 0.f;
    if (body_query) sign = (ra == qa ? 1.f : 0.f) - (rb == qa ? 1.f : 0.f);
    else if (ra == qa && rb == qb) sign = 1.f;
    else if (ra == qb && rb == qa) sign = -1.f;
    if (sign != 0.f && S.pair_cnt[(size_t)p * N + e] > 0)
      s += f3{SOA(S.pair_imp, 3 * p), SOA(S.pair_imp, 3 * p + 1), SOA(S.pair_imp, 3 * p + 2)} * sign;
  }
  float* o = out + 3 * ((size_t)k * N + e);
  o[0] = s.x; o[1] = s.y; o[2] = s.z;
}

// End-effector block of the action map (pd_ee_delta_pos): 3 action columns = translation of link `link` in the
// root frame; the joints flagged 4 in the joint map get  target = qpos + J^T (J J^T + 1e-9 I)^-1 a  with J the
// translational Jacobian of the link over the joints on its path that are not flagged 64 (held: another controller's
// joints, which stay where they are; agents/controllers/utils/kinematics.py `compute_ik`)
struct EeMap {
  int link;    // < 0: no end-effector block
  int col0;    // first action column
  int rows;    // 3: translation (pd_ee_delta_pos), 6: translation + rotation vector (pd_ee_delta_pose)
  float lo, hi;
  float rot_scale;  // rows == 6: the rotation columns are clipped by their norm to 1 and scaled by this (pd_ee_pose.py:197-210)
  int flags;   // 2: clip to [-1, 1] and map to [lo, hi] (translation) / clip by norm and scale (rotation)
};
// affine action -> drive targets (user-visible buffer + simulation state)
__global__ void k_apply_action(DevModel M, DevState S, mssim_buffers B, const float* __restrict__ action, int adim,
                               const int* __restrict__ col, const float* __restrict__ lo, const float* __restrict__ hi,
                               const int* __restrict__ flags, EeMap ee) {
  const int N = S.N;
  int e = xcd_chunk(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x;
  if (e >= N) return;
  const int n = M.n_dof;
  for (int j = 0; j < n; j++) {
    const int cj = col[j];
    if (cj < 0) continue;
    float a = action[(size_t)e * adim + cj];
    if (flags[j] & 2) {
      a = clip_unit(a);
      a = 0.5f * (hi[j] + lo[j]) + 0.5f * (hi[j] - lo[j]) * a;
    }
    if (flags[j] & 48) {  // forward velocity of a planar base in its own frame (include/mssim.h set_action_map)
      const int jy = (flags[j] >> 8) & 31;
      const float yaw = B.art_qpos ? B.art_qpos[(size_t)e * n + jy] : SOA(S.q, jy);
      a *= (flags[j] & 16) ? cosf(yaw) : sinf(yaw);
    }
    if (flags[j] & 8) {  // velocity drive target (pd_joint_vel, agents/controllers/pd_joint_vel.py:31-33)
      SOA(S.qdt, j) = a;
      if (B.art_target_qvel) B.art_target_qvel[(size_t)e * n + j] = a;
      continue;
    }
    const float qj = B.art_qpos ? B.art_qpos[(size_t)e * n + j] : SOA(S.q, j);  // what `controller.qpos` reads
    const float t = ((flags[j] & 1) ? qj : 0.f) + a;
    SOA(S.qt, j) = t;
    if (B.art_target_qpos) B.art_target_qpos[(size_t)e * n + j] = t;
  }
  if (ee.link >= 0) {
    const pose_t root = pose_soa(S.root, 0, N, e);
    const m3 Rr = qmat(root.q);
    const int b = M.link_body[ee.link];
    const pose_t Pb = b < 0 ? root : pose_soa(S.bodypose, 7 * b, N, e);
    const f3 pe = pmul(Pb, pose_from(M.link_frame + 7 * ee.link)).p;
    const unsigned path = b < 0 ? 0u : (M.dof_anc[b] | (1u << b));
    float av[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int r = 0; r < 3; r++) {
      float a = action[(size_t)e * adim + ee.col0 + r];
      if (ee.flags & 2) {
        a = clip_unit(a);
        a = 0.5f * (ee.hi + ee.lo) + 0.5f * (ee.hi - ee.lo) * a;
      }
      av[r] = a;
    }
    if (ee.rows == 6) {
      f3 rot = f3{action[(size_t)e * adim + ee.col0 + 3], action[(size_t)e * adim + ee.col0 + 4], action[(size_t)e * adim + ee.col0 + 5]};
      if (ee.flags & 2) {
        const float nr = sqrtf(dot(rot, rot));
        if (nr > 1.f) rot = rot * (1.f / fmaxf(nr, 1e-12f));
        rot = rot * ee.rot_scale;
      }
      av[3] = rot.x; av[4] = rot.y; av[5] = rot.z;
    }
    // column j of the link's Jacobian in the root frame: linear part, angular part
    auto jcol = [&](int j, f3& jw) {
      const f3 a = f3{SOA(S.bodyaux, 6 * j), SOA(S.bodyaux, 6 * j + 1), SOA(S.bodyaux, 6 * j + 2)};
      const f3 an = f3{SOA(S.bodyaux, 6 * j + 3), SOA(S.bodyaux, 6 * j + 4), SOA(S.bodyaux, 6 * j + 5)};
      const bool rev = M.dof_type[j] == MSSIM_JOINT_REVOLUTE;
      jw = rev ? mtmulv(Rr, a) : f3{0.f, 0.f, 0.f};
      return mtmulv(Rr, rev ? cross(a, pe - an) : a);
    };
    float y[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (ee.rows == 3) {
      s3 G = s3{1e-9f, 1e-9f, 1e-9f, 0.f, 0.f, 0.f};  // xx yy zz xy xz yz
      for (int j = 0; j < n; j++)
        if (((path >> j) & 1u) && !(flags[j] & 64)) {
          f3 w;
          const f3 v = jcol(j, w);
          G.xx += v.x * v.x; G.yy += v.y * v.y; G.zz += v.z * v.z; G.xy += v.x * v.y; G.xz += v.x * v.z; G.yz += v.y * v.z;
        }
      // (G >= 1e-9 I in exact arithmetic; a determinant lost to cancellation moves nothing rather than everything)
      const float detG = G.xx * (G.yy * G.zz - G.yz * G.yz) - G.xy * (G.xy * G.zz - G.yz * G.xz) + G.xz * (G.xy * G.yz - G.yy * G.xz);
      const f3 y3 = detG > 1e-30f ? smulv(sinverse(G), f3{av[0], av[1], av[2]}) : f3{0.f, 0.f, 0.f};
      y[0] = y3.x; y[1] = y3.y; y[2] = y3.z;
    } else {
      // 6 x 6: J J^T + 1e-9 I is symmetric positive definite -> Cholesky without pivoting, two triangular solves
      float G[6][6];
#pragma unroll
      for (int r = 0; r < 6; r++)
#pragma unroll
        for (int q = 0; q < 6; q++) G[r][q] = r == q ? 1e-9f : 0.f;
      for (int j = 0; j < n; j++)
        if (((path >> j) & 1u) && !(flags[j] & 64)) {
          f3 w;
          const f3 v = jcol(j, w);
          const float cj[6] = {v.x, v.y, v.z, w.x, w.y, w.z};
#pragma unroll
          for (int r = 0; r < 6; r++)
#pragma unroll
            for (int q = 0; q <= r; q++) G[r][q] += cj[r] * cj[q];
        }
      float Lc[6][6];
#pragma unroll
      for (int r = 0; r < 6; r++)
#pragma unroll
        for (int q = 0; q <= r; q++) {
          float sum = G[r][q];
#pragma unroll
          for (int m = 0; m < q; m++) sum -= Lc[r][m] * Lc[q][m];
          Lc[r][q] = r == q ? sqrtf(fmaxf(sum, 1e-20f)) : sum / Lc[q][q];
        }
      float z[6];
#pragma unroll
      for (int r = 0; r < 6; r++) {
        float sum = av[r];
#pragma unroll
        for (int m = 0; m < r; m++) sum -= Lc[r][m] * z[m];
        z[r] = sum / Lc[r][r];
      }
#pragma unroll
      for (int r = 5; r >= 0; r--) {
        float sum = z[r];
#pragma unroll
        for (int m = r + 1; m < 6; m++) sum -= Lc[m][r] * y[m];
        y[r] = sum / Lc[r][r];
      }
    }
    for (int j = 0; j < n; j++)
      if (((path >> j) & 1u) && (flags[j] & 4)) {
        f3 w;
        const f3 v = jcol(j, w);
        const float qj = B.art_qpos ? B.art_qpos[(size_t)e * n + j] : SOA(S.q, j);
        const float t = qj + v.x * y[0] + v.y * y[1] + v.z * y[2] + w.x * y[3] + w.y * y[4] + w.z * y[5];
        SOA(S.qt, j) = t;
        if (B.art_target_qpos) B.art_target_qpos[(size_t)e * n + j] = t;
      }
  }
}

#include "mssim_ik.h"  // iterative IK block of the action map (the end-effector modes that track a target pose)

// The robot's is_static under a robot profile (mssim_set_task_robot, R.n_ranges > 0), as the static threshold of a task
// struct that makes the per-env function below decide the same: +inf where the robot is static, -1 where it is not (the
// functions test max |qvel| <= threshold, and that maximum is never NaN). qvel: the env's row of the visible buffer. The
// comparison is signed where the profile says so (Fetch.is_static: a joint moving fast in the negative direction counts as
// static); a NaN velocity is not static under either. The per-env functions themselves do not know of the profile: the
// tail instances of k_solve16 compile them as before, and so does every k_task_*<FETCH, false>.
MS_DEV float profile_static_thresh(const mssim_task_robot& R, const float* __restrict__ qvel) {
  bool is_static = true;
  for (int r = 0; r < R.n_ranges; r++)
    for (int j = R.first[r]; j < R.first[r] + R.count[r]; j++) {
      const float v = qvel[j];
      is_static = is_static && (R.signed_compare ? v : fabsf(v)) <= R.thresh[r];
    }
  return is_static ? INFINITY : -1.f;
}

// PickCube-style evaluate / obs / reward
// FETCH: the launch first performs mssim_fetch(what) for its envs (fetch_in_block; 256 threads per block)
MS_DEV void task_pick_env(const DevModel& M, const DevState& S, const mssim_buffers& B, const mssim_pick_task& T, const int* __restrict__ pairs, int npairs,
                                                    float* __restrict__ obs, float* __restrict__ reward, uint8_t* __restrict__ flags, int e) {
  const int N = S.N;
  const int n = M.n_dof;
  const int D = 2 * n + 24;
  float* o = obs + (size_t)e * D;
  auto rowp = [&](int row) { return B.rigid_body_data + 13 * ((size_t)row * N + e); };
  float qv_max = 0.f, qv_sq = 0.f;
  for (int j = 0; j < n; j++) {
    const float q = B.art_qpos[(size_t)e * n + j], v = B.art_qvel[(size_t)e * n + j];
    o[j] = q;
    o[n + j] = v;
    if (j < T.n_static_dofs) { qv_max = fmaxf(qv_max, fabsf(v)); qv_sq += v * v; }
  }
  const float* tcp = rowp(T.tcp_row);
  const float* ob = rowp(T.obj_row);
  const float* gl = rowp(T.goal_row);
  const f3 ptcp = f3{tcp[0], tcp[1], tcp[2]}, pobj = f3{ob[0], ob[1], ob[2]}, pgoal = f3{gl[0], gl[1], gl[2]};
  // pairwise contact impulses finger <-> object during the last substep (scene.py:736-796); the few
  // candidate pairs are listed by the host: entry = pair | finger (bit 30: 0 left, 1 right) | object is shape A (bit 31)
  f3 lf = f3{0, 0, 0}, rf = f3{0, 0, 0};
  for (int k = 0; k < npairs; k++) {
    const unsigned ent = (unsigned)pairs[k];
    const int p = (int)(ent & 0x3FFFFFFFu);
    if (S.pair_cnt[(size_t)p * N + e] <= 0) continue;
    // impulse on the finger from the object: +imp if the finger is shape A, -imp otherwise
    f3 imp = f3{SOA(S.pair_imp, 3 * p), SOA(S.pair_imp, 3 * p + 1), SOA(S.pair_imp, 3 * p + 2)} * ((ent >> 31) ? -1.f : 1.f);
    if ((ent >> 30) & 1u) rf += imp; else lf += imp;
  }
  const float inv_dt = 1.f / M.dt;
  lf = lf * inv_dt; rf = rf * inv_dt;
  auto yaxis = [&](const float* r) { return mcol(qmat(qnormalized(q4{r[3], r[4], r[5], r[6]})), 1); };
  auto angle_deg = [&](f3 a, f3 b) {
    const float na = norm(a), nb = norm(b);
    a = a * (1.f / (na < 1e-6f ? 1.f : na));
    b = b * (1.f / (nb < 1e-6f ? 1.f : nb));
    return acosf(fminf(fmaxf(dot(a, b), -1.f), 1.f)) * 57.29577951308232f;
  };
  const f3 ldir = yaxis(rowp(T.finger1_row)), rdir = -yaxis(rowp(T.finger2_row));
  const bool lflag = norm(lf) >= T.min_force && angle_deg(ldir, lf) <= T.max_angle_deg;
  const bool rflag = norm(rf) >= T.min_force && angle_deg(rdir, rf) <= T.max_angle_deg;
  const bool grasped = lflag && rflag;
  const float d_goal = norm(pgoal - pobj);
  const bool placed = d_goal <= T.goal_thresh;
  const bool is_static = qv_max <= T.static_thresh;
  const bool success = placed && is_static;
  // observation
  int k = 2 * n;
  o[k++] = grasped ? 1.f : 0.f;
  for (int i = 0; i < 7; i++) o[k++] = tcp[i];
  o[k++] = pgoal.x; o[k++] = pgoal.y; o[k++] = pgoal.z;
  for (int i = 0; i < 7; i++) o[k++] = ob[i];
  o[k++] = pobj.x - ptcp.x; o[k++] = pobj.y - ptcp.y; o[k++] = pobj.z - ptcp.z;
  o[k++] = pgoal.x - pobj.x; o[k++] = pgoal.y - pobj.y; o[k++] = pgoal.z - pobj.z;
  // dense reward (pick_cube.py:128-158)
  float r = 1.f - tanhf(5.f * norm(pobj - ptcp));
  if (grasped) r += 1.f + (1.f - tanhf(5.f * d_goal));
  if (placed) r += 1.f - tanhf(5.f * sqrtf(qv_sq));
  if (success) r = 5.f;
  reward[e] = r * T.reward_scale;
  uint8_t* f = flags + 4 * (size_t)e;
  f[0] = success; f[1] = placed; f[2] = is_static; f[3] = grasped;
  if (T.terminated_out) T.terminated_out[e] = success;
  if (T.elapsed_steps) { const int v = T.elapsed_steps[e] + 1; T.elapsed_steps[e] = v; if (T.elapsed_out) T.elapsed_out[e] = v; if (T.truncated_out) T.truncated_out[e] = v >= T.time_limit ? 1 : 0; }
}
// FETCH: the launch first performs mssim_fetch(what) for its envs (fetch_in_block; 256 threads per block)
// PROFILE: the handle has a robot profile R: its static rule decides, and the reward's velocity norm covers R.pick_norm_dofs joints
template <bool FETCH, bool PROFILE>
__global__ __launch_bounds__(256) void k_task_pick(DevModel M, DevState S, mssim_buffers B, unsigned what, mssim_pick_task T, const int* __restrict__ pairs, int npairs,
                                                    float* __restrict__ obs, float* __restrict__ reward, uint8_t* __restrict__ flags, mssim_task_robot R) {
  int e;
  if (FETCH) { e = fetch_in_block(M, S, B, what); if (e < 0) return; }
  else { e = xcd_chunk(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x; if (e >= S.N) return; }
  if constexpr (PROFILE) {
    T.static_thresh = profile_static_thresh(R, B.art_qvel + (size_t)e * M.n_dof);
    T.n_static_dofs = R.pick_norm_dofs;
  }
  task_pick_env(M, S, B, T, pairs, npairs, obs, reward, flags, e);
}

MS_DEV void task_push_env(const DevModel& M, const DevState& S, const mssim_buffers& B, const mssim_push_task& T, float* __restrict__ obs, float* __restrict__ reward,
                                                    uint8_t* __restrict__ flags, int e) {
  const int N = S.N;
  const int n = M.n_dof;
  float* o = obs + (size_t)e * (2 * n + 17);
  auto rowp = [&](int row) { return B.rigid_body_data + 13 * ((size_t)row * N + e); };
  for (int j = 0; j < n; j++) {
    o[j] = B.art_qpos[(size_t)e * n + j];
    o[n + j] = B.art_qvel[(size_t)e * n + j];
  }
  const float* tcp = rowp(T.tcp_row);
  const float* ob = rowp(T.obj_row);
  const float* gl = rowp(T.goal_row);
  int k = 2 * n;
  for (int i = 0; i < 7; i++) o[k++] = tcp[i];
  for (int i = 0; i < 3; i++) o[k++] = gl[i];
  for (int i = 0; i < 7; i++) o[k++] = ob[i];
  // evaluate (push_cube.py:165-176) and dense reward (:209-232)
  const float dx = ob[0] - gl[0], dy = ob[1] - gl[1];
  const float obj_to_goal = sqrtf(dx * dx + dy * dy);
  // the lift threshold as the torch path forms it: half + 5e-3 in double, rounded once (0.02f + 5e-3f is one ulp below
  // float(0.025), and a cube at exactly that height was judged differently; tests/task_cases.py exact edges)
  const bool success = obj_to_goal < T.goal_radius && ob[2] < (float)((double)T.cube_half_size + 5e-3);
  const f3 push_p = f3{ob[0] - T.cube_half_size - 0.005f, ob[1], ob[2]};
  const float dist = norm(push_p - f3{tcp[0], tcp[1], tcp[2]});
  float r = 1.f - tanhf(5.f * dist);
  if (dist < 0.01f) r += 1.f - tanhf(5.f * obj_to_goal);
  if (success) r = 3.f;
  reward[e] = r * T.reward_scale;
  flags[e] = success;
  if (T.terminated_out) T.terminated_out[e] = success;
  if (T.elapsed_steps) { const int v = T.elapsed_steps[e] + 1; T.elapsed_steps[e] = v; if (T.elapsed_out) T.elapsed_out[e] = v; if (T.truncated_out) T.truncated_out[e] = v >= T.time_limit ? 1 : 0; }
}
// FETCH: the launch first performs mssim_fetch(what) for its envs (fetch_in_block; 256 threads per block)
template <bool FETCH>
__global__ __launch_bounds__(256) void k_task_push(DevModel M, DevState S, mssim_buffers B, unsigned what, mssim_push_task T, float* __restrict__ obs, float* __restrict__ reward,
                                                    uint8_t* __restrict__ flags) {
  int e;
  if (FETCH) { e = fetch_in_block(M, S, B, what); if (e < 0) return; }
  else { e = xcd_chunk(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x; if (e >= S.N) return; }
  task_push_env(M, S, B, T, obs, reward, flags, e);
}

// RollBall evaluate / obs / reward (roll_ball.py evaluate, _get_obs_extra, compute_dense_reward, in its order of
// operations). T.reached is the env's latch: read, set where the tcp is at the hit point (only with T.update_reached), and
// read by the reward in its new value. One lane per env; never at the control-step kernel's tail.
MS_DEV void task_roll_env(const DevModel& M, const DevState& S, const mssim_buffers& B, const mssim_roll_task& T, float* __restrict__ obs, float* __restrict__ reward,
                          uint8_t* __restrict__ flags, int e) {
  const int N = S.N;
  const int n = M.n_dof;
  float* o = obs + (size_t)e * (2 * n + 26);
  auto rowp = [&](int row) { return B.rigid_body_data + 13 * ((size_t)row * N + e); };
  for (int j = 0; j < n; j++) {
    o[j] = B.art_qpos[(size_t)e * n + j];
    o[n + j] = B.art_qvel[(size_t)e * n + j];
  }
  const float* tcp = rowp(T.tcp_row);
  const float* bl = rowp(T.ball_row);
  const float* gl = rowp(T.goal_row);
  const f3 ptcp = f3{tcp[0], tcp[1], tcp[2]}, pball = f3{bl[0], bl[1], bl[2]}, pgoal = f3{gl[0], gl[1], gl[2]};
  int k = 2 * n;
  for (int i = 0; i < 7; i++) o[k++] = tcp[i];
  o[k++] = pgoal.x; o[k++] = pgoal.y; o[k++] = pgoal.z;
  for (int i = 0; i < 7; i++) o[k++] = bl[i];
  for (int i = 7; i < 10; i++) o[k++] = bl[i];
  o[k++] = pball.x - ptcp.x; o[k++] = pball.y - ptcp.y; o[k++] = pball.z - ptcp.z;
  o[k++] = pgoal.x - pball.x; o[k++] = pgoal.y - pball.y; o[k++] = pgoal.z - pball.z;
  const float dx = pball.x - pgoal.x, dy = pball.y - pgoal.y;
  const float ball_to_goal = sqrtf(dx * dx + dy * dy);
  const bool success = ball_to_goal < T.goal_radius;
  // the hit point: behind the ball, seen from the goal (the offset as the torch path forms it: the sum in double, rounded once)
  const f3 away = pball - pgoal;
  const float na = norm(away);
  const f3 unit = f3{away.x / na, away.y / na, away.z / na};
  const f3 hit = pball + unit * (float)((double)T.ball_radius + (double)T.hit_offset);
  const float dist = norm(hit - ptcp);
  float latch = T.reached[e];
  if (T.update_reached && dist < T.reach_thresh) { latch = 1.f; T.reached[e] = 1.f; }
  float r = 20.f * (1.f - tanhf(ball_to_goal)) * latch + (1.f - tanhf(2.f * dist)) * (1.f - latch) + latch;
  if (success) r = 30.f;
  reward[e] = r * T.reward_scale;
  flags[e] = success;
  if (T.terminated_out) T.terminated_out[e] = success;
  if (T.elapsed_steps) { const int v = T.elapsed_steps[e] + 1; T.elapsed_steps[e] = v; if (T.elapsed_out) T.elapsed_out[e] = v; if (T.truncated_out) T.truncated_out[e] = v >= T.time_limit ? 1 : 0; }
}
// FETCH: the launch first performs mssim_fetch(what) for its envs (fetch_in_block; 256 threads per block)
template <bool FETCH>
__global__ __launch_bounds__(256) void k_task_roll(DevModel M, DevState S, mssim_buffers B, unsigned what, mssim_roll_task T, float* __restrict__ obs, float* __restrict__ reward,
                                                    uint8_t* __restrict__ flags) {
  int e;
  if (FETCH) { e = fetch_in_block(M, S, B, what); if (e < 0) return; }
  else { e = xcd_chunk(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x; if (e >= S.N) return; }
  task_roll_env(M, S, B, T, obs, reward, flags, e);
}

// PullCube evaluate / obs / reward (pull_cube.py): PushCube's observation; the pull point lies behind the cube (+x), and
// success has no height condition. One lane per env; never at the control-step kernel's tail.
MS_DEV void task_pull_env(const DevModel& M, const DevState& S, const mssim_buffers& B, const mssim_pull_task& T, float* __restrict__ obs, float* __restrict__ reward,
                          uint8_t* __restrict__ flags, int e) {
  const int N = S.N;
  const int n = M.n_dof;
  float* o = obs + (size_t)e * (2 * n + 17);
  auto rowp = [&](int row) { return B.rigid_body_data + 13 * ((size_t)row * N + e); };
  for (int j = 0; j < n; j++) {
    o[j] = B.art_qpos[(size_t)e * n + j];
    o[n + j] = B.art_qvel[(size_t)e * n + j];
  }
  const float* tcp = rowp(T.tcp_row);
  const float* ob = rowp(T.obj_row);
  const float* gl = rowp(T.goal_row);
  int k = 2 * n;
  for (int i = 0; i < 7; i++) o[k++] = tcp[i];
  for (int i = 0; i < 3; i++) o[k++] = gl[i];
  for (int i = 0; i < 7; i++) o[k++] = ob[i];
  const float dx = ob[0] - gl[0], dy = ob[1] - gl[1];
  const float obj_to_goal = sqrtf(dx * dx + dy * dy);
  const bool success = obj_to_goal < T.goal_radius;
  // (the offset as the torch path forms it: half + 2 x 5 mm in double, rounded once)
  const f3 pull_p = f3{ob[0] + (float)((double)T.cube_half_size + 0.01), ob[1], ob[2]};
  const float dist = norm(pull_p - f3{tcp[0], tcp[1], tcp[2]});
  float r = 1.f - tanhf(5.f * dist);
  if (dist < 0.01f) r += 1.f - tanhf(5.f * obj_to_goal);
  if (success) r = 3.f;
  reward[e] = r * T.reward_scale;
  flags[e] = success;
  if (T.terminated_out) T.terminated_out[e] = success;
  if (T.elapsed_steps) { const int v = T.elapsed_steps[e] + 1; T.elapsed_steps[e] = v; if (T.elapsed_out) T.elapsed_out[e] = v; if (T.truncated_out) T.truncated_out[e] = v >= T.time_limit ? 1 : 0; }
}
// FETCH: the launch first performs mssim_fetch(what) for its envs (fetch_in_block; 256 threads per block)
template <bool FETCH>
__global__ __launch_bounds__(256) void k_task_pull(DevModel M, DevState S, mssim_buffers B, unsigned what, mssim_pull_task T, float* __restrict__ obs, float* __restrict__ reward,
                                                    uint8_t* __restrict__ flags) {
  int e;
  if (FETCH) { e = fetch_in_block(M, S, B, what); if (e < 0) return; }
  else { e = xcd_chunk(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x; if (e >= S.N) return; }
  task_pull_env(M, S, B, T, obs, reward, flags, e);
}

// Pose algebra exactly as the Python `Pose` class does it (utils/structs/pose.py, rotation_conversions.py:
// no re-normalisation, rotation as p + w t + v x t with t = 2 v x p, product standardised to w >= 0), so
// that the fused task outputs equal the torch path also for the slightly non-unit quaternions users set
MS_DEV f3 tq_apply(q4 q, f3 p) {
  const f3 v = f3{q.x, q.y, q.z};
  const f3 t = cross(v, p) * 2.f;
  return p + t * q.w + cross(v, t);
}
MS_DEV pose_t tq_mul(pose_t a, pose_t b) {
  q4 q = qmul(a.q, b.q);
  if (q.w < 0.f) q = q4{-q.w, -q.x, -q.y, -q.z};
  return pose_t{a.p + tq_apply(a.q, b.p), q};
}
MS_DEV pose_t tq_inv(pose_t a) {
  const q4 qc = q4{a.q.w, -a.q.x, -a.q.y, -a.q.z};
  return pose_t{tq_apply(qc, -a.p), qc};
}
// PegInsertionSide evaluate / obs / reward (peg_insertion_side.py:247-355)
MS_DEV void task_peg_env(const DevModel& M, const DevState& S, const mssim_buffers& B, const mssim_peg_task& T, const int* __restrict__ pairs, int npairs,
                                                   float* __restrict__ obs, float* __restrict__ reward, uint8_t* __restrict__ flags, float* __restrict__ head_out, int e) {
  const int N = S.N;
  const int n = M.n_dof;
  float* o = obs + (size_t)e * (2 * n + 25);
  auto rowp = [&](int row) { return B.rigid_body_data + 13 * ((size_t)row * N + e); };
  auto rowpose = [&](int row) { const float* r = rowp(row); return pose_t{f3{r[0], r[1], r[2]}, q4{r[3], r[4], r[5], r[6]}}; };
  for (int j = 0; j < n; j++) {
    o[j] = B.art_qpos[(size_t)e * n + j];
    o[n + j] = B.art_qvel[(size_t)e * n + j];
  }
  const float* tcp = rowp(T.tcp_row);
  const float* pg = rowp(T.peg_row);
  const pose_t Ptcp = rowpose(T.tcp_row), Ppeg = rowpose(T.peg_row), Pbox = rowpose(T.box_row);
  const f3 hs = f3{T.peg_half_sizes[3 * e], T.peg_half_sizes[3 * e + 1], T.peg_half_sizes[3 * e + 2]};
  const f3 hoff = f3{T.box_hole_offsets[3 * e], T.box_hole_offsets[3 * e + 1], T.box_hole_offsets[3 * e + 2]};
  const float rad = T.box_hole_radii[e];
  const q4 qi = q4{1, 0, 0, 0};
  const pose_t head = tq_mul(Ppeg, pose_t{f3{hs.x, 0, 0}, qi});      // peg head (orange end)
  const pose_t hole = tq_mul(Pbox, pose_t{hoff, qi});                 // hole centre frame
  const f3 hah = tq_mul(tq_inv(hole), head).p;                          // head in the hole frame
  const bool success = hah.x >= -0.015f && fabsf(hah.y) <= rad && fabsf(hah.z) <= rad;
  // finger <-> peg contact forces of the last substep (Panda.is_grasping, panda.py:236-264)
  f3 lf = f3{0, 0, 0}, rf = f3{0, 0, 0};
  for (int k = 0; k < npairs; k++) {
    const unsigned ent = (unsigned)pairs[k];
    const int p = (int)(ent & 0x3FFFFFFFu);
    if (S.pair_cnt[(size_t)p * N + e] <= 0) continue;
    f3 imp = f3{SOA(S.pair_imp, 3 * p), SOA(S.pair_imp, 3 * p + 1), SOA(S.pair_imp, 3 * p + 2)} * ((ent >> 31) ? -1.f : 1.f);
    if ((ent >> 30) & 1u) rf += imp; else lf += imp;
  }
  const float inv_dt = 1.f / M.dt;
  lf = lf * inv_dt; rf = rf * inv_dt;
  auto yaxis = [&](int row) { return mcol(qmat(qnormalized(rowpose(row).q)), 1); };
  auto angle_deg = [&](f3 a, f3 b) {
    const float na = norm(a), nb = norm(b);
    a = a * (1.f / (na < 1e-6f ? 1.f : na));
    b = b * (1.f / (nb < 1e-6f ? 1.f : nb));
    return acosf(fminf(fmaxf(dot(a, b), -1.f), 1.f)) * 57.29577951308232f;
  };
  const f3 ldir = yaxis(T.finger1_row), rdir = -yaxis(T.finger2_row);
  const bool grasped = norm(lf) >= T.min_force && angle_deg(ldir, lf) <= T.max_angle_deg && norm(rf) >= T.min_force && angle_deg(rdir, rf) <= T.max_angle_deg;
  // observation
  int k = 2 * n;
  for (int i = 0; i < 7; i++) o[k++] = tcp[i];
  for (int i = 0; i < 7; i++) o[k++] = pg[i];
  o[k++] = hs.x; o[k++] = hs.y; o[k++] = hs.z;
  o[k++] = hole.p.x; o[k++] = hole.p.y; o[k++] = hole.p.z; o[k++] = hole.q.w; o[k++] = hole.q.x; o[k++] = hole.q.y; o[k++] = hole.q.z;
  o[k++] = rad;
  // dense reward
  const f3 grasp_target = tq_mul(Ppeg, pose_t{f3{-0.06f, 0, 0}, qi}).p;
  float r = 1.f - tanhf(4.f * norm(Ptcp.p - grasp_target));
  if (grasped) r += 1.f;
  const pose_t goal_inv = tq_inv(tq_mul(hole, pose_t{f3{-hs.x, 0, 0}, qi}));   // goal = box * hole_offset * head_offset^-1
  const f3 hg = tq_mul(goal_inv, head).p, bg = tq_mul(goal_inv, Ppeg).p;
  const float head_yz = sqrtf(hg.y * hg.y + hg.z * hg.z), body_yz = sqrtf(bg.y * bg.y + bg.z * bg.z);
  if (grasped) r += 3.f * (1.f - tanhf(0.5f * (head_yz + body_yz) + 4.5f * fmaxf(head_yz, body_yz)));
  if (grasped && head_yz < 0.01f && body_yz < 0.01f) r += 5.f * (1.f - tanhf(5.f * norm(hah)));
  if (success) r = 10.f;
  reward[e] = r * T.reward_scale;
  flags[e] = success;
  head_out[3 * (size_t)e] = hah.x; head_out[3 * (size_t)e + 1] = hah.y; head_out[3 * (size_t)e + 2] = hah.z;
  if (T.terminated_out) T.terminated_out[e] = success;
  if (T.elapsed_steps) { const int v = T.elapsed_steps[e] + 1; T.elapsed_steps[e] = v; if (T.elapsed_out) T.elapsed_out[e] = v; if (T.truncated_out) T.truncated_out[e] = v >= T.time_limit ? 1 : 0; }
}
// FETCH: the launch first performs mssim_fetch(what) for its envs (fetch_in_block; 256 threads per block)
template <bool FETCH>
__global__ __launch_bounds__(256) void k_task_peg(DevModel M, DevState S, mssim_buffers B, unsigned what, mssim_peg_task T, const int* __restrict__ pairs, int npairs,
                                                   float* __restrict__ obs, float* __restrict__ reward, uint8_t* __restrict__ flags, float* __restrict__ head_out) {
  int e;
  if (FETCH) { e = fetch_in_block(M, S, B, what); if (e < 0) return; }
  else { e = xcd_chunk(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x; if (e >= S.N) return; }
  task_peg_env(M, S, B, T, pairs, npairs, obs, reward, flags, head_out, e);
}

// StackCube evaluate / obs / reward (stack_cube.py evaluate, _get_obs_extra, compute_dense_reward)
MS_DEV void task_stack_env(const DevModel& M, const DevState& S, const mssim_buffers& B, const mssim_stack_task& T, const int* __restrict__ pairs, int npairs,
                           float* __restrict__ obs, float* __restrict__ reward, uint8_t* __restrict__ flags, int e) {
  const int N = S.N;
  const int n = M.n_dof;
  float* o = obs + (size_t)e * (2 * n + 30);
  auto rowp = [&](int row) { return B.rigid_body_data + 13 * ((size_t)row * N + e); };
  for (int j = 0; j < n; j++) {
    o[j] = B.art_qpos[(size_t)e * n + j];
    o[n + j] = B.art_qvel[(size_t)e * n + j];
  }
  const float* tcp = rowp(T.tcp_row);
  const float* ca = rowp(T.cubeA_row);
  const float* cb = rowp(T.cubeB_row);
  const f3 ptcp = f3{tcp[0], tcp[1], tcp[2]}, pa = f3{ca[0], ca[1], ca[2]}, pb = f3{cb[0], cb[1], cb[2]};
  // finger <-> cube A contact forces of the last substep (Panda.is_grasping, as task_pick_env)
  f3 lf = f3{0, 0, 0}, rf = f3{0, 0, 0};
  for (int k = 0; k < npairs; k++) {
    const unsigned ent = (unsigned)pairs[k];
    const int p = (int)(ent & 0x3FFFFFFFu);
    if (S.pair_cnt[(size_t)p * N + e] <= 0) continue;
    f3 imp = f3{SOA(S.pair_imp, 3 * p), SOA(S.pair_imp, 3 * p + 1), SOA(S.pair_imp, 3 * p + 2)} * ((ent >> 31) ? -1.f : 1.f);
    if ((ent >> 30) & 1u) rf += imp; else lf += imp;
  }
  const float inv_dt = 1.f / M.dt;
  lf = lf * inv_dt; rf = rf * inv_dt;
  auto yaxis = [&](const float* r) { return mcol(qmat(qnormalized(q4{r[3], r[4], r[5], r[6]})), 1); };
  auto angle_deg = [&](f3 a, f3 b) {
    const float na = norm(a), nb = norm(b);
    a = a * (1.f / (na < 1e-6f ? 1.f : na));
    b = b * (1.f / (nb < 1e-6f ? 1.f : nb));
    return acosf(fminf(fmaxf(dot(a, b), -1.f), 1.f)) * 57.29577951308232f;
  };
  const f3 ldir = yaxis(rowp(T.finger1_row)), rdir = -yaxis(rowp(T.finger2_row));
  const bool grasped = norm(lf) >= T.min_force && angle_deg(ldir, lf) <= T.max_angle_deg && norm(rf) >= T.min_force && angle_deg(rdir, rf) <= T.max_angle_deg;
  // evaluate
  const f3 off = pa - pb;
  const bool on = sqrtf(off.x * off.x + off.y * off.y) <= T.on_xy_thresh && fabsf(off.z - T.cube_half_size * 2.f) <= T.on_z_thresh;
  const f3 va = f3{ca[7], ca[8], ca[9]}, wa = f3{ca[10], ca[11], ca[12]};
  const float v = norm(va), av = norm(wa);
  const bool is_static = v <= T.static_lin_thresh && av <= T.static_ang_thresh;
  const bool success = on && is_static && !grasped;
  // observation
  int k = 2 * n;
  for (int i = 0; i < 7; i++) o[k++] = tcp[i];
  for (int i = 0; i < 7; i++) o[k++] = ca[i];
  for (int i = 0; i < 7; i++) o[k++] = cb[i];
  o[k++] = pa.x - ptcp.x; o[k++] = pa.y - ptcp.y; o[k++] = pa.z - ptcp.z;
  o[k++] = pb.x - ptcp.x; o[k++] = pb.y - ptcp.y; o[k++] = pb.z - ptcp.z;
  o[k++] = pb.x - pa.x; o[k++] = pb.y - pa.y; o[k++] = pb.z - pa.z;
  // dense reward, tiered: reach A, A grasped (+ place), A on B (+ ungrasp, static), success
  float r = 2.f * (1.f - tanhf(5.f * norm(ptcp - pa)));
  if (grasped) r = 4.f + (1.f - tanhf(5.f * norm(f3{pb.x, pb.y, pb.z + T.cube_half_size * 2.f} - pa)));
  if (on) {
    const float ungrasp = grasped ? (B.art_qpos[(size_t)e * n + n - 2] + B.art_qpos[(size_t)e * n + n - 1]) / T.gripper_width : 1.f;
    r = 6.f + (ungrasp + (1.f - tanhf(v * 10.f + av))) / 2.f;
  }
  if (success) r = 8.f;
  reward[e] = r * T.reward_scale;
  uint8_t* f = flags + 4 * (size_t)e;
  f[0] = success; f[1] = on; f[2] = is_static; f[3] = grasped;
  if (T.terminated_out) T.terminated_out[e] = success;
  if (T.elapsed_steps) { const int v = T.elapsed_steps[e] + 1; T.elapsed_steps[e] = v; if (T.elapsed_out) T.elapsed_out[e] = v; if (T.truncated_out) T.truncated_out[e] = v >= T.time_limit ? 1 : 0; }
}
// FETCH: the launch first performs mssim_fetch(what) for its envs (fetch_in_block; 256 threads per block)
template <bool FETCH>
__global__ __launch_bounds__(256) void k_task_stack(DevModel M, DevState S, mssim_buffers B, unsigned what, mssim_stack_task T, const int* __restrict__ pairs, int npairs,
                                                     float* __restrict__ obs, float* __restrict__ reward, uint8_t* __restrict__ flags) {
  int e;
  if (FETCH) { e = fetch_in_block(M, S, B, what); if (e < 0) return; }
  else { e = xcd_chunk(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x; if (e >= S.N) return; }
  task_stack_env(M, S, B, T, pairs, npairs, obs, reward, flags, e);
}

// Panda.is_grasping from the finger <-> object contact forces of the last substep, as task_pick_env computes it (the pair
// list is finger_pair_list's); f1 / f2: the fingers' rigid_body_data rows of env e.
// task_pick_env, task_peg_env and task_stack_env still carry this block inline: they are compiled into k_solve16 instances,
// which stay byte for byte as they are here. They should move to this helper in a change of their own; until then a fix to
// the block has to be made in all four places.
MS_DEV bool fingers_grasp(const DevModel& M, const DevState& S, const int* __restrict__ pairs, int npairs, const float* f1, const float* f2, float min_force,
                          float max_angle_deg, int e) {
  const int N = S.N;
  f3 lf = f3{0, 0, 0}, rf = f3{0, 0, 0};
  for (int k = 0; k < npairs; k++) {
    const unsigned ent = (unsigned)pairs[k];
    const int p = (int)(ent & 0x3FFFFFFFu);
    if (S.pair_cnt[(size_t)p * N + e] <= 0) continue;
    f3 imp = f3{SOA(S.pair_imp, 3 * p), SOA(S.pair_imp, 3 * p + 1), SOA(S.pair_imp, 3 * p + 2)} * ((ent >> 31) ? -1.f : 1.f);
    if ((ent >> 30) & 1u) rf += imp; else lf += imp;
  }
  const float inv_dt = 1.f / M.dt;
  lf = lf * inv_dt; rf = rf * inv_dt;
  auto yaxis = [&](const float* r) { return mcol(qmat(qnormalized(q4{r[3], r[4], r[5], r[6]})), 1); };
  auto angle_deg = [&](f3 a, f3 b) {
    const float na = norm(a), nb = norm(b);
    a = a * (1.f / (na < 1e-6f ? 1.f : na));
    b = b * (1.f / (nb < 1e-6f ? 1.f : nb));
    return acosf(fminf(fmaxf(dot(a, b), -1.f), 1.f)) * 57.29577951308232f;
  };
  const f3 ldir = yaxis(f1), rdir = -yaxis(f2);
  return norm(lf) >= min_force && angle_deg(ldir, lf) <= max_angle_deg && norm(rf) >= min_force && angle_deg(rdir, rf) <= max_angle_deg;
}
// The third angle of the XYZ Tait-Bryan decomposition of q's rotation matrix, atan2(-R01, R00), with the two entries as
// rotation_conversions.quaternion_to_matrix forms them: scaled by 2 / |q|^2, no unit norm assumed
MS_DEV float tq_euler_z(q4 q) {
  const float two_s = 2.f / (q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);
  const float r00 = 1.f - two_s * (q.y * q.y + q.z * q.z);
  const float r01 = two_s * (q.x * q.y - q.z * q.w);
  return atan2f(-r01, r00);
}

// PokeCube evaluate / obs / reward (poke_cube.py evaluate, _get_obs_extra, compute_dense_reward, in its order of masks).
// The head position is peg + (half length, 0, 0) unrotated; only the quaternion of the head POSE (peg * offset) is read.
// One lane per env; never at the control-step kernel's tail.
MS_DEV void task_poke_env(const DevModel& M, const DevState& S, const mssim_buffers& B, const mssim_poke_task& T, const int* __restrict__ pairs, int npairs,
                          float* __restrict__ obs, float* __restrict__ reward, uint8_t* __restrict__ flags, float* __restrict__ metrics, int e) {
  const int N = S.N;
  const int n = M.n_dof;
  float* o = obs + (size_t)e * (2 * n + 36);
  auto rowp = [&](int row) { return B.rigid_body_data + 13 * ((size_t)row * N + e); };
  float qv_max = 0.f, qv_sq = 0.f;
  for (int j = 0; j < n; j++) {
    const float q = B.art_qpos[(size_t)e * n + j], v = B.art_qvel[(size_t)e * n + j];
    o[j] = q;
    o[n + j] = v;
    if (j < T.n_static_dofs) { qv_max = fmaxf(qv_max, fabsf(v)); qv_sq += v * v; }
  }
  const float* tcp = rowp(T.tcp_row);
  const float* pg = rowp(T.peg_row);
  const float* cb = rowp(T.cube_row);
  const float* gl = rowp(T.goal_row);
  const f3 ptcp = f3{tcp[0], tcp[1], tcp[2]}, ppeg = f3{pg[0], pg[1], pg[2]}, pcube = f3{cb[0], cb[1], cb[2]}, pgoal = f3{gl[0], gl[1], gl[2]};
  const f3 phead = f3{ppeg.x + T.peg_half_length, ppeg.y, ppeg.z};
  const bool grasped = fingers_grasp(M, S, pairs, npairs, rowp(T.finger1_row), rowp(T.finger2_row), T.min_force, T.max_angle_deg, e);
  // evaluate
  const float gx = pcube.x - pgoal.x, gy = pcube.y - pgoal.y;
  const bool placed = sqrtf(gx * gx + gy * gy) < T.goal_radius;
  const pose_t head = tq_mul(pose_t{ppeg, q4{pg[3], pg[4], pg[5], pg[6]}}, pose_t{f3{T.peg_half_length, 0, 0}, q4{1, 0, 0, 0}});
  const float angle_diff = fabsf(tq_euler_z(head.q) - tq_euler_z(q4{cb[3], cb[4], cb[5], cb[6]}));
  const float hx = phead.x - pcube.x, hy = phead.y - pcube.y;
  const float head_to_cube = sqrtf(hx * hx + hy * hy);
  // (the threshold as the torch path forms it: half + 5 mm in double, rounded once)
  const bool fit = angle_diff < T.align_thresh && head_to_cube <= (float)((double)T.cube_half_size + 5e-3);
  const bool is_static = qv_max <= T.static_thresh;
  const bool success = placed && is_static;
  // observation
  int k = 2 * n;
  for (int i = 0; i < 7; i++) o[k++] = tcp[i];
  for (int i = 0; i < 7; i++) o[k++] = cb[i];
  for (int i = 0; i < 7; i++) o[k++] = pg[i];
  o[k++] = ppeg.x; o[k++] = ppeg.y; o[k++] = ppeg.z;  // "goal_pos": the peg's position
  o[k++] = ppeg.x - ptcp.x; o[k++] = ppeg.y - ptcp.y; o[k++] = ppeg.z - ptcp.z;
  o[k++] = pcube.x - ppeg.x; o[k++] = pcube.y - ppeg.y; o[k++] = pcube.z - ppeg.z;
  o[k++] = pgoal.x - pcube.x; o[k++] = pgoal.y - pcube.y; o[k++] = pgoal.z - pcube.z;
  o[k++] = phead.x - pcube.x; o[k++] = phead.y - pcube.y; o[k++] = phead.z - pcube.z;
  // dense reward: each tier replaces the one before
  const float tcp_to_peg = norm(ptcp - ppeg);
  float r = 2.f * (1.f - tanhf(5.f * tcp_to_peg));
  const bool held = grasped && tcp_to_peg < T.reach_thresh;
  if (held) r = 4.f + (1.f - tanhf(5.f * head_to_cube)) + (1.f - tanhf(5.f * angle_diff));
  if (fit && held) r = 7.f + (1.f - tanhf(5.f * norm(pgoal - pcube)));
  if (placed) r += 1.f - tanhf(5.f * sqrtf(qv_sq));
  if (success) r = 10.f;
  reward[e] = r * T.reward_scale;
  uint8_t* f = flags + 4 * (size_t)e;
  f[0] = success; f[1] = placed; f[2] = fit; f[3] = grasped;
  metrics[2 * (size_t)e] = angle_diff; metrics[2 * (size_t)e + 1] = head_to_cube;
  if (T.terminated_out) T.terminated_out[e] = success;
  if (T.elapsed_steps) { const int v = T.elapsed_steps[e] + 1; T.elapsed_steps[e] = v; if (T.elapsed_out) T.elapsed_out[e] = v; if (T.truncated_out) T.truncated_out[e] = v >= T.time_limit ? 1 : 0; }
}
// FETCH: the launch first performs mssim_fetch(what) for its envs (fetch_in_block; 256 threads per block)
// PROFILE: the handle has a robot profile R: its static rule decides (the reward's norm stays over qvel[:n_static_dofs] for every robot)
template <bool FETCH, bool PROFILE>
__global__ __launch_bounds__(256) void k_task_poke(DevModel M, DevState S, mssim_buffers B, unsigned what, mssim_poke_task T, const int* __restrict__ pairs, int npairs,
                                                    float* __restrict__ obs, float* __restrict__ reward, uint8_t* __restrict__ flags, float* __restrict__ metrics,
                                                    mssim_task_robot R) {
  int e;
  if (FETCH) { e = fetch_in_block(M, S, B, what); if (e < 0) return; }
  else { e = xcd_chunk(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x; if (e >= S.N) return; }
  if constexpr (PROFILE) T.static_thresh = profile_static_thresh(R, B.art_qvel + (size_t)e * M.n_dof);
  task_poke_env(M, S, B, T, pairs, npairs, obs, reward, flags, metrics, e);
}

// LiftPegUpright evaluate / obs / reward (lift_peg_upright.py): upright = the third XYZ Euler angle within upright_thresh of
// +-pi/2 (pi/2 as float32, what the torch path subtracts); the rotation term |R20| is the z component of the peg's x axis.
// One lane per env; never at the control-step kernel's tail.
MS_DEV void task_liftpeg_env(const DevModel& M, const DevState& S, const mssim_buffers& B, const mssim_liftpeg_task& T, const int* __restrict__ pairs, int npairs,
                             float* __restrict__ obs, float* __restrict__ reward, uint8_t* __restrict__ flags, int e) {
  const int N = S.N;
  const int n = M.n_dof;
  float* o = obs + (size_t)e * (2 * n + 14);
  auto rowp = [&](int row) { return B.rigid_body_data + 13 * ((size_t)row * N + e); };
  for (int j = 0; j < n; j++) {
    o[j] = B.art_qpos[(size_t)e * n + j];
    o[n + j] = B.art_qvel[(size_t)e * n + j];
  }
  const float* tcp = rowp(T.tcp_row);
  const float* pg = rowp(T.peg_row);
  int k = 2 * n;
  for (int i = 0; i < 7; i++) o[k++] = tcp[i];
  for (int i = 0; i < 7; i++) o[k++] = pg[i];
  const bool grasped = fingers_grasp(M, S, pairs, npairs, rowp(T.finger1_row), rowp(T.finger2_row), T.min_force, T.max_angle_deg, e);
  const q4 q = q4{pg[3], pg[4], pg[5], pg[6]};
  const float z_dist = fabsf(pg[2] - T.peg_half_length);
  const bool success = fabsf(fabsf(tq_euler_z(q)) - 1.5707963267948966f) < T.upright_thresh && z_dist < T.height_thresh;
  const float two_s = 2.f / (q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);
  float r = fabsf(two_s * (q.x * q.z - q.y * q.w));
  r += 1.f - tanhf(5.f * z_dist);
  const float reaching = grasped ? 1.f : 1.f - tanhf(5.f * norm(f3{pg[0], pg[1], pg[2]} - f3{tcp[0], tcp[1], tcp[2]}));
  r += reaching / 5.f;
  if (success) r = 3.f;
  reward[e] = r * T.reward_scale;
  flags[e] = success;
  if (T.terminated_out) T.terminated_out[e] = success;
  if (T.elapsed_steps) { const int v = T.elapsed_steps[e] + 1; T.elapsed_steps[e] = v; if (T.elapsed_out) T.elapsed_out[e] = v; if (T.truncated_out) T.truncated_out[e] = v >= T.time_limit ? 1 : 0; }
}
// FETCH: the launch first performs mssim_fetch(what) for its envs (fetch_in_block; 256 threads per block)
template <bool FETCH>
__global__ __launch_bounds__(256) void k_task_liftpeg(DevModel M, DevState S, mssim_buffers B, unsigned what, mssim_liftpeg_task T, const int* __restrict__ pairs, int npairs,
                                                       float* __restrict__ obs, float* __restrict__ reward, uint8_t* __restrict__ flags) {
  int e;
  if (FETCH) { e = fetch_in_block(M, S, B, what); if (e < 0) return; }
  else { e = xcd_chunk(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x; if (e >= S.N) return; }
  task_liftpeg_env(M, S, B, T, pairs, npairs, obs, reward, flags, e);
}

// PlaceSphere evaluate / obs / reward (place_sphere.py evaluate, _get_obs_extra, compute_dense_reward, in its order of
// overwrites): StackCube's place-and-release shape against a kinematic bin, with the robot's is_static as a third term of
// the on-bin tier. Every sum is formed left to right as the torch path forms it (off_z - radius - bin_base_half; bin_z +
// bin_base_half + radius). One lane per env; never at the control-step kernel's tail.
MS_DEV void task_place_env(const DevModel& M, const DevState& S, const mssim_buffers& B, const mssim_place_task& T, const int* __restrict__ pairs, int npairs,
                           float* __restrict__ obs, float* __restrict__ reward, uint8_t* __restrict__ flags, int e) {
  const int N = S.N;
  const int n = M.n_dof;
  float* o = obs + (size_t)e * (2 * n + 21);
  auto rowp = [&](int row) { return B.rigid_body_data + 13 * ((size_t)row * N + e); };
  float qv_max = 0.f;
  for (int j = 0; j < n; j++) {
    const float q = B.art_qpos[(size_t)e * n + j], v = B.art_qvel[(size_t)e * n + j];
    o[j] = q;
    o[n + j] = v;
    if (j < T.n_static_dofs) qv_max = fmaxf(qv_max, fabsf(v));
  }
  const float* tcp = rowp(T.tcp_row);
  const float* ob = rowp(T.obj_row);
  const float* bn = rowp(T.bin_row);
  const f3 ptcp = f3{tcp[0], tcp[1], tcp[2]}, pobj = f3{ob[0], ob[1], ob[2]}, pbin = f3{bn[0], bn[1], bn[2]};
  const bool grasped = fingers_grasp(M, S, pairs, npairs, rowp(T.finger1_row), rowp(T.finger2_row), T.min_force, T.max_angle_deg, e);
  // evaluate
  const f3 off = pobj - pbin;
  const bool on = sqrtf(off.x * off.x + off.y * off.y) <= T.on_bin_tol && fabsf(off.z - T.radius - T.bin_base_half) <= T.on_bin_tol;
  const float v = norm(f3{ob[7], ob[8], ob[9]}), av = norm(f3{ob[10], ob[11], ob[12]});
  const bool is_static = v <= T.static_lin_thresh && av <= T.static_ang_thresh;
  const bool success = on && is_static && !grasped;
  // observation
  int k = 2 * n;
  o[k++] = grasped ? 1.f : 0.f;
  for (int i = 0; i < 7; i++) o[k++] = tcp[i];
  o[k++] = pbin.x; o[k++] = pbin.y; o[k++] = pbin.z;
  for (int i = 0; i < 7; i++) o[k++] = ob[i];
  o[k++] = pobj.x - ptcp.x; o[k++] = pobj.y - ptcp.y; o[k++] = pobj.z - ptcp.z;
  // dense reward: each tier replaces the one before
  float r = 2.f * (1.f - tanhf(5.f * norm(ptcp - pobj)));
  if (grasped) r = 4.f + (1.f - tanhf(5.f * norm(f3{pbin.x, pbin.y, pbin.z + T.bin_base_half + T.radius} - pobj)));
  if (on) {
    const float ungrasp = grasped ? (B.art_qpos[(size_t)e * n + n - 2] + B.art_qpos[(size_t)e * n + n - 1]) / T.gripper_width : 16.f;
    const float robot_static = qv_max <= T.robot_static_thresh ? 1.f : 0.f;
    r = 6.f + (ungrasp + (1.f - tanhf(v * 10.f + av)) + robot_static) / 3.f;
  }
  if (success) r = 13.f;
  reward[e] = r * T.reward_scale;
  uint8_t* f = flags + 4 * (size_t)e;
  f[0] = success; f[1] = grasped; f[2] = on; f[3] = is_static;
  if (T.terminated_out) T.terminated_out[e] = success;
  if (T.elapsed_steps) { const int v = T.elapsed_steps[e] + 1; T.elapsed_steps[e] = v; if (T.elapsed_out) T.elapsed_out[e] = v; if (T.truncated_out) T.truncated_out[e] = v >= T.time_limit ? 1 : 0; }
}
// FETCH: the launch first performs mssim_fetch(what) for its envs (fetch_in_block; 256 threads per block)
// PROFILE: the handle has a robot profile R: its static rule gives the robot_static term of the on-bin tier
template <bool FETCH, bool PROFILE>
__global__ __launch_bounds__(256) void k_task_place(DevModel M, DevState S, mssim_buffers B, unsigned what, mssim_place_task T, const int* __restrict__ pairs, int npairs,
                                                     float* __restrict__ obs, float* __restrict__ reward, uint8_t* __restrict__ flags, mssim_task_robot R) {
  int e;
  if (FETCH) { e = fetch_in_block(M, S, B, what); if (e < 0) return; }
  else { e = xcd_chunk(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x; if (e >= S.N) return; }
  if constexpr (PROFILE) T.robot_static_thresh = profile_static_thresh(R, B.art_qvel + (size_t)e * M.n_dof);
  task_place_env(M, S, B, T, pairs, npairs, obs, reward, flags, e);
}

// PullCubeTool evaluate / obs / reward (pull_cube_tool.py evaluate, _get_obs_extra, compute_dense_reward): the reward is
// computed once, where the torch path computes it in evaluate() and again in get_reward(). The offsets are formed as the
// torch path forms them: the Python sums in double, rounded once to float32. The per-env values of the two batch means of
// evaluate() go to `metrics`; the means themselves are the caller's (no atomics here: the result stays deterministic).
// One lane per env; never at the control-step kernel's tail.
MS_DEV void task_pulltool_env(const DevModel& M, const DevState& S, const mssim_buffers& B, const mssim_pulltool_task& T, const int* __restrict__ pairs, int npairs,
                              float* __restrict__ obs, float* __restrict__ reward, uint8_t* __restrict__ flags, float* __restrict__ metrics, int e) {
  const int N = S.N;
  const int n = M.n_dof;
  float* o = obs + (size_t)e * (2 * n + 21);
  auto rowp = [&](int row) { return B.rigid_body_data + 13 * ((size_t)row * N + e); };
  for (int j = 0; j < n; j++) {
    o[j] = B.art_qpos[(size_t)e * n + j];
    o[n + j] = B.art_qvel[(size_t)e * n + j];
  }
  const float* tcp = rowp(T.tcp_row);
  const float* cb = rowp(T.cube_row);
  const float* tl = rowp(T.tool_row);
  const float* bs = rowp(T.base_row);
  int k = 2 * n;
  for (int i = 0; i < 7; i++) o[k++] = tcp[i];
  for (int i = 0; i < 7; i++) o[k++] = cb[i];
  for (int i = 0; i < 7; i++) o[k++] = tl[i];
  const f3 ptcp = f3{tcp[0], tcp[1], tcp[2]}, pcube = f3{cb[0], cb[1], cb[2]}, ptool = f3{tl[0], tl[1], tl[2]}, pbase = f3{bs[0], bs[1], bs[2]};
  const bool grasped = fingers_grasp(M, S, pairs, npairs, rowp(T.finger1_row), rowp(T.finger2_row), T.min_force, T.max_angle_deg, e);
  // evaluate
  const float bx = pcube.x - pbase.x, by = pcube.y - pbase.y;
  const bool success = sqrtf(bx * bx + by * by) < T.pulled_close_dist;
  const float to_workspace = norm(pcube - f3{pbase.x + (float)((double)T.arm_reach * 0.1), pbase.y, pbase.z});
  const float progress = 1.f - tanhf(3.f * to_workspace);
  // dense reward: reach the tool's handle, grasp it, bring the hook behind the cube, pull the cube in
  const float g = grasped ? 1.f : 0.f;
  const float tcp_to_tool = norm(ptcp - f3{ptool.x + 0.02f, ptool.y, ptool.z});
  float r = 2.f * (1.f - tanhf(5.f * tcp_to_tool)) + 2.f * g;
  const f3 ideal_hook = f3{pcube.x + (float)(-((double)T.hook_length + (double)T.cube_half_size)), pcube.y + -0.067f, pcube.z};
  const float positioning_dist = norm(ptool - ideal_hook);
  const float positioned = positioning_dist < 0.05f ? 1.f : 0.f;
  const f3 target = f3{pbase.x + 0.05f, pbase.y, pbase.z};
  const float cube_to_target = norm(pcube - target);
  const float initial_dist = norm(f3{(float)((double)T.arm_reach + 0.1), 0.f, (float)((double)T.cube_size / 2)} - target);
  r += 1.5f * (1.f - tanhf(3.f * positioning_dist)) * g;
  r += 3.f * ((initial_dist - cube_to_target) / initial_dist) * positioned * g;
  if (pcube.x > (float)((double)T.arm_reach + 0.15)) r -= 2.f;
  if (success) r += 5.f;
  reward[e] = r * T.reward_scale;
  flags[e] = success;
  float* m = metrics + 3 * (size_t)e;
  m[0] = to_workspace; m[1] = progress; m[2] = r / 5.f;
  if (T.terminated_out) T.terminated_out[e] = success;
  if (T.elapsed_steps) { const int v = T.elapsed_steps[e] + 1; T.elapsed_steps[e] = v; if (T.elapsed_out) T.elapsed_out[e] = v; if (T.truncated_out) T.truncated_out[e] = v >= T.time_limit ? 1 : 0; }
}
// FETCH: the launch first performs mssim_fetch(what) for its envs (fetch_in_block; 256 threads per block)
template <bool FETCH>
__global__ __launch_bounds__(256) void k_task_pulltool(DevModel M, DevState S, mssim_buffers B, unsigned what, mssim_pulltool_task T, const int* __restrict__ pairs, int npairs,
                                                        float* __restrict__ obs, float* __restrict__ reward, uint8_t* __restrict__ flags, float* __restrict__ metrics) {
  int e;
  if (FETCH) { e = fetch_in_block(M, S, B, what); if (e < 0) return; }
  else { e = xcd_chunk(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x; if (e >= S.N) return; }
  task_pulltool_env(M, S, B, T, pairs, npairs, obs, reward, flags, metrics, e);
}

// PlugCharger evaluate / obs / reward (plug_charger.py evaluate, _get_obs_extra; the dense reward is zero). The goal comes
// from the env's stored tensor T.goal_pose [N][7], not from a body row. The angle is taken from the relative quaternion
// r = conj(goal.q) * charger.q directly, 2 atan2(|r.xyz|, r.w) after the sign flip to r.w >= 0 that quaternion_multiply
// makes: the torch path's |r.xyz / (sin(a / 2) / a)| is the same number, and its min(a, 2 pi - a) cannot bite for a <= pi.
// A NaN pose gives NaN metrics and, every comparison with a NaN being false, success = 0.
// One lane per env; never at the control-step kernel's tail.
MS_DEV void task_plug_env(const DevModel& M, const DevState& S, const mssim_buffers& B, const mssim_plug_task& T,
                          float* __restrict__ obs, float* __restrict__ reward, uint8_t* __restrict__ flags, float* __restrict__ metrics, int e) {
  const int N = S.N;
  const int n = M.n_dof;
  float* o = obs + (size_t)e * (2 * n + 28);
  auto rowp = [&](int row) { return B.rigid_body_data + 13 * ((size_t)row * N + e); };
  for (int j = 0; j < n; j++) {
    o[j] = B.art_qpos[(size_t)e * n + j];
    o[n + j] = B.art_qvel[(size_t)e * n + j];
  }
  const float* tcp = rowp(T.tcp_row);
  const float* ch = rowp(T.charger_row);
  const float* rc = rowp(T.receptacle_row);
  const float* gl = T.goal_pose + 7 * (size_t)e;
  int k = 2 * n;
  for (int i = 0; i < 7; i++) o[k++] = tcp[i];
  for (int i = 0; i < 7; i++) o[k++] = ch[i];
  for (int i = 0; i < 7; i++) o[k++] = rc[i];
  for (int i = 0; i < 7; i++) o[k++] = gl[i];
  // evaluate
  const float dist = norm(f3{gl[0], gl[1], gl[2]} - f3{ch[0], ch[1], ch[2]});
  const float aw = gl[3];
  const f3 av = f3{-gl[4], -gl[5], -gl[6]}, bv = f3{ch[4], ch[5], ch[6]};
  const float bw = ch[3];
  float rw = aw * bw - dot(av, bv);
  f3 rv = bv * aw + av * bw + cross(av, bv);
  if (rw < 0.f) { rw = -rw; rv = -rv; }
  const float angle = 2.f * atan2f(norm(rv), rw);
  const bool success = dist <= T.dist_thresh && angle <= T.angle_thresh;
  reward[e] = 0.f * T.reward_scale;
  flags[e] = success;
  metrics[2 * (size_t)e] = dist; metrics[2 * (size_t)e + 1] = angle;
  if (T.terminated_out) T.terminated_out[e] = success;
  if (T.elapsed_steps) { const int v = T.elapsed_steps[e] + 1; T.elapsed_steps[e] = v; if (T.elapsed_out) T.elapsed_out[e] = v; if (T.truncated_out) T.truncated_out[e] = v >= T.time_limit ? 1 : 0; }
}
// FETCH: the launch first performs mssim_fetch(what) for its envs (fetch_in_block; 256 threads per block)
template <bool FETCH>
__global__ __launch_bounds__(256) void k_task_plug(DevModel M, DevState S, mssim_buffers B, unsigned what, mssim_plug_task T,
                                                    float* __restrict__ obs, float* __restrict__ reward, uint8_t* __restrict__ flags, float* __restrict__ metrics) {
  int e;
  if (FETCH) { e = fetch_in_block(M, S, B, what); if (e < 0) return; }
  else { e = xcd_chunk(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x; if (e >= S.N) return; }
  task_plug_env(M, S, B, T, obs, reward, flags, metrics, e);
}

// DrawTriangle dot layer / evaluate / obs (draw_triangle.py _after_control_step, evaluate, _get_obs_extra; the rules are
// stated at mssim_draw_task). The drawing is the env's own tables, updated in place: with T.update the dot of this control
// step is appended at index draw_step[e] before the tables are evaluated; a counter at max_dots appends nothing.
// 16 lanes per env, all 64 lanes of a wave call this (the ballots): lane c takes the reference points c, c + 16, ... against
// the new dot, the words c, c + 16, ... of the env's dot_near row (four dots a word; a zero byte is a drawn dot away from
// the outline) and the observation floats c, c + 16, ...; three ballots give the env's any / all. The tables are read before
// the ballots and written after them, lane 0 writing the dot. `live`: the group has an env. No atomics, no LDS.
MS_DEV void task_draw_env(const DevModel& M, const DevState& S, const mssim_buffers& B, const mssim_draw_task& T,
                          float* __restrict__ obs, float* __restrict__ reward, uint8_t* __restrict__ flags, int e, int c, bool live) {
  const int N = S.N;
  const int n = M.n_dof;
  const int shift = (int)(threadIdx.x & 48u);  // the group's 16 bits of a ballot
  const float* tcp = B.rigid_body_data + 13 * ((size_t)T.tcp_row * N + (live ? e : 0));
  float tx = 0.f, ty = 0.f;
  int k = 0;
  bool append = false, drawn = false, any_hit = false, all_ref = true, none_far = true;
  if (live) {
    tx = tcp[0]; ty = tcp[1];
    k = T.draw_step[e];
    append = T.update != 0 && k >= 0 && k < T.max_dots;
    drawn = append && tcp[2] < T.z_thresh;
    const float* tri = T.triangles + 2 * (size_t)e * T.n_ref;
    uint8_t* rh = T.ref_hit + (size_t)e * T.n_ref;
    for (int p = c; p < T.n_ref; p += 16) {
      bool hit;
      {
#pragma clang fp contract(off)  // (the torch path rounds both products and the sum)
        const float dx = tx - tri[2 * p], dy = ty - tri[2 * p + 1];
        hit = drawn && dx * dx + dy * dy < T.near_thresh2;
      }
      const bool was = rh[p] != 0;
      if (hit && !was) rh[p] = 1;  // (a byte no other lane reads or writes)
      any_hit = any_hit || hit;
      all_ref = all_ref && (hit || was);
    }
    const uint32_t* dn = reinterpret_cast<const uint32_t*>(T.dot_near + (size_t)e * T.max_dots);
    for (int w = c; w < (T.max_dots >> 2); w += 16) {
      uint32_t v = dn[w];
      if (append && w == (k >> 2)) v |= 0xffu << (8 * (k & 3));  // (the slot this call writes: judged by its new value below)
      none_far = none_far && ((v - 0x01010101u) & ~v & 0x80808080u) == 0u;
    }
  }
  const bool near = ((__ballot(any_hit) >> shift) & 0xffffull) != 0ull;
  const bool refs = ((__ballot(all_ref) >> shift) & 0xffffull) == 0xffffull;
  const bool dots_ok = ((__ballot(none_far) >> shift) & 0xffffull) == 0xffffull;
  if (!live) return;
  const bool success = refs && dots_ok && !(drawn && !near);
  if (c == 0) {
    if (append) {
      const size_t at = (size_t)e * T.max_dots + k;
      T.dots[2 * at] = drawn ? tx : 0.f; T.dots[2 * at + 1] = drawn ? ty : 0.f;
      T.dot_near[at] = drawn ? (near ? 1 : 0) : -1;
      T.draw_step[e] = k + 1;
    }
    reward[e] = success ? T.reward_scale : 0.f;
    flags[e] = success;
    if (T.terminated_out) T.terminated_out[e] = success;
    if (T.elapsed_steps) { const int v = T.elapsed_steps[e] + 1; T.elapsed_steps[e] = v; if (T.elapsed_out) T.elapsed_out[e] = v; if (T.truncated_out) T.truncated_out[e] = v >= T.time_limit ? 1 : 0; }
  }
  const float* gl = B.rigid_body_data + 13 * ((size_t)T.goal_row * N + e);
  const float* vt = T.vertices + 9 * (size_t)e;
  float* o = obs + (size_t)e * (2 * n + 35);
  for (int i = c; i < 2 * n + 35; i += 16) {
    const int j = i - 2 * n;
    float v;
    if (i < n) v = B.art_qpos[(size_t)e * n + i];
    else if (j < 0) v = B.art_qvel[(size_t)e * n + i - n];
    else if (j < 7) v = tcp[j];
    else if (j < 14) v = gl[j - 7];
    else if (j < 23) v = vt[j - 14] - tcp[(j - 14) % 3];
    else if (j < 26) v = gl[j - 23];
    else v = vt[j - 26];
    o[i] = v;
  }
}
// COPYOUT: the launch first performs mssim_fetch(what) for its 64 envs (fetch_in_block). Either way 256 threads per block:
// wave w serves the envs 16 w .. 16 w + 15 of the block's 64, four at a time
template <bool COPYOUT>
__global__ __launch_bounds__(256) void k_task_draw(DevModel M, DevState S, mssim_buffers B, unsigned what, mssim_draw_task T,
                                                    float* __restrict__ obs, float* __restrict__ reward, uint8_t* __restrict__ flags) {
  if (COPYOUT) (void)fetch_in_block(M, S, B, what);  // (ends with the block's barrier: every lane sees the rows)
  const int first = xcd_chunk(blockIdx.x, gridDim.x) * 64 + 16 * (int)(threadIdx.x >> 6);
  for (int it = 0; it < 4; it++) {
    if (first + 4 * it >= S.N) break;  // (wave-uniform)
    const int e = first + 4 * it + (int)((threadIdx.x & 63u) >> 4);
    task_draw_env(M, S, B, T, obs, reward, flags, e, (int)(threadIdx.x & 15u), e < S.N);
  }
}

// PushT pseudo-render (push_t.py pseudo_render_intersection): every template pixel (i, j) of the block's T, at its uv
// grid centre (U[j], V[i], 1), is mapped by world_to_goal @ tee_to_world, divided by the third row, scaled to pixel
// indices and truncated toward zero (.long()); an index outside [0, 64) sends the pixel to (0, 0). Index pair (x, y)
// lands on image row 63 - y, column x (the reference's permute + flip), so (0, 0) lands on row 63, column 0, which the
// template does not cover. The result counts the template pixels hit by at least one mapped pixel.
// Runs on the 16 lanes c = 0..15 of one env (all of them call it): each lane maps the template words c, c + 16, ...
// and sets bits of the env's 128-word bitmap `bm` in LDS; then AND with the template, popcount, and a sum over the
// 16 lanes. Every lane returns the count.
MS_DEV void pusht_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
MS_DEV int pusht_intersection16(const int32_t* __restrict__ K, float px, float py, float yaw, int c, unsigned* bm) {
  for (int w = c; w < 128; w += 16) bm[w] = 0u;
  pusht_wave_sync();
  // tee_to_goal = world_to_goal @ [[cos, -sin, px], [sin, cos, py], [0, 0, 1]] (quat_to_zrot + the translation)
  const float ca = cosf(yaw), sa = sinf(yaw);
  float W[9], T[9];
#pragma unroll
  for (int k = 0; k < 9; k++) W[k] = __int_as_float(K[MSSIM_PUSHT_W2G + k]);
#pragma unroll
  for (int r = 0; r < 3; r++) {
    T[3 * r + 0] = W[3 * r + 0] * ca + W[3 * r + 1] * sa;
    T[3 * r + 1] = W[3 * r + 0] * -sa + W[3 * r + 1] * ca;
    T[3 * r + 2] = W[3 * r + 0] * px + W[3 * r + 1] * py + W[3 * r + 2];
  }
  const float scale = (float)(64.0 / 2.0 / 0.15);  // (res / 2) / uv_half_width: a double, cast to f32 by the torch op
  for (int w = c; w < 128; w += 16) {
    unsigned bits = (unsigned)K[MSSIM_PUSHT_TEMPLATE + w];
    while (bits) {
      const int p = 32 * w + (__ffs(bits) - 1);
      bits &= bits - 1u;
      const float u = __int_as_float(K[MSSIM_PUSHT_U + (p & 63)]), v = __int_as_float(K[MSSIM_PUSHT_V + (p >> 6)]);
      const float hx = T[0] * u + T[1] * v + T[2], hy = T[3] * u + T[4] * v + T[5], hw = T[6] * u + T[7] * v + T[8];
      const float fx = truncf(__fdiv_rn(hx, hw) * scale + 32.f), fy = truncf(__fdiv_rn(hy, hw) * scale + 32.f);
      const bool ok = fx >= 0.f && fx < 64.f && fy >= 0.f && fy < 64.f;  // (false for NaN as well)
      const int x = ok ? (int)fx : 0, y = ok ? (int)fy : 0;
      const int bit = 64 * (63 - y) + x;
      atomicOr(bm + (bit >> 5), 1u << (bit & 31));
    }
  }
  pusht_wave_sync();
  int cnt = 0;
  for (int w = c; w < 128; w += 16) cnt += __popc(bm[w] & (unsigned)K[MSSIM_PUSHT_TEMPLATE + w]);
  cnt += __shfl_xor(cnt, 8, 16);
  cnt += __shfl_xor(cnt, 4, 16);
  cnt += __shfl_xor(cnt, 2, 16);
  cnt += __shfl_xor(cnt, 1, 16);
  return cnt;
}

// PushT evaluate / obs / reward (push_t.py evaluate, _get_obs_extra, compute_dense_reward) on the env's 16 lanes: the
// intersection over all of them, the rest on lane 0. `bm`: the env's 128 words of LDS.
MS_DEV void task_pusht_env(const DevModel& M, const DevState& S, const mssim_buffers& B, const mssim_pusht_task& T, float* __restrict__ obs,
                           float* __restrict__ reward, uint8_t* __restrict__ flags, float* __restrict__ inter_out, int e, int c, unsigned* bm) {
  const int N = S.N;
  const int n = M.n_dof;
  auto rowp = [&](int row) { return B.rigid_body_data + 13 * ((size_t)row * N + e); };
  const float* tee = rowp(T.tee_row);
  const float tx = tee[0], ty = tee[1], tz = tee[2], qw = tee[3], qz = tee[6];
  // quat_to_z_euler: 2 acos(sign(q_z) q_w), sign(0) = +1
  const float yaw = 2.f * acosf(qz < 0.f ? -qw : qw);
  const int cnt = pusht_intersection16(T.consts, tx, ty, yaw, c, bm);
  if (c != 0) return;
  const float frac = __fdiv_rn((float)cnt, (float)T.consts[MSSIM_PUSHT_AREA]);
  const bool success = frac >= T.intersection_thresh;
  float* o = obs + (size_t)e * (2 * n + 17);
  for (int j = 0; j < n; j++) {
    o[j] = B.art_qpos[(size_t)e * n + j];
    o[n + j] = B.art_qvel[(size_t)e * n + j];
  }
  const float* tcp = rowp(T.tcp_row);
  const float* gl = rowp(T.goal_row);
  int k = 2 * n;
  for (int i = 0; i < 7; i++) o[k++] = tcp[i];
  for (int i = 0; i < 3; i++) o[k++] = gl[i];
  for (int i = 0; i < 7; i++) o[k++] = tee[i];
  // dense reward: rotation, planar distance to the goal, tcp near the block
  const float rot = (cosf(yaw - T.goal_z_rot) + 1.f) / 2.f;
  float r = rot * rot / 2.f;
  const float dx = tx - gl[0], dy = ty - gl[1];
  const float dg = 1.f - tanhf(5.f * __fsqrt_rn(dx * dx + dy * dy));
  r += dg * dg / 2.f;
  const f3 d3 = f3{tx - tcp[0], ty - tcp[1], tz - tcp[2]};
  // 1 - tanh x as 2 / (e^2x + 1): far from the block 1 - tanhf cancels to a few ulp of 1, which the square root
  // magnifies 100-fold (7.6e-7 against float64 at 1.2 m, tests/test_gpu_task_epilogues.py); x >= 0, e^2x = inf gives 0
  r += __fsqrt_rn(__fdiv_rn(2.f, expf(10.f * __fsqrt_rn(dot(d3, d3))) + 1.f)) / 20.f;
  if (success) r = 3.f;
  reward[e] = __fdiv_rn(r, T.reward_div);
  flags[e] = success;
  if (inter_out) inter_out[e] = (float)cnt;
  if (T.terminated_out) T.terminated_out[e] = success;
  if (T.elapsed_steps) { const int v = T.elapsed_steps[e] + 1; T.elapsed_steps[e] = v; if (T.elapsed_out) T.elapsed_out[e] = v; if (T.truncated_out) T.truncated_out[e] = v >= T.time_limit ? 1 : 0; }
}
// 16 lanes per env, 16 envs per block of 256 threads, 512 B of LDS per env. FETCH: the launch first performs
// mssim_fetch(what) for its envs, the rows of an env strided over its 16 lanes (all in one wave).
template <bool FETCH>
__global__ __launch_bounds__(256) void k_task_pusht(DevModel M, DevState S, mssim_buffers B, unsigned what, mssim_pusht_task T, float* __restrict__ obs,
                                                     float* __restrict__ reward, uint8_t* __restrict__ flags, float* __restrict__ inter_out) {
  __shared__ unsigned bm[16 * 128];
  const int c = threadIdx.x & 15, le = threadIdx.x >> 4;
  const int e = xcd_chunk(blockIdx.x, gridDim.x) * 16 + le;
  if (e >= S.N) return;  // (whole 16-lane groups)
  if (FETCH) {
    const int R = M.n_link + M.n_free + M.n_kin;
    for (int row = c; row < R; row += 16) fetch_row(M, S, B, what, e, row);
    for (int j = c; j < M.n_dof; j += 16) fetch_art_joint(M, S, B, what, e, j);
    __threadfence_block();
    pusht_wave_sync();
  }
  task_pusht_env(M, S, B, T, obs, reward, flags, inter_out, e, c, bm + 128 * le);
}

// geometric Jacobian of link `link` in the root frame: out [N][6][n_dof] (see include/mssim.h)
__global__ void k_link_jacobian(DevModel M, DevState S, int link, float* __restrict__ out) {
  const int N = S.N;
  int e = xcd_chunk(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x;
  if (e >= N) return;
  const int n = M.n_dof;
  const pose_t root = pose_soa(S.root, 0, N, e);
  const m3 Rr = qmat(root.q);
  const int b = M.link_body[link];
  const pose_t Pb = b < 0 ? root : pose_soa(S.bodypose, 7 * b, N, e);
  const f3 pe = pmul(Pb, pose_from(M.link_frame + 7 * link)).p;
  const unsigned path = b < 0 ? 0u : (M.dof_anc[b] | (1u << b));
  float* o = out + (size_t)e * 6 * n;
  for (int j = 0; j < n; j++) {
    f3 jv = f3{0, 0, 0}, jw = f3{0, 0, 0};
    if ((path >> j) & 1u) {
      const f3 a = f3{SOA(S.bodyaux, 6 * j), SOA(S.bodyaux, 6 * j + 1), SOA(S.bodyaux, 6 * j + 2)};
      const f3 an = f3{SOA(S.bodyaux, 6 * j + 3), SOA(S.bodyaux, 6 * j + 4), SOA(S.bodyaux, 6 * j + 5)};
      if (M.dof_type[j] == MSSIM_JOINT_REVOLUTE) { jv = cross(a, pe - an); jw = a; }
      else jv = a;
      jv = mtmulv(Rr, jv);
      jw = mtmulv(Rr, jw);
    }
    o[0 * n + j] = jv.x; o[1 * n + j] = jv.y; o[2 * n + j] = jv.z;
    o[3 * n + j] = jw.x; o[4 * n + j] = jw.y; o[5 * n + j] = jw.z;
  }
}

__global__ void k_fill(float* dst, float v, size_t count) {
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i < count) dst[i] = v;
}
__global__ void k_i2f(const int* src, float* dst, size_t count) {
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i < count) dst[i] = (float)src[i];
}

// =================================================================================================
// host side
#include "mssim_solve16.h"
#include "mssim_model_pack.h"
#include "mssim_dispatch.h"

// every compiled instance of the control-step kernel, in the order of mssim_dispatch::kInstances
using solve16_fn = void (*)(DevModel, DevState, int);
#define MSSIM_SOLVE16_FN_(NDOF, TASK, TRI, NR) k_solve16<NDOF, TASK, TRI, NR>,
static const solve16_fn kSolve16[] = {MSSIM_SOLVE16_INSTANCES(MSSIM_SOLVE16_FN_)};
#undef MSSIM_SOLVE16_FN_
static_assert(S16_ENVS_PER_BLOCK == 4, "mssim_dispatch::tail_fits counts waves of 4 envs");

// What is owed to the next call on the handle (settle() performs it). mssim_defer_step_action: a step_action; a task
// epilogue runs it, the copy-out and itself as ONE launch of the control-step kernel. mssim_defer_fetch: a copy-out.
struct Owed {
  const float* action = nullptr; int adim = 0, nsub = 0; hipStream_t stream = nullptr;
  unsigned fetch = 0u;
};

struct RcObject;  // a ray-cast scene with its cameras (mssim_raycast.h)

struct mssim_sim {
  int device = 0;
  int N = 0;
  DevModel M{};
  DevState S{};
  mssim_buffers buf{};
  std::vector<void*> allocs;
  std::vector<float> drive_host;
  float* d_drive = nullptr;
  bool panda = false;
  bool has_tri = false;  // the model has triangle-mesh shapes: control steps run the kernel variant with the mesh stage
  int rows_per_env = 1;  // 16-lane rows an env takes in the control-step kernel (its template parameter NR): 2 when the model has more than 16 velocity components
  bool dirty = true;
  int n_cu = 256;  // compute units of the device
  // the control-step kernel of this model (mssim_dispatch.h, resolved by mssim_create): the plain step, and per task id
  // the instance with that task's epilogue at its tail (null: the epilogue is a launch of its own)
  solve16_fn step_fn = nullptr, tail_fn[mssim_dispatch::kNumTasks] = {};
  dim3 step_grid;
  Owed owed;
  std::vector<float> h_dof_pack; float* d_dof_pack = nullptr;  // (drive gains are patched by set_drive_properties)
  std::vector<int32_t> h_shape_row, h_pair_shape;  // host copies (contact-pair lists of the task epilogues)
  // finger <-> object candidate pairs of the task epilogue that asked last, and the (object, finger, finger) rows they are for
  int* d_finger_pairs = nullptr; int n_finger_pairs = 0; int finger_pair_rows[3] = {-1, -1, -1};
  long long n_tail_steps = 0;  // control steps that ran with the task epilogue at the kernel's tail (mssim_tail_step_count)
  mssim_task_robot task_robot = {};  // mssim_set_task_robot; n_ranges == 0: the rules of the task structs (the Panda's)
  std::vector<int*> queries;
  std::vector<int> query_n;
  std::vector<int> query_kind;
  std::vector<std::shared_ptr<RcObject>> raycasts;  // by id; a destroyed one leaves an empty entry
  std::string err;
  int* d_act_col = nullptr; float* d_act_lo = nullptr; float* d_act_hi = nullptr; int* d_act_flags = nullptr;
  EeMap ee{-1, 0, 3, 0.f, 0.f, 0.f, 0};
  IkChain ik = [] { IkChain c{}; c.link = -1; return c; }();  // iterative-IK block (mssim_set_ee_ik_map); excludes `ee`
  float* ik_target_pose = nullptr;                            // the caller's [N][7] state of that block
  int act_max_col = -1;  // highest action column the joint map reads
  // profiling (bench roofline block): event pairs recorded on the launch stream
  bool profiling = false;
  std::vector<hipEvent_t> ev[2];  // [kernel] start/stop interleaved
  size_t ev_used[2] = {0, 0};
};

static std::string g_create_error;

#define HIPCHK(h, call)                                                                   \
  do {                                                                                    \
    hipError_t _e = (call);                                                               \
    if (_e != hipSuccess) {                                                               \
      std::string _m = std::string(#call) + ": " + hipGetErrorString(_e);                 \
      if (h) (h)->err = _m; else g_create_error = _m;                                     \
      return 100 + (int)_e;                                                               \
    }                                                                                     \
  } while (0)

template <typename Tt>
static int upload(mssim_sim* S, const Tt* src, size_t count, const Tt** dst) {
  void* d = nullptr;
  size_t bytes = (count > 0 ? count : 1) * sizeof(Tt);
  HIPCHK(S, hipMalloc(&d, bytes));
  S->allocs.push_back(d);
  if (count > 0 && src) HIPCHK(S, hipMemcpy(d, src, count * sizeof(Tt), hipMemcpyHostToDevice));
  else HIPCHK(S, hipMemset(d, 0, bytes));
  *dst = (const Tt*)d;
  return 0;
}
template <typename Tt>
static int dalloc(mssim_sim* S, size_t count, Tt** dst) {
  void* d = nullptr;
  size_t bytes = (count > 0 ? count : 1) * sizeof(Tt);
  HIPCHK(S, hipMalloc(&d, bytes));
  HIPCHK(S, hipMemset(d, 0, bytes));
  S->allocs.push_back(d);
  *dst = (Tt*)d;
  return 0;
}
static int dset(mssim_sim* S, float* dst, int byte, size_t count) {
  HIPCHK(S, hipMemset(dst, byte, count * sizeof(float)));
  return 0;
}
static int dput(mssim_sim* S, float* dst, const std::vector<float>& v) {
  HIPCHK(S, hipMemcpy(dst, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
  return 0;
}

static inline int pad8(int n) { return (n + 7) / 8 * 8; }
static inline dim3 env_grid(int N, int block) { return dim3(pad8((N + block - 1) / block)); }  // kernels map blocks with xcd_chunk

// The kernel pointers of the model's control step. find_instance(plain) is never -1: mssim_dispatch.h proves at compile
// time (plain_steps_compiled) that the list holds plain_step() of every model with at most 16 joints and 1, 2 or 4 rows,
// which is all validate_model (mssim_model_pack.h) lets through -- relax that limit and that proof together. A tail has
// the rows per env, so the grid, of the plain step.
static void resolve_control_step(mssim_sim* S, int n_dof) {
  using namespace mssim_dispatch;
  static_assert(S16_LANES == 16, "plain_steps_compiled() covers n_dof <= 16");
  const Key plain = plain_step(n_dof, S->rows_per_env, S->has_tri);
  S->step_fn = kSolve16[find_instance(plain)];
  S->step_grid = env_grid(S->N, S16_WAVES * S16_ENVS_PER_BLOCK / plain.nr);
  for (int task = 1; task < kNumTasks; task++) {
    const Key tail = tail_step(task, n_dof, S->rows_per_env, S->has_tri, S->N, S->n_cu);
    if (!(tail == kNone)) S->tail_fn[task] = kSolve16[find_instance(tail)];
  }
}

extern "C" {

int mssim_abi_version(void) { return MSSIM_ABI_VERSION; }
const char* mssim_last_error(mssim_handle h) { return h ? h->err.c_str() : g_create_error.c_str(); }

void mssim_destroy(mssim_handle h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  for (void* p : h->allocs) (void)hipFree(p);
  for (int k = 0; k < 2; k++)
    for (auto& e : h->ev[k]) (void)hipEventDestroy(e);
  delete h;
}

// validate -> pack (mssim_model_pack.h: host only, a malformed model is turned down before the device is touched) ->
// upload -> initialise the state
int mssim_create(const mssim_model_desc* d, int32_t num_envs, int32_t device, mssim_handle* out) {
  if (!out) { g_create_error = "bad arguments"; return 1; }
  PackedModel P;
  int rc = validate_model(d, num_envs, &g_create_error);
  if (!rc) rc = pack_model(d, num_envs, &P, &g_create_error);
  if (rc) return rc;
  const hipError_t e0 = hipSetDevice(device);
  if (e0 != hipSuccess) { g_create_error = std::string("hipSetDevice: ") + hipGetErrorString(e0); return 6; }
  // The handle frees what it holds on every return but the last. The first device call that fails sets rc and its
  // message; every step after it is skipped, and the one failure exit is at the end.
  std::unique_ptr<mssim_sim, void (*)(mssim_sim*)> owner(new mssim_sim(), mssim_destroy);
  mssim_sim* S = owner.get();
  auto up = [&](const auto* src, size_t count, auto dst) { if (!rc) rc = upload(S, src, count, dst); };   // a model array
  auto upv = [&](const auto& v, auto dst) { up(v.data(), v.size(), dst); };                               // a packed table
  auto al = [&](size_t count, auto dst) { if (!rc) rc = dalloc(S, count, dst); };                         // zeroed state
  auto empty = [&](float* dst, size_t count) { if (!rc) rc = dset(S, dst, 0xFF, count); };                // all bits set: int -1 / NaN
  auto put = [&](float* dst, size_t at, const std::vector<float>& v) { if (!rc) rc = dput(S, dst + at, v); };
  S->device = device;
  S->N = num_envs;
  S->rows_per_env = P.rows_per_env;
  S->has_tri = P.has_tri;
  S->panda = P.panda;
  { int ncu = 0; if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && ncu > 0) S->n_cu = ncu; }
  const size_t n = d->n_dof, ns = d->n_shape, nf = d->n_free, np = d->n_pair, N = num_envs;
  S->h_shape_row.assign(d->shape_row, d->shape_row + ns);
  S->h_pair_shape.assign(d->pair_shape, d->pair_shape + 2 * np);

  DevModel& M = S->M;
  M.n_dof = d->n_dof; M.n_tendon = d->n_tendon; M.n_link = d->n_link; M.n_free = d->n_free; M.n_kin = d->n_kin;
  M.n_shape = d->n_shape; M.n_pair = d->n_pair;
  M.gx = d->gravity[0]; M.gy = d->gravity[1]; M.gz = d->gravity[2];
  M.dt = d->timestep; M.contact_offset = d->contact_offset; M.rest_offset = d->rest_offset; M.erp = d->erp;
  M.max_depen = d->max_depenetration_velocity; M.pos_iters = d->position_iterations; M.vel_iters = d->velocity_iterations;
  M.sleep_threshold = d->sleep_threshold;
  up(d->dof_parent, n, &M.dof_parent); up(d->dof_type, n, &M.dof_type); up(d->dof_frame, 7 * n, &M.dof_frame); up(d->dof_axis, 3 * n, &M.dof_axis);
  up(d->tendon_dof, 2 * (size_t)d->n_tendon, &M.tendon_dof); up(d->tendon_param, 5 * (size_t)d->n_tendon, &M.tendon_param);
  up(d->link_body, d->n_link, &M.link_body); up(d->link_frame, 7 * (size_t)d->n_link, &M.link_frame);
  up(d->free_inertial, 10 * nf, &M.free_inertial); up(d->free_damping, 2 * nf, &M.free_damping); up(d->free_gravity, nf, &M.free_gravity);
  up(d->shape_row, ns, &M.shape_row); up(d->pair_shape, 2 * np, &M.pair_shape);
  up(d->tri_soup, 12 * (size_t)d->n_tri, &M.tri_soup); up(d->tri_bvh, 112 * (size_t)d->n_tri_node, &M.tri_bvh);
  up(d->env_shape_frame, 7 * d->n_env_shape * N, &M.env_shape_frame); up(d->env_shape_bound, 4 * d->n_env_shape * N, &M.env_shape_bound);
  up(d->env_free_inertial, 10 * d->n_env_free * N, &M.env_free_inertial);
  upv(P.dof_anc, &M.dof_anc); upv(P.dof_pack, &M.dof_pack); upv(P.shape_pack, &M.shape_pack);
  upv(P.shape_hull, &M.shape_hull); upv(P.hull_verts, &M.hull_verts); upv(P.env_shape_param, &M.env_shape_param);
  upv(P.free_env_slot, &M.free_env_slot); upv(P.pair_mesh_slot, &M.pair_mesh_slot); upv(P.pair_packed, &M.pair_packed);
  S->h_dof_pack = std::move(P.dof_pack);
  S->d_dof_pack = const_cast<float*>(M.dof_pack);
  // tables from before shape_pack / dof_pack that no kernel reads
  up(d->body_gravity, n, &M.body_gravity); up(d->dof_limit, 2 * n, &M.dof_limit); up(d->dof_drive, 4 * n, &M.dof_drive);
  up(d->dof_armature, n, &M.dof_armature); up(d->body_inertial, 10 * n, &M.body_inertial);
  up(d->shape_type, ns, &M.shape_type); up(d->shape_body_kind, ns, &M.shape_kind); up(d->shape_body_index, ns, &M.shape_index);
  up(d->shape_frame, 7 * ns, &M.shape_frame); up(d->shape_param, 4 * ns, &M.shape_param); up(d->shape_material, 4 * ns, &M.shape_material);
  up(d->shape_bound, 4 * ns, &M.shape_bound); up(P.shape_center.data(), 3 * ns, &M.shape_center); up(P.shape_half.data(), 3 * ns, &M.shape_half);
  upv(P.shape_env_slot, &M.shape_env_slot);
  S->d_drive = const_cast<float*>(M.dof_drive);

  DevState& D = S->S;
  D.N = num_envs;
  al(7 * N, &D.root); al(n * N, &D.q); al(n * N, &D.qd); al(n * N, &D.qt); al(n * N, &D.qdt); al(n * N, &D.qf); al(n * N, &D.qacc);
  al(13 * nf * N, &D.free_s); al(3 * nf * N, &D.free_force); al(nf * N, &D.free_wake); al(7 * d->n_kin * N, &D.kin);
  al(7 * n * N, &D.bodypose); al(6 * n * N, &D.bodyvel); al(6 * n * N, &D.bodyaux);
  al(np * N, &D.pair_cnt); al(3 * np * N, &D.pair_imp); al((1 + MAXC) * N, &D.hit_list); al(N, &D.overflow); al(N, &D.pcm_tick);
  al(N * S16_ROWS_GLB * S16_ROWLEN_(S->rows_per_env), &D.rows);
  // caches start empty: manifold slots with pair = -1, multipliers with stamp = -1 (nothing to start from), and no
  // clearance known for any (convex shape, mesh) pair (mssim_solve16.h stage T0)
  const size_t n_pcm = N * MSSIM_PCM_SLOTS * S16_PCM_LEN, n_warm = 4 * (np > 0 ? np : 1) * N * 4, n_clear = 4 * (size_t)(P.n_mesh_pair > 0 ? P.n_mesh_pair : 1) * N;
  al(n_pcm, &D.pcm); empty(D.pcm, n_pcm);
  al(n_warm, &D.warm); empty(D.warm, n_warm);
  al(n_clear, &D.tri_clear); empty(D.tri_clear, n_clear);
  // identity quaternions; every free body awake
  const std::vector<float> ones(N, 1.0f);
  put(D.root, 3 * N, ones);
  for (size_t b = 0; b < nf; b++) put(D.free_s, (13 * b + 3) * N, ones);
  for (size_t k = 0; k < (size_t)d->n_kin; k++) put(D.kin, (7 * k + 3) * N, ones);
  if (nf > 0) put(D.free_wake, 0, std::vector<float>(nf * N, MSSIM_WAKE_TIME));
  if (rc) { g_create_error = S->err; return rc; }
  resolve_control_step(S, d->n_dof);
  *out = owner.release();
  return 0;
}

static void settle(mssim_handle h, hipStream_t st, bool keep_fetch = false);
int mssim_bind_buffers(mssim_handle h, const mssim_buffers* b) {
  if (h) settle(h, (hipStream_t)0);
  if (!h || !b) return 1;
  h->buf = *b;
  return 0;
}

int mssim_set_timestep(mssim_handle h, float dt) {
  settle(h, h->owed.stream);
  if (!(dt > 0.f)) { h->err = "timestep must be positive"; return 1; }
  h->M.dt = dt;
  return 0;
}
float mssim_get_timestep(mssim_handle h) { return h->M.dt; }

int mssim_set_drive_properties(mssim_handle h, const float* drive) {
  settle(h, h->owed.stream);
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpy(h->d_drive, drive, sizeof(float) * 4 * h->M.n_dof, hipMemcpyHostToDevice));
  for (int j = 0; j < h->M.n_dof; j++)
    for (int k = 0; k < 4; k++) h->h_dof_pack[32 * (size_t)j + 13 + k] = drive[4 * j + k];
  HIPCHK(h, hipMemcpy(h->d_dof_pack, h->h_dof_pack.data(), sizeof(float) * h->h_dof_pack.size(), hipMemcpyHostToDevice));
  return 0;
}

int mssim_apply(mssim_handle h, uint32_t what, void* stream) {
  settle(h, (hipStream_t)stream);
  hipLaunchKernelGGL(k_apply, env_grid(h->N, 256), dim3(256), 0, (hipStream_t)stream, h->M, h->S, h->buf, what);
  h->dirty = true;
  HIPCHK(h, hipGetLastError());
  return 0;
}

static void launch_fetch(mssim_handle h, unsigned what, hipStream_t st) {
  hipLaunchKernelGGL(k_fetch, dim3(pad8((h->N + 63) / 64), h->M.n_link + h->M.n_free + h->M.n_kin + 1), dim3(64), 0, st, h->M, h->S, h->buf, what);
}
int mssim_defer_fetch(mssim_handle h, uint32_t what) {
  h->owed.fetch |= what;
  return 0;
}

int mssim_fetch(mssim_handle h, uint32_t what, void* stream) {
  settle(h, (hipStream_t)stream, /*keep_fetch=*/true);  // the owed copy-out joins this one
  launch_fetch(h, what | std::exchange(h->owed.fetch, 0u), (hipStream_t)stream);
  HIPCHK(h, hipGetLastError());
  return 0;
}

static void launch_fk(mssim_handle h, hipStream_t st) {
  if (h->panda) hipLaunchKernelGGL(k_fk<TopoPanda>, env_grid(h->N, 64), dim3(64), 0, st, h->M, h->S);
  else hipLaunchKernelGGL(k_fk<TopoDyn>, env_grid(h->N, 64), dim3(64), 0, st, h->M, h->S);
}
static void fk_if_dirty(mssim_handle h, hipStream_t st) {
  if (h->dirty) { launch_fk(h, st); h->dirty = false; }
}

int mssim_wake_all(mssim_handle h, void* stream) {
  settle(h, (hipStream_t)stream);
  const size_t cnt = (size_t)h->M.n_free * h->N;
  if (cnt > 0) hipLaunchKernelGGL(k_fill, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, (hipStream_t)stream, h->S.free_wake, MSSIM_WAKE_TIME, cnt);
  HIPCHK(h, hipMemsetAsync(h->S.pcm, 0xFF, (size_t)h->N * MSSIM_PCM_SLOTS * S16_PCM_LEN * sizeof(float), (hipStream_t)stream));  // every slot empty
  HIPCHK(h, hipMemsetAsync(h->S.warm, 0xFF, (size_t)16 * (h->M.n_pair > 0 ? h->M.n_pair : 1) * h->N * sizeof(float), (hipStream_t)stream));
  HIPCHK(h, hipGetLastError());
  return 0;
}

// hidden state of the listed envs back to "fresh": every free body awake, manifold cache empty, no multipliers to start from
__global__ void k_wake_envs(DevModel M, DevState S, const long long* __restrict__ idx, int n_idx) {
  const int N = S.N;
  if ((int)blockIdx.x >= n_idx) return;
  const long long e64 = idx[blockIdx.x];
  if (e64 < 0 || e64 >= N) return;
  const int e = (int)e64;
  for (int b = threadIdx.x; b < M.n_free; b += blockDim.x) SOA(S.free_wake, b) = MSSIM_WAKE_TIME;
  for (int s = threadIdx.x; s < MSSIM_PCM_SLOTS; s += blockDim.x) reinterpret_cast<int*>(S.pcm)[((size_t)e * MSSIM_PCM_SLOTS + s) * S16_PCM_LEN] = -1;  // pair = -1: slot empty
  for (int k = threadIdx.x; k < 4 * M.n_pair; k += blockDim.x) reinterpret_cast<int*>(S.warm)[((size_t)k * N + e) * 4 + 3] = -1;  // stamp -1
}
int mssim_wake_envs(mssim_handle h, const int64_t* env_idx, int32_t n_idx, void* stream) {
  settle(h, (hipStream_t)stream);
  if (n_idx <= 0) return 0;
  if (!env_idx) { h->err = "wake_envs: no index array"; return 1; }
  hipLaunchKernelGGL(k_wake_envs, dim3((unsigned)n_idx), dim3(256), 0, (hipStream_t)stream, h->M, h->S, reinterpret_cast<const long long*>(env_idx), (int)n_idx);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int mssim_update_kinematics(mssim_handle h, void* stream) {
  settle(h, (hipStream_t)stream);
  launch_fk(h, (hipStream_t)stream);
  h->dirty = false;
  HIPCHK(h, hipGetLastError());
  return 0;
}

static inline void prof_mark(mssim_handle h, int k, hipStream_t st) {
  if (!h->profiling || h->ev_used[k] >= h->ev[k].size()) return;
  (void)hipEventRecord(h->ev[k][h->ev_used[k]++], st);
}

// one control step: `k` is the handle's step_fn or one of its tail_fn (whose epilogue reads S.tail_*)
static void launch_control_step(mssim_handle h, solve16_fn k, const DevState& S, int n_substeps, hipStream_t st) {
  prof_mark(h, 0, st);
  hipLaunchKernelGGL(k, h->step_grid, dim3(64 * S16_WAVES), 0, st, h->M, S, n_substeps);
  prof_mark(h, 0, st);
}
static int step_now(mssim_handle h, const DevState& S, int n_substeps, hipStream_t st) {
  fk_if_dirty(h, st);
  if (n_substeps > 0) launch_control_step(h, h->step_fn, S, n_substeps, st);
  HIPCHK(h, hipGetLastError());
  return 0;
}
int mssim_step(mssim_handle h, int32_t n_substeps, void* stream) {
  settle(h, (hipStream_t)stream);
  return step_now(h, h->S, (int)n_substeps, (hipStream_t)stream);
}

static DevState state_with_action(mssim_handle h, const float* action, int action_dim) {
  DevState S = h->S;
  S.act = action; S.act_dim = action_dim;
  S.act_col = h->d_act_col; S.act_lo = h->d_act_lo; S.act_hi = h->d_act_hi; S.act_flags = h->d_act_flags;
  S.act_qpos = h->buf.art_qpos; S.act_target = h->buf.art_target_qpos; S.act_target_vel = h->buf.art_target_qvel;
  return S;
}
// every column the maps read must exist: the kernels index action[env * action_dim + column] unchecked
static int check_action_dim(mssim_handle h, int32_t action_dim) {
  if (!h->d_act_col) { h->err = "set_action_map has not been called"; return 1; }
  const int need = std::max({h->act_max_col + 1, h->ee.link >= 0 ? h->ee.col0 + h->ee.rows : 0, h->ik.link >= 0 ? h->ik.col0 + h->ik.rows : 0});
  if (action_dim < need) {
    h->err = "action has " + std::to_string(action_dim) + " columns, the action map reads " + std::to_string(need);
    return 2;
  }
  return 0;
}
// the iterative-IK launch, either form: a chain with held joints starts from their composed transform (mssim_ik.h)
static void launch_ee_ik(mssim_handle h, const IkIo& io, hipStream_t st) {
  auto k = h->ik.n_held > 0 ? (h->ik.rows == 6 ? k_ee_ik<6, true> : k_ee_ik<3, true>) : (h->ik.rows == 6 ? k_ee_ik<6, false> : k_ee_ik<3, false>);
  hipLaunchKernelGGL(k, env_grid(h->N, 64), dim3(64), 0, st, h->ik, h->S, h->buf, h->M.n_dof, io);
}
static void launch_apply_action(mssim_handle h, const float* action, int action_dim, hipStream_t st) {
  hipLaunchKernelGGL(k_apply_action, env_grid(h->N, 256), dim3(256), 0, st, h->M, h->S, h->buf, action, action_dim,
                     h->d_act_col, h->d_act_lo, h->d_act_hi, h->d_act_flags, h->ee);
  if (h->ik.link >= 0) {  // the joint-space rows are written; the iterative-IK block follows in a launch of its own
    const IkIo io{action, action_dim, h->d_act_flags, h->ik_target_pose, nullptr, nullptr, nullptr};
    launch_ee_ik(h, io, st);
  }
}
static int step_action_now(mssim_handle h, const float* action, int32_t action_dim, int32_t n_substeps, hipStream_t st) {
  if (n_substeps <= 0 || h->ee.link >= 0 || h->ik.link >= 0) {  // end-effector block: apply_action, then step
    launch_apply_action(h, action, action_dim, st);
    return step_now(h, h->S, n_substeps, st);
  }
  return step_now(h, state_with_action(h, action, action_dim), n_substeps, st);
}
// Everything owed to the handle, in order: the step on the stream it was deferred on, then the copy-out on `st`. Every
// entry point that touches the state or the buffers calls this first, so a deferral is only an ordering of launches,
// never a change of results. `keep_fetch`: the copy-out stays owed to the caller, which performs it inside its own
// launch (a task epilogue: k_task_*<true>).
static void settle(mssim_handle h, hipStream_t st, bool keep_fetch) {
  if (h->owed.action) {
    const float* a = h->owed.action;
    h->owed.action = nullptr;
    (void)step_action_now(h, a, h->owed.adim, h->owed.nsub, h->owed.stream);
  }
  if (!keep_fetch && h->owed.fetch) launch_fetch(h, std::exchange(h->owed.fetch, 0u), st);
}

int mssim_step_action(mssim_handle h, const float* action, int32_t action_dim, int32_t n_substeps, void* stream) {
  if (int rc = check_action_dim(h, action_dim)) return rc;
  settle(h, (hipStream_t)stream);
  return step_action_now(h, action, action_dim, n_substeps, (hipStream_t)stream);
}

int mssim_defer_step_action(mssim_handle h, const float* action, int32_t action_dim, int32_t n_substeps, void* stream) {
  if (int rc = check_action_dim(h, action_dim)) return rc;
  settle(h, (hipStream_t)stream);
  h->owed.action = action; h->owed.adim = action_dim; h->owed.nsub = n_substeps; h->owed.stream = (hipStream_t)stream;
  return 0;
}

int mssim_link_jacobian(mssim_handle h, int32_t link_index, float* out, void* stream) {
  settle(h, (hipStream_t)stream);
  if (link_index < 0 || link_index >= h->M.n_link || !out) { h->err = "link_jacobian: bad link index / output"; return 1; }
  hipStream_t st = (hipStream_t)stream;
  fk_if_dirty(h, st);
  hipLaunchKernelGGL(k_link_jacobian, env_grid(h->N, 256), dim3(256), 0, st, h->M, h->S, (int)link_index, out);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int mssim_profile_enable(mssim_handle h, int32_t on) {
  HIPCHK(h, hipSetDevice(h->device));
  if (on && h->ev[0].empty()) {
    for (int k = 0; k < 2; k++) {
      h->ev[k].resize(2 * 4096);
      for (auto& e : h->ev[k]) HIPCHK(h, hipEventCreate(&e));
    }
  }
  h->profiling = on != 0;
  h->ev_used[0] = h->ev_used[1] = 0;
  return 0;
}

int mssim_profile_read(mssim_handle h, float* out_ms, int32_t* out_counts) {
  settle(h, h->owed.stream);
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipDeviceSynchronize());
  for (int k = 0; k < 2; k++) {
    float total = 0.f;
    size_t pairs = h->ev_used[k] / 2;
    for (size_t i = 0; i < pairs; i++) {
      float ms = 0.f;
      HIPCHK(h, hipEventElapsedTime(&ms, h->ev[k][2 * i], h->ev[k][2 * i + 1]));
      total += ms;
    }
    out_ms[k] = total;
    out_counts[k] = (int32_t)pairs;
    h->ev_used[k] = 0;
  }
  return 0;
}

int mssim_set_action_map(mssim_handle h, const int32_t* column, const float* low, const float* high, const int32_t* flags) {
  settle(h, h->owed.stream);
  HIPCHK(h, hipSetDevice(h->device));
  const int n = h->M.n_dof > 0 ? h->M.n_dof : 1;
  for (int j = 0; j < h->M.n_dof; j++)
    if ((flags[j] & 48) && (((flags[j] >> 8) & 31) >= h->M.n_dof || (flags[j] & 48) == 48)) { h->err = "set_action_map: base-frame flags need one of cos / sin and a yaw joint of the articulation"; return 1; }
  if (!h->d_act_col) {
    int rc;
    if ((rc = dalloc(h, n, &h->d_act_col)) || (rc = dalloc(h, n, &h->d_act_lo)) || (rc = dalloc(h, n, &h->d_act_hi)) || (rc = dalloc(h, n, &h->d_act_flags))) return rc;
  }
  HIPCHK(h, hipMemcpy(h->d_act_col, column, sizeof(int) * h->M.n_dof, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(h->d_act_lo, low, sizeof(float) * h->M.n_dof, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(h->d_act_hi, high, sizeof(float) * h->M.n_dof, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(h->d_act_flags, flags, sizeof(int) * h->M.n_dof, hipMemcpyHostToDevice));
  h->act_max_col = -1;
  for (int j = 0; j < h->M.n_dof; j++) h->act_max_col = column[j] > h->act_max_col ? column[j] : h->act_max_col;
  return 0;
}

int mssim_set_ee_action_map(mssim_handle h, int32_t link_index, int32_t column0, int32_t rows, float low, float high, float rot_scale, int32_t flags) {
  settle(h, h->owed.stream);
  if (link_index >= h->M.n_link || (link_index >= 0 && rows != 3 && rows != 6)) { h->err = "set_ee_action_map: bad link index / rows"; return 1; }
  h->ee = EeMap{link_index < 0 ? -1 : (int)link_index, (int)column0, (int)rows, low, high, rot_scale, (int)flags};
  if (link_index >= 0) h->ik.link = -1;  // the two end-effector blocks exclude each other
  return 0;
}

// a small constant table of the model back on the host (set-time only)
extern "C++" {
template <typename Tt>
static int download(mssim_handle h, const Tt* src, size_t count, std::vector<Tt>* dst) {
  dst->resize(count);
  if (count > 0) HIPCHK(h, hipMemcpy(dst->data(), src, count * sizeof(Tt), hipMemcpyDeviceToHost));
  return 0;
}
}

int mssim_set_ee_ik_map(mssim_handle h, const mssim_ee_ik_map* map, float* target_pose) {
  settle(h, h->owed.stream);
  if (!map) { h->err = "set_ee_ik_map: no map"; return 1; }
  if (map->link_index < 0) { h->ik.link = -1; h->ik_target_pose = nullptr; return 0; }
  const DevModel& M = h->M;
  if (map->link_index >= M.n_link || (map->rows != 3 && map->rows != 6) || (map->mode != 0 && map->mode != 1) || map->column0 < 0 || map->max_iters < 0) {
    h->err = "set_ee_ik_map: bad link index / rows / mode / column / iteration count"; return 1;
  }
  if (!target_pose) { h->err = "set_ee_ik_map: no target_pose buffer"; return 1; }
  if (!h->d_act_flags) { h->err = "set_ee_ik_map: set_action_map has not been called"; return 1; }
  HIPCHK(h, hipSetDevice(h->device));
  std::vector<int> parent, type, link_body, flags;
  std::vector<float> frame, axis, limit, link_frame;
  int rc;
  if ((rc = download(h, M.dof_parent, (size_t)M.n_dof, &parent)) || (rc = download(h, M.dof_type, (size_t)M.n_dof, &type)) ||
      (rc = download(h, M.link_body, (size_t)M.n_link, &link_body)) || (rc = download(h, (const int*)h->d_act_flags, (size_t)M.n_dof, &flags)) ||
      (rc = download(h, M.dof_frame, (size_t)7 * M.n_dof, &frame)) || (rc = download(h, M.dof_axis, (size_t)3 * M.n_dof, &axis)) ||
      (rc = download(h, M.dof_limit, (size_t)2 * M.n_dof, &limit)) || (rc = download(h, M.link_frame, (size_t)7 * M.n_link, &link_frame)))
    return rc;
  std::vector<int> path;
  for (int b = link_body[map->link_index]; b >= 0; b = parent[b]) path.insert(path.begin(), b);
  if (path.empty()) { h->err = "set_ee_ik_map: the link has no joint on its path"; return 1; }
  // every path joint is solved (flagged 4) or held (flagged 64: another controller's, kept where it is)
  std::vector<int> solved, held;
  for (int j : path) {
    if (flags[j] & 4) solved.push_back(j);
    else if (flags[j] & 64) held.push_back(j);
    else { h->err = "set_ee_ik_map: dof " + std::to_string(j) + " is on the link's path but not flagged 4 in the joint map"; return 1; }
  }
  if ((int)solved.size() > MSSIM_IK_MAX_JOINTS) {
    h->err = "set_ee_ik_map: the link has " + std::to_string(solved.size()) + " joints" + (held.empty() ? "" : " flagged 4") + " on its path, the iterative IK takes at most " + std::to_string(MSSIM_IK_MAX_JOINTS);
    return 1;
  }
  if (solved.empty()) { h->err = "set_ee_ik_map: every joint on the link's path is held (flagged 64), none is left to solve for"; return 1; }
  for (size_t k = 0; k < held.size(); k++)
    if (path[k] != held[k]) {
      h->err = "set_ee_ik_map: dof " + std::to_string(held[k]) + " is held (flagged 64) behind a solved joint: the held joints must be a root-side prefix of the link's path";
      return 1;
    }
  if ((int)held.size() > MSSIM_IK_MAX_HELD) { h->err = "set_ee_ik_map: more than " + std::to_string(MSSIM_IK_MAX_HELD) + " held joints on the link's path"; return 1; }
  auto unit7 = [](const float* src, float* dst) {  // the quaternion normalised in double, as the reference does
    const double w = src[3], x = src[4], y = src[5], z = src[6], n = std::sqrt(w * w + x * x + y * y + z * z);
    for (int c = 0; c < 3; c++) dst[c] = src[c];
    dst[3] = (float)(w / n); dst[4] = (float)(x / n); dst[5] = (float)(y / n); dst[6] = (float)(z / n);
  };
  IkChain c{};
  c.link = map->link_index; c.n = (int)solved.size(); c.rows = map->rows; c.col0 = map->column0; c.mode = map->mode; c.flags = map->flags;
  c.lo = map->low; c.hi = map->high; c.rot_scale = map->rot_scale;
  c.max_iters = map->max_iters; c.damping = map->damping; c.max_step = map->max_step; c.tol = map->tolerance;
  for (int k = 0; k < c.n; k++) {
    const int j = solved[k];
    c.dof[k] = j; c.revolute[k] = type[j] == MSSIM_JOINT_REVOLUTE;
    unit7(&frame[7 * (size_t)j], c.frame[k]);
    for (int a = 0; a < 3; a++) c.axis[k][a] = axis[3 * (size_t)j + a];
    c.lower[k] = limit[2 * (size_t)j]; c.upper[k] = limit[2 * (size_t)j + 1];
  }
  unit7(&link_frame[7 * (size_t)map->link_index], c.tip);
  c.n_held = (int)held.size();
  for (int k = 0; k < c.n_held; k++) {
    const int j = held[k];
    c.held_dof[k] = j;
    if (type[j] == MSSIM_JOINT_REVOLUTE) c.held_revolute |= 1u << k;
    unit7(&frame[7 * (size_t)j], c.held_frame[k]);
    for (int a = 0; a < 3; a++) c.held_axis[k][a] = axis[3 * (size_t)j + a];
  }
  h->ik = c;
  h->ik_target_pose = target_pose;
  h->ee.link = -1;  // the two end-effector blocks exclude each other
  return 0;
}

int mssim_ee_ik_solve(mssim_handle h, const float* target_pose, const float* q0, float* q_out, int32_t* iters_out, void* stream) {
  settle(h, (hipStream_t)stream);
  if (h->ik.link < 0) { h->err = "ee_ik_solve: set_ee_ik_map has not been called"; return 1; }
  if (!target_pose || !q_out) { h->err = "ee_ik_solve: no target_pose / q_out"; return 1; }
  const IkIo io{nullptr, 0, nullptr, const_cast<float*>(target_pose), q0, q_out, iters_out};  // (read only in this form)
  launch_ee_ik(h, io, (hipStream_t)stream);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int mssim_apply_action(mssim_handle h, const float* action, int32_t action_dim, void* stream) {
  settle(h, (hipStream_t)stream);
  if (int rc = check_action_dim(h, action_dim)) return rc;
  launch_apply_action(h, action, action_dim, (hipStream_t)stream);
  HIPCHK(h, hipGetLastError());
  return 0;
}

// candidate finger <-> object pairs (a handful of the ~100 pairs of the scene) for the task epilogues:
// entry = pair | finger (bit 30: 0 left, 1 right) | object is shape A (bit 31); cached per (object, fingers)
static int finger_pair_list(mssim_handle h, int obj_row, int f1_row, int f2_row) {
  if (h->finger_pair_rows[0] == obj_row && h->finger_pair_rows[1] == f1_row && h->finger_pair_rows[2] == f2_row && h->d_finger_pairs) return 0;
  std::vector<int32_t> lst;
  for (int p = 0; p < h->M.n_pair; p++) {
    const int ra = h->h_shape_row[h->h_pair_shape[2 * p]], rb = h->h_shape_row[h->h_pair_shape[2 * p + 1]];
    const bool a_obj = ra == obj_row, b_obj = rb == obj_row;
    if (!(a_obj || b_obj)) continue;
    const int other = a_obj ? rb : ra;
    if (other != f1_row && other != f2_row) continue;
    lst.push_back((int32_t)((unsigned)p | (other == f2_row ? 1u << 30 : 0u) | (a_obj ? 1u << 31 : 0u)));
  }
  HIPCHK(h, hipSetDevice(h->device));
  if (!h->d_finger_pairs) { HIPCHK(h, hipMalloc((void**)&h->d_finger_pairs, sizeof(int32_t) * (h->M.n_pair > 0 ? h->M.n_pair : 1))); h->allocs.push_back(h->d_finger_pairs); }
  if (!lst.empty()) HIPCHK(h, hipMemcpy(h->d_finger_pairs, lst.data(), sizeof(int32_t) * lst.size(), hipMemcpyHostToDevice));
  h->n_finger_pairs = (int)lst.size();
  h->finger_pair_rows[0] = obj_row; h->finger_pair_rows[1] = f1_row; h->finger_pair_rows[2] = f2_row;
  return 0;
}

// A task epilogue, the one sequence behind the thirteen mssim_task_*_outputs. Refusals come first and leave what is owed owed.
// An owed step_action + an owed fetch + the epilogue = ONE launch of the control-step kernel, where mssim_create found an
// instance with the task's tail for the model (h->tail_fn). Otherwise what is owed is performed and the epilogue is a launch
// of its own: `standalone(std::true_type, what, st)` launches k_task_*<true>, which first performs the owed copy-out `what`,
// `standalone(std::false_type, 0, st)` launches k_task_*<false>.
struct TaskCall {
  int id; const char* name;  // mssim_dispatch::Task and its name in the messages
  const char* refused;       // the task's own check failed: its message (rc 3); else null
  const int* pair_rows;      // (object, finger 1, finger 2) rows of the contact pairs the task reads, or null
  float *obs, *reward; uint8_t* flags;
  float* extra;              // DevState::tail_head, or null
};
extern "C++" {
using TailTask = decltype(DevState::tail_task);
// the refusals of a task call; rows: the body rows the task reads
template <size_t NROWS>
static int task_refusals(mssim_handle h, const TaskCall& c, const int (&rows)[NROWS]) {
  const int R = h->M.n_link + h->M.n_free + h->M.n_kin;
  for (int r : rows)
    if (r < 0 || r >= R) { h->err = std::string("task_") + c.name + "_outputs: body row out of range"; return 1; }
  if (!h->buf.rigid_body_data || !h->buf.art_qpos || !h->buf.art_qvel) { h->err = "buffers not bound"; return 2; }
  if (c.refused) { h->err = c.refused; return 3; }
  if (c.pair_rows)
    if (int rc = finger_pair_list(h, c.pair_rows[0], c.pair_rows[1], c.pair_rows[2])) return rc;
  return 0;
}
// The tail-less path, for a task without a member in the tail_task union (RollBall, PullCube, PokeCube, LiftPegUpright, PlaceSphere,
// PullCubeTool, PlugCharger, DrawTriangle: h->tail_fn[c.id] is null for every model): an owed step_action runs as the plain control step, the epilogue is always a launch of its own.
template <size_t NROWS, class Standalone>
static int task_outputs(mssim_handle h, const TaskCall& c, const int (&rows)[NROWS], hipStream_t st, Standalone standalone) {
  if (int rc = task_refusals(h, c, rows)) return rc;
  settle(h, st, /*keep_fetch=*/true);
  if (const unsigned what = std::exchange(h->owed.fetch, 0u)) standalone(std::true_type{}, what, st);
  else standalone(std::false_type{}, 0u, st);
  HIPCHK(h, hipGetLastError());
  return 0;
}
// slot: the task's member of the tail_task union
template <class Task, size_t NROWS, class Standalone>
static int task_outputs(mssim_handle h, const TaskCall& c, Task TailTask::*slot, const Task* task, const int (&rows)[NROWS], hipStream_t st, Standalone standalone) {
  if (int rc = task_refusals(h, c, rows)) return rc;
  const Owed& o = h->owed;
  if (h->tail_fn[c.id] && o.action && o.fetch && o.nsub > 0 && st == o.stream && h->ee.link < 0 && h->ik.link < 0 && h->task_robot.n_ranges == 0) {
    DevState S = state_with_action(h, o.action, o.adim);
    S.tail_task.*slot = *task;
    S.tail_pairs = c.pair_rows ? h->d_finger_pairs : nullptr; S.tail_npairs = c.pair_rows ? h->n_finger_pairs : 0;
    S.tail_obs = c.obs; S.tail_reward = c.reward; S.tail_flags = c.flags; S.tail_head = c.extra;
    S.tail_fetch = std::exchange(h->owed.fetch, 0u);
    S.tail_buf = h->buf;
    h->owed.action = nullptr;
    fk_if_dirty(h, st);
    launch_control_step(h, h->tail_fn[c.id], S, o.nsub, st);
    h->n_tail_steps++;
  } else {
    settle(h, st, /*keep_fetch=*/true);
    if (const unsigned what = std::exchange(h->owed.fetch, 0u)) standalone(std::true_type{}, what, st);
    else standalone(std::false_type{}, 0u, st);
  }
  HIPCHK(h, hipGetLastError());
  return 0;
}
}  // extern "C++"

int mssim_task_pick_outputs(mssim_handle h, const mssim_pick_task* task, float* obs, float* reward, uint8_t* flags, void* stream) {
  const int rows[] = {task->tcp_row, task->obj_row, task->goal_row, task->finger1_row, task->finger2_row};
  const int pair_rows[] = {task->obj_row, task->finger1_row, task->finger2_row};
  const TaskCall call{mssim_dispatch::kPick, "pick", /*refused=*/nullptr, pair_rows, obs, reward, flags, /*extra=*/nullptr};
  return task_outputs(h, call, &TailTask::pick, task, rows, (hipStream_t)stream, [&](auto fetch, unsigned what, hipStream_t st) {
    const auto k = h->task_robot.n_ranges > 0 ? k_task_pick<decltype(fetch)::value, true> : k_task_pick<decltype(fetch)::value, false>;
    hipLaunchKernelGGL(k, env_grid(h->N, 64), dim3(fetch ? 256 : 64), 0, st,
                       h->M, h->S, h->buf, what, *task, h->d_finger_pairs, h->n_finger_pairs, obs, reward, flags, h->task_robot);
  });
}

int mssim_task_push_outputs(mssim_handle h, const mssim_push_task* task, float* obs, float* reward, uint8_t* flags, void* stream) {
  const int rows[] = {task->tcp_row, task->obj_row, task->goal_row};
  const TaskCall call{mssim_dispatch::kPush, "push", /*refused=*/nullptr, /*pair_rows=*/nullptr, obs, reward, flags, /*extra=*/nullptr};
  return task_outputs(h, call, &TailTask::push, task, rows, (hipStream_t)stream, [&](auto fetch, unsigned what, hipStream_t st) {
    // (no copy-out: an env per lane, 256 envs per block)
    hipLaunchKernelGGL(k_task_push<decltype(fetch)::value>, env_grid(h->N, fetch ? 64 : 256), dim3(256), 0, st,
                       h->M, h->S, h->buf, what, *task, obs, reward, flags);
  });
}

int mssim_task_peg_outputs(mssim_handle h, const mssim_peg_task* task, float* obs, float* reward, uint8_t* flags, float* head_at_hole, void* stream) {
  const int rows[] = {task->tcp_row, task->peg_row, task->box_row, task->finger1_row, task->finger2_row};
  const int pair_rows[] = {task->peg_row, task->finger1_row, task->finger2_row};
  const bool ok = task->peg_half_sizes && task->box_hole_offsets && task->box_hole_radii && head_at_hole;
  const TaskCall call{mssim_dispatch::kPeg, "peg", ok ? nullptr : "task_peg_outputs: missing per-env geometry / output", pair_rows,
                      obs, reward, flags, head_at_hole};
  return task_outputs(h, call, &TailTask::peg, task, rows, (hipStream_t)stream, [&](auto fetch, unsigned what, hipStream_t st) {
    hipLaunchKernelGGL(k_task_peg<decltype(fetch)::value>, env_grid(h->N, 64), dim3(fetch ? 256 : 64), 0, st,
                       h->M, h->S, h->buf, what, *task, h->d_finger_pairs, h->n_finger_pairs, obs, reward, flags, head_at_hole);
  });
}

int mssim_task_stack_outputs(mssim_handle h, const mssim_stack_task* task, float* obs, float* reward, uint8_t* flags, void* stream) {
  const int rows[] = {task->tcp_row, task->cubeA_row, task->cubeB_row, task->finger1_row, task->finger2_row};
  const int pair_rows[] = {task->cubeA_row, task->finger1_row, task->finger2_row};
  const bool ok = h->M.n_dof >= 2 && task->gripper_width > 0.f;
  const TaskCall call{mssim_dispatch::kStack, "stack", ok ? nullptr : "task_stack_outputs: needs two finger joints and a gripper width > 0", pair_rows,
                      obs, reward, flags, /*extra=*/nullptr};
  return task_outputs(h, call, &TailTask::stack, task, rows, (hipStream_t)stream, [&](auto fetch, unsigned what, hipStream_t st) {
    hipLaunchKernelGGL(k_task_stack<decltype(fetch)::value>, env_grid(h->N, 64), dim3(fetch ? 256 : 64), 0, st,
                       h->M, h->S, h->buf, what, *task, h->d_finger_pairs, h->n_finger_pairs, obs, reward, flags);
  });
}

int mssim_task_pusht_outputs(mssim_handle h, const mssim_pusht_task* task, float* obs, float* reward, uint8_t* flags, float* intersection, void* stream) {
  const int rows[] = {task->tcp_row, task->tee_row, task->goal_row};
  const bool ok = task->consts && task->reward_div > 0.f;
  const TaskCall call{mssim_dispatch::kPushT, "pusht", ok ? nullptr : "task_pusht_outputs: needs the constants block and a reward divisor > 0", /*pair_rows=*/nullptr,
                      obs, reward, flags, intersection};
  return task_outputs(h, call, &TailTask::pusht, task, rows, (hipStream_t)stream, [&](auto fetch, unsigned what, hipStream_t st) {
    // 16 lanes per env: 16 envs per block of 256
    hipLaunchKernelGGL(k_task_pusht<decltype(fetch)::value>, env_grid(h->N, 16), dim3(256), 0, st,
                       h->M, h->S, h->buf, what, *task, obs, reward, flags, intersection);
  });
}

int mssim_task_roll_outputs(mssim_handle h, const mssim_roll_task* task, float* obs, float* reward, uint8_t* flags, void* stream) {
  const int rows[] = {task->tcp_row, task->ball_row, task->goal_row};
  const TaskCall call{mssim_dispatch::kRoll, "roll", task->reached ? nullptr : "task_roll_outputs: needs the reached latch (device [N] f32)", /*pair_rows=*/nullptr,
                      obs, reward, flags, /*extra=*/nullptr};
  return task_outputs(h, call, rows, (hipStream_t)stream, [&](auto fetch, unsigned what, hipStream_t st) {
    // an env per lane as k_task_push: 256 envs per block, 64 behind the copy-out
    hipLaunchKernelGGL(k_task_roll<decltype(fetch)::value>, env_grid(h->N, fetch ? 64 : 256), dim3(256), 0, st,
                       h->M, h->S, h->buf, what, *task, obs, reward, flags);
  });
}

int mssim_task_pull_outputs(mssim_handle h, const mssim_pull_task* task, float* obs, float* reward, uint8_t* flags, void* stream) {
  const int rows[] = {task->tcp_row, task->obj_row, task->goal_row};
  const TaskCall call{mssim_dispatch::kPull, "pull", /*refused=*/nullptr, /*pair_rows=*/nullptr, obs, reward, flags, /*extra=*/nullptr};
  return task_outputs(h, call, rows, (hipStream_t)stream, [&](auto fetch, unsigned what, hipStream_t st) {
    hipLaunchKernelGGL(k_task_pull<decltype(fetch)::value>, env_grid(h->N, fetch ? 64 : 256), dim3(256), 0, st,
                       h->M, h->S, h->buf, what, *task, obs, reward, flags);
  });
}

int mssim_task_poke_outputs(mssim_handle h, const mssim_poke_task* task, float* obs, float* reward, uint8_t* flags, float* metrics, void* stream) {
  const int rows[] = {task->tcp_row, task->peg_row, task->cube_row, task->goal_row, task->finger1_row, task->finger2_row};
  const int pair_rows[] = {task->peg_row, task->finger1_row, task->finger2_row};
  const TaskCall call{mssim_dispatch::kPoke, "poke", metrics ? nullptr : "task_poke_outputs: needs the metrics output (device [N][2] f32)", pair_rows,
                      obs, reward, flags, metrics};
  return task_outputs(h, call, rows, (hipStream_t)stream, [&](auto fetch, unsigned what, hipStream_t st) {
    // launch shapes as mssim_task_pick_outputs
    const auto k = h->task_robot.n_ranges > 0 ? k_task_poke<decltype(fetch)::value, true> : k_task_poke<decltype(fetch)::value, false>;
    hipLaunchKernelGGL(k, env_grid(h->N, 64), dim3(fetch ? 256 : 64), 0, st,
                       h->M, h->S, h->buf, what, *task, h->d_finger_pairs, h->n_finger_pairs, obs, reward, flags, metrics, h->task_robot);
  });
}

int mssim_task_liftpeg_outputs(mssim_handle h, const mssim_liftpeg_task* task, float* obs, float* reward, uint8_t* flags, void* stream) {
  const int rows[] = {task->tcp_row, task->peg_row, task->finger1_row, task->finger2_row};
  const int pair_rows[] = {task->peg_row, task->finger1_row, task->finger2_row};
  const TaskCall call{mssim_dispatch::kLiftPeg, "liftpeg", /*refused=*/nullptr, pair_rows, obs, reward, flags, /*extra=*/nullptr};
  return task_outputs(h, call, rows, (hipStream_t)stream, [&](auto fetch, unsigned what, hipStream_t st) {
    hipLaunchKernelGGL(k_task_liftpeg<decltype(fetch)::value>, env_grid(h->N, 64), dim3(fetch ? 256 : 64), 0, st,
                       h->M, h->S, h->buf, what, *task, h->d_finger_pairs, h->n_finger_pairs, obs, reward, flags);
  });
}

int mssim_task_place_outputs(mssim_handle h, const mssim_place_task* task, float* obs, float* reward, uint8_t* flags, void* stream) {
  const int rows[] = {task->tcp_row, task->obj_row, task->bin_row, task->finger1_row, task->finger2_row};
  const int pair_rows[] = {task->obj_row, task->finger1_row, task->finger2_row};
  const bool ok = h->M.n_dof >= 2 && task->gripper_width > 0.f;
  const TaskCall call{mssim_dispatch::kPlace, "place", ok ? nullptr : "task_place_outputs: needs two finger joints and a gripper width > 0", pair_rows,
                      obs, reward, flags, /*extra=*/nullptr};
  return task_outputs(h, call, rows, (hipStream_t)stream, [&](auto fetch, unsigned what, hipStream_t st) {
    // launch shapes as mssim_task_pick_outputs
    const auto k = h->task_robot.n_ranges > 0 ? k_task_place<decltype(fetch)::value, true> : k_task_place<decltype(fetch)::value, false>;
    hipLaunchKernelGGL(k, env_grid(h->N, 64), dim3(fetch ? 256 : 64), 0, st,
                       h->M, h->S, h->buf, what, *task, h->d_finger_pairs, h->n_finger_pairs, obs, reward, flags, h->task_robot);
  });
}

int mssim_task_pulltool_outputs(mssim_handle h, const mssim_pulltool_task* task, float* obs, float* reward, uint8_t* flags, float* metrics, void* stream) {
  const int rows[] = {task->tcp_row, task->cube_row, task->tool_row, task->base_row, task->finger1_row, task->finger2_row};
  const int pair_rows[] = {task->tool_row, task->finger1_row, task->finger2_row};  // (both boxes of the tool: one body row)
  const TaskCall call{mssim_dispatch::kPullTool, "pulltool", metrics ? nullptr : "task_pulltool_outputs: needs the metrics output (device [N][3] f32)", pair_rows,
                      obs, reward, flags, metrics};
  return task_outputs(h, call, rows, (hipStream_t)stream, [&](auto fetch, unsigned what, hipStream_t st) {
    hipLaunchKernelGGL(k_task_pulltool<decltype(fetch)::value>, env_grid(h->N, 64), dim3(fetch ? 256 : 64), 0, st,
                       h->M, h->S, h->buf, what, *task, h->d_finger_pairs, h->n_finger_pairs, obs, reward, flags, metrics);
  });
}

int mssim_task_plug_outputs(mssim_handle h, const mssim_plug_task* task, float* obs, float* reward, uint8_t* flags, float* metrics, void* stream) {
  const int rows[] = {task->tcp_row, task->charger_row, task->receptacle_row};
  const bool ok = task->goal_pose && metrics;
  const TaskCall call{mssim_dispatch::kPlug, "plug", ok ? nullptr : "task_plug_outputs: needs the goal poses (device [N][7] f32) and the metrics output (device [N][2] f32)",
                      /*pair_rows=*/nullptr, obs, reward, flags, metrics};
  return task_outputs(h, call, rows, (hipStream_t)stream, [&](auto fetch, unsigned what, hipStream_t st) {
    // launch shapes as mssim_task_place_outputs
    hipLaunchKernelGGL(k_task_plug<decltype(fetch)::value>, env_grid(h->N, 64), dim3(fetch ? 256 : 64), 0, st,
                       h->M, h->S, h->buf, what, *task, obs, reward, flags, metrics);
  });
}

int mssim_task_draw_outputs(mssim_handle h, const mssim_draw_task* task, float* obs, float* reward, uint8_t* flags, void* stream) {
  const int rows[] = {task->tcp_row, task->goal_row};
  const bool ok = task->vertices && task->triangles && task->dots && task->dot_near && task->ref_hit && task->draw_step && task->max_dots > 0 &&
                  task->max_dots % 4 == 0 && task->n_ref > 0 && ((uintptr_t)task->dot_near & 3u) == 0;
  const TaskCall call{mssim_dispatch::kDraw, "draw", ok ? nullptr : "task_draw_outputs: needs the vertices, the reference points and the four dot tables (device), max_dots a "
                      "positive multiple of 4, n_ref > 0 and dot_near 4-byte aligned", /*pair_rows=*/nullptr, obs, reward, flags, /*extra=*/nullptr};
  return task_outputs(h, call, rows, (hipStream_t)stream, [&](auto fetch, unsigned what, hipStream_t st) {
    // 64 envs a block in both forms: four waves of 16 lanes per env
    hipLaunchKernelGGL(k_task_draw<decltype(fetch)::value>, env_grid(h->N, 64), dim3(256), 0, st,
                       h->M, h->S, h->buf, what, *task, obs, reward, flags);
  });
}

int64_t mssim_tail_step_count(mssim_handle h) { return h ? h->n_tail_steps : -1; }

int mssim_set_task_robot(mssim_handle h, const mssim_task_robot* robot) {
  if (!h) return 1;
  if (!robot || robot->n_ranges == 0) { h->task_robot = mssim_task_robot{}; return 0; }
  const int n = h->M.n_dof;
  bool ok = robot->n_ranges >= 1 && robot->n_ranges <= 2 && robot->pick_norm_dofs >= 0 && robot->pick_norm_dofs <= n;
  for (int r = 0; ok && r < robot->n_ranges; r++)
    ok = robot->first[r] >= 0 && robot->count[r] >= 0 && robot->first[r] <= n && robot->count[r] <= n - robot->first[r] && robot->thresh[r] == robot->thresh[r];
  if (!ok) { h->err = "set_task_robot: up to two joint ranges within [0, n_dof) with a threshold each, and a norm over at most n_dof joints"; return 3; }
  h->task_robot = *robot;
  return 0;
}

static int make_query(mssim_handle h, const int32_t* data, int count_ints, int nq, int kind, int32_t* qid) {
  HIPCHK(h, hipSetDevice(h->device));
  int* d = nullptr;
  HIPCHK(h, hipMalloc((void**)&d, sizeof(int) * (count_ints > 0 ? count_ints : 1)));
  h->allocs.push_back(d);
  if (count_ints > 0) HIPCHK(h, hipMemcpy(d, data, sizeof(int) * count_ints, hipMemcpyHostToDevice));
  h->queries.push_back(d);
  h->query_n.push_back(nq);
  h->query_kind.push_back(kind);
  *qid = (int)h->queries.size() - 1;
  return 0;
}

int mssim_create_pair_query(mssim_handle h, const int32_t* body_pairs, int32_t n_pairs, int32_t* qid) {
  return make_query(h, body_pairs, 2 * n_pairs, n_pairs, 0, qid);
}
int mssim_create_body_query(mssim_handle h, const int32_t* rows, int32_t n, int32_t* qid) { return make_query(h, rows, n, n, 1, qid); }

static int run_query(mssim_handle h, int32_t qid, int kind, float* out, void* stream) {
  settle(h, (hipStream_t)stream);
  if (qid < 0 || qid >= (int)h->queries.size() || h->query_kind[qid] != kind) { h->err = "bad query id"; return 1; }
  int nq = h->query_n[qid];
  if (nq == 0) return 0;
  hipLaunchKernelGGL(k_query, dim3((h->N + 255) / 256, nq), dim3(256), 0, (hipStream_t)stream, h->M, h->S, h->queries[qid], nq, kind, out);
  HIPCHK(h, hipGetLastError());
  return 0;
}
int mssim_query_pair_impulses(mssim_handle h, int32_t qid, float* out, void* stream) { return run_query(h, qid, 0, out, stream); }
int mssim_query_body_impulses(mssim_handle h, int32_t qid, float* out, void* stream) { return run_query(h, qid, 1, out, stream); }

int mssim_read_internal(mssim_handle h, const char* name, float* out, int32_t max_items, void* stream) {
  settle(h, (hipStream_t)stream);
  std::string s(name);
  const size_t N = (size_t)h->N;
  const float* src = nullptr;
  int items = 0;
  hipStream_t st = (hipStream_t)stream;
  if (s == "q") { src = h->S.q; items = h->M.n_dof; }
  else if (s == "qd") { src = h->S.qd; items = h->M.n_dof; }
  else if (s == "free") { src = h->S.free_s; items = 13 * h->M.n_free; }
  else if (s == "kin") { src = h->S.kin; items = 7 * h->M.n_kin; }
  else if (s == "free_wake") { src = h->S.free_wake; items = h->M.n_free; }
  else if (s == "root") { src = h->S.root; items = 7; }
  else if (s == "bodypose") { src = h->S.bodypose; items = 7 * h->M.n_dof; }
  else if (s == "pair_impulse") { src = h->S.pair_imp; items = 3 * h->M.n_pair; }
  else if (s == "contact_count" || s == "overflow") {
    const int* isrc = s == "overflow" ? h->S.overflow : h->S.pair_cnt;
    items = s == "overflow" ? 1 : h->M.n_pair;
    int take = items < max_items ? items : max_items;
    size_t cnt = (size_t)take * N;
    if (cnt > 0) hipLaunchKernelGGL(k_i2f, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, isrc, out, cnt);
    HIPCHK(h, hipGetLastError());
    return items;
  } else {
    h->err = "unknown internal array: " + s;
    return -1;
  }
  int take = items < max_items ? items : max_items;
  if (take > 0) HIPCHK(h, hipMemcpyAsync(out, src, sizeof(float) * (size_t)take * N, hipMemcpyDeviceToDevice, st));
  return items;
}

int mssim_overflow_count(mssim_handle h, void* stream) {
  settle(h, (hipStream_t)stream);
  std::vector<int> host(h->N);
  hipStream_t st = (hipStream_t)stream;
  if (hipStreamSynchronize(st) != hipSuccess) return -1;
  if (hipMemcpy(host.data(), h->S.overflow, sizeof(int) * h->N, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  (void)hipMemset(h->S.overflow, 0, sizeof(int) * h->N);
  int c = 0;
  for (int v : host) c += v != 0;
  return c;
}

}  // extern "C"

#include "mssim_raycast_desc.h"  // what mssim_raycast_create accepts (host only)
#include "mssim_raycast.h"       // the ray caster of the camera observations: k_raycast and the mssim_raycast_* entry points
#include "mssim_raycast_shade.h" // its flat-shaded view for render(): k_raycast_shade, mssim_raycast_set_colours / _shade
#include "mssim_raycast_dots.h"  // a dot layer composited over that view: k_raycast_dots, mssim_raycast_draw_dots
#include "mssim_test_collide.h"  // test hook, not part of the ABI: the manifold routines of k_solve16 on explicit shape pairs

#ifdef MSSIM_PHASE_CLOCKS
// debug builds only (not part of include/mssim.h): cycles per phase of k_solve16 summed over blocks
extern "C" int mssim_debug_phase_clocks(unsigned long long* out32, int reset) {
  if (hipMemcpyFromSymbol(out32, HIP_SYMBOL(g_phase_clk), 32 * sizeof(unsigned long long)) != hipSuccess) return -1;
  if (reset < 0) return 0;
  if (reset) {
    unsigned long long z[32] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_phase_clk), z, sizeof(z)) != hipSuccess) return -1;
  }
  return 0;
}
extern "C" int mssim_debug_mpr_hist(unsigned* out32) {
  return hipMemcpyFromSymbol(out32, HIP_SYMBOL(g_mpr_hist), 32 * sizeof(unsigned)) == hipSuccess ? 0 : -1;
}
extern "C" int mssim_debug_mpr_clocks(unsigned long long* out8, int reset) {
  if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_mpr_clk), 8 * sizeof(unsigned long long)) != hipSuccess) return -1;
  if (reset) {
    unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_mpr_clk), z, sizeof(z)) != hipSuccess) return -1;
  }
  return 0;
}
extern "C" int mssim_debug_phase_blocks(unsigned* out, int nblocks) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_phase_blk), (size_t)nblocks * 32 * sizeof(unsigned)) == hipSuccess ? 0 : -1;
}
#elif defined(MSSIM_BLOCK_TIMES)
extern "C" int mssim_debug_phase_blocks(unsigned* out, int nblocks) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_phase_blk), (size_t)nblocks * 32 * sizeof(unsigned)) == hipSuccess ? 0 : -1;
}
#endif
