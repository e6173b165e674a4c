// mssim_ik.h -- iterative inverse kinematics of one articulation link, one env per lane (include/mssim_hip_tasks.h
// `set_ee_ik_map`, `ee_ik_solve`): the end-effector modes that track a target pose (pd_ee_target_delta_pos,
// pd_ee_target_delta_pose, pd_ee_pose). Included by mssim_kernels.hip after DevState / SOA / xcd_chunk.
//
// Per env, what agents/controllers/utils/kinematics.py `compute_ik` does in its iterative branch for that env alone:
//
//   q = q0[solved]; (p0, r0) = the held joints of the path composed at q0[held] (identity without one)
//   repeat at most max_iters:
//     (pe, qe, J) = FK + geometric Jacobian of the link over the solved dofs on its path, in the ROOT frame, from
//                   (p0, r0) and the chain's constant tables (never the root pose or the simulation's body poses)
//     err = tp - pe ; rows == 6: append the rotation vector of tq * conj(qe) (w >= 0, angle = 2 atan2(|v|, w))
//     if max|err| < tolerance: stop                       <- this env only
//     step = J^T (J J^T + damping I)^-1 err               (rows x rows SPD: Cholesky without pivoting)
//     step *= max_step / max(max|step|, max_step)
//     q = min(max(q + step, lower), upper)                (a NaN stays a NaN, as torch.maximum / torch.minimum keep it)
//
// THE EXIT IS PER ENV. The torch branch leaves its loop when the slowest env of the whole batch has converged and
// keeps iterating the converged ones meanwhile, so there an env's answer depends on which envs share its batch. Here
// an env stops at its own convergence: its answer is a function of its own inputs alone (the first envs of a large
// batch are bit-identical to a small batch), and a torch call with a batch of one is the same algorithm.
//
// HELD JOINTS. A path joint flagged 64 in the joint map (include/mssim.h) belongs to another controller: it takes part
// in the forward kinematics where it is, has no Jacobian column and gets no target. The held joints form a root-side
// prefix of the path (the Fetch: base x, y, yaw and the torso before the seven arm joints), so each lane composes them
// once, before the loop, into one transform (p0, r0) from which the solved chain starts; the loop itself is the one of a
// chain without held joints. k_ee_ik<ROWS, false> is that chain's kernel, instruction for instruction what it was
// before held joints existed; k_ee_ik<ROWS, true> starts from (p0, r0). A NaN held position makes (p0, r0) NaN, hence
// every solved joint of that env, as a NaN target does.
//
// Layout: 64-thread blocks, one env per lane; a wave ends with its slowest lane. The chain's constants (at most
// MSSIM_IK_MAX_JOINTS joints) come by value in the kernel arguments: wave-uniform, read with scalar loads. Every loop
// over joints and rows is unrolled to its compile-time maximum under a uniform `k < n` guard, so q, the Jacobian and
// the Cholesky factor stay in registers. sincosf / atan2f / sqrtf are the precise library versions.
#pragma once

#define MSSIM_IK_MAX_JOINTS 8  // solved
#define MSSIM_IK_MAX_HELD 15   // held: an articulation has at most 16 dofs and one of them is solved

struct IkChain {
  int link;   // < 0: no block
  int n;      // solved joints on the link's path, root side first
  int rows;   // 3: position, 6: position + orientation
  int col0, mode, flags;
  float lo, hi, rot_scale;
  int max_iters;
  float damping, max_step, tol;
  int dof[MSSIM_IK_MAX_JOINTS];
  int revolute[MSSIM_IK_MAX_JOINTS];
  float frame[MSSIM_IK_MAX_JOINTS][7];  // parent body -> joint frame, unit quaternion
  float axis[MSSIM_IK_MAX_JOINTS][3];
  float lower[MSSIM_IK_MAX_JOINTS], upper[MSSIM_IK_MAX_JOINTS];
  float tip[7];                          // last body -> link frame, unit quaternion
  int n_held;                            // held joints: the path's root-side prefix, before dof[0]
  int held_dof[MSSIM_IK_MAX_HELD];
  unsigned held_revolute;                // bit k: held joint k is revolute
  float held_frame[MSSIM_IK_MAX_HELD][7];
  float held_axis[MSSIM_IK_MAX_HELD][3];
};

// v rotated by the unit quaternion q: v + w t + u x t, t = 2 u x v
MS_DEV f3 ik_qrot(q4 q, f3 v) {
  const f3 u = f3{q.x, q.y, q.z};
  const f3 t = cross(u, v) * 2.f;
  return v + t * q.w + cross(u, t);
}

// the loop above on q[0 .. C.n), the chain starting at (p0, r0) (HELD; else at the root); returns the number of steps taken
template <int ROWS, bool HELD>
MS_DEV int ik_solve(const IkChain& C, f3 tp, q4 tq, float (&q)[MSSIM_IK_MAX_JOINTS], f3 p0, q4 r0) {
  constexpr int MJ = MSSIM_IK_MAX_JOINTS;
  int it = 0;
  for (;;) {
    // ---- FK down the chain: world axis and anchor of every joint
    f3 p = HELD ? p0 : f3{0.f, 0.f, 0.f};
    q4 r = HELD ? r0 : q4{1.f, 0.f, 0.f, 0.f};
    f3 ax[MJ], an[MJ];
#pragma unroll
    for (int k = 0; k < MJ; k++) {
      if (k < C.n) {
        const f3 jp = p + ik_qrot(r, f3{C.frame[k][0], C.frame[k][1], C.frame[k][2]});
        const q4 jq = qmul(r, q4{C.frame[k][3], C.frame[k][4], C.frame[k][5], C.frame[k][6]});
        const f3 axis = f3{C.axis[k][0], C.axis[k][1], C.axis[k][2]};
        const f3 a = ik_qrot(jq, axis);
        ax[k] = a; an[k] = jp;
        if (C.revolute[k]) {
          float s, c;
          sincosf(0.5f * q[k], &s, &c);
          p = jp; r = qmul(jq, q4{c, s * axis.x, s * axis.y, s * axis.z});
        } else {
          p = jp + a * q[k]; r = jq;
        }
      }
    }
    const f3 pe = p + ik_qrot(r, f3{C.tip[0], C.tip[1], C.tip[2]});
    // ---- error
    float err[ROWS];
    err[0] = tp.x - pe.x; err[1] = tp.y - pe.y; err[2] = tp.z - pe.z;
    if (ROWS == 6) {
      const q4 qe = qmul(r, q4{C.tip[3], C.tip[4], C.tip[5], C.tip[6]});
      q4 d = qmul(tq, q4{qe.w, -qe.x, -qe.y, -qe.z});
      if (d.w < 0.f) d = q4{-d.w, -d.x, -d.y, -d.z};
      const float nv = sqrtf(d.x * d.x + d.y * d.y + d.z * d.z);
      const float ang = 2.f * atan2f(nv, d.w);
      const float den = nv < 1e-9f ? 1e-9f : nv;  // (a NaN stays)
      err[ROWS - 3] = d.x / den * ang; err[ROWS - 2] = d.y / den * ang; err[ROWS - 1] = d.z / den * ang;
    }
    bool done = true;  // max|err| < tol; false for a NaN
#pragma unroll
    for (int i = 0; i < ROWS; i++) done = done && (fabsf(err[i]) < C.tol);
    if (done || it >= C.max_iters) break;
    // ---- Jacobian columns, Gram matrix summed joint by joint
    float J[MJ][ROWS];
    float G[ROWS][ROWS];
#pragma unroll
    for (int i = 0; i < ROWS; i++)
#pragma unroll
      for (int j = 0; j <= i; j++) G[i][j] = i == j ? C.damping : 0.f;
#pragma unroll
    for (int k = 0; k < MJ; k++) {
      if (k < C.n) {
        const f3 v = C.revolute[k] ? cross(ax[k], pe - an[k]) : ax[k];
        J[k][0] = v.x; J[k][1] = v.y; J[k][2] = v.z;
        if (ROWS == 6) {
          J[k][ROWS - 3] = C.revolute[k] ? ax[k].x : 0.f; J[k][ROWS - 2] = C.revolute[k] ? ax[k].y : 0.f; J[k][ROWS - 1] = C.revolute[k] ? ax[k].z : 0.f;
        }
#pragma unroll
        for (int i = 0; i < ROWS; i++)
#pragma unroll
          for (int j = 0; j <= i; j++) G[i][j] += J[k][i] * J[k][j];
      }
    }
    // ---- G y = err: Cholesky without pivoting, two triangular solves
    float L[ROWS][ROWS];
#pragma unroll
    for (int i = 0; i < ROWS; i++)
#pragma unroll
      for (int j = 0; j <= i; j++) {
        float sum = G[i][j];
#pragma unroll
        for (int m = 0; m < j; m++) sum -= L[i][m] * L[j][m];
        L[i][j] = i == j ? sqrtf(fmaxf(sum, 1e-20f)) : sum / L[j][j];
      }
    float z[ROWS], y[ROWS];
#pragma unroll
    for (int i = 0; i < ROWS; i++) {
      float sum = err[i];
#pragma unroll
      for (int m = 0; m < i; m++) sum -= L[i][m] * z[m];
      z[i] = sum / L[i][i];
    }
#pragma unroll
    for (int i = ROWS - 1; i >= 0; i--) {
      float sum = z[i];
#pragma unroll
      for (int m = i + 1; m < ROWS; m++) sum -= L[m][i] * y[m];
      y[i] = sum / L[i][i];
    }
    // ---- step = J^T y, capped, into the limits
    float step[MJ];
    float big = 0.f;  // max|step|; a NaN wins, as torch.amax
#pragma unroll
    for (int k = 0; k < MJ; k++) {
      if (k < C.n) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < ROWS; i++) s += J[k][i] * y[i];
        step[k] = s;
        const float a = fabsf(s);
        big = (a > big || a != a) ? a : big;
      }
    }
    const float scale = C.max_step / (big < C.max_step ? C.max_step : big);
#pragma unroll
    for (int k = 0; k < MJ; k++) {
      if (k < C.n) {
        float t = q[k] + step[k] * scale;
        t = t < C.lower[k] ? C.lower[k] : t;
        t = t > C.upper[k] ? C.upper[k] : t;
        q[k] = t;
      }
    }
    it++;
  }
  return it;
}

// The two forms of one launch. Map form (`action` set; runs right after k_apply_action): the block's columns ->
// target pose (updated in place) -> joint targets of the path dofs flagged 4, in the visible buffer and the simulation
// state, started from the visible qpos. Solve form (`action` null): q_out = q0 with the solved path dofs solved for
// target_pose (held and off-path dofs are q0's bits); q0 null: the visible qpos buffer (else the simulation's own). Both are the same kernel, so the same
// inputs give the same bits in either form.
struct IkIo {
  const float* action; int adim; const int* flags;  // map form
  float* target_pose;                               // [N][7]: map form reads and writes it, solve form reads it
  const float* q0; float* q_out; int* iters_out;    // solve form
};

// (the chain travels by value: the whole argument block stays well under the 4 KB a launch may carry)
static_assert(sizeof(IkChain) + sizeof(DevState) + sizeof(mssim_buffers) + sizeof(IkIo) + 64 <= 3072, "k_ee_ik's kernel arguments");

template <int ROWS, bool HELD>
__global__ __launch_bounds__(64) void k_ee_ik(IkChain C, DevState S, mssim_buffers B, int n_dof, IkIo io) {
  const int N = S.N;
  const int e = xcd_chunk(blockIdx.x, gridDim.x) * 64 + threadIdx.x;
  if (e >= N) return;
  float* t = io.target_pose + (size_t)e * 7;
  f3 tp = f3{t[0], t[1], t[2]};
  q4 tq = q4{t[3], t[4], t[5], t[6]};
  if (io.action) {
    const float* a = io.action + (size_t)e * io.adim + C.col0;
    f3 lin = f3{a[0], a[1], a[2]};
    if (C.flags & 2) {
      const float mid = 0.5f * (C.hi + C.lo), half = 0.5f * (C.hi - C.lo);
      lin = f3{mid + half * clip_unit(lin.x), mid + half * clip_unit(lin.y), mid + half * clip_unit(lin.z)};
    }
    if (C.mode == 1) {
      tp = tp + lin;
    } else {
      tp = lin;
      tq = q4{1.f, 0.f, 0.f, 0.f};
    }
    if (ROWS == 6) {
      f3 rot = f3{a[ROWS - 3], a[ROWS - 2], a[ROWS - 1]};
      if (C.flags & 2) {
        const float nr = sqrtf(dot(rot, rot));
        if (nr > 1.f) rot = rot * (1.f / fmaxf(nr, 1e-12f));
        rot = rot * C.rot_scale;
      }
      // XYZ Euler angles: R = Rx Ry Rz
      float sx, cx, sy, cy, sz, cz;
      sincosf(0.5f * rot.x, &sx, &cx); sincosf(0.5f * rot.y, &sy, &cy); sincosf(0.5f * rot.z, &sz, &cz);
      const q4 qr = qmul(qmul(q4{cx, sx, 0.f, 0.f}, q4{cy, 0.f, sy, 0.f}), q4{cz, 0.f, 0.f, sz});
      tq = C.mode == 1 ? qmul(qr, tq) : qr;
    }
    t[0] = tp.x; t[1] = tp.y; t[2] = tp.z; t[3] = tq.w; t[4] = tq.x; t[5] = tq.y; t[6] = tq.z;
  }
  auto start = [&](int j) { return io.q0 ? io.q0[(size_t)e * n_dof + j] : (B.art_qpos ? B.art_qpos[(size_t)e * n_dof + j] : SOA(S.q, j)); };
  if (io.q_out)
    for (int j = 0; j < n_dof; j++) io.q_out[(size_t)e * n_dof + j] = start(j);
  float q[MSSIM_IK_MAX_JOINTS];
#pragma unroll
  for (int k = 0; k < MSSIM_IK_MAX_JOINTS; k++) q[k] = k < C.n ? start(C.dof[k]) : 0.f;
  // the held prefix at its current positions, composed once: joint frame, then the joint's own motion
  f3 p0 = f3{0.f, 0.f, 0.f};
  q4 r0 = q4{1.f, 0.f, 0.f, 0.f};
  if (HELD) {
    for (int k = 0; k < C.n_held; k++) {
      const float qk = start(C.held_dof[k]);
      const f3 jp = p0 + ik_qrot(r0, f3{C.held_frame[k][0], C.held_frame[k][1], C.held_frame[k][2]});
      const q4 jq = qmul(r0, q4{C.held_frame[k][3], C.held_frame[k][4], C.held_frame[k][5], C.held_frame[k][6]});
      const f3 axis = f3{C.held_axis[k][0], C.held_axis[k][1], C.held_axis[k][2]};
      if ((C.held_revolute >> k) & 1u) {
        float s, c;
        sincosf(0.5f * qk, &s, &c);
        p0 = jp; r0 = qmul(jq, q4{c, s * axis.x, s * axis.y, s * axis.z});
      } else {
        p0 = jp + ik_qrot(jq, axis) * qk; r0 = jq;
      }
    }
  }
  const int it = ik_solve<ROWS, HELD>(C, tp, tq, q, p0, r0);
#pragma unroll
  for (int k = 0; k < MSSIM_IK_MAX_JOINTS; k++)
    if (k < C.n) {
      if (io.q_out) io.q_out[(size_t)e * n_dof + C.dof[k]] = q[k];
      if (io.action && (io.flags[C.dof[k]] & 4)) {
        SOA(S.qt, C.dof[k]) = q[k];
        if (B.art_target_qpos) B.art_target_qpos[(size_t)e * n_dof + C.dof[k]] = q[k];
      }
    }
  if (io.iters_out) io.iters_out[e] = it;
}
