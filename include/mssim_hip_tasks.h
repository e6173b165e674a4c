/* mssim_hip_tasks.h -- extras of the HIP library only (libmssim.so), outside the core ABI of mssim.h: task epilogues,
 * the iterative-IK block of the action map, and the ray caster of the camera observations.
 *
 * mssim.h is the contract both implementations export (the HIP library and the CPU oracle, every MSSIM_FN of it under
 * its own prefix). The entry points below exist in the HIP library alone: plain extern "C" symbols, bound by
 * maniskill_amd/native.py as optional extras. They follow the conventions of the task_*_outputs calls of mssim.h
 * (device pointers, the caller's stream, no host sync; a deferred step_action + fetch makes the whole control step
 * one launch). */
#ifndef MSSIM_HIP_TASKS_H
#define MSSIM_HIP_TASKS_H

#include "mssim.h"

#ifdef __cplusplus
extern "C" {
#endif

/* StackCube-style evaluate + state observation + dense reward in one launch
 * (envs/tasks/tabletop/stack_cube.py, agents/robots/panda/panda.py is_grasping). Reads the user-visible buffers (after
 * fetch) and the last substep's contact impulses.
 * obs [N][2*n_dof+30] f32 (qpos, qvel, tcp_pose7, cubeA_pose7, cubeB_pose7, tcp_to_cubeA3, tcp_to_cubeB3, cubeA_to_cubeB3),
 * reward [N] f32, flags [N][4] u8 = success, is_cubeA_on_cubeB, is_cubeA_static, is_cubeA_grasped.
 * The struct is no larger than mssim_peg_task (the control-step kernel carries every task struct in one union). */
typedef struct mssim_stack_task {
  int32_t tcp_row, cubeA_row, cubeB_row, finger1_row, finger2_row; /* rigid_body_data body rows */
  float cube_half_size;       /* 0.02: A is on B when |dz - 2 half| <= on_z_thresh ...                              */
  float on_xy_thresh;         /* ... and |dxy| <= this (|half_xy| + 0.005, as evaluate() computes it in f32)        */
  float on_z_thresh;          /* 0.005 */
  float gripper_width;        /* upper limit of the last finger joint x 2 (ungrasp reward = finger gap / this)         */
  float static_lin_thresh;    /* 1e-2 m/s   (Actor.is_static of cube A)                                              */
  float static_ang_thresh;    /* 0.5 rad/s                                                                           */
  float min_force;            /* 0.5 N  (is_grasping of cube A)                                                      */
  float max_angle_deg;        /* 85                                                                                  */
  float reward_scale;         /* 1 (dense) or 1/8 (normalized_dense)                                                 */
  int32_t* elapsed_steps;     /* optional, as in mssim_pick_task */
  int32_t* elapsed_out;
  uint8_t* truncated_out;     /* optional device [N]: new elapsed_steps >= time_limit */
  int32_t time_limit;
  uint8_t* terminated_out;    /* optional device [N]: a copy of success */
} mssim_stack_task;

int mssim_task_stack_outputs(mssim_handle h, const mssim_stack_task* task, float* obs, float* reward, uint8_t* flags, void* stream);

/* PushT-style evaluate + state observation + dense reward in one launch (envs/tasks/tabletop/push_t.py): the
 * reference's 64 x 64 pseudo-render of the T block in the goal T's frame, intersected with the goal's template.
 * obs [N][2*n_dof+17] f32 (qpos, qvel, tcp_pose7, goal_pos3, obj_pose7), reward [N] f32, flags [N][1] u8 = success,
 * intersection: optional device [N] f32, the count of template pixels hit (success = count / area >= threshold).
 * `consts` is a device block of MSSIM_PUSHT_CONSTS_WORDS 32-bit words that the env builds once from its own tensors:
 *   [0, 9)     world_to_goal, 3 x 3 f32 row-major (the inverse of the goal's planar transform, as the env computed it)
 *   [9, 73)    u of grid column j (f32), [73, 137) v of grid row i (f32): the uv grid's pixel centres
 *   [137, 265) the template, 64 x 64 bits, bit (64 i + j) = word (64 i + j) / 32, bit (64 i + j) % 32
 *   [265]      the template's pixel count (int32)
 * The struct is no larger than mssim_peg_task (the control-step kernel carries every task struct in one union). */
#define MSSIM_PUSHT_W2G 0
#define MSSIM_PUSHT_U 9
#define MSSIM_PUSHT_V 73
#define MSSIM_PUSHT_TEMPLATE 137
#define MSSIM_PUSHT_AREA 265
#define MSSIM_PUSHT_CONSTS_WORDS 266
typedef struct mssim_pusht_task {
  int32_t tcp_row, tee_row, goal_row; /* rigid_body_data body rows */
  float goal_z_rot;           /* 5 pi / 3: reward term cos(yaw - goal_z_rot), yaw = 2 acos(sign(q_z) q_w)              */
  float intersection_thresh;  /* 0.9 */
  float reward_div;           /* 1 (dense) or 3 (normalized_dense) */
  const int32_t* consts;      /* device block, see above */
  int32_t* elapsed_steps;     /* optional, as in mssim_pick_task */
  int32_t* elapsed_out;
  uint8_t* truncated_out;     /* optional device [N]: new elapsed_steps >= time_limit */
  int32_t time_limit;
  uint8_t* terminated_out;    /* optional device [N]: a copy of success */
} mssim_pusht_task;

int mssim_task_pusht_outputs(mssim_handle h, const mssim_pusht_task* task, float* obs, float* reward, uint8_t* flags, float* intersection, void* stream);

/* RollBall-style evaluate + state observation + dense reward in one launch (envs/tasks/tabletop/roll_ball.py).
 * obs [N][2*n_dof+26] f32 (qpos, qvel, tcp_pose7, goal_pos3, ball_pose7, ball linear velocity 3, ball - tcp, goal - ball),
 * reward [N] f32, flags [N][1] u8 = success (|ball - goal|_xy < goal_radius).
 * The reward carries a per-env latch, `reached` (0 or 1), that lives in the caller's memory from step to step:
 *   u = (ball - goal) / |ball - goal| (3-D), hit = ball + u (ball_radius + hit_offset), d = |hit - tcp|
 *   update_reached != 0 and d < reach_thresh: reached = 1 (written in place)
 *   r = 20 (1 - tanh |ball - goal|_xy) reached + (1 - tanh 2 d) (1 - reached) + reached; success: 30; times reward_scale
 * With update_reached == 0 (the outputs of a reset) the latch is read and never written.
 * This task and the next never run at the control-step kernel's tail: with a step_action + fetch owed, the control step
 * and the copy-out + epilogue are two launches. */
typedef struct mssim_roll_task {
  int32_t tcp_row, ball_row, goal_row; /* rigid_body_data body rows */
  float goal_radius;          /* 0.1   */
  float ball_radius;          /* 0.035 */
  float hit_offset;           /* 0.05: the hit point lies ball_radius + hit_offset behind the ball's centre, seen from the goal */
  float reach_thresh;         /* 0.04  */
  float reward_scale;         /* 1 (dense) or 1/30 (normalized_dense) */
  float* reached;             /* device [N] f32, read and (update_reached != 0) written in place; required */
  int32_t update_reached;
  int32_t* elapsed_steps;     /* optional, as in mssim_pick_task */
  int32_t* elapsed_out;
  uint8_t* truncated_out;     /* optional device [N]: new elapsed_steps >= time_limit */
  int32_t time_limit;
  uint8_t* terminated_out;    /* optional device [N]: a copy of success */
} mssim_roll_task;

int mssim_task_roll_outputs(mssim_handle h, const mssim_roll_task* task, float* obs, float* reward, uint8_t* flags, void* stream);

/* PullCube-style evaluate + state observation + dense reward in one launch (envs/tasks/tabletop/pull_cube.py).
 * obs [N][2*n_dof+17] f32 (qpos, qvel, tcp_pose7, goal_pos3, obj_pose7), reward [N] f32, flags [N][1] u8 = success
 * (|obj - goal|_xy < goal_radius; no height condition).
 *   d = |obj + (cube_half_size + 0.01, 0, 0) - tcp|; r = 1 - tanh 5 d; d < 0.01: + 1 - tanh 5 |obj - goal|_xy; success: 3;
 *   times reward_scale */
typedef struct mssim_pull_task {
  int32_t tcp_row, obj_row, goal_row; /* rigid_body_data body rows */
  float goal_radius;          /* 0.1  */
  float cube_half_size;       /* 0.02 */
  float reward_scale;         /* 1 (dense) or 1/3 (normalized_dense) */
  int32_t* elapsed_steps;     /* optional, as in mssim_pick_task */
  int32_t* elapsed_out;
  uint8_t* truncated_out;
  int32_t time_limit;
  uint8_t* terminated_out;
} mssim_pull_task;

int mssim_task_pull_outputs(mssim_handle h, const mssim_pull_task* task, float* obs, float* reward, uint8_t* flags, void* stream);

/* PokeCube-style evaluate + state observation + dense reward in one launch (envs/tasks/tabletop/poke_cube.py,
 * agents/robots/panda/panda.py is_grasping / is_static). Reads the user-visible buffers (after fetch) and the last substep's
 * finger <-> peg contact impulses. The model has two free bodies (two rows of the control-step kernel per env); like the two
 * tasks above, this one and the next never run at the control-step kernel's tail.
 * obs [N][2*n_dof+36] f32 (qpos, qvel, tcp_pose7, cube_pose7, peg_pose7, "goal_pos" = the PEG's position 3, peg - tcp,
 * cube - peg, goal - cube, peg head - cube, the head being peg + (peg_half_length, 0, 0), unrotated),
 * reward [N] f32, flags [N][4] u8 = success, is_cube_placed, is_peg_cube_fit, is_peg_grasped,
 * metrics [N][2] f32 = angle_diff, head_to_cube_dist; required.
 *   yaw(q) = atan2(-R01, R00) of the rotation matrix of q (entries scaled by 2 / |q|^2): the third XYZ Euler angle
 *   angle_diff = |yaw(peg * head offset) - yaw(cube)| (not wrapped); head_to_cube_dist = |head - cube|_xy
 *   placed = |cube - goal|_xy < goal_radius; fit = angle_diff < align_thresh and head_to_cube_dist <= cube_half_size +
 *   0.005; static = max |qvel[:n_static_dofs]| <= static_thresh; success = placed and static
 *   r = 2 (1 - tanh 5 |tcp - peg|); grasped and |tcp - peg| < reach_thresh: r = 4 + (1 - tanh 5 head_to_cube_dist) +
 *   (1 - tanh 5 angle_diff); and fit: r = 7 + (1 - tanh 5 |goal - cube|); placed: r += 1 - tanh 5 |qvel[:n_static_dofs]|;
 *   success: 10; times reward_scale */
typedef struct mssim_poke_task {
  int32_t tcp_row, peg_row, cube_row, goal_row, finger1_row, finger2_row; /* rigid_body_data body rows */
  int32_t n_static_dofs;      /* leading joints of is_static and of the static reward (all but the two fingers) */
  float peg_half_length;      /* 0.12: the head offset along the peg's x axis                                   */
  float cube_half_size;       /* 0.02: the head is close within this + 0.005 (the sum formed in double, rounded once) */
  float goal_radius;          /* 0.05 */
  float align_thresh;         /* 0.05 rad */
  float reach_thresh;         /* 0.01 */
  float static_thresh;        /* 0.2 rad/s */
  float min_force;            /* 0.5 N  (is_grasping of the peg) */
  float max_angle_deg;        /* 85 */
  float reward_scale;         /* 1 (dense) or 1/10 (normalized_dense) */
  int32_t* elapsed_steps;     /* optional, as in mssim_pick_task */
  int32_t* elapsed_out;
  uint8_t* truncated_out;     /* optional device [N]: new elapsed_steps >= time_limit */
  int32_t time_limit;
  uint8_t* terminated_out;    /* optional device [N]: a copy of success */
} mssim_poke_task;

int mssim_task_poke_outputs(mssim_handle h, const mssim_poke_task* task, float* obs, float* reward, uint8_t* flags, float* metrics, void* stream);

/* LiftPegUpright-style evaluate + state observation + dense reward in one launch
 * (envs/tasks/tabletop/lift_peg_upright.py, Panda.is_grasping).
 * obs [N][2*n_dof+14] f32 (qpos, qvel, tcp_pose7, obj_pose7), reward [N] f32, flags [N][1] u8 = success:
 *   | |yaw(peg)| - pi/2 | < upright_thresh (yaw as above) and |peg_z - peg_half_length| < height_thresh
 *   r = |R20| + (1 - tanh 5 |peg_z - peg_half_length|) + (grasped ? 1 : 1 - tanh 5 |peg - tcp|) / 5; success: 3;
 *   times reward_scale */
typedef struct mssim_liftpeg_task {
  int32_t tcp_row, peg_row, finger1_row, finger2_row; /* rigid_body_data body rows */
  float peg_half_length;      /* 0.12  */
  float upright_thresh;       /* 0.08 rad */
  float height_thresh;        /* 0.005 */
  float min_force;            /* 0.5 N  (is_grasping of the peg) */
  float max_angle_deg;        /* 85 */
  float reward_scale;         /* 1 (dense) or 1/3 (normalized_dense) */
  int32_t* elapsed_steps;     /* optional, as in mssim_pick_task */
  int32_t* elapsed_out;
  uint8_t* truncated_out;
  int32_t time_limit;
  uint8_t* terminated_out;
} mssim_liftpeg_task;

int mssim_task_liftpeg_outputs(mssim_handle h, const mssim_liftpeg_task* task, float* obs, float* reward, uint8_t* flags, void* stream);

/* PlaceSphere-style evaluate + state observation + dense reward in one launch (envs/tasks/tabletop/place_sphere.py,
 * Panda.is_grasping / is_static, Actor.is_static). Reads the user-visible buffers (after fetch) and the last substep's
 * finger <-> sphere contact impulses. Like the four tasks above, this one and the next never run at the control-step
 * kernel's tail.
 * obs [N][2*n_dof+21] f32 (qpos, qvel, is_grasped as 0 / 1, tcp_pose7, bin_pos3, obj_pose7, obj - tcp),
 * reward [N] f32, flags [N][4] u8 = success, is_obj_grasped, is_obj_on_bin, is_obj_static.
 *   off = obj - bin; on_bin = |off|_xy <= on_bin_tol and |off_z - radius - bin_base_half| <= on_bin_tol
 *   static = |v_obj| <= static_lin_thresh and |w_obj| <= static_ang_thresh; success = on_bin and static and not grasped
 *   r = 2 (1 - tanh 5 |tcp - obj|); grasped: r = 4 + (1 - tanh 5 |bin + (bin_base_half + radius) z - obj|);
 *   on_bin: r = 6 + (ungrasp + (1 - tanh(10 |v_obj| + |w_obj|)) + robot_static) / 3 with ungrasp = (sum of the two finger
 *   joints) / gripper_width if grasped, else 16, and robot_static = 1 where max |qvel[:n_static_dofs]| <=
 *   robot_static_thresh, else 0; success: 13; times reward_scale.
 * Refused (rc 3) for a model with fewer than two joints or gripper_width <= 0, as mssim_task_stack_outputs. */
typedef struct mssim_place_task {
  int32_t tcp_row, obj_row, bin_row, finger1_row, finger2_row; /* rigid_body_data body rows */
  int32_t n_static_dofs;      /* leading joints of the robot's is_static (all but the two fingers) */
  float radius;               /* 0.02: the sphere's                                                  */
  float bin_base_half;        /* 0.0025: half the thickness of the bin's bottom block                */
  float on_bin_tol;           /* 0.005: both the xy and the z tolerance of is_obj_on_bin             */
  float static_lin_thresh;    /* 1e-2 m/s  */
  float static_ang_thresh;    /* 0.5 rad/s */
  float robot_static_thresh;  /* 0.2 rad/s */
  float gripper_width;        /* fully open finger gap (2 x the last joint's upper limit) */
  float min_force;            /* 0.5 N  (is_grasping of the sphere) */
  float max_angle_deg;        /* 85 */
  float reward_scale;         /* 1 (dense) or 1/13 (normalized_dense) */
  int32_t* elapsed_steps;     /* optional, as in mssim_pick_task */
  int32_t* elapsed_out;
  uint8_t* truncated_out;     /* optional device [N]: new elapsed_steps >= time_limit */
  int32_t time_limit;
  uint8_t* terminated_out;    /* optional device [N]: a copy of success */
} mssim_place_task;

int mssim_task_place_outputs(mssim_handle h, const mssim_place_task* task, float* obs, float* reward, uint8_t* flags, void* stream);

/* PullCubeTool-style evaluate + state observation + dense reward in one launch (envs/tasks/tabletop/pull_cube_tool.py,
 * Panda.is_grasping). The tool is one body row with two shapes; the model has two free bodies (two rows of the
 * control-step kernel per env).
 * obs [N][2*n_dof+21] f32 (qpos, qvel, tcp_pose7, cube_pose7, tool_pose7), reward [N] f32, flags [N][1] u8 = success,
 * metrics [N][3] f32 = cube_to_workspace_dist, 1 - tanh(3 cube_to_workspace_dist), dense reward / 5; required.
 *   success = |cube - base|_xy < pulled_close_dist; cube_to_workspace_dist = |cube - (base + (0.1 arm_reach, 0, 0))|
 *   d_t = |tcp - (tool + (0.02, 0, 0))|, g = 1 where the tool is grasped, else 0
 *   d_p = |tool - (cube + (-(hook_length + cube_half_size), -0.067, 0))|, positioned = d_p < 0.05
 *   target = base + (0.05, 0, 0), d_c = |cube - target|, d_0 = |(arm_reach + 0.1, 0, cube_size / 2) - target|
 *   r = 2 (1 - tanh 5 d_t) + 2 g + 1.5 (1 - tanh 3 d_p) g + 3 ((d_0 - d_c) / d_0) positioned g;
 *   cube_x > arm_reach + 0.15: r -= 2; success: r += 5; reward = r times reward_scale, metrics[2] = r / 5.
 * (The two centres differ, 0.1 arm_reach = 0.035 against 0.05, as in the task definition.) */
typedef struct mssim_pulltool_task {
  int32_t tcp_row, cube_row, tool_row, base_row, finger1_row, finger2_row; /* rigid_body_data body rows */
  float cube_half_size;       /* 0.02 */
  float hook_length;          /* 0.05 */
  float arm_reach;            /* 0.35 */
  float cube_size;            /* 0.02 (sic: the task definition carries both) */
  float pulled_close_dist;    /* 0.6  */
  float min_force;            /* 0.5 N  (is_grasping of the tool) */
  float max_angle_deg;        /* 20 */
  float reward_scale;         /* 1 (dense) or 1/5 (normalized_dense) */
  int32_t* elapsed_steps;     /* optional, as in mssim_pick_task */
  int32_t* elapsed_out;
  uint8_t* truncated_out;
  int32_t time_limit;
  uint8_t* terminated_out;
} mssim_pulltool_task;

int mssim_task_pulltool_outputs(mssim_handle h, const mssim_pulltool_task* task, float* obs, float* reward, uint8_t* flags, float* metrics, void* stream);

/* PlugCharger-style evaluate + state observation + (zero) dense reward in one launch (envs/tasks/tabletop/plug_charger.py).
 * The goal is not a body row: `goal_pose` is the env's stored [N][7] tensor (p, q wxyz), written at reset; a receptacle
 * moved afterwards leaves it where it was. No grasp and no robot rule is read: no contact pairs, no robot profile. Like the
 * six tasks above, this one never runs at the control-step kernel's tail (the one-row plain step, then this launch).
 * obs [N][2*n_dof+28] f32 (qpos, qvel, tcp_pose7, charger_pose7, receptacle_pose7, goal_pose7), reward [N] f32 = 0 times
 * reward_scale (the task definition's dense reward is zero), flags [N][1] u8 = success,
 * metrics [N][2] f32 = obj_to_goal_dist, obj_to_goal_angle; required.
 *   dist = |goal.p - charger.p|
 *   r = conj(goal.q) * charger.q (Hamilton product, no normalisation), negated where r.w < 0 (quaternion_multiply's
 *   standardisation); angle = 2 atan2(|r.xyz|, r.w), in [0, pi] since r.w >= 0: the task definition's min(a, 2 pi - a) is
 *   then inert and is not applied. (The task definition reaches the same angle as |r.xyz / k|, k = sin(a / 2) / a.)
 *   success = dist <= dist_thresh and angle <= angle_thresh
 * A NaN in the charger's or the goal's position gives a NaN dist, one in either quaternion a NaN angle; every comparison
 * with a NaN is false, so success is 0 for that env, and for that env alone. The observation copies NaNs as they are. */
typedef struct mssim_plug_task {
  int32_t tcp_row, charger_row, receptacle_row; /* rigid_body_data body rows */
  const float* goal_pose;     /* device [N][7] p, q(wxyz): read at every call, kept by the caller; required */
  float dist_thresh;          /* 5e-3 m  */
  float angle_thresh;         /* 0.2 rad */
  float reward_scale;         /* 1 (dense and normalized_dense: the reward is zero either way) */
  int32_t* elapsed_steps;     /* optional, as in mssim_pick_task */
  int32_t* elapsed_out;
  uint8_t* truncated_out;     /* optional device [N]: new elapsed_steps >= time_limit */
  int32_t time_limit;
  uint8_t* terminated_out;    /* optional device [N]: a copy of success */
} mssim_plug_task;

int mssim_task_plug_outputs(mssim_handle h, const mssim_plug_task* task, float* obs, float* reward, uint8_t* flags, float* metrics, void* stream);

/* DrawTriangle-style dot layer + evaluate + state observation in one launch (envs/tasks/tabletop/draw_triangle.py). The
 * drawing is no set of bodies: it is the env's own device tables, which this call updates IN PLACE (update != 0) before it
 * evaluates them. Per env, with k = draw_step[e]:
 *   update and k < max_dots:
 *     drawn = tcp.z < z_thresh (strict; false for a NaN)
 *     dots[e][k] = drawn ? (tcp.x, tcp.y) : (0, 0)
 *     hit_p = drawn and dx * dx + dy * dy < near_thresh2 (each product and the sum rounded to float32; strict), for every
 *             reference point p < n_ref of triangles[e]
 *     dot_near[e][k] = drawn ? (any hit_p ? 1 : 0) : -1;  ref_hit[e][p] |= hit_p;  draw_step[e] = k + 1
 *   update and k >= max_dots: nothing is written to the tables and the counter stays (a step past the table draws nothing)
 *   success = no dot_near[e][i] == 0 for i < max_dots (every drawn dot is near) and every ref_hit[e][p], p < n_ref
 * so an env with nothing drawn fails on its unhit reference points, and a NaN tcp position draws nothing or a dot that is
 * not near: never a success of its own making, and no other env is touched. update == 0 (a reset's outputs) reads only.
 * obs [N][2*n_dof+35] f32 (qpos, qvel, tcp_pose7, goal_pose7, vertices - tcp.p 9, goal_pos3, vertices 9),
 * reward [N] f32 = success * reward_scale (1: sparse, 0: none), flags [N][1] u8 = success.
 * The reference points of an env are spread over the 16 lanes that serve it and reduced with a ballot; no atomics, plain
 * vector stores. Like the seven tasks above, this one never runs at the control-step kernel's tail.
 * Refused (rc 3): a missing table, max_dots that is not a positive multiple of 4, n_ref <= 0, dot_near not 4-byte aligned. */
typedef struct mssim_draw_task {
  int32_t tcp_row, goal_row;  /* rigid_body_data body rows */
  const float* vertices;      /* device [N][3][3]: the goal triangle's corners in the env frame; required */
  const float* triangles;     /* device [N][n_ref][2]: the reference points of the outline; required */
  float* dots;                /* device [N][max_dots][2], in place; required */
  int8_t* dot_near;           /* device [N][max_dots] -1 / 0 / 1, in place; required, 4-byte aligned */
  uint8_t* ref_hit;           /* device [N][n_ref] 0 / 1, in place; required */
  int32_t* draw_step;         /* device [N]: dots appended so far, in place; required */
  int32_t max_dots, n_ref;    /* 300, 153 */
  float z_thresh;             /* 0.028 m */
  float near_thresh2;         /* 0.025^2 m^2 */
  int32_t update;             /* 1: append this step's dot first; 0: outputs of the tables as they are */
  float reward_scale;
  int32_t* elapsed_steps;     /* optional, as in mssim_pick_task */
  int32_t* elapsed_out;
  uint8_t* truncated_out;     /* optional device [N]: new elapsed_steps >= time_limit */
  int32_t time_limit;
  uint8_t* terminated_out;    /* optional device [N]: a copy of success */
} mssim_draw_task;

int mssim_task_draw_outputs(mssim_handle h, const mssim_draw_task* task, float* obs, float* reward, uint8_t* flags, void* stream);

/* The robot-dependent rules of the task epilogues, stored on the handle: what "the robot is static" means and how many
 * joints the velocity norm of PickCube's static reward covers. With no profile set (or after a NULL / n_ranges == 0 call)
 * every epilogue applies the Panda's rules from its own task struct, as before: static = max |qvel[:n_static_dofs]| <=
 * static_thresh, norm over qvel[:n_static_dofs].
 * With a profile set, the separate-launch epilogues that read the robot's velocities (pick, poke, place) use instead
 *     static = for every range r < n_ranges and every joint j in [first[r], first[r] + count[r]):
 *                  (signed_compare ? qvel[j] : |qvel[j]|) <= thresh[r]
 *     PickCube's static reward: 1 - tanh 5 |qvel[:pick_norm_dofs]|  (the other tasks keep their n_static_dofs)
 * and the task struct's static_thresh / robot_static_thresh is not read. The Fetch (agents/robots/fetch/fetch.py
 * is_static): ranges {0, 3, 0.05} (the base) and {3, n - 5, threshold} (body and arm), signed_compare = 1 -- a joint moving
 * fast in the negative direction counts as static, as in the torch path -- and pick_norm_dofs = n (pick_cube.py slices
 * the two finger joints off for "panda" only).
 * The grasp rule needs no entry here: the epilogues test the force on finger1_row against +y of that link and the force on
 * finger2_row against -y; a robot whose fingers close the other way round (the Fetch: -y of the left finger, +y of the
 * right) hands its right finger in as finger 1 and its left as finger 2.
 * The control-step kernel's tail epilogues never read the profile: while one is set, every epilogue of the handle runs as
 * a launch of its own. Refused (rc 3): n_ranges outside [0, 2], a range outside [0, n_dof), pick_norm_dofs outside
 * [0, n_dof], a threshold that is NaN. A null handle returns 1. */
typedef struct mssim_task_robot {
  int32_t n_ranges;            /* 0 (no profile), 1 or 2 */
  int32_t first[2], count[2];  /* joint ranges, within [0, n_dof) */
  float thresh[2];
  int32_t signed_compare;      /* 0: |qvel| <= thresh, 1: qvel <= thresh */
  int32_t pick_norm_dofs;      /* leading joints of PickCube's reward norm, in [0, n_dof] */
} mssim_task_robot;
int mssim_set_task_robot(mssim_handle h, const mssim_task_robot* robot);

/* How many control steps of this handle so far ran as one launch with a task epilogue at the control-step kernel's
 * tail (a deferred step_action + fetch consumed by a task_*_outputs call), against the separate epilogue launch.
 * A host counter: no sync. */
int64_t mssim_tail_step_count(mssim_handle h);

/* Iterative-IK block of the action map: the end-effector modes that track a target pose (pd_ee_pose,
 * pd_ee_target_delta_pos, pd_ee_target_delta_pose; agents/controllers/pd_ee_pose.py). With the block set, apply_action,
 * step_action and defer_step_action clip and scale its columns as the block of set_ee_action_map does, update
 * `target_pose` in place
 *     mode 0: p = lin, q = euler_xyz(rot) (identity with 3 rows)
 *     mode 1: p = p_prev + lin, q = euler_xyz(rot) * q_prev (q_prev with 3 rows); no renormalisation
 * and solve, per env, a damped-least-squares IK of link `link_index` for that pose in the articulation's ROOT frame
 * over the solved joints on the link's path (flagged 4), from the visible qpos buffer:
 *     repeat at most max_iters: err = target - FK(q) (6 rows: + rotation vector of q_t * conj(q_e));
 *       stop when max|err| < tolerance; step = J^T (J J^T + damping I)^-1 err, scaled so that max|step| <= max_step;
 *       q = clip(q + step, joint limits)
 * The exit is per env: an env's answer does not depend on the batch it is in. The result becomes the position target
 * (visible buffer and simulation state) of the solved dofs. Every path dof must be flagged 4 (solved; at most 8) or 64
 * (held: another controller's joint) in set_action_map (call it first). Held dofs enter the forward kinematics at
 * their visible qpos, read once before the loop, have no column in J and get no target from the block; they must form a
 * root-side prefix of the path (the Fetch: base x, y, yaw and torso before the seven arm joints), anything else is
 * refused. A NaN in an env's columns or target gives NaN targets and a NaN target pose for that env alone; a NaN in
 * its held positions gives NaN targets on its solved dofs alone. The block runs as one launch after the joint-space map, followed by the step. Setting this block
 * removes the one of set_ee_action_map and the other way round. */
typedef struct mssim_ee_ik_map {
  int32_t link_index;     /* < 0 removes the block */
  int32_t column0, rows;  /* 3: position, 6: position + XYZ Euler angles */
  int32_t mode;           /* 0 absolute (pd_ee_pose): target = action; 1 target-delta: target = compose(previous target, action) */
  float low, high, rot_scale; int32_t flags;   /* as set_ee_action_map: flags & 2 = clip and map / clip by norm and scale */
  int32_t max_iters; float damping, max_step, tolerance;   /* 60, 1e-3, 0.3, 1e-5; tolerance 0 = run exactly max_iters */
} mssim_ee_ik_map;
int mssim_set_ee_ik_map(mssim_handle h, const mssim_ee_ik_map* map, float* target_pose /* device [N][7] p, q(wxyz): read and written in place by every apply */);
/* The solve alone, with the chain and settings of the block set last: q_out = q0 with the solved path dofs solved; held
 * dofs are read from q0 and copied, as every dof off the path. */
int mssim_ee_ik_solve(mssim_handle h, const float* target_pose /* [N][7] */, const float* q0 /* [N][n_dof] or NULL = visible qpos */,
                      float* q_out /* [N][n_dof]; dofs off the path copied from q0 */, int32_t* iters_out /* optional [N] */, void* stream);

/* ---- Ray-cast camera observations: depth, actor-level segmentation and position --------------------------------
 * A scene is the geometry of one env as the ray caster sees it: analytic shapes, convex hulls (as face planes) and
 * triangle meshes (the model's tri_soup and 16-wide tri_bvh) on rows of `rigid_body_data`, with the same optional per-env
 * overrides as mssim_model_desc ([items][N], env fastest), per-env hulls and per-env segmentation ids included.
 * All arrays of the scene are HOST arrays, read once by mssim_raycast_create. Refused there (non-zero return code and
 * a last_error text, nothing is uploaded or launched): a triangle-mesh shape in a scene without a triangle table, a
 * per-env TRIMESH type in a slot whose shared type is not TRIMESH, a per-env CONVEX type in a slot whose shared type is
 * not CONVEX, rows / plane ranges / triangle ranges / BVH references / slots out of range (per-env ranges in every
 * env), a BVH whose child references form a cycle or that is deeper than MSSIM_RAYCAST_MESH_DEPTH levels.
 *
 * Conventions. The camera pose is in the SAPIEN convention (x forward, y left, z up), relative to the env frame
 * (mount_row < 0) or to the body of `mount_row`, whose pose the kernel reads from rigid_body_data itself. Pixel
 * (column u, row v) casts the ray o + t dir, dir = ((u + 0.5 - cx) / fx, (v + 0.5 - cy) / fy, 1) in the OpenCV camera
 * frame (x right, y down, z forward), not normalised: t is the z-depth. Every shape but a mesh is convex; such a shape's
 * hit is its ENTRY parameter, and counts when near <= t <= min(far, 32.767) -- a shape entered in front of `near`, or
 * holding the ray's start, gives no hit (back faces are culled), and a surface beyond the int16 millimetre range is
 * "nothing". The pixel takes the smallest hit of the env's shapes (the first shape in scene order on an exact tie).
 * Shapes are intersected in their own frames: plane = the half space x <= 0, box = slabs, sphere, capsule / cylinder
 * about +x (side plus caps), convex = clip against the planes (a ray parallel to a plane and outside it misses).
 * A triangle mesh is a SURFACE, not a solid: its hit is the smallest t in [near, min(far, 32.767)] over its triangles,
 * each of them TWO-SIDED (a camera inside a closed mesh sees its walls; the winding of a triangle does not matter). The
 * edge tests are inclusive: a ray through the shared edge or corner of two triangles hits at least one of them. A ray
 * in a triangle's plane misses it. Ties between shapes go to the first in scene order, as above. */
typedef struct mssim_raycast_scene {
  int32_t n_shape;
  const int32_t* shape_type;     /* [n_shape] MSSIM_SHAPE_*                                                                */
  const int32_t* shape_row;      /* [n_shape] rigid_body_data body row of the owner, -1 = fixed in the env frame          */
  const float* shape_frame;      /* [n_shape][7] p, q(wxyz): shape frame in the body (or env) frame                       */
  const float* shape_param;      /* [n_shape][4] as mssim_model_desc.shape_param; TRIMESH: word 0 = first triangle in
                                    tri_soup, word 1 = triangle count, word 2 = root node in tri_bvh (float-valued integers:
                                    the model's shape_param words 0, 1 and its shape_hull word 0)                          */
  const float* shape_bound;      /* [n_shape][4] bounding sphere: centre in the BODY frame, radius; radius < 0 = unbounded */
  const int16_t* shape_seg;      /* [n_shape] segmentation id written where the shape is hit (0 is the background's)       */
  const int32_t* shape_planes;   /* [n_shape][2] CONVEX: first plane, plane count in `planes`; others ignored             */
  int32_t n_plane;
  const float* planes;           /* [n_plane][4] outward unit normal n and offset d in the shape frame, n . x <= d inside  */
  int32_t n_env_shape;           /* per-env override slots                                                                 */
  const int32_t* shape_env_slot; /* [n_shape] slot or -1; may be NULL when n_env_shape == 0                                */
  const float* env_shape_frame;  /* [n_env_shape * 7][N]                                                                   */
  const float* env_shape_param;  /* [n_env_shape * 4][N]: rows 0..2 parameters (TRIMESH: first triangle, triangle count,
                                    root node of THIS env's mesh, as in mssim_model_desc), row 3 = the env's
                                    MSSIM_SHAPE_* + 1 (MSSIM_SHAPE_NONE: the env has nothing in the slot), 0 = the shared type */
  const float* env_shape_bound;  /* [n_env_shape * 4][N]: centre in the BODY frame, radius                                 */
  /* ---- members added for meshes and per-env hulls; 0 / NULL = absent ---- */
  int32_t n_tri;
  const float* tri_soup;         /* [n_tri][12] as mssim_model_desc.tri_soup: centroid, three corners relative to it      */
  int32_t n_tri_node;
  const float* tri_bvh;          /* [n_tri_node][112] as mssim_model_desc.tri_bvh                                          */
  const int32_t* env_shape_planes; /* [n_env_shape * 2][N] first plane, plane count of the env's hull where the env's type
                                    is CONVEX: a different hull per env. NULL: every env renders shape_planes[i]           */
  const int16_t* env_shape_seg;  /* [n_env_shape][N] the id of the slot's shape in each env (the actor that owns the
                                    geometry THERE). NULL: shape_seg[i] in every env                                       */
} mssim_raycast_scene;

typedef struct mssim_camera_desc {
  int32_t width, height;
  float fx, fy, cx, cy;          /* pinhole intrinsics in pixels                                                           */
  float near, far;               /* 0 < near < far                                                                         */
  int32_t mount_row;             /* -1 = the env frame, else the rigid_body_data body row the camera rides on              */
  float pose[7];                 /* p, q(wxyz) relative to the mount; used when env_pose is NULL                           */
  const float* env_pose;         /* optional DEVICE [N][7]: a pose per env instead; read at every render, kept by the caller */
} mssim_camera_desc;

#define MSSIM_RAYCAST_MAX_MM 32767 /* the largest depth a pixel can carry, in millimetres */
#define MSSIM_RAYCAST_CHUNK 64     /* shapes staged on chip at a time: a scene with more is walked in chunks of this many */
#define MSSIM_RAYCAST_MESH_DEPTH 8 /* levels of tri_bvh nodes below (and with) a mesh's root that the kernel's traversal stack holds */

/* Uploads the scene and the cameras; *id names them in the calls below. Allocates: not for the step loop. */
int mssim_raycast_create(mssim_handle h, const mssim_raycast_scene* scene, const mssim_camera_desc* cameras, int32_t n_cameras, int32_t* id);
int mssim_raycast_destroy(mssim_handle h, int32_t id);
/* Renders camera `camera` of every env from the bound rigid_body_data as it is (call it after fetch), on the caller's
 * stream, without host sync or allocation.
 * pos_seg   device int16 [N][H][W][4]: x, y, z in millimetres (truncated toward zero, saturated to int16) in the
 *           camera's OpenGL frame (x right, y up, z backward: (x_cv t, -y_cv t, -t)), then the segmentation id;
 *           all four are 0 where nothing is hit. One 8-byte store per pixel.
 * depth_f32 optional device float [N][H][W]: t in metres, 0 where nothing is hit. */
int mssim_raycast_render(mssim_handle h, int32_t id, int32_t camera, int16_t* pos_seg, float* depth_f32, void* stream);

/* ---- A flat-shaded view of the same scene: what render() and the episode videos show -----------------------------
 * A picture for people of the geometry the ray caster knows (collision shapes, plus whatever shapes the caller appended
 * to the scene for the viewer): the nearest surface per pixel as above, its unit normal at the entry point, one colour
 * per shape and two fixed lights. It is NOT the colour observation of a renderer with visual meshes and textures.
 *   normal   plane +x; box: the axis whose slab set the entry parameter, signed against the ray (lowest axis on a tie);
 *            sphere p / |p|; cylinder (+-1, 0, 0) where the cap slab set the entry, else (0, p_y, p_z) / r; capsule: of
 *            whichever of its cylinder and two balls gave the earliest entry; hull: of the first plane in index order
 *            that set the entry; triangle (e1 x e2) / |e1 x e2| turned to face the ray (two-sided, as for depth).
 *   light    ambient 0.3, two white directional lights along (1, 1, -1) / sqrt 3 and (0, 0, -1) in the env frame, no
 *            shadows, no specular term: c = albedo * min(1, 0.3 + sum_i max(0, -l_i . n)), byte = floor(255 min(c, 1) + 0.5).
 *   albedo   rgb of the shape's colour; word 3 is a checker cell size w in metres (0: none): where
 *            floor(p.x / w) + floor(p.y / w) + floor(p.z / w) is odd, p the entry point in the SHAPE frame (a plane's
 *            p.x counts as exactly 0), the albedo is scaled by 0.8.
 * mssim_raycast_set_colours: HOST arrays, copied. shape_rgba [n_shape][4]; env_shape_rgba [n_env_shape][N][4] (slot,
 * then env) or NULL: a colour per env for the shapes in per-env slots, where actors of different sub-scenes share a body
 * row. Refused (non-zero code, last_error text, tables unchanged): a negative or non-finite colour or cell size, a per-env
 * table for a scene without per-env slots. It waits for the device and may allocate: not for the step loop.
 * mssim_raycast_shade: one launch on the caller's stream, no host sync, no allocation. rgba_u8 device uint8 [N][H][W][4]:
 * r, g, b, 255; a pixel that hits nothing gets one background colour. One 4-byte store per pixel: rgba_u8 must be 4-byte
 * aligned. Refused: a bad id or camera, shading before any colours were set, a misaligned or missing output. */
int mssim_raycast_set_colours(mssim_handle h, int32_t id, const float* shape_rgba, const float* env_shape_rgba);
int mssim_raycast_shade(mssim_handle h, int32_t id, int32_t camera, uint8_t* rgba_u8, void* stream);

/* ---- A dot layer composited over a shaded view: the drawing of DrawTriangle-style tasks ---------------------------
 * The dots are no shapes of the scene: they are an env's table of xy positions (mssim_draw_task). One launch over the
 * RGBA picture of mssim_raycast_shade: a pixel's ray meets the horizontal plane z = `z` of the env frame at parameter t
 * (the z-depth, as above); where t >= near, the point lies within `radius` of a drawn dot (dot_near[e][i] >= 0,
 * i < min(count[e], max_dots)) and nothing of the scene is more than 1 mm nearer (depth_f32 of mssim_raycast_render for the
 * same scene, camera and state: 0 = nothing, else t <= depth + 1e-3), the pixel becomes `rgba`; every other pixel keeps
 * what it had. One 4-byte store per painted pixel, no atomics. Refused: a bad id or camera, a missing table or buffer,
 * max_dots outside [1, 1024], a misaligned picture. */
typedef struct mssim_dot_layer {
  const float* dots;        /* device [N][max_dots][2] */
  const int8_t* dot_near;   /* device [N][max_dots]: < 0 = not drawn */
  const int32_t* count;     /* device [N]: table entries in use */
  int32_t max_dots;
  float z, radius;          /* plane height and disc radius, metres */
  uint32_t rgba;            /* r | g << 8 | b << 16 | a << 24 */
} mssim_dot_layer;
int mssim_raycast_draw_dots(mssim_handle h, int32_t id, int32_t camera, const mssim_dot_layer* layer, const float* depth_f32, uint8_t* rgba_u8, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MSSIM_HIP_TASKS_H */
