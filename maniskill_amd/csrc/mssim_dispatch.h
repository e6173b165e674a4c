// mssim_dispatch.h -- which instance of the control-step kernel k_solve16<NDOF, TASK, TRI, NR> (mssim_solve16.h) a handle
// runs: the list of instances the library compiles, the one a plain step takes, and the one (if any) that carries a
// task's epilogue at its tail. mssim_create resolves both to kernel pointers once. Plain C++17, no HIP:
// tests/native/dispatch_check.cpp checks the rules on a CPU.
#pragma once

namespace mssim_dispatch {

// TASK: 0 = plain control step; else the copy-out + that task's epilogue at the kernel's tail. kRoll, kPull, kPoke,
// kLiftPeg, kPlace, kPullTool, kPlug and kDraw have no row in kTails: their epilogue is always a launch of its own, tail_step() answers
// kNone for them (kPoke and kPullTool on the two-row plain step, the other six on the one-row one; kDraw steps with <7, 0, false, 1>).
enum Task { kPlain = 0, kPick = 1, kPush = 2, kPeg = 3, kStack = 4, kPushT = 5, kRoll = 6, kPull = 7, kPoke = 8, kLiftPeg = 9, kPlace = 10, kPullTool = 11,
            kPlug = 12, kDraw = 13, kNumTasks = 14 };

struct Key {
  int ndof;  // joints unrolled at compile time (9: the Panda, 7: panda_stick, 15: the Fetch), 0 = any topology
  int task;
  bool tri;  // carries the triangle-mesh stage
  int nr;    // 16-lane rows per env
};
constexpr bool operator==(const Key& a, const Key& b) { return a.ndof == b.ndof && a.task == b.task && a.tri == b.tri && a.nr == b.nr; }
constexpr Key kNone{-1, -1, false, 0};

// THE instance list, X(NDOF, TASK, TRI, NR): mssim_kernels.hip instantiates exactly these and launches nothing else.
#ifdef MSSIM_ONLY_PANDA
// (timing experiments, scripts/ab_variants.sh: only the benchmark's instances -- a fifth of the build time. Every model
// runs the Panda's one-row instance, StackCube and PushT take the separate epilogue launch.)
#define MSSIM_SOLVE16_INSTANCES(X) X(9, 0, false, 1) X(9, 1, false, 1) X(9, 2, false, 1) X(9, 3, false, 1)
#else
#define MSSIM_SOLVE16_INSTANCES(X)                                                                           \
  /* four rows (three to six free bodies, a whole wave per env): generic topology only */                    \
  X(0, 0, true, 4) X(0, 0, false, 4)                                                                         \
  /* two rows (more than 16 velocity components); TASK 4: StackCube, the Panda with two cubes */             \
  X(9, 0, true, 2) X(15, 0, true, 2) X(0, 0, true, 2)                                                        \
  X(9, 0, false, 2) X(9, 4, false, 2) X(15, 0, false, 2) X(0, 0, false, 2)                                   \
  /* one row; a model with meshes never carries a task tail; <7, 0> so that PushT steps with the same */     \
  /* physics fused and unfused */                                                                            \
  X(9, 0, true, 1) X(15, 0, true, 1) X(0, 0, true, 1)                                                        \
  X(9, 0, false, 1) X(9, 1, false, 1) X(9, 2, false, 1) X(9, 3, false, 1) X(7, 0, false, 1) X(7, 5, false, 1) \
  X(15, 0, false, 1) X(0, 0, false, 1)
#endif

#define MSSIM_DISPATCH_KEY_(NDOF, TASK, TRI, NR) Key{NDOF, TASK, TRI, NR},
constexpr Key kInstances[] = {MSSIM_SOLVE16_INSTANCES(MSSIM_DISPATCH_KEY_)};
#undef MSSIM_DISPATCH_KEY_
constexpr int kNumInstances = sizeof(kInstances) / sizeof(kInstances[0]);

// position of `k` in the list, -1: not compiled
constexpr int find_instance(const Key& k) {
  for (int i = 0; i < kNumInstances; i++)
    if (kInstances[i] == k) return i;
  return -1;
}

// the instance a plain step of a model runs
constexpr Key plain_step(int n_dof, int rows_per_env, bool has_tri) {
#ifdef MSSIM_ONLY_PANDA
  (void)n_dof; (void)rows_per_env; (void)has_tri;
  return Key{9, 0, false, 1};
#else
  if (rows_per_env == 4) return Key{0, 0, has_tri, 4};
  const bool unrolled = n_dof == 9 || n_dof == 15 || (n_dof == 7 && rows_per_env == 1 && !has_tri);
  return Key{unrolled ? n_dof : 0, 0, has_tri, rows_per_env};
#endif
}

// every model mssim_create accepts (at most 16 joints; 1, 2 or 4 rows) has its plain step in the list
constexpr bool plain_steps_compiled() {
  for (int n_dof = 0; n_dof <= 16; n_dof++)
    for (int rows = 1; rows <= 4; rows *= 2)
      if (find_instance(plain_step(n_dof, rows, false)) < 0 || find_instance(plain_step(n_dof, rows, true)) < 0) return false;
  return true;
}
static_assert(plain_steps_compiled(), "MSSIM_SOLVE16_INSTANCES lacks an instance that plain_step() selects");

// the model a task's tail is compiled for
struct TailRow { int task, n_dof, rows_per_env; };
constexpr TailRow kTails[] = {{kPick, 9, 1}, {kPush, 9, 1}, {kPeg, 9, 1}, {kStack, 9, 2}, {kPushT, 7, 1}};

// The tail runs at the kernel's one wave per SIMD: worth it while the whole launch is resident at once and latency-bound
// anyway; beyond that the separate, fully occupied copy-out + epilogue launch is cheaper than a tail per block. One row:
// waves of 4 envs, at most 4 per CU (N <= 4096 on 256 CUs). Two rows: blocks of 8 envs, the same count (N <= 8192 on 256
// CUs). Measured (StackCube, 4096 envs, 1000 unreset steps): 0.947 ms per step with the tail, 0.963 ms with the
// separate launch.
constexpr bool tail_fits(int rows_per_env, int N, int n_cu) {
  const int envs = rows_per_env == 1 ? 4 : 8;
  return (N + envs - 1) / envs <= 4 * n_cu;
}

// the instance that runs a control step of the model with `task`'s epilogue at its tail, kNone: there is none (the
// control step and the epilogue are two launches)
constexpr Key tail_step(int task, int n_dof, int rows_per_env, bool has_tri, int N, int n_cu) {
  for (const TailRow& t : kTails) {
    if (t.task != task || t.n_dof != n_dof || t.rows_per_env != rows_per_env || has_tri || !tail_fits(rows_per_env, N, n_cu)) continue;
    const Key k{t.n_dof, t.task, false, t.rows_per_env};
    return find_instance(k) >= 0 ? k : kNone;
  }
  return kNone;
}

}  // namespace mssim_dispatch
