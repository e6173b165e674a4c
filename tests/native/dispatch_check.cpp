// dispatch_check.cpp -- CPU check of maniskill_amd/csrc/mssim_dispatch.h: the instance list of the control-step kernel,
// the instance a plain step selects and the instance (or none) that carries a task's tail, for every model shape
// mssim_create accepts. The expectations are written out here, not derived from the header. Stand-alone
// (tests/test_dispatch.py builds it with ASan + UBSan and expects exit status 0).
#include <cstdio>

#include "../../maniskill_amd/csrc/mssim_dispatch.h"

using namespace mssim_dispatch;

static int g_failed = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::printf("%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond);   \
      g_failed++;                                                            \
    }                                                                        \
  } while (0)

// the 20 instances of the default build, (NDOF, TASK, TRI, NR)
static const Key kExpected[] = {
    {0, 0, true, 4},  {0, 0, false, 4},
    {9, 0, true, 2},  {15, 0, true, 2},  {0, 0, true, 2},
    {9, 0, false, 2}, {9, 4, false, 2},  {15, 0, false, 2}, {0, 0, false, 2},
    {9, 0, true, 1},  {15, 0, true, 1},  {0, 0, true, 1},
    {9, 0, false, 1}, {9, 1, false, 1},  {9, 2, false, 1},  {9, 3, false, 1}, {7, 0, false, 1}, {7, 5, false, 1}, {15, 0, false, 1}, {0, 0, false, 1},
};

static bool same(const Key& a, const Key& b) { return a.ndof == b.ndof && a.task == b.task && a.tri == b.tri && a.nr == b.nr; }
static bool listed(const Key& k) {
  for (const Key& i : kInstances)
    if (same(i, k)) return true;
  return false;
}

static void check_instance_list() {
  CHECK(kNumInstances == 20);
  CHECK(sizeof(kExpected) / sizeof(kExpected[0]) == 20);
  for (int i = 0; i < kNumInstances; i++)
    for (int j = i + 1; j < kNumInstances; j++) CHECK(!same(kInstances[i], kInstances[j]));
  for (const Key& k : kExpected) CHECK(listed(k));
  for (int i = 0; i < kNumInstances; i++) CHECK(find_instance(kInstances[i]) == i);
  CHECK(find_instance(Key{9, 5, false, 1}) == -1);
  CHECK(find_instance(kNone) == -1);
}

static void check_selection() {
  const int kRows[] = {1, 2, 4};
  int tails = 0;
  for (int n_dof = 0; n_dof <= 16; n_dof++)
    for (int rows : kRows)
      for (int tri = 0; tri < 2; tri++) {
        // plain step: four rows run the generic instance; two rows keep 9 and 15 joints; one row keeps 9 and 15, and 7 without a mesh
        int ndof = 0;
        if (rows == 2 && (n_dof == 9 || n_dof == 15)) ndof = n_dof;
        if (rows == 1 && (n_dof == 9 || n_dof == 15 || (n_dof == 7 && !tri))) ndof = n_dof;
        const Key plain = plain_step(n_dof, rows, tri != 0);
        CHECK(same(plain, Key{ndof, 0, tri != 0, rows}));
        CHECK(listed(plain));
        for (int task = 0; task <= 5; task++) {
          // a tail: pick / push / peg on the Panda's one row, stack on its two, pusht on panda_stick's one; never with a mesh
          const bool expect = !tri && ((task >= 1 && task <= 3 && n_dof == 9 && rows == 1) || (task == 4 && n_dof == 9 && rows == 2) || (task == 5 && n_dof == 7 && rows == 1));
          const Key tail = tail_step(task, n_dof, rows, tri != 0, 1, 256);
          if (expect) {
            CHECK(same(tail, Key{n_dof, task, false, rows}));
            CHECK(listed(tail));
            tails++;
          } else {
            CHECK(same(tail, kNone));
          }
        }
      }
  CHECK(tails == 5);
  // spelled out
  CHECK(same(plain_step(9, 1, false), Key{9, 0, false, 1}));
  CHECK(same(plain_step(7, 1, false), Key{7, 0, false, 1}));
  CHECK(same(plain_step(7, 1, true), Key{0, 0, true, 1}));
  CHECK(same(plain_step(7, 2, false), Key{0, 0, false, 2}));
  CHECK(same(plain_step(15, 2, true), Key{15, 0, true, 2}));
  CHECK(same(plain_step(9, 4, false), Key{0, 0, false, 4}));
  CHECK(same(plain_step(12, 1, false), Key{0, 0, false, 1}));
  CHECK(same(tail_step(kPick, 9, 1, false, 64, 256), Key{9, 1, false, 1}));
  CHECK(same(tail_step(kPush, 9, 1, false, 64, 256), Key{9, 2, false, 1}));
  CHECK(same(tail_step(kPeg, 9, 1, false, 64, 256), Key{9, 3, false, 1}));
  CHECK(same(tail_step(kStack, 9, 2, false, 64, 256), Key{9, 4, false, 2}));
  CHECK(same(tail_step(kPushT, 7, 1, false, 64, 256), Key{7, 5, false, 1}));
  CHECK(same(tail_step(kStack, 9, 1, false, 64, 256), kNone));
  CHECK(same(tail_step(kPick, 9, 2, false, 64, 256), kNone));
  CHECK(same(tail_step(kPick, 7, 1, false, 64, 256), kNone));
  CHECK(same(tail_step(kPick, 9, 1, true, 64, 256), kNone));
}

static void check_size_rule() {
  // one row: ceil(N / 4) <= 4 * n_cu; two rows: ceil(N / 8) <= 4 * n_cu
  CHECK(tail_fits(1, 1, 256) && tail_fits(2, 1, 256));
  CHECK(tail_fits(1, 4096, 256) && !tail_fits(1, 4097, 256));
  CHECK(tail_fits(2, 8192, 256) && !tail_fits(2, 8193, 256));
  CHECK(same(tail_step(kPick, 9, 1, false, 1, 256), Key{9, 1, false, 1}));
  CHECK(same(tail_step(kPick, 9, 1, false, 4096, 256), Key{9, 1, false, 1}));
  CHECK(same(tail_step(kPick, 9, 1, false, 4097, 256), kNone));
  CHECK(same(tail_step(kPushT, 7, 1, false, 4096, 256), Key{7, 5, false, 1}));
  CHECK(same(tail_step(kPushT, 7, 1, false, 4097, 256), kNone));
  CHECK(same(tail_step(kStack, 9, 2, false, 1, 256), Key{9, 4, false, 2}));
  CHECK(same(tail_step(kStack, 9, 2, false, 8192, 256), Key{9, 4, false, 2}));
  CHECK(same(tail_step(kStack, 9, 2, false, 8193, 256), kNone));
  CHECK(same(tail_step(kPick, 9, 1, false, 16, 1), Key{9, 1, false, 1}));
  CHECK(same(tail_step(kPick, 9, 1, false, 17, 1), kNone));
}

int main() {
  check_instance_list();
  check_selection();
  check_size_rule();
  if (g_failed) {
    std::printf("dispatch_check: %d check(s) failed\n", g_failed);
    return 1;
  }
  std::printf("dispatch_check: ok\n");
  return 0;
}
