"""The DrawTriangle epilogue in the dispatch table (maniskill_amd/csrc/mssim_dispatch.h), asked through the table's own
constexpr API by a small program compiled here: kDraw is a task id of its own, no instance of the control-step kernel
carries its tail (its epilogue is always a launch of its own, after the plain step <7, 0, false, 1>), and
MSSIM_SOLVE16_INSTANCES is the list of twenty it was before the task came."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdio>
#include <initializer_list>
#include "mssim_dispatch.h"
using namespace mssim_dispatch;
int main() {
  std::printf("kDraw %d kPlug %d kNumTasks %d\n", (int)kDraw, (int)kPlug, (int)kNumTasks);
  for (int i = 0; i < kNumInstances; i++) std::printf("X %d %d %d %d\n", kInstances[i].ndof, kInstances[i].task, (int)kInstances[i].tri, kInstances[i].nr);
  int tails = 0;
  for (int n_dof = 0; n_dof <= 16; n_dof++)
    for (int rows = 1; rows <= 4; rows *= 2)
      for (int tri = 0; tri < 2; tri++)
        for (int N : {1, 64, 4096, 65536}) tails += !(tail_step(kDraw, n_dof, rows, tri != 0, N, 256) == kNone);
  std::printf("draw tails %d\n", tails);
  const Key p = plain_step(7, 1, false);
  std::printf("plain %d %d %d %d at %d\n", p.ndof, p.task, (int)p.tri, p.nr, find_instance(p));
  for (const TailRow& t : kTails) std::printf("T %d %d %d\n", t.task, t.n_dof, t.rows_per_env);
  return 0;
}
"""

# (NDOF, TASK, TRI, NR), in the list's order, as on the parent of the commit that added DrawTriangle
INSTANCES = [(0, 0, 1, 4), (0, 0, 0, 4), (9, 0, 1, 2), (15, 0, 1, 2), (0, 0, 1, 2), (9, 0, 0, 2), (9, 4, 0, 2), (15, 0, 0, 2), (0, 0, 0, 2), (9, 0, 1, 1),
             (15, 0, 1, 1), (0, 0, 1, 1), (9, 0, 0, 1), (9, 1, 0, 1), (9, 2, 0, 1), (9, 3, 0, 1), (7, 0, 0, 1), (7, 5, 0, 1), (15, 0, 0, 1), (0, 0, 0, 1)]
TAILS = [(1, 9, 1), (2, 9, 1), (3, 9, 1), (4, 9, 2), (5, 7, 1)]


def test_draw_is_in_the_table_and_the_instance_list_is_unchanged(tmp_path):
    src, exe = tmp_path / "draw_dispatch.cpp", str(tmp_path / "draw_dispatch")
    src.write_text(PROGRAM)
    built = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "maniskill_amd", "csrc"), "-o", exe, str(src)],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    lines = ran.stdout.splitlines()
    assert lines[0] == "kDraw 13 kPlug 12 kNumTasks 14", lines[0]
    assert [tuple(int(x) for x in l.split()[1:]) for l in lines if l.startswith("X ")] == INSTANCES
    assert [tuple(int(x) for x in l.split()[1:]) for l in lines if l.startswith("T ")] == TAILS
    assert "draw tails 0" in lines, "no instance of the control-step kernel carries DrawTriangle's tail"
    assert f"plain 7 0 0 1 at {INSTANCES.index((7, 0, 0, 1))}" in lines


def test_the_library_exports_the_epilogue_and_the_dot_layer():
    with open(os.path.join(ROOT, "include", "mssim_hip_tasks.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "maniskill_amd", "csrc", "mssim_kernels.hip")) as f:
        kernels = f.read()
    assert "int mssim_task_draw_outputs(" in header and "int mssim_raycast_draw_dots(" in header
    assert "mssim_dispatch::kDraw" in kernels and "k_task_draw<decltype(fetch)::value>" in kernels
    from maniskill_amd import native

    lib = native.NativeLib.load()
    assert lib.task_draw_outputs is not None and lib.raycast_draw_dots is not None
