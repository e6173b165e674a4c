"""Which instance of the control-step kernel a model runs, with or without a task's tail
(maniskill_amd/csrc/mssim_dispatch.h: what mssim_create resolves to kernel pointers) on the CPU:
tests/native/dispatch_check.cpp, a stand-alone program, built with AddressSanitizer + UndefinedBehaviorSanitizer and run
as a child process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dispatch_check_passes_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "dispatch_check")
    src = os.path.join(ROOT, "tests", "native", "dispatch_check.cpp")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-o", exe, src]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    assert "dispatch_check: ok" in ran.stdout
