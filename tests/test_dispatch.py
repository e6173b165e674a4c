"""Which instance of the control-step kernel a model runs, with or without a task's tail
(maniskill_amd/csrc/mssim_dispatch.h: what mssim_create resolves to kernel pointers) on the CPU:
tests/native/dispatch_check.cpp, a stand-alone program, built with AddressSanitizer + UndefinedBehaviorSanitizer and run
as a child process."""
import os
import re
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


def compiled_instances():
    """(NDOF, TASK, TRI, NR) of every X(...) of the full MSSIM_SOLVE16_INSTANCES list (the #else branch: not MSSIM_ONLY_PANDA's)"""
    with open(os.path.join(ROOT, "maniskill_amd", "csrc", "mssim_dispatch.h")) as f:
        text = f.read()
    full = text.split("#define MSSIM_SOLVE16_INSTANCES(X)")[2].split("#endif")[0]
    found = re.findall(r"\bX\(\s*(\d+)\s*,\s*(\d+)\s*,\s*(true|false)\s*,\s*(\d+)\s*\)", full)
    assert len(found) == full.count("X(") and found, full
    return [(int(a), int(b), c == "true", int(d)) for a, b, c, d in found]


def test_every_plain_instance_has_a_direct_lcp_scene(tmp_path):
    """the scenes and mesh variants of tests/articulated_lcp_cases.py -- each asserts, where it compiles its model, the instance it
    runs -- reach every plain-step (TASK 0) instance of the list and nothing else: an instance added to the list without a scene
    held to the direct LCP solution fails here"""
    from tests import articulated_lcp_cases as cases

    inst = compiled_instances()
    assert len(inst) == len(set(inst))
    plain = {(ndof, nr, tri) for ndof, task, tri, nr in inst if task == 0}
    reached = {}
    for name in cases.CASES:
        sc = cases.make_scene(name, tmp_path)
        cases.compile_scene(sc)  # (asserts that the model's joints, free bodies and meshes select sc.instance)
        reached.setdefault(sc.instance, []).append(name)
    assert set(reached) == plain, (sorted(plain - set(reached)), sorted(set(reached) - plain))
