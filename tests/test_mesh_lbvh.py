"""The linear BVH builder and the refit (ipu_path_trace_amd/csrc/pt_mesh_build.h: one set of functions for the kernels and the host) on
the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer, as the stand-alone program tests/mesh_lbvh_main.cpp.  For the six
fixtures of tests/mesh_bvh_main.cpp and eight small ones (2, 3, 4, 5, 8, 9 triangles, nine copies of one triangle, an exactly planar
mesh): the reference builder's invariants, two builds identical, the parallel form (the kernels' per-thread functions run one after
the other) identical to it, walk == brute force bit for bit over 2^16 rays, and the same for the SAH and the linear tree refitted
under three poses.  Zero differences required.  A refit without the pad, and one that keeps the old root's pad, must each fail it."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
         "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ipu_path_trace_amd", "csrc"),
         "-I" + os.path.join(ROOT, "tests")]
N_FIXTURES = 14


def _build_and_run(tmp_path, name, extra=(), args=()):
    exe = str(tmp_path / name)
    build = subprocess.run(["g++"] + FLAGS + list(extra) + ["-o", exe, os.path.join(ROOT, "tests", "mesh_lbvh_main.cpp")],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=900)
    assert "runtime error" not in run.stderr and "ERROR: AddressSanitizer" not in run.stderr, run.stderr[-4000:]
    return run


def test_reference_builder_parallel_form_and_refit_under_sanitizers(tmp_path):
    run = _build_and_run(tmp_path, "mesh_lbvh")
    print(run.stdout)
    assert run.returncode == 0 and "MESH_LBVH_OK" in run.stdout, run.stdout[-3000:] + run.stderr[-4000:]
    world = [l for l in run.stdout.splitlines() if " world " in l]
    posed = [l for l in run.stdout.splitlines() if "SAH refit" in l]
    assert len(world) == N_FIXTURES and all(" 0 differences, 0 against the SAH walk" in l for l in world)
    assert len(posed) == 3 * N_FIXTURES
    assert all(l.endswith("SAH refit 0, linear refit 0, host rebuild 0, linear build 0 differences") for l in posed)


@pytest.mark.parametrize("macro", ["PT_LBVH_MUTATE_NO_PAD", "PT_LBVH_MUTATE_KEEP_PAD"])
def test_a_mutated_refit_fails(tmp_path, macro):
    run = _build_and_run(tmp_path, "mesh_lbvh_" + macro.lower(), ["-D" + macro], ["--only", "icosphere2"])
    assert run.returncode == 1 and "MESH_LBVH_FAILED" in run.stdout and "MESH_LBVH_OK" not in run.stdout, run.stdout[-3000:]
    assert "refit" in run.stderr, run.stderr[-3000:]
