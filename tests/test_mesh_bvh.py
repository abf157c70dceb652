"""The mesh builder (ipu_path_trace_amd/csrc/ptmi_mesh.h) and the stackless walk the kernels run (csrc/pt_mesh.h) on the CPU, under
AddressSanitizer and UndefinedBehaviorSanitizer, as the stand-alone program tests/mesh_bvh_main.cpp: the tree's invariants on six
fixtures, then walk == brute force bit for bit in (t, triangle) on 2^16 rays per fixture, zero differences required (the calibration
of the boxes' pad), and a part with pad 0 where every operation is exact.  The two mutations of the walk -- < for <= in the node
cull, a NaN in the slab test rejecting the node -- must each fail it."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
         "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ipu_path_trace_amd", "csrc")]


def _build_and_run(tmp_path, name, extra=(), args=()):
    exe = str(tmp_path / name)
    build = subprocess.run(["g++"] + FLAGS + list(extra) + ["-o", exe, os.path.join(ROOT, "tests", "mesh_bvh_main.cpp")],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=600)
    assert "runtime error" not in run.stderr and "ERROR: AddressSanitizer" not in run.stderr, run.stderr[-4000:]
    return run


def test_tree_invariants_and_walk_equals_brute_force_under_sanitizers(tmp_path):
    run = _build_and_run(tmp_path, "mesh_bvh")
    print(run.stdout)
    assert run.returncode == 0 and "MESH_BVH_OK" in run.stdout, run.stdout[-3000:] + run.stderr[-4000:]
    lines = [l for l in run.stdout.splitlines() if "differences" in l]
    assert len(lines) == 7 and all(l.endswith(" 0 differences") for l in lines)       # six fixtures and the exact part


@pytest.mark.parametrize("macro,where", [("PT_MESH_MUTATE_CULL", ("grid", "exact")), ("PT_MESH_MUTATE_NAN", ("exact",))])
def test_a_mutated_walk_fails(tmp_path, macro, where):
    """With the production pad a ray in a node's slab plane cannot meet that node's triangles, so the NaN rule shows in the exact
    part alone (pad 0); the cull's <= shows there and on the grid's far family, where the pad is absorbed by rounding."""
    run = _build_and_run(tmp_path, "mesh_bvh_" + macro.lower(), ["-D" + macro], ["--only", "grid"])
    assert run.returncode == 1 and "MESH_BVH_FAILED" in run.stdout and "MESH_BVH_OK" not in run.stdout, run.stdout[-3000:]
    for name in where:
        line = [l for l in run.stdout.splitlines() if l.startswith(name + " ")]
        assert len(line) == 1 and not line[0].endswith(" 0 differences"), run.stdout[-3000:]
