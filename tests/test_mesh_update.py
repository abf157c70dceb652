"""The rule of pt_update_mesh_vertices (ipu_path_trace_amd/csrc/pt_mesh_update.h: one set of functions for the kernels, the host and
this program) on the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer, as the stand-alone program
tests/mesh_update_main.cpp.  For seven fixtures, original and deformed: frame_thread == ptmesh::world_frames and
corner_normals_thread == ptmesh::corner_normals byte for byte; a SAH and a linear tree built on the original and refitted
(ptlbvh::refit) to the deformed frames pass the tree invariants and walk == brute force on 2^14 rays, in the world frame and under
a pose; seeded bad vertices and normals get the triangle and the kind of fault ptmesh::check / check_normals name.  Zero
differences required.  e2 = v2 - v1, and "any offending triangle" for "the lowest", must each fail it."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
         "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ipu_path_trace_amd", "csrc"),
         "-I" + os.path.join(ROOT, "tests")]
FIXTURES = ["icosphere2", "grid", "single", "tri4", "tri5", "tri9", "sliver"]
FAULTS = ["a NaN vertex", "an inf vertex", "a cross product that overflows", "an exactly collinear triangle", "two bad triangles",
          "a NaN normal", "a zero normal", "dot(n, n) overflows", "two bad normals"]


def _build_and_run(tmp_path, name, extra=()):
    exe = str(tmp_path / name)
    build = subprocess.run(["g++"] + FLAGS + list(extra) + ["-o", exe, os.path.join(ROOT, "tests", "mesh_update_main.cpp")],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert "runtime error" not in run.stderr and "ERROR: AddressSanitizer" not in run.stderr, run.stderr[-4000:]
    return run


def test_the_header_compiles_alone(tmp_path):
    """pt_mesh_update.h holds no HIP type: g++ -ffp-contract=off compiles it on its own."""
    src = tmp_path / "alone.cpp"
    src.write_text('#include "pt_mesh_update.h"\nint main() { float fr[12]; const unsigned ix[3] = {0, 1, 2}; const float v[9] = {0, 0, 0, 1, 0, 0, 0, 1, 0};\n'
                   "  return ptupdate::frame_thread(0, ix, v, fr) == ptupdate::kStatusOk && fr[11] == 1.0f ? 0 : 1; }\n")
    exe = str(tmp_path / "alone")
    build = subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "ipu_path_trace_amd", "csrc"),
                            "-o", exe, str(src)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    assert subprocess.run([exe]).returncode == 0


def test_frames_refit_and_faults_under_sanitizers(tmp_path):
    run = _build_and_run(tmp_path, "mesh_update")
    print(run.stdout)
    assert run.returncode == 0 and "MESH_UPDATE_OK" in run.stdout, run.stdout[-3000:] + run.stderr[-4000:]
    lines = run.stdout.splitlines()
    refits = [l for l in lines if " refit " in l and " rays, " in l]
    assert len(refits) == 4 * len(FIXTURES)                       # (world, posed) x (SAH, linear)
    assert all(": 16384 rays, " in l and l.endswith(" 0 differences") for l in refits)
    for name in FIXTURES:
        assert sum(l.startswith(name + " ") for l in refits) == 4
    for what in FAULTS:
        assert sum(l.startswith(what) for l in lines) >= 1, what
    assert sum(l.startswith("a NaN normal") or l.startswith("a zero normal") for l in lines) == 4   # per vertex and per corner


@pytest.mark.parametrize("macro,names", [("PT_MESH_UPDATE_MUTATE_EDGE", "frame_thread differs from ptmesh::world_frames"),
                                         ("PT_MESH_UPDATE_MUTATE_ANY", "the pass reports")])
def test_a_mutated_rule_fails(tmp_path, macro, names):
    run = _build_and_run(tmp_path, "mesh_update_" + macro.lower(), ["-D" + macro])
    assert run.returncode == 1 and "MESH_UPDATE_FAILED" in run.stdout and "MESH_UPDATE_OK" not in run.stdout, run.stdout[-3000:]
    assert names in run.stderr, run.stderr[-3000:]
