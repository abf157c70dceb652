"""The parallel form of the binned-SAH builder (ipu_path_trace_amd/csrc/pt_mesh_sah.h: one set of functions for the kernels and the host)
on the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer, as the stand-alone program tests/mesh_sah_main.cpp.  For the six
fixtures of tests/mesh_bvh_main.cpp and the eight small ones of tests/mesh_lbvh_main.cpp, in the world frame and under two poses: the
parallel form run thread by thread, in thread order and in reversed thread order, gives ptmesh::build's bytes; the depth cap at 2
and 3 agrees with a direct recursive restatement; walk == brute force over 2^16 rays.  Zero differences required.  A partition
that is not stable, and a cost scan with <= for <, must each fail it."""
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
    build = subprocess.run(["g++"] + FLAGS + list(extra) + ["-o", exe, os.path.join(ROOT, "tests", "mesh_sah_main.cpp")],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=900)
    assert "runtime error" not in run.stderr and "ERROR: AddressSanitizer" not in run.stderr, run.stderr[-4000:]
    return run


def test_parallel_form_equals_the_host_builder_under_sanitizers(tmp_path):
    run = _build_and_run(tmp_path, "mesh_sah")
    print(run.stdout)
    assert run.returncode == 0 and "MESH_SAH_OK" in run.stdout, run.stdout[-3000:] + run.stderr[-4000:]
    lines = run.stdout.splitlines()
    frames = [l for l in lines if " levels, forward " in l]
    caps = [l for l in lines if " cap 2 " in l or " cap 3 " in l]
    rays = [l for l in lines if " rays   " in l]
    assert len(frames) == 3 * N_FIXTURES and all(l.endswith("forward identical, reversed identical") for l in frames)
    assert len(caps) == 2 * N_FIXTURES and all(l.endswith(": identical") for l in caps)
    assert len(rays) == N_FIXTURES and all(l.endswith(" 0 differences") for l in rays)
    assert any(" 0 levels" in l for l in frames) and any(" 12 levels" in l for l in frames)      # a lone leaf, and a tree with large ranges


@pytest.mark.parametrize("macro", ["PT_SAH_MUTATE_UNSTABLE", "PT_SAH_MUTATE_LE"])
def test_a_mutated_rule_fails(tmp_path, macro):
    run = _build_and_run(tmp_path, "mesh_sah_" + macro.lower(), ["-D" + macro], ["--only", "icosphere2"])
    assert run.returncode == 1 and "MESH_SAH_FAILED" in run.stdout and "MESH_SAH_OK" not in run.stdout, run.stdout[-3000:]
    assert "the parallel form" in run.stderr and "differs from ptmesh::build" in run.stderr, run.stderr[-3000:]
