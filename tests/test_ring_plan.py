"""The ring of batch-buffer sets (ipu_path_trace_amd/csrc/ptmi_step_plan.h: ring_slot, ring_predecessor, store_region) and the
owner-map count in the automatic sharing budget (ptmi_share_plan.h) on the CPU, under AddressSanitizer and
UndefinedBehaviorSanitizer.  Both headers include nothing from HIP, so the stand-alone program tests/ring_plan_main.cpp
compiles with g++ alone."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ring_plan_under_sanitizers(tmp_path):
    exe = str(tmp_path / "ring_plan")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "ipu_path_trace_amd", "csrc"), "-o", exe,
                            os.path.join(ROOT, "tests", "ring_plan_main.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "RING_PLAN_OK" in run.stdout, run.stdout[-3000:] + run.stderr[-4000:]
    assert "runtime error" not in run.stderr and "ERROR: AddressSanitizer" not in run.stderr, run.stderr[-4000:]
