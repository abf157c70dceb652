"""The integer arithmetic of a step (ipu_path_trace_amd/csrc/ptmi_step_plan.h) on the CPU, under AddressSanitizer and
UndefinedBehaviorSanitizer: how pt_path_trace deals a step's sample iterations into batches, the reciprocal the trace kernel
splits a path index with (item_divider: its comment carries the proof sketch, this the check) and the trace grid of a batch.
The header includes nothing from HIP, so the stand-alone program tests/step_plan_main.cpp compiles with g++ alone; the
reference has no counterpart (Poplar compiles its graph for a fixed batch)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_step_plan_under_sanitizers(tmp_path):
    exe = str(tmp_path / "step_plan")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "ipu_path_trace_amd", "csrc"), "-o", exe,
                            os.path.join(ROOT, "tests", "step_plan_main.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "STEP_PLAN_OK" in run.stdout, run.stdout[-3000:] + run.stderr[-4000:]
    assert "runtime error" not in run.stderr and "ERROR: AddressSanitizer" not in run.stderr, run.stderr[-4000:]
