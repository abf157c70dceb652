"""The clean-table hand-off (ipu_path_trace_amd/csrc/ptmi_share_plan.h) on the CPU, under AddressSanitizer and
UndefinedBehaviorSanitizer: the clean mark against a model of the table over every sequence of three steps drawn from step
scope, batch scope, the memo, sharing off, a failed step and a resized table (behind every history of one step) -- a
step-scope step never starts on a table that holds a key, and the mark never says more than is true.  (The early / late
predicate of a split expand pass is not checked: the split was measured slower and is not in the tree, DESIGN.md section
4.5.)  Plain C++: tests/handoff_plan_main.cpp compiles with g++."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_handoff_plan_under_sanitizers(tmp_path):
    exe = str(tmp_path / "handoff_plan")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "ipu_path_trace_amd", "csrc"), "-o", exe,
                            os.path.join(ROOT, "tests", "handoff_plan_main.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "HANDOFF_PLAN_OK" in run.stdout, run.stdout[-3000:] + run.stderr[-4000:]
    assert "runtime error" not in run.stderr and "ERROR: AddressSanitizer" not in run.stderr, run.stderr[-4000:]
