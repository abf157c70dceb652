"""The arithmetic of NIF sharing and the memo (ipu_path_trace_amd/csrc/ptmi_share_plan.h) on the CPU, under AddressSanitizer and
UndefinedBehaviorSanitizer: the worst-case table of a batch or a step (powers of two, monotone in the entries and in the free
memory, entry counts of 0, 1 and 2^31 - 1), the memory budget under which the automatic default declines, the owner word of
both tables (round trips, the three kinds exclusive, its limits) and the slots of a memo of a given size.  The header
includes nothing from HIP, so the stand-alone program tests/share_plan_main.cpp compiles with g++ alone."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_share_plan_under_sanitizers(tmp_path):
    exe = str(tmp_path / "share_plan")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "ipu_path_trace_amd", "csrc"), "-o", exe,
                            os.path.join(ROOT, "tests", "share_plan_main.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "SHARE_PLAN_OK" in run.stdout, run.stdout[-3000:] + run.stderr[-4000:]
    assert "runtime error" not in run.stderr and "ERROR: AddressSanitizer" not in run.stderr, run.stderr[-4000:]
