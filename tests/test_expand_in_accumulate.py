"""Expand inside the accumulate pass of a mapped step (ipu_path_trace_amd/csrc/ptmi_share_plan.h: kNoQueueSlot, mapped_row) on
the CPU: tests/expand_in_accumulate_main.cpp, built under AddressSanitizer and UndefinedBehaviorSanitizer and run -- a sequential
model of "inverse slot map + expand while accumulating" against expand-then-accumulate over generated batches with emitters, dead
paths, padding items and pending class words.  The header includes nothing from HIP, so g++ alone compiles the program."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "expand_in_accumulate_main.cpp")
INC = "-I" + os.path.join(ROOT, "ipu_path_trace_amd", "csrc")


def test_expand_in_accumulate_model_under_sanitizers(tmp_path):
    exe = str(tmp_path / "expand_in_accumulate_san")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", INC, "-o", exe, SRC], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "EXPAND_IN_ACCUMULATE_OK" in run.stdout, run.stdout[-3000:] + run.stderr[-4000:]
    assert "runtime error" not in run.stderr and "ERROR: AddressSanitizer" not in run.stderr, run.stderr[-4000:]
