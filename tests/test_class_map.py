"""The class map of a mapped step (ipu_path_trace_amd/csrc/ptmi_share_plan.h: class_axis_index, class_map_index,
map_clear_skippable, map_mark_after_step) on the CPU: tests/class_map_main.cpp, built under AddressSanitizer and
UndefinedBehaviorSanitizer and run -- the axis index over every float coordinate of [0, 2], the pair index, a sequential model
of the class claim, the expand pass's hop and the release, and the mark rule over every sequence of step kinds.  The header
includes nothing from HIP, so g++ alone compiles the program."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "class_map_main.cpp")
INC = "-I" + os.path.join(ROOT, "ipu_path_trace_amd", "csrc")


def test_class_map_under_sanitizers(tmp_path):
    exe = str(tmp_path / "class_map_san")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-fno-omit-frame-pointer", INC, "-o", exe, SRC], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "CLASS_MAP_OK" in run.stdout, run.stdout[-3000:] + run.stderr[-4000:]
    assert "swept 1073741825 coordinates" in run.stdout, run.stdout[-3000:]
    assert "runtime error" not in run.stderr and "ERROR: AddressSanitizer" not in run.stderr, run.stderr[-4000:]
