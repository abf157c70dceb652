"""The key and the sizing rule of the NIF stage's class level (ipu_path_trace_amd/csrc/ptmi_share_plan.h: class_coord, class_key,
class_slots, class_fits) on the CPU.  tests/class_key_main.cpp is built twice: plain, for the sweep of every float coordinate
of [0, 2] (equal class_coord implies equal encoder inputs a_j for all j < 16, as bits), and under AddressSanitizer and
UndefinedBehaviorSanitizer, for the rounding boundaries, the ends of the range, what lies outside it, every 257th float and the
corner cases of the sizing rule.  The header includes nothing from HIP, so g++ alone compiles the program."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "class_key_main.cpp")
INC = "-I" + os.path.join(ROOT, "ipu_path_trace_amd", "csrc")


def _run(exe, *args):
    run = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "CLASS_KEY_OK" in run.stdout, run.stdout[-3000:] + run.stderr[-4000:]
    return run


def test_class_key_full_sweep(tmp_path):
    exe = str(tmp_path / "class_key")
    build = subprocess.run(["g++", "-std=c++17", "-O2", "-pthread", INC, "-o", exe, SRC], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = _run(exe, "--full")
    assert "swept 1073741825 coordinates" in run.stdout, run.stdout[-3000:]


def test_class_key_under_sanitizers(tmp_path):
    exe = str(tmp_path / "class_key_san")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-fno-omit-frame-pointer", INC, "-o", exe, SRC], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = _run(exe)
    assert "runtime error" not in run.stderr and "ERROR: AddressSanitizer" not in run.stderr, run.stderr[-4000:]
