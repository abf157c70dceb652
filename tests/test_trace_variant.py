"""Which instance of the trace, trace-paths and feature kernels a launch takes (ipu_path_trace_amd/csrc/ptmi_trace_variant.h) on
the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer: over all 2^10 states, select, the template flags and the
occupancy pin derived from the variant equal the three ladders of hand-written kernel names they replaced (transcribed in
tests/trace_variant_main.cpp), the dense numbering round-trips and every instance is reached.  The header includes nothing from
HIP, so the stand-alone program compiles with g++ alone; the reference has no counterpart (its one kernel is compiled per scene)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_trace_variant_under_sanitizers(tmp_path):
    exe = str(tmp_path / "trace_variant")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "ipu_path_trace_amd", "csrc"), "-o", exe,
                            os.path.join(ROOT, "tests", "trace_variant_main.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "TRACE_VARIANT_OK 57 + 19 + 5 instances" in run.stdout, run.stdout[-3000:] + run.stderr[-4000:]
    assert "runtime error" not in run.stderr and "ERROR: AddressSanitizer" not in run.stderr, run.stderr[-4000:]
