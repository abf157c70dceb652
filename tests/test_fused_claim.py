"""The owner words and the two-hop resolve of the fused claim (ipu_path_trace_amd/csrc/ptmi_share_plan.h: owner_class,
resolve_two_hops) and a sequential model of fused claim + resolve (pt_nif_group.h: ShareClassTable) on the CPU:
tests/fused_claim_main.cpp, built under AddressSanitizer and UndefinedBehaviorSanitizer and run.  The header includes nothing
from HIP, so g++ alone compiles the program."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "fused_claim_main.cpp")
INC = "-I" + os.path.join(ROOT, "ipu_path_trace_amd", "csrc")


def test_fused_claim_model_under_sanitizers(tmp_path):
    exe = str(tmp_path / "fused_claim_san")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-fno-omit-frame-pointer", INC, "-o", exe, SRC], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "FUSED_CLAIM_OK" in run.stdout, run.stdout[-3000:] + run.stderr[-4000:]
    assert "runtime error" not in run.stderr and "ERROR: AddressSanitizer" not in run.stderr, run.stderr[-4000:]
