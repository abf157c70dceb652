"""The tiles of the claim pass (ipu_path_trace_amd/csrc/ptmi_share_plan.h) on the CPU, under AddressSanitizer and
UndefinedBehaviorSanitizer: how many tiles a region gets, which entries a (workgroup, thread, k) takes -- every entry below
the region's count exactly once, none at or above it, for counts around 256 and around the tile and capacities that are no
multiple of the tile -- that an idle workgroup is recognised by a test uniform over it, and that the waves' offsets inside
a tile's reservation are the exclusive scan of their append counts.  Plain C++: tests/claim_plan_main.cpp compiles with g++."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_claim_plan_under_sanitizers(tmp_path):
    exe = str(tmp_path / "claim_plan")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "ipu_path_trace_amd", "csrc"), "-o", exe,
                            os.path.join(ROOT, "tests", "claim_plan_main.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "CLAIM_PLAN_OK" in run.stdout, run.stdout[-3000:] + run.stderr[-4000:]
    assert "runtime error" not in run.stderr and "ERROR: AddressSanitizer" not in run.stderr, run.stderr[-4000:]
