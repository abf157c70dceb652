"""The split of csrc/ptmi_env_guide.h into the mass loop and build_from_masses, on the CPU: a stand-alone program
(tests/env_guide_masses_main.cpp) built with AddressSanitizer + UBSan; nothing is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ipu_path_trace_amd", "csrc")


def test_build_from_masses_equals_build_under_the_sanitizers(tmp_path):
    """build_from_masses over masses summed by hand equals build() entry for entry (threshold, alias, q, P, ideal, alpha) for
    sun_map, a random 24 x 40 image and a sun on black, on the grids 8 x 16 and 1 x 2; a cell without mass ends with threshold 0
    and no alias pointing at it; no mass at all is refused naming the total."""
    exe = str(tmp_path / "env_guide_masses_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "env_guide_masses_main.cpp")])
    r = subprocess.run([exe, "check"], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.strip().splitlines()[-1] == "ok 18"
