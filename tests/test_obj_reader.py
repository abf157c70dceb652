"""The OBJ reader of --scene meshes (ipu_path_trace_amd/host/ObjReader.hpp) as the stand-alone program tests/obj_reader_main.cpp
under AddressSanitizer and UndefinedBehaviorSanitizer: the face forms v, v/vt, v//vn, v/vt/vn, negative indices, quads and n-gons
triangulated as fans, CR LF; its error messages; and a fuzz pass -- every truncation of a seed file and 20000 corruptions of it --
in which every text either parses to in-range indices or is refused with a message, and nothing crashes."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_obj_reader_plain_and_fuzz_under_sanitizers(tmp_path):
    exe = str(tmp_path / "obj_reader")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "ipu_path_trace_amd", "host"), "-o", exe,
                            os.path.join(ROOT, "tests", "obj_reader_main.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "OBJ_READER_OK" in run.stdout, run.stdout[-3000:] + run.stderr[-4000:]
    assert "runtime error" not in run.stderr and "ERROR: AddressSanitizer" not in run.stderr, run.stderr[-4000:]
