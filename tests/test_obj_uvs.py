"""The OBJ reader's path with texture coordinates (ipu_path_trace_amd/host/ObjReader.hpp: parse_with_uvs, --scene's "uvs": "file") as
the stand-alone program tests/obj_uvs_main.cpp under AddressSanitizer and UndefinedBehaviorSanitizer: `vt u [v [w]]` lines, the second
field of v/vt and v/vt/vn corners, negative indices, fans; its error messages, a face without a texture index among them; that
parse() and parse_with_normals() return on the same texts what they returned before; and a fuzz pass -- every truncation of a seed
file and 20000 corruptions of it -- in which every text either parses to in-range indices or is refused with a message, under all
three entries, and nothing crashes."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_obj_uvs_plain_and_fuzz_under_sanitizers(tmp_path):
    exe = str(tmp_path / "obj_uvs")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "ipu_path_trace_amd", "host"), "-o", exe,
                            os.path.join(ROOT, "tests", "obj_uvs_main.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "OBJ_UVS_OK" in run.stdout, run.stdout[-3000:] + run.stderr[-4000:]
    assert "runtime error" not in run.stderr and "ERROR: AddressSanitizer" not in run.stderr, run.stderr[-4000:]
