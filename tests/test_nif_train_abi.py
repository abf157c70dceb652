"""The NIF trainer (pt_nif_train_*): the C-ABI, the binding, ipu_trace --train-nif --compile-only and the host-side checks that
need no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import nif_train_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ipu_path_trace_amd", "host")
SYMBOLS = ("pt_nif_train_default_params", "pt_nif_train_begin", "pt_nif_train_layer_shapes", "pt_nif_train_steps",
           "pt_nif_train_get_weights", "pt_nif_train_set_weights", "pt_nif_train_get_encode_params", "pt_nif_train_export",
           "pt_nif_train_install", "pt_nif_train_end", "pt_nif_train_batch", "pt_nif_train_gradients")
INVALID = -1


def write_pfm(path, bgr):
    """A little-endian three-channel .pfm (R, G, B; rows bottom to top) of a B, G, R image."""
    h, w, _ = bgr.shape
    with open(path, "wb") as f:
        f.write(b"PF\n%d %d\n-1.0\n" % (w, h))
        f.write(np.ascontiguousarray(bgr[::-1, :, ::-1], dtype="<f4").tobytes())


def test_entry_points_are_exported_and_bound(ptmi_lib):
    lib = ptmi_lib.load_library()
    for sym in SYMBOLS:
        assert hasattr(lib, sym) and sym in ptmi_lib.EXPORTS
    assert callable(ptmi_lib.Renderer.train_nif)
    for name in ("steps", "loss", "weights", "set_weights", "encode_params", "export", "install", "batch", "gradients", "close"):
        assert callable(getattr(ptmi_lib.NifTrainer, name))
    # additive: the ABI version and the pinned structs do not move
    assert lib.pt_abi_version() == 5 and C.sizeof(ptmi_lib.Config) == 56 and C.sizeof(ptmi_lib.Stats) == 80 and C.sizeof(ptmi_lib.Layer) == 32


def test_struct_size_equals_the_c_one(ptmi_lib, tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ptmi.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu\\n", sizeof(pt_nif_train_params), offsetof(pt_nif_train_params, batch),\n'
                   '         offsetof(pt_nif_train_params, adam_eps), offsetof(pt_nif_train_params, seed), offsetof(pt_nif_train_params, eps));\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P = ptmi_lib.NifTrainParams
    assert got == [C.sizeof(P), P.batch.offset, P.adam_eps.offset, P.seed.offset, P.eps.offset] == [56, 16, 32, 40, 52]


def test_defaults_need_no_device(ptmi_lib):
    lib = ptmi_lib.load_library()
    assert lib.pt_nif_train_default_params(None) == INVALID
    p = ptmi_lib.NifTrainParams()
    assert lib.pt_nif_train_default_params(C.byref(p)) == 0
    f32 = lambda x: float(np.float32(x))   # noqa: E731
    # the reference's train_command (embedding 12, 6 x 320, log tone map, eps 1e-8), batch 65536, Keras's Adam constants
    assert p.struct_size == C.sizeof(ptmi_lib.NifTrainParams)
    assert p.as_dict() == dict(embedding_dim=12, hidden=320, layer_count=6, batch=65536, learning_rate=f32(1e-3), beta1=f32(0.9),
                               beta2=f32(0.999), adam_eps=f32(1e-7), seed=1, log_tone_map=1, eps=f32(1e-8))
    assert ptmi_lib.default_nif_train_params(hidden=64).hidden == 64
    with pytest.raises(ValueError):
        ptmi_lib.default_nif_train_params(width=64)


def test_bad_parameters_are_rejected_by_name(ptmi_lib):
    lib = ptmi_lib.load_library()
    good = ptmi_lib.default_nif_train_params

    def call(p):
        rc = lib.pt_nif_train_begin(None, C.byref(p) if p is not None else None)
        return rc, lib.pt_last_error(None).decode()

    assert call(good()) == (INVALID, "pt_nif_train_begin: null handle")
    assert call(None)[0] == INVALID
    p = good()
    p.struct_size = 52
    rc, msg = call(p)
    assert rc == INVALID and "struct_size" in msg
    for field, value in (("hidden", 48), ("hidden", 2048), ("batch", 100), ("embedding_dim", 0), ("layer_count", 0),
                         ("learning_rate", float("nan")), ("learning_rate", float("inf")), ("embedding_dim", 17), ("embedding_dim", 16), ("layer_count", 16),
                         ("hidden", 0), ("batch", 0), ("beta1", 1.0), ("beta2", -0.1), ("adam_eps", 0.0), ("log_tone_map", 2),
                         ("eps", float("nan"))):
        rc, msg = call(good(**{field: value}))
        assert rc == INVALID and field in msg, (field, value, msg)
    for fn in ("pt_nif_train_steps", "pt_nif_train_install", "pt_nif_train_end"):
        assert getattr(lib, fn)(None, *([0, None] if fn == "pt_nif_train_steps" else [])) == INVALID


def test_cli_compile_only_validates_arguments_and_file(tmp_path):
    exe = os.path.join(HOST, "ipu_trace")
    good = tmp_path / "map.pfm"
    write_pfm(str(good), M.procedural_map(8, 16))
    cut = tmp_path / "cut.pfm"
    cut.write_bytes(good.read_bytes()[:300])
    base = ["--train-steps", "50", "--train-out", str(tmp_path / "out"), "--train-layer-size", "64", "--train-layer-count", "2", "--compile-only"]
    r = subprocess.run([exe, "--train-nif", str(good)] + base, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "16 x 8" in r.stdout + r.stderr and not (tmp_path / "out").exists()
    r = subprocess.run([exe, "--train-nif", str(cut)] + base, capture_output=True, text=True)
    assert r.returncode != 0 and str(cut) in r.stdout + r.stderr and "truncated" in r.stdout + r.stderr
    r = subprocess.run([exe, "--train-nif", str(good)] + base + ["--train-batch", "100"], capture_output=True, text=True)
    assert r.returncode != 0 and "batch" in r.stdout + r.stderr
    r = subprocess.run([exe, "--train-nif", str(good), "--compile-only"], capture_output=True, text=True)
    assert r.returncode != 0 and "--train-out" in r.stdout + r.stderr


def test_write_metadata_takes_the_trainers_values(tmp_path):
    from ipu_path_trace_amd import nif_assets
    meta = {"embedding_dimension": 4, "hidden_size": 64, "layer_count": 2, "eps": float(np.float32(1e-8)), "log_tone_map": True,
            "max": np.float32(1.75), "mean": [np.float32(-0.5), np.float32(-0.25), np.float32(0.125)], "original_image_shape": [8, 16, 3]}
    nif_assets.write_metadata(str(tmp_path / "m.txt"), meta, name="map.pfm")
    got = nif_assets.load_metadata(str(tmp_path / "m.txt"))
    assert got["name"] == "map.pfm" and got["hidden_size"] == 64 and got["layer_count"] == 2 and got["embedding_dimension"] == 4
    assert got["max"] == 1.75 and got["mean_folded"] == [float(np.float32(np.float32(m) - np.float32(1e-8))) for m in meta["mean"]]
    nif_assets.write_metadata(str(tmp_path / "d.txt"))                                  # the existing signature and defaults
    assert nif_assets.load_metadata(str(tmp_path / "d.txt"))["name"] == "synthetic"


def test_host_code_is_clean_under_the_sanitizers(tmp_path):
    """Parameter validation and the .ptnif / metadata writers, as a stand-alone program built with AddressSanitizer + UBSan."""
    exe = str(tmp_path / "nif_train_fuzz")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ipu_path_trace_amd", "csrc"), "-I" + HOST,
                           "-o", exe, os.path.join(ROOT, "tests", "nif_train_fuzz_main.cpp")])
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:allocator_may_return_null=1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    cases, accepted, rejected, unnamed, refused = [int(x) for x in r.stdout.strip().splitlines()[-1].split()[1::2]]
    assert cases > 50 and accepted > 0 and rejected > 0 and unnamed == 0 and refused == 6


def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    for s in ("int pt_nif_train_default_params(pt_nif_train_params* p);", "int pt_nif_train_begin(pt_handle h, const pt_nif_train_params* p);",
              "int pt_nif_train_install(pt_handle h);", "int pt_nif_train_steps(pt_handle h, uint32_t n, float* last_loss);",
              "#define PTMI_ABI_VERSION 5"):
        assert s in text, s
