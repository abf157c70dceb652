"""The trainer's precision mode (pt_nif_train_set_precision and its two companions): the C-ABI, the binding,
ipu_trace --train-precision under --compile-only and the host-side validation that needs no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import nif_train_model as M
from tests.test_nif_train_abi import write_pfm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ipu_path_trace_amd", "host")
SYMBOLS = ("pt_nif_train_default_precision", "pt_nif_train_set_precision", "pt_nif_train_get_precision_state")
INVALID = -1


def test_entry_points_are_exported_and_bound(ptmi_lib):
    lib = ptmi_lib.load_library()
    for sym in SYMBOLS:
        assert hasattr(lib, sym) and sym in ptmi_lib.EXPORTS
    for name in ("set_precision", "precision_state"):
        assert callable(getattr(ptmi_lib.NifTrainer, name))
    assert callable(ptmi_lib.default_nif_train_precision)
    import inspect
    assert "precision" in inspect.signature(ptmi_lib.Renderer.train_nif).parameters
    # additive: the ABI version and the pinned structs do not move
    assert lib.pt_abi_version() == 5 and C.sizeof(ptmi_lib.NifTrainParams) == 56
    assert C.sizeof(ptmi_lib.Config) == 56 and C.sizeof(ptmi_lib.Stats) == 80 and C.sizeof(ptmi_lib.Layer) == 32


def test_struct_sizes_equal_the_c_ones(ptmi_lib, tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ptmi.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu\\n", sizeof(pt_nif_train_precision), offsetof(pt_nif_train_precision, mode),\n'
                   '         offsetof(pt_nif_train_precision, loss_scale), offsetof(pt_nif_train_precision, dynamic),\n'
                   '         offsetof(pt_nif_train_precision, growth_interval));\n'
                   '  printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(pt_nif_train_precision_state), offsetof(pt_nif_train_precision_state, mode),\n'
                   '         offsetof(pt_nif_train_precision_state, loss_scale), offsetof(pt_nif_train_precision_state, good_steps),\n'
                   '         offsetof(pt_nif_train_precision_state, applied_steps), offsetof(pt_nif_train_precision_state, skipped_steps));\n'
                   '  printf("%zu %d %d %d\\n", sizeof(pt_nif_train_params), PTMI_ABI_VERSION, PT_NIF_TRAIN_F32, PT_NIF_TRAIN_MIXED_F16);\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    lines = [[int(x) for x in line.split()] for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()]
    P, S = ptmi_lib.NifTrainPrecision, ptmi_lib.NifTrainPrecisionState
    assert lines[0] == [C.sizeof(P), P.mode.offset, P.loss_scale.offset, P.dynamic.offset, P.growth_interval.offset] == [20, 4, 8, 12, 16]
    assert lines[1] == [C.sizeof(S), S.mode.offset, S.loss_scale.offset, S.good_steps.offset, S.applied_steps.offset, S.skipped_steps.offset] \
        == [32, 4, 8, 12, 16, 24]
    assert lines[2] == [56, 5, ptmi_lib.NIF_TRAIN_MODES["f32"], ptmi_lib.NIF_TRAIN_MODES["mixed"]] == [56, 5, 0, 1]


def test_defaults_need_no_device(ptmi_lib):
    lib = ptmi_lib.load_library()
    assert lib.pt_nif_train_default_precision(None) == INVALID
    p = ptmi_lib.NifTrainPrecision()
    assert lib.pt_nif_train_default_precision(C.byref(p)) == 0
    assert p.struct_size == C.sizeof(ptmi_lib.NifTrainPrecision) == 20
    assert p.as_dict() == dict(mode=0, loss_scale=65536.0, dynamic=1, growth_interval=2000)
    q = ptmi_lib.default_nif_train_precision(mode="mixed", loss_scale=1024.0, dynamic=0)
    assert q.as_dict() == dict(mode=1, loss_scale=1024.0, dynamic=0, growth_interval=2000)
    with pytest.raises(ValueError):
        ptmi_lib.default_nif_train_precision(scale=2.0)
    with pytest.raises(ValueError):
        ptmi_lib.default_nif_train_precision(mode="bf16")


def test_bad_fields_are_rejected_by_name_without_a_handle(ptmi_lib):
    lib = ptmi_lib.load_library()
    good = ptmi_lib.default_nif_train_precision

    def call(p):
        rc = lib.pt_nif_train_set_precision(None, C.byref(p) if p is not None else None)
        return rc, lib.pt_last_error(None).decode()

    assert call(good()) == (INVALID, "pt_nif_train_set_precision: null handle")
    assert call(good(mode="mixed")) == (INVALID, "pt_nif_train_set_precision: null handle")
    rc, msg = call(None)
    assert rc == INVALID and "null pt_nif_train_precision" in msg
    p = good()
    p.struct_size = 16
    rc, msg = call(p)
    assert rc == INVALID and "struct_size" in msg
    for field, value in (("mode", 2), ("mode", -1), ("loss_scale", 3.0), ("loss_scale", 0.5), ("loss_scale", 0.0), ("loss_scale", -1024.0),
                         ("loss_scale", 2.0 ** 31), ("loss_scale", float("nan")), ("loss_scale", float("inf")), ("dynamic", 2), ("dynamic", -1),
                         ("growth_interval", 0), ("growth_interval", 2 ** 31 + 1)):
        rc, msg = call(good(**{field: value}))
        assert rc == INVALID and field in msg, (field, value, msg)
    rc, msg = call(good(mode=3, loss_scale=3.0, dynamic=2, growth_interval=0))          # checked in field order
    assert rc == INVALID and "mode" in msg and "loss_scale" not in msg
    rc, msg = call(good(loss_scale=3.0, dynamic=2, growth_interval=0))
    assert rc == INVALID and "loss_scale" in msg and "dynamic" not in msg
    for value in (1.0, 2.0 ** 30):
        assert call(good(loss_scale=value))[1] == "pt_nif_train_set_precision: null handle"
    assert call(good(growth_interval=2 ** 31))[1] == "pt_nif_train_set_precision: null handle"
    assert lib.pt_nif_train_get_precision_state(None, None) == INVALID


def test_cli_compile_only_validates_the_precision(tmp_path):
    exe = os.path.join(HOST, "ipu_trace")
    good = tmp_path / "map.pfm"
    write_pfm(str(good), M.procedural_map(8, 16))
    base = [exe, "--train-nif", str(good), "--train-steps", "50", "--train-out", str(tmp_path / "out"), "--train-layer-size", "64",
            "--train-layer-count", "2", "--compile-only"]
    r = subprocess.run(base + ["--train-precision", "mixed", "--train-loss-scale", "1024", "--train-loss-scale-static"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "precision mixed" in r.stdout + r.stderr and not (tmp_path / "out").exists()
    r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0 and "precision f32" in r.stdout + r.stderr
    r = subprocess.run(base + ["--train-precision", "bf16"], capture_output=True, text=True)
    assert r.returncode != 0 and "--train-precision" in r.stdout + r.stderr and "bf16" in r.stdout + r.stderr
    for scale in ("3", "0", "nonsense", "4294967296"):
        r = subprocess.run(base + ["--train-precision", "mixed", "--train-loss-scale", scale], capture_output=True, text=True)
        assert r.returncode != 0 and "loss_scale" in r.stdout + r.stderr, scale


def test_the_validation_is_clean_under_the_sanitizers(tmp_path):
    """check_precision and the metadata writer's train_command, as a stand-alone program built with AddressSanitizer + UBSan."""
    exe = str(tmp_path / "nif_train_mixed_fuzz")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ipu_path_trace_amd", "csrc"), "-I" + HOST,
                           "-o", exe, os.path.join(ROOT, "tests", "nif_train_mixed_fuzz_main.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    cases, accepted, rejected, unnamed = [int(x) for x in r.stdout.strip().splitlines()[-1].split()[1::2]]
    assert cases > 30 and accepted > 0 and rejected > 0 and unnamed == 0


def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    for s in ("int pt_nif_train_default_precision(pt_nif_train_precision* p);",
              "int pt_nif_train_set_precision(pt_handle h, const pt_nif_train_precision* p);",
              "int pt_nif_train_get_precision_state(pt_handle h, pt_nif_train_precision_state* s);",
              "#define PT_NIF_TRAIN_F32        0", "#define PT_NIF_TRAIN_MIXED_F16  1", "#define PTMI_ABI_VERSION 5"):
        assert s in text, s
    assert "mixed-precision training is not part of it" not in text
