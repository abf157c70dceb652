"""First-hit feature buffers and the film denoiser (pt_feature_buffers / pt_denoise / pt_denoise_default_params): the C-ABI, the
binding and the checks that need no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pt_feature_buffers", "pt_denoise", "pt_denoise_default_params")
INVALID = -1


def test_entry_points_are_exported_and_bound(ptmi_lib):
    lib = ptmi_lib.load_library()
    for sym in SYMBOLS:
        assert hasattr(lib, sym) and sym in ptmi_lib.EXPORTS
    for name in ("feature_buffers", "denoise"):
        assert callable(getattr(ptmi_lib.Renderer, name))
    # additive: the ABI version and the pinned structs do not move
    assert lib.pt_abi_version() == 5 and C.sizeof(ptmi_lib.Config) == 56 and C.sizeof(ptmi_lib.Stats) == 80
    assert C.sizeof(ptmi_lib.Camera) == 48 and ptmi_lib.SCENE_DTYPE.itemsize == 48


def test_struct_sizes_equal_the_c_ones(ptmi_lib, tmp_path):
    """sizeof and offsetof as a C compiler sees include/ptmi.h against the ctypes structs."""
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ptmi.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(pt_features), offsetof(pt_features, object_id), offsetof(pt_features, albedo),\n'
                   '         sizeof(pt_denoise_params), offsetof(pt_denoise_params, sigma_depth), offsetof(pt_denoise_params, demodulate));\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    F, D = ptmi_lib.Features, ptmi_lib.DenoiseParams
    assert got == [C.sizeof(F), F.object_id.offset, F.albedo.offset, C.sizeof(D), D.sigma_depth.offset, D.demodulate.offset]
    assert got == [40, 8, 32, 28, 16, 24]


def test_defaults_are_as_documented(ptmi_lib):
    lib = ptmi_lib.load_library()
    assert lib.pt_denoise_default_params(None) == INVALID
    p = ptmi_lib.DenoiseParams()
    assert lib.pt_denoise_default_params(C.byref(p)) == 0
    assert p.struct_size == C.sizeof(ptmi_lib.DenoiseParams)
    assert p.as_dict() == dict(iterations=5, sigma_colour=4.0, sigma_normal=0.5, sigma_depth=np.float32(0.1), object_stop=1,
                               demodulate=1)
    assert ptmi_lib.default_denoise_params(iterations=3, demodulate=0).as_dict()["iterations"] == 3
    with pytest.raises(ValueError):
        ptmi_lib.default_denoise_params(sigma_color=1.0)
    assert (ptmi_lib.DENOISE_HOST_IMAGE, ptmi_lib.DENOISE_ACCUMULATORS, ptmi_lib.DENOISE_FILM) == (0, 1, 2)


def test_null_handle_and_bad_parameters_name_the_field(ptmi_lib):
    """The checks that need no device run first, so they are reachable here: with no handle the message is
    pt_last_error(NULL)'s."""
    lib = ptmi_lib.load_library()
    img = np.zeros((4, 4, 3), np.float32)
    out = np.zeros_like(img)

    def call(p, source=0, inp=img, outp=out):
        rc = lib.pt_denoise(None, C.byref(p) if p is not None else None, source, inp.ctypes.data if inp is not None else None,
                            outp.ctypes.data if outp is not None else None)
        return rc, lib.pt_last_error(None).decode()

    good = ptmi_lib.default_denoise_params
    assert call(good()) == (INVALID, "pt_denoise: null handle")
    assert call(None) == (INVALID, "pt_denoise: null handle")                    # NULL params are the defaults
    for it in (0, 7, 9):
        rc, msg = call(good(iterations=it))
        assert rc == INVALID and "iterations" in msg and "1..6" in msg
    for field in ("sigma_colour", "sigma_normal", "sigma_depth"):
        for bad in (float("nan"), float("inf"), float("-inf")):
            rc, msg = call(good(**{field: bad}))
            assert rc == INVALID and field in msg and "finite" in msg, (field, bad, msg)
        assert call(good(**{field: 0.0}))[1] == "pt_denoise: null handle"        # <= 0 disables a stop: valid
        assert call(good(**{field: -1.0}))[1] == "pt_denoise: null handle"
    for source in (-1, 3):
        rc, msg = call(good(), source=source)
        assert rc == INVALID and "source" in msg
    rc, msg = call(good(), outp=None)
    assert rc == INVALID and "host_bgr_out" in msg
    rc, msg = call(good(), inp=None)
    assert rc == INVALID and "host_bgr_in" in msg
    assert call(good(), source=2, inp=None)[1] == "pt_denoise: null handle"      # the device sources take no input image
    p = good()
    p.struct_size = 24
    rc, msg = call(p)
    assert rc == INVALID and "struct_size" in msg
    f = ptmi_lib.Features()
    f.struct_size = C.sizeof(ptmi_lib.Features)
    assert lib.pt_feature_buffers(None, C.byref(f)) == INVALID and lib.pt_feature_buffers(None, None) == INVALID


def test_header_states_the_definitions():
    text = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    for s in ("int pt_feature_buffers(pt_handle h, pt_features* out);", "int pt_denoise_default_params(pt_denoise_params* p);",
              "enum { PT_DENOISE_HOST_IMAGE = 0, PT_DENOISE_ACCUMULATORS = 1, PT_DENOISE_FILM = 2 };", "#define PTMI_ABI_VERSION 5"):
        assert s in text, s
    flat = " ".join(text[text.index("First-hit feature buffers"):text.index("Multi-GPU film hand-off")].replace("*", " ").split())
    for s in ("EXTENSION", "zero AA noise and no lens", "ignored on purpose", "-1 for a miss", "WORLD space", "B, G, R",
              "pt_set_scene, pt_set_camera and pt_set_render_settings", "k = (3/8, 1/4, 1/16)", "sigma_colour 2^-i",
              "max(d[p], 1e-6)", "max(albedo[p], 1e-3)", "a hard zero", "not computed through exp", ">= 9/64", "convex combination",
              "no clamping, no wrap", "Non-finite input colours are not validated and propagate", "1 / film_steps",
              "before anything touches a device", "PT_ERR_NOT_READY", "PT_ERR_OUT_OF_MEMORY"):
        assert s in flat, s
