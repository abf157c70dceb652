"""The environment guide built from the environment in force (pt_set_env_guide_from_environment): the C-ABI, the order of its
validation, check_auto's agreement with it, the binding and the CLI's refusal -- everything that needs no device."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ipu_path_trace_amd", "csrc")
HOST = os.path.join(ROOT, "ipu_path_trace_amd", "host")
SYMBOLS = ("pt_set_env_guide_from_environment", "pt_get_env_guide_info", "pt_get_env_guide_tables")
INVALID = -1
GOOD = dict(rows=8, cols=16, supersample=2, alpha=0.5, follow=1)
# one bad value per field, in the order the header states; each request also carries every LATER bad field, so the message
# shows which check came first
BAD = (("struct_size", 20), ("rows", 3), ("cols", 4096), ("supersample", 3), ("alpha", 0.95), ("follow", 2))


def _auto(ptmi_lib, **fields):
    v = dict(GOOD, struct_size=C.sizeof(ptmi_lib.EnvGuideAuto))
    v.update(fields)
    return ptmi_lib.EnvGuideAuto(v["struct_size"], v["rows"], v["cols"], v["supersample"], v["alpha"], v["follow"])


@pytest.fixture(scope="module")
def check_auto(tmp_path_factory):
    """ptguide::check_auto through the stand-alone program: fields -> message ("" = accepted)."""
    exe = str(tmp_path_factory.mktemp("env_guide_auto") / "env_guide_masses_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "env_guide_masses_main.cpp")])

    def run(a):
        args = ["null"] if a is None else [str(x) for x in (a.struct_size, a.rows, a.cols, a.supersample, repr(float(a.alpha)), a.follow)]
        return subprocess.run([exe, "auto"] + args, capture_output=True, text=True, check=True).stdout.rstrip("\n")
    return run


def test_entry_points_are_exported_and_bound(ptmi_lib):
    lib = ptmi_lib.load_library()
    for sym in SYMBOLS:
        assert hasattr(lib, sym) and sym in ptmi_lib.EXPORTS
    for name in ("set_env_guide_from_environment", "env_guide_info", "env_guide_tables"):
        assert callable(getattr(ptmi_lib.Renderer, name))
    # additive: the ABI version and the pinned structs do not move
    assert lib.pt_abi_version() == 5 and C.sizeof(ptmi_lib.Config) == 56 and C.sizeof(ptmi_lib.Stats) == 80
    assert C.sizeof(ptmi_lib.EnvGuide) == 32


def test_struct_sizes_equal_the_c_ones(ptmi_lib, tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ptmi.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(pt_env_guide_auto), offsetof(pt_env_guide_auto, supersample),\n'
                   '         offsetof(pt_env_guide_auto, follow), sizeof(pt_env_guide_info), offsetof(pt_env_guide_info, alpha),\n'
                   '         offsetof(pt_env_guide_info, stale), offsetof(pt_env_guide_info, rebuilds), offsetof(pt_env_guide_info, build_ms));\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    A, I = ptmi_lib.EnvGuideAuto, ptmi_lib.EnvGuideInfo
    assert got == [C.sizeof(A), A.supersample.offset, A.follow.offset, C.sizeof(I), I.alpha.offset, I.stale.offset, I.rebuilds.offset,
                   I.build_ms.offset] == [24, 12, 20, 64, 24, 32, 40, 56]


def test_bad_fields_are_rejected_by_name_in_the_stated_order(ptmi_lib, check_auto):
    lib = ptmi_lib.load_library()

    def call(a):
        rc = lib.pt_set_env_guide_from_environment(None, C.byref(a) if a is not None else None)
        return rc, lib.pt_last_error(None).decode()

    # 1. a NULL struct comes before everything
    rc, msg = call(None)
    assert rc == INVALID and "null" in msg and msg == check_auto(None)
    # 2..7: with every later field bad as well, the message names the first bad one
    for i, (field, value) in enumerate(BAD):
        a = _auto(ptmi_lib, **dict(BAD[i:]))
        rc, msg = call(a)
        assert rc == INVALID and field in msg, (field, msg)
        for later, _ in BAD[i + 1:]:
            assert later not in msg, (field, later, msg)
        assert msg == check_auto(a)
        # ... and alone
        rc, alone = call(_auto(ptmi_lib, **{field: value}))
        assert rc == INVALID and field in alone and alone == check_auto(_auto(ptmi_lib, **{field: value}))
    for field, value in (("rows", 0), ("rows", 2048), ("cols", 0), ("cols", 48), ("supersample", 0), ("supersample", 8),
                         ("alpha", -0.1), ("alpha", float("nan")), ("alpha", float("inf")), ("follow", -1)):
        a = _auto(ptmi_lib, **{field: value})
        rc, msg = call(a)
        assert rc == INVALID and field in msg and msg == check_auto(a), (field, value, msg)
    # 8. only then the NULL handle; the caps and alpha's ends themselves are accepted
    for ok in (_auto(ptmi_lib), _auto(ptmi_lib, rows=1024, cols=2048, supersample=4, alpha=0.9, follow=0),
               _auto(ptmi_lib, rows=1, cols=1, supersample=1, alpha=0.0)):
        assert check_auto(ok) == ""
        assert call(ok) == (INVALID, "pt_set_env_guide_from_environment: null handle")
    info = ptmi_lib.EnvGuideInfo()
    info.struct_size = C.sizeof(info)
    assert lib.pt_get_env_guide_info(None, C.byref(info)) == INVALID
    assert lib.pt_get_env_guide_tables(None, None, None, None, 0) == INVALID


def test_header_declares_the_entry_points_and_the_contract():
    text = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    for s in ("int pt_set_env_guide_from_environment(pt_handle h, const pt_env_guide_auto* a);",
              "int pt_get_env_guide_info(pt_handle h, pt_env_guide_info* out);",
              "int pt_get_env_guide_tables(pt_handle h, uint32_t* threshold, uint32_t* alias, float* q, size_t n);",
              "x' = x >= 0 ? fminf(x, FLT_MAX) : 0", "BIT FOR BIT", "#define PTMI_ABI_VERSION 5"):
        assert s in text, s


def test_cli_refuses_bad_values_and_a_missing_environment_before_a_device(tmp_path):
    from ipu_path_trace_amd import nif_assets
    exe = os.path.join(HOST, "ipu_trace")
    if not os.path.exists(exe):
        pytest.fail("ipu_trace has not been built (__graft_entry__.build)")
    assets = tmp_path / "assets.extra"
    assets.mkdir()
    nif_assets.write_metadata(str(assets / "nif_metadata.txt"))
    nif_assets.write_ptnif(str(assets / "converted.ptnif"), nif_assets.synthetic_nif(), 12)
    base = [exe, "--outfile", str(tmp_path / "o.png"), "--env-guide", "env", "--compile-only"]
    r = subprocess.run(base + ["--assets", str(assets)], capture_output=True, text=True)
    assert r.returncode == 0 and "256 x 512 cells, 2 x 2 lookups per cell" in r.stdout + r.stderr, r.stdout + r.stderr
    r = subprocess.run(base + ["--assets", str(assets), "--env-guide-supersample", "3"], capture_output=True, text=True)
    assert r.returncode != 0 and "supersample must be 1, 2 or 4 (got 3)" in r.stdout + r.stderr
    r = subprocess.run(base + ["--assets", str(assets), "--env-guide-size", "48x64"], capture_output=True, text=True)
    assert r.returncode != 0 and "rows must be a power of two" in r.stdout + r.stderr
    # no environment option at all: the library's own words, and no --assets complaint
    r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode != 0 and "no environment has been set (none of pt_upload_nif, pt_set_env_map, pt_set_constant_env" in r.stdout + r.stderr
