"""Persistent memo of NIF evaluations across steps (pt_set_nif_memo): the C-ABI, the binding and the CLI surface, without a GPU."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ipu_path_trace_amd", "host")
SYMBOLS = ("pt_set_nif_memo", "pt_clear_nif_memo", "pt_get_nif_memo_stats")


def test_memo_entry_points_are_exported_and_bound(ptmi_lib):
    lib = ptmi_lib.load_library()
    for sym in SYMBOLS:
        assert hasattr(lib, sym) and sym in ptmi_lib.EXPORTS
    S = ptmi_lib.NifMemoStats
    assert C.sizeof(S) == 88
    assert [(n, S.__dict__[n].offset) for n, _ in S._fields_] == [
        ("struct_size", 0), ("enabled", 4), ("slots", 8), ("occupied", 16), ("escaped", 24), ("served", 32),
        ("evaluations", 40), ("inserted", 48), ("overflowed", 56), ("generation", 64), ("retains", 72), ("memo_ms", 80)]
    for name in ("set_nif_memo", "clear_nif_memo", "nif_memo_stats"):
        assert callable(getattr(ptmi_lib.Renderer, name))
    # additive: the ABI version and the pinned structs (the sharing stats included) do not move
    assert lib.pt_abi_version() == 5 and C.sizeof(ptmi_lib.Config) == 56 and C.sizeof(ptmi_lib.Stats) == 80
    assert C.sizeof(ptmi_lib.NifSharingStats) == 48


def test_null_handle_is_an_invalid_argument(ptmi_lib):
    lib = ptmi_lib.load_library()
    assert lib.pt_set_nif_memo(None, 0) == -1
    assert lib.pt_set_nif_memo(None, 2 << 30) == -1
    assert lib.pt_clear_nif_memo(None) == -1
    st = ptmi_lib.NifMemoStats()
    st.struct_size = C.sizeof(st)
    assert lib.pt_get_nif_memo_stats(None, C.byref(st)) == -1


def test_header_states_the_memo_contract():
    text = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    for s in ("int pt_set_nif_memo(pt_handle h, uint64_t max_bytes);", "int pt_clear_nif_memo(pt_handle h);",
              "typedef struct pt_nif_memo_stats", "int pt_get_nif_memo_stats(pt_handle h, pt_nif_memo_stats* out);",
              "#define PTMI_ABI_VERSION 5"):
        assert s in text, s
    memo = text[text.index("Persistent memo of NIF evaluations"):text.index("int pt_get_nif_memo_stats")]
    flat = " ".join(memo.replace("*", " ").split())
    for s in ("bit-identical to memo off", "every kernel family", "any capacity", "Independent of the sharing mode",
              "evaluations == escaped holds only when both sharing and the memo are off", "pt_upload_nif",
              "a pt_path_trace that fails", "new generation", "Nothing else invalidates the memo", "pt_set_render_settings",
              "pt_setup", "pt_set_constant_env", "no memo pass runs", "PT_ERR_OUT_OF_MEMORY", "left off", "2^30 slots"):
        assert s in flat, s
    assert "pt_diag_set_nif_memo_slots" not in text


def test_diag_slot_hook_lives_only_in_the_diag_library(ptmi_lib):
    product = ptmi_lib.load_library()
    diag = ptmi_lib.load_library(diag=True)
    assert not hasattr(product, "pt_diag_set_nif_memo_slots")
    assert hasattr(diag, "pt_diag_set_nif_memo_slots")
    assert diag.pt_diag_set_nif_memo_slots(None, 64) == -1
    assert b"pt_diag_set_nif_memo_slots" not in open(product._name, "rb").read()


def _exe():
    exe = os.path.join(HOST, "ipu_trace")
    if not os.path.exists(exe):
        pytest.fail("ipu_trace has not been built (__graft_entry__.build)")
    return exe


def test_cli_lists_and_validates_nif_memo_gib(tmp_path):
    exe = _exe()
    help_text = subprocess.run([exe, "--help"], capture_output=True, text=True).stdout
    assert "--nif-memo-gib" in help_text
    base = [exe, "-o", str(tmp_path / "x.png"), "--assets", str(tmp_path), "--constant-env", "1,1,1"]
    for bad in ("two", "-1", "2GiB", "nan", "inf", ""):
        r = subprocess.run(base + ["--nif-memo-gib", bad], capture_output=True, text=True)
        assert r.returncode == 1 and "--nif-memo-gib" in r.stdout, (bad, r.returncode, r.stdout[-500:])
        assert "Could not attach" not in r.stdout
    for good in ("0", "2", "0.5"):
        r = subprocess.run(base + ["--nif-memo-gib", good, "--compile-only"], capture_output=True, text=True)
        assert r.returncode == 0 and "Compile only mode selected: finished." in r.stdout, (good, r.stdout[-500:])
    assert not (tmp_path / "x.png").exists()
