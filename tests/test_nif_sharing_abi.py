"""Exact sharing of NIF evaluations (pt_set_nif_sharing): the C-ABI, the binding and the CLI surface, without a GPU."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ipu_path_trace_amd", "host")


def test_sharing_entry_points_are_exported_and_bound(ptmi_lib):
    lib = ptmi_lib.load_library()
    for sym in ("pt_set_nif_sharing", "pt_get_nif_sharing_stats"):
        assert hasattr(lib, sym) and sym in ptmi_lib.EXPORTS
    assert ptmi_lib.NIF_SHARE_OFF == 0 and ptmi_lib.NIF_SHARE_BATCH == 1 and ptmi_lib.NIF_SHARE_STEP == 2
    S = ptmi_lib.NifSharingStats
    assert C.sizeof(S) == 48
    assert [(n, S.__dict__[n].offset) for n, _ in S._fields_] == [
        ("struct_size", 0), ("mode", 4), ("escaped", 8), ("evaluations", 16), ("overflowed", 24), ("table_slots", 32),
        ("share_ms", 40)]
    # the ABI version and the pinned structs do not move: the feature is added entry points only
    assert lib.pt_abi_version() == 5 and C.sizeof(ptmi_lib.Config) == 56 and C.sizeof(ptmi_lib.Stats) == 80


def test_header_declares_the_sharing_contract():
    text = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    for s in ("PT_NIF_SHARE_OFF = 0", "PT_NIF_SHARE_BATCH = 1", "PT_NIF_SHARE_STEP = 2", "typedef struct pt_nif_sharing_stats",
              "int pt_set_nif_sharing(pt_handle h, int32_t mode);",
              "int pt_get_nif_sharing_stats(pt_handle h, pt_nif_sharing_stats* out);"):
        assert s in text, s
    assert "pt_diag_set_nif_share_capacity" not in text


def test_null_handle_and_bad_mode_are_invalid_arguments(ptmi_lib):
    lib = ptmi_lib.load_library()
    assert lib.pt_set_nif_sharing(None, 0) == -1
    assert lib.pt_set_nif_sharing(None, 2) == -1
    st = ptmi_lib.NifSharingStats()
    st.struct_size = C.sizeof(st)
    assert lib.pt_get_nif_sharing_stats(None, C.byref(st)) == -1
    assert lib.pt_set_nif_sharing(None, 3) == -1 and lib.pt_set_nif_sharing(None, -1) == -1
    # (a bad mode on a real handle: tests/test_gpu_nif_sharing.py); the binding refuses unknown names before any call
    r = ptmi_lib.Renderer.__new__(ptmi_lib.Renderer)
    r._lib, r.handle = lib, None
    with pytest.raises(ValueError):
        r.set_nif_sharing("sometimes")


def test_diag_capacity_hook_lives_only_in_the_diag_library(ptmi_lib):
    product = ptmi_lib.load_library()
    diag = ptmi_lib.load_library(diag=True)
    assert not hasattr(product, "pt_diag_set_nif_share_capacity")
    assert hasattr(diag, "pt_diag_set_nif_share_capacity")
    assert diag.pt_diag_set_nif_share_capacity(None, 4) == -1
    assert b"pt_diag_set_nif_share_capacity" not in open(product._name, "rb").read()


def test_stale_library_without_the_symbols_asks_for_a_rebuild(ptmi_lib, monkeypatch):
    """Same ABI version, fewer entry points (an in-tree build from before the feature): the binding says "rebuild it"."""
    import ipu_path_trace_amd.ptmi as P
    monkeypatch.setattr(P, "EXPORTS", P.EXPORTS + ["pt_entry_point_that_does_not_exist"])
    monkeypatch.setattr(P, "_libs", {})
    with pytest.raises(RuntimeError, match="rebuild it"):
        P.load_library()


def _exe():
    exe = os.path.join(HOST, "ipu_trace")
    if not os.path.exists(exe):
        pytest.fail("ipu_trace has not been built (__graft_entry__.build)")
    return exe


def test_cli_lists_and_validates_share_nif_evaluations(tmp_path):
    exe = _exe()
    help_text = subprocess.run([exe, "--help"], capture_output=True, text=True).stdout
    assert "--share-nif-evaluations" in help_text
    base = [exe, "-o", str(tmp_path / "x.png"), "--assets", str(tmp_path), "--constant-env", "1,1,1"]
    for bad in ("on", "Step", "2", ""):
        r = subprocess.run(base + ["--share-nif-evaluations", bad], capture_output=True, text=True)
        assert r.returncode == 1 and "--share-nif-evaluations" in r.stdout, (bad, r.returncode, r.stdout[-500:])
        assert "Could not attach" not in r.stdout
    for good in ("off", "batch", "step"):
        r = subprocess.run(base + ["--share-nif-evaluations", good, "--compile-only"], capture_output=True, text=True)
        assert r.returncode == 0 and "Compile only mode selected: finished." in r.stdout, (good, r.stdout[-500:])
    assert not (tmp_path / "x.png").exists()
