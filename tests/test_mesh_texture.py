"""Texture coordinates and image textures of meshes (pt_set_mesh_texture) on the CPU, under AddressSanitizer and
UndefinedBehaviorSanitizer, as the stand-alone program tests/mesh_texture_main.cpp: every message of the host validation in the
contract's order, the index rules at s' == 1 and t' == 0 for both wraps and both filters on a non-square 5 x 3 image and on a 1 x 1
image, and the lookup the kernels run (csrc/pt_mesh.h) on 2^14 rays per fixture of tests/mesh_texture_fixtures.py: NEAREST returns a
texel of the image bit for bit -- the one a float64 restatement names --, BILINEAR lies within the range of its four taps and on the
float64 value, a constant image returns the constant exactly, an untextured mesh beside a textured one returns uv 0 and bgr 1."""
import subprocess

import numpy as np
import pytest

from tests import mesh_texture_fixtures as F


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return F.build_program(tmp_path_factory.mktemp("mesh_texture"))


def test_every_validation_message_and_index_rule_under_sanitizers(program):
    run = subprocess.run([program, "--validate"], capture_output=True, text=True, timeout=600)
    assert "runtime error" not in run.stderr and "ERROR: AddressSanitizer" not in run.stderr, run.stderr[-4000:]
    assert run.returncode == 0 and "MESH_TEXTURE_VALIDATE_OK" in run.stdout, run.stdout[-3000:] + run.stderr[-4000:]


def _counts(stdout):
    line = [l for l in stdout.splitlines() if l.startswith("rays ")][0].split()
    return {line[i]: int(line[i + 1]) for i in range(0, len(line), 2)}


@pytest.mark.parametrize("name", F.NAMES)
def test_lookup_properties_on_every_fixture(program, tmp_path, name):
    stdout, dump = F.run_fixture(program, tmp_path, name)
    print(stdout)
    c = _counts(stdout)
    assert c["rays"] >= 1 << 14 and c["textured"] >= 1000 and c["plain"] >= 1000
    assert c["outside-unit-square"] >= 200                      # the wrap decides, it is not idle
    assert c["ties"] * 10 < c["textured"]                       # the float64 restatement judged nine hits in ten at least
    if name.startswith("nearest"):
        assert c["nearest"] == c["textured"] and c["bilinear"] == 0
    else:
        assert c["bilinear"] >= 1000 and c["constant"] >= 100   # the third mesh: a constant image (1 x 1, or 3 x 2 under NEAREST)
    d = F.read_dump(dump)
    assert len(d["t"]) == c["rays"] and int((d["mesh"] >= 0).sum()) == c["hits"]
    plain = d["mesh"] == 0
    assert plain.any() and np.all(d["uv"][plain] == 0.0) and np.all(d["bgr"][plain] == 1.0)
    miss = d["mesh"] < 0
    assert miss.any() and np.all(d["uv"][miss] == 0.0) and np.all(d["bgr"][miss] == 0.0)
    textured = d["mesh"] > 0
    assert len(np.unique(d["bgr"][textured], axis=0)) >= 10     # the image varies over the surface
