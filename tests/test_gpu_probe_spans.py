"""The query entry points' one path (csrc/ptmi_probe.h) on the GPU: how the caller's arrays are packed into the scratch buffer, and
the last, partial workgroup of each kernel.

Every probe computes item i from item i's inputs alone.  So each of the ten is called on prefixes of ONE input batch, in an order
that makes the scratch buffer grow and then be reused by a smaller call, and every prefix's outputs must equal the same rows of the
full batch bit for bit: no reference, no tolerance.  Odd lengths put 16-byte padding between the spans (n x 4 bytes, n odd); 255 and
257 (127 and 129 for pt_trace_paths, whose workgroups are 128 wide) end in a partial workgroup on either side of a full one.

The scene is one two-triangle mesh with normals and a 2 x 2 texture beside an emissive sphere, so that the mesh hooks, the emitter
guide and the textured trace-paths instance all have work.
"""
import numpy as np
import pytest

from ipu_path_trace_amd import nif_assets

pytestmark = pytest.mark.gpu

F32 = np.float32
W = H = 32
BATCH, PREFIXES = 513, (1, 3, 255, 513, 257)
PATHS_BATCH, PATHS_PREFIXES = 257, (1, 127, 257, 129)


def _unit(a):
    return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(F32)


def _scene():
    quad = np.array([(-0.5, -0.5, -1.5), (0.5, -0.5, -1.5), (0.5, 0.5, -1.5), (-0.5, 0.5, -1.4)], F32)
    return [{"shape": "mesh", "material": "diffuse", "colour": (0.8, 0.7, 0.5), "vertices": quad, "triangles": [(0, 1, 2), (0, 2, 3)],
             "normals": _unit(np.array([(0.2, 0.1, 1.0), (-0.2, 0.1, 1.0), (-0.1, -0.2, 1.0), (0.1, -0.1, 1.0)])),
             "texture": np.arange(12, dtype=F32).reshape(2, 2, 3) / 8 + F32(0.125),
             "uvs": np.array([(0.0, 0.0), (1.7, 0.0), (1.7, 1.7), (0.0, 1.7)], F32)},
            {"shape": "sphere", "material": "emissive", "centre": (0.0, 0.6, -1.0), "radius": 0.15, "colour": (5.0, 4.0, 3.0)}]


@pytest.fixture(scope="module")
def renderer(ptmi_lib):
    rng = np.random.default_rng(2)
    r = ptmi_lib.Renderer(W, H, max_path_length=6)
    r.init_nif_weights(nif_assets.synthetic_nif(), 12, nif_assets.URBAN_ALLEY_META["max"], nif_assets.folded_mean())
    r.init_render_settings(seed=7, samples_per_step=1)
    r.set_scene(_scene())
    r.set_env_guide(rng.random((8, 16, 3), dtype=F32) + F32(0.05), alpha=0.4)
    r.set_light_guide(0.4)
    yield r
    r.close()


@pytest.fixture(scope="module")
def batch():
    """The one input batch: BATCH rows of everything a probe takes."""
    rng = np.random.default_rng(1)
    n = BATCH
    aim = np.stack([rng.uniform(-0.8, 0.8, n), rng.uniform(-0.8, 0.8, n), np.full(n, -1.5)], axis=1)
    return {
        "u": rng.random(n, dtype=F32), "v": rng.random(n, dtype=F32),
        "g1": rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32),
        "g2": rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32),
        "g3": rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32),
        "unit": _unit(rng.normal(size=(n, 3))),
        "normal": _unit(rng.normal(size=(n, 3))),
        "point": (rng.uniform(-0.3, 0.3, (n, 3)) + (0.0, 0.0, -1.0)).astype(F32),
        "origin": rng.uniform(-0.05, 0.05, (n, 3)).astype(F32),
        "dir": _unit(aim),
        "pu": rng.integers(0, W, n).astype(np.uint16), "pv": rng.integers(0, H, n).astype(np.uint16),
        "ps": rng.integers(0, 64, n).astype(np.uint32),
    }


def _check(call, inputs, prefixes=PREFIXES):
    """call(*rows[:p]) for every prefix length p in order; each result against the same rows of the longest call's.  Returns the
    longest call's outputs."""
    full_n = max(prefixes)
    assert all(len(a) >= full_n for a in inputs)
    got = {}
    for p in prefixes:
        out = call(*[a[:p] for a in inputs])
        got[p] = out if isinstance(out, tuple) else (out,)
    full = got[full_n]
    for p in prefixes:
        for k, (a, b) in enumerate(zip(got[p], full)):
            assert len(a) == p
            same = np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b[:p]).tobytes()
            assert same, "prefix of %d items: output %d differs from the first rows of the %d-item call" % (p, k, full_n)
    return full


def test_nif_infer(renderer, batch):
    (bgr,) = _check(renderer.nif_infer, (batch["u"], batch["v"]))
    assert len(np.unique(bgr, axis=0)) > BATCH // 2


def test_env_map_lookup(ptmi_lib, batch):
    r = ptmi_lib.Renderer(W, H)
    try:
        r.set_env_map(np.random.default_rng(3).random((4, 8, 3), dtype=F32))
        (bgr,) = _check(r.env_map_lookup, (batch["u"], batch["v"]))
    finally:
        r.close()
    assert len(np.unique(bgr, axis=0)) > BATCH // 2


def test_env_guide_sample(renderer, batch):
    uv, cell = _check(renderer.env_guide_sample, (batch["g1"], batch["g2"], batch["g3"]))
    assert len(np.unique(cell)) > 8 and len(np.unique(uv, axis=0)) > BATCH // 2


def test_env_guide_eval(renderer, batch):
    cell, g = _check(renderer.env_guide_eval, (batch["unit"],))
    assert len(np.unique(cell)) > 8 and np.all(g > 0)


def test_light_guide_sample(renderer, batch):
    d, light = _check(renderer.light_guide_sample, (batch["point"], batch["normal"], batch["g1"], batch["g2"], batch["g3"]))
    assert (light >= 0).any() and np.any(d[light >= 0] != 0)


def test_light_guide_eval(renderer, batch):
    towards = _unit(np.array((0.0, 0.6, -1.0)) - batch["point"].astype(np.float64))   # the emitter's centre
    total, pe = _check(renderer.light_guide_eval, (batch["point"], batch["normal"], towards))
    assert (total > 0).any() and (pe > 0).any()


@pytest.mark.parametrize("brute", [False, True])
def test_mesh_intersect(renderer, batch, brute):
    t, obj, tri = _check(lambda o, d: renderer.mesh_intersect(o, d, brute=brute), (batch["origin"], batch["dir"]))
    assert set(np.unique(tri)) == {-1, 0, 1} and (obj < 0).any() and np.all(t[obj >= 0] > 0)


def test_mesh_shade(renderer, batch):
    t, obj, tri, bary, normal = _check(renderer.mesh_shade, (batch["origin"], batch["dir"]))
    assert set(np.unique(tri)) == {-1, 0, 1} and np.all(np.any(normal[tri >= 0] != 0, axis=1)) and np.all(normal[tri < 0] == 0)


def test_mesh_texel(renderer, batch):
    t, obj, tri, uv, bgr = _check(renderer.mesh_texel, (batch["origin"], batch["dir"]))
    assert set(np.unique(tri)) == {-1, 0, 1} and len(np.unique(bgr[tri >= 0], axis=0)) > 4 and np.all(bgr[obj < 0] == 0)


def test_trace_paths(renderer, batch):
    (rec,) = _check(renderer.trace_paths, (batch["pu"], batch["pv"], batch["ps"]), PATHS_PREFIXES)
    assert len(rec) == PATHS_BATCH and len(np.unique(rec["length"])) > 1
    assert renderer.trace_variant()["paths"]["launches"] == len(PATHS_PREFIXES)
