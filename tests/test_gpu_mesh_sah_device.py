"""SAH mesh trees built on the device (pt_set_mesh_device_tree) on the GPU.

1. pt_mesh_tree under (device, sah) equals, byte for byte, pt_mesh_tree of a second handle under the host builder, and the CPU
   program's SAH tree (tests/mesh_lbvh_main.cpp --dump): fourteen fixtures, the world frame and two poses, each as the SECOND mesh
   of a scene so that its bases are not 0.
2. A mesh of 2 x 37 x 53 = 3922 triangles, four tiles of the partition's prefix sum and no multiple of one: the smallest shape at
   which the tile-sum hand-off can go wrong.
3. A refit after a device SAH build equals the CPU refit of the SAH tree; one refit and no build are counted.
4. linear -> sah -> linear on a live scene rebuilds each time, and a refit never keeps the other kind's topology.
5. pt_mesh_intersect: walk == brute force == the CPU program's (t, triangle).
6. Renders: (device, sah, rebuild) and (device, sah, refit) against the default over four cameras, both sample precisions --
   pt_trace_paths records, a step's accumulators and the feature buffers bit for bit.
7. pt_update_mesh_vertices(mode="rebuild") under (device, sah): the tree and the render of a fresh host-builder handle.
8. The CLI's --mesh-builder device --mesh-device-tree sah writes --mesh-builder host's EXR.
The fixtures, the scenes and the tree comparison are those of tests/test_gpu_mesh_device_build.py.
"""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import test_gpu_mesh_device_build as DB

pytestmark = pytest.mark.gpu

program = DB.program          # (the module's fixture: tests/mesh_lbvh_main.cpp, built once)
F32 = np.float32
W, H = DB.W, DB.H


def _sah_renderer(P, on_pose="rebuild", **more):
    r = DB._renderer(P, **more)
    r.set_mesh_build("device", on_pose)
    r.set_mesh_device_tree("sah")
    return r


def _tree_of(r, k):
    """Mesh k's tree as _assert_tree wants it."""
    nodes, orig = r.mesh_tree(k)
    info = r.mesh_info(k)
    return {"n_nodes": info["n_nodes"], "depth": info["depth"], "max_leaf": info["max_leaf"], "pad": F32(info["pad"]), "nodes": nodes, "orig": orig}


# ---- 1. the device SAH builder against the host builder

@pytest.mark.parametrize("name", DB.MAIN + DB.SMALL)
def test_device_sah_tree_equals_the_host_builders(ptmi_lib, program, name):
    P = ptmi_lib
    fx, other = DB._dump(P, program, name), DB._dump(P, program, "tri9" if name != "tri9" else "tri5")
    r, host = _sah_renderer(P), DB._renderer(P)
    try:
        for x in (r, host):
            x.set_scene(DB._two_mesh_scene(other, fx))
        info, tree = r.mesh_build_info(), r.mesh_device_tree_info()
        assert (info["builder"], info["device_builds"], info["host_builds"], info["refits"], info["last_kind"]) == (1, 1, 0, 0, P.MESH_LAST_DEVICE_BUILD)
        assert (tree["kind"], tree["sah_builds"]) == (P.MESH_DEVICE_TREE_SAH, 1) and tree["last_ms"] > 0
        assert 0 < tree["device_bytes"] < info["device_bytes"]
        for frame, cam in (("world", None), ("pose0", fx["cams"][0]), ("pose1", fx["cams"][1])):
            if cam:
                r.set_camera(**cam)
                host.set_camera(**cam)
            for k in (0, 1):
                _want = _tree_of(host, k)
                DB._assert_tree(r, k, _want, "%s %s, mesh %d" % (name, frame, k))
            if frame == "world":
                DB._assert_tree(r, 1, fx["trees"]["sah_world"], "%s world against the CPU program" % name)
            assert r.mesh_device_tree_info()["last_levels"] == r.mesh_info(1)["depth"] - 1      # the last mesh built
        info, tree = r.mesh_build_info(), r.mesh_device_tree_info()
        assert (info["device_builds"], info["host_builds"], info["refits"], info["last_kind"]) == (3, 0, 0, P.MESH_LAST_DEVICE_BUILD)
        assert tree["sah_builds"] == 3 and r.mesh_info(1)["build_ms"] > 0
        assert host.mesh_device_tree_info() == dict(host.mesh_device_tree_info(), kind=0, sah_builds=0, last_levels=0, device_bytes=0)
    finally:
        r.close()
        host.close()


# ---- 2. tile boundaries of the partition's prefix sum

def test_a_mesh_over_four_scan_tiles(ptmi_lib):
    P = ptmi_lib
    nx, nz = 37, 53
    xs, zs = np.meshgrid(np.arange(nx + 1), np.arange(nz + 1))
    x, z = xs.ravel() / 64.0 - 0.3, zs.ravel() / 64.0 - 3.4
    v = F32(np.stack([x, 0.05 * np.sin(9.0 * x) * np.cos(7.0 * z) - 0.2, z], axis=1))
    a = (zs[:-1, :-1] * (nx + 1) + xs[:-1, :-1]).ravel()
    t = np.concatenate([np.stack([a + 1, a + nx + 2, a + nx + 1], axis=1), np.stack([a, a + 1, a + nx + 1], axis=1)]).astype(np.uint32)
    t = t[np.random.default_rng(5).permutation(len(t))]                 # (index order carries no locality)
    assert len(t) == 2 * 37 * 53 == 3922 and len(t) % 1024 != 0 and len(t) > 3 * 1024
    r, host = _sah_renderer(P), DB._renderer(P)
    try:
        for x_ in (r, host):
            x_.set_scene([DB._mesh(v, t)])
        DB._assert_tree(r, 0, _tree_of(host, 0), "3922 triangles, world")
        cam = dict(position=(0.4, 0.3, 0.2), look_at=(0.0, -0.2, -3.0), up=(0.2, 1.0, 0.0))
        r.set_camera(**cam)
        host.set_camera(**cam)
        DB._assert_tree(r, 0, _tree_of(host, 0), "3922 triangles, posed")
        assert r.mesh_device_tree_info()["sah_builds"] == 2 and r.mesh_build_info()["host_builds"] == 0
    finally:
        r.close()
        host.close()


# ---- 3. the refit of a device-built SAH tree

@pytest.mark.parametrize("name", ["icosphere4", "grid", "tri9", "copies9"])
def test_refit_after_a_device_sah_build(ptmi_lib, program, name):
    P = ptmi_lib
    fx, other = DB._dump(P, program, name), DB._dump(P, program, "tri9" if name != "tri9" else "tri5")
    r = _sah_renderer(P, on_pose="refit")
    try:
        r.set_scene(DB._two_mesh_scene(other, fx))
        DB._assert_tree(r, 1, fx["trees"]["sah_world"], "%s world" % name)
        for p in (0, 1):
            r.set_camera(**fx["cams"][p])
            DB._assert_tree(r, 0, other["trees"]["sah_refit%d" % p], "%s refit to pose %d, first mesh" % (name, p))
            DB._assert_tree(r, 1, fx["trees"]["sah_refit%d" % p], "%s refit to pose %d" % (name, p))
            info = r.mesh_build_info()
            assert (info["refits"], info["device_builds"], info["host_builds"], info["last_kind"]) == (p + 1, 1, 0, P.MESH_LAST_REFIT)
        assert r.mesh_device_tree_info()["sah_builds"] == 1
    finally:
        r.close()


# ---- 4. switching the kind on a live scene

def test_switching_the_kind_rebuilds_and_no_refit_keeps_the_other_kind(ptmi_lib, program):
    P = ptmi_lib
    fx = DB._dump(P, program, "doubled")
    r = DB._renderer(P)
    try:
        r.set_mesh_device_tree("sah")                              # under the host builder: accepted and inert
        r.set_scene([DB._mesh(fx["v"], fx["t"])])
        assert (r.mesh_build_info()["host_builds"], r.mesh_device_tree_info()["sah_builds"], r.mesh_device_tree_info()["device_bytes"]) == (1, 0, 0)
        r.set_mesh_device_tree("linear")
        r.mesh_tree(0)
        assert r.mesh_build_info()["host_builds"] == 1             # nothing went stale
        r.set_mesh_build("device", "refit")
        DB._assert_tree(r, 0, fx["trees"]["linear_world"], "linear")
        r.set_mesh_device_tree("sah")
        assert r.mesh_device_tree_info()["device_bytes"] > 0
        DB._assert_tree(r, 0, fx["trees"]["sah_world"], "linear -> sah")
        info = r.mesh_build_info()
        assert (info["device_builds"], info["refits"], r.mesh_device_tree_info()["sah_builds"]) == (2, 0, 1)
        r.set_mesh_device_tree("sah")                              # the same kind again: nothing is stale
        r.mesh_tree(0)
        assert r.mesh_build_info()["device_builds"] == 2
        r.set_camera(**fx["cams"][0])                              # the SAH topology is the kind's in force: a refit
        DB._assert_tree(r, 0, fx["trees"]["sah_refit0"], "sah, refit to pose 0")
        assert (r.mesh_build_info()["device_builds"], r.mesh_build_info()["refits"]) == (2, 1)
        r.set_mesh_device_tree("linear")                           # the pose stands, the kind changes: a build, never a refit
        DB._assert_tree(r, 0, fx["trees"]["linear_pose0"], "sah -> linear under pose 0")
        info = r.mesh_build_info()
        assert (info["device_builds"], info["refits"], info["host_builds"], r.mesh_device_tree_info()["sah_builds"]) == (3, 1, 1, 1)
        r.set_mesh_device_tree("sah")
        r.set_camera(**fx["cams"][1])                              # kind and pose both changed: a build in the new frame
        assert r.mesh_tree(0)[1].tolist() != fx["trees"]["linear_refit1"]["orig"].tolist()
        info = r.mesh_build_info()
        assert (info["device_builds"], info["refits"], r.mesh_device_tree_info()["sah_builds"]) == (4, 1, 2)
        r.set_scene([DB._mesh(fx["v"], fx["t"])])                  # the kind outlives the scene
        assert (r.mesh_device_tree_info()["kind"], r.mesh_device_tree_info()["sah_builds"]) == (1, 3) and r.mesh_device_tree_info()["device_bytes"] > 0
        rc = r._lib.pt_set_mesh_device_tree(r.handle, 2)           # a rejected kind leaves the one in force
        assert rc == -1 and "kind must be 0 (linear) or 1 (sah) (got 2)" in r._lib.pt_last_error(r.handle).decode()
        assert r.mesh_device_tree_info()["kind"] == 1
    finally:
        r.close()


# ---- 5. pt_mesh_intersect

@pytest.mark.parametrize("name", DB.MAIN)
def test_mesh_intersect_on_a_device_sah_tree(ptmi_lib, program, name):
    P = ptmi_lib
    fx = DB._dump(P, program, name)
    r = _sah_renderer(P)
    try:
        r.set_scene([DB._mesh(fx["v"], fx["t"])])
        r.set_camera(**fx["cams"][0])
        r.mesh_tree(0)                           # the trees follow the camera; the hook ignores it and builds in the world frame again
        walk = r.mesh_intersect(fx["o"], fx["d"])
        brute = r.mesh_intersect(fx["o"], fx["d"], brute=True)
        assert r.mesh_build_info()["host_builds"] == 0 and r.mesh_device_tree_info()["sah_builds"] == 3
    finally:
        r.close()
    for a, b in zip(walk, brute):
        assert a.tobytes() == b.tobytes()
    diff = np.flatnonzero((walk[0].view(np.uint32) != fx["ht"].view(np.uint32)) | (walk[2] != fx["htri"]))
    for i in diff[:5]:
        print("%s ray %d: device (%.9g, %d), CPU program (%.9g, %d)" % (name, i, walk[0][i], walk[2][i], fx["ht"][i], fx["htri"][i]))
    assert len(diff) == 0 and np.count_nonzero(fx["htri"] >= 0) * 16 >= len(fx["ht"])


# ---- 6. renders

_renders = {}


def _render(P, program, half, on_pose):
    """DB._render's sequence under (device, sah, on_pose): per camera (records, accumulators, features, counts)."""
    key = (half, on_pose)
    if key not in _renders:
        r = _sah_renderer(P, on_pose=on_pose, half=half, spp=2)
        out = []
        try:
            r.set_scene(DB._render_scene(P, program))
            for cam in DB.CAMERAS:
                if cam:
                    r.set_camera(**cam)
                rec = P.worklist(W, H)
                r.setup(rec)
                r.path_trace()
                r.read_results(rec)
                paths = r.trace_paths(rec["u"], rec["v"], np.full(len(rec), 1, np.uint32))
                f = r.feature_buffers()
                out.append((paths.tobytes(), rec.tobytes(), {k: np.ascontiguousarray(f[k]).tobytes() for k in ("object_id", "depth", "normal", "albedo")}))
            _renders[key] = (out, r.mesh_build_info(), r.mesh_device_tree_info())
        finally:
            r.close()
    return _renders[key]


@pytest.mark.parametrize("half", [False, True], ids=["float", "half"])
@pytest.mark.parametrize("on_pose", ["rebuild", "refit"])
def test_renders_equal_the_default(ptmi_lib, program, on_pose, half):
    P = ptmi_lib
    want, base = DB._render(P, program, half, None)
    got, info, tree = _render(P, program, half, on_pose)
    builds = len(DB.CAMERAS) + 1                   # the scene; again at the first render, for its normals and its texture; three poses
    assert (base["host_builds"], base["device_builds"], base["refits"]) == (builds, 0, 0)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0], "pt_trace_paths records differ under camera %d" % k
        assert g[1] == w[1], "accumulators differ under camera %d" % k
        for key in w[2]:
            assert g[2][key] == w[2][key], "feature %s differs under camera %d" % (key, k)
        assert w[3] > 30 and w[4] > 100                                          # both meshes are in view
    refits = len(DB.CAMERAS) - 1 if on_pose == "refit" else 0
    assert (info["refits"], info["device_builds"], info["host_builds"]) == (refits, builds - refits, 0)
    assert tree["sah_builds"] == builds - refits


# ---- 7. animated meshes

def test_update_rebuild_under_device_sah_equals_a_fresh_host_handle(ptmi_lib, program):
    P = ptmi_lib
    fx, other = DB._dump(P, program, "icosphere4"), DB._dump(P, program, "tri9")
    v = np.asarray(fx["v"], np.float64)
    c = v.mean(0)
    v2 = F32(c + (v - c) * (1.0 + 0.35 * np.sin(40.0 * v[:, [1]]) * np.array([1.0, 0.2, 0.6])))     # a deformation no refit would like

    def paths(r):
        rec = P.worklist(W, H)
        r.setup(rec)
        r.path_trace()
        r.read_results(rec)
        return rec.tobytes()
    cam = dict(position=(0.3, -0.1, -2.4), look_at=(0.37, -0.21, -2.9), up=(0.1, 1.0, 0.0))
    r, host = _sah_renderer(P), DB._renderer(P)
    try:
        r.set_scene(DB._two_mesh_scene(other, fx))
        r.set_camera(**cam)
        r.mesh_tree(1)                                             # the trees follow the camera: the update rebuilds in its frame
        before = (r.mesh_build_info()["device_builds"], r.mesh_device_tree_info()["sah_builds"])
        r.update_mesh_vertices(1, v2, mode="rebuild")
        up, info, tree = r.mesh_update_info(), r.mesh_build_info(), r.mesh_device_tree_info()
        assert (up["updates"], up["rebuilds"], up["refits"], up["fallbacks"], up["last_kind"]) == (1, 1, 0, 0, P.MESH_LAST_DEVICE_BUILD)
        assert (info["device_builds"], tree["sah_builds"], info["host_builds"]) == (before[0] + 1, before[1] + 1, 0)
        host.set_scene(DB._two_mesh_scene(other, dict(fx, v=v2)))
        host.set_camera(**cam)
        for k in (0, 1):
            DB._assert_tree(r, k, _tree_of(host, k), "mesh %d after the update" % k)
        assert r.mesh_build_info()["device_builds"] == before[0] + 1            # pt_mesh_tree found the trees up to date
        assert r.mesh_device_tree_info()["last_levels"] == r.mesh_info(1)["depth"] - 1
        got, want = paths(r), paths(host)
        assert got == want and len(set(got)) > 100
    finally:
        r.close()
        host.close()


# ---- 8. the CLI

def test_cli_device_sah_writes_the_hosts_exr(program, ptmi_lib, tmp_path):
    exe = os.path.join(DB.HOST, "ipu_trace")
    if not os.path.exists(exe):
        pytest.fail("ipu_trace has not been built (__graft_entry__.build)")
    fx = DB._dump(ptmi_lib, program, "icosphere2")
    v = DB._scaled(fx["v"], 1.1, (0.03, -0.03, -0.55))
    objects = [{"shape": "mesh", "material": "refractive", "colour": [0.9, 0.95, 0.9], "vertices": v.tolist(), "triangles": fx["t"].tolist()},
               {"shape": "sphere", "material": "emissive", "emission": list(DB.LAMP), "centre": [-0.1, 0.15, -0.5], "radius": 0.04},
               {"shape": "mesh", "material": "diffuse", "colour": [0.8, 0.7, 0.5], "vertices": [[-0.5, -0.2, -1.0], [0.5, -0.2, -1.0], [0.5, -0.22, -0.2], [-0.5, -0.22, -0.2]],
                "triangles": [[0, 1, 2], [0, 2, 3]]}]
    path = tmp_path / "scene.json"
    path.write_text(json.dumps({"objects": objects, "camera": {"position": [0.05, 0.02, 0.15], "look_at": [0.0, -0.02, -0.3], "up": [0.05, 1, 0]}}))
    out = {}
    for tag, options in (("host", ["--mesh-builder", "host"]), ("sah", ["--mesh-builder", "device", "--mesh-device-tree", "sah"])):
        r = subprocess.run([exe, "--assets", str(tmp_path), "--constant-env", ",".join(str(x) for x in DB.ENV), "-w", str(W), "-h", str(H), "-s", "4",
                            "--samples-per-step", "4", "--max-path-length", "7", "-o", str(tmp_path / (tag + ".png")), "--save-interval", "1",
                            "--scene", str(path)] + options, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
        out[tag] = (tmp_path / (tag + ".exr")).read_bytes()
    assert out["host"] == out["sah"] and len(set(out["host"])) > 100
