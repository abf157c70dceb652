"""Mesh trees built and refitted on the device (pt_set_mesh_build) on the GPU.

1. pt_mesh_tree after a device build equals the CPU reference builder's nodes and slot map (tests/mesh_lbvh_main.cpp --dump), byte
   for byte: fourteen fixtures, the world frame and two poses, each as the SECOND mesh of a scene so that its bases are not 0.
2. pt_mesh_tree after a refit equals the CPU refit, byte for byte, for SAH and linear topology; n_nodes, depth and max_leaf do not
   move and pt_get_mesh_build_info counts one refit and no build.
3. pt_mesh_intersect under the device builder: walk == brute force == the CPU program's (t, triangle) on its rays.
4. Renders: (device, rebuild), (host, refit) and (device, refit) against the default over four cameras set one after the other, both
   sample precisions -- pt_trace_paths records, a step's accumulators and the feature buffers bit for bit -- on a glass icosphere with
   vertex normals over a textured grid.
5. Lifetimes.   6. The CLI's --mesh-builder device writes --mesh-builder host's EXR.
"""
import os
import subprocess

import numpy as np
import pytest

from tests import scene_poly_model as PM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ipu_path_trace_amd", "host")
F32 = np.float32
W, H = 64, 48
ENV = (0.75, 1.5, 3.0)
LAMP = (6.0, 4.5, 3.0)
MAIN = ["icosphere2", "icosphere4", "grid", "doubled", "sliver", "single"]
SMALL = ["tri2", "tri3", "tri4", "tri5", "tri8", "tri9", "copies9", "planar"]
TREES = ["linear_world", "linear_pose0", "linear_pose1", "linear_refit0", "linear_refit1", "sah_refit0", "sah_refit1", "sah_world"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mesh_lbvh") / "mesh_lbvh")
    build = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                            "-I" + os.path.join(ROOT, "ipu_path_trace_amd", "csrc"), "-I" + os.path.join(ROOT, "tests"), "-o", exe,
                            os.path.join(ROOT, "tests", "mesh_lbvh_main.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    return exe


_dumps = {}


def _dump(P, exe, name):
    """A fixture as the CPU program made it: v, t, rays o and d, the walk's ht and htri, two cameras, and the eight trees of TREES."""
    if name not in _dumps:
        path = os.path.join(os.path.dirname(exe), name + ".bin")
        subprocess.run([exe, "--dump", name, path], check=True, timeout=120)
        raw = np.fromfile(path, np.uint32)
        os.remove(path)
        assert raw[0] == 0x4c425648
        nv, nt, nr = int(raw[1]), int(raw[2]), int(raw[3])
        at = 4

        def take(count, dtype):
            nonlocal at
            out = raw[at:at + count].view(dtype)
            at += count
            return out
        d = {"v": take(3 * nv, F32).reshape(-1, 3), "t": take(3 * nt, np.uint32).reshape(-1, 3), "o": take(3 * nr, F32).reshape(-1, 3),
             "d": take(3 * nr, F32).reshape(-1, 3), "ht": take(nr, F32), "htri": take(nr, np.int32), "cams": [], "trees": {}}
        for _ in range(2):
            c = take(9, F32)
            d["cams"].append(dict(position=tuple(map(float, c[0:3])), look_at=tuple(map(float, c[3:6])), up=tuple(map(float, c[6:9]))))
        for key in TREES:
            head = take(4, np.uint32)
            pad = take(1, F32)[0]
            nodes = take(8 * int(head[0]), np.uint32).copy().view(P.MESH_NODE_DTYPE)
            d["trees"][key] = {"n_nodes": int(head[0]), "depth": int(head[1]), "max_leaf": int(head[2]), "pad": pad, "nodes": nodes,
                               "orig": take(nt, np.uint32)}
        assert at == len(raw)
        _dumps[name] = d
    return _dumps[name]


def _mesh(v, t, material="diffuse", colour=(0.8, 0.7, 0.5), **more):
    return dict({"shape": "mesh", "material": material, "colour": colour, "vertices": v, "triangles": t}, **more)


def _renderer(P, half=False, spp=1):
    r = P.Renderer(W, H, max_path_length=PM.DEPTH, roulette_depth=PM.ROULETTE, sample_precision=P.SAMPLES_HALF if half else P.SAMPLES_FLOAT)
    r.set_constant_env(ENV)
    r.init_render_settings(seed=PM.SEED, samples_per_step=spp, aa_noise_scale=PM.AA_SCALE)
    return r


def _assert_tree(r, k, want, what):
    nodes, orig = r.mesh_tree(k)
    info = r.mesh_info(k)
    assert (info["n_nodes"], info["depth"], info["max_leaf"]) == (want["n_nodes"], want["depth"], want["max_leaf"]), what
    assert F32(info["pad"]).tobytes() == F32(want["pad"]).tobytes(), what
    assert np.array_equal(orig, want["orig"]), what
    bad = np.flatnonzero(nodes.view(np.uint32).reshape(-1, 8) != want["nodes"].view(np.uint32).reshape(-1, 8))
    if len(bad):
        i = bad[0] // 8
        print("%s: node %d: device %r, reference %r" % (what, i, nodes[i], want["nodes"][i]))
    assert len(bad) == 0 and len(nodes) == want["n_nodes"], what


def _two_mesh_scene(first, second):
    return [{"shape": "sphere", "material": "emissive", "colour": LAMP, "centre": (0.0, 0.3, -2.5), "radius": 0.05},
            _mesh(first["v"], first["t"]), _mesh(second["v"], second["t"], "specular")]


# ---- 1. the device builder against the CPU reference builder

@pytest.mark.parametrize("name", MAIN + SMALL)
def test_device_build_equals_the_reference_builder(ptmi_lib, program, name):
    P = ptmi_lib
    fx, other = _dump(P, program, name), _dump(P, program, "tri9" if name != "tri9" else "tri5")
    r = _renderer(P)
    try:
        r.set_mesh_build(builder="device")
        r.set_scene(_two_mesh_scene(other, fx))
        info = r.mesh_build_info()
        assert (info["builder"], info["on_pose"], info["device_builds"], info["host_builds"], info["refits"]) == (1, 0, 1, 0, 0)
        assert info["last_kind"] == P.MESH_LAST_DEVICE_BUILD and info["device_bytes"] > 48 * (len(fx["t"]) + len(other["t"])) and info["last_ms"] > 0
        for frame, cam in (("world", None), ("pose0", fx["cams"][0]), ("pose1", fx["cams"][1])):
            if cam:
                r.set_camera(**cam)
            _assert_tree(r, 0, other["trees"]["linear_" + frame], "%s %s, first mesh" % (name, frame))
            _assert_tree(r, 1, fx["trees"]["linear_" + frame], "%s %s" % (name, frame))
        info = r.mesh_build_info()
        assert (info["device_builds"], info["host_builds"], info["refits"]) == (3, 0, 0)
        assert r.mesh_info(1)["build_ms"] > 0
    finally:
        r.close()


# ---- 2. the refit against the CPU refit

@pytest.mark.parametrize("builder", ["host", "device"])
@pytest.mark.parametrize("name", MAIN + SMALL)
def test_refit_equals_the_reference_refit(ptmi_lib, program, name, builder):
    P = ptmi_lib
    fx, other = _dump(P, program, name), _dump(P, program, "tri9" if name != "tri9" else "tri5")
    kind = "sah" if builder == "host" else "linear"
    r = _renderer(P)
    try:
        r.set_mesh_build(builder=builder, on_pose="refit")
        r.set_scene(_two_mesh_scene(other, fx))
        _assert_tree(r, 1, fx["trees"][kind + "_world"], "%s world (%s)" % (name, kind))
        before = r.mesh_build_info()
        assert before["refits"] == 0 and before["host_builds"] + before["device_builds"] == 1
        for p in (0, 1):
            shape = [(r.mesh_info(k)["n_nodes"], r.mesh_info(k)["depth"], r.mesh_info(k)["max_leaf"]) for k in (0, 1)]
            r.set_camera(**fx["cams"][p])
            _assert_tree(r, 0, other["trees"]["%s_refit%d" % (kind, p)], "%s refit to pose %d, first mesh (%s)" % (name, p, kind))
            _assert_tree(r, 1, fx["trees"]["%s_refit%d" % (kind, p)], "%s refit to pose %d (%s)" % (name, p, kind))
            assert shape == [(r.mesh_info(k)["n_nodes"], r.mesh_info(k)["depth"], r.mesh_info(k)["max_leaf"]) for k in (0, 1)]
            info = r.mesh_build_info()
            assert info["refits"] == p + 1 and info["last_kind"] == P.MESH_LAST_REFIT
            assert (info["host_builds"], info["device_builds"]) == (before["host_builds"], before["device_builds"])   # one refit and no build
        # the hooks force the world frame: a refit back, and the world tree's bytes
        t, obj, tri = r.mesh_intersect(fx["o"][:256], fx["d"][:256])
        assert r.mesh_build_info()["refits"] == 3
        r.set_camera()
        _assert_tree(r, 1, fx["trees"][kind + "_world"], "%s back in the world frame (%s)" % (name, kind))
    finally:
        r.close()


# ---- 3. pt_mesh_intersect under the device builder

@pytest.mark.parametrize("name", MAIN)
def test_mesh_intersect_on_a_device_built_tree(ptmi_lib, program, name):
    P = ptmi_lib
    fx = _dump(P, program, name)
    r = _renderer(P)
    try:
        r.set_mesh_build(builder="device", on_pose="refit")
        r.set_scene([_mesh(fx["v"], fx["t"])])
        r.set_camera(**fx["cams"][0])            # (the hook ignores the camera: it refits to the world frame)
        walk = r.mesh_intersect(fx["o"], fx["d"])
        brute = r.mesh_intersect(fx["o"], fx["d"], brute=True)
    finally:
        r.close()
    for a, b in zip(walk, brute):
        assert a.tobytes() == b.tobytes()
    diff = np.flatnonzero((walk[0].view(np.uint32) != fx["ht"].view(np.uint32)) | (walk[2] != fx["htri"]))
    for i in diff[:5]:
        print("%s ray %d: device (%.9g, %d), CPU program (%.9g, %d)" % (name, i, walk[0][i], walk[2][i], fx["ht"][i], fx["htri"][i]))
    assert len(diff) == 0 and np.count_nonzero(fx["htri"] >= 0) * 16 >= len(fx["ht"])


# ---- 4. renders

def _scaled(v, scale, centre):
    v = np.asarray(v, np.float64)
    return F32((v - v.mean(0)) * scale + np.asarray(centre, np.float64))


def _render_scene(P, program):
    ball, floor = _dump(P, program, "icosphere4"), _dump(P, program, "grid")
    bv = _scaled(ball["v"], 1.1, (0.03, -0.03, -0.55))          # 0.22 across
    fv = _scaled(floor["v"], 0.8, (0.0, -0.19, -0.55))
    normals = bv.astype(np.float64) - bv.astype(np.float64).mean(0)
    normals = F32(normals / np.linalg.norm(normals, axis=1)[:, None])
    rng = np.random.default_rng(7)
    image = F32(rng.uniform(0.2, 1.0, (8, 8, 3)))
    uvs = F32((fv[:, [0, 2]] - fv[:, [0, 2]].min(0)) / np.ptp(fv[:, [0, 2]], axis=0) * 3.0)
    return [_mesh(bv, ball["t"], "refractive", (0.9, 0.95, 0.9), normals=normals),
            _mesh(fv, floor["t"], "diffuse", (0.8, 0.8, 0.8), texture=image, uvs=uvs),
            {"shape": "parallelogram", "material": "emissive", "colour": LAMP,
             "vertices": ((-0.08, 0.22, -0.62), (0.08, 0.23, -0.62), (-0.08, 0.2, -0.48))},
            {"shape": "sphere", "material": "specular", "centre": (-0.15, -0.1, -0.6), "radius": 0.05, "colour": (1.0, 1.0, 1.0)}]


CAMERAS = [None, dict(PM.MOVED), dict(position=(-0.25, 0.1, 0.2), look_at=(0.0, -0.05, -0.55), up=(0.3, 1.0, 0.1)),
           dict(position=(0.1, 0.3, -1.3), look_at=(0.0, -0.05, -0.55), up=(0.0, 1.0, 0.0))]
_renders = {}


def _render(P, program, half, options, late=False):
    """Per camera of CAMERAS, set one after the other on one handle: (records, accumulators, features).  late: the options are
    set after the scene, its normals and its texture."""
    key = (half, options, late)
    if key not in _renders:
        r = _renderer(P, half=half, spp=2)
        out = []
        try:
            if options and not late:
                r.set_mesh_build(*options)
            r.set_scene(_render_scene(P, program))
            if options and late:
                r.set_mesh_build(*options)
            for cam in CAMERAS:
                if cam:
                    r.set_camera(**cam)
                rec = P.worklist(W, H)
                r.setup(rec)
                r.path_trace()
                r.read_results(rec)
                paths = r.trace_paths(rec["u"], rec["v"], np.full(len(rec), 1, np.uint32))
                f = r.feature_buffers()
                out.append((paths.tobytes(), rec.tobytes(), {k: np.ascontiguousarray(f[k]).tobytes() for k in ("object_id", "depth", "normal", "albedo")},
                            int(np.count_nonzero(f["object_id"] == 0)), int(np.count_nonzero(f["object_id"] == 1))))
            _renders[key] = (out, r.mesh_build_info())
        finally:
            r.close()
    return _renders[key]


@pytest.mark.parametrize("half", [False, True], ids=["float", "half"])
@pytest.mark.parametrize("options", [("device", "rebuild"), ("host", "refit"), ("device", "refit")], ids=lambda o: "-".join(o))
def test_renders_equal_the_default(ptmi_lib, program, options, half):
    P = ptmi_lib
    want, base = _render(P, program, half, None)
    got, info = _render(P, program, half, options)
    builds = len(CAMERAS) + 1                      # the scene; again at the first render, for its normals and its texture; three poses
    assert (base["host_builds"], base["device_builds"], base["refits"]) == (builds, 0, 0)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0], "pt_trace_paths records differ under camera %d" % k
        assert g[1] == w[1], "accumulators differ under camera %d" % k
        for key in w[2]:
            assert g[2][key] == w[2][key], "feature %s differs under camera %d" % (key, k)
        assert w[3] > 30 and w[4] > 100                                          # both meshes are in view
    refits = len(CAMERAS) - 1 if options[1] == "refit" else 0
    assert info["refits"] == refits and info["host_builds"] + info["device_builds"] == builds - refits
    assert (info["device_builds"] == 0) == (options[0] == "host")


# ---- 5. lifetimes

def test_a_handle_that_never_calls_the_api_reports_the_defaults(ptmi_lib, program):
    P = ptmi_lib
    fx = _dump(P, program, "icosphere2")
    r = _renderer(P)
    try:
        info = r.mesh_build_info()
        assert info == dict(info, builder=0, on_pose=0, host_builds=0, device_builds=0, refits=0, last_kind=0, device_bytes=0) and info["last_ms"] == 0
        r.set_scene([_mesh(fx["v"], fx["t"])])
        r.set_camera(**fx["cams"][0])
        nodes, orig = r.mesh_tree(0)
        assert len(nodes) == r.mesh_info(0)["n_nodes"] and sorted(orig.tolist()) == list(range(len(fx["t"])))
        info = r.mesh_build_info()
        assert (info["host_builds"], info["device_builds"], info["refits"], info["device_bytes"], info["last_kind"]) == (2, 0, 0, 0, P.MESH_LAST_HOST_BUILD)
        assert r._lib.pt_mesh_tree(r.handle, 0, np.zeros(1, P.MESH_NODE_DTYPE).ctypes.data, 1, None, 0) == -1       # a capacity too small
        assert "node_capacity must be >= " in r._lib.pt_last_error(r.handle).decode()
        assert r._lib.pt_mesh_tree(r.handle, 0, None, 0, None, 5) == -1                                             # NULL with a capacity
        assert r._lib.pt_mesh_tree(r.handle, 1, None, 0, None, 0) == -1                                             # no such mesh
        r.set_scene(None)
        assert r._lib.pt_mesh_tree(r.handle, 0, None, 0, None, 0) == -5                                             # PT_ERR_NOT_READY
    finally:
        r.close()


def test_options_survive_a_new_scene_and_null_returns_to_the_host_path(ptmi_lib, program):
    P = ptmi_lib
    a, b = _dump(P, program, "doubled"), _dump(P, program, "sliver")
    r = _renderer(P)
    try:
        r.set_scene([_mesh(a["v"], a["t"])])
        host_nodes = r.mesh_info(0)["n_nodes"]
        assert host_nodes == a["trees"]["sah_world"]["n_nodes"]
        r.set_mesh_build("device", "refit")                       # a change of builder: the trees of the scene in force are stale
        _assert_tree(r, 0, a["trees"]["linear_world"], "doubled after the option")
        assert r.mesh_build_info()["device_builds"] == 1
        r.set_mesh_build("device", "rebuild")                     # on_pose alone: nothing is stale
        r.mesh_tree(0)
        assert r.mesh_build_info()["device_builds"] == 1
        r.set_scene([_mesh(b["v"], b["t"])])                      # the options outlive the scene
        info = r.mesh_build_info()
        assert (info["builder"], info["on_pose"], info["device_builds"]) == (1, 0, 2)
        _assert_tree(r, 0, b["trees"]["linear_world"], "sliver, a new scene under the option")
        r.set_scene(None)
        r.set_scene([_mesh(a["v"], a["t"])])
        assert r._lib.pt_set_mesh_build(r.handle, None) == 0       # NULL: HOST + REBUILD
        info = r.mesh_build_info()
        assert (info["builder"], info["on_pose"]) == (0, 0)
        _assert_tree(r, 0, a["trees"]["sah_world"], "doubled back on the host path")
        assert r.mesh_info(0)["n_nodes"] == host_nodes
    finally:
        r.close()


def test_normals_and_texture_before_or_after_the_option_give_the_same_bytes(ptmi_lib, program):
    P = ptmi_lib
    for half in (False,):
        early, _ = _render(P, program, half, ("device", "refit"))
        late, info = _render(P, program, half, ("device", "refit"), late=True)
        assert [e[:3] for e in early] == [l[:3] for l in late]
        assert (info["refits"], info["device_builds"], info["host_builds"]) == (len(CAMERAS) - 1, 1, 1)   # (the scene was set under the defaults)


# ---- 6. the CLI

def test_cli_mesh_builder_device_writes_the_hosts_exr(program, ptmi_lib, tmp_path):
    import json
    exe = os.path.join(HOST, "ipu_trace")
    if not os.path.exists(exe):
        pytest.fail("ipu_trace has not been built (__graft_entry__.build)")
    fx = _dump(ptmi_lib, program, "icosphere2")
    v = _scaled(fx["v"], 1.1, (0.03, -0.03, -0.55))
    objects = [{"shape": "mesh", "material": "refractive", "colour": [0.9, 0.95, 0.9], "vertices": v.tolist(), "triangles": fx["t"].tolist()},
               {"shape": "sphere", "material": "emissive", "emission": list(LAMP), "centre": [-0.1, 0.15, -0.5], "radius": 0.04},
               {"shape": "mesh", "material": "diffuse", "colour": [0.8, 0.7, 0.5], "vertices": [[-0.5, -0.2, -1.0], [0.5, -0.2, -1.0], [0.5, -0.22, -0.2], [-0.5, -0.22, -0.2]],
                "triangles": [[0, 1, 2], [0, 2, 3]]}]
    path = tmp_path / "scene.json"
    path.write_text(json.dumps({"objects": objects, "camera": {"position": [0.05, 0.02, 0.15], "look_at": [0.0, -0.02, -0.3], "up": [0.05, 1, 0]}}))
    out = {}
    for builder in ("host", "device"):
        r = subprocess.run([exe, "--assets", str(tmp_path), "--constant-env", ",".join(str(x) for x in ENV), "-w", str(W), "-h", str(H), "-s", "4",
                            "--samples-per-step", "4", "--max-path-length", "7", "-o", str(tmp_path / (builder + ".png")), "--save-interval", "1",
                            "--scene", str(path), "--mesh-builder", builder], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
        out[builder] = (tmp_path / (builder + ".exr")).read_bytes()
    assert out["host"] == out["device"] and len(set(out["host"])) > 100
