"""Runtime scenes on the GPU (pt_set_scene): the built-in table round-trips bit for bit, a 32-object scene, closed-form checks
that need no inferred light:: routine (a mirror under a constant sky, the furnace test, an emitting shell), geometry through
pt_trace_paths against float64 numpy, sharing and the memo on a scene with an emitter, and the CLI's --scene."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from ipu_path_trace_amd import nif_assets

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ipu_path_trace_amd", "host")
META = nif_assets.URBAN_ALLEY_META
L_SKY = (0.75, 1.5, 3.0)        # few mantissa bits: L x 1 and sums of powers of two of them are exact
MIRROR = 1                      # index of the mirror sphere in the built-in scene


def _render(P, W, H, scene=None, const=None, layers=None, spp=4, steps=1, depth=8, roulette=3, precision=0, memo=0,
            mode="off", scene_after=None, seed=1):
    """`steps` steps with the film resident; returns (records of the last step, film bytes, stats of every step)."""
    r = P.Renderer(W, H, max_path_length=depth, roulette_depth=roulette, sample_precision=precision, iterations_per_batch=2)
    try:
        if const is not None:
            r.set_constant_env(const)
        else:
            r.init_nif_weights(layers if layers is not None else nif_assets.synthetic_nif(), 12, META["max"],
                               nif_assets.folded_mean())
        r.init_render_settings(seed=seed, samples_per_step=spp)
        if scene is not None:
            r.set_scene(scene)
        r.set_nif_sharing(mode)
        if memo:
            r.set_nif_memo(memo)
        rec = P.worklist(W, H)
        r.setup(rec)
        stats = []
        for s in range(steps):
            if scene_after is not None and s == steps // 2:
                r.set_scene(scene_after)
            r.path_trace()
            stats.append(r.read_results(rec).as_dict())
            r.film_accumulate()
        film = r.gather_hdr(W * H, P.HDR_FILM)[0].copy()
        return rec, film, stats
    finally:
        r.close()


def _paths(P, W, H, scene=None, const=L_SKY, n=4096, depth=8, roulette=8, seed=7):
    r = P.Renderer(W, H, max_path_length=depth, roulette_depth=roulette)
    try:
        r.set_constant_env(const)
        r.init_render_settings(seed=3, samples_per_step=1)
        if scene is not None:
            r.set_scene(scene)
        rng = np.random.default_rng(seed)
        u = rng.integers(0, W, n).astype(np.uint16)
        v = rng.integers(0, H, n).astype(np.uint16)
        s = rng.integers(0, 1000, n).astype(np.uint32)
        return r.trace_paths(u, v, s)
    finally:
        r.close()


def _sphere(centre, radius, material, colour=(1, 1, 1)):
    return {"shape": "sphere", "centre": centre, "radius": radius, "material": material, "colour": colour}


def test_builtin_table_round_trips_bit_for_bit(ptmi_lib):
    P = ptmi_lib
    table = P.builtin_scene()
    for kw in ({"layers": nif_assets.synthetic_nif()}, {"const": (0.6, 0.9, 1.3)}):
        rec0, film0, st0 = _render(P, 96, 72, spp=6, steps=2, **kw)
        rec1, film1, st1 = _render(P, 96, 72, scene=table, spp=6, steps=2, **kw)
        assert rec0.tobytes() == rec1.tobytes() and film0.tobytes() == film1.tobytes()
        for a, b in zip(st0, st1):
            assert (a["paths"], a["segments"], a["escaped"]) == (b["paths"], b["segments"], b["escaped"])
    assert _paths(P, 96, 72, roulette=3).tobytes() == _paths(P, 96, 72, scene=table, roulette=3).tobytes()
    # (NULL, 0) restores the built-in scene; a rejected table leaves the scene in force
    r = P.Renderer(32, 32)
    try:
        r.set_scene([_sphere((0, 0, -3), 1, "emissive")])
        with pytest.raises(P.PtError) as e:
            r.set_scene([_sphere((0, 0, -3), -1, "diffuse")])
        assert e.value.code == -1 and "scene object 0" in str(e.value) and "radius" in str(e.value)
        assert len(r.scene()) == 1 and r.scene()[0]["material"] == P.MATERIAL_EMISSIVE
        r.set_scene(None)
        assert r.scene().tobytes() == table.tobytes()
    finally:
        r.close()


def _inner_spheres(radius, dist):
    """26 spheres around the mirror sphere's centre on its camera side (+z), `dist` from it."""
    c = np.array(P_BUILTIN_MIRROR_CENTRE, dtype=np.float64)
    out = []
    for k in range(26):
        th = 0.15 + 1.2 * (k % 13) / 12.0
        ph = 2 * np.pi * k / 26.0 + (0.3 if k >= 13 else 0.0)
        d = np.array([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)])
        out.append(_sphere(tuple(c + dist * d), radius, "diffuse", (1.5, 0.2, 0.2)))
    return out


P_BUILTIN_MIRROR_CENTRE = (0.74795, -0.55, -4.3816)


def test_32_objects_inside_the_mirror_change_nothing(ptmi_lib):
    P = ptmi_lib
    table = P.builtin_scene()
    assert table[MIRROR]["material"] == P.MATERIAL_SPECULAR and table[MIRROR]["radius"] == np.float32(1.05)
    assert np.allclose(table[MIRROR]["centre"], P_BUILTIN_MIRROR_CENTRE)
    # the built-in rows first, then 26 spheres: reach 0.85 < 1.05, so no ray gets there (no ray enters a specular sphere)
    inside = np.concatenate([table, P.scene_array(_inner_spheres(0.05, 0.8))])
    assert len(inside) == 32
    poking = np.concatenate([table, P.scene_array(_inner_spheres(0.4, 0.8))])      # reach 1.2 > 1.05
    for kw in ({"const": (0.6, 0.9, 1.3)}, {"layers": nif_assets.synthetic_nif()}):
        rec0, film0, _ = _render(P, 128, 96, spp=4, **kw)
        rec1, film1, _ = _render(P, 128, 96, scene=inside, spp=4, **kw)
        assert rec0.tobytes() == rec1.tobytes() and film0.tobytes() == film1.tobytes()
        rec2, film2, _ = _render(P, 128, 96, scene=poking, spp=4, **kw)
        assert film2.tobytes() != film0.tobytes()
        assert np.count_nonzero(np.any(film2 != film0, axis=1)) > 100


# A mirror sphere that fills the view (angular radius asin(2.5 / 3) = 56 degrees > the 51 degrees of the image's corners): every
# camera ray meets it at least 20 degrees off grazing.  Near grazing, the hit point's rounding can leave a reflected ray inside
# the sphere by more than the intersection epsilon (1e-5), which then bounces inside until the stack is full -- the reference's
# numerics (codelets.cpp, light::Sphere), kept here -- so a mirror whose silhouette is in view is not L at every pixel.
MIRROR_SCENE = [_sphere((0.0, 0.0, -3.0), 2.5, "specular")]


def test_mirror_under_a_constant_sky_is_the_sky_exactly(ptmi_lib):
    P = ptmi_lib
    rec, film, st = _render(P, 128, 96, scene=MIRROR_SCENE, const=L_SKY, spp=8, depth=6, roulette=6)
    assert np.all(film == np.float32([L_SKY[2], L_SKY[1], L_SKY[0]]))      # BGR
    assert np.all(rec["pathLength"] == 16)                                   # 8 paths of length 2: one bounce, then the sky
    assert st[0]["escaped"] == st[0]["paths"] == 128 * 96 * 8 and st[0]["segments"] == 2 * st[0]["paths"]


def _silhouette_mask(W, H, centre, radius, margin):
    """Pixels whose camera ray (fov 90: tan = 1) passes at least `margin` (radians, about) inside the sphere's silhouette."""
    c = np.arange(W) + 0.5
    r = np.arange(H) + 0.5
    px = (2 * c - W) / W
    py = -((2 * r - H) / H) * (H / W)
    d = np.stack(np.broadcast_arrays(px[None, :], py[:, None], -np.ones((H, W))), -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    cc = np.array(centre) / np.linalg.norm(centre)
    ang = np.arccos(np.clip(d @ cc, -1, 1))
    return ang < np.arcsin(radius / np.linalg.norm(centre)) - margin


@pytest.mark.parametrize("roulette", [8, 1])
def test_furnace(ptmi_lib, roulette):
    """One diffuse sphere of colour c under a constant L: inside its silhouette E[cos theta] = 1/2, so the mean is c L / 2."""
    P = ptmi_lib
    W, H, spp = 128, 96, 64
    c, L = np.array([0.8, 0.5, 0.25]), 2.0
    centre = (0.0, 0.0, -3.0)
    rec, film, st = _render(P, W, H, scene=[_sphere(centre, 1.0, "diffuse", tuple(c))], const=(L, L, L), spp=spp, depth=8,
                            roulette=roulette, precision=P.SAMPLES_FLOAT)
    mask = _silhouette_mask(W, H, centre, 1.0, 0.03).reshape(-1)
    n = int(mask.sum()) * spp
    assert n > 50000
    bgr = film[mask].astype(np.float64)
    mean = bgr.mean(axis=0)[::-1]                                          # RGB
    stop = float(np.float16(0.3))
    second = 1.0 / 3.0 / (1.0 - stop) if roulette == 1 else 1.0 / 3.0   # E[(c L cos)^2 rr^2 ...] / (c L)^2
    sigma = c * L * np.sqrt((second - 0.25) / n)
    assert np.all(np.abs(mean - c * L / 2) < 5 * sigma), (mean, c * L / 2, sigma)
    if roulette == 1:
        assert st[0]["escaped"] < st[0]["paths"]   # roulette really stopped some paths


def test_emitting_shell(ptmi_lib):
    """The camera inside an emissive sphere (radius 50) with an inner diffuse sphere in view: no path escapes, with a NIF."""
    P = ptmi_lib
    W, H, spp = 128, 96, 32
    E = np.array([0.5, 1.0, 2.0])
    c = np.array([0.75, 0.5, 0.25])
    centre = (0.0, 0.0, -3.0)
    scene = [_sphere((0, 0, 0), 50.0, "emissive", tuple(E)), _sphere(centre, 1.0, "diffuse", tuple(c))]
    rec, film, st = _render(P, W, H, scene=scene, spp=spp, depth=8, roulette=8, precision=P.SAMPLES_FLOAT)
    assert st[0]["escaped"] == 0
    assert st[0]["segments"] == int(rec["pathLength"].astype(np.int64).sum())
    assert np.all(rec["pathLength"] >= spp)                                  # the EMIT entry counts
    outside = ~_silhouette_mask(W, H, centre, 1.0, -0.05).reshape(-1)        # rays that cannot touch the inner sphere
    assert outside.sum() > 5000
    assert np.all(rec["pathLength"][outside] == spp)
    assert np.all(film[outside] == np.float32(E[::-1]))
    mask = _silhouette_mask(W, H, centre, 1.0, 0.03).reshape(-1)
    n = int(mask.sum()) * spp
    mean = film[mask].astype(np.float64).mean(axis=0)[::-1]
    sigma = c * E * np.sqrt((1.0 / 3.0 - 0.25) / n)
    assert np.all(np.abs(mean - c * E / 2) < 5 * sigma), (mean, c * E / 2, sigma)
    # the same scene under a constant environment: nothing escapes either, and the film is the same
    _, film_c, st_c = _render(P, W, H, scene=scene, const=(9.0, 9.0, 9.0), spp=spp, depth=8, roulette=8, precision=P.SAMPLES_FLOAT)
    assert st_c[0]["escaped"] == 0 and film_c.tobytes() == film.tobytes()


def _cam_dirs(p):
    d = np.stack([p["cam"][:, 0].astype(np.float64), p["cam"][:, 1].astype(np.float64), -np.ones(len(p))], -1)
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def test_geometry_through_trace_paths(ptmi_lib):
    P = ptmi_lib
    W, H = 200, 150
    # a mirror sphere
    c, rad = np.array([0.3, -0.2, -3.5]), 1.2
    p = _paths(P, W, H, scene=[_sphere(tuple(c), rad, "specular")])
    d = _cam_dirs(p)
    tc = d @ c
    dist = np.sqrt(np.maximum(c @ c - tc * tc, 0))
    keep = np.abs(dist - rad) > 1e-4
    hit = (dist < rad) & (tc > 0)
    assert 200 < np.count_nonzero(hit & keep) < np.count_nonzero(keep) - 200
    assert np.array_equal((p["length"] >= 2)[keep], hit[keep])
    assert np.all(p["length"][~hit & keep] == 1) and np.all(p["escaped"][~hit & keep] == 1)
    # reflections away from grazing (|cos| > 0.3 at the hit: see MIRROR_SCENE; the rounding of the camera ray's hit distance
    # grows as the discriminant shrinks) bounce once and escape
    cos_in = np.sqrt(np.maximum(1 - (dist / rad) ** 2, 0))
    h = hit & (cos_in > 0.3)
    assert np.count_nonzero(h) > 200
    assert np.all(p["escaped"][h] == 1) and np.all(p["length"][h] == 2)
    t = tc[h] - np.sqrt(rad * rad - dist[h] ** 2)
    x = d[h] * t[:, None]
    nrm = (x - c) / rad
    refl = d[h] - 2 * np.sum(d[h] * nrm, -1, keepdims=True) * nrm
    assert np.max(np.abs(p["dir"][h] - refl)) < 1e-5
    assert np.all(p["throughput"][h] == 1.0)
    # a disc with a tilted normal (normalised by the library)
    n_in = np.array([0.3, 1.0, 0.5], dtype=np.float32)
    cd, rd = np.array([0.2, -0.6, -3.0]), 1.5
    disc = [{"shape": "disc", "centre": tuple(cd), "normal": tuple(n_in), "radius": rd, "material": "specular"}]
    r = P.Renderer(W, H)
    try:
        r.set_scene(disc)
        stored = r.scene()[0]["normal"]
    finally:
        r.close()
    x_, y_, z_ = (np.float32(t) for t in n_in)
    assert np.array_equal(stored, n_in / np.sqrt((x_ * x_ + y_ * y_) + z_ * z_))   # n / sqrtf(dot(n, n)) in binary32
    p = _paths(P, W, H, scene=disc)
    d = _cam_dirs(p)
    n = stored.astype(np.float64)
    t = (cd @ n) / (d @ n)
    x = d * t[:, None]
    rr = np.linalg.norm(x - cd, axis=-1)
    keep = np.abs(rr - rd) > 1e-4
    hit = (t > 0) & (rr <= rd)
    assert 200 < np.count_nonzero(hit & keep) < np.count_nonzero(keep) - 200
    assert np.array_equal((p["length"] >= 2)[keep], hit[keep])
    h = hit & keep & (np.abs(d @ n) > 0.3)
    assert np.count_nonzero(h) > 200
    assert np.all(p["escaped"][h] == 1) and np.all(p["length"][h] == 2)
    refl = d[h] - 2 * (d[h] @ n)[:, None] * n
    assert np.max(np.abs(p["dir"][h] - refl)) < 1e-5 and np.all(p["throughput"][h] == 1.0)
    # an emitter: escaped == 2, length 1, throughput 1
    p = _paths(P, W, H, scene=[_sphere(tuple(c), rad, "emissive", (3, 3, 3))])
    d = _cam_dirs(p)
    tc = d @ c
    dist = np.sqrt(np.maximum(c @ c - tc * tc, 0))
    keep = np.abs(dist - rad) > 1e-4
    hit = (dist < rad) & (tc > 0)
    assert np.array_equal((p["escaped"] == 2)[keep], hit[keep])
    assert np.all(p["escaped"][keep & ~hit] == 1)
    assert np.all(p["length"][hit & keep] == 1) and np.all(p["throughput"][hit & keep] == 1.0)


def test_sharing_and_memo_on_a_scene_with_an_emitter(ptmi_lib):
    P = ptmi_lib
    table = P.builtin_scene()
    light = P.scene_array([_sphere((1.2, 1.6, -3.5), 0.6, "emissive", (6, 5, 4))])
    first = np.concatenate([table, light])
    second = np.concatenate([table[:3], light, table[3:]])
    kw = dict(scene=first, scene_after=second, spp=6, steps=4)
    _, off, st = _render(P, 128, 96, **kw)
    _, step, _ = _render(P, 128, 96, mode="step", **kw)
    _, batch, _ = _render(P, 128, 96, mode="batch", **kw)
    _, memo, _ = _render(P, 128, 96, memo=1 << 28, **kw)
    assert off.tobytes() == step.tobytes() == batch.tobytes() == memo.tobytes()
    assert all(s["escaped"] > 0 for s in st)
    _, plain, _ = _render(P, 128, 96, spp=6, steps=4)
    assert plain.tobytes() != off.tobytes()


def _exe():
    exe = os.path.join(HOST, "ipu_trace")
    if not os.path.exists(exe):
        pytest.fail("ipu_trace has not been built (__graft_entry__.build)")
    return exe


def _read_exr(path, W, H):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    L = C.CDLL(os.path.join(HOST, "libpthost.so"))
    L.pth_read_exr.argtypes = [C.c_char_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    film = np.zeros((H, W, 3), dtype=np.float32)
    ww, hh = C.c_size_t(), C.c_size_t()
    assert L.pth_read_exr(str(path).encode(), film.ctypes.data, film.size, C.byref(ww), C.byref(hh)) == 0
    return film


def test_cli_scene(tmp_path):
    exe = _exe()
    W, H = 96, 64
    mirror = tmp_path / "mirror.json"
    mirror.write_text(json.dumps({"objects": [{"shape": "sphere", "centre": [0, 0, -3], "radius": 2.5, "material": "specular"}]}))
    r = subprocess.run([exe, "--assets", str(tmp_path), "--constant-env", ",".join(str(x) for x in L_SKY), "--scene", str(mirror),
                        "-w", str(W), "-h", str(H), "-s", "8", "--samples-per-step", "8", "--max-path-length", "6",
                        "--roulette-depth", "6", "-o", str(tmp_path / "mirror.png"), "--save-interval", "1"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    film = _read_exr(tmp_path / "mirror.exr", W, H)
    assert np.all(film == np.float32([L_SKY[2], L_SKY[1], L_SKY[0]]))
    # an emitter scene over two logical devices on one GPU equals one device, bit for bit
    assets = tmp_path / "assets.extra"
    assets.mkdir()
    nif_assets.write_metadata(str(assets / "nif_metadata.txt"))
    nif_assets.write_ptnif(str(assets / "converted.ptnif"), nif_assets.synthetic_nif(), 12)
    lit = tmp_path / "lit.json"
    lit.write_text(json.dumps({"objects": [
        {"shape": "sphere", "centre": [0, 0, -3], "radius": 1, "material": "diffuse", "colour": [1.6, 1.6, 1.6]},
        {"shape": "disc", "centre": [0, -1.6, -5], "normal": [0, 1, 0], "radius": 3.5, "material": "specular"},
        {"shape": "sphere", "centre": [2, 3, -4], "radius": 0.3, "material": "emissive", "emission": [8, 8, 8]},
        {"shape": "sphere", "centre": [-1.5, 0.5, -3], "radius": 0.5, "material": "refractive", "colour": [0.9, 0.9, 0.7]}]}))
    films = []
    for name, extra in (("one", ["--ipus", "1"]), ("two", ["--ipus", "2", "--devices", "0,0"])):
        r = subprocess.run([exe, "--assets", str(assets), "--scene", str(lit), "-w", str(W), "-h", str(H), "-s", "12",
                            "--samples-per-step", "4", "--max-path-length", "7", "-o", str(tmp_path / (name + ".png")),
                            "--save-interval", "3"] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
        films.append(_read_exr(tmp_path / (name + ".exr"), W, H))
    assert films[0].tobytes() == films[1].tobytes()
    assert np.count_nonzero(films[0]) > 0
