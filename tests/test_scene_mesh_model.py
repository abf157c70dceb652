"""The float64 model of mesh scenes (tests/scene_mesh_model.py) on the CPU: the expansion is what it says, the model over it is
scene_poly_model's, and the cases used on the device leave at most the project's cap of fragile paths."""
import numpy as np
import pytest

from tests import scene_model as M
from tests import scene_mesh_model as MM
from tests import scene_poly_model as PM


def test_expansion_lists_every_triangle_in_index_order():
    objs = MM.world_scene("moved")
    rows, origin = MM.expand(objs)
    counts = [len(o["triangles"]) if o["shape"] == "mesh" else 1 for o in objs]
    assert counts == [320, 1, 128, 1] and len(rows) == sum(counts) and np.array_equal(origin, np.repeat(np.arange(4), counts))
    ball = objs[0]
    for j in (0, 17, 319):
        r = rows[j]
        assert r["shape"] == "triangle" and r["material"] == "refractive" and r["colour"] == ball["colour"]
        assert np.array_equal(np.float32(r["vertices"]), np.float32(ball["vertices"])[ball["triangles"][j]])
    t = MM.stored(objs)
    assert len(t) == 450 and t["shape"].tolist() == [2] * 320 + [3] + [2] * 128 + [0]
    # a fifth of a unit across, and unit normals made as the library makes a triangle's
    v = np.float32(ball["vertices"])
    assert 0.19 < np.ptp(v, axis=0).max() < 0.21
    assert np.allclose(np.linalg.norm(t["normal"][:320].astype(np.float64), axis=1), 1.0, atol=1e-6)


def test_the_model_sees_both_meshes_and_every_outcome(oracle):
    u, v, ss, cam, plain, fragile, spread = MM.case("none", False)
    origin = MM.expand(MM.world_scene("none"))[1]
    first = PM.first_hit(MM.stored(MM.world_scene("none")), None, cam)[0]               # (the trace's own `hits` are int8: they serve
    rows = np.where(first >= 0, origin[np.maximum(first, 0)], -1)                       # its run-to-run comparison, not as indices)
    assert np.count_nonzero(rows == 0) > 30 and np.count_nonzero(rows == 2) > 100      # the ball and the floor are seen
    assert set(np.unique(plain["escaped"]).tolist()) == {0, 1, 2} and plain["length"].max() >= 4


@pytest.mark.parametrize("camera,half", MM.CASES)
def test_fragile_share_of_the_device_cases_stays_under_the_cap(oracle, camera, half):
    u, v, ss, cam, plain, fragile, spread = MM.case(camera, half)
    print("%s / %s: %d paths, fragile %.2f %%" % (camera, "half" if half else "float", len(u), 100 * fragile.mean()))
    assert len(u) == 1024 and fragile.mean() <= M.FRAGILE_CAP
    # the rule is not vacuous on these cases: the model against itself passes it, and a second plain run is the first
    same, ratio = PM.compare(plain, plain, fragile, spread)
    assert same and ratio == 0.0
