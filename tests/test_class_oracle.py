"""The property the NIF stage's class level rests on, against the strict oracle on the CPU: coordinates of one class
(ptmi_share_plan.h: class_coord -- the bits of (float)half(x), x = (coord - 1) * 2, for 2^-14 <= |x| <= 2) give identical bytes
from Nif.infer, at E = 12 and at E = 16, where u = 0 (x = -2) overflows to infinity in its last feature.  The class key is
numpy's (tests/class_key_model.py)."""
import numpy as np
import pytest

from ipu_path_trace_amd import nif_assets
from tests.class_key_model import class_coord, class_key, class_mates

META = nif_assets.URBAN_ALLEY_META


@pytest.mark.parametrize("emb", [12, 16])
def test_one_class_one_output(oracle, emb):
    rng = np.random.default_rng(7)
    nif = oracle.Nif(nif_assets.synthetic_nif(hidden=64, layer_count=3, embedding_dim=emb), emb, META["max"], nif_assets.folded_mean())
    ua, ub = class_mates(rng, 512)
    va, vb = class_mates(rng, 512)
    va, vb = va[::-1].copy(), vb[::-1].copy()
    assert int((ua.view(np.uint32) != ub.view(np.uint32)).sum()) > 400 and int((va.view(np.uint32) != vb.view(np.uint32)).sum()) > 400
    assert np.array_equal(class_key(ua, va), class_key(ub, vb))
    out_a, out_b = nif.infer(ua, va), nif.infer(ub, vb)
    assert out_a.tobytes() == out_b.tobytes()
    # u = 0: x = -2, and at E = 16 the last feature's argument -2 x 2^15 is past the largest half
    feats = oracle.nif_encode(emb, 0.0, 0.5)
    assert np.isnan(feats[emb - 1]) == (emb == 16)
    # the other way round, as a guard against a test that cannot fail: a neighbouring class gives another output somewhere
    uc = (ua.view(np.int32) + np.int32(1 << 14)).view(np.float32)
    differs = class_coord(uc) != class_coord(ua)
    assert differs.sum() > 400
    out_c = nif.infer(uc, va)
    assert (out_c[differs] != out_a[differs]).any()
