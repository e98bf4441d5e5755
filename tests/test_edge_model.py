"""tests/edge_model.py against itself, no GPU: the brute-force squared distance against the separable two-pass
restatement, the root against float64, and the properties of the bilinear sample the device tests rely on."""
import numpy as np
import pytest

import edge_model as em

SHAPES = [(1, 1), (1, 9), (9, 1), (5, 3), (33, 17), (67, 31)]


def planes(w, h):
    """(name, outside) at the densities 0, 1/500 and 1/2, and all outside"""
    rng = np.random.default_rng(w * 1000 + h)
    yield "none", np.zeros((h, w), bool)
    yield "1/500", rng.uniform(size=(h, w)) < 1.0 / 500.0
    yield "1/2", rng.uniform(size=(h, w)) < 0.5
    yield "all", np.ones((h, w), bool)


@pytest.mark.parametrize("cyclic", [False, True])
@pytest.mark.parametrize("w,h", SHAPES)
def test_brute_force_equals_two_passes(w, h, cyclic):
    for name, out in planes(w, h):
        a, b = em.d2_brute(out, cyclic), em.d2_two_pass(out, cyclic)
        assert a.dtype == np.int32 and (a == b).all(), (name, w, h, cyclic)
        if name == "none":
            assert (a == 2 ** 31 - 1).all()
        if name == "all":
            assert (a == 0).all()
        assert (a[out] == 0).all() and (a[~out] > 0).all()


def test_one_sparse_plane_has_outside_pixels():
    """the density 1/500 is not the empty plane at the largest shape"""
    out = dict(planes(67, 31))["1/500"]
    assert 0 < out.sum() < 20


def test_cyclic_rows_reach_round_the_seam():
    out = np.zeros((3, 10), bool)
    out[1, 0] = True
    plain, cyc = em.d2_brute(out, False), em.d2_brute(out, True)
    assert plain[1, 9] == 81 and cyc[1, 9] == 1 and cyc[0, 9] == 2 and cyc[1, 5] == 25 and cyc[1, 6] == 16
    assert (cyc <= plain).all()


def test_outside_is_an_ieee_compare():
    tiny = np.float32(1.401298464324817e-45)
    a = np.array([[np.nan, -1.0, -0.0, 0.0, tiny, 1e-30, 1.0]], np.float32)
    assert em.outside(a).tolist() == [[True, True, True, True, False, False, False]]


def test_root_is_correctly_rounded():
    d2 = np.concatenate([np.arange(0, 2 ** 16 + 1, dtype=np.int64), [2 ** 31 - 1]]).astype(np.int32)
    got = em.root(d2)
    assert got.dtype == np.float32
    # the operand: int32 -> float32 to nearest (exact below 2^24; 2^31 - 1 becomes 2^31)
    x = d2.astype(np.float32)
    assert x[-1] == np.float32(2.0 ** 31) and (x[:-1].astype(np.int64) == d2[:-1]).all()
    # correctly rounded: the float32 nearest the float64 root (which is itself within half an ulp of float64 of the
    # true root - 29 bits finer than float32, and no root of an integer up to 2^31 lies that close to a float32 tie)
    want = np.sqrt(x.astype(np.float64)).astype(np.float32)
    assert (got.view(np.uint32) == want.view(np.uint32)).all()
    exact = np.arange(0, 257, dtype=np.int64)
    assert (em.root((exact * exact).astype(np.int32)) == exact.astype(np.float32)).all()


def test_sample_at_centres_and_between():
    D = np.array([[0, 1, 2, 3], [1, 1, 2, 3], [2, 2, 2, 3]], np.float32)
    yy, xx = np.mgrid[0:3, 0:4]
    s = em.sample(D, xx.astype(np.float32), yy.astype(np.float32), False)
    assert (s == D - np.float32(0.5)).all()
    # half way between two columns; beyond the last centre the indices clamp, or wrap
    assert em.sample(D, [0.5], [0.0], False)[0] == np.float32(0.0)
    assert em.sample(D, [3.25], [0.0], False)[0] == np.float32(2.5)
    assert em.sample(D, [3.25], [0.0], True)[0] == np.float32(3.0 + (0.0 - 3.0) * 0.25 - 0.5)
    assert em.sample(D, [-0.5], [0.0], False)[0] == np.float32(-0.5)
    assert em.sample(D, [-0.5], [0.0], True)[0] == np.float32(3.0 + (0.0 - 3.0) * 0.5 - 0.5)
    assert em.sample(D, [1.0], [2.4], False)[0] == em.sample(D, [1.0], [2.0], False)[0]


def test_weight_without_a_plane_is_feathers():
    import feather_model as fm
    rng = np.random.default_rng(5)
    sx, sy = rng.uniform(-0.5, 47.5, (9, 11)).astype(np.float32), rng.uniform(-0.5, 31.5, (9, 11)).astype(np.float32)
    fc = dict(sx=sx, sy=sy, win=(48, 32), border=(True, True))
    assert (em.edge_weight(fc, 6.0) == fm.edge_weight(sx, sy, (48, 32), (True, True), 6.0)).all()
    # a plane without an outside pixel leaves the window ramp alone; one with a hole pulls the weight down to the floor
    far = em.distance_plane(np.ones((32, 48), np.float32))
    assert (em.edge_weight(dict(fc, dist=far, cyclic=False), 6.0) == em.edge_weight(fc, 6.0)).all()
    alpha = np.ones((32, 48), np.float32)
    alpha[10:20, 10:30] = 0
    e = em.edge_weight(dict(fc, dist=em.distance_plane(alpha), cyclic=False), 6.0)
    inside = (sx > 11) & (sx < 28) & (sy > 11) & (sy < 18)
    assert inside.any() and (e[inside] == fm.FLOOR).all() and (e <= em.edge_weight(fc, 6.0)).all()
