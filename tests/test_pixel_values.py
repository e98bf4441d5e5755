"""tests/pixel_values.py itself: the classes hold what their names say, the alpha plane meets every gate in every kind
of 16-pixel group, and the two comparisons fail on what they must fail on."""
import numpy as np
import pytest

import pixel_values as pv


def test_classes_hold_what_they_say():
    h, w, n = 64, 96, 3
    imp = pv.impulse(h, w, n)
    lit = (imp != 0).any(axis=2)
    assert 1 <= lit.sum() <= 6 and imp[lit].min() >= 0.5 and imp[lit].max() <= 4.0
    hd = pv.hdr(h, w, n)
    assert hd.min() >= np.float32(1e-6) and hd.max() <= np.float32(6e4) and (hd < 1e-4).mean() > 0.1 and (hd > 1e3).mean() > 0.1
    sg = pv.signed(h, w, n)
    bits = sg.view(np.uint32)
    assert 0.27 < (bits == 0).mean() < 0.33 and 0.08 < (bits == 0x80000000).mean() < 0.12
    assert sg.min() < -900 and sg.max() > 900
    dn = pv.denormal(h, w, n)
    assert pv.is_denormal(dn).all() and (dn < 0).any() and (dn > 0).any()
    bg = pv.big(h, w, n)
    assert np.isfinite(bg).all() and np.abs(bg).max() > 9e36 and (bg < 0).any() and (bg > 0).any()
    nf = pv.nonfinite(h, w, n)
    odd = ~np.isfinite(nf) | (np.abs(nf) > 1e38)
    assert 0.002 < odd.mean() < 0.01
    assert np.isnan(nf).any() and (nf == np.inf).any() and (nf == -np.inf).any() and (nf == np.float32(3e38)).any()
    for cls in pv.CLASSES:
        a, b = pv.make(cls, 9, 7, 4, seed=5), pv.make(cls, 9, 7, 4, seed=5)
        assert a.dtype == np.float32 and a.shape == (9, 7, 4) and (a.view(np.uint32) == b.view(np.uint32)).all()


def test_alpha_plane_meets_every_gate():
    a = pv.alpha_plane(64, 96)
    bits = a.view(np.uint32)
    gate = pv.ALPHA_GATE
    assert (bits == 0).any() and (bits == 0x80000000).any() and pv.is_denormal(a).any()
    for v in (np.nextafter(gate, np.float32(0)), gate, np.nextafter(gate, np.float32(1)), np.float32(1.0)):
        assert (a == v).any(), v
    assert ((a > 0) & (a < 1)).any() and (a > 1).any() and (a < 0).any()
    assert min(pv.group_kinds(a)) > 0
    img = pv.with_alpha(pv.hdr(64, 96, 4), associated=True)
    assert (img[:, :, 3].view(np.uint32) == bits).all() and (img[:, :, :3][a == 0] == 0).all()
    assert pv.with_alpha(pv.hdr(8, 8, 3)).shape == (8, 8, 3)


@pytest.mark.parametrize("cls", pv.FINITE)
def test_scaled_unit_lies_around_the_unit_interval(cls):
    v = pv.scaled_unit(cls, 40, 50, 2)
    b = v.view(np.uint32)
    assert np.isfinite(v).all() and (b == 0).any() and (b == 0x80000000).any() and (v == 1).any() and (v > 1).any()
    assert ((v > 0) & (v < 1)).any()


def test_the_comparisons_fail_where_they_must():
    ref = np.float32([0.0, 1.0, np.inf, np.nan, 1e-40])
    pv.assert_bits(ref[[0, 1, 2, 4]], ref[[0, 1, 2, 4]].copy())
    pv.assert_bits_nan(ref, ref.copy())
    other_nan = ref.copy()
    other_nan.view(np.uint32)[3] = 0xFFC01234                # another sign and payload: outside the contract
    pv.assert_bits_nan(other_nan, ref)
    with pytest.raises(AssertionError):
        pv.assert_bits(other_nan, ref)
    for i, v in ((0, -0.0), (2, -np.inf), (4, 0.0), (1, np.nan), (3, 1.0)):
        bad = ref.copy()
        bad[i] = v
        with pytest.raises(AssertionError):
            pv.assert_bits_nan(bad, ref)
    with pytest.raises(AssertionError):
        pv.assert_bits_nan(ref[:4], ref)
    with pytest.raises(AssertionError):
        pv.assert_exercised("denormal", np.float32([1e-40, 1.0]), 3)
    with pytest.raises(AssertionError):
        pv.assert_exercised("nonfinite", np.float32([np.nan, 1.0]), 1)
    pv.assert_exercised("nonfinite", np.float32([np.nan, np.inf, 1.0, 2.0]), 1)
