"""Feathered seams: properties of the numpy model (tests/feather_model.py) on oracle inputs. No GPU: what the device
is held to in tests/test_gpu_feather.py is checked here for being what the definition promises."""
import numpy as np
import pytest

import envutil_amd as ea
import euo
import jobs
import feather_model as fm


def target(**kw):
    return ea.arguments(ea.SPHERICAL, 96, 40, 120.0, synopsis="feather", **kw)


def pair(nch, degree=1, yaws=(-14.0, 15.0), brightens=(1.0, 1.0), constant=None, masked=(-1, -1)):
    out = []
    for k in range(2):
        img = jobs.synth_image(48, 32, nch, seed=40 + k)
        if constant is not None:
            img[:, :, :] = constant
        out.append(fm.Facet(euo.RECTILINEAR, 48, 32, 50.0, img, degree, yaw=yaws[k], pitch=2.0 * k - 1.0, roll=3.0 * k,
                            brighten=brightens[k], masked=masked[k]))
    return out


@pytest.mark.parametrize("nch", [3, 4])
def test_where_one_facet_hits_the_frame_is_the_panoramas(nch):
    a = target(spline_degree=1)
    fs = pair(nch)
    frame, qsum, count = fm.model_frame(a, fs, nch, details=True)
    pano = jobs.oracle_render(ea.arguments(ea.SPHERICAL, 96, 40, 120.0, spline_degree=1), [f.o for f in fs])
    for n in (0, 1, 2):
        assert (count == n).sum() > 50, f"{(count == n).sum()} pixels with {n} facets"
    sel = count <= 1
    d = jobs.bits(frame)[sel] != jobs.bits(pano)[sel]
    assert not d.any(), f"{int(d.sum())} values differ where at most one facet hits"
    # and in the overlap the two differ: feathering does something
    assert (jobs.bits(frame)[count == 2] != jobs.bits(pano)[count == 2]).mean() > 0.5
    assert np.isfinite(frame).all()


def test_two_constant_facets_ramp_monotonically_between_their_values():
    """brighten 1 and 1.25 over the constant 0.5 (degree 0: the facets' pixels are 0.5 and 0.625 exactly). Along a row
    through the overlap, from the last pixel only the left facet covers to the first only the right one covers, the
    values never fall; those two pixels hold the facets' own values, and everything between lies between them."""
    a = target(spline_degree=0)
    fs = pair(3, degree=0, yaws=(-14.0, 15.0), brightens=(1.0, 1.25), constant=0.5)
    for f in fs:
        f.o.s.pitch = f.o.s.roll = f.white.s.pitch = f.white.s.roll = 0.0
    frame, qsum, count = fm.model_frame(a, fs, 3, details=True)
    rows = 0
    for y in range(8, 32):
        two = np.flatnonzero(count[y] == 2)
        if len(two) < 8:
            continue
        x0, x1 = two[0] - 1, two[-1] + 1
        assert (count[y, x0:x1 + 1] == np.r_[1, np.full(len(two), 2), 1]).all(), "the overlap is one run of pixels"
        v = frame[y, x0:x1 + 1, :]
        assert (v[0] == np.float32(0.5)).all() and (v[-1] == np.float32(0.625)).all()
        assert (np.diff(v.astype(np.float64), axis=0) >= 0).all(), f"row {y} is not monotone: {v[:, 0]}"
        assert (v[1:-1] > 0.5).all() and (v[1:-1] < 0.625).all()
        assert (v[:, 0] == v[:, 1]).all() and (v[:, 0] == v[:, 2]).all()
        rows += 1
    assert rows >= 10


def test_mask_for_frames_are_normalised_weights_that_sum_to_one():
    """--mask_for N paints facet N white and the others black: the feathered frame is then facet N's normalised blend
    weight. Over N the weights sum to 1 wherever a facet hits, within n * 2^-23: one rounding per quotient e / qsum
    (2^-24 of the weight each, 2^-24 in the sum) and n - 1 roundings of qsum (2^-24 each); products with the paint 1
    and sums with 0 are exact."""
    a = target(spline_degree=1, feather=9.0)
    n = 3
    geo = [dict(yaw=-16.0, pitch=1.0), dict(yaw=6.0, pitch=-2.0, roll=4.0), dict(yaw=20.0, pitch=3.0)]
    total = np.zeros((40, 96), np.float64)
    hits = None
    for paint in range(n):
        fs = [fm.Facet(euo.RECTILINEAR, 48, 32, 50.0, jobs.synth_image(48, 32, 3, seed=60 + k), 1,
                       masked=1 if k == paint else 0, **geo[k]) for k in range(n)]
        frame, qsum, count = fm.model_frame(a, fs, 3, details=True)
        assert (frame[:, :, 0] == frame[:, :, 1]).all() and (frame[:, :, 0] == frame[:, :, 2]).all()
        assert (frame >= 0).all() and (frame <= 1).all()
        total += frame[:, :, 0]
        hits = count
    assert (hits == 3).sum() > 20 and (hits == 2).sum() > 50 and (hits == 0).sum() > 50
    err = np.abs(total - 1.0)[hits > 0]
    assert err.max() <= n * 2.0 ** -23, f"weights sum to 1 +- {err.max():.3g}"
    assert (total[hits == 0] == 0).all()


def test_edge_weight_floor_clamp_and_borderless_axes():
    sx = np.array([-0.5, -0.4999, 0.0, 7.5, 23.5, 46.0, 47.5, 47.6], np.float32)
    sy = np.full(8, 15.5, np.float32)
    e = fm.edge_weight(sx, sy, (48, 32), (True, True), 8.0)
    assert e[0] == fm.FLOOR and e[-1] == fm.FLOOR and e[-2] == fm.FLOOR       # on and beyond the border
    assert e[3] == 1.0 and e[4] == 1.0 and e[2] == np.float32(0.0625)
    assert (e >= fm.FLOOR).all() and (e <= 1).all()
    # default width: half the shorter side - the ramp reaches the centre and nowhere else
    e = fm.edge_weight(np.float32([23.5, 23.5]), np.float32([15.5, 15.0]), (48, 32), (True, True))
    assert e[0] == 1.0 and e[1] < 1.0
    assert (fm.edge_weight(sx, sy, (48, 32), (False, False), 8.0) == 1).all()
    assert (fm.edge_weight(sx, np.float32([0.0] * 8), (48, 32), (True, False), 8.0) == fm.edge_weight(sx, sy, (48, 32), (True, False), 8.0)).all()
    assert fm.borders(euo.SPHERICAL, 360.0, 64, 32) == (False, False)
    assert fm.borders(euo.SPHERICAL, 360.0, 64, 20) == (False, True)
    assert fm.borders(euo.CYLINDRICAL, 360.0, 64, 20) == (False, True)
    assert fm.borders(euo.CUBEMAP, 90.0, 16, 96) == (False, False)
    assert fm.borders(euo.FISHEYE, 360.0, 32, 32) == (False, False)
    assert fm.borders(euo.RECTILINEAR, 60.0, 48, 32) == (True, True)
