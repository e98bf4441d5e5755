"""eu_render5_kernel's first loop renders groups of 16x16 tiles from one run of the coordinate stage
(envutil_amd/csrc/eu_share_groups.h: the column mirror of a double row, the same rows of another cube
face). Which tiles share is decided from the bits of the tables the kernel reads: cube faces of 64 and
128 pixels form groups, faces of 96 and 41 must not - and every frame is the oracle's, bit for bit.
eu_hip_share_follower_tiles() counts the tiles the last launch rendered as followers, so that these
tests cannot pass without a single shared tile."""
import ctypes as C
import os

import numpy as np
import pytest

import devout
import envutil_amd as ea
import euo
import jobs
from test_gpu_parity import assert_bits, make_pair

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def staged_everywhere():
    old = {k: os.environ.get(k) for k in ("EU_HIP_R4", "EU_HIP_SHARE")}
    os.environ["EU_HIP_R4"] = "1"
    os.environ.pop("EU_HIP_SHARE", None)
    yield
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


@pytest.fixture(scope="module")
def latlon():
    return {n: jobs.synth_image(512, 256, n) for n in (3, 4)}


def render(a, g, nch=None, r0=0, r1=None, band=None, what="frame"):
    """envutil_amd.render()'s frame, rendered into a guarded device buffer that is all fill word before the call
    (tests/devout.py): a tile a launch skips is not found rendered by the job before it, and a miss must be written"""
    return devout.rendered(what, a, g, nch, r0, r1, band=band)


def followers():
    f = ea.lib().eu_hip_share_follower_tiles
    f.restype = C.c_ulonglong
    return int(f())


@pytest.mark.parametrize("face", [64, 128])
@pytest.mark.parametrize("degree", [2, 3])
@pytest.mark.parametrize("nch", [3, 4])
def test_power_of_two_faces_share(latlon, face, degree, nch):
    o, g = make_pair(euo.SPHERICAL, 512, 256, 360.0, latlon[nch], degree)
    a = ea.arguments(ea.CUBEMAP, face, 6 * face, 90.0, spline_degree=degree)
    got = render(a, g, nch)
    n = followers()
    print(f"face {face} degree {degree} nch {nch}: follower tiles {n}")
    assert_bits(got, jobs.oracle_render(a, o), "pixels")
    assert n > 0


@pytest.mark.parametrize("face", [96, 41])
@pytest.mark.parametrize("degree", [2, 3])
def test_other_faces_do_not_share(latlon, face, degree):
    o, g = make_pair(euo.SPHERICAL, 512, 256, 360.0, latlon[3], degree)
    a = ea.arguments(ea.CUBEMAP, face, 6 * face, 90.0, spline_degree=degree)
    got = render(a, g, 3)
    n = followers()
    print(f"face {face} degree {degree}: follower tiles {n}")
    assert_bits(got, jobs.oracle_render(a, o), "pixels")
    assert n == 0


@pytest.mark.parametrize("tw,th,thfov", [(256, 128, 90.0), (224, 120, 100.0), (208, 120, 100.0), (200, 120, 100.0)])
@pytest.mark.parametrize("degree", [2, 3])
def test_rectilinear_width_multiple_of_16_or_not(latlon, tw, th, thfov, degree):
    """every row of a rectilinear target has its own latitude: only column mirrors can share, and only where the
    width is a multiple of 16 with an even number of tile columns (208 = 13 x 16 has a middle column). Whether
    the columns of 256 and 224 are mirror images by bits is for the tables to say: the count is printed"""
    o, g = make_pair(euo.SPHERICAL, 512, 256, 360.0, latlon[3], degree)
    a = ea.arguments(ea.RECTILINEAR, tw, th, thfov, spline_degree=degree)
    got = render(a, g, 3)
    n = followers()
    print(f"rectilinear {tw}x{th} hfov {thfov} degree {degree}: follower tiles {n}")
    assert_bits(got, jobs.oracle_render(a, o), "pixels")
    if tw in (208, 200):
        assert n == 0


@pytest.mark.parametrize("tprj,tw,th,thfov", [(ea.CUBEMAP, 64, 384, 90.0), (ea.RECTILINEAR, 208, 120, 100.0)])
@pytest.mark.parametrize("ypr", [(40, 0, 0), (0, 20, 0), (25, -10, 5)])
def test_yawed_and_pitched_targets(latlon, tprj, tw, th, thfov, ypr):
    o, g = make_pair(euo.SPHERICAL, 512, 256, 360.0, latlon[3], 3)
    a = ea.arguments(tprj, tw, th, thfov, yaw=ypr[0], pitch=ypr[1], roll=ypr[2], spline_degree=3)
    got = render(a, g, 3)
    print(f"target {tprj} ypr {ypr}: follower tiles {followers()}")
    assert_bits(got, jobs.oracle_render(a, o), f"pixels ypr {ypr}")


@pytest.mark.parametrize("face", [64, 128])
def test_partial_source_misses(face):
    """a 120 degree lat/lon window: tiles with misses, tiles without any hit"""
    img = jobs.synth_image(256, 128, 3)
    o, g = make_pair(euo.SPHERICAL, 256, 128, 120.0, img, 3)
    a = ea.arguments(ea.CUBEMAP, face, 6 * face, 90.0, spline_degree=3)
    got, ref = render(a, g), jobs.oracle_render(a, o)
    assert_bits(got, ref, "pixels")
    assert (ref == 0).any() and (ref != 0).any()


@pytest.mark.parametrize("face", [64, 128])
def test_row_ranges_cut_groups_and_bands(latlon, face):
    o, g = make_pair(euo.SPHERICAL, 512, 256, 360.0, latlon[3], 3)
    a = ea.arguments(ea.CUBEMAP, face, 6 * face, 90.0, spline_degree=3)
    ref = jobs.oracle_render(a, o)
    parts = [render(a, g, 3, r0, r1) for r0, r1 in ((0, 101), (101, 102), (102, 6 * face))]
    assert_bits(np.concatenate(parts, 0), ref, "row ranges")
    frame = np.zeros_like(ref)
    for k in range(3):
        band = (8, 3, k)
        rows = ea.band_frame_rows(6 * face, *band)
        frame[rows] = render(a, g, 3, 0, len(rows), band=band)
        assert followers() == 0
    assert_bits(frame, ref, "bands")


@pytest.mark.parametrize("mode", ["0", "m", "f"])
def test_switch_against_default(latlon, mode):
    o, g = make_pair(euo.SPHERICAL, 512, 256, 360.0, latlon[3], 3)
    a = ea.arguments(ea.CUBEMAP, 128, 768, 90.0, spline_degree=3)
    on = render(a, g)
    n_on = followers()
    os.environ["EU_HIP_SHARE"] = mode
    off = render(a, g)
    n_off = followers()
    print(f"EU_HIP_SHARE unset: {n_on} follower tiles, {mode}: {n_off}")
    assert_bits(on, off, f"EU_HIP_SHARE unset vs {mode}")
    assert n_on > 0
    if mode == "0":
        assert n_off == 0
    else:
        assert 0 < n_off < n_on
