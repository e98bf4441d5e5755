"""The distance plane of a source loaded with EU_LOAD_EDGES (eu_edges.hip) through eu_hip_source_edge_distance, bit
for bit against the brute-force model of tests/edge_model.py: the shapes at which the two passes change their path
(one column, one row, one wave of columns and just over, a row longer than a workgroup, a tall narrow plane), the alpha
patterns and values that decide inside and outside, closed rows, the guarded download, the five feeds. (Reloads: tests/test_reload_edges_gpu.py.)"""
import ctypes as C

import numpy as np
import pytest

import envutil_amd as ea
import devout
import edge_model as em
import jobs
import ycbcr_model as ym

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 9), (9, 1), (5, 3), (64, 64), (65, 63), (67, 131), (300, 7), (7, 300)]
TINY = np.float32(1.401298464324817e-45)      # the smallest positive denormal


def patterns(w, h):
    """(name, alpha plane) - 1 inside, 0 outside unless the pattern is about the values"""
    rng = np.random.default_rng(w * 1000 + h)
    yy, xx = np.mgrid[0:h, 0:w]
    one = np.ones((h, w), np.float32)
    yield "none outside", one.copy()
    yield "all outside", np.zeros((h, w), np.float32)
    a = one.copy()
    a[0, 0] = a[0, w - 1] = a[h - 1, 0] = a[h - 1, w - 1] = 0
    yield "corners", a
    yield "checkerboard", ((xx + yy) % 2).astype(np.float32)
    yield "random 1/500", (rng.uniform(size=(h, w)) >= 1.0 / 500.0).astype(np.float32)
    yield "random 1/2", (rng.uniform(size=(h, w)) >= 0.5).astype(np.float32)
    a = one.copy()
    a[h // 4:h // 4 + max(h // 3, 1), w // 3:w // 3 + max(w // 4, 1)] = 0
    yield "rectangle", a
    r = 0.45 * min(w, h)
    yield "disc", (((xx - 0.5 * (w - 1)) ** 2 + (yy - 0.5 * (h - 1)) ** 2) <= r * r).astype(np.float32)
    a = one.copy()
    a[::3] = (rng.uniform(size=a[::3].shape) >= 0.3).astype(np.float32)
    yield "rows without an outside pixel between rows with some", a
    vals = np.array([np.nan, -1.0, -0.0, 0.0, TINY, 1e-30, 1.0], np.float32)
    yield "values", vals[rng.integers(0, len(vals), (h, w))]


def load(w, h, alpha, nch=2, prj=ea.RECTILINEAR, hfov=60.0, degree=1, **kw):
    img = jobs.synth_image(w, h, nch, seed=3)
    img[:, :, nch - 1] = alpha
    return ea.Source.load(ea.facet_spec(prj, w, h, hfov, nchannels=nch), img, degree, edges=True, **kw)


def assert_plane(src, alpha, cyclic, what):
    got = src.edge_distance()
    want = em.distance_plane(alpha, cyclic)
    assert got.shape == want.shape, (what, got.shape)
    d = jobs.bits(got) != jobs.bits(want)
    assert not d.any(), f"{what}: {int(d.sum())} of {d.size} distances differ, first at {np.argwhere(d)[0]}: " \
                        f"{got[tuple(np.argwhere(d)[0])]!r} model {want[tuple(np.argwhere(d)[0])]!r}"


@pytest.mark.parametrize("w,h", SHAPES)
def test_plane_against_the_brute_force_model(w, h):
    for name, alpha in patterns(w, h):
        src = load(w, h, alpha, nch=2 if (w + h) % 2 else 4)
        assert src.has_edges
        assert_plane(src, alpha, False, f"{w} x {h} {name}")
        if name == "none outside":
            assert (src.edge_distance() == np.sqrt(np.float32(2.0 ** 31))).all()
        if name == "values":
            # NaN, -1 and both zeros are outside, the denormal and 1e-30 inside
            got = src.edge_distance()
            with np.errstate(invalid="ignore"):
                assert ((got == 0) == ~(alpha > 0)).all()


@pytest.mark.parametrize("nch", [2, 4])
def test_closed_rows(nch):
    """a 360-degree spherical facet: the distance reaches round the seam; the same planes on 180 degrees do not wrap"""
    w, h = 70, 35
    for col in (0, w - 1):
        alpha = np.ones((h, w), np.float32)
        alpha[5:9, col] = 0
        alpha[30, col] = 0
        full = load(w, h, alpha, nch, ea.SPHERICAL, 360.0)
        half = load(w, h, alpha, nch, ea.SPHERICAL, 180.0)
        assert_plane(full, alpha, True, f"360 degrees, column {col}")
        assert_plane(half, alpha, False, f"180 degrees, column {col}")
        other = w - 1 - col
        assert full.edge_distance()[6, other] == 1.0 and half.edge_distance()[6, other] == w - 1
    rng = np.random.default_rng(9)
    alpha = (rng.uniform(size=(h, w)) >= 0.02).astype(np.float32)
    assert_plane(load(w, h, alpha, nch, ea.CYLINDRICAL, 360.0), alpha, True, "cylinder, random")
    # a full sphere (2:1): rows still do not wrap
    alpha = np.ones((35, 70), np.float32)
    alpha[0, 3] = 0
    s = load(70, 35, alpha, nch, ea.SPHERICAL, 360.0, degree=3)
    assert_plane(s, alpha, True, "full sphere")
    assert s.edge_distance()[34, 3] == 34.0


def test_download_into_a_guarded_padded_buffer():
    import torch
    w, h = 67, 31
    alpha = dict(patterns(w, h))["random 1/2"]
    src = load(w, h, alpha)
    want = em.distance_plane(alpha)
    for pad, lead in ((3, 1), (0, 0), (6, 2)):
        buf = devout.Guarded(h, w, pad=pad, lead=lead)
        assert buf.stride_bytes % 16
        rc = ea.lib().eu_hip_source_edge_distance(src.handle, C.c_void_p(buf.ptr()), buf.stride_bytes, 1, None)
        assert rc == 0, ea.lib().eu_hip_last_error()
        ea.sync()
        torch.cuda.synchronize()
        frame, outside = buf.frame(), buf.outside()
        assert outside, str(outside)
        assert not (frame == devout.FILL).any(), "a word of the rows was left unwritten"
        assert (frame == jobs.bits(want)).all()
    # host output with a stride
    out = np.full((h, w + 3), -1.0, np.float32)
    assert ea.lib().eu_hip_source_edge_distance(src.handle, C.c_void_p(out.ctypes.data), out.strides[0], 0, None) == 0
    assert (jobs.bits(out[:, :w]) == jobs.bits(want)).all() and (out[:, w:] == -1.0).all()
    # a source without a plane, a stride that is none
    plain = ea.Source.load(ea.facet_spec(ea.RECTILINEAR, w, h, 60.0, nchannels=2), jobs.synth_image(w, h, 2), 1)
    assert not plain.has_edges and plain.edge_device_ptr() is None
    with pytest.raises(ea.EuError, match="no distance plane"):
        plain.edge_distance()
    assert ea.lib().eu_hip_source_edge_distance(src.handle, C.c_void_p(out.ctypes.data), 4 * w - 4, 0, None) < 0
    assert ea.lib().eu_hip_source_edge_distance(src.handle, C.c_void_p(out.ctypes.data), 4 * w + 2, 0, None) < 0


# ---- the five feeds: one geometry, one elliptic crop plus one polygon ----------------------------------------------

W, H = 61, 43
CROP = (4, 57, 2, 41)
MASKS = [(np.array([10.0, 30.0, 22.0]), np.array([8.0, 12.0, 30.0]))]


def edit_alpha():
    """eu_hip_facet_alpha's alpha_out for the crop and the polygon"""
    px = np.ones((H, W, 4), np.float32)
    return ea.facet_alpha(px, MASKS, CROP, 2)


def test_the_five_feeds_build_one_plane():
    rng = np.random.default_rng(21)
    fct = ea.facet_spec(ea.FISHEYE, W, H, 120.0, nchannels=4)
    kw = dict(masks=MASKS, crop=CROP, crop_kind=2)
    plane = edit_alpha()
    assert (plane == 0).any() and (plane == 1).any() and ((plane > 0) & (plane < 1)).any()
    rgba = rng.random((H, W, 4), dtype=np.float32)
    own = (rng.uniform(size=(H, W)) >= 0.01).astype(np.float32)         # the feed's own alpha: a few holes
    rgba[:, :, 3] = own
    s8 = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    q = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    q[..., 3] = 120 + q[..., 3] % 16
    y, cb, cr = ym.planes(rng, H, W, 2, 2, 8, "nv12", 1)
    m = ea.ycbcr_matrix("709")
    feeds = [("floats", lambda e: ea.Source.load(fct, rgba, 1, edges=e, **kw), own),
             ("edited floats that gain the channel", lambda e: ea.Source.load(fct, rgba[:, :, :3].copy(), 1, edges=e, **kw), None),
             ("8-bit samples", lambda e: ea.Source.load_samples(fct, s8, spline_degree=1, edges=e, **kw), None),
             ("rgbe", lambda e: ea.Source.load_rgbe(fct, q, spline_degree=1, edges=e, **kw), None),
             ("nv12", lambda e: ea.Source.load_ycbcr(fct, y, (cb, cr), m, spline_degree=1, edges=e, **kw), None)]
    gained = None
    for name, make, feed_alpha in feeds:
        flagged, plainly = make(True), make(False)
        assert flagged.has_edges and not plainly.has_edges, name
        alpha = plane if feed_alpha is None else em.fm.f32(feed_alpha * plane)
        assert_plane(flagged, alpha, False, name)
        a, b = flagged.download(), plainly.download()
        assert (jobs.bits(a) == jobs.bits(b)).all(), f"{name}: the flag changed the container"
        if feed_alpha is None:
            d = flagged.edge_distance()
            assert gained is None or (jobs.bits(d) == jobs.bits(gained)).all(), f"{name}: another plane than the feed before"
            gained = d


def test_flags_zero_is_the_old_load():
    """eu_hip_source_load_pixels with flags == 0: the container of the matching load, bit for bit"""
    rng = np.random.default_rng(4)
    fct = ea.facet_spec(ea.RECTILINEAR, W, H, 70.0, nchannels=4)
    rgb = rng.random((H, W, 3), dtype=np.float32)
    ptr, pch, on_device, e, hold = ea.Source._float_feed(fct, rgb, MASKS, CROP, 1)
    px = ea.api.Pixels(ea.api.PX_FLOATS, ptr, pch, 0, None, None, None, None)
    a = ea.Source._load_pixels(fct, px, e, 3, 3, 8, 64, 0)
    b = ea.Source.load(fct, rgb, 3, masks=MASKS, crop=CROP, crop_kind=1)
    assert not a.has_edges
    assert (jobs.bits(a.download()) == jobs.bits(b.download())).all()
