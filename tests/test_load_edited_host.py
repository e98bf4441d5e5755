"""Float pixels through the alpha edit, host side: the argument checks of eu_hip_source_load_edited. Like those of
eu_hip_source_load_samples (tests/test_load_samples_host.py) they are all made before a device is looked for, so
they run without one; a call that passes them returns 0 where there is a device and EU_ERR_NO_DEVICE where there is
none - also the call whose edit changes nothing, which is handed on to eu_hip_source_load. That entry point looks for
a device first."""
import ctypes as C

import numpy as np
import pytest

import envutil_amd as ea
from envutil_amd import api

EU_ERR_NO_DEVICE, EU_ERR_ARGUMENT = -1, -2
W, H = 8, 4
TRIANGLE = (np.array([1, 5, 3], np.float32), np.array([1, 1, 3], np.float32))


def call(fct, pixels, edit, degree=1, prefilter=1, out=True):
    L = api.lib()
    h = C.c_void_p()
    rc = L.eu_hip_source_load_edited(C.byref(fct) if fct is not None else None,
                                     pixels.ctypes.data if pixels is not None else None,
                                     C.byref(edit) if edit is not None else None, degree, prefilter, 8, 64,
                                     C.byref(h) if out else None)
    if rc == 0:
        L.eu_hip_source_release(h)              # a machine with a device: the call went through
    else:
        assert not h.value, "a refused call must not make a source"
    return rc, L.eu_hip_last_error().decode()


def refused(rc, msg):
    return rc == EU_ERR_ARGUMENT and len(msg) > 0


def facet(nchannels=4):
    return ea.facet_spec(ea.RECTILINEAR, W, H, 60.0, nchannels=nchannels).c_struct()


def pixels(channels):
    return np.zeros((H, W, channels), np.float32)


def masked(pixel_channels, on_device=False):
    """(an edit that changes something: one polygon; what it points into)"""
    return api._facet_edit([TRIANGLE], None, 0, pixel_channels, on_device)


def test_null_pointers():
    edit, hold = masked(3)
    assert refused(*call(None, pixels(3), edit))
    assert refused(*call(facet(), None, edit))
    assert refused(*call(facet(), pixels(3), edit, out=False))
    # ... and without an edit
    assert refused(*call(None, pixels(4), None))
    assert refused(*call(facet(), None, None))
    assert refused(*call(facet(), pixels(4), None, out=False))


def test_degrees():
    for degree, prefilter in ((-1, 1), (10, 1), (1, -1), (1, 10)):
        for edit, hold in (masked(3), (None, None)):
            rc, msg = call(facet(), pixels(3 if edit is not None else 4), edit, degree, prefilter)
            assert refused(rc, msg) and "degree" in msg, (degree, prefilter, msg)


def test_crop_kind():
    edit, hold = masked(3)
    edit.crop_kind = 3
    assert refused(*call(facet(), pixels(3), edit))
    edit, hold = api._facet_edit([], (1, 6, 1, 3), 1, 4, False)
    edit.crop_kind = 3
    assert refused(*call(facet(), pixels(4), edit))


def test_polygon_without_vertices():
    for null_x, null_y in ((True, False), (False, True), (True, True)):
        edit, hold = masked(3)
        poly = C.cast(edit.polygons, C.POINTER(api.MaskPolygon))
        assert poly[0].n == 3
        if null_x:
            poly[0].x = None
        if null_y:
            poly[0].y = None
        assert refused(*call(facet(), pixels(3), edit)), (null_x, null_y)
    # n > 0 polygons and no array of them
    edit, hold = masked(3)
    edit.polygons = None
    assert refused(*call(facet(), pixels(3), edit))


def test_pixel_channels():
    # neither the facet's count nor one less
    for nch, pch in ((3, 1), (3, 4), (4, 2), (1, 2), (4, 5), (1, 0), (1, -1)):
        edit, hold = api._facet_edit([], None, 0, pch, False)
        rc, msg = call(facet(nch), pixels(max(pch, 1)), edit)
        assert refused(rc, msg), (nch, pch, msg)
        if pch >= 1:
            assert "pixel_channels" in msg, (nch, pch, msg)


def test_edit_needs_alpha():
    """an edit that changes something - a mask, a crop, a gained channel - wants an alpha channel to put it in"""
    for nch in (1, 3):
        edit, hold = masked(nch)
        rc, msg = call(facet(nch), pixels(nch), edit)
        assert refused(rc, msg) and "2 or 4 channels" in msg, msg
        edit, hold = api._facet_edit([], (1, 6, 1, 3), 1, nch, False)
        rc, msg = call(facet(nch), pixels(nch), edit)
        assert refused(rc, msg) and "2 or 4 channels" in msg, msg
    edit, hold = api._facet_edit([], None, 0, 2, False)          # 2 -> 3 channels
    rc, msg = call(facet(3), pixels(2), edit)
    assert refused(rc, msg) and "2 or 4 channels" in msg, msg


def reaches_the_device(rc, msg):
    if ea.device_count() > 0:
        return rc == 0
    return rc == EU_ERR_NO_DEVICE and "no HIP device" in msg      # every check passed


def test_valid_arguments_reach_the_device():
    # a mask on pixels that gain their alpha channel, a crop on pixels that have one, the channel gain alone
    edit, hold = masked(3)
    rc, msg = call(facet(), pixels(3), edit)
    assert reaches_the_device(rc, msg), (rc, msg)
    edit, hold = api._facet_edit([], (1, 6, 1, 3), 2, 4, False)
    rc, msg = call(facet(), pixels(4), edit)
    assert reaches_the_device(rc, msg), (rc, msg)
    edit, hold = api._facet_edit([], None, 0, 1, False)
    rc, msg = call(facet(2), pixels(1), edit)
    assert reaches_the_device(rc, msg), (rc, msg)


def test_an_edit_that_edits_nothing_reaches_the_device():
    """no edit, and an edit without polygons or crop at the facet's channel count: the route through the plain load"""
    for nch in (1, 3, 4):
        rc, msg = call(facet(nch), pixels(nch), None)
        assert reaches_the_device(rc, msg), (nch, rc, msg)
        edit, hold = api._facet_edit([], None, 0, nch, False)
        rc, msg = call(facet(nch), pixels(nch), edit)
        assert reaches_the_device(rc, msg), (nch, rc, msg)


def test_plain_load_looks_for_a_device_first():
    L = api.lib()
    h = C.c_void_p()
    px = pixels(4)
    rc = L.eu_hip_source_load(None, px.ctypes.data, 1, 1, 8, 64, C.byref(h))
    msg = L.eu_hip_last_error().decode()
    assert rc < 0 and not h.value and len(msg) > 0
    if ea.device_count() == 0:
        assert rc == EU_ERR_NO_DEVICE and "no HIP device" in msg
