"""The row plan of a masked / cropped facet's alpha plane (eu_hip_facet_alpha_rows): the integer tables the
device form of the edit reads, rasterised with numpy and compared with the oracle's plane before the
binomial (euo.facet_alpha(..., stage=0)) - bit for bit, it is zeros and ones. And the argument checks of
eu_hip_source_load_edited / eu_hip_facet_alpha_dev, which come before a device is looked for.
No GPU needed: this is load-time host code."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import envutil_amd as ea
import euo
from envutil_amd import api

SHAPES = [(1, 1), (2, 3), (4, 4), (5, 7), (63, 65), (64, 16), (65, 17), (127, 33), (257, 129), (1000, 3), (3, 1000)]


def random_polygons(rng, w, h, n):
    """the generator of tests/test_imageprep.py"""
    polys = []
    for _ in range(n):
        k = int(rng.integers(3, 9))
        # vertices also outside the image, self-intersecting orders, integer and fractional coordinates
        x = rng.uniform(-0.3 * w, 1.3 * w, k).astype(np.float32)
        y = rng.uniform(-0.3 * h, 1.3 * h, k).astype(np.float32)
        if rng.random() < 0.3:
            x, y = np.round(x), np.round(y)
        polys.append((x, y))
    return polys


# seeds of the cases below, where 0 does not do: a case at least 32 pixels wide and high must have exact
# zeros, exact ones and values in between in the oracle's final plane (three_classes)
SEEDS = {(63, 65, 0): 1, (257, 129, 0): 1}     # seed 0 draws no polygon there, and without a crop nothing is cleared


def shape_case(w, h, kind, npoly=None):
    """0-3 random polygons (npoly None: drawn) with vertices uniform in [-0.3, 1.3] of the size, the crop at
    1/10 and 1/8 of the edges"""
    fixed = 0 if npoly is None else 1 + npoly
    rng = np.random.default_rng([77, w, h, kind, fixed, SEEDS.get((w, h, kind), 0)])
    polys = random_polygons(rng, w, h, int(rng.integers(0, 4)) if npoly is None else npoly)
    crop = (w // 10, w - w // 8, h // 10, h - h // 8) if kind else None
    if kind == 2 and (crop[1] == crop[0] or crop[3] == crop[2]):
        crop = (0, w + 1, 0, h + 1)          # a degenerate ellipse divides by zero in the reference too
    return polys, crop


def rasterise(w, h, keep, row_start, spans):
    """the plane the tables describe, by their definition"""
    plane = np.zeros((h, w), np.float32)
    for y in range(h):
        plane[y, keep[y, 0]:keep[y, 1]] = 1
    rows = np.repeat(np.arange(h), np.diff(row_start))
    for y, (x0, x1) in zip(rows.tolist(), spans.tolist()):
        plane[y, x0:x1] = 0
    return plane


def check_plan(w, h, polys, crop, kind):
    keep, row_start, spans = ea.facet_alpha_rows(w, h, polys, crop, kind)
    # well-formed: intervals and spans inside the image, spans not empty, offsets rising
    assert keep.shape == (h, 2) and (keep >= 0).all() and (keep <= w).all() and (keep[:, 0] <= keep[:, 1]).all()
    assert row_start[0] == 0 and row_start[-1] == len(spans) and (np.diff(row_start) >= 0).all()
    if len(spans):
        assert (spans[:, 0] >= 0).all() and (spans[:, 1] <= w).all() and (spans[:, 0] < spans[:, 1]).all()
    if crop is None or kind == 0:
        assert (keep[:, 0] == 0).all() and (keep[:, 1] == w).all()
    want = euo.facet_alpha(w, h, polys, crop, kind, stage=0)
    got = rasterise(w, h, keep, row_start, spans)
    assert (got.view(np.uint32) == want.view(np.uint32)).all(), (w, h, kind, int((got != want).sum()))
    return want


def three_classes(w, h, polys, crop, kind):
    """no case is vacuous: the ORACLE's final plane has exact zeros, exact ones and values in between"""
    f = euo.facet_alpha(w, h, polys, crop, kind)
    assert (f == 0).any() and (f == 1).any() and ((f > 0) & (f < 1)).any(), (w, h, kind)


@pytest.mark.parametrize("seed", range(12))
def test_rows_are_the_oracles_stage0_seeded(seed):
    """the twelve cases of tests/test_imageprep.py::test_library_alpha_is_the_oracles"""
    rng = np.random.default_rng(1000 + seed)
    w, h = int(rng.integers(8, 90)), int(rng.integers(8, 70))
    polys = random_polygons(rng, w, h, int(rng.integers(0, 4)))
    kind = int(rng.integers(0, 3))
    x0, x1 = sorted(rng.integers(-5, w + 5, 2).tolist())
    y0, y1 = sorted(rng.integers(-5, h + 5, 2).tolist())
    if kind == 2 and (x1 == x0 or y1 == y0):
        x1, y1 = x0 + 7, y0 + 5
    check_plan(w, h, polys, (x0, x1, y0, y1) if kind else None, kind)


@pytest.mark.parametrize("w,h", SHAPES)
def test_rows_are_the_oracles_stage0_shapes(w, h):
    for kind in range(3):
        polys, crop = shape_case(w, h, kind)
        check_plan(w, h, polys, crop, kind)
        if w >= 32 and h >= 32:
            three_classes(w, h, polys, crop, kind)


@pytest.mark.parametrize("w,h", SHAPES)
def test_rows_are_the_oracles_stage0_every_polygon_count(w, h):
    """beyond the cases above: every count of polygons with every crop kind (the plane of ones among them)"""
    for npoly in range(4):
        for kind in range(3):
            polys, crop = shape_case(w, h, kind, npoly)
            check_plan(w, h, polys, crop, kind)


@pytest.mark.parametrize("w,h,kind", [(4096, 3072, 2), (6000, 4000, 1)])
def test_rows_are_the_oracles_stage0_fullsize(w, h, kind):
    polys, crop = shape_case(w, h, kind, 3)
    check_plan(w, h, polys, crop, kind)
    three_classes(w, h, polys, crop, kind)


def test_crops_beyond_the_image_and_empty():
    for crop, kind in [((-5, 200, -3, 100), 1), ((-40, 30, -20, 20), 2), ((50, 20, 5, 30), 1), ((10, 30, 40, 40), 1),
                       ((300, 400, 300, 400), 1), ((300, 400, 300, 400), 2), ((-9, -2, 3, 20), 2)]:
        check_plan(60, 40, [], crop, kind)


def _polygon_array(polys):
    keep = [(np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)) for x, y in polys]
    arr = (api.MaskPolygon * max(len(keep), 1))()
    for i, (x, y) in enumerate(keep):
        arr[i].n, arr[i].x, arr[i].y = len(x), x.ctypes.data, y.ctypes.data
    return arr, keep


def test_count_only_then_exact_size():
    L = ea.lib()
    w, h = 257, 129
    polys, crop = shape_case(w, h, 1, 3)
    arr, hold = _polygon_array(polys)
    args = (w, h, C.cast(arr, C.c_void_p), len(polys), 1) + crop
    n = L.eu_hip_facet_alpha_rows(*args, None, None, None, 0)
    assert n > 0
    keep, row_start, spans = np.zeros((h, 2), np.int32), np.zeros(h + 1, np.int32), np.full((n, 2), -7, np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.eu_hip_facet_alpha_rows(*args, ptr(keep), ptr(row_start), ptr(spans), n) == n
    assert (spans != -7).all() and row_start[-1] == n
    want = euo.facet_alpha(w, h, polys, crop, 1, stage=0)
    assert (rasterise(w, h, keep, row_start, spans) == want).all()
    # one too few: refused, with a message
    assert L.eu_hip_facet_alpha_rows(*args, ptr(keep), ptr(row_start), ptr(spans), n - 1) == -2
    assert b"too small" in L.eu_hip_last_error()
    # the refusals of eu_hip_facet_alpha
    assert L.eu_hip_facet_alpha_rows(0, h, None, 0, 0, 0, 0, 0, 0, None, None, None, 0) == -2
    assert L.eu_hip_facet_alpha_rows(w, h, None, 0, 3, 0, 0, 0, 0, None, None, None, 0) == -2
    assert L.eu_hip_facet_alpha_rows(w, h, None, 2, 0, 0, 0, 0, 0, None, None, None, 0) == -2
    bad = (api.MaskPolygon * 1)()
    bad[0].n, bad[0].x, bad[0].y = 4, None, None
    assert L.eu_hip_facet_alpha_rows(w, h, C.cast(bad, C.c_void_p), 1, 0, 0, 0, 0, 0, None, None, None, 0) == -2


def _edit(npolygons=0, polygons=None, crop_kind=0, pixel_channels=4, on_device=0):
    e = api.FacetEdit()
    e.polygons, e.npolygons, e.crop_kind = polygons, npolygons, crop_kind
    e.crop_x0, e.crop_x1, e.crop_y0, e.crop_y1 = 2, 14, 2, 10
    e.pixel_channels, e.pixels_on_device = pixel_channels, on_device
    return e


def test_load_edited_refuses_before_it_looks_for_a_device():
    """EU_ERR_ARGUMENT (-2), not EU_ERR_NO_DEVICE (-1), with or without a GPU - and a message"""
    L = ea.lib()
    px = np.zeros((12, 16, 4), np.float32)
    out = C.c_void_p()

    def load(nch, e, pixels=px):
        cf = ea.facet_spec(ea.RECTILINEAR, 16, 12, 60.0, nchannels=nch).c_struct()
        rc = L.eu_hip_source_load_edited(C.byref(cf), pixels.ctypes.data_as(C.c_void_p) if pixels is not None else None,
                                         C.byref(e) if e is not None else None, 1, 1, 8, 64, C.byref(out))
        return rc, L.eu_hip_last_error()

    bad = (api.MaskPolygon * 1)()
    bad[0].n, bad[0].x, bad[0].y = 4, None, None
    for nch, e in [(3, _edit(crop_kind=1, pixel_channels=3)),                 # an edit needs 2 or 4 channels
                   (1, _edit(crop_kind=2, pixel_channels=1)),
                   (3, _edit(pixel_channels=2)),                              # ... also when it only widens
                   (4, _edit(npolygons=1, polygons=C.cast(bad, C.c_void_p))),  # a polygon without vertices
                   (4, _edit(npolygons=1, polygons=None)),
                   (4, _edit(npolygons=-1)),
                   (4, _edit(crop_kind=3)), (4, _edit(crop_kind=-1)),         # crop_kind outside 0..2
                   (4, _edit(pixel_channels=2)), (4, _edit(pixel_channels=5)), (4, _edit(pixel_channels=0)),
                   (2, _edit(pixel_channels=0)), (2, _edit(pixel_channels=3))]:
        rc, msg = load(nch, e)
        assert rc == -2 and msg, (nch, e.crop_kind, e.pixel_channels, rc, msg)
    assert load(4, _edit(crop_kind=1), pixels=None)[0] == -2
    # the device twin's own
    f = L.eu_hip_facet_alpha_dev
    assert f(None, 16, 12, 4, C.byref(_edit(crop_kind=1)), None, None) == -2
    assert f(C.c_void_p(16), 16, 12, 3, C.byref(_edit(crop_kind=1, pixel_channels=3)), None, None) == -2
    assert f(C.c_void_p(16), 16, 12, 4, C.byref(_edit(crop_kind=1, pixel_channels=3)), None, None) == -2
    assert f(C.c_void_p(16), 16, 12, 4, C.byref(_edit(crop_kind=5)), None, None) == -2
    assert f(C.c_void_p(16), 0, 12, 4, C.byref(_edit(crop_kind=1)), None, None) == -2


def test_without_a_device_a_valid_edit_fails_loudly():
    if ea.device_count() > 0:
        pytest.skip("a HIP device is present")
    fct = ea.facet_spec(ea.RECTILINEAR, 16, 12, 60.0, nchannels=4)
    with pytest.raises(ea.EuError, match="no HIP device"):
        ea.Source.load(fct, np.zeros((12, 16, 3), np.float32), 1, crop=(2, 14, 2, 10), crop_kind=1)


def test_facet_edit_struct_matches_the_header(tmp_path):
    """sizeof / offsetof of eu_facet_edit as gcc lays it out against the ctypes mirror"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "eu_hip.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(eu_facet_edit));']
    lines += [f'  printf("{f} %zu\\n", offsetof(eu_facet_edit, {f}));' for f, _ in api.FacetEdit._fields_]
    lines += ['  return 0;', '}']
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c11", "-I" + os.path.join(root, "include"), str(tmp_path / "layout.c"),
                           "-o", str(tmp_path / "layout")])
    out = dict(ln.split() for ln in subprocess.check_output([str(tmp_path / "layout")], text=True).splitlines())
    assert C.sizeof(api.FacetEdit) == int(out.pop("size"))
    assert len(out) == len(api.FacetEdit._fields_)
    for f, v in out.items():
        assert getattr(api.FacetEdit, f).offset == int(v), f
