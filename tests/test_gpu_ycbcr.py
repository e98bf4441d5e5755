"""Y'CbCr planes on the device (eu_hip_source_load_ycbcr, eu_ycbcr.hip; Source.load_ycbcr). What is expected comes from
tests/ycbcr_model.py, a numpy float32 model written from the three formulas - not from the library's host function:
the container of load_ycbcr is, bit for bit, Source.load of the model's floats, with the same edit. A thread of the
decode owns four floats of a destination row behind the row's first 16-byte boundary and reads its samples out of
aligned dwords, so widths, channel counts, container pitches, plane pitches and plane addresses are chosen for every
alignment; a width of more than 1024 floats takes a second workgroup, more than 8 rows a second row block."""
import numpy as np
import pytest

import envutil_amd as ea
import ycbcr_model as ym

pytestmark = pytest.mark.gpu

LAYOUTS = ("planar", "nv12", "nv21")


def bits_of(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_container(a, b, what):
    ca, cb = a.download(), b.download()
    assert ca.shape == cb.shape, what
    bad = int((bits_of(ca) != bits_of(cb)).sum())
    assert bad == 0, f"{what}: {bad} of {ca.size} floats differ"


def flat_facet(w, h, nch=3):
    return ea.facet_spec(ea.RECTILINEAR, w, h, 60.0, nchannels=nch)


def on_device(a):
    """a device tensor with the strides of the numpy view `a` (a padded row pitch, interleaved samples)"""
    import torch
    base = a
    while base.base is not None:
        base = base.base
    t = torch.from_numpy(np.ascontiguousarray(base)).to("cuda:0")
    off = (a.__array_interface__["data"][0] - base.__array_interface__["data"][0]) // a.itemsize
    return t.reshape(-1).as_strided(a.shape, tuple(s // a.itemsize for s in a.strides), off)


def check_load(fct, planes, subs, tables, matrix, degree, what, device=False, **edit):
    y, cb, cr = planes
    yt, ct = tables
    want = ea.Source.load(fct, ym.floats(y, cb, cr, subs[0], subs[1], yt, ct, matrix), degree, **edit)
    if device:
        y, cb, cr = on_device(y), on_device(cb), on_device(cr)
    got = ea.Source.load_ycbcr(fct, y, (cb, cr), matrix, yt, ct, spline_degree=degree, **edit)
    same_container(got, want, what)
    return got


@pytest.mark.parametrize("nch", [3, 4])
@pytest.mark.parametrize("bits", [8, 16])
def test_load_flat_facets(bits, nch):
    """degree 1: no prefilter, the container's core holds the decoded floats themselves (pitch = width + frame)"""
    rng = np.random.default_rng(10 * bits + nch)
    tables = [ym.random_tables(rng, bits), ea.ycbcr_tables(bits)]
    k = 0
    for h in (1, 2, 3, 5):
        for w in (1, 2, 3, 5, 63, 64, 65, 257):
            for sub_x, sub_y in ((1, 1), (2, 1), (1, 2), (2, 2)):
                layout, pad = LAYOUTS[k % 3], (0, 1, 3)[(k // 3) % 3]
                m = ea.ycbcr_matrix(("601", "709", "2020")[k % 3])
                p = ym.planes(rng, h, w, sub_x, sub_y, bits, layout, pad)
                check_load(flat_facet(w, h, nch), p, (sub_x, sub_y), tables[k % 2], m, 1,
                           (w, h, nch, bits, sub_x, sub_y, layout, pad), device=k % 2 == 1)
                k += 1


def test_more_than_one_block_and_row_group():
    """1400 x 3 floats: five workgroups along a row; 21 rows: three row groups, the last one ragged"""
    rng = np.random.default_rng(3)
    for bits, nch, layout in ((8, 3, "nv12"), (16, 4, "planar"), (8, 4, "nv21"), (16, 3, "nv12")):
        p = ym.planes(rng, 21, 1400, 2, 2, bits, layout, 2)
        check_load(flat_facet(1400, 21, nch), p, (2, 2), ym.random_tables(rng, bits), ea.ycbcr_matrix("709"), 1,
                   ("wide", bits, nch, layout), device=bits == 8)


def test_load_degree_3_and_window():
    rng = np.random.default_rng(4)
    t8 = ea.ycbcr_tables(8)
    m = ea.ycbcr_matrix("709")
    for w, h in ((5, 3), (65, 9), (257, 4)):
        for nch in (3, 4):
            check_load(flat_facet(w, h, nch), ym.planes(rng, h, w, 2, 2, 8, "nv12"), (2, 2), t8, m, 3, (w, h, nch, "degree 3"))
    # a window whose container pitch differs from the width
    fct = ea.facet_spec(ea.RECTILINEAR, 200, 100, 70.0, nchannels=3, window=(67, 45, 20, 10))
    check_load(fct, ym.planes(rng, 45, 67, 2, 2, 8, "planar"), (2, 2), t8, m, 3, "window")
    p010 = ea.ycbcr_tables(16, depth=10, msb_aligned=True)
    y, cb, cr = ym.planes(rng, 45, 67, 2, 2, 16, "nv12", 1)
    y &= 0xffc0
    check_load(fct, (y, cb, cr), (2, 2), p010, ea.ycbcr_matrix("2020"), 3, "window, P010 on the device", device=True)


def test_load_full_sphere_and_cubemaps():
    rng = np.random.default_rng(5)
    t8 = ea.ycbcr_tables(8, full_range=True)
    m = ea.ycbcr_matrix("601")
    for nch in (3, 4):
        check_load(ea.facet_spec(ea.SPHERICAL, 6, 3, 360.0, nchannels=nch), ym.planes(rng, 3, 6, 2, 2, 8, "planar"),
                   (2, 2), t8, m, 3, ("6 x 3 sphere", nch))
    # the plane of a cubemap is the 1:6 stack of its faces, treated as one image
    for face in (9, 64):
        fct = ea.facet_spec(ea.CUBEMAP, face, 6 * face, 90.0)
        check_load(fct, ym.planes(rng, 6 * face, face, 2, 2, 8, "nv12"), (2, 2), t8, m, 3, ("cubemap", face), device=face == 9)


def test_load_with_masks_and_crop():
    """4 channels with a polygon mask and an elliptic crop: the decode writes the dense buffer the edit reads"""
    rng = np.random.default_rng(6)
    t8 = ea.ycbcr_tables(8)
    m = ea.ycbcr_matrix("709")
    for (w, h), device in (((67, 45), False), ((130, 77), True)):
        poly = [(np.array([0.1, 0.7, 0.5, 0.2]) * w, np.array([0.2, 0.1, 0.8, 0.6]) * h)]
        crop = (w // 10, w - w // 8, h // 9, h - h // 7)
        fct = ea.facet_spec(ea.FISHEYE, w, h, 120.0, nchannels=4)
        p = ym.planes(rng, h, w, 2, 2, 8, "nv12")
        check_load(fct, p, (2, 2), t8, m, 3, ("edit", w, h), device=device, masks=poly, crop=crop, crop_kind=2)
        check_load(fct, p, (2, 2), t8, m, 1, ("mask only", w, h), device=device, masks=poly)
    with pytest.raises(ea.EuError):
        ea.Source.load_ycbcr(flat_facet(130, 77, 3), p[0], (p[1], p[2]), m, spline_degree=1, masks=poly)


def test_planes_packed_back_to_back_at_odd_addresses():
    """one decoder buffer: luma, then chroma right behind it, the frame a view that starts at byte 1, 2 and 3"""
    import torch
    rng = np.random.default_rng(7)
    w, h = 37, 11
    cw, ch = (w + 1) // 2, (h + 1) // 2
    m = ea.ycbcr_matrix("709")
    tabs = ym.random_tables(rng, 8)
    for start in (1, 2, 3):
        buf = rng.integers(0, 256, start + w * h + 2 * cw * ch, dtype=np.uint8)
        y = buf[start:start + w * h].reshape(h, w)
        c = buf[start + w * h:].reshape(ch, cw, 2)
        want = ea.Source.load(flat_facet(w, h), ym.floats(y, c[..., 0], c[..., 1], 2, 2, *tabs, m), 1)
        dev = torch.from_numpy(buf).to("cuda:0")
        dy = dev[start:start + w * h].reshape(h, w)
        dc = dev[start + w * h:].reshape(ch, cw, 2)
        same_container(ea.Source.load_ycbcr(flat_facet(w, h), dy, dc, m, *tabs), want, ("device, start", start))
        same_container(ea.Source.load_ycbcr(flat_facet(w, h), y, c, m, *tabs), want, ("host, start", start))


def test_render_from_a_ycbcr_source():
    """spherical 256 x 128 NV12 to a 64-wide cubemap, degree 3: the same frame from either source"""
    rng = np.random.default_rng(8)
    y, cb, cr = ym.planes(rng, 128, 256, 2, 2, 8, "nv12")
    m = ea.ycbcr_matrix("709")
    yt, ct = ea.ycbcr_tables(8)
    fct = ea.facet_spec(ea.SPHERICAL, 256, 128, 360.0)
    args = ea.arguments(ea.CUBEMAP, 64, 384, 90.0, spline_degree=3)
    got = ea.render(args, ea.Source.load_ycbcr(fct, y, (cb, cr), m, spline_degree=3))
    want = ea.render(args, ea.Source.load(fct, ym.floats(y, cb, cr, 2, 2, yt, ct, m), 3))
    assert (bits_of(got) == bits_of(want)).all() and np.isfinite(got).all()
