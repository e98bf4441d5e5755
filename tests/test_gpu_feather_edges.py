"""Feathering to alpha edges in the blend (eu_feather_weight in eu_multi_dev.h): frames of jobs whose facets keep a
distance plane (EU_LOAD_EDGES), bit for bit against tests/edge_model.py - feather and multiband, every way in and out
of a frame that shares the weight - and three checks that keep a wrong result from passing unseen: jobs without a
plane are unchanged, the seam really moves, the cropped facet fades out at its crop."""
import numpy as np
import pytest

import envutil_amd as ea
import euo
import jobs
import edge_model as em
import feather_model as fm

pytestmark = pytest.mark.gpu


def assert_bits(got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    d = jobs.bits(got) != jobs.bits(ref)
    assert not d.any(), f"{what}: {int(d.sum())} of {d.size} values differ, first at {np.argwhere(d)[0]}: " \
                        f"{got[tuple(np.argwhere(d)[0])]!r} model {ref[tuple(np.argwhere(d)[0])]!r}"


def fisheyes(nch, degree, edges=True, **kw):
    """two fisheye facets of 40 x 40 with elliptic crops, overlapping in the middle of a 96 x 48 target"""
    out = []
    for k in range(2):
        img = jobs.synth_image(40, 40, nch, seed=60 + k)
        out.append(em.Facet(euo.FISHEYE, 40, 40, 100.0, img, degree, crop=(2 + k, 37 + k, 3, 38), crop_kind=2, edges=edges,
                            yaw=-22.0 + 44.0 * k, pitch=2.0 * k - 1.0, roll=4.0 * k, brighten=1.0 + 0.25 * k, **kw))
    return out


POLYGON = [(np.array([30.0, 47.5, 47.5, 36.0]), np.array([4.0, 2.0, 28.0, 25.0]))]


def rectilinears(nch, degree, edges=(True, True, True), **kw):
    """three rectilinear facets of 48 x 32 in a row, the middle one with a polygon mask over its right part"""
    out = []
    for k in range(3):
        img = jobs.synth_image(48, 32, nch, seed=80 + k)
        out.append(em.Facet(euo.RECTILINEAR, 48, 32, 50.0, img, degree, masks=POLYGON if k == 1 else (), edges=edges[k],
                            yaw=-26.0 + 26.0 * k, pitch=1.5 * k - 1.0, roll=2.0 * k, brighten=1.0 + 0.2 * k, **kw))
    return out


def fisheye_target(**kw):
    return ea.arguments(ea.SPHERICAL, 96, 48, 160.0, synopsis="feather", **kw)


def rect_target(**kw):
    return ea.arguments(ea.SPHERICAL, 80, 60, 120.0, synopsis="feather", **kw)


def held(what, a, fs, nch, overlap=20):
    gs = [f.gpu() for f in fs]
    assert [g.has_edges for g in gs] == [f.edges for f in fs]
    ref, qsum, count = em.model_frame(a, fs, nch, details=True)
    assert np.isfinite(ref).all()
    assert (count >= 2).sum() >= overlap, f"{what}: {(count >= 2).sum()} pixels see more than one facet"
    got = ea.render(a, gs, nch)
    assert_bits(got, ref, what)
    return got, gs, count


# ---- frames against the model ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("width", [0.0, 5.0])
@pytest.mark.parametrize("nch", [2, 4])
@pytest.mark.parametrize("degree", [1, 3])
def test_fisheye_facets_with_elliptic_crops(degree, nch, width):
    held(f"fisheyes degree {degree} nch {nch} width {width}", fisheye_target(spline_degree=degree, feather=width),
         fisheyes(nch, degree), nch)


@pytest.mark.parametrize("width", [0.0, 7.0])
@pytest.mark.parametrize("nch", [2, 4])
@pytest.mark.parametrize("degree", [1, 3])
def test_rectilinear_facets_with_a_polygon_mask(degree, nch, width):
    held(f"rectilinears degree {degree} nch {nch} width {width}", rect_target(spline_degree=degree, feather=width),
         rectilinears(nch, degree), nch)


def test_flagged_beside_unflagged():
    """one job, facets with and without a plane: the unflagged facet keeps the window ramp"""
    fs = rectilinears(4, 1, edges=(False, True, False))
    a = rect_target(spline_degree=1, feather=6.0)
    got, gs, _ = held("mixed", a, fs, 4)
    # neither the job without any plane nor the job with every plane
    assert (jobs.bits(got) != jobs.bits(ea.render(a, [f.gpu(edges=False) for f in fs], 4))).any()


def test_mask_for_is_the_weight_and_the_cropped_facet_fades_out():
    """--mask_for 0 under feather: facet 0 white, facet 1 black - colour channel 0 of the frame is facet 0's normalised
    weight q0 / (q0 + q1) times amax <= 1. Where the model's D of facet 0 is below 1.5 its d is below 1, so e0 <= 1 / width
    and q0 = a0 * e0 <= 1 / width; where the other facet's q1 is at least 1/2 the weight is then below 2 / width."""
    width = 8.0
    fs = fisheyes(4, 1)
    for k, f in enumerate(fs):
        fs[k] = em.Facet(f.prj, f.width, f.height, f.hfov, f.raw, 1, crop=f.crop, crop_kind=2, **dict(f.kw, masked=1 - k, brighten=1.0))
    a = fisheye_target(spline_degree=1, feather=width)
    got, gs, count = held("mask_for", a, fs, 4)
    arr = [em.facet_arrays(a, f, 4) for f in fs]
    both = arr[0]["hit"] & arr[1]["hit"]
    d0 = em.sample(fs[0].dist, arr[0]["sx"], arr[0]["sy"], False) + np.float32(0.5)
    q1 = arr[1]["pixel"][:, :, 3] * em.edge_weight(arr[1], width)
    near = both & (d0 < 1.5) & (q1 >= 0.5)
    assert near.sum() >= 5, f"{near.sum()} pixels along the crop circle: the assertion would be vacuous"
    assert (got[near][:, 0] < 2.0 / width).all(), got[near][:, 0].max()
    assert got[:, :, 0].max() > 0.9 and got[:, :, 0].min() == 0.0


def test_the_seam_really_moves():
    a = fisheye_target(spline_degree=1, feather=6.0)
    fs = fisheyes(4, 1)
    flagged, gs, count = held("flagged", a, fs, 4)
    plain = ea.render(a, [f.gpu(edges=False) for f in fs], 4)
    # the unflagged frame is feather's own model: the window ramp alone
    assert_bits(plain, fm.model_frame(a, fs, 4), "unflagged against feather_model")
    band = count >= 2
    moved = (jobs.bits(flagged) != jobs.bits(plain)).any(axis=2)
    assert band.sum() > 100 and moved[band].mean() > 0.1, (band.sum(), moved[band].mean())
    assert not moved[count == 1].any() and not moved[count == 0].any()


def test_views_samples_and_twining():
    a = rect_target(spline_degree=1, feather=7.0)
    fs = rectilinears(4, 1)
    got, gs, _ = held("the shared job", a, fs, 4)
    views = [(0.0, 0.0, 0.0), (9.0, -3.0, 2.0)]
    vs = ea.render_views(a, views, gs, nchannels=4)
    assert_bits(vs[0], got, "view 0 is the job")
    b = rect_target(spline_degree=1, feather=7.0, yaw=9.0, pitch=-3.0, roll=2.0)
    assert_bits(vs[1], em.model_frame(b, fs, 4), "view 1 against the model")
    for bits in (8, 16):
        assert (ea.render_samples(a, gs, 4, bits=bits) == ea.encode_samples(got, bits=bits)).all(), f"{bits}-bit samples"
    # twined: the model per tap ray
    t = rect_target(spline_degree=1, feather=7.0, twine=2)
    gws = [f.gpu_white() for f in fs]
    ref = em.model_frame_at_rays(t, fs, gs, gws, 4)
    assert np.isfinite(ref).all() and (ref != 0).mean() > 0.2
    assert_bits(ea.render(t, gs, 4), ref, "twine 2")


def test_single_target():
    lens = dict(a=0.01, b=-0.03, c=0.02, h=0.02, v=-0.01)
    kw = dict(yaw=2.0, pitch=-2.0, roll=1.0, lens=lens)
    fspec = ea.facet_spec(ea.RECTILINEAR, 80, 60, 90.0, **kw)
    a = ea.arguments.for_single(fspec, spline_degree=1, synopsis="feather")
    a.single_oracle = jobs.OracleSource(euo.RECTILINEAR, 80, 60, 90.0, jobs.synth_image(80, 60, 3, seed=1), 1, **kw)
    fs = rectilinears(4, 1)
    gs, gws = [f.gpu() for f in fs], [f.gpu_white() for f in fs]
    ref = em.model_frame_at_rays(a, fs, gs, gws, 4)
    assert np.isfinite(ref).all() and (ref != 0).mean() > 0.2
    assert_bits(ea.render(a, gs, 4), ref, "--single")


@pytest.mark.parametrize("bands", [1, 0])
def test_multiband_takes_the_new_weight(bands):
    for what, fs, a in (("fisheyes", fisheyes(4, 1), ea.arguments(ea.SPHERICAL, 96, 48, 160.0, spline_degree=1, synopsis="multiband", feather=6.0, bands=bands)),
                        ("rectilinears", rectilinears(2, 1), ea.arguments(ea.SPHERICAL, 80, 60, 120.0, spline_degree=1, synopsis="multiband", bands=bands))):
        nch = fs[0].nch
        gs = [f.gpu() for f in fs]
        ref = em.model_multiband(a, fs, nch)
        assert np.isfinite(ref).all()
        got = ea.render(a, gs, nch)
        assert_bits(got, ref, f"multiband {what} bands {bands}")
        plain = ea.render(a, [f.gpu(edges=False) for f in fs], nch)
        assert (jobs.bits(plain) != jobs.bits(got)).any()


# ---- jobs without a plane are the jobs they were ---------------------------------------------------------------------------

def load_pixels_unflagged(f):
    """the facet through eu_hip_source_load_pixels with flags == 0"""
    spec = ea.facet_spec(f.prj, f.width, f.height, f.hfov, nchannels=f.nch, **f._spec_kw())
    ptr, pch, on_device, e, hold = ea.Source._float_feed(spec, f.raw, f.masks, f.crop, f.crop_kind)
    px = ea.api.Pixels(ea.api.PX_FLOATS, ptr, pch, 0, None, None, None, None)
    return ea.Source._load_pixels(spec, px, e, f.degree, f.degree, 8, 64, 0)


@pytest.mark.parametrize("synopsis", ["feather", "multiband", "hdr_merge", "panorama"])
def test_unchanged_jobs(synopsis):
    fs = fisheyes(4, 1, edges=False)
    a = ea.arguments(ea.SPHERICAL, 96, 48, 160.0, spline_degree=1, synopsis=synopsis, feather=6.0)
    new = [load_pixels_unflagged(f) for f in fs]
    old = [f.gpu(edges=False) for f in fs]          # eu_hip_source_load_edited
    assert not any(g.has_edges for g in new + old)
    x, y = ea.render(a, new, 4), ea.render(a, old, 4)
    assert (x != 0).mean() > 0.1
    assert_bits(x, y, synopsis)
    # and planes change nothing under the synopses that have no ramp
    if synopsis in ("hdr_merge", "panorama"):
        assert_bits(ea.render(a, [f.gpu(edges=True) for f in fs], 4), y, synopsis + " with planes")
