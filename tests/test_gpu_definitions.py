"""The HIP library's PIXELS against the float64 model of tests/definitions64.py - never against the oracle, which
this module does not load: pixels in (Source.load: the device bracing, prefilter and cube frame fill), pixels out,
the product alone. One small case per kernel family, at the shapes of definitions64's case lists (widths that fill
neither a 16 x 8 wave tile, a 32 x 16 tile, a 64-pixel tile nor a 128-pixel strip), camera upright and rotated.

The tolerances are those of tests/test_oracle_definitions.py: the ENVELOPES table of definitions64, measured with
the CPU oracle against the model, by source kind, degree and distance from the seam, the poles, the cube face
edges and the image border. There are no numbers of the GPU's own: the library is bit-identical to the oracle, so
the envelope holds unchanged, and where it does not, that is a finding. Pixels that the model says no facet covers
(by more than two texels) are exactly zero."""
import numpy as np
import pytest

import definitions64 as d
import envutil_amd as ea

pytestmark = pytest.mark.gpu

_sources = {}


def load(f, nch, degree):
    key = (f.prj, f.w, f.h, f.hfov, f.yaw, f.pitch, f.roll, f.brighten, tuple(sorted((f.lens or {}).items())),
           tuple(sorted((f.translation or {}).items())), nch, degree)
    if key not in _sources:
        spec = ea.facet_spec(f.prj, f.w, f.h, f.hfov, nchannels=nch, yaw=f.yaw, pitch=f.pitch, roll=f.roll,
                             brighten=f.brighten, lens=f.lens, translation=f.translation)
        _sources[key] = ea.Source.load(spec, d.facet_image(f, nch), degree)
    return _sources[key]


@pytest.fixture(scope="module", autouse=True)
def release_sources():
    yield
    for s in _sources.values():
        s.release()
    _sources.clear()


def gpu_render(facets, degree, args, nch):
    srcs = [load(f, nch, degree) for f in facets]
    return ea.render(args, srcs if len(srcs) > 1 else srcs[0], nch)


def check(got, a, facets, nch, degree, what, kind=None):
    j = d.judge(got, a, facets, nch)
    kind = kind or (d.kind_of(facets[0]) if len(facets) == 1 else ("plain", 0))
    print(what, kind, degree, j.bins(), "outside", j.outside_max)
    assert j.covered_share >= 0.5, what
    assert j.outside_max == 0.0, what
    d.assert_within(j, kind, degree, what)
    return j


FAMILIES = {"default": {}, "general": {"EU_HIP_KERNEL": "1"}, "direct": {"EU_HIP_KERNEL": "1", "EU_HIP_DIRECT": "1"},
            "packed": {"EU_HIP_R4": "0", "EU_HIP_HYBRID": "2"}}

SINGLE = d.single_sources()
FISH = d.PLAIN["fisheye"]


@pytest.mark.parametrize("source", list(SINGLE))
@pytest.mark.parametrize("family", list(FAMILIES))
def test_single_facet_kernels(family, source, monkeypatch):
    """the general kernel with and without LDS staging, the packed kernels (and packed in runs), and what the
    library picks by itself; 3 channels at degrees 2 and 3, 1 and 4 channels at degree 3"""
    for k, v in FAMILIES[family].items():
        monkeypatch.setenv(k, v)
    f = SINGLE[source]
    for degree, nch in ((3, 3), (2, 3), (3, 4), (3, 1)):
        for t, ypr in d.jobs_of(f):
            a = d.make_args(t, ypr, degree)
            check(gpu_render([f], degree, a, nch), a, [f], nch, degree, f"{family} {source} nch {nch} -> {t} {ypr}")


STAGED_SWITCHES = [{}, {"EU_HIP_SHARE": "0"}, {"EU_HIP_BOXTAB": "0"}]


@pytest.mark.parametrize("nch", [3, 4])
@pytest.mark.parametrize("degree", [2, 3])
def test_staged_kernels(degree, nch, monkeypatch):
    """EU_HIP_R4=1: lat/lon onto the upright cubemap (column plans, follower tiles, the polar faces' second loop),
    the sphere and a rotated window, with shared rows and box tables as by default and each switched off; a cube
    source onto the sphere and a rotated window"""
    monkeypatch.setenv("EU_HIP_R4", "1")
    for f, targets in ((d.LATLON[256], [(d.T_CUBE48, d.UPRIGHT), (d.T_CUBE24, d.UPRIGHT), (d.T_SPH, d.UPRIGHT), (d.T_RECT, d.ROTATED),
                                       (d.T_CUBE48, d.ROTATED)]),
                       (d.LATLON[128], [(d.T_CUBE48, d.UPRIGHT), (d.T_SPH, d.ROTATED)]),
                       (d.CUBES[("cubemap", 64)], [(d.T_SPH, d.UPRIGHT), (d.T_RECT, d.ROTATED)]),
                       (d.CUBES[("cubemap", 32)], [(d.T_SPH, d.UPRIGHT), (d.T_RECT, d.ROTATED)])):
        for t, ypr in targets:
            a = d.make_args(t, ypr, degree)
            for sw in STAGED_SWITCHES:
                for k in ("EU_HIP_SHARE", "EU_HIP_BOXTAB"):
                    monkeypatch.delenv(k, raising=False)
                for k, v in sw.items():
                    monkeypatch.setenv(k, v)
                check(gpu_render([f], degree, a, nch), a, [f], nch, degree, f"staged {d.kind_of(f)} nch {nch} -> {t} {ypr} {sw}")


def check_views(facets, t, views, degree, nch, what, **kw):
    a = d.make_args(t, d.UPRIGHT, degree, **kw)
    srcs = [load(f, nch, degree) for f in facets]
    out = ea.render_views(a, views, srcs if len(srcs) > 1 else srcs[0], nch)
    assert out.shape == (len(views), t[2], t[1], nch)
    for k, (tk, ypr) in enumerate(d.view_jobs(t, views)):
        check(out[k], d.make_args(tk, ypr, degree, **kw), facets, nch, degree, f"{what} view {views[k]}")


@pytest.mark.parametrize("general", [False, True])
def test_render_views(general, monkeypatch):
    """three views of a resident source in one call, one with an hfov of its own: packed and general kernels"""
    if general:
        monkeypatch.setenv("EU_HIP_KERNEL", "1")
    for name, fs, t, syn, views in d.view_cases()[:2]:
        for degree in (2, 3):
            check_views(fs, t, views, degree, 3, f"views {name} general {general}")


@pytest.mark.parametrize("nch", [3, 4])
def test_render_views_of_six_facets(nch):
    """a six-facet list in one call: panorama (holes: exact zeros) and an hdr_merge bracket"""
    for name, fs, t, syn, views in d.view_cases()[2:]:
        check_views(fs, t, views, 3, nch, name, synopsis=syn)


@pytest.mark.parametrize("general", [False, True])
def test_render_rays(general, monkeypatch):
    """`act` alone: the caller's rays, made in float64 from the definitions and rounded to float32, three inputs;
    and ninepacks {ray, x-neighbour, y-neighbour}. A ninepack's neighbours lie a QUARTER of a pixel away (the bias
    of the reference's deriv_stepper; the library scales the taps by its reciprocal, as twine_t's set-up does).
    These belong to a rectilinear target and are not normalised, so ray + 4 dx (ray_x - ray) + 4 dy (ray_y - ray)
    IS the ray of the planar coordinate offset by (dx, dy) pixels: the tap sum is the model's weighted sum to the
    float32 floor, whatever the size of the target"""
    if general:
        monkeypatch.setenv("EU_HIP_KERNEL", "1")
    for f in (d.LATLON[256], d.CUBES[("cubemap", 64)], FISH):
        for degree in (2, 3):
            src = load(f, 3, degree)
            for t, ypr in ((d.T_RECT, d.ROTATED), (d.T_SPH, d.ROTATED)) if f is not FISH else (d.looking_at(f),):
                a = d.make_args(t, ypr, degree)
                rays = (d.camera_rays(a) @ f.matrix).astype(np.float32)          # in the source's frame
                check(ea.render_rays(src, rays), a, [f], 3, degree, f"rays {d.kind_of(f)} -> {t} general {general}")
            for twine in (2, 3):
                t, ypr = d.looking_at(f) if f is FISH else (d.T_RECT, d.ROTATED)
                a = d.make_args(t, ypr, degree, twine=twine)
                nine = np.concatenate([d.camera_rays(a, dx, dy) @ f.matrix for dx, dy in ((0, 0), (0.25, 0), (0, 0.25))], -1)
                got = ea.render_rays(src, nine.astype(np.float32), taps=a.twine_spread)
                # the taps of a pixel reach into the neighbouring bins: judged where all of them are in the last one
                j = d.judge(got, a, [f], 3)
                far = j.counted & (j.dist >= 10.0)
                print("ninepacks", d.kind_of(f), degree, twine, general, far.mean(), j.err[far].max())
                assert far.mean() > 0.04 and j.err[far].max() <= d.floor_tolerance(degree)


@pytest.mark.parametrize("nch", [3, 4])
@pytest.mark.parametrize("degree", [2, 3])
@pytest.mark.parametrize("case", d.synopsis_cases(), ids=lambda c: c[0])
def test_multi_facet_render(case, degree, nch):
    """panorama of six facets with holes, an hdr_merge bracket, and a job with lens-polynomial facets"""
    name, fs, t, ypr, syn = case
    a = d.make_args(t, ypr, degree, synopsis=syn)
    j = check(gpu_render(fs, degree, a, nch), a, fs, nch, degree, f"{name} nch {nch}")
    assert j.outside.any()


def test_twined_render():
    """the twined job of the CPU module, on the device: the envelope of the twining sum"""
    for n, f, t, ypr, _ in d.twine_cases():
        a = d.make_args(t, ypr, 3, twine=n)
        j = d.judge(gpu_render([f], 3, a, 3), a, [f], 3)
        print("twine", n, j.max())
        assert j.covered_share >= 0.5 and j.max() <= d.BIN_MARGIN * d.ENVELOPES[("twine", n)]


@pytest.mark.parametrize("degree", [2, 3])
def test_translated_facet(degree):
    """TrX, TrY, TrZ, Tpy, Tpp against plain geometry: see tests/test_oracle_definitions.py"""
    f = d.translated_facet()
    for t, ypr in (((d.RECTILINEAR, 150, 77, 60.0), (5.0, -2.0, 0.0)), ((d.RECTILINEAR, 150, 77, 60.0), (12.0, 4.0, 8.0))):
        a = d.make_args(t, ypr, degree)
        j = d.judge_translated(gpu_render([f], degree, a, 3), a, f, 3)
        print("translated", degree, ypr, j.bins())
        assert j.covered_share >= 0.5 and j.far_max() <= d.floor_tolerance(degree)
