"""Spline degrees 4, 6, 7, 8 and 9 on the device against the CPU oracle, float32 compared as uint32, 0 ULP, no pixel left
out. These degrees have no templated kernel: every call family reaches the run-time-degree evaluator
(eu_bspline_generic, and its copy in eu_render_layers.hip) through the `default:` arm of its launcher's switch over
the degree, a translated facet through launch_nd<NCH, -1>, and from degree 6 on the device prefilter runs three and
four poles (make_iir, icc / iacc, solve_line_stream and its checkpointed form in eu_setup.hip).

The render tests give the device the oracle's coefficients (Source.adopt), so a difference is the evaluator's or the
launcher's; the set-up tests compare Source.load(...).download() with the oracle's container. Sources of at most
330 x 166, targets of a few thousand pixels. The job lists, the fuzz's draw function and its seeds are in
tests/high_degree_cases.py; tests/test_high_degree_host.py replays every single-facet job of this module on the CPU:
no tap leaves its container. The oracle itself is pinned to the reference at these degrees
by tests/test_oracle_vs_ref.py and to a float64 spline by tests/test_spline64_oracle.py."""
import os

import numpy as np
import pytest

import envutil_amd as ea
import euo
import high_degree_cases as hd
import jobs
from test_gpu_feather import held as feather_held, pair as feather_pair, target as feather_target
from test_gpu_parity import assert_bits, facet_set

pytestmark = pytest.mark.gpu

DEGREES = hd.DEGREES
_pairs = {}


def pair(name, nch, degree, seed=31):
    """(oracle source, device source holding the oracle's coefficients): made once, shared"""
    key = (name, nch, degree, seed)
    if key not in _pairs:
        o = hd.oracle_source(name, nch, degree, seed)
        _pairs[key] = (o, ea.Source.adopt(hd.facet(name, nch), o.container, degree, o.bc[0], o.bc[1]))
    return _pairs[key]


@pytest.fixture(scope="module", autouse=True)
def release_sources():
    yield
    for o, g in _pairs.values():
        g.release()
    _pairs.clear()
    for os_, gs in _sets.values():
        for g in gs:
            g.release()
    _sets.clear()


_refs = {}


def oracle_frame(name, nch, degree, target, ypr, **kw):
    """the oracle's frame of a single-facet job: computed once, shared, read-only"""
    key = (name, nch, degree, target, ypr, tuple(sorted(kw.items())))
    if key not in _refs:
        r = jobs.oracle_render(hd.args_of(target, ypr, degree, **kw), pair(name, nch, degree)[0])
        r.setflags(write=False)
        _refs[key] = r
    return _refs[key]


SWITCHES = [{}, {"EU_HIP_KERNEL": "1"}, {"EU_HIP_R4": "1"}]


# ---- render, single facet -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(hd.SOURCES))
@pytest.mark.parametrize("degree", DEGREES)
def test_render_single_facet(degree, name, monkeypatch):
    """every source, 1, 3 and 4 channels, three targets upright and rotated; by default, under EU_HIP_KERNEL=1 and
    under EU_HIP_R4=1: each time the oracle's frame, from one launch. One launch rules out the staged pair and a
    frame split into runs, no more: that eu_select.h names the general kernel for these degrees under every switch is
    shown on the CPU, by test_high_degrees() of tests/csrc/select_demo.cc (tests/test_select.py)"""
    for nch in hd.CHANNELS:
        o, g = pair(name, nch, degree)
        for target in hd.TARGETS:
            for ypr in hd.YPRS:
                a = hd.args_of(target, ypr, degree)
                ref = oracle_frame(name, nch, degree, target, ypr)
                for sw in SWITCHES:
                    for k, v in sw.items():
                        monkeypatch.setenv(k, v)
                    before = ea.launch_count()
                    got = ea.render(a, g)
                    assert ea.launch_count() - before == 1, (name, degree, sw)
                    assert_bits(got, ref, f"{name} degree {degree} nch {nch} -> {target} {ypr} {sw}")
                    for k in sw:
                        monkeypatch.delenv(k)
    if name == "rectilinear":
        assert (ref == 0).all(axis=2).any() and (ref != 0).any()          # the miss path ran


@pytest.mark.parametrize("name", list(hd.SOURCES))
@pytest.mark.parametrize("degree", hd.TWINE_DEGREES)
@pytest.mark.parametrize("twine", [2, 3])
def test_twining(twine, degree, name):
    o, g = pair(name, 3, degree)
    for target, ypr in hd.TWINE_JOBS:
        a = hd.args_of(target, ypr, degree, twine=twine)
        assert_bits(ea.render(a, g), jobs.oracle_render(a, o), f"{name} degree {degree} twine {twine} -> {target}")


@pytest.mark.parametrize("degree", DEGREES)
def test_fewer_output_channels_than_the_source_has(degree):
    for name, src_n, out_n in hd.FEWER_CHANNELS:
        o, g = pair(name, src_n, degree)
        a = hd.args_of(hd.TARGETS[1], hd.YPRS[1], degree)
        assert_bits(ea.render(a, g, out_n), jobs.oracle_render(a, o, nch=out_n), f"{name} {src_n} -> {out_n} degree {degree}")


@pytest.mark.parametrize("name", ["latlon", "cubemap", "rectilinear"])
@pytest.mark.parametrize("degree", DEGREES)
def test_rows_and_bands_assemble_the_frame(degree, name):
    """rows [0, 7) [7, 20) [20, h), and bands of 4 rows dealt to three parts"""
    o, g = pair(name, 3, degree)
    for target in hd.TARGETS:
        a = hd.args_of(target, hd.YPRS[1], degree)
        ref = oracle_frame(name, 3, degree, target, hd.YPRS[1])
        h = target[2]
        rows = np.concatenate([ea.render(a, g, row_begin=r0, row_end=r1) for r0, r1 in ((0, 7), (7, 20), (20, h))])
        assert_bits(rows, ref, f"{name} degree {degree} -> {target}: row ranges")
        frame = np.full_like(ref, np.nan)
        for part in range(3):
            frame[ea.band_frame_rows(h, 4, 3, part)] = ea.render(a, g, 3, band=(4, 3, part))
        assert_bits(frame, ref, f"{name} degree {degree} -> {target}: bands")


# ---- views, layers, rays ------------------------------------------------------------------------------------------

view_args = hd.view_args


@pytest.mark.parametrize("name", hd.VIEW_SOURCES)
@pytest.mark.parametrize("degree", DEGREES)
def test_render_views(degree, name):
    """three views in one call, one with an hfov of its own"""
    o, g = pair(name, 3, degree)
    for target in hd.BATCH_TARGETS:
        got = ea.render_views(hd.args_of(target, (0, 0, 0), degree), hd.VIEWS, g)
        assert got.shape == (3, target[2], target[1], 3)
        for k, v in enumerate(hd.VIEWS):
            assert_bits(got[k], jobs.oracle_render(view_args(target, v, degree), o), f"{name} degree {degree} -> {target} view {v}")


@pytest.mark.parametrize("name", hd.LAYER_SOURCES)
@pytest.mark.parametrize("degree", DEGREES)
@pytest.mark.parametrize("twine", [0, 2])
def test_render_layers(twine, degree, name):
    """three layers: the evaluator's copy. Each layer is its own render, and the oracle's frame of its picture"""
    pairs = [pair(name, 3, degree, seed=31 + k) for k in range(3)]
    layers = [g for o, g in pairs]
    kw = dict(twine=twine) if twine else {}
    for target in hd.BATCH_TARGETS:
        a = hd.args_of(target, hd.YPRS[1], degree, **kw)
        got = ea.render_layers(a, layers)
        assert got.shape == (3, target[2], target[1], 3)
        for k, (o, g) in enumerate(pairs):
            assert_bits(got[k], ea.render(a, g), f"{name} degree {degree} twine {twine} -> {target}: layer {k} against render")
            assert_bits(got[k], jobs.oracle_render(a, o), f"{name} degree {degree} twine {twine} -> {target}: layer {k}")
        assert all((jobs.bits(got[k]) != jobs.bits(got[0])).any() for k in (1, 2))


@pytest.mark.parametrize("name", hd.RAY_SOURCES)
@pytest.mark.parametrize("degree", DEGREES)
def test_render_rays(degree, name):
    """the oracle's stage-1 rays of a job give the job's frame; the stages 1, 3 and 4 of a twined job, as ninepacks
    with its taps, the twined job's frame"""
    o, g = pair(name, 3, degree)
    for target in hd.BATCH_TARGETS:
        a = hd.args_of(target, hd.YPRS[1], degree)
        assert_bits(ea.render_rays(g, jobs.oracle_render(a, o, stage=1)), oracle_frame(name, 3, degree, target, hd.YPRS[1]),
                    f"{name} degree {degree} -> {target}: rays")
        a = hd.args_of(target, hd.YPRS[1], degree, twine=3)
        nine = np.concatenate([jobs.oracle_render(a, o, stage=k) for k in (1, 3, 4)], axis=2)
        assert_bits(ea.render_rays(g, nine, taps=a.twine_spread), jobs.oracle_render(a, o), f"{name} degree {degree} -> {target}: ninepacks")


# ---- multi-facet jobs ---------------------------------------------------------------------------------------------

MULTI_LENS = dict(a=0.01, b=-0.03, c=0.02)
_sets = {}


def fish(nch, degree):
    """six fisheye facets 64 x 64 of 140 degrees with the lens polynomial: (oracle sources, device sources)"""
    key = (nch, degree)
    if key not in _sets:
        _sets[key] = facet_set(euo.FISHEYE, 64, 64, 140.0, nch, degree, MULTI_LENS)
    return _sets[key]


@pytest.mark.parametrize("degree", DEGREES)
@pytest.mark.parametrize("synopsis,nch", [("panorama", 3), ("panorama", 4), ("hdr_merge", 2), ("hdr_merge", 4)])
def test_six_fisheye_facets(synopsis, nch, degree):
    os_, gs = fish(nch, degree)
    for target, ypr in ((hd.TARGETS[1], hd.YPRS[1]), (hd.TARGETS[0], hd.YPRS[1])):
        a = hd.args_of(target, ypr, degree, synopsis=synopsis)
        ref = jobs.oracle_render(a, os_)
        assert_bits(ea.render(a, gs, nch), ref, f"{synopsis} nch {nch} degree {degree} -> {target}")
        assert (ref[:, :, 0] != 0).mean() > 0.5


@pytest.mark.parametrize("degree", [4, 8, 9])
def test_render_views_multi(degree):
    os_, gs = fish(3, degree)
    target = hd.TARGETS[1]
    got = ea.render_views(hd.args_of(target, (0, 0, 0), degree), hd.VIEWS, gs, 3)
    for k, v in enumerate(hd.VIEWS):
        assert_bits(got[k], jobs.oracle_render(view_args(target, v, degree), os_), f"views of six facets, degree {degree}, view {v}")


@pytest.mark.parametrize("degree", [4, 9])
def test_feathered_seams(degree):
    """tests/feather_model.py takes the degree: two overlapping rectilinear facets, with and without alpha"""
    for nch, tw, th in ((3, 67, 38), (4, 96, 40)):
        got, gs = feather_held(f"feather degree {degree} nch {nch}", feather_target(tw, th, spline_degree=degree, feather=6.0),
                               feather_pair(nch, degree), nch)
        for g in gs:
            g.release()


@pytest.mark.parametrize("degree", hd.TRANSLATED_DEGREES)
def test_translated_facet(degree):
    """definitions64.translated_facet() goes to the generic stepper and launch_nd<NCH, -1>: the run-time-degree kernel
    at every degree. At degree 3 it must give what the oracle gives, as the templated kernel does for other facets"""
    o, spec = hd.translated_source(degree)
    ol = hd.oracle_source("latlon", 3, degree)
    g = ea.Source.adopt(spec, o.container, degree, o.bc[0], o.bc[1])
    gl = ea.Source.adopt(hd.facet("latlon", 3), ol.container, degree, ol.bc[0], ol.bc[1])
    try:
        for ypr, twine in hd.TRANSLATED_JOBS:
            a = hd.args_of(hd.TRANSLATED_TARGET, ypr, degree, twine=twine)
            ref = jobs.oracle_render(a, o)
            assert_bits(ea.render(a, g), ref, f"translated facet degree {degree} {ypr} twine {twine}")
            assert (ref != 0).mean() > 0.5
        # a --single target recreates a facet through the same stepper
        a = hd.single_target_args(degree)
        assert_bits(ea.render(a, gl), jobs.oracle_render(a, ol), f"--single target, degree {degree}")
    finally:
        g.release()
        gl.release()


# ---- device set-up: Source.load(...).download() against the oracle's container ---------------------------------------

SETUP_DEGREES = (4, 6, 8, 9)


class iir_stream:
    """EU_HIP_IIR_STREAM: unset - streamed with checkpoints; 3 - streamed, four passes per axis; 0 - one thread per line"""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        self.keep = os.environ.pop("EU_HIP_IIR_STREAM", None)
        if self.mode is not None:
            os.environ["EU_HIP_IIR_STREAM"] = self.mode

    def __exit__(self, *a):
        os.environ.pop("EU_HIP_IIR_STREAM", None)
        if self.keep is not None:
            os.environ["EU_HIP_IIR_STREAM"] = self.keep


def loaded(prj, w, h, hfov, img, degree, pdeg=None, **kw):
    g = ea.Source.load(ea.facet_spec(prj, w, h, hfov, nchannels=img.shape[2]), img, degree, pdeg, **kw)
    got = g.download()
    g.release()
    return got


@pytest.mark.parametrize("sw,sh", [(200, 100), (330, 166)])
@pytest.mark.parametrize("degree", SETUP_DEGREES)
def test_full_sphere_prefilter(degree, sw, sh):
    """the 2H line of 200 samples makes three full blocks of 64, so the checkpointed form runs; 330 x 166 leaves
    remainders on every axis. 1 to 4 channels, every form of the kernels"""
    for nch in (1, 2, 3, 4):
        img = jobs.synth_image(sw, sh, nch, seed=21 + nch)
        want = jobs.OracleSource(euo.SPHERICAL, sw, sh, 360.0, img, degree).container
        for mode in (None, "3", "0"):
            with iir_stream(mode):
                assert_bits(loaded(ea.SPHERICAL, sw, sh, 360.0, img, degree), want,
                            f"full sphere {sw} x {sh} x {nch} degree {degree} EU_HIP_IIR_STREAM {mode}")


@pytest.mark.parametrize("sprj,sw,sh,shfov", [(euo.CYLINDRICAL, 200, 70, 360.0), (euo.STEREOGRAPHIC, 97, 201, 120.0)])
@pytest.mark.parametrize("degree", SETUP_DEGREES)
def test_ordinary_prefilter(degree, sprj, sw, sh, shfov):
    """PERIODIC / REFLECT and REFLECT / REFLECT"""
    for nch in (1, 3, 4):
        img = jobs.synth_image(sw, sh, nch, seed=5 + nch)
        want = jobs.OracleSource(sprj, sw, sh, shfov, img, degree).container
        for mode in (None, "3", "0"):
            with iir_stream(mode):
                assert_bits(loaded(sprj, sw, sh, shfov, img, degree), want,
                            f"projection {sprj} {sw} x {sh} x {nch} degree {degree} EU_HIP_IIR_STREAM {mode}")


@pytest.mark.parametrize("sw,sh", [(9, 34), (20, 33), (33, 20), (34, 9), (9, 9), (33, 34)])
@pytest.mark.parametrize("degree", SETUP_DEGREES)
def test_lines_no_longer_than_the_horizon(degree, sw, sh):
    """at degree 9 the last pole's horizon is about 33 samples: lines of 9, 20, 33 and 34 take the closed-form start
    values of icc / iacc with up to four poles; REFLECT and PERIODIC rows"""
    for sprj, hfov in ((euo.RECTILINEAR, 60.0), (euo.CYLINDRICAL, 360.0)):
        for nch in (1, 3):
            img = jobs.synth_image(sw, sh, nch, seed=sw * 31 + sh)
            want = jobs.OracleSource(sprj, sw, sh, hfov, img, degree).container
            for mode in (None, "0"):
                with iir_stream(mode):
                    assert_bits(loaded(sprj, sw, sh, hfov, img, degree), want,
                                f"short lines {sw} x {sh} x {nch} projection {sprj} degree {degree} EU_HIP_IIR_STREAM {mode}")


@pytest.mark.parametrize("sw,sh", [(2, 40), (40, 2), (3, 3), (1, 30)])
@pytest.mark.parametrize("degree", [8, 9])
def test_sources_narrower_than_the_frame(degree, sw, sh):
    """the narrow cores of tests/test_gpu_prefilter_stream.py, whose brace is wider than the core"""
    for sprj, hfov in ((euo.RECTILINEAR, 60.0), (euo.CYLINDRICAL, 360.0), (euo.SPHERICAL, 90.0)):
        for nch in (1, 3):
            img = jobs.synth_image(sw, sh, nch, seed=sw * 31 + sh)
            want = jobs.OracleSource(sprj, sw, sh, hfov, img, degree).container
            assert_bits(loaded(sprj, sw, sh, hfov, img, degree), want, f"narrow {sw} x {sh} x {nch} projection {sprj} degree {degree}")


@pytest.mark.parametrize("face", [33, 64, 100])
@pytest.mark.parametrize("degree", SETUP_DEGREES)
def test_cubemap_ir(degree, face):
    """the intermediate image with the default frame (support_min 8) and with the smallest a degree-d window needs"""
    faces = jobs.synth_cubefaces(face, 3)
    for support_min in (8, degree // 2 + 1):
        want = jobs.OracleSource(euo.CUBEMAP, face, 6 * face, 90.0, faces, degree, support_min=support_min).container
        assert_bits(loaded(ea.CUBEMAP, face, 6 * face, 90.0, faces, degree, support_min=support_min), want,
                    f"cubemap IR face {face} degree {degree} support_min {support_min}")


@pytest.mark.parametrize("degree,pdeg", [(9, 3), (4, 9)])
def test_prefilter_degree_other_than_the_spline_degree(degree, pdeg):
    for prj, w, h, hfov in ((euo.SPHERICAL, 128, 64, 360.0), (euo.RECTILINEAR, 97, 65, 80.0), (euo.CUBEMAP, 33, 198, 90.0)):
        img = jobs.synth_cubefaces(w, 3) if hd.cube(prj) else jobs.synth_image(w, h, 3, seed=9)
        o = jobs.OracleSource(prj, w, h, hfov, img, degree, pdeg)
        assert_bits(loaded(prj, w, h, hfov, img, degree, pdeg), o.container, f"projection {prj} degree {degree} prefilter {pdeg}")


def test_reload_and_integer_samples():
    """they share the launchers: one reload at degree 8, one load of 8-bit samples at degree 9"""
    prj, w, h, hfov = hd.RELOAD_SOURCE
    first, second = hd.reload_pictures()
    g = ea.Source.load(ea.facet_spec(prj, w, h, hfov), first, hd.RELOAD_DEGREE)
    try:
        g.reload(second)
        o = jobs.OracleSource(prj, w, h, hfov, second, hd.RELOAD_DEGREE)
        assert_bits(g.download(), o.container, "reloaded full sphere, degree 8")
        a = hd.args_of(*hd.RELOAD_JOB, hd.RELOAD_DEGREE)
        assert_bits(ea.render(a, g), jobs.oracle_render(a, o), "a render after the reload")
    finally:
        g.release()
    s = np.random.default_rng(8).integers(0, 256, (45, 67, 3), dtype=np.uint8)
    g = ea.Source.load_samples(ea.facet_spec(ea.RECTILINEAR, 67, 45, 70.0), s, spline_degree=9)
    try:
        o = jobs.OracleSource(euo.RECTILINEAR, 67, 45, 70.0, s.astype(np.float32) / np.float32(255.0), 9)
        assert_bits(g.download(), o.container, "8-bit samples, degree 9")
    finally:
        g.release()


# ---- fuzz ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", hd.FUZZ_SEEDS)
def test_random_high_degree_jobs_bit_identical(seed):
    """hd.fuzz_jobs: five jobs per seed, degrees drawn from 4 to 9; single-facet and multi-facet jobs, twining, crops,
    channel adaption"""
    for job in hd.fuzz_jobs(seed):
        os_ = [f[0] for f in job["facets"]]
        gs = [ea.Source.adopt(spec, o.container, job["degree"], o.bc[0], o.bc[1]) for o, spec, _, _ in job["facets"]]
        try:
            got = ea.render(job["args"], gs, job["out_n"])
            ref = jobs.oracle_render(job["args"], os_ if len(os_) > 1 else os_[0], nch=job["out_n"])
            assert_bits(got, ref, job["what"])
        finally:
            for g in gs:
                g.release()


# ---- several device slots: LAST in this file ----------------------------------------------------------------------
# eu_hip_init_devices cannot be undone: from here on the process has three slots (as after tests/test_gpu_multidevice.py,
# which lists the same three). Plain renders stay on slot 0.

def test_render_devices():
    """three slots of the one device, degree 9"""
    ea.lib()
    ea.init_devices([0, 0, 0])
    assert ea.device_slots() == 3
    for name in ("latlon", "fisheye"):
        o, g = pair(name, 3, 9)
        for target in hd.TARGETS:
            a = hd.args_of(target, hd.YPRS[1], 9)
            assert_bits(ea.render_devices(a, g, 3), oracle_frame(name, 3, 9, target, hd.YPRS[1]), f"{name} over three slots -> {target}")
    os_, gs = fish(4, 9)
    a = hd.args_of(hd.TARGETS[1], hd.YPRS[1], 9)
    assert_bits(ea.render_devices(a, gs, 4), jobs.oracle_render(a, os_), "six facets over three slots")
