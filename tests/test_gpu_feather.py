"""Feathered seams on the device (--synopsis feather, EU_SYN_FEATHER: eu_synopsis_feather in eu_multi_dev.h) against
the numpy model of tests/feather_model.py, bit for bit, whole frames; and the calls behind a render against render().
Small jobs: targets around 96 x 40 (widths 67 and 129 - a second and a third 64-pixel tile with a few lanes -, a height
that is no multiple of the 4-row tile), facets around 48 x 32. Pixels are finite throughout."""
import math
import os
import subprocess

import numpy as np
import pytest

import envutil_amd as ea
import euo
import jobs
import feather_model as fm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "envutil_amd", "bin", "envutil_hip")


def assert_bits(got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    d = jobs.bits(got) != jobs.bits(ref)
    assert not d.any(), f"{what}: {int(d.sum())} of {d.size} values differ, first at {np.argwhere(d)[0]}: " \
                        f"{got[tuple(np.argwhere(d)[0])]!r} model {ref[tuple(np.argwhere(d)[0])]!r}"


def target(w=96, h=40, hfov=120.0, **kw):
    return ea.arguments(ea.SPHERICAL, w, h, hfov, synopsis="feather", **kw)


def pair(nch, degree, seed=40, **kw):
    """two rectilinear facets of 48 x 32 that overlap in the middle of the target"""
    out = []
    for k in range(2):
        img = jobs.synth_image(48, 32, nch, seed=seed + k)
        out.append(fm.Facet(euo.RECTILINEAR, 48, 32, 50.0, img, degree, yaw=-14.0 + 29.0 * k, pitch=2.0 * k - 1.0,
                            roll=3.0 * k, brighten=1.0 + 0.25 * k, **kw))
    return out


def held(what, a, fs, nch, overlap=20):
    """the device's frame against the model's, through the single-facet stages; returns (frame, sources)"""
    gs = [f.gpu() for f in fs]
    ref, qsum, count = fm.model_frame(a, fs, nch, details=True)
    assert np.isfinite(ref).all()
    assert (count >= 2).sum() >= overlap, f"{what}: {(count >= 2).sum()} pixels see more than one facet"
    got = ea.render(a, gs, nch)
    assert_bits(got, ref, what)
    return got, gs


# ---- single calls against the model -----------------------------------------------------------------------------

@pytest.mark.parametrize("width", [0.0, 6.0, 1000.0])
@pytest.mark.parametrize("degree,tw,th", [(0, 96, 40), (1, 67, 38), (3, 129, 41)])
def test_two_rectilinear_facets(degree, tw, th, width):
    a = target(tw, th, spline_degree=degree, feather=width)
    got, gs = held(f"two facets degree {degree} {tw} x {th} width {width}", a, pair(3, degree), 3)
    # the same facets as a panorama give something else: the synopsis reaches the kernel
    pano = ea.render(ea.arguments(ea.SPHERICAL, tw, th, 120.0, spline_degree=degree), gs, 3)
    assert (jobs.bits(pano) != jobs.bits(got)).any()


@pytest.mark.parametrize("nch", [2, 4])
@pytest.mark.parametrize("degree", [0, 1])
def test_alpha_planes_around_the_gate(nch, degree):
    """alpha 0, values on both sides of the gate 1e-6, and 1, in stripes that cross the overlap; the colour is associated"""
    fs = []
    for k in range(2):
        img = jobs.synth_image(48, 32, nch, seed=70 + k)
        yy, xx = np.mgrid[0:32, 0:48]
        a = np.choose(((xx + 5 * k) // 4 + yy // 6) % 5, [0.0, 5e-7, 2e-6, 1.0, 0.5]).astype(np.float32)
        img[:, :, nch - 1] = a
        img[:, :, :nch - 1] *= a[:, :, None]
        fs.append(fm.Facet(euo.RECTILINEAR, 48, 32, 50.0, img, degree, yaw=-12.0 + 25.0 * k, pitch=1.0 - 2.0 * k,
                           brighten=1.0 + 0.5 * k))
    got, _ = held(f"alpha nch {nch} degree {degree}", target(spline_degree=degree, feather=9.0), fs, nch)
    al = got[:, :, nch - 1]
    assert (al == 0).any() and (al == 1).any() and ((al > 0) & (al < 1e-6)).any() and ((al > 1e-6) & (al < 1e-5)).any()


def test_one_and_four_channel_facets_on_three_channels():
    fs = [fm.Facet(euo.RECTILINEAR, 48, 32, 50.0, jobs.synth_image(48, 32, 1, seed=80), 1, yaw=-13.0, brighten=1.2),
          fm.Facet(euo.RECTILINEAR, 48, 32, 50.0, jobs.synth_image(48, 32, 4, seed=81), 1, yaw=14.0, pitch=2.0, roll=-2.0)]
    held("1 + 4 channels -> 3", target(67, 38, spline_degree=1), fs, 3)
    # and as misses: a facet of another channel count that the ray misses contributes nothing, not its adapted zero pixel
    held("1 + 4 channels -> 4", target(67, 38, spline_degree=1), fs[::-1], 4)


def test_fisheye_window_and_full_sphere():
    lens = dict(a=0.01, b=-0.03, c=0.02, h=0.02, v=-0.01, g=0.01, t=-0.02)
    fs = [fm.Facet(euo.FISHEYE, 40, 40, 100.0, jobs.synth_image(40, 40, 3, seed=90), 1, yaw=-20.0, pitch=3.0, roll=5.0, lens=lens),
          fm.Facet(euo.RECTILINEAR, 56, 36, 60.0, jobs.synth_image(40, 24, 3, seed=91), 1, yaw=16.0, pitch=-2.0,
                   window=(40, 24, 6, 5), brighten=0.8),
          fm.Facet(euo.SPHERICAL, 64, 32, 360.0, jobs.synth_image(64, 32, 3, seed=92), 1, yaw=30.0)]
    assert fs[2].border == (False, False) and fs[1].win == (40, 24)
    a = target(129, 41, hfov=200.0, yaw=4.0, pitch=-3.0, roll=2.0, spline_degree=1)
    ref, qsum, count = fm.model_frame(a, fs, 3, details=True)
    assert (count == 3).sum() > 20 and (count == 2).sum() > 100 and (count >= 1).all()
    held("fisheye + window + sphere", a, fs, 3)


def test_cubemap_source():
    fs = [fm.Facet(euo.CUBEMAP, 16, 96, 90.0, jobs.synth_cubefaces(16, 3), 1, yaw=10.0),
          fm.Facet(euo.RECTILINEAR, 48, 32, 50.0, jobs.synth_image(48, 32, 3, seed=95), 1, yaw=5.0, brighten=1.3)]
    assert fs[0].border == (False, False)
    held("cubemap + rectilinear", target(spline_degree=1, feather=5.0), fs, 3)


def test_sixty_six_facets():
    """no per-facet state: more facets than the alpha compositing has mask bits, with and without alpha"""
    for nch in (3, 4):
        fs = [fm.Facet(euo.RECTILINEAR, 8, 8, 30.0, jobs.synth_image(8, 8, nch, seed=200 + k), 1, yaw=5.2 * k - 170.0,
                       pitch=10.0 * math.sin(1.3 * k), roll=4.0 * k, brighten=0.7 + 0.01 * k) for k in range(66)]
        held(f"66 facets nch {nch}", target(96, 40, hfov=360.0, spline_degree=1), fs, nch, overlap=200)


def test_mask_for_is_the_blend_weight():
    """--mask_for 1: facet 1 painted white, facet 0 black - the frame is facet 1's normalised weight"""
    fs = pair(3, 1)
    for k, f in enumerate(fs):
        fs[k] = fm.Facet(f.prj, f.width, f.height, f.hfov, jobs.synth_image(48, 32, 3, seed=40 + k), 1, **dict(f.kw, masked=k, brighten=1.0))
    got, _ = held("mask_for", target(spline_degree=1), fs, 3)
    assert got.min() == 0.0 and got.max() == 1.0 and ((got > 0) & (got < 1)).sum() > 60


# ---- the route through the rays: generic stepper, twining ---------------------------------------------------------

def held_at_rays(what, a, fs, nch):
    gs, gws = [f.gpu() for f in fs], [f.gpu_white() for f in fs]
    ref = fm.model_frame_at_rays(a, fs, gs, gws, nch)
    assert np.isfinite(ref).all() and (ref != 0).mean() > 0.2
    got = ea.render(a, gs, nch)
    assert_bits(got, ref, what)
    return got, gs


def test_the_two_routes_agree():
    """the model through the single-facet stages and through the rays: one frame"""
    a, fs = target(67, 38, spline_degree=1), pair(3, 1)
    gs, gws = [f.gpu() for f in fs], [f.gpu_white() for f in fs]
    assert_bits(fm.model_frame_at_rays(a, fs, gs, gws, 3), fm.model_frame(a, fs, 3), "rays against stages")


def test_translated_facet_and_rectilinear_target():
    fs = pair(3, 1)
    fs[1] = fm.Facet(euo.RECTILINEAR, 48, 32, 50.0, jobs.synth_image(48, 32, 3, seed=41), 1, yaw=12.0, pitch=1.0,
                     translation=dict(x=0.1, y=-0.05, z=0.04, tp_y=3.0, tp_p=-2.0))
    a = ea.arguments(ea.RECTILINEAR, 96, 40, 80.0, spline_degree=1, synopsis="feather", feather=10.0)
    held_at_rays("translated facet", a, fs, 3)


def test_single_target():
    """--single: the target recreates a facet with lens polynomial and shift; every facet goes through the generic stepper"""
    lens = dict(a=0.01, b=-0.03, c=0.02, h=0.02, v=-0.01)
    kw = dict(yaw=4.0, pitch=-2.0, roll=1.0, lens=lens)
    fspec = ea.facet_spec(ea.RECTILINEAR, 96, 40, 70.0, **kw)
    a = ea.arguments.for_single(fspec, spline_degree=1, synopsis="feather")
    a.single_oracle = jobs.OracleSource(euo.RECTILINEAR, 96, 40, 70.0, jobs.synth_image(96, 40, 3, seed=1), 1, **kw)
    held_at_rays("--single", a, pair(3, 1), 3)


def test_twined_job():
    """twine 3: the model per tap ray - eu_syn_ray's rays from the three steppers of each facet's single-facet twined
    job, pixel and hit through render_rays, coordinates through the oracle - and the kernel's weighted sum"""
    a = target(67, 38, spline_degree=1, twine=3, feather=7.0)
    got, gs = held_at_rays("twine 3", a, pair(3, 1), 3)
    views = [(0.0, 0.0, 0.0)]
    assert_bits(ea.render_views(a, views, gs, nchannels=3)[0], got, "twined view against render")


def test_twined_job_with_alpha_and_taps_at_the_centre():
    fs = pair(4, 1, seed=44)
    a = target(67, 38, spline_degree=1, twine=2, feather=7.0)
    held_at_rays("twine 2, alpha", a, fs, 4)
    # taps that all sit at (0, 0): every tap sees the untwined job's ray
    a0 = target(67, 38, spline_degree=1, feather=7.0)
    b = target(67, 38, spline_degree=1, feather=7.0)
    b.twine_spread = np.array([[0, 0, 0.25], [0, 0, 0.5], [0, 0, 0.25]], np.float32)
    gs = [f.gpu() for f in fs]
    one = fm.model_frame(a0, fs, 4)
    want = np.zeros_like(one)
    for w in (0.25, 0.5, 0.25):
        want = fm.f32(want + fm.f32(np.float32(w) * one))
    assert_bits(ea.render(b, gs, 4), want, "taps at the centre")


# ---- the calls behind a render --------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def job():
    a = target(129, 41, spline_degree=1)
    fs = pair(3, 1)
    gs = [f.gpu() for f in fs]
    ref = fm.model_frame(a, fs, 3)
    whole = ea.render(a, gs, 3)
    assert_bits(whole, ref, "the shared job")
    return a, fs, gs, whole


def test_row_range_crop_and_bands(job):
    a, fs, gs, whole = job
    assert_bits(ea.render(a, gs, 3, row_begin=5, row_end=23), whole[5:23], "rows 5..23")
    # A crop window that starts at column 0 is its slice of the whole frame. One that starts elsewhere is not, under
    # any synopsis and in the oracle too: the steppers' column arithmetic starts at the window (a lane's start plus
    # steps of 16 columns), so the rays differ in their last bits - 1543 values of this job's PANORAMA frame
    # differ from the slice in the oracle. Such a window is held to the model of the cropped job instead, bit for bit.
    c = target(129, 41, spline_degree=1, crop=(0, 101, 6, 33))
    assert_bits(ea.render(c, gs, 3), whole[6:33, 0:101], "crop window from column 0")
    c = target(129, 41, spline_degree=1, crop=(30, 101, 6, 33))
    assert_bits(ea.render(c, gs, 3), fm.model_frame(c, fs, 3), "crop window from column 30")
    for index in range(2):
        rows = ea.band_frame_rows(41, 4, 2, index)
        assert_bits(ea.render(a, gs, 3, band=(4, 2, index)), whole[rows], f"bands of part {index}")


def test_views_in_chunks(job, monkeypatch):
    a, fs, gs, whole = job
    views = [(0.0, 0.0, 0.0), (8.0, -3.0, 2.0), (-11.0, 4.0, -5.0, 100.0)]
    monkeypatch.setenv("EU_HIP_VIEWS_MAX_KB", "1")
    got = ea.render_views(a, views, gs, nchannels=3)
    assert_bits(got[0], whole, "view 0 is the job")
    for k, v in enumerate(views):
        b = target(129, 41, hfov=v[3] if len(v) == 4 else 120.0, yaw=v[0], pitch=v[1], roll=v[2], spline_degree=1)
        assert_bits(got[k], ea.render(b, gs, 3), f"view {k}")
    assert (jobs.bits(got[1]) != jobs.bits(got[0])).any()


def test_guarded_device_output(job):
    import devout
    a, fs, gs, whole = job
    frame, outside, _ = devout.render_dev(a, gs, 3, pad=5, lead=3)
    devout.check("feather into a padded device buffer", frame, outside, whole)


def test_render_samples(job):
    a, fs, gs, whole = job
    for bits in (8, 16):
        got = ea.render_samples(a, gs, 3, bits=bits)
        assert (got == ea.encode_samples(whole, bits=bits)).all(), f"{bits}-bit samples"


def write_pfm(path, img):
    h, w = img.shape[:2]
    with open(path, "wb") as f:
        f.write({1: b"Pf", 3: b"PF", 4: b"PF4"}[img.shape[2]] + b"\n%d %d\n-1.0\n" % (w, h))
        f.write(np.ascontiguousarray(img[::-1], "<f4").tobytes())


def test_command_line_pto(tmp_path):
    if not os.path.exists(EXE) or not os.path.exists(ea.lib_path()):
        ea.build()
    imgs = [jobs.synth_image(48, 32, 3, seed=40 + k) for k in range(2)]
    for k, img in enumerate(imgs):
        write_pfm(tmp_path / f"f{k}.pfm", img)
    (tmp_path / "two.pto").write_text('p f2 w96 h48 v360 n"TIFF"\n'
                                      'i w48 h32 f0 v50 y-14 p-1 r0 n"f0.pfm"\n'
                                      'i w48 h32 f0 v50 y15 p1 r3 n"f1.pfm"\n')
    argv = ["--pto", "two.pto", "--degree", "1", "--twine", "0", "--synopsis", "feather"]
    fcts = [ea.facet_spec(ea.RECTILINEAR, 48, 32, 50.0, yaw=-14, pitch=-1, roll=0),
            ea.facet_spec(ea.RECTILINEAR, 48, 32, 50.0, yaw=15, pitch=1, roll=3)]
    gs = [ea.Source.load(f, img, 1) for f, img in zip(fcts, imgs)]
    for extra, width in (([], 0.0), (["--feather", "6.5"], 6.5)):
        r = subprocess.run([EXE] + argv + extra + ["--output", "o.pfm", "-v"], capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
        assert r.returncode == 0, r.stderr
        assert "synopsis feather" in r.stdout and ("6.5" in r.stdout) == bool(extra)
        want = ea.render(ea.arguments(ea.SPHERICAL, 96, 48, 360.0, spline_degree=1, synopsis="feather", feather=width), gs, 3)
        raw = (tmp_path / "o.pfm").read_bytes()
        head = raw.split(b"\n", 3)
        assert head[0] == b"PF" and head[1].split() == [b"96", b"48"] and float(head[2]) < 0
        assert head[3] == np.ascontiguousarray(want[::-1], "<f4").tobytes(), f"--feather {width}: the file's pixels"
    # two facets of 50 x 34.5 degrees that share 21 degrees cover about 4 % of the sphere; and the seam is blended
    assert (want != 0).mean() > 0.03
    pano = ea.render(ea.arguments(ea.SPHERICAL, 96, 48, 360.0, spline_degree=1), gs, 3)
    assert ((want != 0) == (pano != 0)).all() and (jobs.bits(want) != jobs.bits(pano)).sum() > 30
