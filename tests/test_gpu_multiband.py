"""Multi-band blending on the device (--synopsis multiband, EU_SYN_MULTIBAND: eu_synopsis_layers in eu_multi_dev.h
and the pyramid kernels of eu_multiband.hip; eu_hip_blend_layers) against the numpy model of
tests/multiband_model.py, bit for bit, whole frames. Small jobs: feather's shapes - targets of 96 x 40 and 97 x 41,
facets around 48 x 32 - and pictures from 4 x 4 to 130 x 70. Pixels are finite throughout."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import envutil_amd as ea
import euo
import jobs
import feather_model as fm
import multiband_model as mm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "envutil_amd", "bin", "envutil_hip")


def assert_bits(got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    d = jobs.bits(got) != jobs.bits(ref)
    assert not d.any(), f"{what}: {int(d.sum())} of {d.size} values differ, first at {np.argwhere(d)[0]}: " \
                        f"{got[tuple(np.argwhere(d)[0])]!r} model {ref[tuple(np.argwhere(d)[0])]!r}"


def target(w=96, h=40, hfov=120.0, **kw):
    return ea.arguments(ea.SPHERICAL, w, h, hfov, synopsis="multiband", **kw)


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
    ref, count = mm.model_frame(a, fs, nch, details=True)
    assert np.isfinite(ref).all()
    assert (count >= 2).sum() >= overlap, f"{what}: {(count >= 2).sum()} pixels see more than one facet"
    got = ea.render(a, gs, nch)
    assert_bits(got, ref, what)
    return got, gs


# ---- eu_hip_blend_layers: the pyramid alone -------------------------------------------------------------------------

@pytest.fixture(scope="module")
def blended():
    """the model's frame of every size, once"""
    out = {}
    for w, h, n, c in mm.SIZES:
        colour, weight = mm.pictures(w, h, n, c)
        bands, wrap = mm.setting(w, h)
        out[(w, h)] = (colour, weight, bands, wrap, mm.blend_layers(colour, weight, bands, wrap))
    return out


@pytest.mark.parametrize("w,h,n,c", mm.SIZES)
def test_blend_layers_host_arrays(blended, w, h, n, c):
    colour, weight, bands, wrap, ref = blended[(w, h)]
    assert np.isfinite(ref).all()
    assert_bits(ea.blend_layers(colour, weight, bands=bands, wrap=wrap), ref, f"{w} x {h} host")
    if (w, h) == (33, 17):
        assert (weight[n - 1] == 0).all() and (weight[:, :, w // 3] == 0).all() and (weight == 0).mean() > 0.2
        # padded rows and pictures on the host, and an `out` of the caller's with padded rows
        big_c, big_w = np.zeros((n, h + 2, w + 3, c), np.float32), np.zeros((n, h + 1, w + 5), np.float32)
        big_c[:, :h, :w], big_w[:, :h, :w] = colour, weight
        out = np.full((h, w + 4, c), 7.0, np.float32)
        ea.blend_layers(big_c[:, :h, :w], big_w[:, :h, :w], out=out[:, :w])
        assert_bits(out[:, :w], ref, "padded host arrays")
        assert (out[:, w:] == 7.0).all()


@pytest.mark.parametrize("w,h,n,c", mm.SIZES)
def test_blend_layers_device_tensors_into_a_guarded_buffer(blended, w, h, n, c):
    """torch tensors with padded strides in, a guarded device buffer with padded rows out: nothing outside the rows
    is touched and nothing inside is left unwritten"""
    import torch
    import devout
    colour, weight, bands, wrap, ref = blended[(w, h)]
    big_c = torch.full((n, h + 1, w + 3, c), 9.0, dtype=torch.float32, device="cuda")
    big_w = torch.full((n, h + 2, w + 1), 9.0, dtype=torch.float32, device="cuda")
    big_c[:, :h, :w] = torch.from_numpy(colour).cuda()
    big_w[:, :h, :w] = torch.from_numpy(weight).cuda()
    tc, tw = big_c[:, :h, :w], big_w[:, :h, :w]
    torch.cuda.synchronize()
    buf = devout.Guarded(h, w * c, pad=5, lead=3)
    rc = ea.lib().eu_hip_blend_layers(C.c_void_p(tc.data_ptr()), tc.stride(1) * 4, tc.stride(0) * 4, C.c_void_p(tw.data_ptr()),
                                      tw.stride(1) * 4, tw.stride(0) * 4, 1, n, w, h, c, bands, int(wrap),
                                      C.c_void_p(buf.ptr()), buf.stride_bytes, 1, None)
    assert rc == 0, ea.lib().eu_hip_last_error().decode()
    ea.sync()
    devout.check(f"blend_layers {w} x {h} into a padded device buffer", buf.frame().view(np.float32).reshape(h, w, c), buf.outside(), ref)
    # and through the Python call: a new device tensor
    got = ea.blend_layers(tc, tw, bands=bands, wrap=wrap)
    ea.sync()
    assert_bits(got.cpu().numpy(), ref, f"{w} x {h} device tensors")


def test_blend_layers_levels_and_scratch():
    """the settings reach the kernels: other bands, other bits; wrap, other bits; the scratch comes and goes"""
    colour, weight = mm.pictures(130, 70, 2, 3)
    full = ea.blend_layers(colour, weight)
    for bands in (1, 2):
        got = ea.blend_layers(colour, weight, bands=bands)
        assert_bits(got, mm.blend_layers(colour, weight, bands), f"bands {bands}")
        assert (jobs.bits(got) != jobs.bits(full)).any()
    colour, weight = mm.pictures(64, 16, 2, 3)
    assert (jobs.bits(ea.blend_layers(colour, weight, bands=3, wrap=True)) != jobs.bits(ea.blend_layers(colour, weight, bands=3))).any()
    ea.multiband_scratch_release()
    assert_bits(ea.blend_layers(colour, weight, bands=3, wrap=True), mm.blend_layers(colour, weight, 3, True), "after a release")
    ea.multiband_scratch_release()
    ea.multiband_scratch_release()


def test_scratch_that_cannot_be_allocated_is_the_memory_error():
    """2^18 rows of 2^14 pixels, 4 layers of 4 channels: more than 600 GB of scratch. The call returns the library's
    memory error with a message before anything is read or launched: the pictures are 4 floats, never touched"""
    tiny = np.zeros(4, np.float32)
    ptr = tiny.ctypes.data_as(C.c_void_p)
    w, h = 1 << 14, 1 << 18
    rc = ea.lib().eu_hip_blend_layers(ptr, w * 16, w * 16 * h, ptr, w * 4, w * 4 * h, 0, 4, w, h, 4, 0, 0, ptr, w * 16, 0, None)
    assert rc == -4, (rc, ea.lib().eu_hip_last_error().decode())
    assert "multiband: cannot allocate" in ea.lib().eu_hip_last_error().decode()
    colour, weight = mm.pictures(9, 7, 3, 3)
    assert_bits(ea.blend_layers(colour, weight), mm.blend_layers(colour, weight), "the call after the refusal")


# ---- render: stage A and the pyramid ------------------------------------------------------------------------------

@pytest.mark.parametrize("degree,tw,th,bands", [(0, 96, 40, 0), (1, 97, 41, 0), (3, 96, 40, 2)])
def test_two_rectilinear_facets(degree, tw, th, bands):
    a = target(tw, th, spline_degree=degree, bands=bands, feather=6.0 if degree == 1 else 0.0)
    got, gs = held(f"two facets degree {degree} {tw} x {th} bands {bands}", a, pair(3, degree), 3)
    # the same facets feathered give something else: the synopsis reaches the kernels
    fth = ea.render(ea.arguments(ea.SPHERICAL, tw, th, 120.0, spline_degree=degree, synopsis="feather", feather=a.feather), gs, 3)
    assert (jobs.bits(fth) != jobs.bits(got)).any() and ((fth != 0) == (got != 0)).all()


@pytest.mark.parametrize("nch", [2, 4])
def test_alpha_planes_around_the_gate(nch):
    """alpha 0, values on both sides of the gate 1e-6, and 1, in stripes that cross the overlap; the colour is associated"""
    fs = []
    for k in range(2):
        img = jobs.synth_image(48, 32, nch, seed=70 + k)
        yy, xx = np.mgrid[0:32, 0:48]
        a = np.choose(((xx + 5 * k) // 4 + yy // 6) % 5, [0.0, 5e-7, 2e-6, 1.0, 0.5]).astype(np.float32)
        img[:, :, nch - 1] = a
        img[:, :, :nch - 1] *= a[:, :, None]
        fs.append(fm.Facet(euo.RECTILINEAR, 48, 32, 50.0, img, 1, yaw=-12.0 + 25.0 * k, pitch=1.0 - 2.0 * k,
                           brighten=1.0 + 0.5 * k))
    got, _ = held(f"alpha nch {nch}", target(97, 41, spline_degree=1, feather=9.0), fs, nch)
    al = got[:, :, nch - 1]
    assert (al == 0).any() and (al == 1).any() and ((al > 0) & (al < 1e-6)).any() and ((al > 1e-6) & (al < 1e-5)).any()


def test_windowed_fisheye_and_full_sphere_on_a_target_that_wraps():
    lens = dict(a=0.01, b=-0.03, c=0.02, h=0.02, v=-0.01, g=0.01, t=-0.02)
    fs = [fm.Facet(euo.FISHEYE, 48, 48, 120.0, jobs.synth_image(32, 32, 3, seed=90), 1, yaw=-170.0, pitch=3.0, roll=5.0, lens=lens,
                   window=(32, 32, 8, 8)),
          fm.Facet(euo.SPHERICAL, 64, 32, 360.0, jobs.synth_image(64, 32, 3, seed=92), 1, yaw=30.0, brighten=0.8)]
    a = target(64, 32, hfov=360.0, spline_degree=1)
    assert mm.wraps(a) and mm.levels_of(64, 32, 0, True) == 3 and fs[0].win == (32, 32)
    ref, count = mm.model_frame(a, fs, 3, details=True)
    # the fisheye lies across the frame's left and right edge
    assert (count[:, 0] == 2).any() and (count[:, 63] == 2).any() and (count >= 1).all()
    got, gs = held("windowed fisheye + sphere, 360 degrees", a, fs, 3)
    # a target that does not wrap takes the clamped pyramid: 359 degrees
    b = target(64, 32, hfov=359.0, spline_degree=1)
    assert not mm.wraps(b)
    assert_bits(ea.render(b, gs, 3), mm.model_frame(b, fs, 3), "359 degrees")


def test_cubemap_source():
    fs = [fm.Facet(euo.CUBEMAP, 16, 96, 90.0, jobs.synth_cubefaces(16, 3), 1, yaw=10.0),
          fm.Facet(euo.RECTILINEAR, 48, 32, 50.0, jobs.synth_image(48, 32, 3, seed=95), 1, yaw=5.0, brighten=1.3)]
    held("cubemap + rectilinear", target(spline_degree=1, feather=5.0), fs, 3)


def test_one_and_four_channel_facets_on_three_channels():
    fs = [fm.Facet(euo.RECTILINEAR, 48, 32, 50.0, jobs.synth_image(48, 32, 1, seed=80), 1, yaw=-13.0, brighten=1.2),
          fm.Facet(euo.RECTILINEAR, 48, 32, 50.0, jobs.synth_image(48, 32, 4, seed=81), 1, yaw=14.0, pitch=2.0, roll=-2.0)]
    held("1 + 4 channels -> 3", target(97, 41, spline_degree=1), fs, 3)


def test_rectilinear_target_through_the_rays():
    """a target whose stepper normalises: the facets' arrays at the multi-facet job's own rays"""
    fs = pair(3, 1)
    a = ea.arguments(ea.RECTILINEAR, 96, 40, 80.0, spline_degree=1, synopsis="multiband", feather=10.0)
    gs, gws = [f.gpu() for f in fs], [f.gpu_white() for f in fs]
    ref = mm.model_frame_at_rays(a, fs, gs, gws, 3)
    assert np.isfinite(ref).all() and (ref != 0).mean() > 0.2
    assert_bits(ea.render(a, gs, 3), ref, "rectilinear target")


@pytest.fixture(scope="module")
def job():
    a = target(97, 41, spline_degree=1)
    fs = pair(3, 1)
    gs = [f.gpu() for f in fs]
    whole = ea.render(a, gs, 3)
    assert_bits(whole, mm.model_frame(a, fs, 3), "the shared job")
    return a, fs, gs, whole


def test_render_samples_rgbe_and_a_guarded_device_buffer(job):
    import devout
    a, fs, gs, whole = job
    for bits in (8, 16):
        got = ea.render_samples(a, gs, 3, bits=bits)
        assert (got == ea.encode_samples(whole, bits=bits)).all(), f"{bits}-bit samples"
    assert (ea.render_rgbe(a, gs, 3) == ea.encode_rgbe(whole)).all()
    frame, outside, _ = devout.render_dev(a, gs, 3, pad=5, lead=3)
    devout.check("multiband into a padded device buffer", frame, outside, whole)
    assert ea.multiband_scratch_bytes(a, 2, 3) > 4 * 97 * 41 * 11


def test_stage_time_diagnostic(job):
    """eu_hip_multiband_stage_times (tools/multiband_time.py): the job it times is the job - the frame is render()'s -,
    every stage has a time, and the nominal bytes are the planes' sizes. 97 x 41 -> 49 x 21 -> 25 x 11 -> 13 x 6: L = 3"""
    import torch
    a, fs, gs, whole = job
    out = torch.zeros((41, 97, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    L = ea.lib()
    L.eu_hip_multiband_stage_times.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
    handles = (C.c_void_p * 2)(*[s.handle for s in gs])
    ms, nbytes = (C.c_double * 5)(), (C.c_double * 5)()
    t = a.target(3)
    assert L.eu_hip_multiband_stage_times(C.byref(t), handles, 2, C.c_void_p(out.data_ptr()), 97 * 3 * 4, 2, ms, nbytes) == 0, L.eu_hip_last_error().decode()
    ea.sync()
    assert_bits(out.cpu().numpy(), whole, "the timed job's frame")
    assert all(0.0 < v < 1000.0 for v in ms), list(ms)
    S = [97 * 41, 49 * 21, 25 * 11, 13 * 6]
    want = [4 * (2 * 4 + 3) * S[0], 2 * 16 * S[0], 2 * 4 * 5 * sum(S[l] + S[l + 1] for l in range(3)),
            2 * 4 * (sum(13 * S[l] for l in range(4)) + sum(4 * S[l + 1] for l in range(3))),
            4 * (sum(9 * S[l] + (3 * S[l + 1] if l < 3 else 0) for l in (1, 2, 3)) + 9 * S[0] + 3 * S[1])]
    assert [int(round(v)) for v in nbytes] == want, (list(nbytes), want)
    t.synopsis = ea.api.SYN_FEATHER
    assert L.eu_hip_multiband_stage_times(C.byref(t), handles, 2, C.c_void_p(out.data_ptr()), 97 * 3 * 4, 2, ms, nbytes) == -2


def test_single_facet_jobs_ignore_the_synopsis(job):
    a, fs, gs, whole = job
    plain = ea.arguments(ea.SPHERICAL, 97, 41, 120.0, spline_degree=1)
    assert_bits(ea.render(a, gs[0], 3), ea.render(plain, gs[0], 3), "one facet")
    assert_bits(ea.render(a, gs[0], 3, row_begin=3, row_end=20), ea.render(plain, gs[0], 3, row_begin=3, row_end=20), "one facet, rows")


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
    # no --twine: the default is automatic twining, which a multiband job of several facets does not get
    argv = ["--pto", "two.pto", "--degree", "1", "--synopsis", "multiband"]
    fs = [fm.Facet(euo.RECTILINEAR, 48, 32, 50.0, imgs[0], 1, yaw=-14, pitch=-1, roll=0),
          fm.Facet(euo.RECTILINEAR, 48, 32, 50.0, imgs[1], 1, yaw=15, pitch=1, roll=3)]
    for extra, bands, width, levels in (([], 0, 0.0, 3), (["--bands", "2", "--feather", "6.5", "--twine", "0"], 2, 6.5, 2)):
        r = subprocess.run([EXE] + argv + extra + ["--output", "o.pfm", "-v"], capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
        assert r.returncode == 0, r.stderr
        assert f"synopsis multiband, {levels} levels above level 0, columns wrap" in r.stdout and ("6.5" in r.stdout) == bool(extra)
        a = ea.arguments(ea.SPHERICAL, 96, 48, 360.0, spline_degree=1, synopsis="multiband", bands=bands, feather=width)
        want = mm.model_frame(a, fs, 3)
        raw = (tmp_path / "o.pfm").read_bytes()
        head = raw.split(b"\n", 3)
        assert head[0] == b"PF" and head[1].split() == [b"96", b"48"] and float(head[2]) < 0
        assert head[3] == np.ascontiguousarray(want[::-1], "<f4").tobytes(), f"--bands {bands}: the file's pixels"
    assert (want != 0).mean() > 0.03
    for bad, word in ((["--bands", "3", "--synopsis", "feather"], "--bands goes with --synopsis multiband"),
                      (["--synopsis", "multiband", "--bands", "-1"], "--bands -1"),
                      (["--synopsis", "multiband", "--twine", "3"], "--synopsis multiband blends whole frames")):
        r = subprocess.run([EXE, "--pto", "two.pto", "--output", "o.pfm"] + bad, capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
        assert r.returncode != 0 and word in r.stderr, r.stderr


def test_refusals(job):
    """every one with EU_ERR_ARGUMENT and a message of its own"""
    a, fs, gs, whole = job

    def refused(match, call, *args, **kw):
        with pytest.raises(ea.EuError, match=match) as e:
            call(*args, **kw)
        assert "error -2" in str(e.value)
    refused("multiband: no twining", ea.render, target(97, 41, spline_degree=1, twine=2), gs, 3)
    refused("multiband: the row range", ea.render, a, gs, 3, row_begin=5, row_end=23)
    refused("multiband: no row bands", ea.render, a, gs, 3, band=(4, 2, 0))
    refused("multiband: no crop window", ea.render, target(97, 41, spline_degree=1, crop=(0, 90, 6, 33)), gs, 3)
    refused("multiband: EU_OUT_SRGBA8", ea.render, target(97, 41, spline_degree=1, tethered=True), gs, 3)
    refused("multiband: no twining", ea.render_samples, target(97, 41, spline_degree=1, twine=2), gs, 3)
    refused("multiband: the row range", ea.render_rgbe, a, gs, 3, row_begin=5, row_end=23)
    refused("render_views_multi: no multiband synopsis", ea.render_views, a, [(0.0, 0.0, 0.0)], gs, nchannels=3)
    t = target(97, 41, spline_degree=1)
    t.bands = -1
    refused("bands must be 0", ea.render, t, gs, 3)
    masked = [fm.Facet(f.prj, f.width, f.height, f.hfov, jobs.synth_image(48, 32, 3, seed=40 + k), 1, **dict(f.kw, masked=k)).gpu()
              for k, f in enumerate(fs)]
    refused("multiband: --mask_for", ea.render, a, masked, 3)
    # the job still renders after all that
    assert_bits(ea.render(a, gs, 3), whole, "after the refusals")


def test_render_devices_with_more_than_one_slot_is_refused(job):
    a, fs, gs, whole = job
    ea.init_devices([0, 0, 0])
    assert ea.device_slots() == 3
    with pytest.raises(ea.EuError, match="render_devices: no multiband synopsis on more than one device"):
        ea.render_devices(a, gs, 3)
    assert_bits(ea.render(a, gs, 3), whole, "render on slot 0")
