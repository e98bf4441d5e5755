"""Multi-band blending: properties of the numpy model (tests/multiband_model.py) on oracle inputs, and what the
library answers without a device - levels, fields, refusals. No GPU: what the device is held to in
tests/test_gpu_multiband.py is checked here for being what the definition promises.

TOL. The float32 model against the float64 restatement of the same formulas (the layers X and Q are the same
float32 values on both sides), largest absolute difference measured on the jobs of this file, pixels up to 1.0:
    two rectilinear facets, 3 and 4 channels, L = 3     2.18e-7 (both)
    random pictures 4 x 4 .. 130 x 70, 64 x 16 wrapped   2.5e-8, 3.3e-8, 9.7e-8, 9.7e-8, 1.64e-7, 2.13e-7, 1.67e-7
    the grey pair on 192 x 80 at bands 0, 1, 2           1.45e-7, 8.9e-8, 1.16e-7
    constant facets                                      0 (constant pictures: 6e-8 from the constant)
With the margin of 4 for rounding that depends on the image: TOL = 4 * 2.18e-7 = 8.8e-7, some 15 units in the last
place of 0.5 - a handful of roundings in each of the L + 1 <= 5 bands."""
import ctypes as C

import numpy as np
import pytest

import envutil_amd as ea
import euo
import jobs
import feather_model as fm
import multiband_model as mm

TOL = 8.8e-7
SIZES, pictures = mm.SIZES, mm.pictures


def target(w=96, h=40, hfov=120.0, **kw):
    return ea.arguments(ea.SPHERICAL, w, h, hfov, synopsis="multiband", **kw)


def pair(nch, degree=1, brightens=(1.0, 1.25), constant=None, size=(48, 32)):
    out = []
    for k in range(2):
        img = jobs.synth_image(size[0], size[1], nch, seed=40 + k)
        if constant is not None:
            img[:, :, :] = constant
        out.append(fm.Facet(euo.RECTILINEAR, size[0], size[1], 50.0, img, degree, yaw=-14.0 + 29.0 * k, pitch=2.0 * k - 1.0,
                            roll=3.0 * k, brighten=brightens[k]))
    return out


def both(args, fs, nch):
    a32 = mm.model_frame(args, fs, nch, details=True)
    a64 = mm.model_frame(args, fs, nch, dtype=np.float64)
    return a32[0], a64, a32[1]


def worst(a, b):
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())


@pytest.mark.parametrize("nch", [3, 4])
def test_float32_model_against_float64_on_facets(nch):
    f32, f64, count = both(target(spline_degree=1), pair(nch), nch)
    for n in (0, 1, 2):
        assert (count == n).sum() > 50
    assert np.isfinite(f32).all() and f32.dtype == np.float32 and f64.dtype == np.float64
    d = worst(f32, f64)
    print(f"nch {nch}: float32 against float64 {d:.3g}")
    assert d <= TOL
    assert (f32[count == 0] == 0).all() and (f32[count > 0] != 0).any()


@pytest.mark.parametrize("w,h,n,c", SIZES)
def test_float32_model_against_float64_on_pictures(w, h, n, c):
    colour, weight = pictures(w, h, n, c)
    bands, wrap = mm.setting(w, h)
    d = worst(mm.blend_layers(colour, weight, bands, wrap), mm.blend_layers(colour, weight, bands, wrap, np.float64))
    print(f"{w} x {h}: float32 against float64 {d:.3g}")
    assert d <= TOL


def test_identical_constant_facets_give_the_constant():
    """every facet holds 0.5 (degree 0, brighten 1): all bands below the top are zero, the top is the constant"""
    a = target(spline_degree=0)
    fs = pair(3, degree=0, brightens=(1.0, 1.0), constant=0.5)
    f32, f64, count = both(a, fs, 3)
    assert worst(f32, f64) <= TOL
    assert np.abs(f32[count > 0].astype(np.float64) - 0.5).max() <= TOL
    assert (f32[count == 0] == 0).all()
    colour = np.full((3, 17, 33, 2), 0.3, np.float32)
    _, weight = pictures(33, 17, 3, 2)
    out = mm.blend_layers(colour, weight)
    covered = (weight > 0).any(axis=0)
    assert np.abs(out[covered].astype(np.float64) - np.float32(0.3)).max() <= TOL


def test_rolling_wrapped_pictures_rolls_the_frame():
    """with wrap, a roll of all inputs by a multiple of 2^L columns is a roll of every level: bit for bit"""
    colour, weight = pictures(64, 16, 2, 3)
    assert mm.levels_of(64, 16, 3, True) == 2
    ref = mm.blend_layers(colour, weight, 3, True)
    for shift in (4, 8, 36):
        got = mm.blend_layers(np.roll(colour, shift, axis=2), np.roll(weight, shift, axis=2), 3, True)
        assert (jobs.bits(got) == jobs.bits(np.roll(ref, shift, axis=1))).all(), f"shift {shift}"
    # a roll that is no multiple of 4 moves the samples of level 2: other bits; and without wrap the edges differ
    got = mm.blend_layers(np.roll(colour, 2, axis=2), np.roll(weight, 2, axis=2), 3, True)
    assert (jobs.bits(got) != jobs.bits(np.roll(ref, 2, axis=1))).any()
    assert (jobs.bits(mm.blend_layers(colour, weight, 3, False)) != jobs.bits(ref)).any()


def dilate(mask, r):
    """mask grown by r pixels each way (a square)"""
    h, w = mask.shape
    p = np.pad(mask, r)
    out = np.zeros_like(mask)
    for dy in range(2 * r + 1):
        rows = p[dy:dy + h]
        for dx in range(2 * r + 1):
            out |= rows[:, dx:dx + w]
    return out


def test_grey_facets_seam_is_smoother_than_feathers():
    """Two grey facets, brighten 1 and 1.25 (degree 0: pixels 0.5 and 0.625), against feather at --feather 8: along a
    row across the overlap the largest step between adjacent pixels is smaller under multiband. And where one facet
    alone covers AND the other facet's weight pyramid does not reach - it spreads 4 * 2^L pixels beyond the facet: 2
    level-l pixels per reduce, 1 per expand - the frame is that facet's value within TOL: a grey facet's bands below
    the top are zero, so its pixel comes back through the pyramid but for rounding."""
    size = (96, 64)
    fs = pair(3, degree=0, constant=0.5, size=size)
    for f in fs:
        f.o.s.pitch = f.o.s.roll = f.white.s.pitch = f.white.s.roll = 0.0
    a = target(192, 80, spline_degree=0, feather=8.0)
    arrays = [fm.facet_arrays(a, f, 3) for f in fs]
    feather, _, count = fm.feather(arrays, 3, 8.0, details=True)
    assert mm.levels_of(192, 80, 0, False) == 4
    multi = mm.multiband(arrays, 3, 8.0, 0, False)
    rows = 0
    for y in range(12, 68):
        two = np.flatnonzero(count[y] == 2)
        if len(two) < 16:
            continue
        x0, x1 = two[0] - 8, two[-1] + 9
        assert (count[y, x0:x1] >= 1).all()
        step_f = np.abs(np.diff(feather[y, x0:x1, 0].astype(np.float64))).max()
        step_m = np.abs(np.diff(multi[y, x0:x1, 0].astype(np.float64))).max()
        assert step_m < step_f, f"row {y}: multiband steps {step_m:.4g}, feather {step_f:.4g}"
        rows += 1
    assert rows >= 30
    # one facet alone, out of the other's reach
    for bands in (1, 2):
        frame = mm.multiband(arrays, 3, 8.0, bands, False)
        assert worst(frame, mm.multiband(arrays, 3, 8.0, bands, False, np.float64)) <= TOL
        reach = 4 << bands
        for k, value in ((0, 0.5), (1, 0.625)):
            alone = arrays[k]["hit"] & ~dilate(np.asarray(arrays[1 - k]["hit"], bool), reach)
            assert alone.sum() > 300, f"facet {k}, bands {bands}: {alone.sum()} pixels"
            assert np.abs(frame[alone].astype(np.float64) - value).max() <= TOL
    # ... while next to the seam the low band reaches into the part one facet covers: that is what the bands are for
    frame = mm.multiband(arrays, 3, 8.0, 0, False)
    only0 = arrays[0]["hit"] & ~arrays[1]["hit"]
    assert np.abs(frame[only0].astype(np.float64) - 0.5).max() > 100 * TOL


def test_levels_for_a_table_of_sizes():
    table = [((4, 4, 0, False), 0), ((5, 3, 0, False), 0), ((8, 8, 0, False), 1), ((9, 7, 0, False), 1), ((64, 6, 3, True), 0),
             ((33, 17, 0, False), 2), ((130, 70, 0, False), 4), ((130, 70, 2, False), 2), ((64, 16, 3, True), 2),
             ((64, 16, 1, True), 1), ((36, 32, 0, False), 3), ((36, 32, 0, True), 2), ((37, 32, 0, True), 0),
             ((4096, 2048, 0, False), 8), ((4096, 2048, 20, False), 9), ((4096, 2048, 0, True), 8), ((1, 1, 0, False), 0)]
    for (w, h, bands, wrap), want in table:
        assert mm.levels_of(w, h, bands, wrap) == want, (w, h, bands, wrap)
        assert ea.multiband_levels(w, h, bands, wrap) == want, (w, h, bands, wrap)
    with pytest.raises(ea.EuError, match="bands"):
        ea.multiband_levels(8, 8, -1)


def test_arguments_and_target_fields():
    a = target(bands=3, feather=6.5)
    t = a.target(3)
    assert (t.synopsis, t.bands, t.feather) == (ea.api.SYN_MULTIBAND, 3, 6.5) and ea.api.SYN_MULTIBAND == 4
    # `bands` fills the 4-byte gap between `height` and `x0`: no other field moves, the structure keeps its size
    assert ea.Target.bands.offset == ea.Target.height.offset + 4 == ea.Target.x0.offset - 4
    assert C.sizeof(ea.Target) == ea.Target.feather.offset + 8 == 152
    assert target().target(3).bands == 0
    for bad in (-1, 1.5):
        with pytest.raises(ValueError, match="bands"):
            target(bands=bad)
    with pytest.raises(ValueError, match="multiband"):
        ea.arguments(ea.SPHERICAL, 96, 40, 120.0, synopsis="laplace")
    # the scratch: the formula of eu_hip.h, a host function
    a = target(130, 70)
    S = [130 * 70, 65 * 35, 33 * 18, 17 * 9, 9 * 5]
    T = sum(S)
    for nch, ncol in ((3, 3), (4, 3), (1, 1), (2, 1)):
        want = 4 * (S[0] * (2 * (ncol + 1) + 3) + ncol * (T - S[0]) + 2 * T + (ncol + 1) * T)
        assert ea.multiband_scratch_bytes(a, 2, nch) == want
    assert ea.multiband_scratch_bytes(a, 1, 3) == 0


class NoSource:
    handle = None


def refused(match, a, call=None, **kw):
    with pytest.raises(ea.EuError, match=match) as e:
        (call or ea.render)(a, [NoSource(), NoSource()], 3, **kw)
    assert "error -2" in str(e.value)


def test_refusals_need_no_device():
    """each with EU_ERR_ARGUMENT and a message of its own, before a device is looked for (and before the sources are:
    these handles are null)"""
    refused("multiband: no twining", target(twine=2))
    refused("multiband: the row range", target(), row_begin=0, row_end=20)
    refused("multiband: the row range", target(), row_begin=4)
    refused("multiband: no row bands", target(), band=(4, 2, 0))
    refused("multiband: no crop window", target(crop=(0, 90, 0, 40)))
    refused("multiband: EU_OUT_SRGBA8", target(tethered=True))
    t = target()
    t.bands = -2
    refused("bands must be 0", t)
    refused("multiband: no twining", target(twine=2), ea.render_samples)
    refused("multiband: no crop window", target(crop=(0, 90, 0, 40)), ea.render_rgbe)
    refused("multiband: no row bands", target(), ea.render_rgbe, band=(4, 2, 0))
    # blend_layers' own
    colour, weight = pictures(9, 7, 2, 3)
    with pytest.raises(ea.EuError, match="blend_layers: bands"):
        ea.blend_layers(colour, weight, bands=-1)
    with pytest.raises(ea.EuError, match="colour is"):
        ea.blend_layers(colour, weight[:, :, :5])
    with pytest.raises(ea.EuError, match="float32"):
        ea.blend_layers(colour.astype(np.float64), weight)

