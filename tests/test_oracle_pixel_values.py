"""The CPU oracle against the reference's own zimt headers compiled in place (oracle/_ref/libref_zimt.so) on the
pixel VALUES real images hold (tests/pixel_values.py): impulses on black, HDR range, signed data with both zeros,
denormals, +-1e37, and - where nothing prefilters - inf, NaN and +-3e38. test_oracle_vs_ref.py sweeps geometry with
uniform [0, 1) data; this file keeps the geometry small and sweeps what is in the pixels. Finite classes: float32 bit
patterns, 0 ULP. The non-finite class: where the NaNs are, and every other float's bits (refz.same(any_nan=True));
zimt and the oracle do not always give a NaN the same sign and payload, and no caller can rely on either.
Live where the library is built; elsewhere against tests/golden/pixel_value_digests.json."""
import ctypes as C

import numpy as np
import pytest

import euo
import pixel_values as pv
import refz

pytestmark = pytest.mark.ref

# two shapes large enough for an impulse's tail to turn denormal (3 and 4 channels), an odd one of one channel, and
# two that are shorter than the prefilter's horizon on one axis, one wider than high and one higher than wide
SHAPES = [(200, 100, 3), (97, 61, 1), (160, 80, 4), (33, 7, 2), (18, 130, 3)]
# what the set-up uses: PERIODIC x REFLECT (full-circle lat/lon, cylinder), REFLECT x REFLECT (every other mount),
# NATURAL x NATURAL (a cubemap's IR sections) - and MIRROR x MIRROR
BCS = [(1, 2), (2, 2), (3, 3), (0, 0)]


def coordinates(w, h, n, seed):
    """n spline coordinates, three quarters inside the core, the others up to 2.5 sizes outside"""
    u = pv.unit(pv.u32(2 * n, seed)).reshape(n, 2)
    crd = np.empty((n, 2), np.float64)
    crd[:, 0] = u[:, 0] * (w + 1) - 1
    crd[:, 1] = u[:, 1] * (h + 1) - 1
    far = np.arange(n) % 4 == 3
    crd[far, 0] = u[far, 0] * 6 * w - 2.5 * w
    crd[far, 1] = u[far, 1] * 6 * h - 2.5 * h
    return crd.astype(np.float32)


def both(core, deg, pdeg, b0, b1, spherical=False):
    r = refz.RefSpline(core, deg, b0, b1) if refz.available() else None
    o = euo.BSpline(core, deg, b0, b1)
    if spherical:
        if r:
            r.spherical(pdeg)
        o.spherical_prefilter(pdeg)
    else:
        if r:
            r.prefilter(pdeg)
        o.prefilter(pdeg)
    return o, r


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("cls", pv.FINITE)
def test_finite_classes_prefilter_container_eval(cls, shape):
    """degrees 0 to 7, prefiltered at the spline's degree - `big` at 3 where the degree is higher: the reference's
    own prefilter overflows on +-1e37 from degree 4 on (pixel_values.big), and that cell is left out"""
    w, h, n = shape
    core = pv.make(cls, h, w, n, seed=w + h)
    crd = coordinates(w, h, 192, w * h)
    for deg in range(8):
        for b0, b1 in BCS:
            o, r = both(core, deg, min(deg, pv.BIG_PREFILTER_MAX) if cls == "big" else deg, b0, b1)
            assert np.isfinite(o.container).all(), (cls, deg, b0, b1)
            key = f"pixval_{cls}_{w}x{h}x{n}_{deg}_{b0}{b1}"
            assert refz.same(key + "_container", o.container, lambda: r.container()), (cls, deg, b0, b1)
            assert refz.same(key + "_eval", o.eval(crd), lambda: r.eval(crd)), (cls, deg, b0, b1)
            if cls == "big" and deg > pv.BIG_PREFILTER_MAX:
                # ... and the largest values the whole prefilter of this degree leaves finite
                top = pv.BIG_TOP_5 if deg <= 5 else pv.BIG_TOP_7
                o, r = both(pv.big(h, w, n, seed=w + h, top=top), deg, deg, b0, b1)
                assert np.isfinite(o.container).all() and np.abs(o.container).max() > top, (deg, b0, b1)
                assert refz.same(key + f"_{top:g}_container", o.container, lambda: r.container()), (deg, b0, b1)
                assert refz.same(key + f"_{top:g}_eval", o.eval(crd), lambda: r.eval(crd)), (deg, b0, b1)
            # the inputs did what they are for: the pole of degree 2 (-0.17) is below 1e-38 fifty texels from an
            # impulse, so the two large shapes hold a ring of denormals around each (0.085 of the container)
            if cls == "impulse" and deg == 2 and w >= 160:
                assert pv.denormal_share(o.container) > 0.05
            if cls == "denormal" and deg <= 5:
                assert pv.denormal_share(o.container) > 0.9


@pytest.mark.parametrize("shape", [(200, 100, 3), (160, 80, 4), (62, 31, 1)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("cls", pv.FINITE)
def test_finite_classes_full_sphere_scheme(cls, shape):
    w, h, n = shape
    core = pv.make(cls, h, w, n, seed=3 * w)
    crd = coordinates(w, h, 192, w + 7)
    for deg in (2, 3, 5):
        o, r = both(core, deg, min(deg, pv.BIG_PREFILTER_MAX) if cls == "big" else deg, euo.PERIODIC, euo.REFLECT,
                    spherical=True)
        key = f"pixval_{cls}_sphere_{w}x{h}x{n}_{deg}"
        assert refz.same(key + "_container", o.container, lambda: r.container()), (cls, deg)
        assert refz.same(key + "_eval", o.eval(crd), lambda: r.eval(crd)), (cls, deg)


@pytest.mark.parametrize("shape", SHAPES[:4], ids=lambda s: "x".join(map(str, s)))
def test_nonfinite_class_braced_and_evaluated_without_a_prefilter(shape):
    """one inf or 3e38 turns a whole container NaN under any prefilter of degree 2 or more, so non-finite data means
    something only where nothing prefilters: prefilter degree 0 (the brace alone), evaluated at degrees 0 to 7"""
    w, h, n = shape
    core = pv.nonfinite(h, w, n, seed=w + h, one_in=200 if w * h > 2000 else 40)
    crd = coordinates(w, h, 192, w * h + 1)
    for deg in range(8):
        for b0, b1 in BCS:
            o, r = both(core, deg, 0, b0, b1)
            key = f"pixval_nonfinite_{w}x{h}x{n}_{deg}_{b0}{b1}"
            assert refz.same(key + "_container", o.container, lambda: r.container(), any_nan=True), (deg, b0, b1)
            ev = o.eval(crd)
            assert refz.same(key + "_eval", ev, lambda: r.eval(crd), any_nan=True), (deg, b0, b1)
            if deg >= 3 and w * h > 2000:
                assert np.isnan(ev).any() and np.isfinite(ev).any()
    # and what the issue of spread says: one non-finite texel, prefiltered, leaves no finite coefficient
    for deg in (2, 3):
        o, r = both(core, deg, deg, 2, 2)
        assert not np.isfinite(o.container).any()
        assert refz.same(f"pixval_nonfinite_{w}x{h}x{n}_{deg}_spread", o.container, lambda: r.container(), any_nan=True)


@pytest.mark.parametrize("size", [(64, 48), (97, 61), (16, 5), (5, 33)], ids=lambda s: "x".join(map(str, s)))
def test_binomial_of_the_alpha_plane(size):
    """zimt::convolve with 1 4 6 4 1 / 16 (environment.h:833-843) on planes of exact zeros of both signs, denormals,
    the floats around 0.000001f, values above 1 and small negatives"""
    w, h = size
    for seed in (1, 2):
        plane = pv.alpha_plane(h, w, seed)
        assert refz.same(f"pixval_binomial_{w}x{h}_{seed}", euo.binomial_plane(plane), lambda: refz.binomial_alpha(plane))
    d = pv.denormal(h, w, 1, 9)[:, :, 0]
    assert refz.same(f"pixval_binomial_{w}x{h}_denormal", euo.binomial_plane(d), lambda: refz.binomial_alpha(d))


@pytest.mark.parametrize("cls", pv.FINITE)
def test_screen_lut_on_values_around_the_unit_interval(cls):
    """lut_based_tf (envutil_payload.cc:251-287): the clamp at 0 and at 255 and the linear evaluation, on every
    finite class scaled into and around [0, 1], and on the class as it is (far outside). NaN is left out: the
    reference does not define it (the clamp's comparisons are all false, the index is then whatever the conversion
    of NaN to int gives)."""
    L = euo.lib()
    lut = np.zeros(257, np.float32)
    L.euo_screen_lut(lut.ctypes.data_as(C.c_void_p))
    L.euo_lut_eval.restype = C.c_float
    L.euo_lut_eval.argtypes = [C.c_void_p, C.c_float]
    edges = np.float32([0.0, -0.0, 1.0, np.nextafter(np.float32(1), np.float32(0)), 1.0 / 255.0, 254.5 / 255.0,
                        -1e-45, 1e-45, 3e38, -3e38, np.inf, -np.inf, 0.5, 2.0, -1.0, 1e-6])
    vin = np.ascontiguousarray(np.concatenate([edges, pv.scaled_unit(cls, 40, 50, 1, seed=2).reshape(-1),
                                               pv.make(cls, 20, 48, 1, seed=3).reshape(-1)]), np.float32)
    assert len(vin) % 16 == 0
    if cls != "impulse":
        s = vin[16:2016]
        assert (s < 0).any() and (s > 1).any() and ((s > 0) & (s < 1)).any() and (s == 1).any()
    got = np.array([L.euo_lut_eval(lut.ctypes.data, float(v)) for v in vin], np.float32)
    assert refz.same(f"pixval_lut_{cls}", got, lambda: refz.lut_eval(lut[:256], vin))
