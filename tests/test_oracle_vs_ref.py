"""CPU oracle vs the reference's own zimt headers compiled in place
(oracle/_ref/libref_zimt.so): a wider sweep than the committed fixtures. Live where
that library is built; elsewhere against the digests of its results recorded in
tests/golden/ref_digests.json (refz.same, tests/golden/make_ref_digests.py)."""
import numpy as np
import pytest

import euo
import refz

pytestmark = pytest.mark.ref


def test_lanes_and_segment():
    # the oracle's arithmetic model (oracle/eu_oracle.h: EUO_LANES, EUO_SEGMENT)
    assert refz.same("lanes_segment", [16, 512], lambda: [refz.lib().ref_lanes(), refz.lib().ref_segment()])


@pytest.mark.parametrize("shape", [(24, 12, 3), (40, 17, 4), (7, 5, 1), (64, 32, 2)])
def test_prefilter_brace_eval_sweep(shape):
    w, h, n = shape
    rng = np.random.default_rng(w * 1000 + h)
    core = rng.random((h, w, n), dtype=np.float32)
    for deg in range(0, 10):
        for pdeg in sorted({deg, 0, 3}):
            for b0, b1 in [(1, 2), (2, 2), (0, 0), (3, 3), (1, 1), (2, 3)]:
                r = refz.RefSpline(core, deg, b0, b1) if refz.available() else None
                o = euo.BSpline(core, deg, b0, b1)
                if r:
                    r.prefilter(pdeg)
                o.prefilter(pdeg)
                key = f"sweep_{w}x{h}x{n}_{deg}_{pdeg}_{b0}{b1}"
                assert refz.same(key + "_container", o.container, lambda: r.container()), (deg, pdeg, b0, b1)
                crd = np.stack([rng.uniform(-2.5 * w, 3.5 * w, 256),
                                rng.uniform(-2.5 * h, 3.5 * h, 256)], 1).astype(np.float32)
                crd[:64] = np.stack([rng.uniform(-1, w, 64), rng.uniform(-1, h, 64)], 1)
                assert refz.same(key + "_eval", o.eval(crd), lambda: r.eval(crd)), (deg, pdeg, b0, b1)


@pytest.mark.parametrize("shape", [(32, 16, 3), (64, 32, 4), (16, 8, 1), (128, 64, 3)])
def test_spherical_prefilter_sweep(shape):
    w, h, n = shape
    rng = np.random.default_rng(w)
    core = rng.random((h, w, n), dtype=np.float32)
    for deg in range(0, 10):
        for pdeg in sorted({deg, 3, 1}):
            r = refz.RefSpline(core, deg, 1, 2) if refz.available() else None
            o = euo.BSpline(core, deg, euo.PERIODIC, euo.REFLECT)
            if r:
                r.spherical(pdeg)
            o.spherical_prefilter(pdeg)
            assert refz.same(f"spherical_{w}x{h}x{n}_{deg}_{pdeg}", o.container, lambda: r.container()), (deg, pdeg)


def test_weights_and_poles():
    for d in range(10):
        for k, delta in enumerate(np.linspace(-0.5, 1.0, 31, dtype=np.float32)):
            assert refz.same(f"weights_{d}_{k}", euo.basis_weights(d, float(delta)),
                             lambda: refz.basis_weights(d, float(delta)))
        if d >= 2:
            assert refz.same(f"poles_{d}", euo.poles(d).astype(np.float32), lambda: refz.poles(d).astype(np.float32))


def test_lens_polynomial_sweep():
    """lcp<float>::eval of the oracle against the reference's lens_correction.h, compiled in
    place: random coefficient triples, radii over [0, 4] and all floats of a few binades"""
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.random(20000, dtype=np.float32) * np.float32(4.0),
                        np.arange(0x3f000000, 0x3f000000 + 50000, dtype=np.uint32).view(np.float32),
                        np.arange(0x3f800000 - 25000, 0x3f800000 + 25000, dtype=np.uint32).view(np.float32)])
    for k in range(40):
        a, b, c = (rng.uniform(-0.4, 0.4) for _ in range(3))
        assert refz.same(f"lcp_{k}", euo.lens_factor(a, b, c, x), lambda: refz.lcp_factor(a, b, c, x)), (a, b, c)


def test_inverse_lens_polynomial_sweep():
    """inverse_lcp of the oracle against the reference's class for random mild coefficient triples"""
    rng = np.random.default_rng(9)
    x = np.concatenate([rng.random(5000, dtype=np.float32) * np.float32(2.5), np.float32([0.0, 1e-9, 1.0, 7.0])])
    for i in range(25):
        a, b, c = (rng.uniform(-0.02, 0.02) for _ in range(3))
        r_max = rng.uniform(1.1, 2.0)
        for sz in (32, 100):
            o, k = euo.inverse_lcp(a, b, c, r_max, sz, x)
            ref = refz.inverse_lcp(a, b, c, r_max, sz, x) if refz.available() else (None, None)
            assert (refz.same(f"inverse_lcp_{i}_{sz}_knots", k, lambda: ref[1])
                    and refz.same(f"inverse_lcp_{i}_{sz}", o, lambda: ref[0])), (a, b, c, r_max, sz)
