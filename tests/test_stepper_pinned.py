"""The oracle's ray generators (oracle/eu_oracle.c: stepper_init, planar_at, stepper_ray) against the reference's own
steppers: stepper.h compiled in place into oracle/_ref/libref_zimt.so and driven by zimt::process with pass_through
and storer (refz.stepper_rays, deriv_rays, planar, generic_rays), float32 bit patterns, no tolerance. Live where
that library is built; elsewhere against the digests of its results in tests/golden/stepper_digests.json (refz.same)
and, for the small jobs, against the arrays in tests/golden/stepper_golden.npz (tests/golden/make_stepper_golden.py).

The jobs are those of tests/stepper_cases.py: all seven projections, widths on every path of the driver, four
orientations, plain (normalize = false) and twined (normalize = true, bias .25, the biased neighbours r10 and r01
included), crop windows.

NOT pinned here: the basis. It is rotate(r_camera, r_facet^-1), which the reference computes with Imath and the
oracle with euo_make_r3 / euo_rotate_r3; the steppers of both sides get the oracle's basis as an INPUT. Nor
tf_ex_facet: generic_stepper is driven with a functor of the harness's own, (x, y) -> (x, y, 1), which pins its
planar chain and where it normalizes."""
import os

import numpy as np
import pytest

import euo
import jobs
import refz
from stepper_cases import BIAS, CASES, in_fixture

STEPPERS = "ref_stepper_rays"       # the library is live for these tests when it exports the steppers


def live():
    return refz.available(STEPPERS)


def same(key, ours, reference):
    return refz.same(key, ours, reference, symbol=STEPPERS)


pytestmark = pytest.mark.ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stepper_golden.npz")
_sources = {}


def source(fct):
    """an 8 x 4 lat/lon facet with this orientation: the rays do not depend on its pixels"""
    if fct not in _sources:
        _sources[fct] = jobs.OracleSource(euo.SPHERICAL, 8, 4, 360.0, jobs.synth_image(8, 4, 3), 1,
                                          yaw=fct[0], pitch=fct[1], roll=fct[2])
    return _sources[fct]


def oracle_rays(c):
    """stage 1 of the job, and stages 1, 3, 4 side by side (the ninepack) when it is twined"""
    a, o = c.oracle_args(), source(c.fct)
    r00 = jobs.oracle_render(a, o, stage=1)
    if not c.twined:
        return r00, None
    return r00, np.concatenate([r00, jobs.oracle_render(a, o, stage=3), jobs.oracle_render(a, o, stage=4)], axis=2)


def where(ours, ref):
    """the first differing pixel, for the failure message (live runs only)"""
    bad = np.argwhere((jobs.bits(ours) != jobs.bits(ref)).any(axis=2))
    return f"{len(bad)} pixels differ, first at (y, x) = {tuple(bad[0])}" if len(bad) else "same"


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_rays(c):
    """stage 1 is S<float, 16, twined>'s ray; stages 1 + 3 + 4 of a twined job are deriv_stepper<float, 16, S>'s
    ninepack"""
    r00, nine = oracle_rays(c)
    kw = dict(offset=c.offset, out_shape=c.out_shape)
    assert r00.shape == c.out_shape[::-1] + (3,)
    assert same(f"stepper_{c.name}_rays", r00,
                lambda: refz.stepper_rays(c.prj, c.twined, c.w, c.h, c.extent, c.basis, **kw)), \
        where(r00, refz.stepper_rays(c.prj, c.twined, c.w, c.h, c.extent, c.basis, **kw)) if live() else c.name
    if c.twined:
        assert same(f"stepper_{c.name}_nine", nine,
                    lambda: refz.deriv_rays(c.prj, c.w, c.h, c.extent, c.basis, BIAS, **kw)), \
            where(nine, refz.deriv_rays(c.prj, c.w, c.h, c.extent, c.basis, BIAS, **kw)) if live() else c.name
        # the neighbours are rays of their own, not copies of the centre
        assert (nine[..., 3:6] != nine[..., 0:3]).any() and (nine[..., 6:9] != nine[..., 0:3]).any()


def test_biased_stages_need_a_twined_single_facet_job():
    c = next(c for c in CASES if not c.twined)
    j = euo.Job()
    j.projection, j.width, j.height, j.row_end, j.nch = c.prj, c.w, c.h, c.h, 3
    j.x0, j.x1, j.y0, j.y1 = (float(v) for v in c.extent)
    out = np.zeros((c.h, c.w, 3), np.float32)
    for stage in (3, 4):
        j.stage = stage
        assert euo.lib().euo_render(euo.C.byref(j), euo.C.byref(source(c.fct).s), 1, euo.ptr(out), c.w * 3) == -6


def normalize3(v):
    """xel.h:752-765 and `trg /= norm(trg)`: sqn = v0 * v0; sqn += v1 * v1; sqn += v2 * v2; v / sqrt(sqn), float32"""
    v = v.astype(np.float32)
    sqn = v[..., 0] * v[..., 0]
    sqn = sqn + v[..., 1] * v[..., 1]
    sqn = sqn + v[..., 2] * v[..., 2]
    assert sqn.dtype == np.float32
    return v / np.sqrt(sqn)[..., None]


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_planar_chain(c):
    """euo_planar (planar_at: init per 512-pixel segment, += delta per 16-lane vector) is planar_stepper, unbiased for
    the plain jobs and with each neighbour's bias for the twined ones; followed by (x, y, 1), and by the norm when
    the job is twined, it is generic_stepper over that functor"""
    a = c.oracle_args()
    kw = dict(offset=c.offset, out_shape=c.out_shape)
    for bias in ([(BIAS, 0.0), (0.0, BIAS)] if c.twined else [(0.0, 0.0)]):
        pl = jobs.oracle_planar(a, *bias)
        assert pl.shape == c.out_shape[::-1] + (2,)
        key = f"stepper_{c.name}_b{bias[0]:g}.{bias[1]:g}"
        assert same(key + "_planar", pl, lambda: refz.planar(c.w, c.h, c.extent, bias, **kw)), (c.name, bias)
        xy1 = np.concatenate([pl, np.ones(pl.shape[:2] + (1,), np.float32)], axis=2)
        if c.twined:
            xy1 = normalize3(xy1)
        assert same(key + "_generic", xy1, lambda: refz.generic_rays(c.twined, c.w, c.h, c.extent, bias, **kw)), \
            (c.name, bias)


FIXTURE_CASES = [c for c in CASES if in_fixture(c)]


@pytest.mark.parametrize("c", FIXTURE_CASES, ids=[c.name for c in FIXTURE_CASES])
def test_fixture(c):
    """the reference's arrays as committed, so that a difference can be localised without the reference: the
    fixture's inputs are this job's, and the oracle's rays are the fixture's, bit for bit"""
    g = np.load(GOLDEN)
    assert np.array_equal(g[c.name + "/meta"], c.meta()), "the fixture was made from another job: re-make it"
    assert np.array_equal(g[c.name + "/basis"], c.basis), "the basis (an input of the reference) has changed"
    r00, nine = oracle_rays(c)
    ours, ref = (nine, g[c.name + "/nine"]) if c.twined else (r00, g[c.name + "/rays"])
    assert ours.shape == ref.shape and ref.dtype == np.float32
    assert (jobs.bits(ours) == jobs.bits(ref)).all(), where(ours, ref)


def test_fixture_holds_what_it_should():
    names = {k.split("/")[0] for k in np.load(GOLDEN).files}
    assert names == {c.name for c in FIXTURE_CASES}
    assert os.path.getsize(GOLDEN) < 512 * 1024
    # every projection at widths 15 to 37, one job past a segment boundary, one cropped ninepack
    small = [c for c in FIXTURE_CASES if not c.crop and c.w <= 37]
    assert {c.prj for c in small} == set(range(7))
    assert any(c.w > 512 and not c.crop for c in FIXTURE_CASES) and any(c.crop and c.twined for c in FIXTURE_CASES)
