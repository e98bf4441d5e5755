"""The CPU oracle's PIXELS against a float64 model written from the definitions (tests/definitions64.py):
the source holds an analytic function of the ray direction, the oracle renders it, and the frame is compared
with the same function at the float64 target rays. The bit-for-bit tests pin the kernels to the oracle; this
pins the oracle - its half-texel conventions, boundary schemes, seam, poles, cube frame, twining sum, synopses
and lens polynomial - to something that shares no text with it.

Tolerances come from definitions64.ENVELOPES (measured oracle against model, see there) with the margins of
definitions64.bounds(); the convergence ratio 3 is derived: linear interpolation errs with O(h^2), ratio 4 on
doubling the resolution, a misplacement by a fixed fraction of a texel with O(h), ratio 2.

Every family of assertions is also run on definitions64.shifted(...), the model with a deliberate fault, and
must fail there."""
import numpy as np
import pytest

import definitions64 as d
import euo
import jobs

RATIO = 3.0
MATCHING_FAULT = {"plain": "source_half_texel", "latlon": "source_half_texel", "cubemap": "cube_transposed",
                  "biatan6": "cube_transposed"}


def fails(check, *a, **kw):
    try:
        check(*a, **kw)
    except AssertionError:
        return True
    return False


def test_the_table_is_what_the_oracle_measures():
    got = d.measure_envelopes(d.oracle_render, d.make_args)
    assert set(got) == set(d.ENVELOPES)
    for k, v in got.items():
        for g, t in zip(np.atleast_1d(v), np.atleast_1d(d.ENVELOPES[k])):
            assert abs(g - t) <= 0.02 * t + 1e-9, (k, v, d.ENVELOPES[k])


def test_the_scene_is_smooth_bounded_and_differs_per_channel():
    rays = np.random.default_rng(1).normal(size=(20000, 3))
    v = d.fields(rays, 4)
    assert v[:, :3].min() > 0.1 and v[:, :3].max() < 0.9 and (v[:, 3] == 1.0).all() and (d.fields(rays, 2)[:, 1] == 1.0).all()
    assert np.abs(d.fields(rays, 3) - d.fields(3.7 * rays, 3)).max() < 1e-15      # of the direction alone
    assert min(np.abs(v[:, a] - v[:, b]).max() for a in range(3) for b in range(a)) > 0.2      # a channel swap shows


# ---- interpolation-exact cases --------------------------------------------------------------------------------------

@pytest.mark.parametrize("degree", [2, 3])
@pytest.mark.parametrize("case", d.exact_cases(), ids=lambda c: c[0])
def test_interpolation_exact(case, degree):
    """degree 2 and 3 reproduce the scene to the float32 floor: against the scene itself and against scipy's
    spline of the same samples at float64 coordinates (tier1)"""
    name, f, t, ypr = case
    a = d.make_args(t, ypr, degree)
    got = d.oracle_render([f], degree, a, 3)
    j = d.judge(got, a, [f], 3)
    far = j.counted & (j.dist >= 8.0)
    tol = d.floor_tolerance(degree)
    print(name, degree, "scene", j.far_max(), "tolerance", tol)
    assert j.covered_share >= 0.5 and j.left_out_share <= 0.05 and far.sum() >= 0.9 * j.counted.sum()
    assert j.far_max() <= tol
    t1, _ = d.tier1(a, f, d.facet_image(f, 3), degree)
    e1 = np.abs(got - t1).max(-1)[far].max()
    print(name, degree, "tier1", e1)
    assert e1 <= tol
    # the check can fail, and the tolerance is small against what a fault does
    for fault in ("source_half_texel", "target_half_pixel", "yaw_sign"):
        js = d.judge(d.shifted(fault, a, f, 3), a, [f], 3)
        assert js.far_max() > 10.0 * tol, (fault, js.far_max())
    js = d.judge(d.shifted("source_half_texel", a, f, 3, d.facet_image(f, 3), degree), a, [f], 3)
    assert js.far_max() > 10.0 * tol


def test_the_lens_polynomial_matters():
    """the facets with a lens polynomial, rendered as if they had none, miss the scene by far more than the floor"""
    for name in ("fisheye lens", "rectilinear lens"):
        f = d.PLAIN[name]
        bare = d.Facet(f.prj, f.w, f.h, f.hfov, f.yaw, f.pitch, f.roll)
        t, ypr = d.looking_at(f)
        a = d.make_args(t, ypr, 3)
        cx, cy, _, face = d.source_coordinates(bare, d.camera_rays(a))
        j = d.judge(d.fields(d.coordinates_to_rays(f, cx, cy, face), 3), a, [f], 3)
        assert j.far_max() > 1e-3


# ---- convergence at degree 1 ------------------------------------------------------------------------------------------

def convergence_cases():
    out = [(name, f) + d.looking_at(f, hfov=60.0 if f.prj == d.RECTILINEAR else 80.0) for name, f in d.PLAIN.items()]
    out.append(("latlon", d.LATLON[128], d.T_RECT, (40.0, 10.0, 5.0)))
    out.append(("latlon, whole sphere", d.LATLON[128], d.T_SPH, d.ROTATED))
    out.append(("cubemap", d.CUBES[("cubemap", 32)], d.T_SPH, d.ROTATED))
    out.append(("biatan6", d.CUBES[("biatan6", 32)], d.T_SPH, d.ROTATED))
    return out


def errors_on_doubling(f, t, ypr, render, select=None):
    out = []
    for fct in (f, d.doubled(f)):
        a = d.make_args(t, ypr, 1)
        j = d.judge(render(fct, a), a, [fct], 3)
        m = j.counted if select is None else j.counted & select(j)
        assert j.covered_share >= 0.5 and j.left_out_share <= 0.05
        out.append(float(j.err[m].max()))
    return out


@pytest.mark.parametrize("case", convergence_cases(), ids=lambda c: c[0])
def test_bilinear_error_falls_fourfold_when_the_source_doubles(case):
    name, f, t, ypr = case
    oracle = lambda fct, a: d.oracle_render([fct], 1, a, 3)
    # the outermost half texel of a biatan6 face is first order (see below and DESIGN.md section 2)
    inner = (lambda j: j.dist >= 0.5) if f.prj == d.BIATAN6 else None
    e = errors_on_doubling(f, t, ypr, oracle, inner)
    print(name, e, e[0] / e[1])
    assert e[0] / e[1] >= RATIO
    # a renderer that is half a texel off converges like a misplacement: the same check fails
    if f.prj in d.CUBE:
        faulty = lambda fct, a: d.shifted("source_half_texel", a, fct, 3)
    else:
        faulty = lambda fct, a: d.shifted("source_half_texel", a, fct, 3, d.facet_image(fct, 3), 1)
    s = errors_on_doubling(f, t, ypr, faulty, inner)
    print(name, "shifted", s, s[0] / s[1])
    assert s[0] / s[1] < RATIO


def test_biatan6_support_frame_is_first_order():
    """cubemap.h fills the support frame of a face by picking the neighbour face up at the RECTILINEAR in-face
    coordinate of the frame pixel's ray, for both cube kinds (its comment at fill_frame_t::eval says why); for
    biatan6 that misplaces the frame, so the outermost half texel of a face - which interpolates into the frame -
    converges like a misplacement while the rest of the face converges like bilinear interpolation. Pinned as
    the reference's behaviour; the envelope rows of biatan6 hold its size."""
    f = d.CUBES[("biatan6", 32)]
    oracle = lambda fct, a: d.oracle_render([fct], 1, a, 3)
    edge = errors_on_doubling(f, d.T_SPH, d.ROTATED, oracle, lambda j: j.dist < 0.5)
    rest = errors_on_doubling(f, d.T_SPH, d.ROTATED, oracle, lambda j: j.dist >= 0.5)
    print("outer half texel", edge, edge[0] / edge[1], "rest", rest, rest[0] / rest[1])
    assert 2.0 <= edge[0] / edge[1] < RATIO <= rest[0] / rest[1]
    # the rectilinear cube has no such zone
    f = d.CUBES[("cubemap", 32)]
    edge = errors_on_doubling(f, d.T_SPH, d.ROTATED, oracle, lambda j: j.dist < 0.5)
    assert edge[0] / edge[1] >= RATIO


# ---- envelopes: seam, poles, cube face edges, image borders -----------------------------------------------------------

@pytest.mark.parametrize("degree", [2, 3])
@pytest.mark.parametrize("case", d.envelope_cases(), ids=lambda c: f"{c[0][0]}{c[0][1]}-{c[2][0]}-{c[3][0]}")
def test_envelopes(case, degree):
    kind, f, t, ypr = case
    a = d.make_args(t, ypr, degree)
    j = d.judge(d.oracle_render([f], degree, a, 3), a, [f], 3)
    print(kind, degree, j.bins())
    assert j.covered_share >= 0.5 and j.left_out_share <= 0.05 and j.outside_max == 0.0
    d.assert_within(j, kind, degree, str(kind))
    # the check can fail: the matching fault breaks it, and by ten times the widest bound of the row
    fault = MATCHING_FAULT[kind[0]]
    js = d.judge(d.shifted(fault, a, f, 3), a, [f], 3)
    assert fails(d.assert_within, js, kind, degree)
    assert js.max() > 10.0 * max(d.bounds(kind, degree)), (js.max(), d.bounds(kind, degree))
    # half a texel shows in the bins the envelope holds tight (a texel and more from the structure)
    js = d.judge(d.shifted("source_half_texel", a, f, 3), a, [f], 3)
    assert fails(d.assert_within, js, kind, degree)


def test_seam_and_pole_error_is_the_tolerance_of_the_spherical_prefilter():
    """environment.h's spherical_prefilter builds its periodic filters with tolerance 0.0001 (iir_filter_specs),
    so the causal initial value is a sum over 7 (degree 3) or 6 (degree 2) samples, not over the whole period.
    What is cut off is about 1e-4 of the amplitude, it sits where the filter lines start - the first columns and
    the first rows over the pole - decays by the pole (0.27, 0.17) per texel and does not shrink with the
    resolution. The oracle and the library pass the same tolerance; here the row filter with that tolerance is
    compared with the untruncated one (tolerance 0: the closed form over the whole period)"""
    P = euo.PERIODIC
    for w in (128, 256):
        img = d.facet_image(d.LATLON[w], 3)[:, :, 0]
        for degree, lo, hi in ((3, 2e-5, 2e-4), (2, 5e-6, 1e-4)):
            rows = [np.ascontiguousarray(img) for _ in range(2)]
            for r, tol in zip(rows, (0.0001, 0.0)):
                euo.lib().euo_filter_lines(euo.ptr(r), r.shape[0], w, w, 1, P, degree, tol)
            diff = np.abs(rows[0].astype(np.float64) - rows[1]).max(0)
            print(w, degree, diff[:10], diff[-4:])
            assert lo < diff[:2].max() < hi and diff[10:-10].max() < 1e-6
            assert (diff[:6] > 0.1 * diff[1:7]).all()            # decays, never grows, away from the start
    # the envelope rows of the two sizes agree near the seam: the bins do not converge with the resolution
    for degree in (2, 3):
        a, b = (d.ENVELOPES[("latlon", w, degree)] for w in (128, 256))
        assert 0.5 < a[0] / b[0] < 2.0


@pytest.mark.parametrize("degree", [2, 3])
def test_every_job_of_the_gpu_module_holds_on_the_oracle(degree):
    """the jobs tests/test_gpu_definitions.py gives the library, given to the oracle: the rows of the table cover them"""
    for kind, fs, t, ypr, syn in d.all_envelope_jobs():
        a = d.make_args(t, ypr, degree, synopsis=syn)
        j = d.judge(d.oracle_render(fs, degree, a, 3), a, fs, 3)
        assert j.covered_share >= 0.5 and j.outside_max == 0.0, (kind, t, ypr)
        d.assert_within(j, kind, degree, f"{kind} {t} {ypr}")


# ---- a translated facet ---------------------------------------------------------------------------------------------

TRANSLATED_JOBS = [((d.RECTILINEAR, 150, 77, 60.0), (5.0, -2.0, 0.0)), ((d.RECTILINEAR, 150, 77, 60.0), (12.0, 4.0, 8.0))]


@pytest.mark.parametrize("degree", [2, 3])
def test_translated_facet(degree):
    """tf_ex_facet / generic_r3 with TrX, TrY, TrZ, Tpy, Tpp: a scene on the translation plane, the facet's image
    made by intersecting its pixel rays from where its camera stands with that plane, the expectation by
    intersecting the target's rays from the origin with it - plain geometry in float64 (definitions64)"""
    f = d.translated_facet()
    tol = d.floor_tolerance(degree)
    for t, ypr in TRANSLATED_JOBS:
        a = d.make_args(t, ypr, degree)
        got = d.oracle_render([f], degree, a, 3)
        j = d.judge_translated(got, a, f, 3)
        print(degree, ypr, j.bins())
        assert j.covered_share >= 0.5 and j.left_out_share <= 0.05 and j.far_max() <= tol
        # each convention shows: an image made with the camera on the other side, with the plane turned the other
        # way, or with TrZ alone negated, rendered with the facet's true parameters, is not the scene
        for wrong in (dict(f.translation, x=-0.1, y=0.05, z=-0.08), dict(f.translation, tp_y=-10.0), dict(f.translation, tp_p=5.0),
                      dict(f.translation, z=-0.08)):
            g = d.Facet(f.prj, f.w, f.h, f.hfov, f.yaw, f.pitch, f.roll, translation=wrong)
            o = jobs.OracleSource(f.prj, f.w, f.h, f.hfov, d.translated_image(g, 3), degree, yaw=f.yaw, pitch=f.pitch, roll=f.roll,
                                  translation=f.translation)
            assert d.judge_translated(jobs.oracle_render(a, o), a, f, 3).far_max() > 10.0 * tol, wrong


# ---- twining ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", d.twine_cases(), ids=lambda c: f"twine{c[0]}")
def test_twining(case):
    """the tap sum against the weighted sum of the scene at the rays of the offset planar coordinates. twine_t
    makes the tap rays by differencing (ray + dx (ray_x - ray) + dy (ray_y - ray)): second order in the pixel
    size, so the error falls fourfold when the target doubles"""
    n, f, t, ypr, small = case
    errs = []
    for tgt in (small, t):
        a = d.make_args(tgt, ypr, 3, twine=n)
        assert len(a.twine_spread) == n * n and abs(a.twine_spread[:, 2].sum() - 1.0) < 1e-6
        j = d.judge(d.oracle_render([f], 3, a, 3), a, [f], 3)
        assert j.covered_share >= 0.5 and j.left_out_share <= 0.05
        errs.append(j.max())
    print("twine", n, errs, errs[0] / errs[1])
    bound = d.BIN_MARGIN * d.ENVELOPES[("twine", n)]
    assert errs[1] <= bound
    assert errs[0] / errs[1] >= RATIO
    # model against model: unnormalised weights break the envelope by far, half a target pixel converges first order
    a = d.make_args(t, ypr, 3, twine=n)
    assert d.judge(d.shifted("weights_unnormalised", a, f, 3), a, [f], 3).max() > 10.0 * bound
    s = []
    for tgt in (small, t):
        a = d.make_args(tgt, ypr, 3, twine=n)
        s.append(d.judge(d.shifted("target_half_pixel", a, f, 3), a, [f], 3).max())
    assert s[0] / s[1] < RATIO and s[1] > 10.0 * bound


# ---- synopses ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nch", [3, 4])
@pytest.mark.parametrize("degree", [2, 3])
@pytest.mark.parametrize("case", d.synopsis_cases(), ids=lambda c: c[0])
def test_synopses(case, degree, nch):
    """facets that all hold the same scene, through their own orientations (hdr_merge: divided by their own
    brighten): every covered pixel is the scene, every pixel more than two texels outside all of them is zero"""
    name, fs, t, ypr, syn = case
    a = d.make_args(t, ypr, degree, synopsis=syn)
    j = d.judge(d.oracle_render(fs, degree, a, nch), a, fs, nch)
    print(name, degree, nch, j.covered_share, j.left_out_share, j.outside.mean(), j.bins())
    assert j.covered_share >= 0.5 and j.left_out_share <= 0.05
    assert j.outside.any() and j.outside_max == 0.0
    d.assert_within(j, ("plain", 0), degree, name)
    for fault in ("yaw_sign", "target_half_pixel"):
        assert fails(d.assert_within, d.judge(d.shifted(fault, a, fs[0], nch), a, fs, nch), ("plain", 0), degree), fault
