"""The CPU oracle's spline of every degree 0 to 9 against the float64 spline of tests/spline64.py, which is written
from the definition (Cox-de Boor basis, dense collocation solve, no split of the coordinate) and shares no program
text with the oracle, the library or the reference. No GPU.

The bound is BIN_MARGIN times the ENVELOPES64 table of spline64, which print_envelopes64() measures with this same
oracle over these same cases; tests/test_gpu_spline64.py holds the library to the same rows. That the bound can
fail is shown here: each of spline64.FAULTS - one tap's weight off by 2^-10, the window of an even degree moved by a
texel, the last pole left out, the x and y weights exchanged - breaks it at every degree it applies to."""
import subprocess
import sys

import numpy as np
import pytest

import euo
import spline64 as s64


def test_the_basis_is_a_partition_of_unity_with_the_known_values():
    """the model's own foundation, against closed forms: B_d sums to 1 over the whole numbers at any offset, is
    symmetric, vanishes from (d + 1) / 2 on, and B_3(0) = 2/3, B_3(1) = 1/6, B_2(0) = 3/4, B_5(0) = 66/120"""
    t = np.linspace(-0.5, 0.5, 41)
    for d in s64.DEGREES:
        total = sum(s64.basis(d, t + k) for k in range(-6, 7))
        assert np.abs(total - 1.0).max() < 1e-14, d
        u = np.linspace(0.01, 5.2, 77)
        assert np.abs(s64.basis(d, u) - s64.basis(d, -u)).max() < 1e-15, d
        assert (s64.basis(d, np.array([(d + 1) / 2.0 + 1e-9, 7.0])) == 0.0).all(), d
    assert abs(s64.basis(3, 0.0) - 2 / 3) < 1e-15 and abs(s64.basis(3, 1.0) - 1 / 6) < 1e-15
    assert abs(s64.basis(2, 0.0) - 0.75) < 1e-15 and abs(s64.basis(5, 0.0) - 66 / 120) < 1e-15
    assert abs(s64.basis(9, 0.0) - 156190 / 362880) < 1e-15


@pytest.mark.parametrize("bc", [s64.PERIODIC, s64.REFLECT, s64.MIRROR, s64.NATURAL])
def test_the_model_interpolates_its_samples(bc):
    """what a prefiltered spline is for: at the whole numbers it gives the samples back, under every boundary
    condition, on a line shorter than the degree-9 horizon as well"""
    rng = np.random.default_rng(3)
    for w, h in ((40, 24), (9, 7)):
        img = rng.random((h, w, 2))
        yy, xx = np.mgrid[0:h, 0:w]
        for d in s64.DEGREES:
            m = s64.Spline64(img, d, bc, bc)
            assert np.abs(m(xx.ravel(), yy.ravel()) - img.reshape(-1, 2)).max() < 1e-9, (d, w, h)


def test_the_sphere_model_is_continuous_across_the_poles_and_the_seam():
    """the stacked columns: just above row -1/2 at column x the spline is what it is just below row -1/2 at column
    x + W/2, and column -1/2 is column W - 1/2"""
    img = np.random.default_rng(4).random((16, 32, 1))
    for d in (2, 5, 8, 9):
        m = s64.Spline64(img, d, s64.PERIODIC, s64.REFLECT, sphere=True)
        x = np.linspace(0.0, 15.0, 31)
        assert np.abs(m(x, np.full_like(x, -0.5)) - m(x + 16.0, np.full_like(x, -0.5))).max() < 1e-12, d
        assert np.abs(m(x, np.full_like(x, 15.5)) - m(x + 16.0, np.full_like(x, 15.5))).max() < 1e-12, d
        y = np.linspace(0.0, 15.0, 31)
        assert np.abs(m(np.full_like(y, -0.5), y) - m(np.full_like(y, 31.5), y)).max() < 1e-12, d


@pytest.mark.parametrize("degree", s64.DEGREES)
def test_oracle_plain_cores_within_the_envelope(degree):
    """euo.BSpline(core, d, b0, b1).prefilter(d) then .eval(crd): cores 40 x 24 x 3 and 9 x 7 x 1, uniform noise and
    jobs.synth_image, four boundary pairs, 300 points inside the core with 50 of them near a border"""
    worst = 0.0
    for case in s64.plain_cases():
        got, want = s64.oracle_plain(case, degree)
        assert got.shape == want.shape == (300, case[2])
        worst = max(worst, float(np.abs(got - want).max()))
    print("plain", degree, f"{worst:.3g}", "bound", s64.tolerance("plain", degree))
    assert worst <= s64.tolerance("plain", degree)


def test_the_border_points_are_where_they_should_be():
    for w, h, _ in s64.CORES:
        for d in s64.DEGREES:
            crd = s64.core_coordinates(w, h, d, seed=1)
            assert crd.shape == (300, 2) and (crd >= 0).all() and (crd[:, 0] <= w - 1).all() and (crd[:, 1] <= h - 1).all()
            dist = np.minimum(np.minimum(crd[:, 0], w - 1 - crd[:, 0]), np.minimum(crd[:, 1], h - 1 - crd[:, 1]))
            assert (dist[:50] <= d / 2.0 + 1.0).all()


@pytest.mark.parametrize("degree", s64.DEGREES)
def test_oracle_frames_within_the_envelope(degree):
    """the jobs of tests/test_gpu_spline64.py on the CPU oracle, the lat/lon 64 x 32 source on a rotated 40 x 20
    spherical target among them, modelled at the oracle's own stage-2 coordinates. The conditions that the GPU
    module takes for granted are checked here: at least half of every frame hits, every miss is exactly zero"""
    seen = set()
    for name, kind, target, deg, nch in s64.gpu_cases():
        if deg != degree:
            continue
        err, share, miss = s64.oracle_job(name, target, degree, nch)
        print(name, target, degree, nch, f"{err:.3g}", "bound", s64.tolerance(kind, degree), "hit", share)
        assert share >= 0.5 and miss == 0.0, (name, target)
        assert err <= s64.tolerance(kind, degree), (name, target, nch)
        seen.add(kind)
    assert seen == {"plain", "latlon"}


def test_some_frame_has_misses():
    shares = [s64.oracle_job(name, target, 1, 3)[1] for name in s64.SOURCES for target in s64.TARGETS[name]]
    assert min(shares) < 0.9 and min(shares) >= 0.5


def test_the_table_is_the_oracles_own():
    """ENVELOPES64 is what print_envelopes64() prints: measured, not chosen. A row differs from the measurement by
    the rounding of its three printed digits (half a percent) and the last bits of a float64 solve, no more"""
    table = s64.measure_envelopes64()
    assert set(table) == set(s64.ENVELOPES64)
    for key, measured in table.items():
        assert abs(s64.ENVELOPES64[key] - measured) <= 0.01 * measured, (key, s64.ENVELOPES64[key], measured)


@pytest.mark.parametrize("fault", s64.FAULTS)
def test_every_fault_breaks_the_bound(fault):
    """the proof that the envelope can fail: per kind and per degree the fault applies to"""
    table = s64.measure_envelopes64(fault)
    checked = 0
    for (kind, degree), worst in table.items():
        if s64.applies(fault, degree):
            print(fault, kind, degree, f"{worst:.3g}", "bound", s64.tolerance(kind, degree))
            assert worst > s64.tolerance(kind, degree), (fault, kind, degree, worst)
            checked += 1
    assert checked >= 10


def test_faults_leave_the_other_degrees_alone():
    """a fault that does not apply to a degree is the model itself there"""
    for fault in s64.FAULTS:
        for degree in s64.DEGREES:
            if not s64.applies(fault, degree):
                case = s64.plain_cases()[0]
                assert np.array_equal(s64.oracle_plain(case, degree, fault)[1], s64.oracle_plain(case, degree)[1])


def test_prefilter_degree_other_than_the_spline_degree():
    """(9, 3) and (4, 9): the collocation system is that of the prefilter degree, the basis that of the spline"""
    core = s64.core_image(40, 24, 3, "synth")
    crd = s64.core_coordinates(40, 24, 9, seed=5)
    for d, pd in ((9, 3), (4, 9)):
        o = euo.BSpline(core, d, euo.REFLECT, euo.REFLECT)
        o.prefilter(pd)
        want = s64.Spline64(core, d, s64.REFLECT, s64.REFLECT, prefilter_degree=pd)(crd[:, 0], crd[:, 1])
        assert np.abs(o.eval(crd) - want).max() <= s64.tolerance("plain", 9), (d, pd)


def test_the_gpu_modules_side_of_the_helper_loads_nothing_of_the_oracle():
    """what tests/test_gpu_spline64.py calls - pictures, models, jobs, compare - imports neither the oracle's binding nor
    tests/jobs.py, which imports it"""
    code = ("import sys, numpy as np; sys.path.insert(0, 'tests'); import spline64 as s\n"
            "for name, kind, target, degree, nch in s.gpu_cases()[:3] + s.layer_cases()[-2:]:\n"
            "    m = s.source_model(name, nch, degree); n = s.source_model(name, nch, degree, negative=True)\n"
            "    a = s.make_args(target, degree)\n"
            "    crd = np.zeros((a.height, a.width, 3), np.float32); crd[0, 0, 2] = -1\n"
            "    s.compare(np.zeros((a.height, a.width, nch), np.float32), crd, m)\n"
            "assert 'euo' not in sys.modules and 'jobs' not in sys.modules, sorted(sys.modules)\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=s64.__file__.rsplit("/tests/", 1)[0], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
