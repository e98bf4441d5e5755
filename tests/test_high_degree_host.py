"""Spline degrees 4 to 9 on the host, no GPU. Before a single-facet job of tests/test_gpu_high_degree.py or
tests/test_gpu_spline64.py goes to a device: every tap of its degree-d window lies inside the container - computed from
the CPU oracle's coordinates (stage 2; for a twined job the coordinates of every tap's ray), which the device's are
proven to be bit for bit, and from ea.container_geometry / ea.cubemap_metrics, which size what the device allocates.
The job lists, the fuzz's draw function and its seeds live in tests/high_degree_cases.py, so this module replays what
the GPU module sends. Multi-facet jobs (six fisheye facets, feather, the multi-facet draws of the fuzz) are not walked
here: the issue asks for the single-facet jobs, and a facet of a multi-facet job is evaluated through the same gate
and window. The choice of the kernel at degrees 0 and 4 to 9 (envutil_amd/csrc/eu_select.h: never a packed or a staged
path, under every combination of EU_HIP_R4, EU_HIP_HYBRID, EU_HIP_KERNEL and EU_HIP_DIRECT) is asserted where the four
select demos are already built and run: tests/test_select.py, test_views_host.py, test_rays_host.py, test_layers_host.py."""
import numpy as np
import pytest

import envutil_amd as ea
import euo
import high_degree_cases as hd
import jobs
import spline64 as s64

@pytest.mark.parametrize("name", list(hd.SOURCES))
@pytest.mark.parametrize("degree", hd.DEGREES)
def test_taps_stay_inside_the_container(name, degree):
    """hd.single_facet_jobs(): what test_render_single_facet, test_fewer_output_channels..., test_rows_and_bands...
    and test_render_devices render, and the untwined halves of the views, layers and rays tests. Cube sources with the
    default support_min of 8 and with the smallest frame a degree-d window needs, d // 2 + 1"""
    hits = 0
    for cname, target, ypr in hd.single_facet_jobs():
        if cname != name:
            continue
        hits += hd.check_taps_inside(name, degree, target, ypr)
        if hd.cube(hd.SOURCES[name][0]):
            hd.check_taps_inside(name, degree, target, ypr, support_min=degree // 2 + 1)
    assert hits > 3000          # of 12546 pixels; the rectilinear source covers the least


@pytest.mark.parametrize("name", list(s64.SOURCES))
def test_taps_of_the_float64_jobs_stay_inside(name):
    """the jobs of tests/test_gpu_spline64.py: sources that Source.load builds, degrees 0 to 9"""
    kind, prj, w, h, hfov, lens = s64.SOURCES[name]
    for degree in s64.DEGREES:
        o = jobs.OracleSource(prj, w, h, hfov, s64.source_image(name, 1), degree, lens=lens)
        g = ea.container_geometry(degree, o.bc[0], o.bc[1], w, h)
        for target in s64.TARGETS[name]:
            crd = jobs.oracle_render(s64.make_args(target, degree), o, stage=2).reshape(-1, 3)
            hit = crd[:, 2] >= 0
            for axis, n in enumerate((w, h)):
                first, last = hd.window(hd.gate(crd[hit, axis], o.bc[axis], n), degree)
                assert first.min() >= -g.left[axis] and last.max() <= n - 1 + g.right[axis], (name, degree, target, axis)


def test_the_window_check_can_fail():
    """a frame one texel too narrow, or a window moved by one, is caught: the bounds are tight somewhere"""
    tight = 0
    for degree in hd.DEGREES:
        prj, w, h, hfov, kw = hd.SOURCES["rectilinear"]
        o = hd.oracle_source("rectilinear", 1, degree)
        g = ea.container_geometry(degree, o.bc[0], o.bc[1], w, h)
        crd = jobs.oracle_render(hd.args_of(hd.TARGETS[1], hd.YPRS[1], degree), o, stage=2).reshape(-1, 3)
        hit = crd[:, 2] >= 0
        first, last = hd.window(hd.gate(crd[hit, 0], o.bc[0], w), degree)
        assert first.min() >= -g.left[0] and last.max() <= w - 1 + g.right[0]
        tight += int(first.min() - 1 < -g.left[0]) + int(last.max() + 1 > w - 1 + g.right[0])
    assert tight >= 1


def test_gate_and_window():
    """REFLECT mirrors on -0.5 and n - 0.5, PERIODIC wraps; floor for odd and round-half-away for even degrees"""
    c = np.float32([-0.5, -0.25, 0.0, 9.49, 9.5, 9.75, 10.5, -1.5])
    assert np.allclose(hd.gate(c, euo.REFLECT, 10), [-0.5, -0.25, 0.0, 9.49, 9.5, 9.25, 8.5, 0.5])
    assert np.allclose(hd.gate(c, euo.PERIODIC, 10), [-0.5, -0.25, 0.0, 9.49, -0.5, -0.25, 0.5, 8.5])
    g = np.float32([-0.5, 0.49, 0.5, 2.5, 3.2])
    assert list(hd.window(g, 9)[0]) == [-5, -4, -4, -2, -1] and list(hd.window(g, 9)[1]) == [4, 5, 5, 7, 8]
    assert list(hd.window(g, 8)[0]) == [-5, -4, -3, -1, -1] and list(hd.window(g, 8)[1]) == [3, 4, 5, 7, 7]


@pytest.mark.parametrize("degree", hd.DEGREES)
def test_taps_of_the_twined_view_layer_and_ray_jobs_stay_inside(degree):
    """test_twining (twine 2 and 3), the three views of test_render_views - the third has an hfov of its own -, the
    twine-2 layers of test_render_layers and the ninepacks of test_render_rays (the taps of twine 3)"""
    hits = 0
    if degree in hd.TWINE_DEGREES:
        for name in hd.SOURCES:
            for twine in (2, 3):
                for target, ypr in hd.TWINE_JOBS:
                    hits += hd.check_job(name, degree, hd.args_of(target, ypr, degree, twine=twine), f"twine {twine} -> {target}")
    for target in hd.BATCH_TARGETS:
        for name in hd.VIEW_SOURCES:
            for v in hd.VIEWS:
                hits += hd.check_job(name, degree, hd.view_args(target, v, degree), f"view {v} -> {target}")
        for name in hd.LAYER_SOURCES:
            hits += hd.check_job(name, degree, hd.args_of(target, hd.YPRS[1], degree, twine=2), f"layers, twine 2 -> {target}")
        for name in hd.RAY_SOURCES:
            hits += hd.check_job(name, degree, hd.args_of(target, hd.YPRS[1], degree, twine=3), f"ninepacks -> {target}")
    assert hits > 100000


@pytest.mark.parametrize("degree", hd.TRANSLATED_DEGREES)
def test_taps_of_the_translated_and_single_jobs_stay_inside(degree):
    """test_translated_facet: the translated 128 x 96 facet, plain and twined, and the --single target on the lat/lon
    source, all on the generic stepper"""
    o, spec = hd.translated_source(degree)
    hits = 0
    for ypr, twine in hd.TRANSLATED_JOBS:
        a = hd.args_of(hd.TRANSLATED_TARGET, ypr, degree, twine=twine)
        hits += hd.check_windows(o, spec.projection, spec.width, spec.height, hd.job_coordinates(a, o), degree,
                                 f"translated facet degree {degree} {ypr} twine {twine}")
    prj, w, h, hfov, kw = hd.SOURCES["latlon"]
    ol = hd.oracle_source("latlon", 3, degree)
    hits += hd.check_windows(ol, prj, w, h, hd.job_coordinates(hd.single_target_args(degree), ol), degree, f"--single, degree {degree}")
    assert hits > 20000


def test_taps_of_the_render_after_the_reload_stay_inside():
    prj, w, h, hfov = hd.RELOAD_SOURCE
    o = jobs.OracleSource(prj, w, h, hfov, hd.reload_pictures()[1], hd.RELOAD_DEGREE)
    a = hd.args_of(*hd.RELOAD_JOB, hd.RELOAD_DEGREE)
    assert hd.check_windows(o, prj, w, h, hd.job_coordinates(a, o), hd.RELOAD_DEGREE, "after the reload") == 65 * 33


@pytest.mark.parametrize("seed", hd.FUZZ_SEEDS)
def test_taps_of_the_fuzz_stay_inside(seed):
    """hd.fuzz_jobs(seed) is what test_random_high_degree_jobs_bit_identical renders: every single-facet draw, with
    its twining and its crop"""
    for job in hd.fuzz_jobs(seed):
        if len(job["facets"]) == 1:
            o, spec, (prj, w, h), desc = job["facets"][0]
            hd.check_windows(o, prj, w, h, hd.job_coordinates(job["args"], o), job["degree"], job["what"])


def test_the_fuzz_draws_single_and_multi_facet_jobs_that_hit():
    drawn = [job for seed in hd.FUZZ_SEEDS for job in hd.fuzz_jobs(seed)]
    single = [j for j in drawn if len(j["facets"]) == 1]
    assert len(drawn) == 40 and 10 <= len(single) <= 30
    assert {j["degree"] for j in drawn} == {4, 5, 6, 7, 8, 9}
    hits = [hd.check_windows(j["facets"][0][0], *j["facets"][0][2], hd.job_coordinates(j["args"], j["facets"][0][0]), j["degree"],
                             j["what"]) for j in single]
    assert sum(n > 0 for n in hits) >= 15
