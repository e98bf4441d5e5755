"""`act` alone: ea.render_rays (eu_hip_render_rays) against the CPU oracle. The oracle's stage 1 gives the rays of
a job and its stage 0 evaluates env_eval on exactly those rays, so `render_rays(source, rays of J)` must be J's
frame - float32 bit patterns, 0 ULP, no pixel left out - with no oracle code of its own. Sizes are those of
tests/test_gpu_parity.py."""
import ctypes
import subprocess

import numpy as np
import pytest

import envutil_amd as ea
import euo
import jobs
from test_gpu_parity import SRC_H, SRC_W, TARGETS, assert_bits, make_pair
from test_rays_host import build_demo

pytestmark = pytest.mark.gpu

YPRS = [(0, 0, 0), (30, 15, 7.5)]
FACET_W, FACET_H = 129, 97

# name -> (projection, width, height, hfov, channels, degree, keywords of make_pair, packed form?)
SOURCES = {
    "latlon d1 n1": (euo.SPHERICAL, SRC_W, SRC_H, 360.0, 1, 1, {}, True),
    "latlon d1 n3": (euo.SPHERICAL, SRC_W, SRC_H, 360.0, 3, 1, {}, True),
    "latlon d1 n4": (euo.SPHERICAL, SRC_W, SRC_H, 360.0, 4, 1, {}, True),
    "latlon d3 n1": (euo.SPHERICAL, SRC_W, SRC_H, 360.0, 1, 3, {}, True),
    "latlon d3 n3": (euo.SPHERICAL, SRC_W, SRC_H, 360.0, 3, 3, {}, True),
    "latlon d3 n4": (euo.SPHERICAL, SRC_W, SRC_H, 360.0, 4, 3, {}, True),
    "latlon d0": (euo.SPHERICAL, SRC_W, SRC_H, 360.0, 3, 0, {}, False),
    "latlon d5": (euo.SPHERICAL, SRC_W, SRC_H, 360.0, 3, 5, {}, False),
    "cubemap d2": (euo.CUBEMAP, 32, 192, 90.0, 3, 2, {}, True),
    "biatan6 d3": (euo.BIATAN6, 24, 144, 90.0, 3, 3, {}, True),
    "rectilinear lens": (euo.RECTILINEAR, FACET_W, FACET_H, 80.0, 3, 3,
                         dict(lens=dict(a=0.02, b=0.0, c=-0.01, h=0.01, v=-0.02)), False),
    "fisheye": (euo.FISHEYE, FACET_W, FACET_H, 190.0, 3, 1, {}, False),
    "latlon brighten": (euo.SPHERICAL, SRC_W, SRC_H, 360.0, 4, 3, dict(brighten=0.8), True),
    # the facet's own orientation is part of the stepper's basis, so it is in the rays already: the ray path
    # must not rotate again
    "rectilinear ypr": (euo.RECTILINEAR, FACET_W, FACET_H, 80.0, 3, 1, dict(yaw=40.0, pitch=-15.0, roll=20.0), False),
}

_pairs, _rays = {}, {}


def pair(name):
    if name not in _pairs:
        prj, w, h, hfov, nch, degree, kw, _ = SOURCES[name]
        img = jobs.synth_cubefaces(w, nch) if prj in (euo.CUBEMAP, euo.BIATAN6) else jobs.synth_image(w, h, nch, seed=31)
        _pairs[name] = make_pair(prj, w, h, hfov, img, degree, **kw)
    return _pairs[name]


def job_rays(a, o):
    """the oracle's stage-1 rays of job `a` on source `o`: they depend on the target and the two orientations"""
    key = (a.projection, a.width, a.height, a.hfov, a.yaw, a.pitch, a.roll, o.s.yaw, o.s.pitch, o.s.roll)
    if key not in _rays:
        r = jobs.oracle_render(a, o, stage=1)
        r.setflags(write=False)
        _rays[key] = r
    return _rays[key]


def all_jobs(degree):
    for tprj, tw, th, thfov in TARGETS:
        for ypr in YPRS:
            yield ea.arguments(tprj, tw, th, thfov, yaw=ypr[0], pitch=ypr[1], roll=ypr[2], spline_degree=degree)


@pytest.mark.parametrize("name", list(SOURCES))
def test_rays_of_a_job_give_its_frame(name, monkeypatch):
    """all eight TARGETS at both orientations (1100 x 12 and 129 x 97 end in a lane-pair tail); the packed-eligible
    sources run again under EU_HIP_KERNEL=1, through the general form"""
    o, g = pair(name)
    degree, packed = SOURCES[name][5], SOURCES[name][7]
    for a in all_jobs(degree):
        rays, ref = job_rays(a, o), jobs.oracle_render(a, o)
        what = f"{name}: target {a.projection} {a.width}x{a.height} ypr {a.yaw, a.pitch, a.roll}"
        got = ea.render_rays(g, rays)
        assert got.shape == ref.shape
        assert_bits(got, ref, what)
        if packed:
            monkeypatch.setenv("EU_HIP_KERNEL", "1")
            assert_bits(ea.render_rays(g, rays), ref, what + ", EU_HIP_KERNEL=1")
            monkeypatch.delenv("EU_HIP_KERNEL")


@pytest.mark.parametrize("src_n,out_n", [(s, t) for s in (1, 2, 3, 4) for t in (1, 2, 3, 4) if s != t])
def test_channel_adaption(src_n, out_n):
    """the twelve nch -> nchannels pairs of test_repix_channel_adaption_bit_exact, against the oracle's nch= frames"""
    img = jobs.synth_image(128, 64, src_n, seed=4)
    if src_n in (2, 4):
        img[:, :, src_n - 1] = (np.indices((64, 128))[1] % 7 != 0).astype(np.float32)
    o, g = make_pair(euo.RECTILINEAR, 128, 64, 100.0, img, 1, brighten=1.3)
    a = ea.arguments(ea.SPHERICAL, 150, 75, 360.0, yaw=20, spline_degree=1)
    got = ea.render_rays(g, job_rays(a, o), nchannels=out_n)
    assert_bits(got, jobs.oracle_render(a, o, nch=out_n), f"repix {src_n}->{out_n}")
    # and a source of the packed kind: channel adaption sends it through the general form
    img = jobs.synth_image(SRC_W, SRC_H, src_n, seed=4)
    o, g = make_pair(euo.SPHERICAL, SRC_W, SRC_H, 360.0, img, 3)
    a = ea.arguments(ea.RECTILINEAR, 129, 97, 90.0, pitch=10, spline_degree=3)
    assert_bits(ea.render_rays(g, job_rays(a, o), nchannels=out_n), jobs.oracle_render(a, o, nch=out_n),
                f"repix {src_n}->{out_n}, lat/lon")


@pytest.mark.parametrize("name", ["latlon d3 n3", "cubemap d2", "rectilinear lens"])
@pytest.mark.parametrize("general", [False, True])
def test_no_dependence_on_the_grid(name, general, monkeypatch):
    """the rays of one job, flattened and permuted, as (1, N), (N, 1) and (N / 127, 127), dense and with padded
    ray rows and padded output rows: the same permutation of the oracle's pixels, the padding untouched"""
    if general:
        monkeypatch.setenv("EU_HIP_KERNEL", "1")
    o, g = pair(name)
    a = ea.arguments(ea.SPHERICAL, 200, 100, 360.0, yaw=30, pitch=15, roll=7.5, spline_degree=SOURCES[name][5])
    rays, ref = job_rays(a, o).reshape(-1, 3), jobs.oracle_render(a, o).reshape(-1, 3)
    n = rays.shape[0] // 127 * 127
    perm = np.random.default_rng(20240611).permutation(rays.shape[0])[:n]
    rays, ref = np.ascontiguousarray(rays[perm]), ref[perm]
    for shape in [(1, n), (n, 1), (n // 127, 127), (n,)]:
        got = ea.render_rays(g, rays.reshape(shape + (3,)))
        assert got.shape == shape + (3,)
        assert_bits(got.reshape(-1, 3), ref, f"{name} as {shape}")
    # padded rows on both sides; the output's padding keeps its sentinel
    h, w = n // 127, 127
    wide = np.full((h, w + 5, 3), np.nan, np.float32)
    wide[:, :w] = rays.reshape(h, w, 3)
    sentinel = np.float32(-12345.5)
    out = np.full((h, w + 3, 3), sentinel, np.float32)
    res = ea.render_rays(g, wide[:, :w], out=out[:, :w])
    assert np.shares_memory(res, out)
    assert_bits(out[:, :w].reshape(-1, 3), ref, f"{name}, padded rows")
    assert (out[:, w:] == sentinel).all(), "the padding of `out` was written"


def test_device_buffers_and_streams(monkeypatch):
    """torch tensors in and out on a non-default stream, then eu_hip_sync(); host rays with a device output,
    and device rays with a host output"""
    import torch
    o, g = pair("latlon d3 n3")
    a = ea.arguments(ea.RECTILINEAR, 129, 97, 90.0, yaw=30, pitch=15, roll=7.5, spline_degree=3)
    rays, ref = job_rays(a, o), jobs.oracle_render(a, o)
    dev = torch.device("cuda")
    rays_t = torch.from_numpy(np.array(rays)).to(dev)
    stream = torch.cuda.Stream()
    for general in (False, True):
        out_t = torch.full(ref.shape, -1.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        if general:
            monkeypatch.setenv("EU_HIP_KERNEL", "1")
        assert ea.render_rays(g, rays_t, out=out_t, stream=stream.cuda_stream) is out_t
        ea.sync()
        monkeypatch.delenv("EU_HIP_KERNEL", raising=False)
        assert_bits(out_t.cpu().numpy(), ref, f"device in, device out, general={general}")
    out_t = torch.zeros(ref.shape, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ea.render_rays(g, np.array(rays), out=out_t)
    assert_bits(out_t.cpu().numpy(), ref, "host rays, device output")
    assert_bits(ea.render_rays(g, rays_t), ref, "device rays, host output")
    # a device tensor with padded rows
    wide = torch.zeros((97, 140, 3), dtype=torch.float32, device=dev)
    wide[:, :129] = rays_t
    assert_bits(ea.render_rays(g, wide[:, :129]), ref, "device rays with padded rows")


TWINE_CASES = {
    "latlon d1 n3": None,          # packed, TWINE
    "rectilinear lens": None,      # general
    "latlon d3 n3": 4,             # channel adaption: general
}
SPREADS = [dict(twine=3), dict(twine=7, twine_width=1.0, twine_sigma=1.5, twine_threshold=0.02)]


def ninepacks(a, g):
    """stage 1, 3 and 4 of a twined job: ray, x-neighbour, y-neighbour"""
    return np.concatenate([ea.render(a, g, stage=k) for k in (1, 3, 4)], axis=2)


@pytest.mark.parametrize("name", list(TWINE_CASES))
@pytest.mark.parametrize("spread", [0, 1])
def test_twining_end_to_end(name, spread):
    """the GPU's stages 1, 3, 4 of a twined job are its ninepacks; render_rays(..., taps) must be the oracle's frame
    of the twined job"""
    o, g = pair(name)
    out_n = TWINE_CASES[name]
    for tprj, tw, th, thfov in [TARGETS[2], TARGETS[5], TARGETS[0]]:
        a = ea.arguments(tprj, tw, th, thfov, yaw=30, pitch=15, roll=7.5, spline_degree=SOURCES[name][5], **SPREADS[spread])
        if spread == 0:
            assert len(a.twine_spread) == 9
            assert np.array_equal(a.twine_spread, ea.make_spread(3, 3))
        else:
            assert np.array_equal(a.twine_spread, ea.make_spread(7, 7, 1.0, 1.5, 0.02))
        nine = ninepacks(a, g)
        assert nine.shape == (th, tw, 9)
        assert_bits(nine[:, :, :3], jobs.oracle_render(a, o, stage=1), "stage 1 of the twined job")
        got = ea.render_rays(g, nine, nchannels=out_n, taps=a.twine_spread)
        assert_bits(got, jobs.oracle_render(a, o, nch=out_n), f"{name} twined, target {tprj}, spread {spread}")


def test_stages_3_and_4_need_a_tap_table():
    o, g = pair("latlon d1 n3")
    a = ea.arguments(ea.SPHERICAL, 200, 100, 360.0, spline_degree=1)
    for stage in (3, 4):
        with pytest.raises(ea.EuError, match="tap table"):
            ea.render(a, g, stage=stage)
    # with taps they differ from the centre ray and from each other
    a = ea.arguments(ea.SPHERICAL, 200, 100, 360.0, spline_degree=1, twine=2)
    r00, r10, r01 = (ea.render(a, g, stage=k) for k in (1, 3, 4))
    assert (r10 != r00).any() and (r01 != r00).any() and (r10 != r01).any()


@pytest.mark.parametrize("general", [False, True])
def test_twining_arbitrary_ninepacks(general, monkeypatch):
    """A CONSISTENCY check of the twine loop against the untwined path that test_rays_of_a_job_give_its_frame pins,
    not an independent oracle: the neighbours of a job's rays are perturbed with a fixed seed, and the expected
    frame is a float32 numpy model of twine_t::eval - dx = in[3..5] - in[0..2], dy = in[6..8] - in[0..2], tap rays
    (r + cx * dx) + cy * dy with cx, cy the taps' offsets times 4, acc = acc + w * q from zero, in the taps' order -
    whose q come from the untwined render_rays at the tap rays."""
    if general:
        monkeypatch.setenv("EU_HIP_KERNEL", "1")
    o, g = pair("latlon d1 n3")
    a = ea.arguments(ea.RECTILINEAR, 129, 97, 90.0, yaw=30, pitch=15, roll=7.5, spline_degree=1)
    r = np.array(job_rays(a, o))
    rng = np.random.default_rng(77)
    nine = np.concatenate([r, r + rng.normal(0, 0.01, r.shape).astype(np.float32),
                           r + rng.normal(0, 0.01, r.shape).astype(np.float32)], axis=2).astype(np.float32)
    taps = ea.make_spread(3, 3, 1.2, 1.0, 0.0)
    assert len(taps) == 9
    f32 = np.float32
    dx, dy = nine[..., 3:6] - nine[..., 0:3], nine[..., 6:9] - nine[..., 0:3]
    acc = np.zeros(r.shape, f32)
    for x, y, w in taps:
        cx, cy = f32(x) * f32(4.0), f32(y) * f32(4.0)
        tap_rays = (nine[..., 0:3] + cx * dx) + cy * dy
        assert tap_rays.dtype == np.float32
        q = ea.render_rays(g, tap_rays)
        acc = acc + f32(w) * q
    assert acc.dtype == np.float32
    assert_bits(ea.render_rays(g, nine, taps=taps), acc, "twine loop against its numpy model")


BAD = [np.nan, np.inf, -np.inf]


def host_predicate(groups, n):
    exe = build_demo()
    words = [f"{int(u):08x}" for u in np.ascontiguousarray(groups, np.float32).view(np.uint32).ravel()]
    r = subprocess.run([exe, "miss", str(n)] + words, capture_output=True, text=True, check=True)
    return [int(v) for v in r.stdout.split()]


@pytest.mark.parametrize("name,out_n,general", [("latlon d3 n3", None, False), ("latlon d3 n3", None, True),
                                                ("cubemap d2", None, False), ("biatan6 d3", None, False),
                                                ("rectilinear lens", None, False), ("latlon d1 n3", 4, False)])
def test_guard_rays(name, out_n, general, monkeypatch):
    """NaN and +-inf in each component, and the null ray, scattered through an ordinary array, give zeros in every
    channel; their neighbours give the oracle's pixels"""
    o, g = pair(name)
    a = ea.arguments(ea.RECTILINEAR, 129, 97, 90.0, yaw=30, pitch=15, roll=7.5, spline_degree=SOURCES[name][5])
    rays, ref = np.array(job_rays(a, o)), np.array(jobs.oracle_render(a, o, nch=out_n))
    patterns = []
    for comp in range(3):
        for v in BAD:
            p = np.array([0.3, -0.2, 0.9], np.float32)
            p[comp] = v
            patterns.append(p)
    patterns += [np.zeros(3, np.float32), np.array([-0.0, 0.0, -0.0], np.float32),
                 np.full(3, np.nan, np.float32), np.array([np.inf, -np.inf, np.nan], np.float32)]
    # before anything is launched: the host-compiled predicate calls every pattern a miss and ordinary rays not
    assert host_predicate(np.stack(patterns), 3) == [1] * len(patterns)
    assert host_predicate(rays[40, 60:70], 3) == [0] * 10
    # positions all over the frame: first and last lanes, the lane-pair tail (x >= 128), neighbouring pixels
    spots = [(0, 0), (0, 63), (0, 64), (0, 127), (0, 128), (96, 128), (50, 65), (50, 66), (51, 65), (13, 1), (77, 100),
             (33, 33), (96, 0)]
    assert len(spots) == len(patterns)
    for (y, x), p in zip(spots, patterns):
        rays[y, x] = p
        ref[y, x] = 0.0
    if general:
        monkeypatch.setenv("EU_HIP_KERNEL", "1")
    got = ea.render_rays(g, rays, nchannels=out_n)
    for y, x in spots:
        assert (jobs.bits(got[y, x]) == 0).all(), f"ray at {(y, x)} is not all +0: {got[y, x]}"
    assert_bits(got, ref, f"{name}: guarded rays among ordinary ones")


@pytest.mark.parametrize("name,out_n", [("latlon d1 n3", None), ("cubemap d2", None), ("rectilinear lens", None),
                                        ("latlon d3 n3", 4)])
def test_guard_ninepacks(name, out_n):
    """any of the nine floats non-finite, or a null centre ray, makes the pixel a miss; a tap ray that overflows
    although the nine floats are finite stays inside the container (no fault) and its neighbours are untouched"""
    o, g = pair(name)
    a = ea.arguments(ea.RECTILINEAR, 129, 97, 90.0, yaw=30, pitch=15, roll=7.5, spline_degree=SOURCES[name][5], twine=2)
    nine, ref = ninepacks(a, g), np.array(jobs.oracle_render(a, o, nch=out_n))
    spots = [(0, k * 14 + (k % 3)) for k in range(9)] + [(96, 128), (40, 64), (41, 64)]
    poisoned = []
    for k in range(9):
        p = nine[spots[k]].copy()
        p[k] = BAD[k % 3]
        poisoned.append(p)
    null_centre = nine[spots[9]].copy()
    null_centre[:3] = 0.0
    all_nan = np.full(9, np.nan, np.float32)
    poisoned += [null_centre, all_nan]
    assert host_predicate(np.stack(poisoned), 9) == [1] * len(poisoned)
    assert host_predicate(nine[40, 60:64], 9) == [0] * 4
    for (y, x), p in zip(spots[:11], poisoned):
        nine[y, x] = p
        ref[y, x] = 0.0
    # finite floats whose tap rays overflow: 3e38 + 4 * x * (-3e38 - 3e38)
    big = np.array([3e38, 3e38, 3e38, -3e38, -3e38, -3e38, 3e38, -3e38, 3e38], np.float32)
    assert host_predicate(big[None], 9) == [0]
    nine[spots[11]] = big
    got = ea.render_rays(g, nine, nchannels=out_n, taps=a.twine_spread)
    keep = np.ones(ref.shape[:2], bool)
    keep[spots[11]] = False
    for y, x in spots[:11]:
        assert (jobs.bits(got[y, x]) == 0).all(), f"ninepack at {(y, x)} is not all +0: {got[y, x]}"
    assert_bits(got[keep], ref[keep], f"{name}: guarded ninepacks among ordinary ones")


def test_no_interference_with_a_staged_job(monkeypatch):
    """a staged job (EU_HIP_R4=1), a render_rays call on another stream, the same job again: the first frame's
    bits, and the launch counter counts the renders alone"""
    import torch
    monkeypatch.setenv("EU_HIP_R4", "1")
    o, g = pair("latlon d3 n3")
    a = ea.arguments(ea.CUBEMAP, 40, 240, 90.0, spline_degree=3)
    L = ea.lib()
    L.eu_hip_launch_count.restype = ctypes.c_ulonglong
    n0 = L.eu_hip_launch_count()
    first = ea.render(a, g)
    n1 = L.eu_hip_launch_count()
    assert n1 > n0
    b = ea.arguments(ea.SPHERICAL, 1100, 12, 360.0, yaw=30, pitch=15, roll=7.5, spline_degree=3)
    rays, ref = job_rays(b, o), jobs.oracle_render(b, o)
    rays_t = torch.from_numpy(np.array(rays)).to("cuda")
    out_t = torch.zeros(ref.shape, dtype=torch.float32, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    ea.render_rays(g, rays_t, out=out_t, stream=stream.cuda_stream)
    assert L.eu_hip_launch_count() == n1
    again = ea.render(a, g)
    assert L.eu_hip_launch_count() > n1
    ea.sync()
    assert_bits(again, first, "the staged job after a render_rays call")
    assert_bits(first, jobs.oracle_render(a, o), "the staged job")
    assert_bits(out_t.cpu().numpy(), ref, "the render_rays call between them")
