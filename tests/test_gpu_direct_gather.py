"""The direct-gather kernel eu_render4d_kernel where it renders (nearly) the whole frame, and the two sets of
work-list counters it alternates between (envutil_amd/csrc/eu_worklist.h).

The first three groups are frames whose pixels' windows lie far apart - the regime around a pole, where nothing
coalesces across pixels: a 2048 x 1024 lat/lon source under an upright 32-pixel cubemap (16 texels per pixel) and
under a 40 x 21 spherical target (51 texels per pixel; ragged tiles in both directions, a last tile row with pixels
outside the frame, the seam and both poles inside), 128-face cube sources under a 128 x 64 spherical target (4 texels
per pixel), and a lat/lon source of 120 x 60 degrees under a target that looks past its edges. Every frame is the
oracle's bit for bit, every call is one launch pair.

The listed share. For each frame the test predicts, from the oracle's stage-2 coordinates, tiles that MUST be listed,
and asserts predicted <= listed <= tiles and - a condition on the inputs, not a measurement - predicted >= 0.9 tiles.
The prediction is a lower bound by construction:
  * cube sources (eu4_tile of eu_render4s_kernel): a tile is listed when the box of the base positions of its hitting
    pixels, plus the spline's order, is wider than 64 texels or holds more than 384. That is the kernel's own rule;
    a tile with a lane on a scalar fallback is listed on top of it.
  * lat/lon sources (eu_render5_kernel): a tile is listed when the smallest piece the kernel would stage does not fit
    64 texels in width or 576 texels. Whatever shape that piece has (a 16 x 16 group, a tile, its halves, its
    quarters), it contains whole aligned blocks of 8 x 2 pixels; the prediction lists a tile when one such block
    does not fit. A longitude is taken modulo the source's width in two ways (into [0, w) and into [-w/2, w/2)) and
    a block counts only if it is too wide in both: the periodic gate's own fold is one of the two.
Predicted / tiles as computed on the CPU, the same for both degrees: cubemap 32 48 / 48 (rows 3-19 4 / 4, rows 5-30 and
161-192 8 / 8, the band parts 16 / 16 each), spherical 40 x 21 9 / 9 (rows 2-21 too); cube sources 64 / 64 upright and
rotated, cubemap and biatan6; the 120-degree source under 80 x 40 24 / 25. The jobs of the last test: X 192 / 192,
Y 410 / 1024, the 4096-tile job 0 / 4096 (2 texels per pixel: what it lists is the device's to say), the job that
lists nothing 0 / 1024 - and 192 / 192 for the upright 64-pixel cubemap, which therefore cannot be that job.

The last test runs in a process of its own, so that the list's buffer starts small, and walks the two sets: the same
job five times in a row (both sets used, both emptied by the pair before), a job that lists nothing, jobs on a caller's
stream and on the library's behind it, a job after the buffer has grown. The job that lists nothing is a 512 x 256
rectilinear view of the equator (0.7 texels per pixel, FAST form, away from the seam): an upright cubemap of a
full-sphere source always lists the tiles that hold a pole (the four tiles around it span 90 degrees of longitude
each - 512 texels of this source), whatever its size."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import envutil_amd as ea
import euo
import jobs
from test_gpu_parity import assert_bits, make_pair
from test_gpu_worklist import env, noise_image, render_once, tiles_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = ea.SPHERICAL
SRC_W, SRC_H = 2048, 1024


# ---- the prediction -------------------------------------------------------------------------------------------------

def split(c, degree):
    """the base position of a coordinate: floor for odd degrees, roundf (halves away from zero) for even ones"""
    c = c.astype(np.float64)
    return np.floor(c) if degree & 1 else np.copysign(np.floor(np.abs(c) + 0.5), c)


def too_large(ix, iy, hit, order, texels):
    """per block (first axis): the box of the hitting pixels' base positions does not fit"""
    big = np.iinfo(np.int64).max
    mnx = np.where(hit, ix, big).min(1); mxx = np.where(hit, ix, -big).max(1)
    mny = np.where(hit, iy, big).min(1); mxy = np.where(hit, iy, -big).max(1)
    any_hit = hit.any(1)
    bw, bh = mxx - mnx + order, mxy - mny + order
    return any_hit & ((bw > 64) | (bh > texels) | (bw * bh > texels))


def blocks(a, bh, bw):
    """(rows, width) -> (tiles_y, tiles_x, blocks per tile, pixels per block), 16 x 8 tiles from the first row; the
    frame is padded (with misses, by the caller's choice of `a`) to whole tiles"""
    h, w = a.shape
    ty, tx = -(-h // 8), -(-w // 16)
    p = np.zeros((ty * 8, tx * 16), a.dtype)
    p[:h, :w] = a
    return p.reshape(ty, 8 // bh, bh, tx, 16 // bw, bw).transpose(0, 3, 1, 4, 2, 5).reshape(ty, tx, (8 // bh) * (16 // bw), bh * bw)


def predict_listed(crd, degree, cube, period=None):
    """tiles that must be listed (see the module's docstring). crd: stage-2 coordinates of exactly the rows of the
    call; period: the width of a full-circle lat/lon source"""
    order = degree + 1
    hit = crd[:, :, 2] >= 0
    iy = split(crd[:, :, 1], degree).astype(np.int64)
    bh, bw, texels = (8, 16, 384) if cube else (2, 8, 576)
    hb = blocks(hit, bh, bw)
    yb = blocks(iy, bh, bw)
    sx = crd[:, :, 0].astype(np.float64)
    variants = [sx] if period is None else [np.mod(sx, period), np.mod(sx + period / 2, period) - period / 2]
    bad = None
    for v in variants:
        xb = blocks(split(v, degree).astype(np.int64), bh, bw)
        t = too_large(xb.reshape(-1, bh * bw), yb.reshape(-1, bh * bw), hb.reshape(-1, bh * bw), order, texels).reshape(hb.shape[:3])
        bad = t if bad is None else bad & t
    return int(bad.any(2).sum())


def check(what, a, o, g, nch, cube, period=None, r0=0, r1=None, band=None, ref=None, crd=None, **switches):
    """one call: the oracle's frame, one launch pair, predicted <= listed <= tiles, predicted >= 0.9 tiles"""
    if ref is None:
        ref = jobs.oracle_render(a, o)
    if crd is None:
        crd = jobs.oracle_render(a, o, stage=2)
    rows = np.arange(a.height)[r0:r1] if band is None else ea.band_frame_rows(a.height, *band)[r0:r1]
    with env(**switches):
        got, listed, launches = render_once(a, g, nch, r0, r1 if band is None else len(rows), band)
    ntiles = tiles_of(a.out_width, len(rows))
    predicted = predict_listed(crd[rows], o.degree, cube, period)
    print(f"{what}: listed {listed}, predicted {predicted}, of {ntiles} tiles, {launches} launches")
    assert_bits(got, ref[rows], what)
    assert launches == 2, "not the staged kernels' launch pair"
    assert predicted >= 0.9 * ntiles, "the inputs do not put 90 % of the tiles on the list"
    assert predicted <= listed <= ntiles
    return got


# ---- 1. disjoint windows: a lat/lon source at 16 and 51 texels per pixel --------------------------------------------

@pytest.fixture(scope="module")
def latlon():
    """(oracle source, device source) per (channels, degree), made once"""
    cache = {}

    def get(nch, degree):
        if (nch, degree) not in cache:
            cache[(nch, degree)] = make_pair(euo.SPHERICAL, SRC_W, SRC_H, 360.0, noise_image(SRC_W, SRC_H, nch, 20 + nch), degree)
        return cache[(nch, degree)]
    yield get
    cache.clear()


def pole_target(name, degree):
    if name == "cubemap 32":
        return ea.arguments(ea.CUBEMAP, 32, 192, 90.0, spline_degree=degree)
    return ea.arguments(S, 40, 21, 360.0, spline_degree=degree)


@pytest.mark.parametrize("name", ["cubemap 32", "spherical 40 x 21"])
@pytest.mark.parametrize("degree", [2, 3])
@pytest.mark.parametrize("nch", [3, 4])
def test_pole_regime(latlon, name, degree, nch):
    o, g = latlon(nch, degree)
    check(f"{name}, degree {degree}, {nch} channels", pole_target(name, degree), o, g, nch, False, SRC_W, EU_HIP_R4="1")


@pytest.mark.parametrize("degree", [2, 3])
def test_pole_regime_row_ranges_and_bands(latlon, degree):
    """rows that start and end off the multiples of 8 (the tile grid starts at the call's first row), and the frame
    in three interleaved parts of bands of 8 rows"""
    o, g = latlon(3, degree)
    a = pole_target("cubemap 32", degree)
    ref, crd = jobs.oracle_render(a, o), jobs.oracle_render(a, o, stage=2)
    for r0, r1 in ((3, 19), (5, 30), (161, 192)):
        check(f"cubemap 32 rows {r0}-{r1}, degree {degree}", a, o, g, 3, False, SRC_W, r0=r0, r1=r1, ref=ref, crd=crd, EU_HIP_R4="1")
    frame = np.zeros_like(ref)
    for k in range(3):
        got = check(f"cubemap 32 band part {k}, degree {degree}", a, o, g, 3, False, SRC_W, band=(8, 3, k), ref=ref, crd=crd,
                    EU_HIP_R4="1")
        frame[ea.band_frame_rows(a.height, 8, 3, k)] = got
    assert_bits(frame, ref, "the band parts together")
    a = pole_target("spherical 40 x 21", degree)
    check(f"spherical 40 x 21 rows 2-21, degree {degree}", a, o, g, 3, False, SRC_W, r0=2, r1=21, EU_HIP_R4="1")


# ---- 2. cube sources: eu_render4s_kernel in front -------------------------------------------------------------------

@pytest.fixture(scope="module")
def cubes():
    cache = {}

    def get(sprj, degree):
        if (sprj, degree) not in cache:
            cache[(sprj, degree)] = make_pair(sprj, 128, 768, 90.0, noise_image(128, 768, 3, 31), degree)
        return cache[(sprj, degree)]
    yield get
    cache.clear()


@pytest.mark.parametrize("sprj", [euo.CUBEMAP, euo.BIATAN6])
@pytest.mark.parametrize("degree", [2, 3])
@pytest.mark.parametrize("ypr", [(0, 0, 0), (25, -40, 15)])
def test_cube_sources(cubes, sprj, degree, ypr):
    o, g = cubes(sprj, degree)
    a = ea.arguments(S, 128, 64, 360.0, yaw=ypr[0], pitch=ypr[1], roll=ypr[2], spline_degree=degree)
    check(f"source {sprj} face 128, degree {degree}, ypr {ypr}", a, o, g, 3, True)


# ---- 3. a source that can be missed ---------------------------------------------------------------------------------

@pytest.mark.parametrize("degree", [2, 3])
def test_source_that_is_missed(degree):
    """120 x 60 degrees of lat/lon under a target of 150 x 75: the pixels past the source's edges are zeros, the
    others the oracle's, and every tile has pixels of both kinds or hits alone"""
    o, g = make_pair(euo.SPHERICAL, 1024, 512, 120.0, noise_image(1024, 512, 3, 41), degree)
    a = ea.arguments(S, 80, 40, 150.0, yaw=5, pitch=3, roll=10, spline_degree=degree)
    crd = jobs.oracle_render(a, o, stage=2)
    hit = crd[:, :, 2] >= 0
    assert 0.3 < hit.mean() < 0.9, hit.mean()
    got = check(f"lat/lon 120 degrees, degree {degree}", a, o, g, 3, False, None, crd=crd, EU_HIP_R4="1")
    assert (got[~hit] == 0).all() and (got[hit] != 0).any()


# ---- 5. the two sets of counters ------------------------------------------------------------------------------------

def set_sequence():
    """run in a process of its own (test_two_header_sets): the first staged job of the process is small"""
    import torch
    o, g = make_pair(euo.SPHERICAL, SRC_W, SRC_H, 360.0, noise_image(SRC_W, SRC_H, 3, 23), 3)
    jobs_ = {
        "X": ea.arguments(ea.CUBEMAP, 64, 384, 90.0, spline_degree=3),                       # 192 tiles, 4 to 8 texels per pixel
        "Y": ea.arguments(S, 512, 256, 360.0, yaw=20, pitch=30, roll=10, spline_degree=3),   # 1024 tiles, 4 texels per pixel
        "none": ea.arguments(ea.RECTILINEAR, 512, 256, 60.0, spline_degree=3),               # 1024 tiles, 0.7 texels per pixel
        "big": ea.arguments(S, 1024, 512, 360.0, spline_degree=3),                           # 4096 tiles
    }
    ref = {k: jobs.oracle_render(a, o) for k, a in jobs_.items()}
    lower = {k: predict_listed(jobs.oracle_render(a, o, stage=2), 3, False, SRC_W) for k, a in jobs_.items()}
    print("predicted:", lower)
    assert lower["none"] == 0 and 0 < lower["X"] and tiles_of(64, 384) < lower["Y"]
    seen = {}

    def run(k, what, stream=None):
        a = jobs_[k]
        got, listed, launches = render_once(a, g, 3, stream=stream)
        print(f"{what}: {k} listed {listed} of {tiles_of(a.out_width, a.height)}")
        assert_bits(got, ref[k], what)
        assert launches == 2, what
        assert lower[k] <= listed <= tiles_of(a.out_width, a.height), (what, listed)
        assert seen.setdefault(k, listed) == listed, (what, seen[k], listed)
        return listed

    with env(EU_HIP_R4="1"):
        assert ea.listed_tiles() == 0
        x = run("X", "the first job of the process")
        y = run("Y", "another geometry behind it")
        assert 0 < x < y
        for i in range(5):
            run("X", f"X, time {i + 1} of five in a row")
        assert run("none", "a job that lists nothing") == 0
        run("X", "X behind the job that lists nothing")
        stream = torch.cuda.Stream(device=torch.device("cuda", 0))
        run("Y", "Y on a caller's stream", stream=stream.cuda_stream)
        run("X", "X on the library's stream behind the caller's")
        run("big", "4096 tiles: the buffer grows")
        run("Y", "Y after the buffer has grown")
        run("X", "X after the buffer has grown")
    print(f"sets ok: X {x}, Y {y}")


def test_two_header_sets():
    code = "import sys; sys.path.insert(0, 'tests'); import test_gpu_direct_gather as t; t.set_sequence()"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "sets ok" in r.stdout, r.stdout[-3000:] + r.stderr[-4000:]
