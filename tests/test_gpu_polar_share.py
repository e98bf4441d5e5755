"""eu_render5_kernel's second loop with the box table renders a polar tile, its column mirror, its twin on the
opposite polar face and the twin's mirror from ONE run of the ray, the root and the two atan2 chains, where the
bits of the stepper tables say that their angles differ in a sign bit alone (envutil_amd/csrc/eu_polar_groups.h,
eu_render5.h: eu5_tile_bt). EU_HIP_POLAR_SHARE=0 renders every tile from its own. Every case here holds three frames
to one another bit for bit: the oracle's, the default's and EU_HIP_POLAR_SHARE=0's. eu_hip_polar_follower_tiles()
counts the tiles the last launch rendered as followers, and every case holds it to what the host builder says for
the geometry (tests/csrc/polar_groups_demo.cc), so that no case passes without the path it is about."""
import ctypes as C
import os
import subprocess

import pytest

import devout
import envutil_amd as ea
import euo
import jobs
from test_gpu_parity import assert_bits, make_pair
from test_polar_groups import build_demo

pytestmark = pytest.mark.gpu

SWITCHES = ("EU_HIP_R4", "EU_HIP_POLAR_SHARE", "EU_HIP_BOXTAB")


@pytest.fixture(autouse=True)
def staged_everywhere():
    old = {k: os.environ.get(k) for k in SWITCHES}
    os.environ["EU_HIP_R4"] = "1"
    os.environ.pop("EU_HIP_POLAR_SHARE", None)
    os.environ.pop("EU_HIP_BOXTAB", None)
    yield
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


@pytest.fixture(scope="module")
def demo():
    return build_demo()


@pytest.fixture(scope="module")
def latlon():
    return {n: jobs.synth_image(512, 256, n) for n in (3, 4)}


@pytest.fixture(scope="module")
def pairs(latlon):
    """(oracle source, device source) per (channels, degree) of the 512 x 256 lat/lon image, made once"""
    cache = {}

    def get(nch, degree):
        if (nch, degree) not in cache:
            cache[(nch, degree)] = make_pair(euo.SPHERICAL, 512, 256, 360.0, latlon[nch], degree)
        return cache[(nch, degree)]
    return get


def followers():
    f = ea.lib().eu_hip_polar_follower_tiles
    f.restype = C.c_ulonglong
    return int(f())


def host_says(demo, face, yaw, r0, r1, mode):
    out = subprocess.run([demo, str(face), str(yaw), str(r0), str(r1), mode], capture_output=True, text=True, check=True).stdout
    return int(out.split()[1])


def three_ways(demo, a, o, g, nch, face, yaw=0, r0=0, r1=None, ref=None, mode=None, what="", count=True, host=False):
    """the frame with the groups, the frame without, the oracle's: one frame. Returns the follower tiles. Either variant
    is rendered into a guarded device buffer that is all fill word before the call (tests/devout.py): a tile a variant
    skips is not found rendered by the variant before it. host=True: through envutil_amd.render() into host memory;
    count=False: the frame takes several launches, and the query names the last one's list"""
    def render(which):
        if host:
            return ea.render(a, g, nch, r0, r1)
        return devout.rendered(f"{what}: {which}", a, g, nch, r0, r1)
    if ref is None:
        ref = jobs.oracle_render(a, o, row_begin=r0, row_end=r1)
    if mode is None:
        os.environ.pop("EU_HIP_POLAR_SHARE", None)
    else:
        os.environ["EU_HIP_POLAR_SHARE"] = mode
    on = render("groups")
    n_on = followers()
    os.environ["EU_HIP_POLAR_SHARE"] = "0"
    off = render("EU_HIP_POLAR_SHARE=0")
    n_off = followers()
    os.environ.pop("EU_HIP_POLAR_SHARE", None)
    want = host_says(demo, face, yaw, r0, 6 * face if r1 is None else r1, mode or "b")
    print(f"{what}: follower tiles {n_on} (host builder: {want}); EU_HIP_POLAR_SHARE=0: {n_off}")
    assert_bits(on, ref, f"{what}: groups against the oracle")
    assert_bits(off, ref, f"{what}: EU_HIP_POLAR_SHARE=0 against the oracle")
    assert_bits(on, off, f"{what}: groups against EU_HIP_POLAR_SHARE=0")
    assert (n_on == want or not count) and n_off == 0
    return n_on


# 64: positions of four; 96: twins only (six tile columns, a column table that is not antisymmetric bit for bit); 48:
# twins beside the single rows at the middle of the equatorial faces (batches of two columns, three tile columns);
# 41, 33: nothing lines up - entries of one, an odd number of tile columns, a last tile column of one pixel
@pytest.mark.parametrize("face", [64, 96, 48, 41, 33])
@pytest.mark.parametrize("degree", [2, 3])
@pytest.mark.parametrize("nch", [3, 4])
def test_cube_faces(demo, pairs, face, degree, nch):
    o, g = pairs(nch, degree)
    a = ea.arguments(ea.CUBEMAP, face, 6 * face, 90.0, spline_degree=degree)
    n = three_ways(demo, a, o, g, nch, face, what=f"face {face} degree {degree} nch {nch}")
    assert (n > 0) == (face in (64, 96, 48))


def test_cube_face_512(demo, pairs):
    """32 tile columns, 64 positions of four per 16 columns: several positions per wave, every class of tile inside
    groups. A frame of 1024 rows or more goes to the host as several launches (the query names the last one's list), so
    the followers are counted on a row range of 1008 rows that holds 63 of the 64 tile rows of either polar face; the
    whole frame is compared as well"""
    o, g = pairs(3, 3)
    a = ea.arguments(ea.CUBEMAP, 512, 3072, 90.0, spline_degree=3)
    ref = jobs.oracle_render(a, o)
    three_ways(demo, a, o, g, 3, 512, ref=ref, r1=3072, what="face 512, the frame", count=False, host=True)
    three_ways(demo, a, o, g, 3, 512, ref=ref, r1=3072, what="face 512, the frame as one launch into device memory")
    n = three_ways(demo, a, o, g, 3, 512, r0=1032, r1=2040, ref=ref[1032:2040], what="face 512, rows 1032-2040")
    assert n == 3 * 63 * 16


@pytest.mark.parametrize("rows", [(128, 192), (136, 248), (3, 381)])
def test_row_ranges(demo, pairs, rows):
    """the top face alone (mirrors only), both polar faces cut at both ends (the twins whose rows are inside), a range
    off the tile grid (whatever the bits allow)"""
    o, g = pairs(3, 3)
    a = ea.arguments(ea.CUBEMAP, 64, 384, 90.0, spline_degree=3)
    assert three_ways(demo, a, o, g, 3, 64, r0=rows[0], r1=rows[1], what=f"rows {rows}") > 0


@pytest.mark.parametrize("degree", [2, 3])
def test_source_of_a_few_pixels(demo, degree):
    """an 8 x 4 source: every polar tile's box touches the periodic seam or the poles' mirror (not clean: work list)
    or spans the source - members of the work list inside groups"""
    img = jobs.synth_image(8, 4, 3)
    o, g = make_pair(euo.SPHERICAL, 8, 4, 360.0, img, degree)
    a = ea.arguments(ea.CUBEMAP, 64, 384, 90.0, spline_degree=degree)
    assert three_ways(demo, a, o, g, 3, 64, what=f"8x4 source degree {degree}") == 48


def test_strong_minification(demo):
    """a 1024 x 512 source on faces of 16 pixels: every second-loop tile goes to the work list, leaders and followers
    alike (one tile column: no mirrors; the twins are the top and the bottom face and, the two tile rows of a face
    lying about its middle, the halves of the front and of the back face)"""
    img = jobs.synth_image(1024, 512, 3)
    o, g = make_pair(euo.SPHERICAL, 1024, 512, 360.0, img, 3)
    a = ea.arguments(ea.CUBEMAP, 16, 96, 90.0, spline_degree=3)
    assert three_ways(demo, a, o, g, 3, 16, what="minification") == 3


def test_rotated_target(demo, pairs):
    """yaw 30 degrees: A0, B1, B2 are not zeros - entries of one"""
    o, g = pairs(3, 3)
    a = ea.arguments(ea.CUBEMAP, 64, 384, 90.0, spline_degree=3, yaw=30.0)
    assert three_ways(demo, a, o, g, 3, 64, yaw=30, what="yaw 30") == 0


@pytest.mark.parametrize("mode", ["t", "m"])
def test_modes(demo, pairs, mode):
    o, g = pairs(3, 3)
    a = ea.arguments(ea.CUBEMAP, 64, 384, 90.0, spline_degree=3)
    assert three_ways(demo, a, o, g, 3, 64, mode=mode, what=f"mode {mode}") == 32
