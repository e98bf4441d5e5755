"""eu_render5_kernel's second loop (16x8 tiles on rows without a column plan: the polar faces of a cubemap) takes
its tiles' boxes, pass counts and work-list marks from a table that eu5_boxplan_kernel fills when the plans are
built (envutil_amd/csrc/eu_render5.h: eu5_tile_bt, EU5_BT_*). EU_HIP_BOXTAB=0 is the loop that reduces the boxes
per frame. Every case here holds three frames to one another bit for bit: the oracle's, the default's and
EU_HIP_BOXTAB=0's. eu_hip_boxtab_used() / eu_hip_boxtab_tiles() say whether the last launch read a table and how
many tiles it holds, so that no case passes without the path it is about."""
import ctypes as C
import os

import numpy as np
import pytest

import devout
import envutil_amd as ea
import euo
import jobs
from test_gpu_parity import assert_bits, make_pair

pytestmark = pytest.mark.gpu

SWITCHES = ("EU_HIP_R4", "EU_HIP_BOXTAB", "EU_HIP_BOXTAB_MAX_KB")


@pytest.fixture(autouse=True)
def staged_everywhere():
    old = {k: os.environ.get(k) for k in SWITCHES}
    os.environ["EU_HIP_R4"] = "1"
    os.environ.pop("EU_HIP_BOXTAB", None)
    os.environ.pop("EU_HIP_BOXTAB_MAX_KB", None)
    yield
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


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


def table():
    used = ea.lib().eu_hip_boxtab_used
    used.restype = C.c_int
    tiles = ea.lib().eu_hip_boxtab_tiles
    tiles.restype = C.c_ulonglong
    return int(used()), int(tiles())


def three_ways(a, o, g, nch=None, r0=0, r1=None, ref=None, what="", host=False):
    """the frame with the table, the frame without, the oracle's: one frame. Returns the table's tiles. Either variant
    is rendered into a guarded device buffer that is all fill word before the call (tests/devout.py): a tile a variant
    skips is not found rendered by the variant before it. host=True: through envutil_amd.render() into host memory"""
    def render(which):
        if host:
            return ea.render(a, g, nch, r0, r1)
        return devout.rendered(f"{what}: {which}", a, g, nch, r0, r1)
    if ref is None:
        ref = jobs.oracle_render(a, o, row_begin=r0, row_end=r1)
    os.environ.pop("EU_HIP_BOXTAB", None)
    on = render("table")
    used, tiles = table()
    os.environ["EU_HIP_BOXTAB"] = "0"
    off = render("EU_HIP_BOXTAB=0")
    used_off, _ = table()
    os.environ.pop("EU_HIP_BOXTAB", None)
    print(f"{what}: table used {used}, {tiles} tiles; EU_HIP_BOXTAB=0: used {used_off}")
    assert_bits(on, ref, f"{what}: table against the oracle")
    assert_bits(off, ref, f"{what}: EU_HIP_BOXTAB=0 against the oracle")
    assert_bits(on, off, f"{what}: table against EU_HIP_BOXTAB=0")
    assert used == 1 and used_off == 0
    return tiles


def cube_case(pairs, face, degree, nch):
    o, g = pairs(nch, degree)
    a = ea.arguments(ea.CUBEMAP, face, 6 * face, 90.0, spline_degree=degree)
    tiles = three_ways(a, o, g, nch, what=f"face {face} degree {degree} nch {nch}")
    # the two polar faces at the least: 2 * face rows are 2 * face // 8 - 1 whole tile rows or more, of ceil(face / 16) tiles
    assert tiles >= (2 * face // 8 - 1) * ((face + 15) // 16)


# 96: six tile columns, no groups in the first loop; 41: three tile columns (an odd number: the last batch of a row is
# one tile) and face boundaries inside tiles; 33: one pixel in the last tile column (the second pixel of every lane pair
# there lies outside the frame)
@pytest.mark.parametrize("face", [96, 41, 33])
@pytest.mark.parametrize("degree", [2, 3])
@pytest.mark.parametrize("nch", [3, 4])
def test_cube_faces(pairs, face, degree, nch):
    cube_case(pairs, face, degree, nch)


def test_cube_face_512(pairs):
    """32 tile columns and 127 tile rows in the second loop: several batches per wave, every class of tile. A frame of
    1024 rows or more goes to the host as four launches (the query names the last one's table), so the tiles are counted
    on a row range inside the polar faces; the whole frame is compared as well"""
    o, g = pairs(3, 3)
    a = ea.arguments(ea.CUBEMAP, 512, 3072, 90.0, spline_degree=3)
    ref = jobs.oracle_render(a, o)
    three_ways(a, o, g, 3, ref=ref, what="face 512, the frame", host=True)
    three_ways(a, o, g, 3, ref=ref, what="face 512, the frame as one launch into device memory")
    tiles = three_ways(a, o, g, 3, 1024, 2040, ref=ref[1024:2040], what="face 512, rows 1024-2040")
    assert tiles == 127 * 32


@pytest.mark.parametrize("rows", [(0, 6 * 96), (3, 571), (385, 386), (390, 500), (0, 389)])
def test_row_ranges_off_the_tile_grid(pairs, rows):
    """row ranges that start or end off the multiples of 8: the tile grid starts at row_begin, the last tile row
    is cut"""
    o, g = pairs(3, 3)
    a = ea.arguments(ea.CUBEMAP, 96, 6 * 96, 90.0, spline_degree=3)
    three_ways(a, o, g, 3, rows[0], rows[1], what=f"rows {rows}")


@pytest.mark.parametrize("degree", [2, 3])
def test_source_of_a_few_pixels(degree):
    """an 8 x 4 source: every polar tile's box touches the periodic seam or the poles' mirror (not clean: work list)
    or spans the source"""
    img = jobs.synth_image(8, 4, 3)
    o, g = make_pair(euo.SPHERICAL, 8, 4, 360.0, img, degree)
    a = ea.arguments(ea.CUBEMAP, 64, 384, 90.0, spline_degree=degree)
    assert three_ways(a, o, g, 3, what=f"8x4 source degree {degree}") > 0


def test_strong_minification():
    """a 1024 x 512 source on faces of 16 pixels: a tile covers 90 x 45 degrees - 256 x 128 texels, not even a quarter
    fits the slice - so every second-loop tile goes to the (hashed) work list"""
    img = jobs.synth_image(1024, 512, 3)
    o, g = make_pair(euo.SPHERICAL, 1024, 512, 360.0, img, 3)
    a = ea.arguments(ea.CUBEMAP, 16, 96, 90.0, spline_degree=3)
    assert three_ways(a, o, g, 3, what="minification") > 0


def test_rectilinear_target_has_a_table_of_no_tiles(pairs):
    """an upright rectilinear target: every tile row has a column plan and a partner, the second loop is empty"""
    o, g = pairs(3, 3)
    a = ea.arguments(ea.RECTILINEAR, 256, 128, 90.0, spline_degree=3)
    assert three_ways(a, o, g, 3, what="rectilinear 256x128") == 0


def test_plan_reuse_and_eviction(latlon):
    """the same geometry rendered from other pixels reads the cached table; a second geometry replaces it, and the
    first geometry again builds it anew"""
    img2 = np.ascontiguousarray(latlon[3][::-1, ::-1] * 0.5 + 0.125)
    o1, g1 = make_pair(euo.SPHERICAL, 512, 256, 360.0, latlon[3], 3)
    o2, g2 = make_pair(euo.SPHERICAL, 512, 256, 360.0, img2, 3)
    a = ea.arguments(ea.CUBEMAP, 96, 576, 90.0, spline_degree=3)
    b = ea.arguments(ea.CUBEMAP, 41, 246, 90.0, spline_degree=3)
    ref1, ref2 = jobs.oracle_render(a, o1), jobs.oracle_render(a, o2)
    assert (jobs.bits(ref1) != jobs.bits(ref2)).any()
    first = ea.render(a, g1, 3)
    t1 = table()
    second = ea.render(a, g2, 3)          # same geometry, other pixels
    t2 = table()
    assert_bits(first, ref1, "first source")
    assert_bits(second, ref2, "second source, cached table")
    assert t1 == t2 and t1[0] == 1 and t1[1] > 0
    three_ways(b, o1, g1, 3, what="second geometry")
    again = ea.render(a, g2, 3)
    assert table() == t1
    assert_bits(again, ref2, "first geometry again")
    three_ways(a, o1, g1, 3, ref=ref1, what="first geometry, three ways")


def test_refused_table_gives_the_same_frame(pairs):
    """EU_HIP_BOXTAB_MAX_KB=1: 16 tiles at the most - the job gets no table and takes the reducing loop"""
    o, g = pairs(3, 3)
    a = ea.arguments(ea.CUBEMAP, 96, 576, 90.0, spline_degree=3)
    ref = jobs.oracle_render(a, o)
    with_table = ea.render(a, g, 3)
    assert table()[0] == 1
    os.environ["EU_HIP_BOXTAB_MAX_KB"] = "1"
    refused = ea.render(a, g, 3)
    used, tiles = table()
    os.environ["EU_HIP_BOXTAB_MAX_KB"] = "4096"
    allowed = ea.render(a, g, 3)
    assert table()[0] == 1
    print(f"refused: used {used}, tiles {tiles}")
    assert used == 0 and tiles == 0
    assert_bits(refused, ref, "refused table against the oracle")
    assert_bits(with_table, refused, "table against refused table")
    assert_bits(allowed, ref, "table within a raised bound")
