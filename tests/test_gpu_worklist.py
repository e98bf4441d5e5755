"""Jobs whose tiles (nearly) all go to the work list (envutil_amd/csrc/eu_worklist.h): the regime in which the
direct-gather kernel eu_render4d_kernel renders the frame and every writer of the list matters - eu4_tile of
eu_render4s_kernel (cubemap / biatan6 sources) and the three sites of eu_render5_kernel (lat/lon sources: the first
loop's groups on rows with a column plan, the second loop with and without its box table). A launch of 1024 wave
tiles (16 x 8 pixels) or more with every tile listed is where a list sized for `id % 1024` shards was too short for
the hashed ones (tests/test_worklist.py shows that on the CPU); the frame cannot show it, the reader uses the same
slots, so what these cases hold is that the whole regime works: every frame is the oracle's bit for bit, at 1024 tiles
exactly, just above, on ragged frames, at 4096 tiles, in strips whose own tile counts lie below, at and above
multiples of 1024, in bands, after the list's buffer has grown and shrunk, on a caller's stream, and against the
general kernel.

eu_hip_listed_tiles() says how many tiles the last launch pair listed, eu_hip_launch_count() that it was a pair. The
main cases demand that 90 % of the job's tiles were listed. A staged tile is listed when its box of texels does not
fit a wave's LDS slice - for eu_render4s_kernel the box of the 16 x 8 tile against 384 texels, for eu_render5_kernel
the box of a 16 x 16 group (first loop) or of any 8 x 4 quarter (second loop) against 576, and 64 texels in width for
all of them - so the sources are sized for the targets: at 2 texels per pixel a cubic 16 x 8 tile spans 34 x 18 = 612
texels. A 512-face cube under a 360 x 180 degree target of 512 or 528 pixels has 2 to 6 (except in the two tile rows
at the poles, where a tile's pixels crowd onto a few texels of the polar faces: 4.7 % of the tiles); the targets of
1000 and 1024 pixels take a 1024-face cube for the same density. The lat/lon source is 3840 x 1920: the 8 x 4
quarters of the second loop need 4.4 texels per pixel, (7 * 4.4 + 4) * (3 * 4.4 + 4) > 576, which the corners of the
polar faces of a 256-pixel cube face reach from 3840 texels on (at 2560, 81 % of that target's tiles are listed).

Listed tiles as the oracle's source coordinates predict them (the boxes of floor / round of the stage-2 coordinates
against the rules above; a tile with a lane on a scalar fallback is listed on top of these), listed / tiles, cubic and
quadratic: 512 x 256 from a 512-face cubemap 976 and 960 / 1024, from biatan6 1008 and 1008; 528 x 256: 1024 and 1004
/ 1056, biatan6 1046 and 1046; rotated 512 x 256: 1022 and 1018 / 1024, biatan6 1016 and 1012; from the 1024-face
cubes 1000 x 500: 3754 and 3685 / 3969, biatan6 3861 and 3827; 1024 x 512: 3904 and 3824 / 4096, biatan6 4048 and 4000;
512 x 256: 1024 / 1024; the strips of 1024 x 512: 864 / 960, 1024 / 1024, 1144 / 1152, 896 / 1024; the small job of the
reuse test 49 / 195. Lat/lon 3840 x 1920, cubic: cubemap 256 3008 / 3072 (960 / 1024 on the polar faces), spherical
512 x 256 1024 / 1024, rotated 1010 / 1024.

Observed on an MI355X (every case prints the count the device reports), listed / tiles: 512 x 256 from the 512-face
cubemap 976 cubic and 960 quadratic / 1024, with 3 and with 4 channels, from biatan6 1008 and 1008; 528 x 256: cubemap
cubic 1024 / 1056, biatan6 quadratic 1046; rotated: cubemap quadratic 1018 / 1024, biatan6 cubic 1016; 1000 x 500:
cubemap cubic 3754 / 3969, biatan6 quadratic 3827; 1024 x 512: cubemap cubic 3904 / 4096, biatan6 quadratic 4000; no
switch 1024 / 1024; the strips 864 / 960, 1024 / 1024, 1144 / 1152, 896 / 1024; the band parts 1296 / 1408, 1304 / 1344,
1304 / 1344 (3904 together, the whole frame's); the reuse test 49 / 195 each time and 3904 / 4096 on both streams;
lat/lon -> cubemap 256 3008 / 3072 with the box table, without it and without sharing (896 follower tiles with
sharing, 0 without); lat/lon -> spherical 1024 / 1024, rotated 1010 / 1024. Every observed count EQUALS the predicted
one: in these frames no tile is listed for a lane on a scalar fallback alone, and the lowest share of a whole frame
is 93.75 % (960 of 1024; the tile rows at the poles)."""
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

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class env:
    """EU_HIP_* switches for a block (the library reads them on every call); every other one is unset"""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: v for k, v in os.environ.items() if k.startswith("EU_HIP_") and k != "EU_HIP_LIB"}
        for k in self.old:
            del os.environ[k]
        os.environ.update(self.kw)

    def __exit__(self, *exc):
        for k in self.kw:
            os.environ.pop(k, None)
        os.environ.update(self.old)


def tiles_of(width, rows):
    return -(-width // 16) * -(-rows // 8)


def noise_image(w, h, nch, seed):
    """values in (0.05, 0.95), no structure: cheap at the 7 Mpixel these sources have"""
    return np.random.default_rng(seed).random((h, w, nch), dtype=np.float32) * np.float32(0.9) + np.float32(0.05)


def render_once(a, g, nch=None, r0=0, r1=None, band=None, stream=None):
    """The rows as ONE call that renders into device memory (into host memory a frame of 1024 rows or more goes out
    as four launches). Returns the frame, the tiles the call listed and the kernel launches it made."""
    nch = nch or g.fct.nchannels
    t = a.target(nch, r0, r1, 0, band)
    out = np.zeros((t.row_end - t.row_begin, a.out_width, nch), np.float32)
    L = ea.lib()
    dev = C.c_void_p()
    assert L.eu_hip_malloc(C.byref(dev), out.nbytes) == 0
    try:
        srcs = (C.c_void_p * 1)(g.handle)
        n0 = ea.launch_count()
        rc = L.eu_hip_render(C.byref(t), srcs, 1, dev, a.out_width * nch * 4, 1, C.c_void_p(stream) if stream else None)
        assert rc == 0, L.eu_hip_last_error()
        launches = ea.launch_count() - n0
        listed = ea.listed_tiles()
        ea.sync()
        assert L.eu_hip_memcpy_d2h(out.ctypes.data_as(C.c_void_p), dev, out.nbytes) == 0
    finally:
        L.eu_hip_free(dev)
    return out, listed, launches


def all_listed(what, a, o, g, nch=None, share=0.9, ref=None, **switches):
    """one staged launch pair, the oracle's frame, `share` of the tiles listed; returns (frame, listed)"""
    if ref is None:
        ref = jobs.oracle_render(a, o)
    with env(**switches):
        got, listed, launches = render_once(a, g, nch)
    ntiles = tiles_of(a.out_width, got.shape[0])
    print(f"{what}: listed {listed} of {ntiles} tiles, {launches} launches")
    assert_bits(got, ref, what)
    assert launches == 2, "not the staged kernels' launch pair"
    assert share * ntiles <= listed <= ntiles
    return got, listed


# ---- cubemap and biatan6 sources: eu_render4s_kernel, the default path of quadratic and cubic jobs ----------------

@pytest.fixture(scope="module")
def cubes():
    """(oracle source, device source) per (projection, face, channels, degree), made once"""
    cache = {}

    def get(sprj, face, nch, degree):
        k = (sprj, face, nch, degree)
        if k not in cache:
            cache[k] = make_pair(sprj, face, 6 * face, 90.0, noise_image(face, 6 * face, nch, 7 + nch), degree)
        return cache[k]
    yield get
    cache.clear()


S = ea.SPHERICAL
# name: (source face, target arguments); tiles
CUBE_TARGETS = {
    "1024 tiles": (512, dict(projection=S, width=512, height=256, hfov=360.0)),                 # 32 x 32: ntiles = 1024 exactly
    "1056 tiles": (512, dict(projection=S, width=528, height=256, hfov=360.0)),                 # 33 x 32
    "ragged": (1024, dict(projection=S, width=1000, height=500, hfov=360.0)),                   # 63 x 63, both edges cut
    "4096 tiles": (1024, dict(projection=S, width=1024, height=512, hfov=360.0)),               # 64 x 64
    "rotated": (512, dict(projection=S, width=512, height=256, hfov=360.0, yaw=25, pitch=-40, roll=15)),
}


def cube_args(name, degree):
    face, kw = CUBE_TARGETS[name]
    kw = dict(kw)
    return face, ea.arguments(kw.pop("projection"), kw.pop("width"), kw.pop("height"), kw.pop("hfov"), spline_degree=degree, **kw)


@pytest.mark.parametrize("sprj", [euo.CUBEMAP, euo.BIATAN6])
@pytest.mark.parametrize("degree", [2, 3])
@pytest.mark.parametrize("nch", [3, 4])
def test_cube_source_1024_tiles_all_listed(cubes, sprj, degree, nch):
    """ntiles = 1024: the smallest launch in which a list takes a second entry"""
    face, a = cube_args("1024 tiles", degree)
    o, g = cubes(sprj, face, nch, degree)
    all_listed(f"source {sprj} degree {degree} nch {nch}, 512 x 256", a, o, g, nch)


@pytest.mark.parametrize("name,sprj,degree,nch", [
    ("1056 tiles", euo.CUBEMAP, 3, 3), ("1056 tiles", euo.BIATAN6, 2, 4),
    ("ragged", euo.CUBEMAP, 3, 3), ("ragged", euo.BIATAN6, 2, 4),
    ("4096 tiles", euo.CUBEMAP, 3, 3), ("4096 tiles", euo.BIATAN6, 2, 4),
    ("rotated", euo.CUBEMAP, 2, 3), ("rotated", euo.BIATAN6, 3, 4),
])
def test_cube_source_other_frames_all_listed(cubes, name, sprj, degree, nch):
    face, a = cube_args(name, degree)
    o, g = cubes(sprj, face, nch, degree)
    all_listed(f"{name}: source {sprj} face {face} degree {degree} nch {nch}", a, o, g, nch)


def test_no_switch_set_every_tile_listed(cubes):
    """What a caller gets without any EU_HIP_* variable: a cubic job on a cube source is staged by default
    (eu_select.h; tests/csrc/select_demo.cc has this very job), and a 512 x 256 frame of the sphere has 4 texels of
    a 1024-face cube per pixel or more - every one of its 1024 tiles is listed"""
    o, g = cubes(euo.CUBEMAP, 1024, 3, 3)
    a = ea.arguments(S, 512, 256, 360.0, spline_degree=3)
    got, listed = all_listed("no switch, 512 x 256 from a 1024-face cube", a, o, g, 3, share=1.0)
    assert listed == tiles_of(512, 256) == 1024


def test_strips_and_bands_of_4096_tiles(cubes):
    """the 64 x 64-tile frame in strips of 960, 1024, 1152 and 1024 tiles of their own (the tile grid starts at the
    strip's first row: the last two are off the frame's grid), and in three interleaved parts of bands of 8 rows"""
    face, a = cube_args("4096 tiles", 3)
    o, g = cubes(euo.CUBEMAP, face, 3, 3)
    ref = jobs.oracle_render(a, o)
    whole, listed_whole = all_listed("the whole frame", a, o, g, 3, ref=ref)
    parts, listed, ntiles = [], 0, 0
    with env():
        for r0, r1 in ((0, 120), (120, 248), (248, 385), (385, 512)):
            got, n, launches = render_once(a, g, 3, r0, r1)
            print(f"rows {r0}-{r1}: listed {n} of {tiles_of(1024, r1 - r0)} tiles")
            assert launches == 2 and n > tiles_of(1024, r1 - r0) // 2
            parts.append(got)
            listed += n
            ntiles += tiles_of(1024, r1 - r0)
        assert ntiles == 960 + 1024 + 1152 + 1024 and listed >= 0.9 * ntiles
        assert_bits(np.concatenate(parts, 0), ref, "strips")
        assert_bits(np.concatenate(parts, 0), whole, "strips against the whole frame")
        frame = np.zeros_like(ref)
        listed = 0
        for k in range(3):
            rows = ea.band_frame_rows(512, 8, 3, k)
            got, n, launches = render_once(a, g, 3, 0, len(rows), band=(8, 3, k))
            print(f"band part {k}: listed {n} of {tiles_of(1024, len(rows))} tiles")
            assert launches == 2 and tiles_of(1024, len(rows)) >= 1024
            frame[rows] = got
            listed += n
        # bands of 8 rows are the frame's own tile rows: the parts list the frame's tiles between them
        assert listed == listed_whole
        assert_bits(frame, ref, "bands")


# ---- lat/lon sources: eu_render5_kernel, under EU_HIP_R4=1 ----------------------------------------------------------

@pytest.fixture(scope="module")
def latlon():
    pair = make_pair(euo.SPHERICAL, 3840, 1920, 360.0, noise_image(3840, 1920, 3, 3), 3)
    yield pair
    del pair


@pytest.fixture(scope="module")
def cube256(latlon):
    """the upright cubemap target of 16 x 192 tiles and the oracle's frame"""
    a = ea.arguments(ea.CUBEMAP, 256, 1536, 90.0, spline_degree=3)
    return a, jobs.oracle_render(a, latlon[0])


def followers():
    f = ea.lib().eu_hip_share_follower_tiles
    f.restype = C.c_ulonglong
    return int(f())


def boxtab_used():
    return int(ea.lib().eu_hip_boxtab_used())


def test_latlon_upright_cubemap(latlon, cube256):
    """the FAST form: the equatorial faces' rows have column plans (first loop: the groups' writer), the polar faces
    go through the second loop and its box table. A face of 256 pixels is a power of two, so its rows form groups
    (tests/test_gpu_shared_rows.py): with followers this is another path than the EU_HIP_SHARE=0 case below. No
    export counts the rows that have a column plan; that the first loop's writer is reached follows from the share
    alone - the four equatorial faces are 2048 of the 3072 tiles, so 90 % listed cannot come from the polar faces"""
    a, ref = cube256
    all_listed("lat/lon -> cubemap 256", a, *latlon, 3, ref=ref, EU_HIP_R4="1")
    print(f"box table used {boxtab_used()}, follower tiles {followers()}")
    assert boxtab_used() == 1
    assert followers() > 0


def test_latlon_upright_cubemap_without_box_table(latlon, cube256):
    a, ref = cube256
    all_listed("lat/lon -> cubemap 256, EU_HIP_BOXTAB=0", a, *latlon, 3, ref=ref, EU_HIP_R4="1", EU_HIP_BOXTAB="0")
    assert boxtab_used() == 0


def test_latlon_upright_cubemap_without_sharing(latlon, cube256):
    a, ref = cube256
    all_listed("lat/lon -> cubemap 256, EU_HIP_SHARE=0", a, *latlon, 3, ref=ref, EU_HIP_R4="1", EU_HIP_SHARE="0")
    assert followers() == 0 and boxtab_used() == 1


@pytest.mark.parametrize("ypr", [(0, 0, 0), (20, 30, 10)])
def test_latlon_spherical_target(latlon, ypr):
    """a 360 x 180 degree target of 1024 tiles: 'ray = B * c0 + C * c1 + A', no column plan, not the FAST form"""
    a = ea.arguments(S, 512, 256, 360.0, yaw=ypr[0], pitch=ypr[1], roll=ypr[2], spline_degree=3)
    all_listed(f"lat/lon -> spherical 512 x 256 ypr {ypr}", a, *latlon, 3, EU_HIP_R4="1")
    assert boxtab_used() == 0 and followers() == 0


# ---- the general kernel renders the same frames ---------------------------------------------------------------------

def test_general_kernel_agrees(cubes, latlon, cube256):
    face, a = cube_args("4096 tiles", 3)
    o, g = cubes(euo.CUBEMAP, face, 3, 3)
    with env():
        staged, listed, launches = render_once(a, g, 3)
    assert launches == 2 and listed >= 0.9 * 4096
    with env(EU_HIP_KERNEL="1"):
        general, _, launches = render_once(a, g, 3)
    assert launches == 1
    assert_bits(staged, general, "cube source: staged against EU_HIP_KERNEL=1")
    a, _ = cube256
    with env(EU_HIP_R4="1"):
        staged, listed, launches = render_once(a, latlon[1], 3)
    assert launches == 2 and listed >= 0.9 * tiles_of(256, 1536)
    with env(EU_HIP_KERNEL="1", EU_HIP_R4="1"):
        general, _, launches = render_once(a, latlon[1], 3)
    assert launches == 1
    assert_bits(staged, general, "lat/lon source: staged against EU_HIP_KERNEL=1")


# ---- the list's buffer grows, is reused by a smaller job, and serves another stream ---------------------------------

def reuse_sequence():
    """run in a process of its own (test_buffer_grows_and_is_reused): the first staged job of the process is small"""
    import torch
    face = 1024
    o, g = make_pair(euo.CUBEMAP, face, 6 * face, 90.0, noise_image(face, 6 * face, 3, 10), 3)
    small = ea.arguments(ea.RECTILINEAR, 200, 120, 20.0, yaw=40, spline_degree=3)      # 195 tiles, a face seam through them
    big = ea.arguments(S, 1024, 512, 360.0, spline_degree=3)                           # 4096 tiles
    ref_small, ref_big = jobs.oracle_render(small, o), jobs.oracle_render(big, o)
    with env():
        assert ea.listed_tiles() == 0
        got, first, launches = render_once(small, g, 3)
        assert launches == 2 and 0 < first < 195 // 2, first
        assert_bits(got, ref_small, "small job, first")
        got, n_big, launches = render_once(big, g, 3)
        assert launches == 2 and n_big >= 0.9 * 4096, n_big
        assert_bits(got, ref_big, "4096 tiles behind the small job: the buffer grew")
        got, again, _ = render_once(small, g, 3)
        assert_bits(got, ref_small, "small job behind the large one")
        assert again == first, (first, again)
        stream = torch.cuda.Stream(device=torch.device("cuda", 0))
        got, n_stream, launches = render_once(big, g, 3, stream=stream.cuda_stream)
        assert launches == 2 and n_stream == n_big, (n_big, n_stream)
        assert_bits(got, ref_big, "4096 tiles on a caller's stream")
        got, last, _ = render_once(small, g, 3)
        assert_bits(got, ref_small, "small job on the library's stream behind the caller's")
        assert last == first
    print(f"reuse ok: small {first} of 195, large {n_big} of 4096")


def test_buffer_grows_and_is_reused():
    """small job, 4096 all-listed tiles, small job, the 4096 tiles on a second stream, small job: every frame the
    oracle's, and the small job lists the same tiles each time - the lists were emptied and the grown buffer's
    header cleared. A process of its own, so that the buffer starts small"""
    code = "import sys; sys.path.insert(0, 'tests'); import test_gpu_worklist as t; t.reuse_sequence()"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "reuse ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
