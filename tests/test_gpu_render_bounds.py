"""Where eu_hip_render's kernels write. Every case renders into a guarded, padded buffer of the caller's on the device
(tests/devout.py: all fill word 0x7FA5A5A5 before the call) and holds three things through devout.held: (a) the frame is
the oracle's bit for bit, (b) no word of it is still the fill word - misses and holes are written as zeros -, (c) no
word of the guards, the lead or the rows' padding was touched. Every case runs with a row padding of 0, 1 and 5 words
and with its first row 0 and 1 words off the guard's end (a padding of 1 word puts every second row of 3- and 4-channel
pixels off the 8- and 16-byte boundaries). Each case prints what it found outside the rows and the "this path ran"
counters (launches of the single-facet path, listed tiles, first-loop and second-loop followers, box table), and
asserts those that name its path, so that no case passes on another kernel.

The kernels in envutil_amd/csrc that store pixels for eu_hip_render, and the case that holds each:

  eu_render_kernel              test_general_kernels (EU_HIP_KERNEL=1 with EU_HIP_DIRECT=1; the twined, the translated
                                and the --mask_for job without it too), test_stage_outputs
  eu_render_lds_kernel          test_general_kernels (the job of mostly misses under EU_HIP_KERNEL=1 alone: neither twined
                                nor stepped generically nor painted)
  eu_render2_kernel             test_packed_kernels (EU_HIP_R4=0; EU_HIP_HYBRID=0 and every width below 64), twined too
  eu_render3_kernel             test_packed_kernels (EU_HIP_R4=0 EU_HIP_HYBRID=2, the targets rolled by 90 degrees that are
                                64 pixels wide or wider: source rows run across target rows, the tile layout)
  eu_render4s_kernel            test_staged_cubemap_source
  eu_render4d_kernel            test_work_list (every case asserts listed tiles)
  eu_render5_kernel, first loop             test_staged_cube_faces, test_staged_row_ranges, test_adjacent_strips
                                            (faces 64 and 48: followers asserted; EU_HIP_SHARE=0 without them)
  eu_render5_kernel, reducing second loop   the same under EU_HIP_BOXTAB=0, test_offset_limit at a stride of 2^25 floats,
                                            and its form without the FAST profile: test_bands under EU_HIP_R4=1
  eu_render5_kernel, box-table second loop  test_staged_cube_faces, test_staged_row_ranges, test_staged_rotated_target,
                                            test_offset_limit at a stride of 2^25 - 1 floats (eu_hip_boxtab_used() == 1)
  eu_render_multi_kernel        test_multi_facet, test_crops, test_bands, test_callers_stream
  to_screen_kernel              test_tethered
  encode_kernel                 test_samples_and_quads (8 and 16 bit)
  rgbe_encode_kernel            test_samples_and_quads (quads)

tests/test_gpu_encode.py and tests/test_gpu_rgbe.py check the padding behind the rows of a device buffer for
eu_hip_render_samples and eu_hip_render_rgbe (test_render_samples_device_out_on_a_stream,
test_render_rgbe_device_out_on_a_stream) but neither the memory in front of the first row nor behind the last, so those
two entries have their cases here as well."""
import ctypes as C
import os

import numpy as np
import pytest

import devout
import envutil_amd as ea
import euo
import jobs
import rgbe_model as rm
from test_gpu_encode import want_bytes
from test_gpu_parity import facet_set, make_pair

pytestmark = pytest.mark.gpu

SWITCHES = ("EU_HIP_R4", "EU_HIP_KERNEL", "EU_HIP_DIRECT", "EU_HIP_HYBRID", "EU_HIP_BOXTAB", "EU_HIP_BOXTAB_MAX_KB",
            "EU_HIP_POLAR_SHARE", "EU_HIP_SHARE", "EU_HIP_COLPLAN", "EU_HIP_COLMAJOR", "EU_HIP_REJ")
PADS, LEADS = (0, 1, 5), (0, 1)


@pytest.fixture(autouse=True)
def switches_unset():
    old = {k: os.environ.pop(k, None) for k in SWITCHES}
    yield
    for k, v in old.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


def use(sw):
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(sw)


def name(sw):
    return " ".join(f"{k[7:]}={v}" for k, v in sw.items()) or "default"


def probes(n0):
    L = ea.lib()
    L.eu_hip_share_follower_tiles.restype = C.c_ulonglong
    L.eu_hip_polar_follower_tiles.restype = C.c_ulonglong
    L.eu_hip_boxtab_used.restype = C.c_int
    return dict(launches=ea.launch_count() - n0, listed=ea.listed_tiles(), share=int(L.eu_hip_share_follower_tiles()),
                polar=int(L.eu_hip_polar_follower_tiles()), boxtab=int(L.eu_hip_boxtab_used()))


def paddings(what, a, o, g, nch, ref, expect=None, **kw):
    """the case under every padding and lead; expect: probe name -> value, or a predicate of the value"""
    for pad in PADS:
        for lead in LEADS:
            n0 = ea.launch_count()
            w = f"{what}, pad {pad} lead {lead}"
            _, seen = devout.held(w, a, o, g, nch, ref=ref, probes=lambda: probes(n0), pad=pad, lead=lead, **kw)
            for k, v in (expect or {}).items():
                assert v(seen[k]) if callable(v) else seen[k] == v, f"{w}: probe {k} is {seen[k]}: not the path this case is about"


_kept = {}


def once(key, make):
    """sources and oracle frames are made once and shared, unchanged, between the cases that need them"""
    if key not in _kept:
        _kept[key] = make()
    return _kept[key]


def latlon_pair(nch, degree, w=512, h=256):
    return once(("latlon", w, h, nch, degree),
                lambda: make_pair(euo.SPHERICAL, w, h, 360.0, jobs.synth_image(w, h, nch), degree))


def cube_args(face, degree, **kw):
    return ea.arguments(ea.CUBEMAP, face, 6 * face, 90.0, spline_degree=degree, **kw)


def cube_ref(face, degree, nch, yaw=0.0):
    o, _ = latlon_pair(nch, degree)
    return once(("cube ref", face, degree, nch, yaw), lambda: jobs.oracle_render(cube_args(face, degree, yaw=yaw), o))


# ---- the staged kernels on a lat/lon source: eu_render5_kernel, both loops ----------------------------------------
STAGED = [{}, {"EU_HIP_POLAR_SHARE": "0"}, {"EU_HIP_BOXTAB": "0"}, {"EU_HIP_SHARE": "0"}, {"EU_HIP_COLPLAN": "0"}]


def staged_expect(sw, face, whole=True, polar=True):
    """what the counters must say: the staged pair ran; the box table was read unless switched off; followers where
    the existing tests of these geometries find them (tests/test_gpu_shared_rows.py, tests/test_gpu_polar_share.py)"""
    e = {"launches": 2, "boxtab": 0 if sw.get("EU_HIP_BOXTAB") == "0" else 1}
    colplans = "EU_HIP_COLPLAN" not in sw
    if sw.get("EU_HIP_SHARE") == "0" or not colplans:          # the first loop renders the rows with a column plan
        e["share"] = 0
    elif whole and face == 64:
        e["share"] = lambda n: n > 0
    if sw.get("EU_HIP_POLAR_SHARE") == "0" or sw.get("EU_HIP_BOXTAB") == "0":
        e["polar"] = 0
    elif polar and face in (64, 48) and colplans:
        e["polar"] = lambda n: n > 0
    return e


# 64: positions of four; 48: twins beside single rows, three tile columns; 41: an odd number of tile columns, face
# edges inside tiles; 33: one pixel in the last tile column
@pytest.mark.parametrize("sw", STAGED, ids=name)
@pytest.mark.parametrize("nch", [3, 4])
@pytest.mark.parametrize("face,degree", [(64, 3), (64, 2), (48, 3), (41, 3), (33, 3)])
def test_staged_cube_faces(face, degree, nch, sw):
    o, g = latlon_pair(nch, degree)
    ref = cube_ref(face, degree, nch)
    use(dict(sw, EU_HIP_R4="1"))
    paddings(f"face {face} degree {degree} nch {nch} {name(sw)}", cube_args(face, degree), o, g, nch, ref,
             staged_expect(sw, face))


# the guard in front of the first row is the point: a range off the tile grid, both polar faces cut at both ends, one
# tile row of the top face
@pytest.mark.parametrize("sw", STAGED, ids=name)
@pytest.mark.parametrize("nch", [3, 4])
@pytest.mark.parametrize("rows", [(3, 381), (136, 248), (128, 136)])
def test_staged_row_ranges(rows, nch, sw):
    o, g = latlon_pair(nch, 3)
    ref = cube_ref(64, 3, nch)[rows[0]:rows[1]]
    use(dict(sw, EU_HIP_R4="1"))
    paddings(f"face 64 rows {rows} nch {nch} {name(sw)}", cube_args(64, 3), o, g, nch, ref,
             staged_expect(sw, 64, whole=False, polar=rows != (128, 136)), row_begin=rows[0], row_end=rows[1])


@pytest.mark.parametrize("sw", STAGED[:3], ids=name)
@pytest.mark.parametrize("nch", [3, 4])
def test_staged_rotated_target(nch, sw):
    """yaw 30 degrees: the polar faces' groups are entries of one (no followers) in the box-table loop"""
    o, g = latlon_pair(nch, 3)
    use(dict(sw, EU_HIP_R4="1"))
    paddings(f"face 64 yaw 30 nch {nch} {name(sw)}", cube_args(64, 3, yaw=30.0), o, g, nch, cube_ref(64, 3, nch, 30.0),
             {"launches": 2, "polar": 0, "boxtab": 0 if sw.get("EU_HIP_BOXTAB") == "0" else 1})


# ---- the staged kernel on a cubemap source: eu_render4s_kernel ------------------------------------------------------
@pytest.mark.parametrize("nch", [3, 4])
@pytest.mark.parametrize("target", ["spherical", "rectilinear"])
def test_staged_cubemap_source(target, nch):
    o, g = once(("cube source", nch), lambda: make_pair(euo.CUBEMAP, 64, 384, 90.0, jobs.synth_cubefaces(64, nch), 3))
    a = ea.arguments(ea.SPHERICAL, 200, 100, 360.0, spline_degree=3) if target == "spherical" else \
        ea.arguments(ea.RECTILINEAR, 150, 77, 90.0, yaw=30, pitch=15, roll=7.5, spline_degree=3)
    paddings(f"cube 64 onto {target} nch {nch}", a, o, g, nch, jobs.oracle_render(a, o), {"launches": 2})


# ---- the work list: eu_render4d_kernel ------------------------------------------------------------------------------
@pytest.mark.parametrize("sw", STAGED[:3], ids=name)
@pytest.mark.parametrize("source,face", [((8, 4), 64), ((1024, 512), 16)])
def test_work_list(source, face, sw):
    """an 8 x 4 source: every polar tile's box touches the seam or the poles' mirror; a 1024 x 512 source on faces of
    16 pixels: no tile's box fits the slice"""
    o, g = latlon_pair(3, 3, *source)
    a = cube_args(face, 3)
    ref = once(("work list", source, face), lambda: jobs.oracle_render(a, o))
    use(dict(sw, EU_HIP_R4="1"))
    paddings(f"{source} onto face {face} {name(sw)}", a, o, g, 3, ref, {"launches": 2, "listed": lambda n: n > 0})


# ---- the packed kernels: eu_render2_kernel, eu_render3_kernel -------------------------------------------------------
PACKED_TARGETS = [(ea.RECTILINEAR, w, 5, 90.0) for w in (1, 3, 17, 65, 129, 513)] + [(ea.CUBEMAP, 65, 390, 90.0)]


@pytest.mark.parametrize("hybrid", ["2", "0"])
@pytest.mark.parametrize("degree", [1, 3])
@pytest.mark.parametrize("nch", [1, 3, 4])
def test_packed_kernels(nch, degree, hybrid):
    """rolled by 90 degrees a pixel step along a target row is a step in latitude: under EU_HIP_HYBRID=2 the targets
    of 64 pixels and more take the tile layout (eu_render3_kernel), the narrower ones and EU_HIP_HYBRID=0 the strips"""
    o, g = latlon_pair(nch, degree, 256, 128)
    for tprj, tw, th, thfov in PACKED_TARGETS:
        for twine in ((0, 2) if tw in (17, 129) else (0,)):
            a = ea.arguments(tprj, tw, th, thfov, yaw=20, pitch=10, roll=90, spline_degree=degree, twine=twine)
            ref = once(("packed", tprj, tw, nch, degree, twine), lambda: jobs.oracle_render(a, o))
            use({"EU_HIP_R4": "0", "EU_HIP_HYBRID": hybrid})
            paddings(f"packed {tw} x {th} nch {nch} degree {degree} twine {twine} HYBRID={hybrid}", a, o, g, nch, ref,
                     {"launches": lambda n: n >= 1})


# ---- the general kernels: eu_render_kernel, eu_render_lds_kernel ----------------------------------------------------
def general_jobs():
    def rect(twine):
        o, g = make_pair(euo.RECTILINEAR, 200, 150, 80.0, jobs.synth_image(200, 150, 3, seed=99), 3)
        return ea.arguments(ea.SPHERICAL, 300, 150, 360.0, spline_degree=3, twine=twine), o, g

    def special(**kw):
        img = jobs.synth_image(64, 48, 3)
        o = jobs.OracleSource(euo.RECTILINEAR, 64, 48, 70.0, img, 1, **kw)
        g = ea.Source.adopt(ea.facet_spec(ea.RECTILINEAR, 64, 48, 70.0, **kw), o.container, 1, o.bc[0], o.bc[1])
        return ea.arguments(ea.SPHERICAL, 120, 60, 360.0, spline_degree=1), o, g
    return {"misses": rect(0), "twined": rect(2), "translated": special(translation=dict(x=0.1, z=0.05)),
            "mask_for": special(masked=1)}


@pytest.mark.parametrize("sw", [{"EU_HIP_KERNEL": "1"}, {"EU_HIP_KERNEL": "1", "EU_HIP_DIRECT": "1"}], ids=name)
@pytest.mark.parametrize("job", ["misses", "twined", "translated", "mask_for"])
def test_general_kernels(job, sw):
    a, o, g = once("general jobs", general_jobs)[job]
    ref = once(("general", job), lambda: jobs.oracle_render(a, o))
    if job == "misses":
        assert (ref == 0).all(-1).mean() > 0.5 and (ref != 0).any()        # a 80 degree source under the whole sphere
    use(sw)
    paddings(f"general, {job}, {name(sw)}", a, o, g, 3, ref, {"launches": 1})


# ---- several facets: eu_render_multi_kernel -------------------------------------------------------------------------
def facets():
    return once("facets", lambda: facet_set(euo.RECTILINEAR, 72, 72, 95.0, 4, 1, seed=3))


@pytest.mark.parametrize("synopsis", ["panorama", "hdr_merge"])
def test_multi_facet(synopsis):
    """the four facets around the horizon leave holes at the poles (exact zeros, written); all six merged"""
    os_, gs = facets()
    n = 4 if synopsis == "panorama" else 6
    a = ea.arguments(ea.SPHERICAL, 120, 75, 360.0, spline_degree=1, synopsis=synopsis)
    ref = jobs.oracle_render(a, os_[:n])
    if synopsis == "panorama":
        assert (ref == 0).all(-1).any() and (ref != 0).any()
    paddings(f"multi-facet {synopsis}", a, os_[:n], gs[:n], 4, ref, {"launches": 0})


# ---- stage outputs: 3 floats per pixel whatever the channel count ---------------------------------------------------
@pytest.mark.parametrize("nch", [1, 4])
@pytest.mark.parametrize("stage", [1, 2, 3, 4])
def test_stage_outputs(stage, nch):
    o, g = latlon_pair(nch, 1, 256, 128)
    a = ea.arguments(ea.SPHERICAL, 97, 48, 360.0, yaw=30, pitch=15, roll=7.5, spline_degree=1, twine=2 if stage > 2 else 0)
    paddings(f"stage {stage} nch {nch}", a, o, g, nch, jobs.oracle_render(a, o, stage=stage), {"launches": 1}, stage=stage)


# ---- tethered: packed words behind the float frame (to_screen_kernel) -----------------------------------------------
@pytest.mark.parametrize("nch", [1, 2, 3, 4])
def test_tethered(nch):
    img = jobs.synth_image(256, 128, nch) * 1.6 - 0.2
    if nch in (2, 4):
        img[:, :, nch - 1] = jobs.synth_image(256, 128, 1, seed=99)[:, :, 0]
    o, g = make_pair(euo.SPHERICAL, 256, 128, 360.0, img, 3)
    a = ea.arguments(ea.RECTILINEAR, 333, 77, 90.0, yaw=12, pitch=7, spline_degree=3, tethered=True)
    ref = jobs.oracle_render(a, o)
    assert len(np.unique(ref)) > 100
    paddings(f"tethered nch {nch}", a, o, g, nch, ref)


# ---- crops ----------------------------------------------------------------------------------------------------------
def test_crops():
    o, g = latlon_pair(3, 1, 256, 128)
    a = ea.arguments(ea.CUBEMAP, 48, 288, 90.0, yaw=5, spline_degree=1, crop=(5, 40, 30, 120))
    ref = jobs.oracle_render(a, o)
    assert ref.shape == (90, 35, 3)
    paddings("cropped cubemap", a, o, g, 3, ref)
    paddings("cropped cubemap, rows 0-33", a, o, g, 3, ref[:33], row_begin=0, row_end=33)
    paddings("cropped cubemap, rows 33-90", a, o, g, 3, ref[33:], row_begin=33)
    os_, gs = facets()
    a = ea.arguments(ea.SPHERICAL, 640, 320, 360.0, yaw=20, spline_degree=1, crop=(101, 640, 17, 200))
    paddings("cropped multi-facet", a, os_, gs, 4, jobs.oracle_render(a, os_))


# ---- interleaved row bands: local rows ------------------------------------------------------------------------------
@pytest.mark.parametrize("sw", [{}, {"EU_HIP_R4": "1"}], ids=name)
@pytest.mark.parametrize("band", [(4, 3, 1), (8, 2, 0)])
def test_bands(band, sw):
    """EU_HIP_R4=1: a band part has no FAST profile - eu_render5_kernel's other form"""
    o, g = latlon_pair(3, 3, 256, 128)
    a = ea.arguments(ea.CUBEMAP, 40, 240, 90.0, yaw=3, spline_degree=3)
    ref = once("band ref", lambda: jobs.oracle_render(a, o))[ea.band_frame_rows(240, *band)]
    use(sw)
    expect = {"launches": 2, "share": 0, "boxtab": 0} if sw else {"launches": lambda n: n >= 1}
    paddings(f"band {band} {name(sw)}", a, o, g, 3, ref, expect, band=band)
    n = len(ref)
    paddings(f"band {band} {name(sw)}, local rows 5-{n - 7}", a, o, g, 3, ref[5:n - 7], expect, band=band, row_begin=5,
             row_end=n - 7)
    if not sw:
        os_, gs = facets()
        a = ea.arguments(ea.SPHERICAL, 120, 75, 360.0, spline_degree=1)
        ref = once("band ref, multi-facet", lambda: jobs.oracle_render(a, os_))[ea.band_frame_rows(75, *band)]
        paddings(f"band {band} multi-facet", a, os_, gs, 4, ref, band=band)


# ---- eu_hip_render_samples and eu_hip_render_rgbe: encode_kernel, rgbe_encode_kernel --------------------------------
@pytest.mark.parametrize("entry,nch", [("samples8", 4), ("samples16", 3), ("rgbe", 3)])
def test_samples_and_quads(entry, nch):
    """the float frame goes into the library's buffer, the encoder writes the caller's: pad and lead count samples
    (one or two bytes) and quads. Bytes have no fill word to tell from a value: (b) is part of the comparison."""
    img = jobs.synth_image(256, 128, nch) * np.float32(1.8) - np.float32(0.35)
    o, g = make_pair(euo.SPHERICAL, 256, 128, 360.0, img, 3)
    a = cube_args(32, 3)
    bits = 16 if entry == "samples16" else 8
    table = ea.sample_steps(bits)

    def encode(frame):
        if entry == "rgbe":
            return rm.encode(frame)
        return devout.typed(want_bytes(frame, table, None, bits, False), a, nch, entry=entry)
    ref = encode(jobs.oracle_render(a, o))
    assert len(np.unique(ref)) > 8
    paddings(f"{entry} nch {nch}", a, o, g, nch, ref, entry=entry)
    paddings(f"{entry} nch {nch}, rows 37-150", a, o, g, nch, ref[37:150], entry=entry, row_begin=37, row_end=150)


# ---- a caller's stream ----------------------------------------------------------------------------------------------
def test_callers_stream():
    import torch
    stream = torch.cuda.Stream()
    o, g = latlon_pair(3, 3)
    use({"EU_HIP_R4": "1"})
    paddings("face 64 on a stream", cube_args(64, 3), o, g, 3, cube_ref(64, 3, 3), staged_expect({}, 64),
             stream=stream.cuda_stream)
    paddings("face 64 rows (136, 248) on a stream", cube_args(64, 3), o, g, 3, cube_ref(64, 3, 3)[136:248],
             staged_expect({}, 64, whole=False), stream=stream.cuda_stream, row_begin=136, row_end=248)
    use({})
    os_, gs = facets()
    a = ea.arguments(ea.SPHERICAL, 120, 75, 360.0, spline_degree=1)
    paddings("multi-facet on a stream", a, os_, gs, 4, once("band ref, multi-facet", lambda: jobs.oracle_render(a, os_)),
             stream=stream.cuda_stream)
    stream.synchronize()


def test_two_jobs_back_to_back_on_a_stream():
    """two different jobs queued into two guarded buffers, looked at after one sync(): the second job's plans, work
    list and tables are rewritten behind the first job, not under it"""
    import torch
    stream = torch.cuda.Stream()
    o, g = latlon_pair(3, 3)
    a1, a2 = cube_args(64, 3), cube_args(41, 3)
    use({"EU_HIP_R4": "1"})
    for pad, lead in ((0, 0), (1, 1), (5, 0)):
        b1 = devout.Guarded(384, 64 * 3, pad, lead)
        b2 = devout.Guarded(246, 41 * 3, pad, lead)
        devout.call_into(b1, a1, g, 3, stream=stream.cuda_stream)
        devout.call_into(b2, a2, g, 3, stream=stream.cuda_stream)
        ea.sync()
        devout.check(f"first of two, pad {pad} lead {lead}", devout.typed(b1.frame(), a1, 3), b1.outside(), cube_ref(64, 3, 3))
        devout.check(f"second of two, pad {pad} lead {lead}", devout.typed(b2.frame(), a2, 3), b2.outside(), cube_ref(41, 3, 3))
    stream.synchronize()


# ---- strips of one frame side by side: what a multi-GPU host sees -------------------------------------------------
@pytest.mark.parametrize("nch", [3, 4])
def test_adjacent_strips(nch):
    """three calls into ONE buffer filled once, looked at once at the end: a strip that writes over its neighbour,
    or leaves a row of its own to it, shows"""
    o, g = latlon_pair(nch, 3)
    a = cube_args(64, 3)
    use({"EU_HIP_R4": "1"})
    for pad in PADS:
        for lead in LEADS:
            buf = devout.Guarded(384, 64 * nch, pad, lead)
            n0 = ea.launch_count()
            for r0, r1 in ((0, 131), (131, 250), (250, 384)):
                devout.call_into(buf, a, g, nch, row_begin=r0, row_end=r1, first_row=r0)
            ea.sync()
            seen = probes(n0)
            devout.check(f"three strips nch {nch}, pad {pad} lead {lead}", devout.typed(buf.frame(), a, nch), buf.outside(),
                         cube_ref(64, 3, nch), seen)
            assert seen["launches"] == 6


# ---- the 32-bit offsets of eu5_tile_bt ------------------------------------------------------------------------------
@pytest.mark.parametrize("nch", [3, 4])
@pytest.mark.parametrize("stride,boxtab", [((1 << 25) - 1, 1), (1 << 25, 0)])
def test_offset_limit(stride, boxtab, nch):
    """eu5_tile_bt stores through 32-bit offsets from its tile row's base, and the launcher takes it for row strides
    below 2^25 floats: the last stride that does, the first that does not, one frame. One tile row of the top face,
    eight rows a gigabyte apart end to end; filled and checked on the device."""
    import torch
    free, _ = torch.cuda.mem_get_info()
    if free < 4 << 30:
        pytest.skip(f"{free >> 20} MiB of device memory free: the buffer takes 1 GiB and its check as much again")
    o, g = latlon_pair(nch, 3)
    use({"EU_HIP_R4": "1"})
    n0 = ea.launch_count()
    devout.held(f"rows (128, 136) nch {nch} at a row stride of {stride} floats", cube_args(64, 3), o, g, nch,
                ref=cube_ref(64, 3, nch)[128:136], probes=lambda: probes(n0), pad=stride - 64 * nch, row_begin=128, row_end=136)
    seen = probes(n0)
    torch.cuda.empty_cache()
    assert seen["launches"] == 2 and seen["boxtab"] == boxtab, seen
