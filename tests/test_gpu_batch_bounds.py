"""Where the kernels of eu_hip_render_views, eu_hip_render_views_multi, eu_hip_render_layers and eu_hip_render_rays
write. What tests/test_gpu_render_bounds.py holds for eu_hip_render, held for the entries that write straight into the
caller's memory with an outer stride of their own: every case goes through the C ABI with out_on_device = 1 into a
guarded buffer of several frames (tests/devout.py, GuardedFrames: all fill word 0x7FA5A5A5 before the call) and
holds three things through devout.held_frames: (a) every frame is the ORACLE's bit for bit (jobs.oracle_render per
view, per layer, or of the job whose rays are given - not envutil_amd.render), (b) no word of a frame is still the
fill word - misses and holes are written as zeros -, (c) no word of the guards, the lead, the rows' padding or the
gaps between the frames was touched. Every case runs with a row padding of 0, 1 and 5 words, with its first frame 0
and 1 words off the guard's end, and with 0 and 7 words between one frame's last row and the next frame's first (7 is
no multiple of any row stride here). Every call prints what it found outside the frames and how many frame words
were still fill. All images are finite, so the fill word - a NaN - is no pixel of any frame. tests/test_devout_host.py
shows on the CPU that each of the three checks fails when it should.

These entries leave eu_hip_launch_count() alone, so no counter says which kernel ran. What sends a case to its kernel
is the reason eu_select_view_path / eu_select_layer_path / eu_select_ray_path (envutil_amd/csrc/eu_select.h) give it,
and tests/csrc/select_views_demo.cc, select_layers_demo.cc and select_rays_demo.cc check each reason named below on
the CPU. The kernels that store pixels for these entries, the reason, and the cases that hold each:

  eu_views2_kernel       packed: lat/lon, cubemap and biatan6 sources at degrees 1 - 3, no lens polynomial, no channel
                         adaption, target not fisheye / stereographic
                           each without a switch ([default]): test_views_packed_sources, test_views_chunks,
                           test_views_none_and_one (its one-view half), test_views_on_a_callers_stream,
                           test_views_two_calls_on_one_stream
  eu_views_kernel        the same cases under EU_HIP_KERNEL=1 (the switch: [KERNEL=1] of every test above); and
                         sources the packed form does not cover: degree 0, lens polynomial, fisheye, channel adaption
                         3 -> 4 and 4 -> 1, --mask_for
                           test_views_general_sources, test_views_written_zeros
  eu_views_multi_kernel  every call of eu_hip_render_views_multi with more than one facet (no selection). Of the
                         ladder's forms (eu_multi_ladder, eu_multi_dev.h): the ordinary one with 3 channels; PLUS with
                         4 channels (no case has 2), the facets' coordinates kept in LDS (four and six facets) and,
                         beyond EU_MULTI_KEEP, recomputed (seventeen); HDR (synopsis hdr_merge: six, and the bracket of
                         three); BIG (more than EU_MULTI_MAXF = 64 facets with 4 channels: seventy-two, which with 3
                         channels is the ordinary form again)
                           test_views_multi, test_views_multi_twined, test_views_multi_chunks
  eu_layers2_kernel      packed, as eu_views2_kernel
                           each without a switch ([default]): test_layers_shapes (four packed sources),
                           test_layers_counts_and_launches, test_layers_bracket, test_layers_on_a_callers_stream
  eu_layers_kernel       the same cases under EU_HIP_KERNEL=1 ([KERNEL=1] of every test above); a source with a lens
                         polynomial
                           test_layers_shapes["rectilinear lens"]
  eu_rays2_kernel        packed: what eu_packed_covers_source admits (lat/lon cubic RGB here), rays and ninepacks
                           each without a switch ([packed] / [default]): test_rays_grids, test_rays_flat_lists,
                           test_rays_poisoned, test_rays_from_the_host, test_rays_on_a_callers_stream
  eu_rays_kernel         the same cases under EU_HIP_KERNEL=1 ([KERNEL=1] of every test above); a source with a lens
                         polynomial
                           [lens] of test_rays_grids, test_rays_flat_lists, test_rays_poisoned
  no kernel              calls that have nothing to write launch nothing and leave the whole buffer fill: the no-view
                         half of test_views_none_and_one, test_layers_none

Shapes: the smallest at which these kernels can go wrong. Tiles are 128 x 4 (packed) and 64 x 4 (general), XCD units
are 8 tile rows, a round is 8 units. Widths 1, 3, 17 (the three alignments of 3-channel rows), 65 (one live lane in the
second general tile), 129 (a lane-pair tail), 130 (a second packed tile of `xa` lanes only), 513 (the second segment of
512 columns); heights 1, 5 (a partial tile row), 33 (a second unit), 261 (66 tile rows: a second round over the XCDs,
at 17 and 129 wide). Every width runs with heights 5 and 33 and every height with widths 17 and 129; a cubemap target
of 40 x 240 and a biatan6 target of 24 x 144 have rows that depend on the face; twine 2 on the 17- and 129-wide
targets."""
import os

import numpy as np
import pytest

import devout
import envutil_amd as ea
import euo
import jobs
from test_gpu_parity import SRC_H, SRC_W, facet_set, make_pair
from test_gpu_rays import SOURCES, job_rays, pair
from test_hdr_merge import bracket

pytestmark = pytest.mark.gpu

SWITCHES = ("EU_HIP_KERNEL", "EU_HIP_VIEWS_MAX_KB", "EU_HIP_LAYERS_MAX", "EU_HIP_COLMAJOR", "EU_HIP_R4", "EU_HIP_HYBRID",
            "EU_HIP_DIRECT")
LAYOUTS = [(pad, lead, gap) for pad in (0, 1, 5) for lead in (0, 1) for gap in (0, 7)]
GENERAL = {"EU_HIP_KERNEL": "1"}

WIDTHS, HEIGHTS = (1, 3, 17, 65, 129, 130, 513), (1, 5, 33, 261)
SHAPES = sorted({(w, h) for w in WIDTHS for h in (5, 33)} | {(w, h) for w in (17, 129) for h in HEIGHTS})
# a lat/lon target of 360 degrees is as high as its step says: those that stay within the sphere
TARGETS = [(ea.RECTILINEAR, w, h, 90.0) for w, h in SHAPES] + [(ea.SPHERICAL, w, h, 360.0) for w, h in SHAPES if 2 * h <= w]
FACE_TARGETS = [(ea.CUBEMAP, 40, 240, 90.0), (ea.BIATAN6, 24, 144, 90.0)]
TWINED_TARGETS = [(ea.RECTILINEAR, w, h, 90.0) for w in (17, 129) for h in (5, 33)]


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


_kept = {}


def once(key, make):
    """sources and oracle frames are made once and shared, unchanged, between the cases that need them"""
    if key not in _kept:
        _kept[key] = make()
        if isinstance(_kept[key], np.ndarray):
            _kept[key].setflags(write=False)
    return _kept[key]


def views_of(hfov):
    """two orientations, and one with another hfov (tests/test_gpu_views.py)"""
    return [(0.0, 0.0, 0.0), (30.0, 15.0, 7.5), (-40.0, 20.0, -5.0, hfov * 0.75)]


def five_views(hfov):
    return [(12.0 * k, 5.0 * k - 10.0, 3.0 * k, hfov - 4 * k) for k in range(5)]


def args_of(target, view=(0.0, 0.0, 0.0), **kw):
    tprj, tw, th, thfov = target
    return ea.arguments(tprj, tw, th, view[3] if len(view) == 4 else thfov, yaw=view[0], pitch=view[1], roll=view[2], **kw)


def finite(ref):
    assert np.isfinite(ref).all(), "the fill word must not be a pixel of the oracle's"
    return ref


def view_refs(key, o, target, views, nch=None, **kw):
    """the oracle's frame of every view: jobs.oracle_render of the target with that view's orientation and hfov"""
    return [once(("view", key, target, tuple(v), nch, tuple(sorted(kw.items()))),
                 lambda: finite(jobs.oracle_render(args_of(target, v, **kw), o, nch=nch))) for v in views]


def into_views(what, g, target, views, refs, nch, stream=None, layouts=LAYOUTS, **kw):
    """one call per layout; `g`: a source, or the list of a multi-facet job's"""
    a = args_of(target, **kw)
    _, tw, th, _ = target
    for pad, lead, gap in layouts:
        buf = devout.GuardedFrames(len(views), th, tw * nch, pad, lead, gap)
        devout.views_into(buf, a, views, g, nch, stream)
        ea.sync()
        devout.held_frames(f"{what}, {tw} x {th} of projection {target[0]}, pad {pad} lead {lead} gap {gap}", buf, refs)


# ---- sources: tests/test_gpu_rays.py's, and those of tests/test_gpu_views.py's channel adaption and --mask_for cases ----
def special(kind):
    def make():
        if kind == "mask_for":
            img = jobs.synth_image(64, 48, 3)
            o = jobs.OracleSource(euo.RECTILINEAR, 64, 48, 70.0, img, 1, masked=1)
            return o, ea.Source.adopt(ea.facet_spec(ea.RECTILINEAR, 64, 48, 70.0, masked=1), o.container, 1, o.bc[0], o.bc[1])
        src_n = int(kind[6])
        img = jobs.synth_image(128, 64, src_n, seed=4)
        if src_n == 4:
            img[:, :, 3] = (np.indices((64, 128))[1] % 7 != 0).astype(np.float32)
        return make_pair(euo.RECTILINEAR, 128, 64, 100.0, img, 1, brighten=1.3)
    return once(("special", kind), make)


# name -> (source channels, output channels, degree); the reason for the general form is the name
GENERAL_SOURCES = {"latlon d0": (3, 3, 0), "rectilinear lens": (3, 3, 3), "fisheye": (3, 3, 1),
                   "repix 3 -> 4": (3, 4, 1), "repix 4 -> 1": (4, 1, 1), "mask_for": (3, 3, 1)}
PACKED_SOURCES = ["latlon d1 n1", "latlon d3 n3", "latlon d3 n4", "cubemap d2", "biatan6 d3"]


def source(key):
    return pair(key) if key in SOURCES else special(key)


# =====================================================================================================================
# eu_hip_render_views
# =====================================================================================================================
@pytest.mark.parametrize("sw", [{}, GENERAL], ids=name)
@pytest.mark.parametrize("key", PACKED_SOURCES)
def test_views_packed_sources(key, sw):
    """three views per call; every shape, the face targets, twine 2 at 17 and 129 wide; eu_views2_kernel, and
    eu_views_kernel under the switch"""
    o, g = pair(key)
    nch, degree, packed = SOURCES[key][4], SOURCES[key][5], SOURCES[key][7]
    assert packed and 1 <= degree <= 3
    for targets, kw in ((TARGETS + FACE_TARGETS, {}), (TWINED_TARGETS, dict(twine=2))):
        for target in targets:
            views = views_of(target[3])
            refs = view_refs(key, o, target, views, spline_degree=degree, **kw)
            use(sw)
            into_views(f"views of {key}, {name(sw)}, twine {kw.get('twine', 0)}", g, target, views, refs, nch,
                       spline_degree=degree, **kw)


@pytest.mark.parametrize("key", list(GENERAL_SOURCES))
def test_views_general_sources(key):
    """sources the packed form does not cover: eu_views_kernel without a switch"""
    o, g = source(key)
    src_n, nch, degree = GENERAL_SOURCES[key]
    assert o.nch == src_n and o.degree == degree
    for targets, kw in ((TARGETS + FACE_TARGETS, {}), (TWINED_TARGETS, dict(twine=2))):
        for target in targets:
            views = views_of(target[3])
            refs = view_refs(key, o, target, views, nch, spline_degree=degree, **kw)
            into_views(f"views of {key}, twine {kw.get('twine', 0)}", g, target, views, refs, nch, spline_degree=degree, **kw)


@pytest.mark.parametrize("twine", [0, 2])
def test_views_written_zeros(twine):
    """a facet of 80 degrees under lat/lon targets of the whole sphere: every view's oracle frame holds all-zero pixels
    beside non-zero ones - asserted here, on the oracle - so a miss the kernel does not store shows in (b)"""
    key = "rectilinear lens"
    o, g = pair(key)
    kw = dict(twine=twine) if twine else {}
    for target in ((ea.SPHERICAL, 129, 33, 360.0), (ea.SPHERICAL, 130, 65, 360.0)):
        views = views_of(360.0)
        refs = view_refs(key, o, target, views, spline_degree=3, **kw)
        for k, ref in enumerate(refs):
            assert (ref == 0).all(-1).any() and (ref != 0).any(), f"view {k}: misses and hits in one frame"
        into_views(f"written zeros, twine {twine}", g, target, views, refs, 3, spline_degree=3, **kw)


CHUNK_TARGET = (ea.RECTILINEAR, 65, 33, 90.0)


def chunk_switches(target, nfct=1):
    """one view per chunk; the bound that holds exactly two views' tables (tests/test_gpu_views_multi.py); no switch"""
    _, tw, th, _ = target
    per = nfct * (6 * tw + 24 * th) * 4
    two = -(-2 * per // 1024)
    assert 2 * per <= two * 1024 < 3 * per
    return [{"EU_HIP_VIEWS_MAX_KB": "1"}, {"EU_HIP_VIEWS_MAX_KB": str(two)}, {}]


@pytest.mark.parametrize("general", [{}, GENERAL], ids=name)
def test_views_chunks(general):
    """five views into one buffer in chunks of 1, of 2, 2, 1 and in one: a chunk starts at out + c0 * view stride"""
    key = "latlon d3 n3"
    o, g = pair(key)
    views = five_views(90.0)
    refs = view_refs(key, o, CHUNK_TARGET, views, spline_degree=3)
    for sw in chunk_switches(CHUNK_TARGET):
        use(dict(sw, **general))
        into_views(f"five views, {name(dict(sw, **general))}", g, CHUNK_TARGET, views, refs, 3, spline_degree=3)


@pytest.mark.parametrize("general", [{}, GENERAL], ids=name)
def test_views_none_and_one(general):
    key = "latlon d3 n3"
    o, g = pair(key)
    target = (ea.RECTILINEAR, 129, 33, 90.0)
    a = args_of(target, spline_degree=3)
    views = views_of(90.0)
    refs = view_refs(key, o, target, views, spline_degree=3)
    use(general)
    for pad, lead, gap in LAYOUTS:
        buf = devout.GuardedFrames(2, 33, 129 * 3, pad, lead, gap)
        devout.views_into(buf, a, [], g, 3)
        ea.sync()
        devout.untouched(f"no view, {name(general)}, pad {pad} lead {lead} gap {gap}", buf)
    for k in (1, 2):
        into_views(f"one view, {name(general)}", g, target, views[k:k + 1], refs[k:k + 1], 3, spline_degree=3)


@pytest.mark.parametrize("general", [{}, GENERAL], ids=name)
def test_views_on_a_callers_stream(general):
    import torch
    stream = torch.cuda.Stream()
    key = "latlon d3 n3"
    o, g = pair(key)
    for target in ((ea.RECTILINEAR, 129, 33, 90.0), (ea.CUBEMAP, 40, 240, 90.0)):
        views = views_of(90.0)
        refs = view_refs(key, o, target, views, spline_degree=3)
        use(general)
        into_views(f"views on a stream, {name(general)}", g, target, views, refs, 3, stream=stream.cuda_stream,
                   spline_degree=3)
    stream.synchronize()


@pytest.mark.parametrize("general", [{}, GENERAL], ids=name)
def test_views_two_calls_on_one_stream(general):
    """two different calls queued into two guarded buffers, looked at after one sync(): the second call's tables and
    scalar blocks are rewritten behind the first call, not under it"""
    import torch
    stream = torch.cuda.Stream()
    key = "latlon d3 n3"
    o, g = pair(key)
    t1, t2 = (ea.RECTILINEAR, 129, 33, 90.0), (ea.RECTILINEAR, 65, 33, 90.0)
    v1, v2 = views_of(90.0), five_views(90.0)
    r1, r2 = view_refs(key, o, t1, v1, spline_degree=3), view_refs(key, o, t2, v2, spline_degree=3)
    use(general)
    for pad, lead, gap in LAYOUTS:
        b1 = devout.GuardedFrames(3, 33, 129 * 3, pad, lead, gap)
        b2 = devout.GuardedFrames(5, 33, 65 * 3, pad, lead, gap)
        devout.views_into(b1, args_of(t1, spline_degree=3), v1, g, 3, stream.cuda_stream)
        devout.views_into(b2, args_of(t2, spline_degree=3), v2, g, 3, stream.cuda_stream)
        ea.sync()
        devout.held_frames(f"first of two, {name(general)}, pad {pad} lead {lead} gap {gap}", b1, r1)
        devout.held_frames(f"second of two, {name(general)}, pad {pad} lead {lead} gap {gap}", b2, r2)
    stream.synchronize()


# =====================================================================================================================
# eu_hip_render_views_multi
# =====================================================================================================================
MULTI_TARGETS = [(ea.SPHERICAL, 130, 65, 360.0), (ea.RECTILINEAR, 65, 77, 100.0), (ea.SPHERICAL, 513, 10, 360.0),
                 (ea.CUBEMAP, 40, 240, 90.0)]


def facets(nch):
    """tests/test_gpu_render_bounds.py's six"""
    return once(("facets", nch), lambda: facet_set(euo.RECTILINEAR, 72, 72, 95.0, nch, 1, seed=3))


def rect24(nch):
    """tests/test_gpu_views_multi.py's rect24, with the oracle's sources beside the library's"""
    def make():
        os_, gs = [], []
        for k in range(4):
            o, g = facet_set(euo.RECTILINEAR, 48, 48, 70.0 + 5 * k, nch, 1, seed=40 + k)
            os_, gs = os_ + o, gs + g
        return os_, gs
    return once(("rect24", nch), make)


def facet_job(job, nch):
    """(oracle sources, library sources, keywords of the job)"""
    if job == "panorama of four":
        os_, gs = facets(nch)
        return os_[:4], gs[:4], {}
    if job == "hdr_merge of six":
        os_, gs = facets(nch)
        return os_, gs, dict(synopsis="hdr_merge")
    if job == "seventeen":
        os_, gs = rect24(nch)
        return os_[:17], gs[:17], {}
    if job == "seventy-two":            # every facet three times over: equal z scores, the earlier one on top
        os_, gs = rect24(nch)
        return os_ * 3, gs * 3, {}
    assert job == "bracket"
    os_, gs = once(("bracket", nch), lambda: bracket(euo.RECTILINEAR, 96, 64, 75.0, nch, 1, (4.0, 1.0, 0.25), with_gpu=True,
                                                     alpha_holes=True))
    return os_, gs, dict(synopsis="hdr_merge")


@pytest.mark.parametrize("nch", [3, 4])
@pytest.mark.parametrize("job", ["panorama of four", "hdr_merge of six", "seventeen", "seventy-two", "bracket"])
def test_views_multi(job, nch):
    """four facets around the horizon: holes at the poles, exact zeros, written; six merged (HDR); seventeen, beyond
    EU_MULTI_KEEP: with 4 channels (PLUS) the winners' coordinates are recomputed, not kept in LDS; seventy-two,
    beyond EU_MULTI_MAXF: with 4 channels the BIG form. The bracket of three exposures looks along its axis"""
    os_, gs, kw = facet_job(job, nch)
    for target in MULTI_TARGETS:
        views = views_of(target[3])
        if job == "bracket":
            if target[0] != ea.RECTILINEAR:
                continue
            views = [(0.0, 0.0, 0.0), (10.0, 5.0, 3.0), (-8.0, 4.0, -5.0, 45.0)]
        refs = view_refs((job, nch), os_, target, views, nch, spline_degree=1, **kw)
        if job == "panorama of four" and target == MULTI_TARGETS[0]:          # the one that reaches the poles
            assert all((r == 0).all(-1).any() and (r != 0).any() for r in refs), "holes beside pixels"
        into_views(f"{job}, {nch} channels", gs, target, views, refs, nch, spline_degree=1, **kw)


@pytest.mark.parametrize("nch", [3, 4])
def test_views_multi_twined(nch):
    """65 x 5: one live lane in the second tile, under the twine loop"""
    target = (ea.SPHERICAL, 65, 5, 360.0)
    for job in ("panorama of four", "seventeen", "seventy-two"):
        os_, gs, kw = facet_job(job, nch)
        views = views_of(360.0)
        refs = view_refs((job, nch), os_, target, views, nch, spline_degree=1, twine=2, **kw)
        into_views(f"{job} twined, {nch} channels", gs, target, views, refs, nch, spline_degree=1, twine=2, **kw)


@pytest.mark.parametrize("nch", [3, 4])
def test_views_multi_chunks(nch):
    os_, gs, kw = facet_job("hdr_merge of six", nch)
    target = (ea.RECTILINEAR, 65, 77, 100.0)
    views = five_views(100.0)
    refs = view_refs(("hdr_merge of six", nch), os_, target, views, nch, spline_degree=1, **kw)
    for sw in chunk_switches(target, 6):
        use(sw)
        into_views(f"five views of six facets, {nch} channels, {name(sw)}", gs, target, views, refs, nch, spline_degree=1, **kw)


# =====================================================================================================================
# eu_hip_render_layers
# =====================================================================================================================
CAMERA = (30.0, 15.0, 7.5)


def layers_of(key, count):
    """`count` pictures of the geometry SOURCES[key], layer k carrying seed 31 + k (tests/test_gpu_layers.py): a store
    into the wrong layer's slot is another picture's pixel"""
    prj, w, h, hfov, nch, degree, kw, _ = SOURCES[key]

    def make(k):
        img = jobs.synth_image(w, 6 * w, nch, seed=31 + k) if prj in (euo.CUBEMAP, euo.BIATAN6) else \
            jobs.synth_image(w, h, nch, seed=31 + k)
        return make_pair(prj, w, h, hfov, img, degree, **kw)
    both = [once(("layer", key, k), lambda: make(k)) for k in range(count)]
    return [b[0] for b in both], [b[1] for b in both]


def layer_refs(key, os_, target, **kw):
    return [once(("layer ref", key, k, target, tuple(sorted(kw.items()))),
                 lambda: finite(jobs.oracle_render(args_of(target, CAMERA, **kw), o))) for k, o in enumerate(os_)]


def into_layers(what, gs, target, refs, nch, stream=None, **kw):
    a = args_of(target, CAMERA, **kw)
    _, tw, th, _ = target
    for pad, lead, gap in LAYOUTS:
        buf = devout.GuardedFrames(len(gs), th, tw * nch, pad, lead, gap)
        devout.layers_into(buf, a, gs, nch, stream)
        ea.sync()
        devout.held_frames(f"{what}, {tw} x {th} of projection {target[0]}, pad {pad} lead {lead} gap {gap}", buf, refs)


LAYER_SOURCES = ["latlon d3 n3", "cubemap d2", "latlon d1 n1", "latlon d3 n4"]       # packed-eligible: both kernels


@pytest.mark.parametrize("key,sw", [(k, sw) for k in LAYER_SOURCES for sw in ({}, GENERAL)] + [("rectilinear lens", {})],
                         ids=lambda v: v if isinstance(v, str) else name(v))
def test_layers_shapes(key, sw):
    """two layers per call at every shape and on the face targets, twine 2 at 17 and 129 wide: the tile arithmetic of
    eu_layers2_kernel and eu_layers_kernel and the store loop at k * lp.out_layer. Every packed-eligible source runs
    on both kernels: 1-, 3- and 4-channel rows and a cube source on each"""
    os_, gs = layers_of(key, 2)
    nch, degree = SOURCES[key][4], SOURCES[key][5]
    assert SOURCES[key][7] == (key in LAYER_SOURCES)
    for targets, kw in ((TARGETS + FACE_TARGETS, {}), (TWINED_TARGETS, dict(twine=2))):
        for target in targets:
            refs = layer_refs(key, os_, target, spline_degree=degree, **kw)
            use(sw)
            into_layers(f"layers of {key}, {name(sw)}, twine {kw.get('twine', 0)}", gs, target, refs, nch,
                        spline_degree=degree, **kw)


@pytest.mark.parametrize("general", [{}, GENERAL], ids=name)
@pytest.mark.parametrize("twine", [0, 2])
def test_layers_counts_and_launches(twine, general):
    """1, 2 and 5 layers; five are a launch of four and one of one by default, one launch under EU_HIP_LAYERS_MAX=0,
    five under 1, three (the last one partial) under 2: a launch starts at out + c0 * layer stride, and a twined
    launch stores group by group"""
    key = "latlon d3 n3"
    kw = dict(twine=twine) if twine else {}
    for target in ((ea.RECTILINEAR, 129, 33, 90.0), (ea.RECTILINEAR, 17, 5, 90.0), (ea.SPHERICAL, 130, 5, 360.0)):
        for count in (1, 2, 5):
            os_, gs = layers_of(key, count)
            refs = layer_refs(key, os_, target, spline_degree=3, **kw)
            for most in (None, "0", "1", "2"):
                sw = dict(general, **({"EU_HIP_LAYERS_MAX": most} if most else {}))
                use(sw)
                into_layers(f"{count} layers, twine {twine}, {name(sw)}", gs, target, refs, 3, spline_degree=3, **kw)


@pytest.mark.parametrize("general", [{}, GENERAL], ids=name)
def test_layers_bracket(general):
    """a bracket: one geometry, every layer its own picture and its own brighten (alpha is not brightened)"""
    import pixel_values as pv

    def make(k, b):
        img = pv.with_alpha(jobs.synth_image(SRC_W, SRC_H, 4, seed=31 + k), seed=3)
        return make_pair(euo.SPHERICAL, SRC_W, SRC_H, 360.0, img, 3, brighten=b)
    both = [once(("bracket layer", k), lambda: make(k, b)) for k, b in enumerate((1.0, 0.8, 0.25))]
    os_, gs = [b[0] for b in both], [b[1] for b in both]
    for twine in (0, 2):
        kw = dict(twine=twine) if twine else {}
        for target in ((ea.RECTILINEAR, 129, 33, 90.0), (ea.CUBEMAP, 40, 240, 90.0)):
            refs = layer_refs("bracket", os_, target, spline_degree=3, **kw)
            assert (jobs.bits(refs[1]) != jobs.bits(refs[0])).any()
            use(general)
            into_layers(f"bracket, twine {twine}, {name(general)}", gs, target, refs, 4, spline_degree=3, **kw)


@pytest.mark.parametrize("general", [{}, GENERAL], ids=name)
def test_layers_on_a_callers_stream(general):
    import torch
    stream = torch.cuda.Stream()
    key = "latlon d3 n3"
    os_, gs = layers_of(key, 5)
    target = (ea.RECTILINEAR, 129, 33, 90.0)
    refs = layer_refs(key, os_, target, spline_degree=3)
    use(general)
    into_layers(f"five layers on a stream, {name(general)}", gs, target, refs, 3, stream=stream.cuda_stream, spline_degree=3)
    stream.synchronize()


def test_layers_none():
    _, gs = layers_of("latlon d3 n3", 1)
    a = args_of((ea.RECTILINEAR, 129, 33, 90.0), CAMERA, spline_degree=3)
    for pad, lead, gap in LAYOUTS:
        buf = devout.GuardedFrames(2, 33, 129 * 3, pad, lead, gap)
        devout.layers_into(buf, a, [], 3)
        ea.sync()
        devout.untouched(f"no layer, pad {pad} lead {lead} gap {gap}", buf)


# =====================================================================================================================
# eu_hip_render_rays
# =====================================================================================================================
RAY_SOURCES = [("latlon d3 n3", {}), ("latlon d3 n3", GENERAL), ("rectilinear lens", {})]
RAY_IDS = ["packed", "KERNEL=1", "lens"]
RAY_GRIDS = sorted({(w, h) for w in WIDTHS for h in (2, 5, 33)} | {(3, 257), (129, 257)})
FLAT = (1, 63, 64, 65, 127, 128, 129, 511, 512, 513, 8191, 8192, 8193, 16383, 16384, 16385, 32769)
BAD = (np.nan, np.inf, -np.inf)


def ray_job(key, w, h, nin):
    """(rays or ninepacks, taps, the oracle's frame) of a job of w x h pixels on source `key`: the oracle's stage 1 -
    with stages 3 and 4 of the twined job beside it for ninepacks - and its stage 0. The camera looks along the
    edge of the 80 degree facet: its rows, the first ones too, begin on the facet and end beside it"""
    o, _ = pair(key)
    kw = dict(yaw=30.0, pitch=0.0, roll=5.0, spline_degree=SOURCES[key][5])
    if nin == 3:
        a = ea.arguments(ea.RECTILINEAR, w, h, 90.0, **kw)
        return job_rays(a, o), None, once(("ray ref", key, w, h, 3), lambda: finite(jobs.oracle_render(a, o)))
    a = ea.arguments(ea.RECTILINEAR, w, h, 90.0, twine=2, **kw)
    assert np.array_equal(a.twine_spread, ea.make_spread(2, 2))
    nine = once(("ninepacks", key, w, h),
                lambda: finite(np.concatenate([jobs.oracle_render(a, o, stage=k) for k in (1, 3, 4)], axis=2)))
    return nine, a.twine_spread, once(("ray ref", key, w, h, 9), lambda: finite(jobs.oracle_render(a, o)))


def on_device(rays, pad):
    """the rays on the device in rows `pad` floats longer than they are, the padding NaN: a ray read from it is a miss,
    its pixel a zero the oracle's frame does not have there"""
    import torch
    rays = np.array(rays)       # a copy: the shared rays are read-only
    if rays.ndim == 2:         # a flat list has one row: nothing to pad
        return torch.from_numpy(rays).to("cuda")
    h, w, k = rays.shape
    wide = torch.full((h, w + pad, k), float("nan"), dtype=torch.float32, device="cuda")
    wide[:, :w] = torch.from_numpy(rays).to("cuda")
    return wide[:, :w]


def into_rays(what, g, rays, taps, ref, nch, device=True, stream=None):
    rays = np.asarray(rays)
    h, w = (1, rays.shape[0]) if rays.ndim == 2 else rays.shape[:2]
    for pad, lead, gap in LAYOUTS:
        buf = devout.GuardedFrames(1, h, w * nch, pad, lead, gap)
        keep = devout.rays_into(buf, g, on_device(rays, 2 * pad + 1) if device else np.array(rays), nch, taps, stream)
        ea.sync()
        del keep
        devout.held_frames(f"{what}, {w} x {h}, pad {pad} lead {lead} gap {gap}", buf, [ref])


@pytest.mark.parametrize("nin", [3, 9])
@pytest.mark.parametrize("key,sw", RAY_SOURCES, ids=RAY_IDS)
def test_rays_grids(key, sw, nin):
    """the rays of a job as its grid, in device memory with padded rows. rays_grid takes unit_rows = max(1, min(8,
    tile rows / 8)): heights 2, 5 and 33 (1, 2 and 9 tile rows) have one tile row per XCD unit, 33 rows with a second
    unit on XCD 0; only the grids of 257 rows (65 tile rows) reach unit_rows 8, and a second round over the XCDs -
    3 x 257 in one partial tile column, 129 x 257 with a column tail (a lane-pair tail of the packed tile, a third
    general tile of one lane)"""
    g = pair(key)[1]
    for w, h in RAY_GRIDS:
        rays, taps, ref = ray_job(key, w, h, nin)
        use(sw)
        into_rays(f"{nin} inputs of {key}, {name(sw)}", g, rays, taps, ref, 3)


def flat_job(key, nin, n):
    """the first n rays of a job large enough, flattened, and their pixels"""
    w, h = (257, 129) if nin == 3 else (129, 65)
    assert w * h >= n
    rays, taps, ref = ray_job(key, w, h, nin)
    return rays.reshape(-1, nin)[:n], taps, ref.reshape(-1, ref.shape[-1])[:n]


@pytest.mark.parametrize("nin", [3, 9])
@pytest.mark.parametrize("key,sw", RAY_SOURCES, ids=RAY_IDS)
def test_rays_flat_lists(key, sw, nin):
    """a flat list is dealt out as a virtual grid of 32 tiles of four pieces: the edges of a piece (64 / 128 rays), of
    a tile (256 / 512) and of a row of tiles (8192 / 16384) for both tile widths, and a third row"""
    g = pair(key)[1]
    for n in FLAT:
        if nin == 9 and n > 8193:       # the oracle's work triples
            continue
        rays, taps, ref = flat_job(key, nin, n)
        use(sw)
        into_rays(f"{n} x {nin} inputs of {key}, {name(sw)}", g, rays, taps, ref[None], 3)


def poison(rays, ref, spots):
    """NaN, +-inf in one component or another and the null ray at `spots` (indices into the first axes): zeros"""
    rays, ref = np.array(rays), np.array(ref)
    nin = rays.shape[-1]
    for i, at in enumerate(spots):
        p = rays[at].copy()
        if i % 4 == 3:
            p[:3] = 0.0 if i % 8 == 3 else -0.0        # the null ray: a null centre for a ninepack
        else:
            p[(5 * i) % nin] = BAD[i % 3]
        rays[at] = p
        ref[at] = 0.0
    return rays, ref


@pytest.mark.parametrize("nin", [3, 9])
@pytest.mark.parametrize("key,sw", RAY_SOURCES, ids=RAY_IDS)
def test_rays_poisoned(key, sw, nin):
    """misses among ordinary rays, at the first and the last lane of a piece among others: their pixels are written
    zeros, their neighbours' the oracle's"""
    g = pair(key)[1]
    rays, taps, ref = flat_job(key, nin, 1025)
    spots = [0, 1, 63, 64, 65, 127, 128, 191, 192, 255, 256, 300, 511, 512, 513, 767, 768, 1023, 1024]
    bad, want = poison(rays, ref, spots)
    assert all((want[s] == 0).all() for s in spots), "the poisoned rays' pixels are zeros"
    assert sum((ref[s] != 0).any() for s in spots) >= len(spots) // 4, "and were not before"
    use(sw)
    into_rays(f"poisoned list of {nin} inputs, {key}, {name(sw)}", g, bad, taps, want[None], 3)
    rays, taps, ref = ray_job(key, 129, 5, nin)
    spots = [(0, 0), (0, 63), (0, 64), (0, 127), (0, 128), (1, 1), (2, 65), (3, 128), (4, 0), (4, 127), (4, 128)]
    bad, want = poison(rays, ref, spots)
    into_rays(f"poisoned grid of {nin} inputs, {key}, {name(sw)}", g, bad, taps, want, 3)


@pytest.mark.parametrize("general", [{}, GENERAL], ids=name)
@pytest.mark.parametrize("nin", [3, 9])
def test_rays_from_the_host(nin, general):
    """rays in host memory, `out` on the device: the staged route writes the caller's memory chunk by chunk (one
    chunk here: a chunk is 64 MiB); a grid and a flat list"""
    key = "latlon d3 n3"
    g = pair(key)[1]
    rays, taps, ref = ray_job(key, 129, 33, nin)
    use(general)
    into_rays(f"host rays, {nin} inputs, {name(general)}", g, rays, taps, ref, 3, device=False)
    rays, taps, ref = flat_job(key, nin, 513)
    use(general)
    into_rays(f"host list, {nin} inputs, {name(general)}", g, rays, taps, ref[None], 3, device=False)


@pytest.mark.parametrize("general", [{}, GENERAL], ids=name)
@pytest.mark.parametrize("nin", [3, 9])
def test_rays_on_a_callers_stream(nin, general):
    import torch
    stream = torch.cuda.Stream()
    key = "latlon d3 n3"
    g = pair(key)[1]
    rays, taps, ref = ray_job(key, 129, 33, nin)
    use(general)
    into_rays(f"rays on a stream, {nin} inputs, {name(general)}", g, rays, taps, ref, 3, stream=stream.cuda_stream)
    stream.synchronize()
