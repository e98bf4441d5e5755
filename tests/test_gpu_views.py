"""Many views in one call: ea.render_views (eu_hip_render_views) against ea.render of every view, which is the
library's existing path and itself pinned to the CPU oracle. Float32 bit patterns, 0 ULP, no pixel left out. The
stepper tables the device builds for a view are compared entry by entry with the host's (ea.view_tables), so a
difference names the table and the entry, not just a frame."""
import ctypes as C
import math

import numpy as np
import pytest

import envutil_amd as ea
import euo
import jobs
from test_gpu_parity import SRC_H, SRC_W, TARGETS, assert_bits, make_pair
from test_gpu_rays import SOURCES, pair

pytestmark = pytest.mark.gpu

PACKED = ["latlon d1 n3", "latlon d3 n4", "cubemap d2", "biatan6 d3"]
GENERAL = ["latlon d0", "latlon d5", "rectilinear lens", "fisheye", "rectilinear ypr"]
# at 130 the second 128-pixel tile of the packed form has only `xa` lanes, 129 ends in a lane-pair tail; 513 and
# 1100 (in TARGETS) reach the second segment of 512 columns, where a lane's planar x starts again
WIDTHS = [(ea.RECTILINEAR, 130, 9, 90.0), (ea.SPHERICAL, 129, 5, 360.0), (ea.SPHERICAL, 513, 6, 360.0),
          (ea.RECTILINEAR, 513, 5, 100.0)]


def views_of(hfov):
    """two orientations, and one with another hfov"""
    return [(0.0, 0.0, 0.0), (30.0, 15.0, 7.5), (-40.0, 20.0, -5.0, hfov * 0.75)]


_refs = {}


def reference(g, name, target, view, nch=None, **kw):
    """ea.render of one view: computed once per (source, job), shared, read-only"""
    key = (name, target, tuple(view), nch, tuple(sorted(kw.items())))
    if key not in _refs:
        tprj, tw, th, thfov = target
        hfov = view[3] if len(view) == 4 else thfov
        a = ea.arguments(tprj, tw, th, hfov, yaw=view[0], pitch=view[1], roll=view[2], **kw)
        r = ea.render(a, g, nchannels=nch)
        r.setflags(write=False)
        _refs[key] = r
    return _refs[key]


def check_views(g, name, target, views, what, nch=None, distinct=True, **kw):
    tprj, tw, th, thfov = target
    a = ea.arguments(tprj, tw, th, thfov, **kw)
    got = ea.render_views(a, views, g, nchannels=nch)
    assert got.shape == (len(views), th, tw, nch or g.fct.nchannels)
    for k, v in enumerate(views):
        assert_bits(got[k], reference(g, name, target, v, nch, **kw), f"{what}: target {target}, view {k} {v}")
    # the comparison means something: the views show different things
    assert not distinct or all((jobs.bits(got[k]) != jobs.bits(got[0])).any() for k in range(1, len(views))), what
    return got


# ---- tables -----------------------------------------------------------------------------------------------------

TABLE_PRJ = {
    ea.SPHERICAL: (360.0, 200.0), ea.CYLINDRICAL: (220.0, 100.0), ea.RECTILINEAR: (90.0, 60.0),
    ea.STEREOGRAPHIC: (240.0, 150.0), ea.FISHEYE: (200.0, 120.0), ea.CUBEMAP: (90.0, 67.5), ea.BIATAN6: (90.0, 67.5),
}
COL_NAMES = ["c0", "c1", "c0 x-biased", "c1 x-biased", "planar x", "planar x x-biased"]


def assert_tables(a, view, g, what):
    col_d, row_d, col_h, row_h = ea.view_tables(a, view, g)
    assert col_d.shape == col_h.shape == (6, a.width) and row_d.shape == row_h.shape == (a.height, 24)
    assert np.isfinite(col_h).all() and np.isfinite(row_h).all(), what + ": the test uses finite extents only"
    bad = np.argwhere(jobs.bits(col_d) != jobs.bits(col_h))
    if bad.size:
        r, x = bad[0]
        raise AssertionError(f"{what}: column table differs in {len(bad)} entries, first {COL_NAMES[r]}[{x}]: "
                             f"device {col_d[r, x]!r} host {col_h[r, x]!r}")
    bad = np.argwhere(jobs.bits(row_d) != jobs.bits(row_h))
    if bad.size:
        y, j = bad[0]
        raise AssertionError(f"{what}: row table differs in {len(bad)} entries, first row {y} float {j} "
                             f"(variant {j // 12}, {'ABC'[j % 12 // 3] if j % 12 < 9 else 'planar y / pad'}): "
                             f"device {row_d[y, j]!r} host {row_h[y, j]!r}")


@pytest.mark.parametrize("prj", list(TABLE_PRJ))
@pytest.mark.parametrize("twine", [0, 2])
def test_device_built_tables_equal_the_host_built(prj, twine):
    """every target projection: one lane, a partial lane group, a segment boundary, a second segment with leftover
    lanes; one, seven and twelve rows; the cube targets at 40 x 240 and 24 x 144. The source's own orientation is
    part of the basis."""
    g = pair("rectilinear ypr")[1]
    if prj == ea.CUBEMAP:
        sizes = [(40, 240), (1, 6)]
    elif prj == ea.BIATAN6:
        sizes = [(24, 144), (1, 6)]
    else:
        sizes = [(w, h) for w in (1, 15, 17, 512, 513, 1100) for h in (1, 7, 12)]
    hfov, other = TABLE_PRJ[prj]
    for w, h in sizes:
        a = ea.arguments(prj, w, h, hfov, twine=twine)
        for view in [(0, 0, 0), (30, 15, 7.5), (0, 0, 0, other), (30, 15, 7.5, other)]:
            assert_tables(a, view, g, f"projection {prj} {w}x{h} twine {twine} view {view}")


# ---- frames -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", PACKED + GENERAL)
def test_every_view_is_the_frame_of_render(name, monkeypatch):
    """all eight TARGETS, three views per call; the packed-eligible sources again under EU_HIP_KERNEL=1"""
    g = pair(name)[1]
    degree = SOURCES[name][5]
    assert SOURCES[name][7] == (name in PACKED)
    for target in TARGETS:
        views = views_of(target[3])
        check_views(g, name, target, views, name, spline_degree=degree)
        if name in PACKED:
            monkeypatch.setenv("EU_HIP_KERNEL", "1")
            check_views(g, name, target, views, name + ", EU_HIP_KERNEL=1", spline_degree=degree)
            monkeypatch.delenv("EU_HIP_KERNEL")


@pytest.mark.parametrize("name", ["latlon d1 n3", "latlon d0"])
def test_tile_tails_and_second_segments(name):
    g = pair(name)[1]
    for target in WIDTHS:
        check_views(g, name, target, views_of(target[3]), name, spline_degree=SOURCES[name][5])


@pytest.mark.parametrize("name", ["latlon d3 n3", "rectilinear lens"])
@pytest.mark.parametrize("twine", [2, 3])
def test_twining(name, twine):
    """the x-biased columns and the second row variant: rectilinear, lat/lon across a segment boundary, cubemap,
    cylindrical (its normalisation reads the lane's first column of the segment) and fisheye targets"""
    g = pair(name)[1]
    for target in [TARGETS[2], TARGETS[5], TARGETS[0], TARGETS[3], TARGETS[6]]:
        check_views(g, name, target, views_of(target[3]), f"{name} twine {twine}", spline_degree=SOURCES[name][5],
                    twine=twine)


@pytest.mark.parametrize("src_n,out_n", [(3, 4), (4, 1)])
def test_channel_adaption(src_n, out_n):
    img = jobs.synth_image(128, 64, src_n, seed=4)
    if src_n == 4:
        img[:, :, 3] = (np.indices((64, 128))[1] % 7 != 0).astype(np.float32)
    g = make_pair(euo.RECTILINEAR, 128, 64, 100.0, img, 1, brighten=1.3)[1]
    target = (ea.SPHERICAL, 150, 75, 360.0)
    check_views(g, f"repix rect {src_n}", target, views_of(360.0), f"repix {src_n}->{out_n}", nch=out_n, spline_degree=1)
    check_views(g, f"repix rect {src_n}", target, views_of(360.0), f"repix {src_n}->{out_n} twined", nch=out_n,
                spline_degree=1, twine=2)
    # and a source of the packed kind: channel adaption sends it through the general form
    img = jobs.synth_image(SRC_W, SRC_H, src_n, seed=4)
    g = make_pair(euo.SPHERICAL, SRC_W, SRC_H, 360.0, img, 3)[1]
    check_views(g, f"repix latlon {src_n}", TARGETS[2], views_of(90.0), f"repix {src_n}->{out_n}, lat/lon", nch=out_n,
                spline_degree=3)


def test_mask_for_source():
    """a --mask_for source paints the facet at the inner evaluation: the general form, also for a packed kind of source"""
    for nch, masked in ((3, 1), (4, 0)):
        img = jobs.synth_image(64, 32, nch)
        g = ea.Source.load(ea.facet_spec(ea.SPHERICAL, 64, 32, 360.0, nchannels=nch, masked=masked), img, 1)
        for target in (TARGETS[2], TARGETS[1]):
            got = check_views(g, f"mask {nch} {masked}", target, views_of(target[3]), "--mask_for", distinct=False,
                              spline_degree=1)
            assert (got[..., 0] == float(masked)).any()
    g = ea.Source.load(ea.facet_spec(ea.RECTILINEAR, 64, 48, 70.0, nchannels=4, masked=1), jobs.synth_image(64, 48, 4), 1)
    check_views(g, "mask rect", TARGETS[1], views_of(360.0), "--mask_for 4 -> 2", nch=2, spline_degree=1)


# ---- layout -----------------------------------------------------------------------------------------------------

SENTINEL = np.float32(-12345.5)
LAYOUT_TARGET = TARGETS[2]          # rectilinear 129 x 97


def layout_job():
    g = pair("latlon d3 n3")[1]
    a = ea.arguments(*LAYOUT_TARGET, spline_degree=3)
    views = views_of(LAYOUT_TARGET[3])
    refs = [reference(g, "latlon d3 n3", LAYOUT_TARGET, v, spline_degree=3) for v in views]
    return g, a, views, refs


def test_one_view_and_no_view():
    g, a, views, refs = layout_job()
    got = ea.render_views(a, views[1:2], g)
    assert got.shape == (1, 97, 129, 3)
    assert_bits(got[0], refs[1], "one view")
    assert ea.render_views(a, [], g).shape == (0, 97, 129, 3)
    # no view, and a buffer that could hold one: untouched
    buf = np.full((1, 97, 129, 3), SENTINEL, np.float32)
    t = a.target(3)
    arr = (ea.View * 1)()
    rc = ea.lib().eu_hip_render_views(C.byref(t), arr, 0, g.handle, buf.ctypes.data, 129 * 12, 97 * 129 * 12, 0, None)
    assert rc == 0
    assert (buf == SENTINEL).all()


@pytest.mark.parametrize("general", [False, True])
def test_padded_rows_and_views_numpy(general, monkeypatch):
    if general:
        monkeypatch.setenv("EU_HIP_KERNEL", "1")
    g, a, views, refs = layout_job()
    big = np.full((3, 97 + 2, 129 + 5, 3), SENTINEL, np.float32)
    out = big[:, :97, :129]
    assert ea.render_views(a, views, g, out=out) is out
    for k in range(3):
        assert_bits(np.ascontiguousarray(out[k]), refs[k], f"padded, view {k}")
    assert (big[:, 97:] == SENTINEL).all() and (big[:, :, 129:] == SENTINEL).all(), "the padding of `out` was written"


@pytest.mark.parametrize("general", [False, True])
def test_torch_output_padding_and_stream(general, monkeypatch):
    import torch
    if general:
        monkeypatch.setenv("EU_HIP_KERNEL", "1")
    g, a, views, refs = layout_job()
    dev = torch.device("cuda")
    # dense, on the library's stream
    out_t = torch.full((3, 97, 129, 3), -1.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    assert ea.render_views(a, views, g, out=out_t) is out_t
    ea.sync()
    for k in range(3):
        assert_bits(out_t[k].cpu().numpy(), refs[k], f"torch dense, view {k}")
    # padded rows and views, on a stream of the caller's
    big = torch.full((3, 97 + 1, 129 + 3, 3), float(SENTINEL), dtype=torch.float32, device=dev)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    ea.render_views(a, views, g, out=big[:, :97, :129], stream=stream.cuda_stream)
    ea.sync()
    host = big.cpu().numpy()
    for k in range(3):
        assert_bits(np.ascontiguousarray(host[k, :97, :129]), refs[k], f"torch padded, view {k}")
    assert (host[:, 97:] == SENTINEL).all() and (host[:, :, 129:] == SENTINEL).all(), "the padding of `out` was written"


@pytest.mark.parametrize("on_device", [False, True])
def test_chunks_give_the_same_bits(on_device, monkeypatch):
    """five views whose tables (12408 bytes each) fit a 25 KiB bound two at a time: three chunks"""
    import torch
    g, a, _, _ = layout_job()
    assert (6 * 129 + 24 * 97) * 4 == 12408
    views = [(12.0 * k, 5.0 * k - 10.0, 3.0 * k, 90.0 - 4 * k) for k in range(5)]

    def run():
        if not on_device:
            return ea.render_views(a, views, g)
        out_t = torch.zeros((5, 97, 129, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ea.render_views(a, views, g, out=out_t)
        ea.sync()
        return out_t.cpu().numpy()

    one = run()
    monkeypatch.setenv("EU_HIP_VIEWS_MAX_KB", "25")
    three = run()
    assert_bits(three, one, "three chunks against one")
    for k, v in enumerate(views):
        assert_bits(one[k], reference(g, "latlon d3 n3", LAYOUT_TARGET, v, spline_degree=3), f"view {k}")


def test_render_and_its_caches_are_left_alone():
    """job J through ea.render, render_views with other cameras of the same target, J again: the launch counter
    counts the renders alone, and J's frame has the same bits"""
    g, a, views, _ = layout_job()
    j = ea.arguments(*LAYOUT_TARGET, yaw=11, pitch=-7, roll=3, spline_degree=3)
    first = ea.render(j, g)
    n1 = ea.launch_count()
    ea.render_views(a, views, g)
    ea.render_views(ea.arguments(*LAYOUT_TARGET, spline_degree=3, twine=2), views, g)
    assert ea.launch_count() == n1
    again = ea.render(j, g)
    assert ea.launch_count() > n1
    assert_bits(again, first, "the job after render_views calls")


def test_two_caller_streams_with_a_render_between():
    """views on stream A, a render on the library's stream (it takes over the library's one `last user` slot), other
    views on stream B: the second call must not rewrite the tables under the first"""
    import torch
    g, a, views, refs = layout_job()
    others = [(12.0 * k, 5.0 * k - 10.0, 3.0 * k) for k in range(1, 4)]
    j = ea.arguments(*LAYOUT_TARGET, yaw=11, pitch=-7, roll=3, spline_degree=3)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    out_a = torch.zeros((3, 97, 129, 3), dtype=torch.float32, device="cuda")
    out_b = torch.zeros((3, 97, 129, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ea.render_views(a, views, g, out=out_a, stream=sa.cuda_stream)
    between = ea.render(j, g)
    ea.render_views(a, others, g, out=out_b, stream=sb.cuda_stream)
    ea.sync()
    torch.cuda.synchronize()
    for k in range(3):
        assert_bits(out_a[k].cpu().numpy(), refs[k], f"stream A, view {k}")
        assert_bits(out_b[k].cpu().numpy(), reference(g, "latlon d3 n3", LAYOUT_TARGET, others[k], spline_degree=3),
                    f"stream B, view {k}")
    assert_bits(between, reference(g, "latlon d3 n3", LAYOUT_TARGET, (11, -7, 3), spline_degree=3), "the render between")


# ---- refusals ---------------------------------------------------------------------------------------------------

def test_unsupported_jobs():
    img = jobs.synth_image(64, 48, 3)
    g = ea.Source.load(ea.facet_spec(ea.RECTILINEAR, 64, 48, 70.0, translation=dict(x=0.1, z=0.05)), img, 1)
    with pytest.raises(ea.EuError, match="error -3.*translation"):
        ea.render_views(ea.arguments(ea.SPHERICAL, 64, 32, 360.0), [(0, 0, 0)], g)
    g = pair("latlon d1 n3")[1]
    a = ea.arguments(ea.BIATAN6, 24, 144, 90.0)
    assert math.tan(math.radians(135.0 / 2)) > 1.75
    with pytest.raises(ea.EuError, match="error -3.*1.75"):
        ea.render_views(a, [(0, 0, 0), (0, 0, 0, 135.0)], g)
    with pytest.raises(ea.EuError, match="error -3.*1.75"):
        ea.view_tables(a, (0, 0, 0, 135.0), g)
    # inside the range the same call renders
    assert ea.render_views(a, [(0, 0, 0), (0, 0, 0, 100.0)], g).shape == (2, 144, 24, 3)
