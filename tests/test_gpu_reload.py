"""eu_hip_source_reload (Source.reload, reload_samples, reload_rgbe, reload_ycbcr): new pixels into a resident
container. After a reload the container is, bit for bit, the one the matching load builds from the same pixels -
core, frame, brace, a cubemap's support frame - whatever stood there before (a container full of NaN included); the
slack behind it is still zero, the device address is the same, and renders see the new picture through every cache
that is keyed on the source. Every feed, flat and spherical facets, cubemaps, edits, sources made by adopt and alloc,
host and device pixels; the scratch is reused, released and made again; copies on other device slots are dropped."""
import ctypes as C

import numpy as np
import pytest

import envutil_amd as ea
import jobs
import pixel_values as pv
import ycbcr_model as ym

pytestmark = pytest.mark.gpu


def bits_of(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_container(a, b, what):
    """a's container is b's: the same NaN mask (none, for finite pixels) and the same bits everywhere else"""
    pv.assert_bits_nan(a.download(), b.download(), what)


def slack_floats(src):
    g, nch = src.info()
    return 4 * g.shape[0] * nch + 64 * 4


def read_slack(src):
    ptr, n = src.device_ptr()
    out = np.ones(slack_floats(src), np.float32)
    assert ea.lib().eu_hip_memcpy_d2h(out.ctypes.data, C.c_void_p(ptr + 4 * n), out.nbytes) == 0
    return out


def poison(src):
    """the whole container NaN (the slack stays)"""
    ptr, n = src.device_ptr()
    nan = np.full(n, np.nan, np.float32)
    ea.sync()
    assert ea.lib().eu_hip_memcpy_h2d(C.c_void_p(ptr), nan.ctypes.data, nan.nbytes) == 0
    assert np.isnan(src.download()).all()


def to_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def check_reload(src, reload, fresh, what):
    """`reload` refills src, `fresh` loads the same pixels anew: the same container at the same address, zero slack"""
    ptr = src.device_ptr()
    reload(src)
    ea.sync()
    want = fresh()
    same_container(src, want, what)
    assert src.device_ptr() == ptr, what
    assert not read_slack(src).view(np.uint32).any(), f"{what}: the slack behind the container is no longer zero"
    return want


def facets():
    """(name, facet at 3 channels, frame width, frame height)"""
    return [("flat", ea.facet_spec(ea.RECTILINEAR, 67, 45, 70.0), 67, 45),
            ("window", ea.facet_spec(ea.RECTILINEAR, 200, 100, 70.0, window=(65, 41, 20, 10)), 65, 41),
            ("sphere", ea.facet_spec(ea.SPHERICAL, 64, 32, 360.0), 64, 32),
            ("small sphere", ea.facet_spec(ea.SPHERICAL, 6, 3, 360.0), 6, 3),
            ("cubemap", ea.facet_spec(ea.CUBEMAP, 20, 120, 90.0), 20, 120)]


@pytest.mark.parametrize("degree", [1, 3])
def test_reload_floats(degree):
    rng = np.random.default_rng(degree)
    for name, fct, w, h in facets():
        a, b, c = (rng.random((h, w, 3), dtype=np.float32) for _ in range(3))
        src = ea.Source.load(fct, a, degree)
        check_reload(src, lambda s: s.reload(b), lambda: ea.Source.load(fct, b, degree), (name, "host floats"))
        poison(src)
        check_reload(src, lambda s: s.reload(to_device(c)), lambda: ea.Source.load(fct, c, degree), (name, "device floats over NaN"))
        poison(src)
        check_reload(src, lambda s: s.reload(a), lambda: ea.Source.load(fct, a, degree), (name, "host floats over NaN"))


def test_reload_samples_rgbe_ycbcr_over_nan():
    rng = np.random.default_rng(11)
    m = ea.ycbcr_matrix("709")
    for name, fct, w, h in facets():
        src = ea.Source.load(fct, rng.random((h, w, 3), dtype=np.float32), 3)
        for device in (False, True):
            give = to_device if device else (lambda x: x)
            s8 = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            poison(src)
            check_reload(src, lambda s: s.reload_samples(give(s8)), lambda: ea.Source.load_samples(fct, s8, spline_degree=3),
                         (name, "8-bit samples", device))
            s16 = rng.integers(0, 65536, (h, w, 3)).astype(np.uint16)
            table = rng.random(65536, dtype=np.float32)
            poison(src)
            check_reload(src, lambda s: s.reload_samples(give(s16), table),
                         lambda: ea.Source.load_samples(fct, s16, table, spline_degree=3), (name, "16-bit samples, a table", device))
            q = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
            q[..., 3] = 120 + q[..., 3] % 16
            poison(src)
            check_reload(src, lambda s: s.reload_rgbe(give(q)), lambda: ea.Source.load_rgbe(fct, q, spline_degree=3),
                         (name, "rgbe", device))
            y, cb, cr = ym.planes(rng, h, w, 2, 2, 8, "nv12", 1)
            planes = (on_device_view(y), (on_device_view(cb), on_device_view(cr))) if device else (y, (cb, cr))
            poison(src)
            want = check_reload(src, lambda s: s.reload_ycbcr(planes[0], planes[1], m),
                                lambda: ea.Source.load_ycbcr(fct, y, (cb, cr), m, spline_degree=3), (name, "ycbcr", device))
            same_container(want, ea.Source.load(fct, ym.floats(y, cb, cr, 2, 2, *ea.ycbcr_tables(8), m), 3), (name, "ycbcr model"))
        ea.reload_scratch_release()        # and the next facet's reloads make it again


def on_device_view(a):
    import torch
    base = a
    while base.base is not None:
        base = base.base
    t = torch.from_numpy(np.ascontiguousarray(base)).to("cuda:0")
    off = (a.__array_interface__["data"][0] - base.__array_interface__["data"][0]) // a.itemsize
    return t.reshape(-1).as_strided(a.shape, tuple(s // a.itemsize for s in a.strides), off)


def test_reload_with_masks_and_crop():
    """4 channels, a polygon mask and an elliptic crop, every feed: the dense buffer in front of the edit is scratch"""
    rng = np.random.default_rng(12)
    w, h = 67, 45
    poly = [(np.array([0.1, 0.7, 0.5, 0.2]) * w, np.array([0.2, 0.1, 0.8, 0.6]) * h)]
    edit = dict(masks=poly, crop=(w // 10, w - w // 8, h // 9, h - h // 7), crop_kind=2)
    m = ea.ycbcr_matrix("601")
    for name, fct in (("fisheye", ea.facet_spec(ea.FISHEYE, w, h, 120.0, nchannels=4)),):
        src = ea.Source.load(fct, rng.random((h, w, 4), dtype=np.float32), 3)
        for device in (False, True):
            give = to_device if device else (lambda x: x)
            f3 = rng.random((h, w, 3), dtype=np.float32)
            poison(src)
            check_reload(src, lambda s: s.reload(give(f3), **edit), lambda: ea.Source.load(fct, f3, 3, **edit), (name, "floats", device))
            f4 = rng.random((h, w, 4), dtype=np.float32)
            check_reload(src, lambda s: s.reload(give(f4), masks=poly), lambda: ea.Source.load(fct, f4, 3, masks=poly), (name, "4 floats", device))
            check_reload(src, lambda s: s.reload(give(f3)), lambda: ea.Source.load(fct, f3, 3), (name, "a gained channel alone", device))
            s8 = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            poison(src)
            check_reload(src, lambda s: s.reload_samples(give(s8), **edit), lambda: ea.Source.load_samples(fct, s8, spline_degree=3, **edit),
                         (name, "samples", device))
            q = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
            q[..., 3] = 120 + q[..., 3] % 16
            check_reload(src, lambda s: s.reload_rgbe(give(q), **edit), lambda: ea.Source.load_rgbe(fct, q, spline_degree=3, **edit),
                         (name, "rgbe", device))
            y, cb, cr = ym.planes(rng, h, w, 2, 2, 8, "planar")
            check_reload(src, lambda s: s.reload_ycbcr(give(y), (give(cb), give(cr)), m, **edit),
                         lambda: ea.Source.load_ycbcr(fct, y, (cb, cr), m, spline_degree=3, **edit), (name, "ycbcr", device))
    with pytest.raises(ea.EuError, match="channels"):
        ea.Source.load(ea.facet_spec(ea.RECTILINEAR, w, h, 70.0), f3, 1).reload(f3, masks=poly)


def test_adopted_and_allocated_sources_reload_with_the_bcs_they_hold():
    rng = np.random.default_rng(13)
    fct = ea.facet_spec(ea.SPHERICAL, 64, 32, 360.0)
    a, b = (rng.random((32, 64, 3), dtype=np.float32) for _ in range(2))
    loaded = ea.Source.load(fct, a, 3)
    adopted = ea.Source.adopt(fct, loaded.download(), 3, ea.BC_PERIODIC, ea.BC_REFLECT)
    check_reload(adopted, lambda s: s.reload(b), lambda: ea.Source.load(fct, b, 3), "adopted")
    allocated = ea.Source.alloc(fct, 3)
    check_reload(allocated, lambda s: s.reload(b), lambda: ea.Source.load(fct, b, 3), "allocated")
    # other boundary conditions than a load picks: the refill keeps them
    flat = ea.facet_spec(ea.RECTILINEAR, 64, 32, 70.0)
    mirror = ea.Source.adopt(flat, ea.Source.load(flat, a, 3).download(), 3, ea.BC_MIRROR, ea.BC_MIRROR)
    mirror.reload(b)
    ea.sync()
    g, _ = mirror.info()
    got = mirror.download()
    rows = slice(g.left[1], g.left[1] + 32)
    x0 = g.left[0]
    assert g.left[0] >= 1 and np.isfinite(got).all()
    # MIRROR repeats around the edge sample, REFLECT (a load's choice) around the edge: f(-1) = f(1), not f(0)
    assert (bits_of(got[rows, x0 - 1]) == bits_of(got[rows, x0 + 1])).all()
    assert (bits_of(got[rows, x0 - 1]) != bits_of(got[rows, x0])).any()


def test_renders_follow_the_reload_through_every_cache():
    """plans, tables and work lists are keyed on geometry: a reload changes the picture and none of them. Render,
    views, layers, rays and samples before the reload, the same calls after it: the fresh source's results"""
    fct = ea.facet_spec(ea.SPHERICAL, 512, 256, 360.0)
    a, b = jobs.synth_image(512, 256, 3, seed=1), jobs.synth_image(512, 256, 3, seed=2)
    src, fresh = ea.Source.load(fct, a, 3), ea.Source.load(fct, b, 3)
    cube = ea.arguments(ea.CUBEMAP, 96, 576, 90.0, spline_degree=3)
    rect = ea.arguments(ea.RECTILINEAR, 64, 32, 90.0, yaw=30.0, pitch=10.0, spline_degree=3)
    views = [(0, 0, 0), (40, 10, 5)]
    rays = ea.render(rect, src, 3, stage=1)

    def everything(s):
        return [ea.render(cube, s), ea.render(rect, s), ea.render_views(rect, views, s), ea.render_layers(rect, [s, s]),
                ea.render_rays(s, rays), ea.render_samples(rect, s)]

    before = everything(src)
    src.reload(b)
    after, want = everything(src), everything(fresh)
    for k, (x, y, z) in enumerate(zip(after, want, before)):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"call {k} after the reload"
        assert not np.array_equal(x.view(np.uint8), z.view(np.uint8)), f"call {k} shows the old picture"


def test_tables_that_repeat_and_tables_that_change():
    rng = np.random.default_rng(14)
    fct = ea.facet_spec(ea.RECTILINEAR, 65, 9, 60.0)
    src = ea.Source.load(fct, rng.random((9, 65, 3), dtype=np.float32), 1)
    t1, t2 = rng.random(256, dtype=np.float32), rng.random(256, dtype=np.float32)
    for k, table in enumerate((t1, t1, t2, t2, t1)):
        s8 = rng.integers(0, 256, (9, 65, 3), dtype=np.uint8)
        check_reload(src, lambda s: s.reload_samples(to_device(s8), table),
                     lambda: ea.Source.load_samples(fct, s8, table, spline_degree=1), ("frame", k))


def test_reload_drops_the_copies_on_other_device_slots():
    """(last in this file: it leaves the process with three device slots, as tests/test_gpu_multidevice.py does)"""
    ea.lib()
    ea.init_devices([0, 0, 0])
    fct = ea.facet_spec(ea.SPHERICAL, 256, 128, 360.0)
    a, b = jobs.synth_image(256, 128, 3, seed=3), jobs.synth_image(256, 128, 3, seed=4)
    src = ea.Source.load(fct, a, 3)
    args = ea.arguments(ea.RECTILINEAR, 160, 120, 90.0, spline_degree=3)
    assert np.array_equal(bits_of(ea.render_devices(args, src, 3)), bits_of(ea.render(args, src, 3)))
    src.reload(to_device(b))
    want = ea.render(args, ea.Source.load(fct, b, 3), 3)
    assert np.array_equal(bits_of(ea.render_devices(args, src, 3)), bits_of(want)), "the slots render the old copies"
    assert np.array_equal(bits_of(ea.render(args, src, 3)), bits_of(want))
