"""Radiance RGBE pixels on the device (eu_hip_source_load_rgbe, eu_hip_encode_rgbe, eu_hip_render_rgbe, eu_rgbe.hip;
Source.load_rgbe, encode_rgbe, render_rgbe). What is expected comes from tests/rgbe_model.py, a numpy float32 model
written from the format's definition - not from the library's host functions. 1: the container of load_rgbe is, bit
for bit, Source.load of the model's floats. A thread of the decode owns four floats of a destination row behind the
row's first 16-byte boundary, so widths, channel counts and container pitches are chosen for every alignment. 2: the
quads of encode_rgbe are the model's, byte for byte, with every byte outside the rows checked. 3: render_rgbe equals
encode_rgbe of render's float frame. 4: a render_views result, encoded in one call."""
import ctypes as C

import numpy as np
import pytest

import envutil_amd as ea
from envutil_amd import api
import jobs
import pixel_values as pv
import rgbe_model as rm

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xA5


def bits_of(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_container(a, b, what):
    ca, cb = a.download(), b.download()
    assert ca.shape == cb.shape, what
    bad = int((bits_of(ca) != bits_of(cb)).sum())
    assert bad == 0, f"{what}: {bad} of {ca.size} floats differ"


def make_quads(h, w, seed):
    """random quads: exponent bytes over 0 .. 255 - zero exponents with mantissas that are not zero included, and,
    as far as the size allows, every exponent byte"""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    flat = q.reshape(-1, 4)
    k = min(len(flat), 256)
    flat[rng.permutation(len(flat))[:k], 3] = rng.permutation(256).astype(np.uint8)[:k]
    flat[rng.integers(0, len(flat)), 3] = 0
    return q


def srgb_table():
    """a table that is not the decode: the sRGB curve over the decoded values (clipped, so that it is finite)"""
    e, m = np.mgrid[0:256, 0:256]
    v = rm.decode(np.stack([m, m, m, e], -1).astype(np.uint8))[..., 0].reshape(-1).astype(np.float64)
    v = np.minimum(v, 1e10)
    t = np.where(v <= 0.04045, v / 12.92, ((v + 0.055) / 1.055) ** 2.4)
    return np.ascontiguousarray(t, np.float32)


def table_floats(q, table):
    idx = (q[..., 3].astype(np.int64)[..., None] << 8) | q[..., :3]
    return np.ascontiguousarray(table[idx], np.float32)


def flat_facet(w, h, nch=3):
    return ea.facet_spec(ea.RECTILINEAR, w, h, 60.0, nchannels=nch)


def check_load(fct, q, degree, what, table=None, device=False, **edit):
    floats = rm.decode(q) if table is None else table_floats(q, table)
    want = ea.Source.load(fct, floats, degree, **edit)
    given = q
    if device:
        import torch
        given = torch.from_numpy(q).to("cuda:0")
        assert given.data_ptr() % 4 == 0
    got = ea.Source.load_rgbe(fct, given, table, spline_degree=degree, **edit)
    same_container(got, want, what)


# ---------------------------------------------------------------------------------------------------- load
@pytest.mark.parametrize("nch", [3, 4])
def test_load_flat_facets(nch):
    """degree 1: no prefilter, the container's core holds the decoded floats themselves (pitch = width + frame)"""
    k = 0
    for h in range(1, 10):
        for w in (1, 3, 5, 63, 64, 65, 257):
            check_load(flat_facet(w, h, nch), make_quads(h, w, 100 * h + w), 1, (w, h, nch), device=k % 2 == 1)
            k += 1


def test_load_degree_3_and_window():
    for w, h in ((5, 3), (65, 9), (257, 4)):
        for nch in (3, 4):
            check_load(flat_facet(w, h, nch), make_quads(h, w, w + nch), 3, (w, h, nch, "degree 3"))
    # a window whose container pitch differs from the width
    fct = ea.facet_spec(ea.RECTILINEAR, 200, 100, 70.0, nchannels=3, window=(67, 45, 20, 10))
    check_load(fct, make_quads(45, 67, 8), 3, "window")
    check_load(fct, make_quads(45, 67, 9), 3, "window, device quads", device=True)


def test_load_full_sphere_and_cubemaps():
    for nch in (3, 4):
        check_load(ea.facet_spec(ea.SPHERICAL, 6, 3, 360.0, nchannels=nch), make_quads(3, 6, nch), 3, ("6 x 3 sphere", nch))
    for face in (8, 64):
        fct = ea.facet_spec(ea.CUBEMAP, face, 6 * face, 90.0)
        check_load(fct, make_quads(6 * face, face, face), 3, ("cubemap", face), device=face == 8)


def test_load_with_masks_and_crop():
    """4 channels with a polygon mask and an elliptic crop: the decode writes the dense buffer the edit reads"""
    for (w, h), device in (((67, 45), False), ((130, 77), True)):
        poly = [(np.array([0.1, 0.7, 0.5, 0.2]) * w, np.array([0.2, 0.1, 0.8, 0.6]) * h)]
        crop = (w // 10, w - w // 8, h // 9, h - h // 7)
        fct = ea.facet_spec(ea.FISHEYE, w, h, 120.0, nchannels=4)
        q = make_quads(h, w, w)
        q[..., 3] = 118 + q[..., 3] % 20          # finite through the binomial and the prefilter
        check_load(fct, q, 3, ("edit", w, h), device=device, masks=poly, crop=crop, crop_kind=2)
        check_load(fct, q, 1, ("mask only", w, h), device=device, masks=poly)
    with pytest.raises(ea.EuError):
        ea.Source.load_rgbe(flat_facet(67, 45, 3), q[:45, :67], spline_degree=1, masks=poly)


def test_load_through_a_table():
    table = srgb_table()
    for w, h, nch, device in ((65, 9, 3, False), (63, 5, 4, True), (257, 3, 3, True)):
        q = make_quads(h, w, w + 1)
        assert (bits_of(table_floats(q, table)) != bits_of(rm.decode(q))).any()
        check_load(flat_facet(w, h, nch), q, 3, ("table", w, h, nch), table=table, device=device)


def test_render_from_an_rgbe_source():
    """spherical 256 x 128 to a 64-wide cubemap, degree 3: the same frame from either source"""
    q = make_quads(128, 256, 4)
    q[..., 3] = 120 + q[..., 3] % 16
    fct = ea.facet_spec(ea.SPHERICAL, 256, 128, 360.0)
    args = ea.arguments(ea.CUBEMAP, 64, 384, 90.0, spline_degree=3)
    got = ea.render(args, ea.Source.load_rgbe(fct, q, spline_degree=3))
    want = ea.render(args, ea.Source.load(fct, rm.decode(q), 3))
    assert (bits_of(got) == bits_of(want)).all() and np.isfinite(got).all()


# ---------------------------------------------------------------------------------------------------- encode
def value_pool():
    """the targeted list of the CPU test and the fields of tests/pixel_values.py: the range of an HDR panorama,
    signed data with both zeros, denormals, +-1e37, inf / NaN / +-3e38 texels"""
    parts = [rm.targeted().reshape(-1)]
    for cls in pv.FINITE:
        parts.append(pv.make(cls, 8, 16, 3).reshape(-1))
    parts.append(pv.make("nonfinite", 16, 32, 3, one_in=10).reshape(-1))
    return np.concatenate([np.ascontiguousarray(p, np.float32) for p in parts]).reshape(-1, 3)


def frame_from(pool, h, w, seed):
    idx = (np.arange(h * w) * 7 + seed * 131) % len(pool)
    return pool[idx].reshape(h, w, 3).copy()


def encode_raw(frame, frame_mode, out_dev, pad):
    """eu_hip_encode_rgbe through ctypes, `out` in a buffer filled with 0xA5 with GUARD bytes either side and `pad`
    bytes behind every row. frame_mode: 0 host dense, 1 host padded, 2 device dense, 3 device padded. Returns the
    whole buffer afterwards and the row stride."""
    import torch
    h, w, _ = frame.shape
    stride = w * 4 + pad
    total = GUARD + h * stride + GUARD
    fpad = 3 if frame_mode in (1, 3) else 0
    fhost = np.full((h, w * 3 + fpad), np.float32(0.25), np.float32)
    fhost[:, :w * 3] = frame.reshape(h, -1)
    keep = [fhost]
    if frame_mode >= 2:
        ft = torch.from_numpy(fhost).cuda()
        keep.append(ft)
        fptr = ft.data_ptr()
    else:
        fptr = fhost.ctypes.data
    if out_dev:
        ot = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
        optr = ot.data_ptr() + GUARD
    else:
        oh = np.full(total + 4, FILL, np.uint8)
        skip = (-oh.ctypes.data) % 4
        oh = oh[skip:skip + total]
        optr = oh.ctypes.data + GUARD
    torch.cuda.synchronize()
    rc = api.lib().eu_hip_encode_rgbe(C.c_void_p(fptr), fhost.shape[1] * 4, int(frame_mode >= 2), w, h, C.c_void_p(optr),
                                      stride, int(out_dev), None)
    assert rc == 0, api.lib().eu_hip_last_error().decode()
    ea.sync()
    return (ot.cpu().numpy() if out_dev else oh), stride


def check_buffer(buf, stride, want, what):
    h, row = want.shape
    body = buf[GUARD:GUARD + h * stride].reshape(h, stride)
    bad = np.argwhere((body[:, :row] != want))
    assert not bad.size, f"{what}: {len(bad)} of {want.size} bytes differ, first at {tuple(bad[0])}"
    outside = buf.copy()
    outside[GUARD:GUARD + h * stride].reshape(h, stride)[:, :row] = FILL
    assert (outside == FILL).all(), f"{what}: {int((outside != FILL).sum())} bytes outside the rows were written"


def test_encode_against_the_model():
    pool = value_pool()
    k = 0
    for h in (1, 2, 17):
        for w in (1, 63, 65, 257):
            frame = frame_from(pool, h, w, w + 1000 * h)
            want = rm.encode(frame).reshape(h, -1)
            for pad in (0, 4, 20):
                buf, stride = encode_raw(frame, k % 4, True, pad)
                check_buffer(buf, stride, want, (w, h, pad, k % 4))
                k += 1
            buf, stride = encode_raw(frame, k % 4, False, 8)
            check_buffer(buf, stride, want, (w, h, "host out", k % 4))


def test_encode_every_targeted_pixel():
    """the whole pool in one frame, through the Python entry: host and device, both ways"""
    import torch
    pool = value_pool()
    n = len(pool) // 64 * 64
    frame = pool[:n].reshape(-1, 64, 3)
    want = rm.encode(frame)
    assert (want[..., 3] == 255).any() and (want == 0).all(-1).any() and len(np.unique(want[..., 3])) > 230
    got = ea.encode_rgbe(frame)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    t = torch.from_numpy(frame).cuda()
    dev = ea.encode_rgbe(t)
    ea.sync()
    assert dev.is_cuda and dev.dtype == torch.uint8 and np.array_equal(dev.cpu().numpy(), want)
    assert np.array_equal(ea.encode_rgbe(t, out=np.zeros(want.shape, np.uint8)), want)
    dev = ea.encode_rgbe(frame, out=torch.zeros(want.shape, dtype=torch.uint8, device="cuda"))
    ea.sync()
    assert np.array_equal(dev.cpu().numpy(), want)


def test_encode_more_rows_than_a_launch_has_workgroups():
    """a launch has at most 65535 workgroups of 8 rows each along y: a taller frame is walked in strides"""
    frame = frame_from(value_pool(), 8 * 65535 + 77, 2, 3)
    assert np.array_equal(ea.encode_rgbe(frame), rm.encode(frame))


# ---------------------------------------------------------------------------------------------------- render
@pytest.fixture(scope="module")
def pano():
    """a lat/lon source over the range of an HDR panorama, with negative values"""
    img = jobs.synth_image(256, 128, 3)
    img = (img * np.float32(1.8) - np.float32(0.35)) * pv.hdr(128, 256, 1)
    return ea.Source.load(ea.facet_spec(ea.SPHERICAL, 256, 128, 360.0), np.ascontiguousarray(img, np.float32), 3)


@pytest.fixture(scope="module")
def fisheye():
    img = jobs.synth_image(96, 96, 3, seed=5) * np.float32(900.0) - np.float32(100.0)
    return ea.Source.load(ea.facet_spec(ea.FISHEYE, 96, 96, 170.0), img, 4)


@pytest.fixture(scope="module")
def three_facets():
    out = []
    for k, yaw in enumerate((-40.0, 0.0, 40.0)):
        img = jobs.synth_image(96, 64, 3, seed=3 + k) * np.float32(2.0 ** (4 * k)) - np.float32(0.2)
        out.append(ea.Source.load(ea.facet_spec(ea.RECTILINEAR, 96, 64, 70.0, yaw=yaw, pitch=3.0 * k), img, 1))
    return out


def same_as_encode_of_render(args, sources, what, **kw):
    frame = ea.render(args, sources, **kw)
    want = ea.encode_rgbe(frame)
    assert np.array_equal(want, rm.encode(frame)), what
    got = ea.render_rgbe(args, sources, **kw)
    assert got.shape == frame.shape[:2] + (4,) and got.dtype == np.uint8
    assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} of {got.size} bytes differ"
    assert len(np.unique(got[..., 3])) > 2, what
    return frame


def test_render_rgbe_staged_single_facet(pano):
    same_as_encode_of_render(ea.arguments(ea.CUBEMAP, 32, 192, 90.0, spline_degree=3), pano, "cubemap 32")
    same_as_encode_of_render(ea.arguments(ea.SPHERICAL, 120, 60, 360.0, spline_degree=3, crop=(13, 78, 7, 40)), pano, "crop")
    args = ea.arguments(ea.CUBEMAP, 32, 192, 90.0, spline_degree=3)
    same_as_encode_of_render(args, pano, "rows 37 .. 150", row_begin=37, row_end=150)
    same_as_encode_of_render(args, pano, "bands", band=(4, 2, 1))
    assert ea.render_rgbe(args, pano, row_begin=7, row_end=7).shape == (0, 32, 4)


def test_render_rgbe_general_kernel(fisheye):
    args = ea.arguments(ea.RECTILINEAR, 65, 33, 80.0, yaw=30, pitch=-12, roll=5, spline_degree=4)
    same_as_encode_of_render(args, fisheye, "fisheye source, degree 4")
    same_as_encode_of_render(args, fisheye, "rows 5 .. 22", row_begin=5, row_end=22)
    same_as_encode_of_render(ea.arguments(ea.RECTILINEAR, 130, 66, 80.0, spline_degree=4, crop=(13, 78, 7, 40)), fisheye, "crop")
    same_as_encode_of_render(ea.arguments(ea.RECTILINEAR, 65, 33, 80.0, spline_degree=4, twine=2), fisheye, "twined")


def test_render_rgbe_three_facets(three_facets):
    args = ea.arguments(ea.SPHERICAL, 130, 47, 170.0, spline_degree=1)
    frame = same_as_encode_of_render(args, three_facets, "three facets")
    assert (frame == 0).all(-1).any() and (frame > 100).any()
    same_as_encode_of_render(args, three_facets, "three facets, rows", row_begin=9, row_end=31)
    same_as_encode_of_render(ea.arguments(ea.SPHERICAL, 260, 94, 170.0, spline_degree=1, crop=(40, 190, 11, 80)), three_facets,
                             "three facets, crop")


def test_render_rgbe_four_chunks_to_the_host(pano):
    """1030 rows: the pipeline of four row chunks; a padded host buffer keeps its padding"""
    args = ea.arguments(ea.SPHERICAL, 8, 1030, 20.0, spline_degree=1)
    frame = same_as_encode_of_render(args, pano, "8 x 1030")
    big = np.full((1030, 8 * 4 + 8), FILL, np.uint8)
    out = big[:, :32].reshape(1030, 8, 4)
    assert np.shares_memory(out, big)
    ea.render_rgbe(args, pano, out=out)
    assert np.array_equal(out, rm.encode(frame)) and (big[:, 32:] == FILL).all()


def test_render_rgbe_wants_three_channels(pano):
    with pytest.raises(ea.EuError):
        ea.render_rgbe(ea.arguments(ea.RECTILINEAR, 65, 33, 80.0), pano, nchannels=4)


def test_render_rgbe_device_out_on_a_stream(pano):
    import torch
    args = ea.arguments(ea.RECTILINEAR, 65, 33, 80.0, yaw=10, spline_degree=3)
    other_args = ea.arguments(ea.RECTILINEAR, 65, 33, 80.0, yaw=-70, spline_degree=3)
    want = rm.encode(ea.render(args, pano))
    other_want = rm.encode(ea.render(other_args, pano))
    assert not np.array_equal(want, other_want)
    stream = torch.cuda.Stream()
    big = torch.full((33, 65 + 2, 4), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    out = big[:, :65]
    ea.render_rgbe(args, pano, out=out, stream=stream.cuda_stream)
    # work behind it on that stream, and another job on the library's own stream right behind it: it rewrites the
    # frame buffer, and waits for the first call before it does
    with torch.cuda.stream(stream):
        copy = out.clone()
    other = ea.render_rgbe(other_args, pano)
    again = torch.empty((33, 65, 4), dtype=torch.uint8, device="cuda")
    ea.render_rgbe(args, pano, out=again, stream=stream.cuda_stream)
    stream.synchronize()
    ea.sync()
    host = big.cpu().numpy()
    assert np.array_equal(host[:, :65], want) and (host[:, 65:] == 0x5A).all()
    assert np.array_equal(copy.cpu().numpy(), want) and np.array_equal(again.cpu().numpy(), want)
    assert np.array_equal(other, other_want)


# ---------------------------------------------------------------------------------------------------- views
def test_encode_of_a_render_views_result(pano):
    """four views of 33 x 17 in device memory: the N * H rows in one call equal the per-view encodes"""
    import torch
    args = ea.arguments(ea.RECTILINEAR, 33, 17, 70.0, spline_degree=3)
    views = [(0, 0, 0), (40, 10, 0), (-90, -20, 15), (170, 5, -5, 50.0)]
    frames = torch.zeros((4, 17, 33, 3), dtype=torch.float32, device="cuda")
    ea.render_views(args, views, pano, out=frames)
    quads = ea.encode_rgbe(frames)
    ea.sync()
    host = frames.cpu().numpy()
    assert quads.shape == (4, 17, 33, 4) and np.array_equal(quads.cpu().numpy(), rm.encode(host))
    for k in range(4):
        one = ea.encode_rgbe(frames[k])
        ea.sync()
        assert np.array_equal(one.cpu().numpy(), quads[k].cpu().numpy()), k
        assert np.array_equal(ea.encode_rgbe(host[k]), one.cpu().numpy()), k
    assert len({quads[k].cpu().numpy().tobytes() for k in range(4)}) == 4
