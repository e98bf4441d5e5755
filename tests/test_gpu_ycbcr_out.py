"""Rendering to the planes of a Y'CbCr frame (eu_hip_encode_ycbcr, eu_hip_render_ycbcr, eu_ycbcr_out.hip;
encode_ycbcr, render_ycbcr). 1: the kernel against the numpy model of tests/ycbcr_out_model.py, through ctypes into
device buffers filled with 0xA5 with guard bytes around every plane and padding behind every row - the WHOLE buffers
are compared, so a stray byte fails. A thread owns an aligned dword of a luma row and the chroma under it, luma and
chroma rows align on their own, so widths, heights, plane offsets and pitches are chosen for every alignment of
both. 2: the staged route of a host frame whose chunk would split a chroma row. 3: render_ycbcr equals ycbcr_planes of
render's float frame. 4: torch tensors in and out."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import envutil_amd as ea
from envutil_amd import api
import jobs
import ycbcr_model as ym
import ycbcr_out_model as om

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 257, 1027)
HEIGHTS = (1, 2, 3, 9, 17)
SUBS = [(1, 1), (2, 1), (1, 2), (2, 2)]
LAYOUTS = ["planar", "nv12", "nv21"]


def encode_raw(frame, lay, forward, shift, y_steps, c_steps, frame_dev=True, planes_dev=True, fpad=0, lead=0):
    """eu_hip_encode_ycbcr through ctypes into the buffers of an om.Layout. The frame's rows are `fpad` floats longer
    than their pixels and start `lead` floats behind an aligned address. Returns the whole buffers afterwards."""
    import torch
    h, w, nch = frame.shape
    stride = w * nch + fpad
    fhost = np.full(lead + h * stride, np.float32(0.25), np.float32)
    fhost[lead:].reshape(h, stride)[:, :w * nch] = frame.reshape(h, -1)
    keep = [fhost]
    if frame_dev:
        ft = torch.from_numpy(fhost).cuda()
        keep.append(ft)
        fptr = ft.data_ptr() + 4 * lead
    else:
        fptr = fhost.ctypes.data + 4 * lead
    ybuf, cbuf = lay.buffers()
    if planes_dev:
        yt, ct = torch.from_numpy(ybuf).cuda(), torch.from_numpy(cbuf).cuda()
        assert yt.data_ptr() % 16 == 0 and ct.data_ptr() % 16 == 0
        base = dict(y_base=yt.data_ptr(), c_base=ct.data_ptr())
    else:
        base = {}
    torch.cuda.synchronize()
    o = api.YcbcrOut(base.get("y_base", ybuf.ctypes.data) + lay.y_at, base.get("c_base", cbuf.ctypes.data) + lay.cb_at,
                     base.get("c_base", cbuf.ctypes.data) + lay.cr_at, lay.y_pitch, lay.c_pitch, lay.c_step, lay.sub_x,
                     lay.sub_y, lay.bits, shift, int(planes_dev), y_steps.ctypes.data, c_steps.ctypes.data,
                     *[float(k) for k in forward])
    rc = api.lib().eu_hip_encode_ycbcr(C.c_void_p(fptr), stride * 4, int(frame_dev), w, h, nch, C.byref(o), None)
    assert rc == 0, api.lib().eu_hip_last_error().decode()
    ea.sync()
    return (yt.cpu().numpy(), ct.cpu().numpy()) if planes_dev else (ybuf, cbuf)


def same_buffers(got, want, what):
    for g, x, name in zip(got, want, ("luma", "chroma")):
        bad = np.flatnonzero(g != x)
        assert not bad.size, (what, name, f"{bad.size} bytes differ, first at", bad[:6], g[bad[:6]], x[bad[:6]])


@pytest.fixture(scope="module")
def tables():
    """per sample size: random step tables that are no formula, the second pair with equal neighbours and a NaN tail"""
    rng = np.random.default_rng(99)
    out = {}
    for bits in (8, 16):
        n = 1 << bits
        out[bits] = [(om.random_steps(rng, bits), om.random_steps(rng, bits, -0.7, 0.7)),
                     (om.random_steps(rng, bits, top=n - n // 5, ties=4), om.random_steps(rng, bits, -0.7, 0.7, top=n - n // 7, ties=4))]
    return out


@pytest.mark.parametrize("sub", SUBS, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("bits", [8, 16])
def test_kernel_against_the_model(bits, layout, sub, tables):
    """every width and height; per width every pair of luma and chroma start offsets (0 .. 3 bytes, 16 bit: 0 and 2);
    shift 0 and 6, 3 and 4 channels, padded pitches, frame rows padded and off the 16-byte boundary, host and device
    memory on either side"""
    rng = np.random.default_rng(bits + 3 * len(layout) + 17 * sub[0] + 31 * sub[1])
    sb = bits // 8
    offs = (0, 1, 2, 3) if bits == 8 else (0, 2)
    k = 0
    for hi, h in enumerate(HEIGHTS):
        for wi, w in enumerate(WIDTHS):
            c_off = offs[(hi + wi) % len(offs)]
            for y_off in offs:
                shift = 6 if k % 3 == 1 else 0
                nch = 4 if k % 5 in (1, 3) else 3
                y_steps, c_steps = tables[bits][k % 2]
                forward = ea.ycbcr_forward(("601", "709", "2020")[k % 3])
                frame = om.random_frame(rng, h, w, nch)
                lay = om.Layout(w, h, sub[0], sub[1], bits, layout, y_off=y_off, c_off=c_off, pad=sb * (k % 4))
                frame_dev, planes_dev = k % 7 != 3, k % 11 != 5
                got = encode_raw(frame, lay, forward, shift, y_steps, c_steps, frame_dev, planes_dev, fpad=(0, 1, 3)[k % 3],
                                 lead=(0, 1)[(k // 2) % 2])
                same_buffers(got, lay.expected(frame, forward, shift, y_steps, c_steps),
                             (w, h, nch, "offsets", y_off, c_off, "shift", shift, "frame/planes on device", frame_dev, planes_dev))
                k += 1


@pytest.mark.parametrize("bits,sub", [(8, (2, 2)), (8, (1, 1)), (16, (2, 2)), (16, (1, 2))])
def test_more_rows_than_a_launch_has_workgroups(bits, sub, tables):
    """a launch has at most 4096 workgroups of 8 groups of sub_y rows each: a taller frame is walked in strides"""
    rng = np.random.default_rng(bits)
    h = 8 * 4096 * sub[1] * 2 + 77
    frame = om.random_frame(rng, h, 3, 3)
    y_steps, c_steps = tables[bits][0]
    fw = ea.ycbcr_forward("601")
    y, (cb, cr) = ea.encode_ycbcr(frame, fw, sub, bits=bits, y_steps=y_steps, c_steps=c_steps)
    for a, b in zip((y, cb, cr), om.planes(frame, fw, sub[0], sub[1], bits, 0, y_steps, c_steps)):
        assert np.array_equal(a, b)


def test_every_step_of_a_16_bit_table(tables):
    """Y and U at steps[k] and at the float below it for all 65535 k: every leaf of both searches. With k_g = 1 and the
    other weights 0 a pixel (0, v, 0) has Y = v, and with c_u = 1 a pixel (0, 0, v) has Y = 0 and U = v."""
    y_steps, c_steps = tables[16][0]
    fw = (0.0, 1.0, 0.0, 1.0, 1.0)
    px = []
    for steps, ch in ((y_steps, 1), (c_steps, 2)):
        s = steps[1:]
        p = np.zeros((2 * s.size, 3), np.float32)
        p[:, ch] = np.concatenate([s, np.nextafter(s, np.float32(-np.inf))])
        px.append(p)
    frame = np.concatenate(px).reshape(257, 1020, 3)
    y, (cb, cr) = ea.encode_ycbcr(frame, fw, (1, 1), bits=16, y_steps=y_steps, c_steps=c_steps)
    want = om.planes(frame, fw, 1, 1, 16, 0, y_steps, c_steps)
    for a, b in zip((y, cb, cr), want):
        assert np.array_equal(a, b)
    # random tables have a few equal neighbours; all but those codes appear
    assert len(np.unique(y)) > 65000 and len(np.unique(cb)) > 65000 and y.max() == 65535 and y.min() == 0


def test_rows_behind_2_31_bytes_of_the_frame():
    """offsets are counted in size_t: the last rows of a device frame of more than 2^31 bytes, and the first"""
    import torch
    w, nch = 8192, 3
    h = ((1 << 31) // (w * nch * 4) + 66) & ~1
    assert h * w * nch * 4 > (1 << 31) + 32 * w * nch * 4
    gen = torch.Generator(device="cuda").manual_seed(7)
    frame = torch.rand((h, w, nch), dtype=torch.float32, device="cuda", generator=gen) * 1.4 - 0.2
    fw = ea.ycbcr_forward("709")
    ys, cs = ea.ycbcr_steps(8)
    y, c = ea.encode_ycbcr(frame, fw, interleaved=True, y_steps=ys, c_steps=cs)
    ea.sync()
    for a, b in ((0, 6), (h - 8, h)):
        want = om.planes(frame[a:b].cpu().numpy(), fw, 2, 2, 8, 0, ys, cs)
        got = (y[a:b].cpu().numpy(), c[a // 2:b // 2, :, 0].cpu().numpy(), c[a // 2:b // 2, :, 1].cpu().numpy())
        for g, x, name in zip(got, want, ("y", "cb", "cr")):
            assert np.array_equal(g, x), (a, name, int((g != x).sum()))
    assert len(np.unique(y[h - 8:].cpu().numpy())) > 200


def chunk_bytes():
    src = open(os.path.join(ROOT, "envutil_amd", "csrc", "eu_api_render.hip")).read()
    m = re.search(r"#define\s+EU_ENCODE_CHUNK_BYTES\s+\(\(size_t\)\s*(\d+)\s*<<\s*(\d+)\)", src)
    assert m, "EU_ENCODE_CHUNK_BYTES has moved"
    return int(m.group(1)) << int(m.group(2))


def test_host_frame_taller_than_a_chunk_of_an_odd_row_count():
    """The staged route takes EU_ENCODE_CHUNK_BYTES / (bytes of a row in and out) rows at a time, a row out counted as
    its luma samples and the two chroma rows under it. Where that is odd, an unrounded chunk would split a chroma row
    of a 4:2:0 frame."""
    chunk = chunk_bytes()
    nch, bits, sb = 4, 16, 2
    row = lambda w: w * nch * 4 + (w + 2 * ((w + 1) // 2)) * sb                                  # noqa: E731
    w = chunk // (5 * 20) + 8                                     # 20 bytes per pixel of an even width
    while chunk // row(w) != 5:
        w -= 1
        assert w > 0
    raw = chunk // row(w)
    assert raw % 2 == 1 and w * nch <= 1 << 28
    h = raw + 2
    rng = np.random.default_rng(3)
    frame = om.random_frame(rng, h, w, nch, specials=False)
    fw = ea.ycbcr_forward("709")
    ys, cs = ea.ycbcr_steps(16, 10)
    y, c = ea.encode_ycbcr(frame, fw, (2, 2), interleaved=True, bits=16, shift=6, y_steps=ys, c_steps=cs)         # P010
    want = om.planes(frame, fw, 2, 2, 16, 6, ys, cs)
    for a, b, name in zip((y, c[..., 0], c[..., 1]), want, ("y", "cb", "cr")):
        assert np.array_equal(a, b), (name, np.argwhere(a != b)[:4])


# ------------------------------------------------------------------------------------------ render_ycbcr
@pytest.fixture(scope="module")
def pano():
    """a lat/lon source whose values leave [0, 1] on both sides"""
    img = jobs.synth_image(256, 128, 3)
    img = img * np.float32(1.6) - np.float32(0.3)
    return ea.Source.load(ea.facet_spec(ea.SPHERICAL, 256, 128, 360.0, nchannels=3), img, 3)


VARIANTS = [dict(subsampling=(2, 2), interleaved=True), dict(subsampling=(2, 2)), dict(subsampling=(2, 1)),
            dict(subsampling=(1, 1)), dict(subsampling=(1, 2), interleaved=True, bits=16, shift=6)]


def planes_list(y, chroma):
    return (y, chroma[..., 0], chroma[..., 1]) if not isinstance(chroma, (tuple, list)) else (y, chroma[0], chroma[1])


def same_as_planes_of_render(args, sources, what, variants=VARIANTS, nchannels=None, **kw):
    frame = ea.render(args, sources, nchannels=nchannels, **kw)
    fw = ea.ycbcr_forward("709")
    for v in variants:
        want = planes_list(*ea.ycbcr_planes(frame, fw, **v))
        got = planes_list(*ea.render_ycbcr(args, sources, fw, nchannels=nchannels, **v, **kw))
        for a, b, name in zip(got, want, ("y", "cb", "cr")):
            assert a.shape == b.shape and a.dtype == b.dtype
            assert np.array_equal(a, b), f"{what}, {v}, {name}: {int((a != b).sum())} of {a.size} samples differ"
        assert len(np.unique(got[0])) > 8, what
    return frame


def test_render_ycbcr_latlon_to_rectilinear(pano):
    args = ea.arguments(ea.RECTILINEAR, 65, 33, 80.0, yaw=30, pitch=-12, roll=5, spline_degree=3)
    same_as_planes_of_render(args, pano, "65 x 33")
    same_as_planes_of_render(args, pano, "65 x 33, 4 channels", nchannels=4, variants=VARIANTS[:2])
    same_as_planes_of_render(ea.arguments(ea.RECTILINEAR, 65, 33, 80.0, spline_degree=3, twine=2), pano, "twined", VARIANTS[:1])


def test_render_ycbcr_cubemap_target(pano):
    same_as_planes_of_render(ea.arguments(ea.CUBEMAP, 15, 90, 90.0, spline_degree=3), pano, "cubemap 15")


def test_render_ycbcr_two_facets():
    a = jobs.synth_image(96, 64, 4, seed=3) * np.float32(1.5) - np.float32(0.2)
    b = jobs.synth_image(96, 64, 4, seed=4) * np.float32(1.5) - np.float32(0.2)
    a[..., 3] = 1.0
    b[..., 3] = 1.0
    fa = ea.Source.load(ea.facet_spec(ea.RECTILINEAR, 96, 64, 70.0, nchannels=4, yaw=-20.0), a, 1)
    fb = ea.Source.load(ea.facet_spec(ea.RECTILINEAR, 96, 64, 70.0, nchannels=4, yaw=25.0, pitch=5.0), b, 1)
    args = ea.arguments(ea.SPHERICAL, 131, 47, 150.0, spline_degree=1)
    same_as_planes_of_render(args, [fa, fb], "two facets", VARIANTS[:3])


def test_render_ycbcr_crop_and_odd_row_begin(pano):
    same_as_planes_of_render(ea.arguments(ea.SPHERICAL, 120, 60, 360.0, spline_degree=1, crop=(13, 78, 7, 40)), pano, "crop")
    args = ea.arguments(ea.RECTILINEAR, 65, 33, 80.0, spline_degree=1)
    same_as_planes_of_render(args, pano, "rows 5 .. 22", row_begin=5, row_end=22)
    y, (cb, cr) = ea.render_ycbcr(args, pano, ea.ycbcr_forward("709"), row_begin=7, row_end=7)
    assert y.shape == (0, 65) and cb.shape == (0, 33)


def test_render_ycbcr_four_chunks_to_the_host(pano):
    """1030 rows: the pipeline of four row chunks of 264, 264, 264 and 238 rows, each a whole number of chroma rows;
    padded host planes keep their padding"""
    args = ea.arguments(ea.SPHERICAL, 9, 1030, 20.0, spline_degree=1)
    frame = same_as_planes_of_render(args, pano, "9 x 1030", VARIANTS[:2] + VARIANTS[4:])
    fw = ea.ycbcr_forward("709")
    big = np.full((1030, 16), om.FILL, np.uint8)
    vu = np.full((515, 8, 2), om.FILL, np.uint8)
    ea.render_ycbcr(args, pano, fw, out=(big[:, 2:11], (vu[:, :5, 1], vu[:, :5, 0])))                        # NV21, padded
    y, (cb, cr) = ea.ycbcr_planes(frame, fw)
    assert np.array_equal(big[:, 2:11], y) and np.array_equal(vu[:, :5, 1], cb) and np.array_equal(vu[:, :5, 0], cr)
    assert (big[:, :2] == om.FILL).all() and (big[:, 11:] == om.FILL).all() and (vu[:, 5:] == om.FILL).all()


def test_render_ycbcr_device_out_on_a_stream_behind_a_reload():
    """the device-to-device loop on one stream: reload_ycbcr of the source, then render_ycbcr of it into NV12 tensors"""
    import torch
    rng = np.random.default_rng(8)
    w, h = 96, 64
    fct = ea.facet_spec(ea.RECTILINEAR, w, h, 70.0, nchannels=3)
    m, fw = ea.ycbcr_matrix("709"), ea.ycbcr_forward("709")
    first = ym.planes(rng, h, w, 2, 2, 8, "nv12")
    second = ym.planes(rng, h, w, 2, 2, 8, "nv12")
    src = ea.Source.load_ycbcr(fct, first[0], (first[1], first[2]), m, spline_degree=1)
    args = ea.arguments(ea.RECTILINEAR, 65, 33, 60.0, yaw=3.0, spline_degree=1)
    want = ea.ycbcr_planes(ea.render(args, ea.Source.load_ycbcr(fct, second[0], (second[1], second[2]), m, spline_degree=1)),
                           fw, interleaved=True)
    yd = torch.from_numpy(second[0].copy()).cuda()
    cd = torch.from_numpy(np.stack([second[1], second[2]], -1).copy()).cuda()
    ybig = torch.full((33, 70), 0x5A, dtype=torch.uint8, device="cuda")
    cbig = torch.full((17, 40, 2), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    src.reload_ycbcr(yd, cd, m, stream=stream.cuda_stream)
    ea.render_ycbcr(args, src, fw, interleaved=True, out=(ybig[:, 3:68], cbig[:, 2:35]), stream=stream)
    # other tables on the library's own stream right behind it: the call waits for the first before it rewrites them
    other = ea.render_ycbcr(args, src, fw, y_steps=ea.ycbcr_steps(8, full_range=True)[0])
    stream.synchronize()
    ea.sync()
    yh, ch = ybig.cpu().numpy(), cbig.cpu().numpy()
    assert np.array_equal(yh[:, 3:68], want[0]) and np.array_equal(ch[:, 2:35], want[1])
    assert (yh[:, :3] == 0x5A).all() and (yh[:, 68:] == 0x5A).all() and (ch[:, :2] == 0x5A).all() and (ch[:, 35:] == 0x5A).all()
    assert np.array_equal(other[1][0], want[1][..., 0]) and not np.array_equal(other[0], want[0])


def test_torch_tensors_in_and_out():
    import torch
    rng = np.random.default_rng(4)
    frame = om.random_frame(rng, 17, 63, 4)
    fw = ea.ycbcr_forward("2020")
    t = torch.from_numpy(frame).cuda()
    for bits, shift, tdt in ((8, 0, torch.uint8), (16, 6, torch.uint16)):
        for inter in (False, True):
            want = planes_list(*ea.ycbcr_planes(frame, fw, interleaved=inter, bits=bits, shift=shift))
            y, c = ea.encode_ycbcr(t, fw, interleaved=inter, bits=bits, shift=shift)
            ea.sync()                                      # the call is asynchronous on the library's stream
            assert y.is_cuda and y.dtype == tdt and tuple(y.shape) == (17, 63)
            got = planes_list(y.cpu().numpy(), c.cpu().numpy() if inter else tuple(p.cpu().numpy() for p in c))
            assert all(np.array_equal(a, b) for a, b in zip(got, want))
        # a padded frame and padded planes, on a torch stream
        wide = torch.zeros((17, 70, 4), dtype=torch.float32, device="cuda")
        wide[:, :63] = t
        ybig = torch.zeros((17, 66), dtype=tdt, device="cuda")
        cbig = torch.zeros((9, 34, 2), dtype=tdt, device="cuda")
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        ea.encode_ycbcr(wide[:, :63], fw, interleaved=True, bits=bits, shift=shift, out=(ybig[:, 1:64], cbig[:, :32]), stream=stream)
        stream.synchronize()
        want = planes_list(*ea.ycbcr_planes(frame, fw, interleaved=True, bits=bits, shift=shift))
        assert np.array_equal(ybig[:, 1:64].cpu().numpy(), want[0]) and np.array_equal(cbig[:, :32, 0].cpu().numpy(), want[1])
        assert np.array_equal(cbig[:, :32, 1].cpu().numpy(), want[2]) and not ybig[:, 64:].cpu().numpy().any() and not cbig[:, 32:].cpu().numpy().any()
        # a numpy frame into device planes, a device frame into numpy planes
        yd = torch.zeros((17, 63), dtype=tdt, device="cuda")
        cd = torch.zeros((9, 32, 2), dtype=tdt, device="cuda")
        ea.encode_ycbcr(frame, fw, interleaved=True, bits=bits, shift=shift, out=(yd, cd))
        ea.sync()
        assert np.array_equal(yd.cpu().numpy(), want[0]) and np.array_equal(cd[..., 1].cpu().numpy(), want[2])
        dt = np.uint8 if bits == 8 else np.uint16
        yh, ch = np.zeros((17, 63), dt), np.zeros((9, 32, 2), dt)
        ea.encode_ycbcr(t, fw, interleaved=True, bits=bits, shift=shift, out=(yh, ch))
        assert np.array_equal(yh, want[0]) and np.array_equal(ch[..., 0], want[1]) and np.array_equal(ch[..., 1], want[2])
