"""Radiance RGBE pixels, host side. tests/csrc/rgbe_demo.cc - a stand-alone host program, built with
-fsanitize=address,undefined - holds the two pixel functions of include/eu_rgbe.h against verbatim copies of the
expressions io::read_one and io::write_one used before them, and the readers, the table and the writers of
include/eu_image_io.hpp against files it makes. The numpy model the GPU tests expect (tests/rgbe_model.py) is held
against the same functions. Then the argument checks of eu_hip_source_load_rgbe, eu_hip_encode_rgbe and
eu_hip_render_rgbe, which are made before a device is looked for and so run without one."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import envutil_amd as ea
from envutil_amd import api
import rgbe_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EU_ERR_ARGUMENT, EU_ERR_HANDLE = -2, -5


@pytest.fixture(scope="module")
def rgbe_demo():
    exe = os.path.join(ROOT, "envutil_amd", "build", "rgbe_demo")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "csrc", "rgbe_demo.cc"),
                           "-o", exe])

    def run(*argv):
        return subprocess.run([exe] + [str(a) for a in argv], capture_output=True, text=True, timeout=300)
    return run


def test_pixel_functions_readers_and_writers(rgbe_demo, tmp_path):
    """eu_rgbe_encode equals write_one's old expression byte for byte - every binade from 1e-32f's to 253, the largest
    channel in each position, ties, negative, zero, NaN and denormal channels, 1e-32f and its neighbours - and gives
    the clamped definition at and above 2^127; eu_rgbe_decode equals mantissa * ldexp(1.0f, E - 136) for all 65536
    pairs; decode then encode returns the quad; read_rgbe returns the quads of a flat and of a run-length encoded
    file, truncated files are errors, rgbe_table of equal colour spaces is the decode, write_one's file has not
    changed and write_rgbe writes the same one"""
    r = rgbe_demo("check", tmp_path)
    assert r.returncode == 0 and "failures: 0" in r.stdout, r.stdout + r.stderr


def test_the_numpy_model_is_the_header(rgbe_demo, tmp_path):
    """what the GPU tests expect: the model of tests/rgbe_model.py on its targeted list, on random bit patterns and on
    every (E, mantissa) pair"""
    rng = np.random.default_rng(1)
    px = np.concatenate([rm.targeted(), rm.from_bits(rng.integers(0, 1 << 32, (200000, 3), dtype=np.uint64).astype(np.uint32))])
    px.tofile(tmp_path / "px.f32")
    assert rgbe_demo("encode", tmp_path / "px.f32", tmp_path / "px.rgbe").returncode == 0
    got = np.fromfile(tmp_path / "px.rgbe", np.uint8).reshape(-1, 4)
    want = rm.encode(px)
    bad = np.argwhere((got != want).any(1))
    assert not bad.size, (len(bad), px[bad[0, 0]], got[bad[0, 0]], want[bad[0, 0]])
    assert (got[:, 3] == 255).any() and (got == 0).all(1).any() and len(np.unique(got[:, 3])) > 230

    e, m = np.mgrid[0:256, 0:256]
    quads = np.stack([m, 255 - m, m ^ 0x55, e], -1).astype(np.uint8).reshape(-1, 4)
    quads.tofile(tmp_path / "q.rgbe")
    assert rgbe_demo("decode", tmp_path / "q.rgbe", tmp_path / "q.f32").returncode == 0
    got = np.fromfile(tmp_path / "q.f32", np.float32).reshape(-1, 3)
    assert np.array_equal(rm.bits(got), rm.bits(rm.decode(quads)))


# ---- argument checks: before a device is looked for ----------------------------------------------------------------

def refused(rc, msg):
    return rc == EU_ERR_ARGUMENT and len(msg) > 0


def last_error():
    return api.lib().eu_hip_last_error().decode()


def load(fct, px, edit, degree=1, prefilter=1, out=True):
    L = api.lib()
    h = C.c_void_p()
    rc = L.eu_hip_source_load_rgbe(C.byref(fct) if fct is not None else None, C.byref(px) if px is not None else None,
                                   C.byref(edit) if edit is not None else None, degree, prefilter, 8, 64,
                                   C.byref(h) if out else None)
    if rc == 0:
        L.eu_hip_source_release(h)              # a machine with a device: the call went through
    else:
        assert not h.value, "a refused call must not make a source"
    return rc, last_error()


QUADS = np.zeros((4, 8, 4), np.uint8)


def good(nchannels=3, on_device=0, address=None):
    fct = ea.facet_spec(ea.RECTILINEAR, 8, 4, 60.0, nchannels=nchannels).c_struct()
    return fct, api.Rgbe(QUADS.ctypes.data if address is None else address, on_device, None)


def test_load_null_pointers():
    fct, px = good()
    assert refused(*load(None, px, None))
    assert refused(*load(fct, None, None))
    assert refused(*load(fct, px, None, out=False))
    px.data = None
    assert refused(*load(fct, px, None))


def test_load_channels():
    for nch in (1, 2):
        fct, px = good(nchannels=nch)
        rc, msg = load(fct, px, None)
        assert refused(rc, msg) and "3 channels" in msg, (nch, msg)


def test_load_edit_needs_the_fourth_channel():
    xs, ys = np.array([1, 5, 3], np.float32), np.array([1, 1, 3], np.float32)
    fct, px = good(nchannels=3)
    edit, hold = api._facet_edit([(xs, ys)], None, 0, 3, False)
    rc, msg = load(fct, px, edit)
    assert refused(rc, msg) and "2 or 4 channels" in msg, msg
    edit, hold = api._facet_edit([], (1, 6, 1, 3), 1, 3, False)
    assert refused(*load(fct, px, edit))
    # the edit's own pixel_channels / pixels_on_device do not count: a valid call gets past the checks
    fct, px = good(nchannels=4)
    edit, hold = api._facet_edit([(xs, ys)], None, 0, 17, True)
    rc, msg = load(fct, px, edit)
    assert rc != EU_ERR_ARGUMENT, msg
    edit.crop_kind = 3
    assert refused(*load(fct, px, edit))


def test_load_device_address_and_degrees():
    for address in (0x7f0000001001, 0x7f0000001002):
        fct, px = good(on_device=1, address=address)
        rc, msg = load(fct, px, None)
        assert refused(rc, msg) and "4-byte" in msg
    for degree, prefilter in ((-1, 1), (10, 1), (1, -1), (1, 10)):
        fct, px = good()
        rc, msg = load(fct, px, None, degree, prefilter)
        assert refused(rc, msg) and "degree" in msg, (degree, prefilter, msg)


def test_load_valid_arguments_reach_the_device():
    for nch in (3, 4):
        fct, px = good(nchannels=nch)
        rc, msg = load(fct, px, None)
        if ea.device_count() > 0:
            assert rc == 0, msg
        else:
            assert rc == -1 and "no HIP device" in msg      # EU_ERR_NO_DEVICE: every check passed


def encode(frame_ptr, fstride, w, h, out_ptr, ostride, frame_dev=0, out_dev=0):
    rc = api.lib().eu_hip_encode_rgbe(C.c_void_p(frame_ptr), fstride, frame_dev, w, h, C.c_void_p(out_ptr), ostride, out_dev, None)
    return rc, last_error()


def test_encode_arguments():
    frame = np.zeros((4, 8, 3), np.float32)
    out = np.full((4, 8, 4), 0xAB, np.uint8)
    f, o = frame.ctypes.data, out.ctypes.data
    assert refused(*encode(None, 96, 8, 4, o, 32))
    assert refused(*encode(f, 96, 8, 4, None, 32))
    assert refused(*encode(f, 96, -1, 4, o, 32))
    assert refused(*encode(f, 96, 8, -1, o, 32))
    rc, msg = encode(f, 92, 8, 4, o, 32)
    assert refused(rc, msg) and "stride" in msg
    rc, msg = encode(f, 96, 8, 4, o, 28)
    assert refused(rc, msg) and "stride" in msg
    rc, msg = encode(f, 98, 8, 4, o, 32)
    assert refused(rc, msg) and "multiples of 4" in msg
    rc, msg = encode(f + 2, 96, 8, 4, o, 32)
    assert refused(rc, msg) and "multiples of 4" in msg
    for off, stride in ((1, 32), (2, 32), (0, 34), (0, 33)):
        rc, msg = encode(f, 96, 8, 4, o + off, stride)
        assert refused(rc, msg) and "4-byte" in msg, (off, stride, msg)
    # nothing to do: EU_OK without a device, and nothing written
    for w, h in ((0, 4), (8, 0), (0, 0)):
        rc, msg = encode(f, 96, w, h, o, 32)
        assert rc == 0, msg
    assert (out == 0xAB).all()
    rc, msg = encode(f, 96, 8, 4, o, 32)
    if ea.device_count() > 0:
        assert rc == 0, msg
    else:
        assert rc == -1 and "no HIP device" in msg


def render(t, srcs, nsrc, out_ptr, ostride):
    rc = api.lib().eu_hip_render_rgbe(C.byref(t) if t is not None else None, srcs, nsrc, C.c_void_p(out_ptr), ostride, 0, None)
    return rc, last_error()


def test_render_arguments():
    L = api.lib()
    L.eu_hip_diag_host_source.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    fct = ea.facet_spec(ea.SPHERICAL, 64, 32, 360.0).c_struct()
    src = C.c_void_p()
    assert L.eu_hip_diag_host_source(C.byref(fct), 1, C.byref(src)) == 0     # a handle made without a device
    srcs = (C.c_void_p * 1)(src)
    out = np.full((16, 32, 4), 0xAB, np.uint8)
    o = out.ctypes.data
    args = ea.arguments(ea.RECTILINEAR, 32, 16, 90.0, spline_degree=1)
    try:
        assert refused(*render(None, srcs, 1, o, 128))
        assert refused(*render(args.target(3), None, 1, o, 128))
        assert refused(*render(args.target(3), srcs, 0, o, 128))
        assert refused(*render(args.target(3), srcs, 1, None, 128))
        for nch in (1, 2, 4):
            rc, msg = render(args.target(nch), srcs, 1, o, 128)
            assert refused(rc, msg) and "3 channels" in msg, (nch, msg)
        rc, msg = render(args.target(3, stage=1), srcs, 1, o, 128)
        assert refused(rc, msg) and "stage" in msg
        t = args.target(3)
        t.out_format = 1
        rc, msg = render(t, srcs, 1, o, 128)
        assert refused(rc, msg) and "SRGBA8" in msg
        rc, msg = render(args.target(3), srcs, 1, o, 124)
        assert refused(rc, msg) and "stride" in msg
        for off, stride in ((1, 128), (2, 128), (0, 130)):
            rc, msg = render(args.target(3), srcs, 1, o + off, stride)
            assert refused(rc, msg) and "4-byte" in msg, (off, stride, msg)
        rc, msg = render(args.target(3), (C.c_void_p * 1)(None), 1, o, 128)
        assert rc == EU_ERR_HANDLE, msg
        assert (out == 0xAB).all()
    finally:
        L.eu_hip_source_release(src)


def test_python_entries_refuse_other_arrays():
    fct = ea.facet_spec(ea.RECTILINEAR, 8, 4, 60.0)
    with pytest.raises(ea.EuError):
        ea.Source.load_rgbe(fct, np.zeros((4, 8, 4), np.float32))
    with pytest.raises(ea.EuError):
        ea.Source.load_rgbe(fct, np.zeros((4, 8, 3), np.uint8))
    with pytest.raises(ea.EuError):
        ea.Source.load_rgbe(fct, np.zeros((4, 8, 4), np.uint8), colour_table=np.zeros(256, np.float32))
    with pytest.raises(ea.EuError):
        ea.encode_rgbe(np.zeros((4, 8, 4), np.float32))
    with pytest.raises(ea.EuError):
        ea.encode_rgbe(np.zeros((4, 8, 3), np.float32), out=np.zeros((4, 8, 3), np.uint8))
