"""Integer samples as a source, host side: the argument checks of eu_hip_source_load_samples (reported before a
device is looked for, so they run without one), and - tests/csrc/samples_demo.cc - the tables and the file reader
of include/eu_image_io.hpp against the float route they stand in for."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import envutil_amd as ea
from envutil_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EU_ERR_ARGUMENT = -2


def call(fct, smp, edit, degree=1, prefilter=1, out=True):
    L = api.lib()
    h = C.c_void_p()
    rc = L.eu_hip_source_load_samples(C.byref(fct) if fct is not None else None, C.byref(smp) if smp is not None else None,
                                      C.byref(edit) if edit is not None else None, degree, prefilter, 8, 64,
                                      C.byref(h) if out else None)
    if rc == 0:
        L.eu_hip_source_release(h)              # a machine with a device: the call went through
    else:
        assert not h.value, "a refused call must not make a source"
    return rc, L.eu_hip_last_error().decode()


@pytest.fixture()
def good():
    """a facet, samples and tables that pass every check (the call then goes on to look for a device)"""
    data = np.zeros((4, 8, 3), np.uint8)
    table = (np.arange(65536, dtype=np.float32) / np.float32(255)).astype(np.float32)

    def make(nchannels=3, bits=8, pixel_channels=3, on_device=0, address=None):
        fct = ea.facet_spec(ea.RECTILINEAR, 8, 4, 60.0, nchannels=nchannels).c_struct()
        smp = api.Samples(data.ctypes.data if address is None else address, bits, 0, pixel_channels, on_device,
                          table.ctypes.data, None)
        return fct, smp
    make.keep = (data, table)
    return make


def refused(rc, msg):
    return rc == EU_ERR_ARGUMENT and len(msg) > 0


def test_null_pointers(good):
    fct, smp = good()
    assert refused(*call(None, smp, None))
    assert refused(*call(fct, None, None))
    assert refused(*call(fct, smp, None, out=False))
    smp.data = None
    assert refused(*call(fct, smp, None))


def test_bits(good):
    for bits in (0, 1, 7, 12, 24, 32, -8):
        fct, smp = good(bits=bits)
        rc, msg = call(fct, smp, None)
        assert refused(rc, msg) and "bits" in msg, (bits, msg)


def test_pixel_channels(good):
    # neither the facet's count nor one less
    for nch, pch in ((3, 1), (3, 4), (4, 2), (1, 2), (4, 5)):
        fct, smp = good(nchannels=nch, pixel_channels=pch)
        rc, msg = call(fct, smp, None)
        assert refused(rc, msg) and "pixel_channels" in msg, (nch, pch, msg)
    # below 1: a one-channel facet has nothing to gain a channel from
    for pch in (0, -1):
        fct, smp = good(nchannels=1, pixel_channels=pch)
        assert refused(*call(fct, smp, None)), pch
    # a gained channel is an alpha channel: the facet has 2 or 4
    fct, smp = good(nchannels=3, pixel_channels=2)
    assert refused(*call(fct, smp, None))


def test_null_colour_table(good):
    fct, smp = good()
    smp.colour_table = None
    rc, msg = call(fct, smp, None)
    assert refused(rc, msg) and "table" in msg


def test_edit_needs_alpha(good):
    xs, ys = np.array([1, 5, 3], np.float32), np.array([1, 1, 3], np.float32)
    for nch in (1, 3):
        fct, smp = good(nchannels=nch, pixel_channels=nch)
        edit, hold = api._facet_edit([(xs, ys)], None, 0, nch, False)
        rc, msg = call(fct, smp, edit)
        assert refused(rc, msg) and "2 or 4 channels" in msg, msg
        edit, hold = api._facet_edit([], (1, 6, 1, 3), 1, nch, False)
        assert refused(*call(fct, smp, edit))
    # the edit's own pixel_channels / pixels_on_device do not count: a valid call gets past the checks
    fct, smp = good(nchannels=4, pixel_channels=3)
    edit, hold = api._facet_edit([(xs, ys)], None, 0, 17, True)
    rc, msg = call(fct, smp, edit)
    assert rc != EU_ERR_ARGUMENT, msg
    # a malformed edit is check_edit's to refuse
    edit.crop_kind = 3
    assert refused(*call(fct, smp, edit))


def test_odd_device_address(good):
    fct, smp = good(bits=16, on_device=1, address=0x7f0000001001)
    rc, msg = call(fct, smp, None)
    assert refused(rc, msg) and "even" in msg


def test_degrees(good):
    for degree, prefilter in ((-1, 1), (10, 1), (1, -1), (1, 10)):
        fct, smp = good()
        rc, msg = call(fct, smp, None, degree, prefilter)
        assert refused(rc, msg) and "degree" in msg, (degree, prefilter, msg)


def test_valid_arguments_reach_the_device(good):
    fct, smp = good()
    rc, msg = call(fct, smp, None)
    if ea.device_count() > 0:
        assert rc == 0, msg
    else:
        assert rc == -1 and "no HIP device" in msg      # EU_ERR_NO_DEVICE: every check passed


def test_python_entry_refuses_other_dtypes():
    fct = ea.facet_spec(ea.RECTILINEAR, 8, 4, 60.0)
    with pytest.raises(ea.EuError):
        ea.Source.load_samples(fct, np.zeros((4, 8, 3), np.float32))
    with pytest.raises(ea.EuError):
        ea.Source.load_samples(fct, np.zeros((4, 8, 3), np.uint8), colour_table=np.zeros(255, np.float32))


@pytest.fixture(scope="module")
def samples_demo():
    exe = os.path.join(ROOT, "envutil_amd", "build", "samples_demo")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "csrc", "samples_demo.cc"), "-o", exe])

    def run(cwd):
        return subprocess.run([exe, str(cwd)], capture_output=True, text=True, timeout=120)
    return run


def test_tables_and_reader_match_the_float_route(samples_demo, tmp_path):
    """bits 8 / maxval 255 and 100, bits 16 / maxval 65535 and 1000, every pair of {Linear, sRGB, Rec709}: for all
    1 << bits values sample_tables equals, as bit patterns, read_image + convert_colour on a file holding exactly
    those samples; read_samples returns the bytes of P5, P6 and P7 (2 and 4 channels) files and of six cube faces,
    refuses a .pfm and gives read_one's messages for truncated and missing files"""
    r = samples_demo(tmp_path)
    assert r.returncode == 0 and "failures: 0" in r.stdout, r.stdout + r.stderr
