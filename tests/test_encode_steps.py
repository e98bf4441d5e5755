"""The way out as integer samples, host side. tests/csrc/encode_demo.cc - a stand-alone host program, built with
-fsanitize=address,undefined - sweeps all 2^32 float bit patterns: the count over io::encode_steps' table against
io::convert_colour + the quantiser as io::write_one calls it, the host route that predates the tables and is the
yardstick; the sanitizers' runtimes are linked into the program. Then the argument checks of eu_hip_encode_samples and eu_hip_render_samples, which are made before a device
is looked for and so run without one."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import envutil_amd as ea
from envutil_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EU_ERR_ARGUMENT, EU_ERR_HANDLE = -2, -5


@pytest.fixture(scope="module")
def encode_demo():
    exe = os.path.join(ROOT, "envutil_amd", "build", "encode_demo")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-pthread",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "csrc", "encode_demo.cc"),
                           "-o", exe])

    def run(*argv, timeout=120):
        return subprocess.run([exe] + [str(a) for a in argv], capture_output=True, text=True, timeout=timeout)
    return run


def test_every_float_gets_the_host_routes_code(encode_demo):
    """Every pair of Linear / sRGB / Rec709 at maxval 255 and 65535, all 2^32 floats: zero differences for every
    table the builder accepts, a refusal only where the sweep finds a difference, the two Rec709 tables at 65535
    refused (to_linear of Rec709 drops at 0.081: four codes at 16 bit), and no more than those two of the 18."""
    r = encode_demo("sweep", min(16, os.cpu_count() or 1), timeout=3000)
    print(r.stdout)
    assert r.returncode == 0 and "failures: 0" in r.stdout, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert sum(": accepted, 0 differences" in ln for ln in lines) == 16, r.stdout
    for pair in ("Rec709 -> Linear at 65535: refused", "Rec709 -> sRGB at 65535: refused"):
        assert any(ln.startswith(pair) for ln in lines), r.stdout


def test_linear_steps_equal_the_python_default(encode_demo, tmp_path):
    """the quantiser alone, bisected in C++ and in numpy: the same floats; alpha takes no curve"""
    for bits, maxval in ((8, 255), (8, 100), (16, 65535), (16, 1000)):
        out = tmp_path / f"steps_{bits}_{maxval}.f32"
        r = encode_demo("steps", bits, maxval, "Linear", "Linear", out)
        assert r.returncode == 0, r.stderr
        got = np.fromfile(out, np.float32).reshape(2, 1 << bits)
        want = ea.sample_steps(bits, maxval)
        for t in got:
            assert np.array_equal(t[1:].view(np.uint32), want[1:].view(np.uint32)), (bits, maxval)
        r = encode_demo("steps", bits, maxval, "Linear", "sRGB", out)
        assert r.returncode == 0, r.stderr
        got = np.fromfile(out, np.float32).reshape(2, 1 << bits)
        assert np.array_equal(got[1, 1:].view(np.uint32), want[1:].view(np.uint32))
        assert not np.array_equal(got[0, 1:maxval], want[1:maxval])


def test_refused_table_and_unknown_names(encode_demo, tmp_path):
    r = encode_demo("steps", 16, 65535, "Rec709", "Linear", tmp_path / "r.f32")
    assert r.returncode == 3 and "no step function" in r.stderr and "0.081" in r.stderr, r.stderr
    r = encode_demo("steps", 8, 255, "Rec709", "Linear", tmp_path / "r8.f32")
    assert r.returncode == 0, r.stderr
    r = encode_demo("steps", 8, 255, "ACEScg", "Linear", tmp_path / "x.f32")
    assert r.returncode == 1 and "not known here" in r.stderr
    r = encode_demo("steps", 12, 4095, "sRGB", "Linear", tmp_path / "y.f32")
    assert r.returncode == 1


def write_pfm(path, img):
    h, w, n = img.shape
    with open(path, "wb") as f:
        f.write({1: b"Pf", 3: b"PF", 4: b"PF4"}[n] + b"\n%d %d\n-1.0\n" % (w, h))
        f.write(np.ascontiguousarray(img[::-1], "<f4").tobytes())


def test_host_route_mode_writes_write_ones_file(encode_demo, tmp_path):
    """the demo's second mode is read_image + convert_colour + write_image: with equal colour spaces the payload is
    the quantiser's, as numpy states it in float32"""
    rng = np.random.default_rng(3)
    img = (rng.random((5, 7, 3)) * 1.4 - 0.2).astype(np.float32)
    img[0, 0] = (np.nan, np.inf, -np.inf)
    write_pfm(tmp_path / "a.pfm", img)
    for name, maxval, dt in (("a.ppm", 255, np.uint8), ("a.pam", 65535, ">u2")):
        r = encode_demo("host", tmp_path / "a.pfm", tmp_path / name, "Linear", "Linear")
        assert r.returncode == 0, r.stderr
        body = open(tmp_path / name, "rb").read()[-img.size * np.dtype(dt).itemsize:]
        with np.errstate(invalid="ignore"):
            want = (np.clip(np.nan_to_num(img, nan=0.0), 0, 1) * np.float32(maxval) + np.float32(0.5)).astype(np.uint32)
        assert np.array_equal(np.frombuffer(body, dt).reshape(img.shape), want), name


# ---------------------------------------------------------------------------------------- argument checks
def last_error():
    return api.lib().eu_hip_last_error().decode()


def refused(rc):
    return rc == EU_ERR_ARGUMENT and len(last_error()) > 0


class Case:
    """arguments of eu_hip_encode_samples that pass every check; fields are changed one at a time"""

    def __init__(self, bits=8, w=8, h=4, nch=3):
        self.bits, self.w, self.h, self.nch = bits, w, h, nch
        self.frame = np.zeros((h, w, nch), np.float32)
        self.out = np.zeros((h, w * nch * (bits // 8) + 8), np.uint8)
        self.colour = ea.sample_steps(bits)
        self.alpha = None
        self.big_endian = 0
        self.frame_ptr, self.out_ptr = self.frame.ctypes.data, self.out.ctypes.data
        self.frame_stride, self.out_stride = w * nch * 4, self.out.shape[1]
        self.frame_dev = self.out_dev = 0

    def enc(self):
        return api.Encode(self.bits, self.big_endian, self.colour.ctypes.data if self.colour is not None else None,
                          self.alpha.ctypes.data if self.alpha is not None else None)

    def call(self, enc=True):
        e = self.enc()
        return api.lib().eu_hip_encode_samples(C.c_void_p(self.frame_ptr), self.frame_stride, self.frame_dev, self.w, self.h,
                                               self.nch, C.byref(e) if enc else None, C.c_void_p(self.out_ptr),
                                               self.out_stride, self.out_dev, None)


def render_call(case, trg, srcs=True, enc=True):
    """eu_hip_render_samples with one NULL source handle: every argument check comes before the handle is looked at"""
    e = case.enc()
    arr = (C.c_void_p * 1)(None)
    return api.lib().eu_hip_render_samples(C.byref(trg) if trg is not None else None, arr if srcs else None, 1,
                                           C.byref(e) if enc else None, C.c_void_p(case.out_ptr), case.out_stride, 0, None)


def target(w=8, h=4, nch=3, **kw):
    return ea.arguments(ea.RECTILINEAR, w, h, 60.0).target(nch, **kw)


def bad_tables(bits):
    """(name, table) for every way a table can be invalid"""
    n = 1 << bits
    good = ea.sample_steps(bits, 100)              # numbers up to entry 100, NaN behind
    t1 = good.copy(); t1[50] = np.nan              # a NaN inside the prefix: numbers follow it
    t2 = good.copy(); t2[60] = np.nextafter(t2[59], np.float32(-1))   # a decreasing pair
    t3 = good.copy(); t3[n - 1] = 1.0              # a number behind the first NaN
    t4 = good.copy(); t4[1] = np.nan               # no code above 0
    t5 = np.full(n, np.nan, np.float32)
    return (("NaN in the prefix", t1), ("decreasing", t2), ("number behind NaN", t3), ("steps[1] NaN", t4), ("all NaN", t5))


@pytest.mark.parametrize("bits", [8, 16])
def test_invalid_tables(bits):
    for name, tab in bad_tables(bits):
        c = Case(bits)
        c.colour = tab
        assert refused(c.call()) and "colour steps" in last_error(), (name, last_error())
        assert refused(render_call(c, target())) and "colour steps" in last_error(), (name, last_error())
        c = Case(bits, nch=4)
        c.alpha = tab
        assert refused(c.call()) and "alpha steps" in last_error(), (name, last_error())
        assert refused(render_call(c, target(nch=4))) and "alpha steps" in last_error(), (name, last_error())


def test_valid_tables_pass_the_checks():
    """equal neighbours, a NaN tail, a table of one code: accepted - the call goes on to look for a device"""
    eq = ea.sample_steps(8, 100)
    eq[10:20] = eq[10]
    one = np.full(256, np.nan, np.float32)
    one[1] = 0.5
    for tab in (ea.sample_steps(8), ea.sample_steps(8, 100), eq, one):
        c = Case(8)
        c.colour = tab
        rc = c.call()
        assert rc == (0 if ea.device_count() > 0 else -1), last_error()
        if rc:
            assert "no HIP device" in last_error()
        assert render_call(c, target()) == EU_ERR_HANDLE, last_error()      # the NULL source: every check passed


def test_null_pointers_bits_channels():
    c = Case()
    assert refused(c.call(enc=False))
    c = Case(); c.frame_ptr = None
    assert refused(c.call())
    c = Case(); c.out_ptr = None
    assert refused(c.call())
    c = Case(); c.colour = None
    assert refused(c.call()) and "colour steps" in last_error()
    for bits in (0, 7, 12, 24, 32, -8):
        c = Case(); c.bits = bits
        assert refused(c.call()) and "bits" in last_error(), bits
        assert refused(render_call(c, target())) and "bits" in last_error(), bits
    for nch in (0, 5, -1):
        c = Case(); c.nch = nch
        assert refused(c.call()) and "channels" in last_error(), nch
    c = Case(); c.h = -1
    assert refused(c.call())
    c = Case(); c.w = -1
    assert refused(c.call())
    c = Case()
    assert refused(render_call(c, None))
    assert refused(render_call(c, target(), srcs=False))
    assert refused(render_call(c, target(), enc=False))
    c.out_ptr = None
    assert refused(render_call(c, target()))


def test_strides():
    c = Case(); c.frame_stride = c.w * c.nch * 4 - 4
    assert refused(c.call()) and "stride" in last_error()
    c = Case(); c.frame_stride = c.w * c.nch * 4 + 2
    assert refused(c.call()) and "multiples of 4" in last_error()
    c = Case(); c.frame_ptr += 2
    assert refused(c.call()) and "multiples of 4" in last_error()
    for bits in (8, 16):
        c = Case(bits); c.out_stride = c.w * c.nch * (bits // 8) - 1
        assert refused(c.call()) and "stride" in last_error()
        assert refused(render_call(c, target())) and "stride" in last_error()
    # 8 bit: rows at any byte, strides of any size from a row on
    c = Case(8); c.out_ptr += 1; c.out_stride = c.w * c.nch + 1
    assert render_call(c, target()) == EU_ERR_HANDLE, last_error()


def test_odd_16_bit_addresses():
    c = Case(16); c.out_ptr += 1
    assert refused(c.call()) and "even" in last_error()
    assert refused(render_call(c, target())) and "even" in last_error()
    c = Case(16); c.out_stride = c.w * c.nch * 2 + 1
    assert refused(c.call()) and "even" in last_error()
    assert refused(render_call(c, target())) and "even" in last_error()
    c = Case(16); c.out_ptr += 2; c.out_stride = c.w * c.nch * 2 + 2
    assert render_call(c, target()) == EU_ERR_HANDLE, last_error()


def test_render_samples_refuses_stages_and_srgba8():
    c = Case()
    for stage in (1, 2):
        assert refused(render_call(c, target(stage=stage))) and "stage" in last_error()
    t = target()
    t.out_format = api.OUT_SRGBA8
    assert refused(render_call(c, t)) and "SRGBA8" in last_error()
    t = target()
    t.row_end = 5                                                          # check_target's own refusals come first
    assert refused(render_call(c, t))


def test_python_entries_refuse_what_they_cannot_pass_on():
    with pytest.raises(ea.EuError):
        ea.encode_samples(np.zeros((4, 8, 5), np.float32))
    with pytest.raises(ea.EuError):
        ea.encode_samples(np.zeros((4, 8, 3), np.float32), bits=12)
    with pytest.raises(ea.EuError):
        ea.encode_samples(np.zeros((4, 8, 3), np.float32), colour_steps=np.zeros(255, np.float32))
    with pytest.raises(ea.EuError):
        ea.encode_samples(np.zeros((4, 8, 3), np.float32), out=np.zeros((4, 8, 3), np.uint16))
    with pytest.raises(ea.EuError):
        ea.sample_steps(8, 256)
    # an empty frame needs no device
    assert ea.encode_samples(np.zeros((0, 8, 3), np.float32)).shape == (0, 8, 3)
