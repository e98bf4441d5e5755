"""The Y'CbCr way out, host side: eu_hip_ycbcr_planes - the definition of what eu_hip_encode_ycbcr and
eu_hip_render_ycbcr make on the device - against the numpy model of tests/ycbcr_out_model.py, byte for byte over whole
padded buffers; the round trip planes -> ycbcr_floats -> ycbcr_planes; ycbcr_steps against its quantiser expression;
the argument checks of the three entry points, which are made before a device is looked for; and
tests/csrc/ycbcr_out_demo.cc, a stand-alone program over io::y4m_writer and io::ycbcr_steps, built plainly and with
-fsanitize=address,undefined."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import envutil_amd as ea
from envutil_amd import api
import ycbcr_out_model as om

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EU_ERR_ARGUMENT = -2
SUBS = [(1, 1), (2, 1), (1, 2), (2, 2)]
LAYOUTS = ["planar", "nv12", "nv21"]
SIZES = [(1, 1), (2, 1), (1, 2), (3, 3), (5, 2), (7, 9), (64, 3), (65, 5)]            # (w, h)


def out_struct(lay, ybuf, cbuf, forward, shift, y_steps, c_steps, on_device=0, y_base=None, c_base=None):
    """eu_ycbcr_out over the buffers of an om.Layout (host arrays, or device addresses y_base / c_base)"""
    yb = ybuf.ctypes.data if y_base is None else y_base
    cb = cbuf.ctypes.data if c_base is None else c_base
    return api.YcbcrOut(yb + lay.y_at, cb + lay.cb_at, cb + lay.cr_at, lay.y_pitch, lay.c_pitch, lay.c_step, lay.sub_x,
                        lay.sub_y, lay.bits, shift, on_device, y_steps.ctypes.data, c_steps.ctypes.data,
                        *[float(k) for k in forward])


def host_planes(frame, lay, forward, shift, y_steps, c_steps):
    ybuf, cbuf = lay.buffers()
    o = out_struct(lay, ybuf, cbuf, forward, shift, y_steps, c_steps)
    h, w, nch = frame.shape
    rc = api.lib().eu_hip_ycbcr_planes(frame.ctypes.data_as(C.c_void_p), frame.strides[0], w, h, nch, C.byref(o))
    assert rc == 0, api.lib().eu_hip_last_error().decode()
    return ybuf, cbuf


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("bits", [8, 16])
def test_host_planes_equal_the_model(bits, layout):
    """all subsamplings, shifts, channel counts and sizes; padded pitches, planes off the dword boundary; random tables
    with equal neighbours and a NaN tail; frames with NaN, both infinities and -0"""
    rng = np.random.default_rng(bits * 7 + len(layout))
    sb = bits // 8
    n = 0
    for sub_x, sub_y in SUBS:
        for shift in (0, 6):
            for nch in (3, 4):
                for w, h in SIZES:
                    top = None if (w + h) % 2 else (1 << bits) - 1 - int(rng.integers(1, 1 << (bits - 2)))
                    y_steps = om.random_steps(rng, bits, top=top, ties=3)
                    c_steps = om.random_steps(rng, bits, -0.7, 0.7, top=top, ties=3)
                    forward = ea.ycbcr_forward(("601", "709", "2020")[n % 3])
                    wide = om.random_frame(rng, h, w + 1, nch)
                    frame = wide[:, :w]                                          # rows padded by a pixel
                    lay = om.Layout(w, h, sub_x, sub_y, bits, layout, y_off=sb * (n % 3), c_off=sb * ((n // 3) % 3),
                                    pad=sb * (n % 4))
                    got = host_planes(frame, lay, forward, shift, y_steps, c_steps)
                    want = lay.expected(frame, forward, shift, y_steps, c_steps)
                    for g, x, name in zip(got, want, ("luma", "chroma")):
                        bad = np.flatnonzero(g != x)
                        assert not bad.size, (name, (w, h), (sub_x, sub_y), shift, nch, bad[:8], g[bad[:8]], x[bad[:8]])
                    n += 1
    assert n == 4 * 2 * 2 * len(SIZES)


def test_python_binding_equals_the_model():
    """ycbcr_planes: new planes in load_ycbcr's shapes, and `out` with strides of its own"""
    rng = np.random.default_rng(5)
    frame = om.random_frame(rng, 9, 7, 3)
    fw = ea.ycbcr_forward("709")
    ys, cs = ea.ycbcr_steps(8)
    for (sx, sy) in SUBS:
        want = om.planes(frame, fw, sx, sy, 8, 0, ys, cs)
        y, (cb, cr) = ea.ycbcr_planes(frame, fw, (sx, sy))
        assert all(np.array_equal(a, b) for a, b in zip((y, cb, cr), want))
        y, c = ea.ycbcr_planes(frame, fw, (sx, sy), interleaved=True)
        assert c.shape == cb.shape + (2,) and all(np.array_equal(a, b) for a, b in zip((y, c[..., 0], c[..., 1]), want))
        big = np.full((9, 16), 7, np.uint8)
        vu = np.full(cb.shape + (2,), 7, np.uint8)
        ea.ycbcr_planes(frame, fw, (sx, sy), out=(big[:, 3:10], (vu[..., 1], vu[..., 0])))                  # NV21
        assert np.array_equal(big[:, 3:10], want[0]) and (big[:, :3] == 7).all() and (big[:, 10:] == 7).all()
        assert np.array_equal(vu[..., 1], want[1]) and np.array_equal(vu[..., 0], want[2])
    y, (cb, cr) = ea.ycbcr_planes(frame, fw, bits=16, shift=6)                                                # P010's samples
    ys, cs = ea.ycbcr_steps(16, 10)
    want = om.planes(frame, fw, 2, 2, 16, 6, ys, cs)
    assert y.dtype == np.uint16 and all(np.array_equal(a, b) for a, b in zip((y, cb, cr), want))
    assert (y & 63 == 0).all() and y.max() == 1023 << 6


@pytest.fixture(scope="module")
def all_triples():
    """every 8-bit (y, cb, cr) as a 4096 x 4096 4:4:4 image"""
    v = np.arange(1 << 24, dtype=np.uint32).reshape(4096, 4096)
    return (v & 255).astype(np.uint8), ((v >> 8) & 255).astype(np.uint8), (v >> 16).astype(np.uint8)


def test_round_trip_of_every_8_bit_triple(all_triples):
    """ycbcr_planes(ycbcr_floats(planes)) == planes, BT.709 limited range"""
    y, cb, cr = all_triples
    yt, ct = ea.ycbcr_tables(8)
    frame = ea.ycbcr_floats(y, (cb, cr), ea.ycbcr_matrix("709"), yt, ct)
    y2, (cb2, cr2) = ea.ycbcr_planes(frame, ea.ycbcr_forward("709"), (1, 1))
    for a, b, name in ((y, y2, "y"), (cb, cb2, "cb"), (cr, cr2, "cr")):
        assert np.array_equal(a, b), (name, int((a != b).sum()))


@pytest.mark.parametrize("depth,shift,full", [(8, 0, False), (8, 0, True), (10, 0, False), (10, 6, False), (10, 6, True),
                                              (12, 0, False), (16, 0, False), (16, 0, True)])
def test_round_trip_of_random_planes(depth, shift, full):
    """every subsampling, planar and interleaved, every matrix: decoded with chroma replicated and encoded back, the
    planes return - the mean of equal values is the value"""
    rng = np.random.default_rng(depth * 10 + shift + full)
    bits = 8 if depth == 8 else 16
    yt, ct = ea.ycbcr_tables(bits, depth, full, msb_aligned=shift > 0)
    ys, cs = ea.ycbcr_steps(bits, depth, full)
    for k, (sx, sy) in enumerate(SUBS):
        name = ("601", "709", "2020")[k % 3]
        h, w = 37, 53
        ch, cw = (h + sy - 1) // sy, (w + sx - 1) // sx
        dt = np.uint8 if bits == 8 else np.uint16
        y, cb, cr = ((rng.integers(0, 1 << depth, s) << shift).astype(dt) for s in ((h, w), (ch, cw), (ch, cw)))
        frame = ea.ycbcr_floats(y, (cb, cr), ea.ycbcr_matrix(name), yt, ct)
        y2, c2 = ea.ycbcr_planes(frame, ea.ycbcr_forward(name), (sx, sy), interleaved=bool(k & 1), bits=bits, shift=shift,
                                 y_steps=ys, c_steps=cs)
        cb2, cr2 = (c2[..., 0], c2[..., 1]) if k & 1 else c2
        assert np.array_equal(y, y2) and np.array_equal(cb, cb2) and np.array_equal(cr, cr2), (sx, sy, name)


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("full", [False, True])
def test_steps_are_the_quantiser(depth, full):
    """steps[k] has code k and the float below it code k - 1, for every k; NaN behind 2^depth - 1"""
    bits = 8 if depth == 8 else 16
    top = (1 << depth) - 1
    s = 2.0 ** (depth - 8)
    for steps, (a, b) in zip(ea.ycbcr_steps(bits, depth, full),
                             ((float(top), 0.0), (float(top), 128 * s)) if full else ((219 * s, 16 * s), (224 * s, 128 * s))):
        assert steps.dtype == np.float32 and steps.shape == (1 << bits,)
        q = lambda v: np.clip(np.floor(v.astype(np.float64) * a + b + 0.5), 0, top)                       # noqa: E731
        at = steps[1:top + 1]
        assert np.array_equal(q(at), np.arange(1, top + 1))
        assert np.array_equal(q(np.nextafter(at, np.float32(-np.inf))), np.arange(0, top))
        assert np.isnan(steps[top + 1:]).all() and steps[0] == -np.inf
        # ... and the library's count of compares is that code
        v = np.concatenate([at, np.nextafter(at, np.float32(-np.inf))])
        assert np.array_equal(om.codes(v, steps, bits, 0), q(v).astype(np.uint16))


def test_forward_coefficients():
    for name, (kr, kb) in (("601", (0.299, 0.114)), ("709", (0.2126, 0.0722)), ("2020", (0.2627, 0.0593))):
        want = [np.float32(v) for v in (kr, 1 - kr - kb, kb, 1 / (2 * (1 - kb)), 1 / (2 * (1 - kr)))]
        assert list(ea.ycbcr_forward(name)) == want
    with pytest.raises(ea.EuError):
        ea.ycbcr_forward("240")


def test_ctypes_struct_matches_the_header(tmp_path):
    """sizeof / offsetof of eu_ycbcr_out as gcc lays it out, against api.YcbcrOut"""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "eu_hip.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(eu_ycbcr_out));']
    lines += [f'  printf("{f} %zu\\n", offsetof(eu_ycbcr_out, {f}));' for f, _ in api.YcbcrOut._fields_]
    lines += ['  return 0;', '}']
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")])
    got = dict(ln.split() for ln in subprocess.check_output([str(tmp_path / "layout")], text=True).splitlines())
    assert int(got.pop("size")) == C.sizeof(api.YcbcrOut)
    assert {k: int(v) for k, v in got.items()} == {f: getattr(api.YcbcrOut, f).offset for f, _ in api.YcbcrOut._fields_}


# ---- argument checks: before a device is looked for ----------------------------------------------------------------

W, H = 12, 6
FRAME = np.zeros((H, W, 3), np.float32)
Y8, C8 = np.zeros((H, W), np.uint8), np.zeros((H // 2, W // 2, 2), np.uint8)
Y16, C16 = np.zeros((H, W), np.uint16), np.zeros((H // 2, W // 2, 2), np.uint16)
STEPS = {8: ea.sample_steps(8), 16: ea.sample_steps(16)}


def good(size=8, **kw):
    """a well-formed eu_ycbcr_out of `size`-bit planes with the fields of kw changed"""
    y, c = (Y8, C8) if size == 8 else (Y16, C16)
    o = api.YcbcrOut(y.ctypes.data, c.ctypes.data, c.ctypes.data + size // 8, y.strides[0], c.strides[0], 2, 2, 2, size, 0, 0,
                     STEPS[size].ctypes.data, STEPS[size].ctypes.data, 0.25, 0.5, 0.25, 0.5, 0.5)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def planes_call(o, frame=FRAME.ctypes.data, stride=W * 12, w=W, h=H, nch=3):
    return api.lib().eu_hip_ycbcr_planes(C.c_void_p(frame), stride, w, h, nch, C.byref(o) if o is not None else None)


def encode_call(o, frame=FRAME.ctypes.data, stride=W * 12, w=W, h=H, nch=3):
    return api.lib().eu_hip_encode_ycbcr(C.c_void_p(frame), stride, 0, w, h, nch, C.byref(o) if o is not None else None, None)


def bad_table(kind):
    s = STEPS[8].copy()
    if kind == "nan1":
        s[1] = np.nan
    elif kind == "order":
        s[9] = s[7]
    else:
        s[200] = np.nan
    return s


REFUSALS = [
    ("null dst", lambda: dict(o=None), "null"),
    ("null plane", lambda: dict(o=good(cb=None)), "plane"),
    ("null table", lambda: dict(o=good(c_steps=None)), "table"),
    ("null frame", lambda: dict(o=good(), frame=None), "frame"),
    ("bits", lambda: dict(o=good(bits=12)), "bits"),
    ("shift low", lambda: dict(o=good(shift=-1)), "shift"),
    ("shift high", lambda: dict(o=good(shift=8)), "shift"),
    ("sub_x", lambda: dict(o=good(sub_x=3)), "sub_x"),
    ("sub_y", lambda: dict(o=good(sub_y=0)), "sub_y"),
    ("c_step", lambda: dict(o=good(c_step=3)), "c_step"),
    ("no pair", lambda: dict(o=good(cr=C8.ctypes.data + 2)), "one sample"),
    ("no pair 16", lambda: dict(o=good(16, cr=C16.ctypes.data + 1 * 4)), "one sample"),
    ("y_pitch", lambda: dict(o=good(y_pitch=W - 1)), "y_pitch"),
    ("c_pitch", lambda: dict(o=good(c_pitch=W - 2)), "c_pitch"),
    ("odd plane", lambda: dict(o=good(16, y=Y16.ctypes.data + 1)), "even addresses"),
    ("odd pitch", lambda: dict(o=good(16, y_pitch=2 * W + 1)), "even pitches"),
    ("channels 2", lambda: dict(o=good(), nch=2), "nchannels"),
    ("channels 1", lambda: dict(o=good(), nch=1), "nchannels"),
    ("frame stride short", lambda: dict(o=good(), stride=W * 12 - 4), "stride"),
    ("frame stride odd", lambda: dict(o=good(), stride=W * 12 + 2), "multiples of 4"),
    ("frame odd", lambda: dict(o=good(), frame=FRAME.ctypes.data + 2, stride=W * 12 + 4), "multiples of 4"),
    ("table nan", lambda: dict(o=None, table=("y_steps", "nan1")), "y steps"),
    ("table order", lambda: dict(o=None, table=("c_steps", "order")), "c steps"),
    ("table hole", lambda: dict(o=None, table=("y_steps", "hole")), "y steps"),
]


@pytest.mark.parametrize("name,make,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_argument_errors(name, make, word):
    """each refusal is EU_ERR_ARGUMENT, of the host function and of the device call alike (no device is looked for),
    and its message names what is wrong"""
    kw = make()
    keep = None
    if "table" in kw:
        field, kind = kw.pop("table")
        keep = bad_table(kind)
        kw["o"] = good(**{field: keep.ctypes.data})
    for call, who in ((planes_call, "ycbcr_planes"), (encode_call, "encode_ycbcr")):
        rc = call(**kw)
        msg = api.lib().eu_hip_last_error().decode()
        assert rc == EU_ERR_ARGUMENT and msg.startswith(who) and word in msg, (name, rc, msg)


def test_host_function_refuses_device_planes_and_empty_frames_write_nothing():
    assert planes_call(good(on_device=1)) == EU_ERR_ARGUMENT and "on_device" in api.lib().eu_hip_last_error().decode()
    y = np.full((H, W), 9, np.uint8)
    for call in (planes_call, encode_call):
        assert call(good(y=y.ctypes.data), w=0) == 0 and call(good(y=y.ctypes.data), h=0) == 0
    assert (y == 9).all()


def test_render_refusals():
    """eu_hip_render_ycbcr: what eu_hip_render refuses, stage outputs, EU_OUT_SRGBA8, other channel counts"""
    L = api.lib()
    args = ea.arguments(ea.RECTILINEAR, W, H, 60.0)
    srcs = (C.c_void_p * 1)(C.c_void_p(8))                   # never read: every call is refused before
    o = good()

    def call(t, dst=o, s=srcs, n=1):
        rc = L.eu_hip_render_ycbcr(C.byref(t) if t is not None else None, s, n, C.byref(dst) if dst is not None else None, None)
        return rc, L.eu_hip_last_error().decode()

    rc, msg = call(None)
    assert rc == EU_ERR_ARGUMENT and "render_ycbcr" in msg and "target" in msg
    rc, msg = call(args.target(3), s=None)
    assert rc == EU_ERR_ARGUMENT and "source" in msg
    rc, msg = call(args.target(3, 0, None, 1))
    assert rc == EU_ERR_ARGUMENT and "stage" in msg
    t = args.target(3)
    t.out_format = api.OUT_SRGBA8
    rc, msg = call(t)
    assert rc == EU_ERR_ARGUMENT and "SRGBA8" in msg
    for nch in (1, 2):
        rc, msg = call(args.target(nch))
        assert rc == EU_ERR_ARGUMENT and "nchannels" in msg
    rc, msg = call(args.target(3), dst=None)
    assert rc == EU_ERR_ARGUMENT and "null dst" in msg
    rc, msg = call(args.target(3), dst=good(sub_x=4))
    assert rc == EU_ERR_ARGUMENT and "sub_x" in msg
    t = args.target(3)
    t.width = -1
    assert call(t)[0] == EU_ERR_ARGUMENT


def test_python_entries_refuse_other_arrays():
    fw = ea.ycbcr_forward("601")
    with pytest.raises(ea.EuError, match="shape"):
        ea.ycbcr_planes(np.zeros((4, 4, 2), np.float32), fw)
    with pytest.raises(ea.EuError, match="planes of a"):
        ea.ycbcr_planes(FRAME, fw, out=(Y8, (np.zeros((3, 5), np.uint8), np.zeros((3, 5), np.uint8))))
    with pytest.raises(ea.EuError, match="uint8"):
        ea.ycbcr_planes(FRAME, fw, out=(Y16, (C16[..., 0], C16[..., 1])))
    with pytest.raises(ea.EuError, match="subsampling"):
        ea.ycbcr_planes(FRAME, fw, (4, 1))
    with pytest.raises(ea.EuError, match="forward"):
        ea.ycbcr_planes(FRAME, (1, 2, 3, 4))
    with pytest.raises(ea.EuError, match="depth"):
        ea.ycbcr_steps(8, 10)


# ---- the stand-alone program: io::y4m_writer, io::ycbcr_steps, the header text ----------------------------------------

def build_demo(name, *flags):
    exe = os.path.join(ROOT, "envutil_amd", "build", name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", *flags, "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "csrc", "ycbcr_out_demo.cc"), "-o", exe])
    return exe


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def demo(request):
    exe = (build_demo("ycbcr_out_demo") if request.param == "plain" else
           build_demo("ycbcr_out_demo_san", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan"))

    def run(*argv):
        return subprocess.run([exe] + [str(a) for a in argv], capture_output=True, text=True, timeout=300)
    return run


def test_demo_selftest(demo, tmp_path):
    """every format and depth at odd sizes written with y4m_writer and read back with y4m_reader; the header text;
    truncated and refused parameters"""
    r = demo("selftest", tmp_path)
    assert r.returncode == 0 and "failures: 0" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("depth,full", [(8, False), (8, True), (10, False), (12, True)])
def test_demo_steps_equal_python(demo, tmp_path, depth, full):
    """io::ycbcr_steps is ycbcr_steps, bit for bit"""
    bits = 8 if depth == 8 else 16
    r = demo("steps", bits, depth, int(full), tmp_path / "steps.f32")
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(tmp_path / "steps.f32", np.uint32).reshape(2, 1 << bits)
    want = np.stack(ea.ycbcr_steps(bits, depth, full)).view(np.uint32)
    nan = np.isnan(want.view(np.float32))
    assert np.array_equal(np.isnan(got.view(np.float32)), nan) and np.array_equal(got[~nan], want[~nan])


def test_demo_planes_equal_the_model(demo, tmp_path):
    """the header's host loop, compiled by the host compiler alone, on a frame with odd sizes: the model's planes in a
    .y4m file of one frame"""
    rng = np.random.default_rng(11)
    frame = om.random_frame(rng, 7, 9, 3, specials=False)
    frame.tofile(tmp_path / "frame.f32")
    for fmt, (sx, sy) in (("420", (2, 2)), ("422", (2, 1)), ("444", (1, 1))):
        for depth in (8, 10):
            out = tmp_path / f"o{fmt}_{depth}.y4m"
            r = demo("encode", tmp_path / "frame.f32", 9, 7, fmt, depth, "709", out)
            assert r.returncode == 0, r.stdout + r.stderr
            raw = open(out, "rb").read()
            head, rest = raw.split(b"\n", 1)
            tag = b"C420jpeg" if (fmt, depth) == ("420", 8) else b"C" + fmt.encode() + (b"" if depth == 8 else b"p%d" % depth)
            assert head.split() == [b"YUV4MPEG2", b"W9", b"H7", b"F25:1", b"Ip", b"A1:1", tag], head
            assert rest.startswith(b"FRAME\n")
            bits = 8 if depth == 8 else 16
            ys, cs = ea.ycbcr_steps(bits, depth)
            y, cb, cr = om.planes(frame, ea.ycbcr_forward("709"), sx, sy, bits, 0, ys, cs)
            le = lambda a: a.astype("<u2" if bits == 16 else np.uint8).tobytes()                               # noqa: E731
            assert rest[6:] == le(y) + le(cb) + le(cr), (fmt, depth)
