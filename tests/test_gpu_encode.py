"""Rendering to 8- and 16-bit samples (eu_hip_encode_samples, eu_hip_render_samples, eu_encode.hip; encode_samples,
render_samples, the command line's PNM / PAM outputs). 1: the kernel against the definition of a step table,
numpy.searchsorted(steps[1 : m + 1], v, side="right") with NaN -> 0, compared as bytes, with every byte outside the
rows checked. A thread owns an aligned dword of a destination row, one thread the bytes in front of the row's first
dword boundary, so widths, channel counts, row offsets and strides are chosen for every alignment. 2: render_samples
equals encode_samples of render's float frame. 3: the command line's files equal the host route's
(tests/csrc/encode_demo.cc). 4: the Python defaults."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import envutil_amd as ea
from envutil_amd import api
import jobs
import pixel_values as pv

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "envutil_amd", "bin", "envutil_hip")
WIDTHS = (1, 2, 3, 4, 5, 7, 63, 64, 65, 257)
HEIGHTS = (1, 2, 17)
GUARD, FILL = 64, 0xA5


@pytest.fixture(scope="module")
def demo():
    """tests/csrc/encode_demo.cc as a plain host program (the sanitizer build belongs to the host tests)"""
    exe = os.path.join(ROOT, "envutil_amd", "build", "encode_demo_plain")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-pthread", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "csrc", "encode_demo.cc"), "-o", exe])

    def run(*argv, ok=(0,)):
        r = subprocess.run([exe] + [str(a) for a in argv], capture_output=True, text=True, timeout=120)
        assert r.returncode in ok, r.stderr
        return r
    return run


@pytest.fixture(scope="module")
def steps(demo, tmp_path_factory):
    """(colour, alpha) step tables as io::encode_steps builds them: steps(bits, maxval, from, to)"""
    d = tmp_path_factory.mktemp("steps")
    kept = {}

    def get(bits, maxval, a="Linear", b="sRGB"):
        key = (bits, maxval, a, b)
        if key not in kept:
            f = d / f"{bits}_{maxval}_{a}_{b}.f32"
            demo("steps", bits, maxval, a, b, f)
            t = np.fromfile(f, np.float32).reshape(2, 1 << bits)
            kept[key] = (t[0].copy(), t[1].copy())
        return kept[key]
    return get


def code_of(table, v):
    """the definition: the number of k >= 1 with v >= steps[k]"""
    m = int((~np.isnan(table[1:])).sum())
    c = np.searchsorted(table[1:m + 1], v, side="right")
    c[np.isnan(v)] = 0
    return c


def want_bytes(frame, colour, alpha, bits, big_endian):
    """(h, w * nch * bits / 8) uint8: the rows the call has to write"""
    h, w, nch = frame.shape
    c = code_of(colour, frame.reshape(-1)).reshape(h, w, nch)
    if nch in (2, 4):
        c[..., -1] = code_of(alpha if alpha is not None else colour, frame[..., -1].reshape(-1)).reshape(h, w)
    dt = np.uint8 if bits == 8 else (">u2" if big_endian else "<u2")
    return np.ascontiguousarray(c.astype(dt)).view(np.uint8).reshape(h, -1)


def value_pool(tables):
    """every step itself (a stride of a 16-bit table) with the floats below and above it, and the fields of
    tests/pixel_values.py: both zeros, denormals, +-1e37, inf, NaN, values above 1, negatives"""
    parts = []
    for t in tables:
        m = int((~np.isnan(t[1:])).sum())
        s = t[1:m + 1]
        if m > 255:
            s = np.concatenate([s[::97], s[:3], s[-3:]])
        parts += [s, np.nextafter(s, np.float32(-np.inf)), np.nextafter(s, np.float32(np.inf))]
    for cls in pv.FINITE:
        parts.append(pv.scaled_unit(cls, 8, 16, 3).reshape(-1))
        parts.append(pv.make(cls, 4, 16, 3).reshape(-1))
    parts.append(pv.make("nonfinite", 16, 32, 3, one_in=10).reshape(-1))
    parts.append(np.array([0.0, -0.0, 1.0, np.inf, -np.inf, np.nan, 1e37, -1e37, 1e-45, -1e-45], np.float32))
    return np.concatenate([np.ascontiguousarray(p, np.float32) for p in parts])


def frame_from(pool, h, w, nch, seed):
    n = h * w * nch
    idx = (np.arange(n) * 7 + seed * 131) % pool.size
    return pool[idx].reshape(h, w, nch).copy()


def encode_raw(frame, colour, alpha, bits, big_endian, frame_mode, out_dev, off, pad):
    """eu_hip_encode_samples through ctypes, `out` at byte `off` of a buffer filled with 0xA5 with GUARD bytes either
    side and `pad` bytes behind every row. frame_mode: 0 host dense, 1 host padded, 2 device dense, 3 device padded.
    Returns the whole buffer afterwards and the row stride."""
    import torch
    h, w, nch = frame.shape
    row = w * nch * (bits // 8)
    stride = row + pad
    total = GUARD + off + h * stride + GUARD
    fpad = 3 if frame_mode in (1, 3) else 0
    fhost = np.full((h, w * nch + fpad), np.float32(0.25), np.float32)
    fhost[:, :w * nch] = frame.reshape(h, -1)
    keep = [fhost]
    if frame_mode >= 2:
        ft = torch.from_numpy(fhost).cuda()
        keep.append(ft)
        fptr = ft.data_ptr()
    else:
        fptr = fhost.ctypes.data
    if out_dev:
        ot = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
        optr = ot.data_ptr() + GUARD + off
    else:
        oh = np.full(total, FILL, np.uint8)
        optr = oh.ctypes.data + GUARD + off
    torch.cuda.synchronize()
    e = api.Encode(bits, int(big_endian), colour.ctypes.data, alpha.ctypes.data if alpha is not None else None)
    rc = api.lib().eu_hip_encode_samples(C.c_void_p(fptr), fhost.shape[1] * 4, int(frame_mode >= 2), w, h, nch, C.byref(e),
                                         C.c_void_p(optr), stride, int(out_dev), None)
    assert rc == 0, api.lib().eu_hip_last_error().decode()
    ea.sync()
    return (ot.cpu().numpy() if out_dev else oh), stride


def check_buffer(buf, stride, want, off, what):
    h, row = want.shape
    body = buf[GUARD + off:GUARD + off + h * stride].reshape(h, stride)
    bad = int((body[:, :row] != want).sum())
    assert bad == 0, f"{what}: {bad} of {want.size} bytes differ"
    outside = buf.copy()
    outside[GUARD + off:GUARD + off + h * stride].reshape(h, stride)[:, :row] = FILL
    assert (outside == FILL).all(), f"{what}: {int((outside != FILL).sum())} bytes outside the rows were written"


@pytest.mark.parametrize("nch", [1, 2, 3, 4])
def test_encode_8_bit_against_the_definition(nch, steps):
    colour, alpha = steps(8, 255)
    pool = value_pool([colour, alpha])
    k = 0
    for h in HEIGHTS:
        for w in WIDTHS:
            frame = frame_from(pool, h, w, nch, w + 1000 * h)
            want = want_bytes(frame, colour, alpha, 8, False)
            for off in (0, 1, 3):
                for pad in (0, 5):
                    buf, stride = encode_raw(frame, colour, alpha, 8, False, k % 4, True, off, pad)
                    check_buffer(buf, stride, want, off, (w, h, nch, off, pad, k % 4))
                    k += 1
            buf, stride = encode_raw(frame, colour, alpha, 8, False, k % 4, False, 1, 2)
            check_buffer(buf, stride, want, 1, (w, h, nch, "host out", k % 4))


@pytest.mark.parametrize("big_endian", [False, True])
@pytest.mark.parametrize("nch", [1, 2, 3, 4])
def test_encode_16_bit_against_the_definition(nch, big_endian, steps):
    colour, alpha = steps(16, 65535)
    pool = value_pool([colour, alpha])
    k = 0
    for h in HEIGHTS:
        for w in WIDTHS:
            frame = frame_from(pool, h, w, nch, w + 1000 * h)
            want = want_bytes(frame, colour, alpha, 16, big_endian)
            for off in (0, 2):
                for pad in (0, 6):
                    buf, stride = encode_raw(frame, colour, alpha, 16, big_endian, k % 4, True, off, pad)
                    check_buffer(buf, stride, want, off, (w, h, nch, off, pad, k % 4, big_endian))
                    k += 1
            buf, stride = encode_raw(frame, colour, alpha, 16, big_endian, k % 4, False, 2, 2)
            check_buffer(buf, stride, want, 2, (w, h, nch, "host out", k % 4, big_endian))


def test_every_step_of_the_16_bit_table(steps):
    """all 65535 steps with the floats either side, in one frame: every leaf of the search"""
    colour, alpha = steps(16, 65535)
    s = colour[1:]
    v = np.concatenate([s, np.nextafter(s, np.float32(-np.inf)), np.nextafter(s, np.float32(np.inf)), np.zeros(3, np.float32)])
    frame = v.reshape(64, 1024, 3)
    got = ea.encode_samples(frame, colour, bits=16)
    assert np.array_equal(got.reshape(-1), code_of(colour, v).astype(np.uint16))


def test_more_rows_than_a_launch_has_workgroups(steps):
    """a launch has at most 4096 workgroups of 8 rows each: a taller frame is walked in strides"""
    for bits in (8, 16):
        colour, alpha = steps(bits, (1 << bits) - 1)
        frame = frame_from(value_pool([colour]), 8 * 4096 * 2 + 77, 3, 3, bits)
        got = ea.encode_samples(frame, colour, bits=bits)
        assert np.array_equal(got, code_of(colour, frame.reshape(-1)).reshape(frame.shape).astype(got.dtype))


def test_tables_with_a_nan_tail_and_equal_neighbours(steps):
    """maxval 100: codes above it are never produced, +inf is code 100; equal neighbours skip a code"""
    for bits in (8, 16):
        colour, alpha = steps(bits, 100)
        eq = colour.copy()
        eq[10:20] = eq[10]
        eq[50:53] = eq[52]
        for tab in (colour, eq):
            pool = value_pool([tab])
            frame = frame_from(pool, 17, 65, 3, 5)
            frame[0, 0] = (np.inf, np.nan, 3e38)
            got = ea.encode_samples(frame, tab, bits=bits)
            want = code_of(tab, frame.reshape(-1)).reshape(frame.shape)
            assert np.array_equal(got, want.astype(got.dtype))
            assert got.max() == 100 and got[0, 0, 0] == 100 and got[0, 0, 1] == 0
        got = ea.encode_samples(frame, eq, bits=bits)
        assert not np.isin(got, np.arange(10, 19)).any() and (got == 19).any()


def test_alpha_table_differs_from_the_colour_table(steps):
    colour, alpha = steps(8, 255)
    assert not np.array_equal(colour[1:], alpha[1:])
    pool = value_pool([colour, alpha])
    for nch in (2, 4):
        frame = frame_from(pool, 17, 63, nch, nch)
        got = ea.encode_samples(frame, colour, alpha)
        assert np.array_equal(got.view(np.uint8).reshape(17, -1), want_bytes(frame, colour, alpha, 8, False))
        # no alpha table: the colour table for the last channel too
        got = ea.encode_samples(frame, colour)
        assert np.array_equal(got.view(np.uint8).reshape(17, -1), want_bytes(frame, colour, None, 8, False))


# ------------------------------------------------------------------------------------------ render_samples
@pytest.fixture(scope="module")
def pano():
    """a lat/lon source whose values leave [0, 1] on both sides, with an alpha channel that is not all 1"""
    img = jobs.synth_image(256, 128, 4)
    img[..., :3] = img[..., :3] * np.float32(1.8) - np.float32(0.35)
    img[..., 3] = pv.alpha_plane(128, 256)
    return ea.Source.load(ea.facet_spec(ea.SPHERICAL, 256, 128, 360.0, nchannels=4), img, 3)


def same_as_encode_of_render(args, sources, steps, what, nchannels=None, **kw):
    frame = ea.render(args, sources, nchannels=nchannels, **kw)
    for bits, be in ((8, False), (16, True), (16, False)):
        colour, alpha = steps(bits, (1 << bits) - 1)
        want = ea.encode_samples(frame, colour, alpha, bits=bits, big_endian=be)
        got = ea.render_samples(args, sources, nchannels=nchannels, colour_steps=colour, alpha_steps=alpha, bits=bits,
                                big_endian=be, **kw)
        assert got.shape == frame.shape and got.dtype == want.dtype
        assert np.array_equal(got, want), f"{what}, {bits} bit: {int((got != want).sum())} of {got.size} samples differ"
        assert len(np.unique(got)) > 8, what
    return frame


def test_render_samples_latlon_to_rectilinear(pano, steps):
    args = ea.arguments(ea.RECTILINEAR, 65, 33, 80.0, yaw=30, pitch=-12, roll=5, spline_degree=3)
    for nch in (4, 3, 1):
        same_as_encode_of_render(args, pano, steps, f"65 x 33, {nch} channels", nchannels=nch)
    same_as_encode_of_render(ea.arguments(ea.RECTILINEAR, 65, 33, 80.0, spline_degree=3, twine=2), pano, steps, "twined")


def test_render_samples_cubemap_target(pano, steps):
    same_as_encode_of_render(ea.arguments(ea.CUBEMAP, 16, 96, 90.0, spline_degree=3), pano, steps, "cubemap 16")


def test_render_samples_two_facets(steps):
    a = jobs.synth_image(96, 64, 4, seed=3) * np.float32(1.5) - np.float32(0.2)
    b = jobs.synth_image(96, 64, 4, seed=4) * np.float32(1.5) - np.float32(0.2)
    a[..., 3] = 1.0
    b[..., 3] = 1.0
    fa = ea.Source.load(ea.facet_spec(ea.RECTILINEAR, 96, 64, 70.0, nchannels=4, yaw=-20.0), a, 1)
    fb = ea.Source.load(ea.facet_spec(ea.RECTILINEAR, 96, 64, 70.0, nchannels=4, yaw=25.0, pitch=5.0), b, 1)
    args = ea.arguments(ea.SPHERICAL, 130, 47, 150.0, spline_degree=1)
    frame = same_as_encode_of_render(args, [fa, fb], steps, "two facets")
    assert (frame[..., 3] == 0).any() and (frame[..., 3] == 1).any()
    same_as_encode_of_render(ea.arguments(ea.SPHERICAL, 130, 47, 150.0, spline_degree=1, synopsis="hdr_merge"), [fa, fb],
                             steps, "two facets, hdr_merge")


def test_render_samples_crop_and_row_slice(pano, steps):
    same_as_encode_of_render(ea.arguments(ea.SPHERICAL, 120, 60, 360.0, spline_degree=1, crop=(13, 78, 7, 40)), pano, steps,
                             "crop")
    args = ea.arguments(ea.RECTILINEAR, 65, 33, 80.0, spline_degree=1)
    same_as_encode_of_render(args, pano, steps, "rows 5 .. 22", row_begin=5, row_end=22)
    same_as_encode_of_render(args, pano, steps, "bands", band=(4, 2, 1))
    assert ea.render_samples(args, pano, row_begin=7, row_end=7).shape == (0, 65, 4)


def test_render_samples_four_chunks_to_the_host(pano, steps):
    """1030 rows: the pipeline of four row chunks of 264, 264, 264 and 238 rows; 8 pixels of 3 channels make rows
    of 24 bytes, and a padded host buffer keeps its padding"""
    args = ea.arguments(ea.SPHERICAL, 8, 1030, 20.0, spline_degree=1)
    same_as_encode_of_render(args, pano, steps, "8 x 1030")
    colour, alpha = steps(8, 255)
    big = np.full((1030, 8 * 3 + 5), FILL, np.uint8)
    out = big[:, :24].reshape(1030, 8, 3)
    assert out.base is not None and np.shares_memory(out, big)
    ea.render_samples(args, pano, nchannels=3, colour_steps=colour, out=out)
    assert np.array_equal(out, ea.encode_samples(ea.render(args, pano, nchannels=3), colour))
    assert (big[:, 24:] == FILL).all()


def test_render_samples_device_out_on_a_stream(pano, steps):
    import torch
    args = ea.arguments(ea.RECTILINEAR, 65, 33, 80.0, yaw=10, spline_degree=3)
    frame = ea.render(args, pano)
    stream = torch.cuda.Stream()
    for bits in (8, 16):
        colour, alpha = steps(bits, (1 << bits) - 1)
        want = ea.encode_samples(frame, colour, alpha, bits=bits)
        big = torch.from_numpy(np.full((33, 65 + 2, 4), 0x5A if bits == 8 else 0x5A5A, np.uint8 if bits == 8 else np.uint16)).cuda()
        torch.cuda.synchronize()
        out = big[:, :65]
        ea.render_samples(args, pano, colour_steps=colour, alpha_steps=alpha, bits=bits, out=out, stream=stream.cuda_stream)
        # other tables on the library's own stream right behind it: the call waits for the first before it rewrites them
        other = ea.render_samples(args, pano, bits=bits)
        stream.synchronize()
        ea.sync()
        host = big.cpu().numpy()
        assert np.array_equal(host[:, :65], want)
        assert (host[:, 65:] == (0x5A if bits == 8 else 0x5A5A)).all()
        assert np.array_equal(other, ea.encode_samples(frame, bits=bits))


# ------------------------------------------------------------------------------------------ the command line
def write_pfm(path, img):
    h, w, n = img.shape
    with open(path, "wb") as f:
        f.write({1: b"Pf", 3: b"PF", 4: b"PF4"}[n] + b"\n%d %d\n-1.0\n" % (w, h))
        f.write(np.ascontiguousarray(img[::-1], "<f4").tobytes())


@pytest.fixture(scope="module")
def cli():
    if not os.path.exists(EXE) or not os.path.exists(ea.lib_path()):
        ea.build()

    def run(argv, cwd):
        r = subprocess.run([EXE] + list(argv), capture_output=True, text=True, cwd=str(cwd), timeout=600)
        assert r.returncode == 0, r.stderr
        return r
    return run


def payload(path):
    raw = open(path, "rb").read()
    if raw[:2] == b"P7":
        head, _, data = raw.partition(b"ENDHDR\n")
        return head, data
    # P5 / P6: magic, comment lines, "w h", maxval
    lines, pos = 0, 0
    while lines < 3:
        end = raw.index(b"\n", pos)
        if raw[pos:pos + 1] != b"#":
            lines += 1
        pos = end + 1
    return raw[:pos], raw[pos:]


def test_command_line_files_equal_the_host_route(cli, demo, tmp_path):
    img = jobs.synth_image(256, 128, 3) * np.float32(1.6) - np.float32(0.3)
    write_pfm(tmp_path / "pano.pfm", img)
    job = ["--facet", "pano.pfm", "spherical", "360", "0", "0", "0", "--projection", "rectilinear", "--hfov", "80", "--width", "65",
           "--height", "33", "--yaw", "20", "--degree", "3", "--twine", "0"]
    cli(job + ["--output", "out.pfm"], tmp_path)
    r = cli(job + ["--output_colour_space", "sRGB", "--output", "out.ppm", "-v"], tmp_path)
    assert "8-bit samples, encoded on the device" in r.stdout, r.stdout
    demo("host", tmp_path / "out.pfm", tmp_path / "want.ppm", "Linear", "sRGB")
    head, data = payload(tmp_path / "out.ppm")
    whead, wdata = payload(tmp_path / "want.ppm")
    assert data == wdata and len(data) == 65 * 33 * 3 and len(set(data)) > 100
    assert head.startswith(b"P6\n# Projection: rectilinear\n") and head.endswith(b"65 33\n255\n")
    # four channels, 16 bit
    cli(job + ["--nchannels", "4", "--output", "out4.pfm"], tmp_path)
    r = cli(job + ["--nchannels", "4", "--output_colour_space", "sRGB", "--output", "out4.pam", "-v"], tmp_path)
    assert "16-bit samples, encoded on the device" in r.stdout, r.stdout
    demo("host", tmp_path / "out4.pfm", tmp_path / "want4.pam", "Linear", "sRGB")
    head, data = payload(tmp_path / "out4.pam")
    assert data == payload(tmp_path / "want4.pam")[1] and len(data) == 65 * 33 * 4 * 2
    assert b"# Projection: rectilinear" in head and b"DEPTH 4" in head and b"MAXVAL 65535" in head and b"RGB_ALPHA" in head
    # a table the builder refuses: the host route, said so, and still the same bytes
    cli(job + ["--working_colour_space", "Rec709", "--output_colour_space", "Rec709", "--input_colour_space", "Rec709",
               "--output", "r.pfm"], tmp_path)
    r = cli(job + ["--working_colour_space", "Rec709", "--output_colour_space", "Linear", "--input_colour_space", "Rec709",
                   "--output", "r.pam", "-v"], tmp_path)
    assert "encoded on the host" in r.stdout and "no step function" in r.stdout, r.stdout
    demo("host", tmp_path / "r.pfm", tmp_path / "rwant.pam", "Rec709", "Linear")
    assert payload(tmp_path / "r.pam")[1] == payload(tmp_path / "rwant.pam")[1]
    # ... while the same pair at 8 bit is a step function
    r = cli(job + ["--working_colour_space", "Rec709", "--output_colour_space", "Linear", "--input_colour_space", "Rec709",
                   "--output", "r.ppm", "-v"], tmp_path)
    assert "encoded on the device" in r.stdout, r.stdout
    demo("host", tmp_path / "r.pfm", tmp_path / "rwant.ppm", "Rec709", "Linear")
    assert payload(tmp_path / "r.ppm")[1] == payload(tmp_path / "rwant.ppm")[1]


def test_command_line_cubemap_faces(cli, demo, tmp_path):
    img = jobs.synth_image(256, 128, 3) * np.float32(1.6) - np.float32(0.3)
    write_pfm(tmp_path / "pano.pfm", img)
    job = ["--facet", "pano.pfm", "spherical", "360", "0", "0", "0", "--projection", "cubemap", "--hfov", "90", "--width", "33",
           "--degree", "1", "--twine", "0"]
    cli(job + ["--output", "cube.pfm"], tmp_path)
    r = cli(job + ["--output_colour_space", "sRGB", "--output", "face_%s.ppm", "-v"], tmp_path)
    assert "encoded on the device" in r.stdout, r.stdout
    demo("host", tmp_path / "cube.pfm", tmp_path / "want_%s.ppm", "Linear", "sRGB", "cube")
    for name in ("left", "right", "top", "bottom", "front", "back"):
        head, data = payload(tmp_path / f"face_{name}.ppm")
        assert data == payload(tmp_path / f"want_{name}.ppm")[1] and len(data) == 33 * 33 * 3, name
        assert head == b"P6\n# Projection: rectilinear\n# Hfov: 90\n33 33\n255\n", head


# ------------------------------------------------------------------------------------------ Python defaults
def test_python_default_tables_are_the_quantiser():
    rng = np.random.default_rng(11)
    v = (rng.random((33, 65, 3)) * 1.3 - 0.15).astype(np.float32)
    v[0, :6, 0] = (0.0, -0.0, 1.0, 0.5, 1e-40, 3e38)
    for bits, maxvals, dt in ((8, (255, 100), np.uint8), (16, (65535, 1000), np.uint16)):
        for mv in maxvals:
            want = (np.clip(v, 0, 1) * np.float32(mv) + np.float32(0.5)).astype(dt)
            got = ea.encode_samples(v, bits=bits, maxval=mv)
            assert got.dtype == dt and np.array_equal(got, want), (bits, mv)
    assert np.array_equal(ea.encode_samples(v, bits=16, big_endian=True).view(">u2"), (np.clip(v, 0, 1) * np.float32(65535) + np.float32(0.5)).astype(np.uint16))


def test_torch_tensors_in_and_out():
    import torch
    rng = np.random.default_rng(12)
    v = (rng.random((3, 17, 63, 4)) * 1.3 - 0.15).astype(np.float32)
    t = torch.from_numpy(v).cuda()
    for bits, dt, tdt in ((8, np.uint8, torch.uint8), (16, np.uint16, torch.uint16)):
        want = (np.clip(v, 0, 1) * np.float32((1 << bits) - 1) + np.float32(0.5)).astype(dt)
        got = ea.encode_samples(t, bits=bits)
        ea.sync()
        assert got.is_cuda and got.dtype == tdt and np.array_equal(got.cpu().numpy(), want)
        # a padded view of a device frame into a padded view of a device buffer
        wide = torch.zeros((17, 70, 4), dtype=torch.float32, device="cuda")
        wide[:, :63] = t[1]
        out = torch.zeros((17, 66, 4), dtype=tdt, device="cuda")
        ea.encode_samples(wide[:, :63], bits=bits, out=out[:, :63])
        ea.sync()
        host = out.cpu().numpy()
        assert np.array_equal(host[:, :63], want[1]) and (host[:, 63:] == 0).all()
        # a device frame to host samples, a host frame to device samples
        assert np.array_equal(ea.encode_samples(t[2], bits=bits, out=np.zeros((17, 63, 4), dt)), want[2])
        dev = ea.encode_samples(v[0], bits=bits, out=torch.zeros((17, 63, 4), dtype=tdt, device="cuda"))
        ea.sync()
        assert np.array_equal(dev.cpu().numpy(), want[0])
