"""A .y4m --output on the command line (envutil_hip; eu_hip_render_ycbcr behind io::y4m_writer): the stream's frame
equals ycbcr_planes of the .pfm output of the same job; --frames FIRST LAST writes one stream whose frames are, byte
for byte, those of --frames k k runs; a .y4m stream in and out; and what the route refuses, each with its message."""
import numpy as np
import pytest

import envutil_amd as ea
import ycbcr_model as ym
from test_cli import cli, write_pfm, read_pfm, synth  # noqa: F401  (cli: the fixture)
from test_frames_host import y4m_bytes

pytestmark = pytest.mark.gpu

FACET = ["spherical", "360", "10", "5", "0"]
TARGET = ["--projection", "rectilinear", "--hfov", "80", "--width", "65", "--height", "37", "--degree", "3"]
OW, OH = 65, 37


def stream_of(path):
    """(header tokens, [frame payloads]) of a .y4m file"""
    raw = path.read_bytes()
    head, rest = raw.split(b"\n", 1)
    frames = rest.split(b"FRAME\n")
    assert frames[0] == b""
    return head.split(), frames[1:]


def le_bytes(planes, bits):
    return b"".join(np.ascontiguousarray(p, "<u2" if bits == 16 else np.uint8).tobytes() for p in planes)


@pytest.mark.parametrize("fmt,depth,sub,extra,tag", [
    ("420", 8, (2, 2), [], b"C420jpeg"), ("422", 8, (2, 1), ["--ycbcr_matrix", "2020"], b"C422"),
    ("444", 8, (1, 1), ["--ycbcr_range", "full"], b"C444"), ("420", 10, (2, 2), ["--ycbcr_matrix", "709", "--fps", "30000:1001"], b"C420p10")])
def test_a_y4m_output_is_the_planes_of_the_pfm_output(cli, tmp_path, fmt, depth, sub, extra, tag):
    write_pfm(tmp_path / "pano.pfm", synth(256, 128, 3) * np.float32(1.6) - np.float32(0.3))
    job = ["--facet", "pano.pfm"] + FACET + TARGET
    assert cli(job + ["--output", "out.pfm"], tmp_path).returncode == 0
    r = cli(job + extra + ["--y4m_format", fmt, "--y4m_depth", str(depth), "--output", "out.y4m", "-v"], tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Y'CbCr planes, encoded on the device" in r.stdout and "frame 0" in r.stdout, r.stdout
    head, frames = stream_of(tmp_path / "out.y4m")
    full = "full" in extra
    fps = b"F" + extra[extra.index("--fps") + 1].encode() if "--fps" in extra else b"F25:1"
    assert head == [b"YUV4MPEG2", b"W65", b"H37", fps, b"Ip", b"A1:1", tag] + ([b"XCOLORRANGE=FULL"] if full else []), head
    assert len(frames) == 1
    bits = 8 if depth == 8 else 16
    matrix = extra[extra.index("--ycbcr_matrix") + 1] if "--ycbcr_matrix" in extra else "601"          # 37 rows: below 720
    ys, cs = ea.ycbcr_steps(bits, depth, full)
    y, (cb, cr) = ea.ycbcr_planes(read_pfm(tmp_path / "out.pfm"), ea.ycbcr_forward(matrix), sub, bits=bits, y_steps=ys, c_steps=cs)
    assert frames[0] == le_bytes((y, cb, cr), bits)
    assert len(np.unique(y)) > 50 and len(np.unique(cb)) > 8


def test_frames_make_one_stream_of_the_frames_of_single_runs(cli, tmp_path):
    """.y4m in and .y4m out together: --ycbcr_matrix and --ycbcr_range govern both ends"""
    rng = np.random.default_rng(21)
    w, h = 96, 48
    raw = []
    for _ in range(5):
        planes = ym.planes(rng, h, w, 2, 2, 8, "planar")
        raw.append(le_bytes(planes, 8))
    (tmp_path / "clip.y4m").write_bytes(y4m_bytes(w, h, "C420jpeg", raw))
    job = ["--facet", "clip.y4m"] + FACET + TARGET + ["--ycbcr_matrix", "709", "--ycbcr_range", "full"]
    r = cli(job + ["--frames", "0", "3", "--output", "seq.y4m", "-v"], tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("eu_hip_source_reload") == 3 and r.stdout.count("encoded on the device") == 4, r.stdout
    head, frames = stream_of(tmp_path / "seq.y4m")
    assert head == [b"YUV4MPEG2", b"W65", b"H37", b"F25:1", b"Ip", b"A1:1", b"C420jpeg", b"XCOLORRANGE=FULL"] and len(frames) == 4
    for k in range(4):
        r = cli(job + ["--frames", str(k), str(k), "--output", f"one_{k}.y4m"], tmp_path)
        assert r.returncode == 0, r.stderr
        h1, f1 = stream_of(tmp_path / f"one_{k}.y4m")
        assert h1 == head and len(f1) == 1 and f1[0] == frames[k], f"frame {k}"
    assert frames[0] != frames[3]
    # ... and a frame is the planes of the same job's float output
    assert cli(job + ["--frames", "2", "2", "--output", "two_%d.pfm"], tmp_path).returncode == 0
    ys, cs = ea.ycbcr_steps(8, 8, True)
    y, (cb, cr) = ea.ycbcr_planes(read_pfm(tmp_path / "two_2.pfm"), ea.ycbcr_forward("709"), y_steps=ys, c_steps=cs)
    assert frames[2] == le_bytes((y, cb, cr), 8)
    # without --frames: one frame, the stream's frame 0
    assert cli(job + ["--output", "plain.y4m"], tmp_path).returncode == 0
    assert stream_of(tmp_path / "plain.y4m")[1] == frames[:1]
    # the stream reads back as a facet
    assert cli(["--facet", "seq.y4m"] + FACET + TARGET + ["--frames", "1", "2", "--output", "back_%d.pfm"], tmp_path).returncode == 0


def test_refusals(cli, tmp_path):
    write_pfm(tmp_path / "a.pfm", synth(64, 32, 3))
    write_pfm(tmp_path / "a4.pfm", synth(64, 32, 4))
    write_pfm(tmp_path / "rays.pfm", synth(8, 8, 3))
    facet = ["--facet", "a.pfm"] + FACET
    small = ["--projection", "rectilinear", "--hfov", "60", "--width", "16", "--height", "8"]
    cases = [(["--facet", "a4.pfm"] + FACET + small + ["--output", "o.y4m"], "3 channels"),
             (facet + small + ["--nchannels", "1", "--output", "o.y4m"], "3 channels"),
             (facet + ["--facet", "a.pfm", "spherical", "360", "90", "0", "0"] + small + ["--split", "s%d.pfm", "--output", "o.y4m"], "--split"),
             (facet + small + ["--split", "s%d.y4m"], "--split"),
             (facet + small + ["--layer", "a.pfm", "l.y4m", "--output", "o.pfm"], "--layer"),
             (["--facet", "a.pfm", "spherical", "360", "0", "0", "0", "--ray_map", "rays.pfm", "--output", "o.y4m"], "does not go with --ray_map"),
             (facet + small + ["--output", "o.y4m", "--y4m_format", "411"], "--y4m_format"),
             (facet + small + ["--output", "o.y4m", "--y4m_depth", "9"], "--y4m_depth"),
             (facet + small + ["--output", "o.y4m", "--fps", "0"], "--fps"),
             (facet + small + ["--output", "o.y4m", "--fps", "25:x"], "--fps")]
    for argv, word in cases:
        r = cli(argv, tmp_path)
        assert r.returncode == 2 and word in r.stderr, (argv, r.stderr)
        assert not (tmp_path / "o.y4m").exists()
    r = cli(small + ["-"], tmp_path, stdin=" ".join(facet + ["--output", "o.y4m"]) + "\n")
    assert r.returncode == 2 and "pipe mode" in r.stderr and ".y4m" in r.stderr, r.stderr
    # --frames: every other extension still needs its conversion, with the message it has
    r = cli(facet[:1] + ["a%d.pfm"] + FACET + small + ["--frames", "0", "1", "--output", "o.ppm"], tmp_path)
    assert r.returncode == 2 and "--frames: --output" in r.stderr, r.stderr
