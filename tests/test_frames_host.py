"""Frame sequences on the command line, without a device: the YUV4MPEG2 header parser and reader, the names of a
numbered sequence and the argument checks of --frames (include/eu_image_io.hpp) through a small host program,
tests/csrc/frames_demo.cc - every accepted and every refused colour tag, a truncated frame, FIRST > LAST, names without a
conversion or with two - and what envutil_hip itself refuses before it looks for a device, each with its own message."""
import os
import subprocess

import numpy as np
import pytest

import envutil_amd as ea
from test_cli import EXE as CLI, write_pfm, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "envutil_amd", "build", "frames_demo")

GOOD = {"": (2, 2, 8, 8), "C420": (2, 2, 8, 8), "C420jpeg": (2, 2, 8, 8), "C420mpeg2": (2, 2, 8, 8), "C420paldv": (2, 2, 8, 8),
        "C422": (2, 1, 8, 8), "C444": (1, 1, 8, 8)}
for _base, (_sx, _sy) in (("C420", (2, 2)), ("C422", (2, 1)), ("C444", (1, 1))):
    for _d in (10, 12, 16):
        GOOD[f"{_base}p{_d}"] = (_sx, _sy, 16, _d)
BAD = ["Cmono", "Cmono16", "C444alpha", "C420jpegp10", "C420mpeg2p10", "C411", "C420p9", "C420p14", "C", "Cyuv"]


@pytest.fixture(scope="module")
def demo():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "csrc", "frames_demo.cc"), "-o", EXE])

    def run(*argv):
        r = subprocess.run([EXE] + [str(a) for a in argv], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout.strip()
    return run


@pytest.fixture(scope="module")
def cli():
    if not os.path.exists(CLI) or not os.path.exists(ea.lib_path()):
        ea.build()

    def run(argv, cwd, stdin=None):
        return subprocess.run([CLI] + list(argv), capture_output=True, text=True, cwd=str(cwd), input=stdin, timeout=120)
    return run


def test_selftest_reads_back_every_accepted_tag_at_odd_sizes(demo, tmp_path):
    out = demo("selftest", tmp_path)
    assert "FAILED" not in out and "all ok" in out, out


def test_every_accepted_colour_tag(demo):
    assert len(GOOD) == 16
    for tag, (sx, sy, bits, depth) in GOOD.items():
        w, h = 7, 5
        cw, ch = (w + sx - 1) // sx, (h + sy - 1) // sy
        got = demo("header", f"YUV4MPEG2 W{w} H{h} F30:1 Ip A1:1 {tag}".strip())
        assert got == f"ok {w} {h} {sx} {sy} {bits} {depth} 0 {w * h * bits // 8} {cw * ch * bits // 8}", (tag, got)
    assert demo("header", "YUV4MPEG2 W7 H5 C444p10 XCOLORRANGE=FULL").split()[7] == "1"
    assert demo("header", "YUV4MPEG2 W7 H5 XCOLORRANGE=LIMITED").split()[7] == "0"


def test_every_refused_colour_tag_and_header(demo):
    for tag in BAD:
        got = demo("header", f"YUV4MPEG2 W8 H4 {tag}")
        assert got.startswith("refused:") and "colour tag" in got and tag in got, (tag, got)
    for line in ("YUV4MPEG W8 H4", "YUV4MPEG2 W8", "YUV4MPEG2 H4", "YUV4MPEG2 W0 H4", "YUV4MPEG2 Wx H4", "P6 8 4 255", ""):
        assert demo("header", line).startswith("refused:"), line


def y4m_bytes(w, h, tag, frames):
    head = f"YUV4MPEG2 W{w} H{h} F25:1 {tag}".strip().encode() + b"\n"
    return head + b"".join(b"FRAME\n" + f for f in frames)


def test_frames_are_read_forward_and_a_truncated_one_is_refused(demo, tmp_path):
    rng = np.random.default_rng(1)
    w, h = 5, 3
    n = w * h + 2 * 3 * 2
    frames = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for _ in range(3)]
    p = tmp_path / "s.y4m"
    p.write_bytes(y4m_bytes(w, h, "C420jpeg", frames))
    out = demo("read", p, 0, 2, 1, 3).splitlines()
    assert out[0] == f"frame 0: {n} bytes, sum {sum(frames[0])}" and out[1] == f"frame 2: {n} bytes, sum {sum(frames[2])}"
    assert out[2].startswith("refused:") and "forward" in out[2] and "frame 1" in out[2]
    assert out[3].startswith("refused:") and "frame 3" in out[3]
    p.write_bytes(y4m_bytes(w, h, "C420jpeg", frames)[:-1])
    out = demo("read", p, 1, 2).splitlines()
    assert out[0].startswith("frame 1:") and out[1].startswith("refused:") and "truncated" in out[1] and "frame 2" in out[1]
    p.write_bytes(y4m_bytes(w, h, "C420jpeg", frames[:1]) + b"FRAMX\n" + frames[1])
    assert "no FRAME header" in demo("read", p, 1)
    assert demo("read", tmp_path / "none.y4m", 0).startswith("refused: cannot open")


def test_frames_argument_checks(demo):
    assert demo("check", 0, 9, "in%d.pfm", "out%03d.pfm") == "ok 0 9"
    assert demo("check", 4, 4, "clip.y4m", "out%d.ppm") == "ok 4 4"
    assert demo("name", "f%04d.ppm", 12) == "ok f0012.ppm"
    for argv, word in ((("5", "4", "in%d.pfm", "out%d.pfm"), "beyond"), (("-1", "4", "in%d.pfm", "out%d.pfm"), "at least 0"),
                       (("0", "1.5", "in%d.pfm", "out%d.pfm"), "whole numbers"), (("0", "1", "in.pfm", "out%d.pfm"), "no conversion"),
                       (("0", "1", "in%d_%d.pfm", "out%d.pfm"), "2 conversions"), (("0", "1", "face_%s.pfm", "out%d.pfm"), "cubemap"),
                       (("0", "1", "in%d.pfm", "out.pfm"), "--output"), (("0", "1", "in.y4m", "o%d_%02d.pfm"), "--output"),
                       (("0", "1", "in%f.pfm", "out%d.pfm"), "image")):
        got = demo("check", *argv)
        assert got.startswith("refused:") and word in got, (argv, got)


def test_the_command_line_refuses_what_a_sequence_does_not_do(cli, tmp_path):
    for k in range(2):
        write_pfm(tmp_path / f"a{k}.pfm", synth(32, 16, 3, seed=k))
    facet = ["--facet", "a%d.pfm", "spherical", "360", "0", "0", "0"]
    common = ["--projection", "rectilinear", "--hfov", "90", "--width", "16", "--height", "8"]
    cases = [(facet + facet + ["--frames", "0", "1", "--output", "o%d.pfm"], "ONE facet"),
             (["--pto", "x.pto", "--frames", "0", "1", "--output", "o%d.pfm"], "--pto"),
             (facet + ["--layer", "a1.pfm", "l.pfm", "--frames", "0", "1", "--output", "o%d.pfm"], "--layer"),
             (facet + ["--split", "s%d.pfm", "--frames", "0", "1", "--output", "o%d.pfm"], "--split"),
             (facet + ["--ray_map", "r.pfm", "--frames", "0", "1", "--output", "o%d.pfm"], "--ray_map"),
             (["--facet", "a%s.pfm", "cubemap", "90", "0", "0", "0", "--frames", "0", "1", "--output", "o%d.pfm"], "cubemap"),
             (facet + ["--frames", "1", "0", "--output", "o%d.pfm"], "beyond"),
             (facet + ["--frames", "0", "1", "--output", "o.pfm"], "--output"),
             (["--facet", "a0.pfm", "spherical", "360", "0", "0", "0", "--frames", "0", "1", "--output", "o%d.pfm"], "no conversion"),
             (facet + ["--frames", "0", "1", "--output", "o%d.pfm", "--ycbcr_matrix", "240"], "--ycbcr_matrix"),
             (facet + ["--frames", "0", "1", "--output", "o%d.pfm", "--ycbcr_range", "wide"], "--ycbcr_range")]
    for argv, word in cases:
        r = cli(argv + common, tmp_path)
        assert r.returncode == 2 and word in r.stderr and "HIP device" not in r.stderr, (argv, r.stderr)
    r = cli(facet + ["--output", "o%d.pfm"] + common + ["--frames", "0"], tmp_path)
    assert r.returncode == 2 and "--frames needs 2" in r.stderr, r.stderr
    # pipe mode: the fixed options, then one job per line
    r = cli(common + ["-"], tmp_path, stdin=" ".join(facet + ["--frames", "0", "1", "--output", "o%d.pfm"]) + "\n")
    assert r.returncode == 2 and "pipe mode" in r.stderr, r.stderr
    # a .y4m facet is probed through its header: a refused tag is a message
    (tmp_path / "m.y4m").write_bytes(y4m_bytes(4, 4, "Cmono", [bytes(16)]))
    r = cli(["--facet", "m.y4m", "spherical", "360", "0", "0", "0", "--output", "o.pfm"] + common, tmp_path)
    assert r.returncode == 2 and "failed to open" in r.stderr, r.stderr
