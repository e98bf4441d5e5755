"""Frame sequences on the command line (envutil_hip --frames FIRST LAST): one resident source, the first frame loaded,
every later one refilled in place through the feed its file type takes. A numbered sequence writes, byte for byte, the
files that one run per frame writes without --frames; a Y4M run over A..B writes, for every k, the file of a run with
--frames k k; and a Y4M frame renders as the float picture the numpy model of the Y'CbCr feed makes of its planes."""
import numpy as np
import pytest

import ycbcr_model as ym
from test_cli import cli, write_pfm, synth  # noqa: F401  (cli: the fixture)
from test_frames_host import y4m_bytes

pytestmark = pytest.mark.gpu

W, H = 96, 48
FACET = ["spherical", "360", "10", "5", "0"]
TARGET = ["--projection", "rectilinear", "--hfov", "80", "--width", "64", "--height", "40", "--degree", "3"]


def write_ppm(path, img8):
    h, w = img8.shape[:2]
    path.write_bytes(b"P6\n%d %d\n255\n" % (w, h) + np.ascontiguousarray(img8, np.uint8).tobytes())


def write_hdr(path, quads):
    h, w = quads.shape[:2]
    q = quads.copy()
    q[:, 0, 0] = 100                       # a flat scanline must not begin like a run-length encoded one
    path.write_bytes(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n" % (h, w) + q.tobytes())


def frame_image(kind, k):
    rng = np.random.default_rng(100 + k)
    if kind == "pfm":
        return synth(W, H, 3, seed=k)
    if kind == "ppm":
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    q = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    q[..., 3] = 124 + q[..., 3] % 8
    return q


WRITE = {"pfm": write_pfm, "ppm": write_ppm, "hdr": write_hdr}


@pytest.mark.parametrize("kind,out_ext", [("pfm", "ppm"), ("ppm", "pfm"), ("hdr", "hdr"), ("ppm", "ppm")])
def test_numbered_sequence_writes_the_files_of_one_run_per_frame(cli, tmp_path, kind, out_ext):
    first, last = 3, 6
    for k in range(first, last + 1):
        WRITE[kind](tmp_path / f"in_{k:03d}.{kind}", frame_image(kind, k))
    r = cli(["--facet", f"in_%03d.{kind}"] + FACET + TARGET + ["--frames", str(first), str(last), "--output", f"seq_%d.{out_ext}", "-v"], tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("loaded as a new source") == 1 and r.stdout.count("eu_hip_source_reload") == last - first, r.stdout
    for k in range(first, last + 1):
        r = cli(["--facet", f"in_{k:03d}.{kind}"] + FACET + TARGET + ["--output", f"one_{k}.{out_ext}"], tmp_path)
        assert r.returncode == 0, r.stderr
        a, b = (tmp_path / f"seq_{k}.{out_ext}").read_bytes(), (tmp_path / f"one_{k}.{out_ext}").read_bytes()
        assert a == b, f"frame {k}: the sequence's file differs from the single run's"
    assert (tmp_path / f"seq_{first}.{out_ext}").read_bytes() != (tmp_path / f"seq_{last}.{out_ext}").read_bytes()


def y4m_frames(rng, n, sub_x, sub_y, bits, depth):
    planes, raw = [], []
    for _ in range(n):
        y, cb, cr = ym.planes(rng, H, W, sub_x, sub_y, bits, "planar")
        if bits == 16:
            y, cb, cr = (a >> (16 - depth) for a in (y, cb, cr))          # the code in the low bits
        planes.append((y, cb, cr))
        raw.append(b"".join(np.ascontiguousarray(a, "<u2" if bits == 16 else np.uint8).tobytes() for a in (y, cb, cr)))
    return planes, raw


@pytest.mark.parametrize("tag,sub,bits,depth,extra", [("C420jpeg", (2, 2), 8, 8, []), ("C422", (2, 1), 8, 8, ["--ycbcr_matrix", "2020"]),
                                                      ("C444p10 XCOLORRANGE=FULL", (1, 1), 16, 10, []),
                                                      ("C420p12", (2, 2), 16, 12, ["--ycbcr_range", "full", "--ycbcr_matrix", "709"])])
def test_y4m_sequence(cli, tmp_path, tag, sub, bits, depth, extra):
    import envutil_amd as ea
    rng = np.random.default_rng(bits + depth)
    planes, raw = y4m_frames(rng, 4, sub[0], sub[1], bits, depth)
    (tmp_path / "clip.y4m").write_bytes(y4m_bytes(W, H, tag, raw))
    facet = ["--facet", "clip.y4m"] + FACET
    r = cli(facet + TARGET + extra + ["--frames", "1", "3", "--output", "seq_%02d.pfm", "-v"], tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("eu_hip_source_reload") == 2 and "YCbCr planes, decoded on the device" in r.stdout, r.stdout
    for k in (1, 2, 3):
        r = cli(facet + TARGET + extra + ["--frames", str(k), str(k), "--output", "one_%02d.pfm"], tmp_path)
        assert r.returncode == 0, r.stderr
        assert (tmp_path / f"seq_{k:02d}.pfm").read_bytes() == (tmp_path / f"one_{k:02d}.pfm").read_bytes(), f"frame {k}"
    # without --frames the facet is its frame 0
    assert cli(facet + TARGET + extra + ["--output", "plain.pfm"], tmp_path).returncode == 0
    assert cli(facet + TARGET + extra + ["--frames", "0", "0", "--output", "zero_%d.pfm"], tmp_path).returncode == 0
    assert (tmp_path / "plain.pfm").read_bytes() == (tmp_path / "zero_0.pfm").read_bytes()
    # ... and a frame is the float picture the model makes of its planes: tables and matrix as the options say
    full = "FULL" in tag or "full" in extra
    matrix = extra[extra.index("--ycbcr_matrix") + 1] if "--ycbcr_matrix" in extra else "601"      # 48 rows: below 720
    yt, ct = ea.ycbcr_tables(bits, depth, full_range=full)
    y, cb, cr = planes[2]
    write_pfm(tmp_path / "model.pfm", ym.floats(y, cb, cr, sub[0], sub[1], yt, ct, ea.ycbcr_matrix(matrix)))
    assert cli(["--facet", "model.pfm"] + FACET + TARGET + ["--output", "model_out.pfm"], tmp_path).returncode == 0
    assert (tmp_path / "seq_02.pfm").read_bytes() == (tmp_path / "model_out.pfm").read_bytes()


def test_a_frame_of_another_size_or_type_stops_the_run_with_its_number(cli, tmp_path):
    for k in range(2):
        write_pfm(tmp_path / f"a{k}.pfm", synth(W, H, 3, seed=k))
    write_pfm(tmp_path / "a2.pfm", synth(W + 2, H, 3))
    r = cli(["--facet", "a%d.pfm"] + FACET + TARGET + ["--frames", "0", "2", "--output", "o%d.pfm"], tmp_path)
    assert r.returncode == 2 and "frame 2" in r.stderr and "a2.pfm" in r.stderr, r.stderr
    assert (tmp_path / "o1.pfm").exists() and not (tmp_path / "o2.pfm").exists()
    write_pfm(tmp_path / "a2.pfm", synth(W, H, 1)[..., 0])
    r = cli(["--facet", "a%d.pfm"] + FACET + TARGET + ["--frames", "0", "2", "--output", "p%d.pfm"], tmp_path)
    assert r.returncode == 2 and "frame 2" in r.stderr, r.stderr
    (tmp_path / "clip.y4m").write_bytes(y4m_bytes(W, H, "C444", [bytes(3 * W * H), bytes(3 * W * H - 5)]))
    r = cli(["--facet", "clip.y4m"] + FACET + TARGET + ["--frames", "0", "1", "--output", "q%d.pfm"], tmp_path)
    assert r.returncode == 2 and "frame 1" in r.stderr and "truncated" in r.stderr, r.stderr
