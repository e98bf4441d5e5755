"""--feather_edges on the command line (envutil_hip): a two-facet PTO project with a lens crop on a fisheye image and
an exclude mask (k-line) on the other, under --synopsis feather and multiband - the files are, byte for byte, the
binding's frames with edges=True; -v names the planes; a run without the option writes the bytes of the binding's
unflagged job; and a --frames run over a numbered PAM series with alpha matches one run per frame."""
import numpy as np
import pytest

import envutil_amd as ea
from test_cli import cli, write_pfm, read_pfm, synth, bits  # noqa: F401  (cli: the fixture)

pytestmark = pytest.mark.gpu

PTO = ('p f2 w160 h80 v360 n"TIFF"\n'
       'i w64 h48 f0 v70 y10 p5 r2 n"a.pfm"\n'
       'i w56 h56 f3 v120 y-35 p-4 r0 S4,52,4,52 n"b.pfm"\n'
       'k i0 t0 p"5 6 30 8 34 40 8 36"\n')
POLY = [(np.array([5, 30, 34, 8], np.float32), np.array([6, 8, 40, 36], np.float32))]


def project(tmp_path):
    a, b = synth(64, 48, 3, 1), synth(56, 56, 3, 2)
    write_pfm(tmp_path / "a.pfm", a)
    write_pfm(tmp_path / "b.pfm", b)
    (tmp_path / "two.pto").write_text(PTO)
    fa = ea.facet_spec(ea.RECTILINEAR, 64, 48, 70.0, nchannels=4, yaw=10, pitch=5, roll=2)
    fb = ea.facet_spec(ea.FISHEYE, 56, 56, 120.0, nchannels=4, yaw=-35, pitch=-4, roll=0)

    def sources(edges):
        return [ea.Source.load(fa, a, 1, masks=POLY, edges=edges),
                ea.Source.load(fb, b, 1, crop=(4, 52, 4, 52), crop_kind=2, edges=edges)]
    return sources


@pytest.mark.parametrize("synopsis", ["feather", "multiband"])
def test_pto_project_with_a_crop_and_a_mask(cli, tmp_path, synopsis):
    sources = project(tmp_path)
    argv = ["--pto", "two.pto", "--degree", "1", "--twine", "0", "--synopsis", synopsis, "--feather", "6"]
    a = ea.arguments(ea.SPHERICAL, 160, 80, 360.0, spline_degree=1, synopsis=synopsis, feather=6.0)
    frames = {}
    for flag in (True, False):
        r = cli(argv + (["--feather_edges"] if flag else []) + ["--output", "o.pfm", "-v"], tmp_path)
        assert r.returncode == 0, r.stdout + r.stderr
        assert (r.stdout.count("a distance plane of its alpha channel") == 2) == flag, r.stdout
        if flag:
            assert "a.pfm: a distance plane" in r.stdout and "b.pfm: a distance plane" in r.stdout and "56 x 56" in r.stdout
        got = read_pfm(tmp_path / "o.pfm")
        want = ea.render(a, sources(flag), 4)
        assert got.shape == want.shape == (80, 160, 4)
        assert (bits(got) == bits(want)).all(), f"{synopsis}, --feather_edges {flag}: the file is not the binding's frame"
        frames[flag] = got
    assert (bits(frames[True]) != bits(frames[False])).any() and (frames[True][..., 3] > 0).mean() > 0.02


def test_refused_under_another_synopsis(cli, tmp_path):
    project(tmp_path)
    r = cli(["--pto", "two.pto", "--degree", "1", "--feather_edges", "--output", "o.pfm"], tmp_path)
    assert r.returncode == 2 and "--feather_edges goes with" in r.stderr, r.stderr


def write_pam(path, img8):
    h, w, n = img8.shape
    path.write_bytes(b"P7\nWIDTH %d\nHEIGHT %d\nDEPTH 4\nMAXVAL 255\nTUPLTYPE RGB_ALPHA\nENDHDR\n" % (w, h) +
                     np.ascontiguousarray(img8, np.uint8).tobytes())


def test_frames_over_a_pam_series_with_alpha(cli, tmp_path):
    w, h = 64, 40
    for k in range(3):
        rng = np.random.default_rng(k)
        img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        yy, xx = np.mgrid[0:h, 0:w]
        img[..., 3] = np.where((xx - 20 - 9 * k) ** 2 + (yy - 20) ** 2 < 150, 0, 255)      # a hole that moves
        write_pam(tmp_path / f"in_{k}.pam", img)
    facet = ["rectilinear", "60", "5", "2", "0"]
    target = ["--projection", "rectilinear", "--hfov", "50", "--width", "48", "--height", "32", "--degree", "1", "--twine", "0",
              "--synopsis", "feather", "--feather_edges"]
    r = cli(["--facet", "in_%d.pam"] + facet + target + ["--frames", "0", "2", "--output", "seq_%d.pfm", "-v"], tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("eu_hip_source_reload") == 2 and r.stdout.count("a distance plane of its alpha channel") == 3, r.stdout
    for k in range(3):
        r = cli(["--facet", f"in_{k}.pam"] + facet + target + ["--output", f"one_{k}.pfm"], tmp_path)
        assert r.returncode == 0, r.stderr
        assert (tmp_path / f"seq_{k}.pfm").read_bytes() == (tmp_path / f"one_{k}.pfm").read_bytes(), f"frame {k}"
