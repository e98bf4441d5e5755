"""envutil_hip --layer IMAGE OUTPUT: further pictures of the single facet's geometry, rendered with the facet's
picture in one eu_hip_render_layers call. The files must be byte for byte what separate runs write; what the call
does not render is refused with a message (exit status 2, before any image is loaded)."""
import os
import subprocess

import numpy as np
import pytest

import envutil_amd as ea
from test_cli import EXE, rle_scanline, synth, write_pfm


@pytest.fixture(scope="module")
def cli():
    if not os.path.exists(EXE) or not os.path.exists(ea.lib_path()):
        ea.build()

    def run(argv, cwd, stdin=None, devices=None):
        env = dict(os.environ, EU_HIP_DEVICES=devices) if devices else None
        return subprocess.run([EXE] + list(argv), capture_output=True, text=True, cwd=str(cwd), input=stdin, timeout=600,
                              env=env)
    return run


FACET = ["spherical", "360", "0", "0", "0"]
JOB = ["--projection", "cubemap", "--hfov", "90", "--width", "16", "--degree", "3", "--twine", "0"]


def pictures(tmp_path):
    w, h = 64, 32
    write_pfm(tmp_path / "a.pfm", synth(w, h, 3, 1))
    write_pfm(tmp_path / "b.pfm", synth(w, h, 3, 2))
    rng = np.random.default_rng(12)
    q = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    q[..., 3] = rng.integers(120, 136, (h, w))
    head = b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n" % (h, w)
    (tmp_path / "c.hdr").write_bytes(head + b"".join(rle_scanline(q[y]) for y in range(h)))


@pytest.mark.gpu
@pytest.mark.parametrize("twine", ["0", "2"])
def test_layers_write_the_files_of_separate_runs(cli, tmp_path, twine):
    pictures(tmp_path)
    job = JOB[:-1] + [twine]
    r = cli(["--facet", "a.pfm"] + FACET + job + ["--output", "oa.pfm", "--layer", "b.pfm", "ob.pfm",
             "--layer", "c.hdr", "oc.pfm", "-v"], tmp_path, devices="1")
    assert r.returncode == 0, r.stderr
    assert "eu_hip_render_layers" in r.stdout and "3 pictures" in r.stdout
    assert "c.hdr: RGBE pixels, decoded on the device" in r.stdout
    for src, one, name in (("a.pfm", "oa.pfm", "sa.pfm"), ("b.pfm", "ob.pfm", "sb.pfm"), ("c.hdr", "oc.pfm", "sc.pfm")):
        r = cli(["--facet", src] + FACET + job + ["--output", name], tmp_path, devices="1")
        assert r.returncode == 0, r.stderr
        assert (tmp_path / one).read_bytes() == (tmp_path / name).read_bytes(), f"{one} differs from a run of its own"
    assert (tmp_path / "oa.pfm").read_bytes() != (tmp_path / "ob.pfm").read_bytes()
    assert (tmp_path / "oa.pfm").read_bytes() != (tmp_path / "oc.pfm").read_bytes()


def test_what_layers_do_not_go_with_is_refused(cli, tmp_path):
    """argument errors of the front end: exit status 2 and a message, no device needed"""
    pictures(tmp_path)
    write_pfm(tmp_path / "small.pfm", synth(32, 16, 3, 3))
    write_pfm(tmp_path / "rgba.pfm", synth(64, 32, 4, 4))
    write_pfm(tmp_path / "rays.pfm", synth(8, 4, 3, 5))
    (tmp_path / "two.pto").write_text('p f2 w64 h32 v360\ni w64 h32 f4 v360 y0 p0 r0 n"a.pfm"\ni w64 h32 f4 v360 y90 p0 r0 n"b.pfm"\n')
    one = ["--facet", "a.pfm"] + FACET
    layer = ["--layer", "b.pfm", "ob.pfm"]
    cases = [
        (one + ["--facet", "b.pfm"] + FACET + JOB + ["--output", "o.pfm"] + layer, "ONE facet's geometry: 2 facets"),
        (["--pto", "two.pto", "--output", "o.pfm"] + layer, "ONE facet's geometry: 2 facets"),
        (one + JOB + ["--split", "s%d.pfm"] + layer, "--single / --split"),
        (one + JOB + ["--output", "o.pfm", "--single", "0"] + layer, "--single / --split"),
        (one + ["--degree", "1", "--output", "o.pfm", "--ray_map", "rays.pfm"] + layer, "--ray_map"),
        (one + JOB + ["--output", "o.pfm", "--layer", "small.pfm", "os.pfm"], "small.pfm is 32 x 16, the facet 64 x 32"),
        (one + JOB + ["--output", "o.pfm", "--layer", "rgba.pfm", "or.pfm"], "rgba.pfm has 4 channels, the facet 3"),
        (one + JOB + ["--output", "o.pfm", "--layer", "nope.pfm", "on.pfm"], "failed to open layer image"),
        (one + JOB + ["--output", "o.pfm", "--layer", "b.pfm"], "--layer needs 2 value"),
    ]
    for argv, message in cases:
        r = cli(argv, tmp_path)
        assert r.returncode == 2 and message in r.stderr, (argv, r.returncode, r.stderr)
        assert not (tmp_path / "ob.pfm").exists()
    # pipe mode: the fixed options or the job's line may carry the layer
    r = cli(one + JOB + layer + ["-"], tmp_path, stdin="--output o.pfm\n")
    assert r.returncode == 2 and "pipe mode" in r.stderr, r.stderr
    r = cli(one + JOB + ["-"], tmp_path, stdin="--output o.pfm --layer b.pfm ob.pfm\n")
    assert r.returncode == 2 and "pipe mode" in r.stderr, r.stderr
    assert not (tmp_path / "ob.pfm").exists() and not (tmp_path / "o.pfm").exists()


@pytest.mark.gpu
def test_several_devices_are_refused_or_one_renders(cli, tmp_path):
    """on a host with one visible device the job renders; with several it is refused by name"""
    pictures(tmp_path)
    r = cli(["--facet", "a.pfm"] + FACET + JOB + ["--output", "oa.pfm", "--layer", "b.pfm", "ob.pfm"], tmp_path)
    if ea.device_count() > 1:
        assert r.returncode == 2 and "one device" in r.stderr, r.stderr
    else:
        assert r.returncode == 0, r.stderr
