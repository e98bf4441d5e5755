"""--feather_edges in the front end (include/eu_frontend.hpp), without a device, through tests/csrc/edges_demo.cc: the
option is parsed, refused without one of the two blending synopses, and reaches facet_spec::edges only for facets that
end up with an alpha channel - their own, or gained from a PTO mask or a lens crop."""
import os
import subprocess

import pytest

import envutil_amd as ea
import pto_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "envutil_amd", "build", "edges_demo")
TARGET = ["--projection", "spherical", "--hfov", "120", "--width", "96", "--height", "48", "--output", "o.pfm"]
IMAGES = {"rgba.pam": (40, 30, 4), "rgb.ppm": (40, 30, 3), "ga.pam": (40, 30, 2), "cube.pam": (16, 96, 4),
          "with blank in name.tif": (400, 300, 3), "b.tif": (400, 300, 3)}


@pytest.fixture(scope="module")
def demo():
    if not os.path.exists(ea.lib_path()):
        ea.build()
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "csrc", "edges_demo.cc"), "-o", EXE,
                           "-L" + os.path.join(ROOT, "envutil_amd", "lib"), "-leu_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "envutil_amd", "lib")])

    def run(*argv, cwd=None):
        env = dict(os.environ, EU_TEST_IMAGES=";".join(f"{k}={w}x{h}x{c}" for k, (w, h, c) in IMAGES.items()))
        r = subprocess.run([EXE] + [str(a) for a in argv], capture_output=True, text=True, env=env, cwd=cwd, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout.strip()
    return run


def facets(line):
    """{filename: (nchannels, edges, asset key)} of an "ok" line"""
    assert line.startswith("ok "), line
    out = {}
    for part in line.split(" | ")[1:]:
        name, rest = part.split(" nchannels ")
        nch, rest = rest.split(" edges ")
        edges, key = rest.split(" key ")
        out[name] = (int(nch), int(edges), key)
    return out


def facet(name, yaw, prj="rectilinear", hfov=50):
    return ["--facet", name, prj, hfov, yaw, 0, 0]


def test_selftest(demo):
    out = demo("selftest")
    assert out.endswith("all ok"), out


def test_parsed_and_only_for_facets_with_alpha(demo):
    base = ["parse"] + facet("rgba.pam", -10) + facet("rgb.ppm", 12) + facet("ga.pam", 30) + TARGET
    for syn in ("feather", "multiband"):
        line = demo(*base, "--synopsis", syn, "--feather_edges")
        assert line.startswith("ok feather_edges 1"), line
        f = facets(line)
        assert f["rgba.pam"][:2] == (4, 1) and f["rgb.ppm"][:2] == (3, 0) and f["ga.pam"][:2] == (2, 1), line
        assert f["rgba.pam"][2] != "rgba.pam" and f["rgb.ppm"][2] == "rgb.ppm"
    line = demo(*base, "--synopsis", "feather")
    assert line.startswith("ok feather_edges 0") and all(v[1] == 0 for v in facets(line).values()), line
    assert facets(line)["rgba.pam"][2] == "rgba.pam"


def test_refused_without_a_blending_synopsis(demo):
    base = ["parse"] + facet("rgba.pam", -10) + facet("rgb.ppm", 12) + TARGET
    for extra in (["--synopsis", "panorama"], ["--synopsis", "hdr_merge"], []):
        line = demo(*base, *extra, "--feather_edges")
        assert line.startswith("refused: --feather_edges goes with --synopsis feather or multiband"), line


def test_a_cubemap_keeps_no_plane(demo):
    line = demo("parse", *facet("cube.pam", 0, "cubemap", 90), *facet("rgba.pam", 12), *TARGET, "--synopsis", "feather", "--feather_edges")
    f = facets(line)
    assert f["cube.pam"][:2] == (4, 0) and f["rgba.pam"][:2] == (4, 1), line


def test_facets_that_gain_alpha_from_a_mask_or_a_crop(demo, tmp_path):
    (tmp_path / "m.pto").write_text(pto_cases.CASES["masks_and_crops"])
    line = demo("parse", "--pto", "m.pto", "--output", "o.pfm", "--synopsis", "feather", "--feather_edges", cwd=str(tmp_path))
    f = facets(line)
    # both images are RGB files; a lens crop and exclude masks give each an alpha channel, and with it a plane
    assert f["with blank in name.tif"][:2] == (4, 1) and f["b.tif"][:2] == (4, 1), line
    plain = facets(demo("parse", "--pto", "m.pto", "--output", "o.pfm", "--synopsis", "feather", cwd=str(tmp_path)))
    assert all(v[1] == 0 for v in plain.values())
    assert all(f[k][2] == plain[k][2] + " +edges" for k in f)
