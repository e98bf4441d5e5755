"""--synopsis multiband and --bands N above the kernels, without a GPU: the front end's options and refusals and the
PTO route (tests/csrc/multiband_demo.cc over include/eu_frontend.hpp and eu_dispatch.hpp), and the C ABI's refusals,
which come before a device is looked for."""
import json
import os
import subprocess

import pytest

import envutil_amd as ea

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "envutil_amd", "build", "multiband_demo")
IMAGES = {"a.tif": (200, 150, 3), "b.tif": (200, 150, 3)}
PTO = ('p f2 w300 h150 v360 n"TIFF"\n'
       'i w200 h150 f0 v70 y-20 p0 r0 n"a.tif"\n'
       'i w200 h150 f0 v70 y25 p3 r1 n"b.tif"\n')


@pytest.fixture(scope="module")
def demo():
    if not os.path.exists(ea.lib_path()):
        ea.build()
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "csrc", "multiband_demo.cc"), "-o", EXE,
                           "-L" + os.path.join(ROOT, "envutil_amd", "lib"), "-leu_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "envutil_amd", "lib")])

    def run(argv, cwd=None, payload=False):
        env = dict(os.environ, EU_TEST_IMAGES=";".join(f"{k}={w}x{h}x{c}" for k, (w, h, c) in IMAGES.items()),
                   HIP_VISIBLE_DEVICES="-1")
        if payload:
            env["EU_TEST_PAYLOAD"] = "1"
        r = subprocess.run([EXE] + list(argv), capture_output=True, text=True, env=env, cwd=cwd, timeout=300)
        assert r.stdout, r.stderr
        lines = r.stdout.splitlines()
        return json.loads(lines[0]), lines[1:]
    return run


FACETS = ["--facet", "a.tif", "rectilinear", "70", "-20", "0", "0", "--facet", "b.tif", "rectilinear", "70", "25", "3", "1",
          "--output", "o.tif"]


def test_options(demo):
    j, _ = demo(FACETS)
    assert j["ok"] and j["synopsis"] == "panorama" and j["bands"] == 0
    j, _ = demo(FACETS + ["--synopsis", "multiband"])
    assert j["ok"] and j["synopsis"] == "multiband" and j["bands"] == 0 and j["feather"] == 0.0 and j["nfacets"] == 2
    j, _ = demo(FACETS + ["--synopsis", "multiband", "--bands", "4", "--feather", "12.25"])
    assert j["ok"] and j["bands"] == 4 and j["feather"] == 12.25


def test_refusals(demo):
    for argv, word in ((["--synopsis", "multiband", "--bands", "-3"], "--bands -3"),
                       (["--synopsis", "multiband", "--bands", "x"], "--bands"),
                       (["--bands", "5"], "--bands goes with --synopsis multiband"),
                       (["--synopsis", "feather", "--bands", "5"], "--bands goes with --synopsis multiband"),
                       (["--synopsis", "panorama", "--bands", "0"], "--bands goes with --synopsis multiband"),
                       # the existing refusals keep their wording
                       (["--synopsis", "panorama", "--feather", "5"], "--feather goes with --synopsis feather"),
                       (["--synopsis", "multiband", "--feather", "-3"], "--feather -3"),
                       (["--synopsis", "multiband", "--twine", "2"], "--synopsis multiband blends whole frames"),
                       (["--synopsis", "multiband", "--twf_file", "t.twf"], "no --twf_file")):
        j, _ = demo(FACETS + argv)
        assert not j["ok"] and word in j["error"], (argv, j)


def test_pto_route(demo, tmp_path):
    (tmp_path / "two.pto").write_text(PTO)
    j, tail = demo(["--pto", "two.pto", "--output", "o.tif", "--twine", "0", "--synopsis", "multiband", "--bands", "3"],
                   cwd=str(tmp_path), payload=True)
    assert j["ok"] and j["synopsis"] == "multiband" and j["bands"] == 3 and j["nfacets"] == 2
    assert (j["projection"], j["width"], j["height"]) == (ea.SPHERICAL, 300, 150)
    # the dispatch takes the synopsis: without a device the job ends where the first facet is loaded
    # (rc 0 where a device shows in spite of HIP_VISIBLE_DEVICES)
    assert tail in (["rc -1"], ["rc 0"]), tail


def test_no_twining_by_default(demo, tmp_path):
    """the command line's default is automatic twining (--twine -1); a multiband job of several facets gets none,
    where the same facets feathered do"""
    (tmp_path / "two.pto").write_text(PTO)
    j, _ = demo(["--pto", "two.pto", "--output", "o.tif", "--synopsis", "multiband"], cwd=str(tmp_path))
    assert j["ok"] and j["twine"] == 0, j
    j, _ = demo(["--pto", "two.pto", "--output", "o.tif", "--synopsis", "feather"], cwd=str(tmp_path))
    assert j["ok"] and j["twine"] > 1, j
    j, _ = demo(FACETS + ["--synopsis", "multiband"])
    assert j["ok"] and j["twine"] == 0, j
    j, _ = demo(FACETS + ["--synopsis", "multiband", "--solo", "0"])
    assert j["ok"] and j["twine"] > 1, j


def test_selftest_program(demo):
    """the stand-alone program: its own command lines, the levels, the scratch bytes, and the entry points' refusals"""
    r = subprocess.run([EXE, "selftest"], capture_output=True, text=True, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"), timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "all ok" in r.stdout and "FAILED" not in r.stdout, r.stdout + r.stderr
    assert r.stdout.count("ok: ") >= 18 + 14 + 4 + 7 * 3 + 5 + 10


def test_usage_names_the_options():
    exe = os.path.join(ROOT, "envutil_amd", "bin", "envutil_hip")
    if not os.path.exists(exe):
        ea.build()
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"), timeout=60)
    text = r.stdout + r.stderr
    assert "panorama|hdr_merge|feather|multiband" in text and "--bands N" in text, text
