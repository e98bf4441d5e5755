"""--synopsis feather and --feather WIDTH above the kernels, without a GPU: the front end's options and refusals and
the PTO route (tests/csrc/feather_demo.cc over include/eu_frontend.hpp and eu_dispatch.hpp), envutil_amd.arguments, and
the C ABI's refusals, which come before a device is looked for."""
import ctypes as C
import json
import math
import os
import subprocess

import pytest

import envutil_amd as ea

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "envutil_amd", "build", "feather_demo")
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
                           os.path.join(ROOT, "tests", "csrc", "feather_demo.cc"), "-o", EXE,
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
    assert j["ok"] and j["synopsis"] == "panorama" and j["feather"] == 0.0
    j, _ = demo(FACETS + ["--synopsis", "feather"])
    assert j["ok"] and j["synopsis"] == "feather" and j["feather"] == 0.0 and j["nfacets"] == 2
    j, _ = demo(FACETS + ["--synopsis", "feather", "--feather", "12.25"])
    assert j["ok"] and j["feather"] == 12.25


def test_refusals(demo):
    for argv, word in ((["--synopsis", "feather", "--feather", "-3"], "--feather -3"),
                       (["--synopsis", "feather", "--feather", "nan"], "--feather"),
                       (["--synopsis", "feather", "--feather", "x"], "--feather"),
                       (["--feather", "5"], "--synopsis feather"),
                       (["--synopsis", "panorama", "--feather", "5"], "--synopsis feather"),
                       (["--synopsis", "hdr_merge", "--feather", "0"], "--synopsis feather")):
        j, _ = demo(FACETS + argv)
        assert not j["ok"] and word in j["error"], (argv, j)


def test_pto_route(demo, tmp_path):
    (tmp_path / "two.pto").write_text(PTO)
    j, tail = demo(["--pto", "two.pto", "--output", "o.tif", "--twine", "0", "--synopsis", "feather", "--feather", "8"],
                   cwd=str(tmp_path), payload=True)
    assert j["ok"] and j["synopsis"] == "feather" and j["feather"] == 8.0 and j["nfacets"] == 2
    assert (j["projection"], j["width"], j["height"]) == (ea.SPHERICAL, 300, 150)
    # the dispatch takes the synopsis: without a device the job ends where the first facet is loaded
    # (rc 0 where a device shows in spite of HIP_VISIBLE_DEVICES)
    assert tail in (["rc -1"], ["rc 0"]), tail
    j, tail = demo(["--pto", "two.pto", "--output", "o.tif", "--twine", "0", "--synopsis", "median"], cwd=str(tmp_path), payload=True)
    assert j["ok"] and tail == ["rc -2"], tail


def test_selftest_program(demo):
    """the stand-alone program: its own command lines, payload(), and the three entry points' refusals"""
    r = subprocess.run([EXE, "selftest"], capture_output=True, text=True, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"), timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "all ok" in r.stdout and "FAILED" not in r.stdout, r.stdout + r.stderr
    assert r.stdout.count("ok: ") >= 13 + 3 * 8 + 3 * 3


def test_python_arguments():
    a = ea.arguments(ea.SPHERICAL, 96, 48, 360.0, synopsis="feather")
    assert a.synopsis == "feather" and a.feather == 0.0
    t = a.target(3)
    assert t.synopsis == ea.api.SYN_FEATHER == 2 and t.feather == 0.0
    t = ea.arguments(ea.SPHERICAL, 96, 48, 360.0, synopsis="feather", feather=6.5).target(4)
    assert t.feather == 6.5 and t.synopsis == 2
    assert ea.arguments(ea.SPHERICAL, 96, 48, 360.0).target(3).feather == 0.0
    for bad in (-1.0, math.nan, math.inf, -math.inf):
        with pytest.raises(ValueError, match="feather"):
            ea.arguments(ea.SPHERICAL, 96, 48, 360.0, synopsis="feather", feather=bad)
    with pytest.raises(ValueError, match="synopsis"):
        ea.arguments(ea.SPHERICAL, 96, 48, 360.0, synopsis="median")
    # the mirror: `feather` is the last field, a double behind the `single` pointer
    assert ea.api.Target._fields_[-1] == ("feather", C.c_double)
    assert ea.api.Target.feather.offset == ea.api.Target.single.offset + C.sizeof(C.c_void_p)
    assert C.sizeof(ea.api.Target) == ea.api.Target.feather.offset + 8
