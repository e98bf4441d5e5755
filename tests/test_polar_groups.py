"""The grouping of eu_render5_kernel's second loop (envutil_amd/csrc/eu_polar_groups.h) is plain C++: a host
program builds the stepper tables of cubemap targets with eu::build_stepper_tables and checks the lists of
positions - a face of 64 gives positions of four (a tile, its mirror, its twin on the opposite polar face, the
twin's mirror), faces of 96, 80 and 48 twins only, faces of 41 and 33, a rotated target and bands entries of one,
row ranges what lies inside them, one flipped bit removes exactly the members it touches, and every second-loop
tile appears in exactly one position."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "envutil_amd", "build", "polar_groups_demo")


def build_demo():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "csrc", "polar_groups_demo.cc"), "-o", EXE])
    return EXE


def test_polar_groups_host_program():
    r = subprocess.run([build_demo()], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAILED" not in r.stdout and "all ok" in r.stdout


def test_follower_count_query():
    exe = build_demo()
    out = subprocess.run([exe, "64", "0", "0", "384", "b"], capture_output=True, text=True, check=True).stdout
    assert out.split() == ["followers", "48"]
    out = subprocess.run([exe, "64", "30", "0", "384", "b"], capture_output=True, text=True, check=True).stdout
    assert out.split() == ["followers", "0"]
