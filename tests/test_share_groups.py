"""The grouping of eu_render5_kernel's first loop (envutil_amd/csrc/eu_share_groups.h) is plain C++:
a host program feeds it synthetic row and column tables and checks the group lists - identical
tables give groups of 8, one flipped bit in A1 or in sqrt(rx^2 + rz^2) removes exactly that member,
an odd tile count or a ragged width removes the mirrors, a row range removes the cut members, and
every tile appears in exactly one group."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "envutil_amd", "build", "share_groups_demo")


def test_share_groups_host_program():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "csrc", "share_groups_demo.cc"), "-o", EXE])
    r = subprocess.run([EXE], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAILED" not in r.stdout and "all ok" in r.stdout
