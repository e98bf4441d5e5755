"""The choice of the render kernel (envutil_amd/csrc/eu_select.h) is plain C++: a host program builds
eu_render_params by hand - BASELINE's jobs and the cases each kernel refuses - and checks the chosen path
under the default switches and under each switch value, the two staged profiles, the post-plan test, the
run splitter of the packed kernel's hybrid on hand-made segment flags, and how eu_read_switches() parses
the EU_HIP_* variables."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "envutil_amd", "build", "select_demo")


def test_select_host_program():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "csrc", "select_demo.cc"), "-o", EXE])
    env = {k: v for k, v in os.environ.items() if not k.startswith("EU_HIP_")}
    r = subprocess.run([EXE], capture_output=True, text=True, env=env)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAILED" not in r.stdout and "all ok" in r.stdout
    # degrees 0 and 4 to 9 under every EU_HIP_R4 / HYBRID / KERNEL / DIRECT combination: never packed, never staged
    assert "ok: high degrees: 16128 combinations, all general" in r.stdout
