"""What eu_hip_render_rays does without a device: every argument error is reported as EU_ERR_ARGUMENT with a
message before a device is looked for, a valid call then ends in EU_ERR_NO_DEVICE; the choice between the two
kernel forms (eu_select_ray_path) and the miss predicate (eu_ray_guard.h) are plain C++ and are checked through
a host program."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import envutil_amd as ea

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "envutil_amd", "build", "select_rays_demo")
OK, NO_DEVICE, ARGUMENT, HANDLE = 0, -1, -2, -5


def build_demo():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "csrc", "select_rays_demo.cc"), "-o", EXE])
    return EXE


def test_select_ray_path_and_miss_predicate_host_program():
    """one job per reason for the general form plus the packed cases; the predicate over all exponent classes
    (zero, denormal, normal, inf, quiet and signalling NaN, both signs) in each of the three components of a
    ray and each of the nine of a ninepack"""
    build_demo()
    env = {k: v for k, v in os.environ.items() if not k.startswith("EU_HIP_")}
    r = subprocess.run([EXE], capture_output=True, text=True, env=env)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAILED" not in r.stdout and "all ok" in r.stdout
    assert r.stdout.count("-> packed") >= 72 and r.stdout.count("-> general") >= 12
    # degrees 0 and 4 to 9 under every EU_HIP_R4 / HYBRID / KERNEL / DIRECT combination: never packed
    assert "ok: high degrees: 8064 combinations, all general" in r.stdout


# The calls below run in a child process that is asked not to see a device (HIP_VISIBLE_DEVICES=-1), so that
# they mean the same on a machine with a GPU: argument errors first, then EU_ERR_NO_DEVICE. The source handle
# comes from eu_hip_diag_host_source, which needs no device and has no container.
CHILD = r'''
import ctypes as C, json, sys
import numpy as np
import envutil_amd as ea
L = ea.lib()
L.eu_hip_diag_host_source.argtypes = [C.c_void_p, C.c_int, C.c_void_p]

def source(nch, masked=-1):
    f = ea.facet_spec(ea.SPHERICAL, 256, 128, 360.0, nchannels=nch, masked=masked).c_struct()
    h = C.c_void_p()
    assert L.eu_hip_diag_host_source(C.byref(f), 1, C.byref(h)) == 0
    return h

rays = np.zeros((4, 10, 9), np.float32); rays[..., 2::3] = 1.0
taps = np.array([[0, 0, 1.0]], np.float32)
out = np.zeros((4, 10, 4), np.float32)
src3, src4m = source(3), source(4, masked=0)

def call(timed=False, src=src3, out_ptr=out.ctypes.data, out_stride=None, **kw):
    r = ea.Rays()
    r.width, r.height, r.ninputs, r.nchannels = 10, 4, 3, 3
    r.rays, r.rays_on_device = rays.ctypes.data, int(timed)
    for k, v in kw.items():
        setattr(r, k, v)
    if "ray_row_stride_bytes" not in kw:
        r.ray_row_stride_bytes = r.width * r.ninputs * 4
    if out_stride is None:
        out_stride = r.width * max(r.nchannels, 1) * 4
    ms = C.c_float()
    if timed:
        rc = L.eu_hip_render_rays_timed(C.byref(r), src, C.c_void_p(out_ptr), out_stride, 3, C.byref(ms))
    else:
        rc = L.eu_hip_render_rays(C.byref(r), src, C.c_void_p(out_ptr), out_stride, 0, None)
    return [rc, L.eu_hip_last_error().decode()]

tp = taps.ctypes.data_as(C.POINTER(C.c_float))
res = {}
for timed in (False, True):
    t = "timed " if timed else ""
    res[t + "valid rays"] = call(timed)
    res[t + "valid ninepacks"] = call(timed, ninputs=9, ntaps=1, taps=tp)
    res[t + "valid padded"] = call(timed, ray_row_stride_bytes=10 * 12 + 8, out_stride=10 * 12 + 20)
    res[t + "valid repix"] = call(timed, nchannels=4)
    res[t + "valid mask 4->2"] = call(timed, src=src4m, nchannels=2)
    res[t + "bad null source"] = call(timed, src=None)
    res[t + "bad null out"] = call(timed, out_ptr=None)
    res[t + "bad null rays"] = call(timed, rays=None)
    res[t + "bad ninputs 6"] = call(timed, ninputs=6)
    res[t + "bad ninputs 0"] = call(timed, ninputs=0)
    res[t + "bad taps with rays"] = call(timed, ntaps=1, taps=tp)
    res[t + "bad tap pointer with rays"] = call(timed, taps=tp)
    res[t + "bad ninepacks without taps"] = call(timed, ninputs=9)
    res[t + "bad ninepacks, null tap table"] = call(timed, ninputs=9, ntaps=1)
    res[t + "bad too many taps"] = call(timed, ninputs=9, ntaps=1025, taps=tp)
    res[t + "bad channels 0"] = call(timed, nchannels=0)
    res[t + "bad channels 5"] = call(timed, nchannels=5)
    res[t + "bad mask 4->3"] = call(timed, src=src4m, nchannels=3)
    res[t + "bad width 0"] = call(timed, width=0)
    res[t + "bad height -1"] = call(timed, height=-1)
    res[t + "bad ray stride short"] = call(timed, ray_row_stride_bytes=10 * 12 - 4)
    res[t + "bad ray stride odd"] = call(timed, ray_row_stride_bytes=10 * 12 + 2)
    res[t + "bad out stride short"] = call(timed, out_stride=10 * 12 - 4)
    res[t + "bad out stride odd"] = call(timed, out_stride=10 * 12 + 3)
res["bad null eu_rays"] = [L.eu_hip_render_rays(None, src3, C.c_void_p(out.ctypes.data), 120, 0, None),
                           L.eu_hip_last_error().decode()]
res["devices"] = L.eu_hip_device_count()
for h in (src3, src4m):
    L.eu_hip_source_release(h)
print("RESULT " + json.dumps(res))
'''


@pytest.fixture(scope="module")
def results():
    import json
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def test_argument_errors_come_before_the_device(results):
    bad = {k: v for k, v in results.items() if k.split("timed ")[-1].startswith("bad ")}
    assert "bad null eu_rays" in bad
    assert len(bad) >= 2 * 19
    for what, (rc, msg) in bad.items():
        assert rc == ARGUMENT, (what, rc, msg)
        assert msg and "no HIP device" not in msg, (what, msg)


def test_valid_calls_end_in_no_device(results):
    good = {k: v for k, v in results.items() if k.split("timed ")[-1].startswith("valid ")}
    assert len(good) == 10
    for what, (rc, msg) in good.items():
        if results["devices"] == 0:
            assert rc == NO_DEVICE, (what, rc, msg)
            assert "no HIP device" in msg, (what, msg)
        else:
            # the child saw a device after all: the call gets as far as the handle, which has no container
            assert rc == HANDLE and "no container" in msg, (what, rc, msg)


def test_python_wrapper_refuses_malformed_arrays():
    class fake:
        class fct:
            nchannels = 3
        handle = None
    with pytest.raises(ea.EuError):
        ea.render_rays(fake, np.zeros((5, 4), np.float32))              # neither rays nor ninepacks
    with pytest.raises(ea.EuError):
        ea.render_rays(fake, np.zeros((5, 3), np.float32), out=np.zeros((5, 4), np.float32))   # out of another shape
    with pytest.raises(ea.EuError):
        ea.render_rays(fake, np.zeros((6, 5, 6), np.float32)[..., ::2])  # rays that are not dense
