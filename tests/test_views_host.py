"""What eu_hip_render_views does without a device: every argument error is reported as EU_ERR_ARGUMENT with a
message before a device is looked for, a valid call then ends in EU_ERR_NO_DEVICE; the choice between the two
kernel forms (eu_select_view_path), the chunk size and the EU_HIP_VIEWS_MAX_KB switch are plain C++ and are checked
through a host program."""
import os
import subprocess
import sys

import numpy as np
import pytest

import envutil_amd as ea

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "envutil_amd", "build", "select_views_demo")
OK, NO_DEVICE, ARGUMENT, UNSUPPORTED, HANDLE = 0, -1, -2, -3, -5


def test_select_view_path_chunks_and_switch_host_program():
    """every packed case (three sources, both table forms, degrees 1-3, 1-4 channels, with and without twining),
    one job per reason for the general form, the switches that have no say; EU_HIP_VIEWS_MAX_KB as
    eu_read_switches parses it; views per chunk"""
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "csrc", "select_views_demo.cc"), "-o", EXE])
    env = {k: v for k, v in os.environ.items() if not k.startswith("EU_HIP_")}
    r = subprocess.run([EXE], capture_output=True, text=True, env=env)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAILED" not in r.stdout and "all ok" in r.stdout
    assert r.stdout.count("-> packed") >= 144 and r.stdout.count("-> general") >= 14
    # degrees 0 and 4 to 9 under every EU_HIP_R4 / HYBRID / KERNEL / DIRECT combination: never packed
    assert "ok: high degrees: 16128 combinations, all general" in r.stdout
    assert r.stdout.count("EU_HIP_VIEWS_MAX_KB") >= 6


# The calls below run in a child process that is asked not to see a device (HIP_VISIBLE_DEVICES=-1), so that
# they mean the same on a machine with a GPU: argument errors first, then EU_ERR_NO_DEVICE. The source handle
# comes from eu_hip_diag_host_source, which needs no device and has no container.
CHILD = r'''
import ctypes as C, json, math, sys
import numpy as np
import envutil_amd as ea
L = ea.lib()
L.eu_hip_diag_host_source.argtypes = [C.c_void_p, C.c_int, C.c_void_p]

def source(nch, masked=-1, translation=None):
    f = ea.facet_spec(ea.SPHERICAL, 256, 128, 360.0, nchannels=nch, masked=masked, translation=translation).c_struct()
    h = C.c_void_p()
    assert L.eu_hip_diag_host_source(C.byref(f), 1, C.byref(h)) == 0
    return h

W, H = 10, 4
out = np.zeros((2, H, W, 4), np.float32)
src3, src4m, src_tr = source(3), source(4, masked=0), source(3, translation=dict(x=0.1))
args = ea.arguments(ea.RECTILINEAR, W, H, 60.0, twine=2)
single = ea.facet_spec(ea.RECTILINEAR, W, H, 60.0).c_struct()

def views(n=2, **kw):
    arr = (ea.View * n)()
    for k in range(n):
        arr[k].yaw = 0.1 * k
        arr[k].x0, arr[k].x1, arr[k].y0, arr[k].y1 = (float(v) for v in args.extent)
    for name, v in kw.items():
        setattr(arr[n - 1], name, v)
    return arr

def call(src=src3, out_ptr=out.ctypes.data, nviews=2, vw=None, row=None, view=None, nch=3, trg=True, tables=False,
         prj=None, twine=False, **kw):
    t = args.target(nch)
    if not twine:
        t.ntaps, t.taps = 0, None
    if prj is not None:
        t.projection = prj
    for k, v in kw.items():
        setattr(t, k, v)
    vw = views() if vw is None else vw
    row = W * nch * 4 if row is None else row
    view = H * row if view is None else view
    tp = C.byref(t) if trg else None
    if tables:
        bufs = [np.zeros(6 * W + 24 * H, np.float32) for _ in range(4)]
        rc = L.eu_hip_view_tables(tp, vw, src, *[b.ctypes.data for b in bufs])
    else:
        rc = L.eu_hip_render_views(tp, vw, nviews, src, C.c_void_p(out_ptr), row, view, 0, None)
    return [rc, L.eu_hip_last_error().decode()]

res = {}
res["valid plain"] = call()
res["valid twined"] = call(twine=True)
res["valid one view"] = call(nviews=1)
res["valid padded"] = call(row=W * 12 + 8, view=H * (W * 12 + 8) + 40)
res["valid repix"] = call(nch=4)
res["valid mask 4->2"] = call(src=src4m, nch=2)
res["valid tables"] = call(tables=True)
before = out.copy()
res["zero views"] = call(nviews=0)
res["zero views untouched"] = bool((out == before).all())
res["bad null target"] = call(trg=False)
res["bad null views"] = call(vw=C.c_void_p())
res["bad null source"] = call(src=None)
res["bad null out"] = call(out_ptr=None)
res["bad nviews -1"] = call(nviews=-1)
for f in ("yaw", "pitch", "roll", "x0", "x1", "y0", "y1"):
    for name, v in (("nan", math.nan), ("inf", math.inf), ("-inf", -math.inf)):
        res[f"bad view {f} {name}"] = call(vw=views(**{f: v}))
res["bad non-finite in the first view"] = call(vw=(lambda a: (setattr(a[0], "yaw", math.nan), a)[1])(views()))
res["bad stage 1"] = call(stage=1)
res["bad stage 3"] = call(stage=3, twine=True)
res["bad crop"] = call(crop_w=4, crop_h=2)
res["bad bands"] = call(band_rows=4, band_count=2, band_index=0, row_end=4)
res["bad single"] = call(single=C.pointer(single))
res["bad srgba8"] = call(out_format=ea.api.OUT_SRGBA8)
res["bad row_begin"] = call(row_begin=1)
res["bad row_end"] = call(row_end=H - 1)
res["bad row stride odd"] = call(row=W * 12 + 2)
res["bad view stride odd"] = call(view=H * W * 12 + 2)
res["bad row stride short"] = call(row=W * 12 - 4)
res["bad view stride short"] = call(view=H * W * 12 - 4)
res["bad view stride short for padded rows"] = call(row=W * 12 + 8, view=H * W * 12)
res["bad channels 0"] = call(nch=0)
res["bad channels 5"] = call(nch=5)
res["bad mask 4->3"] = call(src=src4m, nch=3)
res["bad tables null view"] = call(tables=True, vw=C.c_void_p())
res["bad tables crop"] = call(tables=True, crop_w=4, crop_h=2)
res["bad tables nan"] = call(tables=True, vw=views(1, x1=math.nan))
res["unsupported translation"] = call(src=src_tr)
res["unsupported projection"] = call(prj=11)
res["devices"] = L.eu_hip_device_count()
for h in (src3, src4m, src_tr):
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
    bad = {k: v for k, v in results.items() if k.startswith("bad ")}
    assert len(bad) >= 5 + 21 + 18
    for what, (rc, msg) in bad.items():
        assert rc == ARGUMENT, (what, rc, msg)
        assert msg and "no HIP device" not in msg, (what, msg)


def test_unsupported_jobs_are_named(results):
    for what in ("unsupported translation", "unsupported projection"):
        rc, msg = results[what]
        assert rc == UNSUPPORTED and msg and "no HIP device" not in msg, (what, rc, msg)
    assert "translation" in results["unsupported translation"][1]


def test_zero_views_is_ok_and_writes_nothing(results):
    assert results["zero views"][0] == OK
    assert results["zero views untouched"] is True


def test_valid_calls_end_in_no_device(results):
    good = {k: v for k, v in results.items() if k.startswith("valid ")}
    assert len(good) == 7
    for what, (rc, msg) in good.items():
        if results["devices"] == 0:
            assert rc == NO_DEVICE, (what, rc, msg)
            assert "no HIP device" in msg, (what, msg)
        else:
            # the child saw a device after all: the call gets as far as the handle, which has no container
            assert rc == HANDLE and "no container" in msg, (what, rc, msg)


def test_python_wrapper_refuses_what_the_call_does_not_render():
    class fake:
        class fct:
            nchannels = 3
        handle = None
    plain = ea.arguments(ea.RECTILINEAR, 16, 8, 60.0)
    for a in (ea.arguments(ea.RECTILINEAR, 16, 8, 60.0, crop=(0, 8, 0, 4)),
              ea.arguments(ea.RECTILINEAR, 16, 8, 60.0, tethered=True),
              ea.arguments.for_single(ea.facet_spec(ea.RECTILINEAR, 16, 8, 60.0))):
        with pytest.raises(ea.EuError):
            ea.render_views(a, [(0, 0, 0)], fake)
        with pytest.raises(ea.EuError):
            ea.view_tables(a, (0, 0, 0), fake)
    with pytest.raises(ea.EuError):
        ea.render_views(plain, [(0, 0)], fake)                                       # not a view
    with pytest.raises(ea.EuError):
        ea.render_views(plain, [(0, 0, 0)], fake, out=np.zeros((1, 8, 16, 4), np.float32))   # out of another shape
    with pytest.raises(ea.EuError):
        ea.render_views(plain, [(0, 0, 0)], fake, out=np.zeros((1, 8, 16, 6), np.float32)[..., ::2])   # pixels not dense
    with pytest.raises(ea.EuError):
        ea.render_views(plain, [(0, 0, 0)], fake, out=np.zeros((1, 8, 16, 3), np.float64))
