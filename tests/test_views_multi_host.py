"""What eu_hip_render_views_multi does without a device: every argument error is EU_ERR_ARGUMENT (a null entry of
the facet list EU_ERR_HANDLE, a job the path does not render EU_ERR_UNSUPPORTED) with a message that names the
cause, before a device is looked for; a valid call then ends in EU_ERR_NO_DEVICE. The chunk rule with a facet count
is plain C++ and is checked through a host program."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import envutil_amd as ea

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "envutil_amd", "build", "views_multi_chunk_demo")
OK, NO_DEVICE, ARGUMENT, UNSUPPORTED, HANDLE = 0, -1, -2, -3, -5


def test_views_per_chunk_with_a_facet_count_host_program():
    """one facet gives the single-source values, views * nfct never exceeds a grid's y extent, at least one view"""
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "csrc", "views_multi_chunk_demo.cc"), "-o", EXE])
    r = subprocess.run([EXE], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAILED" not in r.stdout and "all ok" in r.stdout
    assert r.stdout.count("ok: ") >= 11


# As in test_views_host.py: a child process that is asked not to see a device (HIP_VISIBLE_DEVICES=-1), source
# handles from eu_hip_diag_host_source, which needs no device and has no container.
CHILD = r'''
import ctypes as C, json, math, sys
import numpy as np
import envutil_amd as ea
L = ea.lib()
L.eu_hip_diag_host_source.argtypes = [C.c_void_p, C.c_int, C.c_void_p]

def source(nch, masked=-1, translation=None, degree=1, yaw=0.0):
    f = ea.facet_spec(ea.SPHERICAL, 256, 128, 360.0, nchannels=nch, masked=masked, translation=translation, yaw=yaw).c_struct()
    h = C.c_void_p()
    assert L.eu_hip_diag_host_source(C.byref(f), degree, C.byref(h)) == 0
    return h

W, H = 10, 4
out = np.zeros((2, H, W, 4), np.float32)
a3, b3, c3 = source(3), source(3, yaw=90.0), source(3, yaw=180.0)
b4m, b3d3, b3tr = source(4, masked=0, yaw=90.0), source(3, degree=3, yaw=90.0), source(3, translation=dict(x=0.1), yaw=90.0)
args = ea.arguments(ea.RECTILINEAR, W, H, 60.0, twine=2)
single = ea.facet_spec(ea.RECTILINEAR, W, H, 60.0).c_struct()
NULL = "null list"

def views(n=2, a=args, **kw):
    arr = (ea.View * n)()
    for k in range(n):
        arr[k].yaw = 0.1 * k
        arr[k].x0, arr[k].x1, arr[k].y0, arr[k].y1 = (float(v) for v in a.extent)
    for name, v in kw.items():
        setattr(arr[n - 1], name, v)
    return arr

def call(srcs=(a3, b3, c3), nsrc=None, out_ptr=out.ctypes.data, nviews=2, vw=None, row=None, view=None, nch=3, trg=True,
         prj=None, twine=False, w=W, h=H, **kw):
    t = args.target(nch)
    t.width, t.height, t.row_end = w, h, h
    if not twine:
        t.ntaps, t.taps = 0, None
    if prj is not None:
        t.projection = prj
    for k, v in kw.items():
        setattr(t, k, v)
    vw = views() if vw is None else vw
    row = w * nch * 4 if row is None else row
    view = h * row if view is None else view
    if srcs == NULL:
        arr, n = None, 3
    else:
        arr = (C.c_void_p * max(len(srcs), 1))(*[s for s in srcs])
        n = len(srcs)
    rc = L.eu_hip_render_views_multi(C.byref(t) if trg else None, vw, nviews, arr, n if nsrc is None else nsrc,
                                     C.c_void_p(out_ptr), row, view, 0, None)
    return [rc, L.eu_hip_last_error().decode()]

res = {}
res["valid plain"] = call()
res["valid twined"] = call(twine=True)
res["valid two facets"] = call(srcs=(a3, b3))
res["valid one facet"] = call(srcs=(a3,))
res["valid one view"] = call(nviews=1)
res["valid padded"] = call(row=W * 12 + 8, view=H * (W * 12 + 8) + 40)
res["valid other channel count"] = call(nch=4)
res["valid hdr_merge"] = call(synopsis=ea.api.SYN_HDR_MERGE)
res["valid mask 4->2"] = call(srcs=(a3, b4m), nch=2)
res["valid mask 4->4"] = call(srcs=(a3, b4m), nch=4)
before = out.copy()
res["zero views"] = call(nviews=0)
res["zero views untouched"] = bool((out == before).all())
res["bad null target"] = call(trg=False)
res["bad null views"] = call(vw=C.c_void_p())
res["bad null sources"] = call(srcs=NULL)
res["bad null out"] = call(out_ptr=None)
res["bad nsrc 0"] = call(nsrc=0)
res["bad nsrc -1"] = call(nsrc=-1)
res["bad nviews -1"] = call(nviews=-1)
res["bad degrees differ"] = call(srcs=(a3, b3d3, c3))
res["bad degrees differ, last"] = call(srcs=(a3, b3, b3d3))
for f in ("yaw", "pitch", "roll", "x0", "x1", "y0", "y1"):
    for name, v in (("nan", math.nan), ("inf", math.inf), ("-inf", -math.inf)):
        res[f"bad view {f} {name}"] = call(vw=views(**{f: v}))
res["bad non-finite in the first view"] = call(vw=(lambda a: (setattr(a[0], "yaw", math.nan), a)[1])(views()))
res["bad stage 1"] = call(stage=1)
res["bad crop"] = call(crop_w=4, crop_h=2, row_end=2)
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
res["bad mask 4->3, second facet"] = call(srcs=(a3, b4m), nch=3)
res["bad mask 4->3, first facet"] = call(srcs=(b4m, a3), nch=3)
res["handle null entry first"] = call(srcs=(None, b3))
res["handle null entry last"] = call(srcs=(a3, b3, None))
res["handle null entry, one facet"] = call(srcs=(None,))
res["unsupported translation, second facet"] = call(srcs=(a3, b3tr))
res["unsupported translation, first facet"] = call(srcs=(b3tr, a3))
res["unsupported projection"] = call(prj=11)
bi = ea.arguments(ea.BIATAN6, 24, 144, 90.0)
wide = ea.arguments(ea.BIATAN6, 24, 144, 135.0)
vb = views(2, bi)
vb[1].x0, vb[1].x1, vb[1].y0, vb[1].y1 = (float(v) for v in wide.extent)
big = np.zeros((2, 144, 24, 3), np.float32)
res["unsupported biatan6 1.75 in the second view"] = call(prj=ea.BIATAN6, w=24, h=144, vw=vb, out_ptr=big.ctypes.data)
res["valid biatan6"] = call(prj=ea.BIATAN6, w=24, h=144, vw=views(2, bi), out_ptr=big.ctypes.data)
res["devices"] = L.eu_hip_device_count()
for h_ in (a3, b3, c3, b4m, b3d3, b3tr):
    L.eu_hip_source_release(h_)
print("RESULT " + json.dumps(res))
'''


@pytest.fixture(scope="module")
def results():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def test_argument_errors_come_before_the_device(results):
    bad = {k: v for k, v in results.items() if k.startswith("bad ")}
    assert len(bad) == 9 + 22 + 16
    for what, (rc, msg) in bad.items():
        assert rc == ARGUMENT, (what, rc, msg)
        assert msg and "no HIP device" not in msg, (what, msg)
    for what, word in (("bad degrees differ", "degree"), ("bad nsrc 0", "source"), ("bad null sources", "null"),
                       ("bad mask 4->3, second facet", "mask_for"), ("bad view yaw nan", "non-finite"),
                       ("bad crop", "crop"), ("bad single", "single"), ("bad row stride short", "stride")):
        assert word in results[what][1], (what, results[what][1])


def test_a_null_entry_is_a_handle_error(results):
    for what in ("handle null entry first", "handle null entry last", "handle null entry, one facet"):
        rc, msg = results[what]
        assert rc == HANDLE and "null source" in msg, (what, rc, msg)


def test_unsupported_jobs_are_named(results):
    un = {k: v for k, v in results.items() if k.startswith("unsupported ")}
    assert len(un) == 4
    for what, (rc, msg) in un.items():
        assert rc == UNSUPPORTED and msg and "no HIP device" not in msg, (what, rc, msg)
    assert "translation" in results["unsupported translation, second facet"][1]
    assert "translation" in results["unsupported translation, first facet"][1]
    assert "stepper" in results["unsupported projection"][1]
    assert "1.75" in results["unsupported biatan6 1.75 in the second view"][1]


def test_zero_views_is_ok_and_writes_nothing(results):
    assert results["zero views"][0] == OK
    assert results["zero views untouched"] is True


def test_valid_calls_end_in_no_device(results):
    good = {k: v for k, v in results.items() if k.startswith("valid ")}
    assert len(good) == 11
    for what, (rc, msg) in good.items():
        if results["devices"] == 0:
            assert rc == NO_DEVICE, (what, rc, msg)
            assert "no HIP device" in msg, (what, msg)
        else:
            # the child saw a device after all: the call gets as far as the handles, which have no container
            assert rc == HANDLE and "no container" in msg, (what, rc, msg)


def test_python_wrapper_refuses_what_the_call_does_not_render():
    class fake:
        class fct:
            nchannels = 3
        handle = None
    plain = ea.arguments(ea.RECTILINEAR, 16, 8, 60.0)
    for sources in ([fake, fake], (fake, fake, fake), [fake]):
        for a in (ea.arguments(ea.RECTILINEAR, 16, 8, 60.0, crop=(0, 8, 0, 4)),
                  ea.arguments(ea.RECTILINEAR, 16, 8, 60.0, tethered=True),
                  ea.arguments.for_single(ea.facet_spec(ea.RECTILINEAR, 16, 8, 60.0))):
            with pytest.raises(ea.EuError, match="no crop, not tethered, no single"):
                ea.render_views(a, [(0, 0, 0)], sources)
        with pytest.raises(ea.EuError, match="a view is"):
            ea.render_views(plain, [(0, 0)], sources)
        with pytest.raises(ea.EuError, match="shape"):
            ea.render_views(plain, [(0, 0, 0)], sources, out=np.zeros((1, 8, 16, 4), np.float32))
    with pytest.raises(ea.EuError, match="no source"):
        ea.render_views(plain, [(0, 0, 0)], [])
