"""What eu_hip_render_layers does without a device: every argument error is reported as EU_ERR_ARGUMENT with a
message before a device is looked for, a valid call then ends in EU_ERR_NO_DEVICE; the choice between the two
kernel forms (eu_select_layer_path), the chunking arithmetic and the EU_HIP_LAYERS_MAX switch are plain C++ and are
checked through a host program."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import envutil_amd as ea

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "envutil_amd", "build", "select_layers_demo")
OK, NO_DEVICE, ARGUMENT, UNSUPPORTED, HANDLE = 0, -1, -2, -3, -5


def test_select_layer_path_chunks_and_switch_host_program():
    """the grid of jobs and switches of the views demo, every answer also held against eu_select_view_path;
    EU_HIP_LAYERS_MAX as eu_read_switches parses it; launches and twined groups over L = 0, 1, G, G + 1, 2 G + 1, max,
    max + 1: every layer walked once, in order"""
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "csrc", "select_layers_demo.cc"), "-o", EXE])
    env = {k: v for k, v in os.environ.items() if not k.startswith("EU_HIP_")}
    r = subprocess.run([EXE], capture_output=True, text=True, env=env)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAILED" not in r.stdout and "all ok" in r.stdout
    assert r.stdout.count("-> packed") >= 144 and r.stdout.count("-> general") >= 14
    # degrees 0 and 4 to 9 under every EU_HIP_R4 / HYBRID / KERNEL / DIRECT combination: never packed
    assert "ok: high degrees: 16128 combinations, all general" in r.stdout
    assert r.stdout.count("EU_HIP_LAYERS_MAX") >= 5 + 6 * 4 * 9
    assert int(re.search(r"^EU_LAYERS_GROUP (\d+)$", r.stdout, re.M).group(1)) in (1, 2, 4)


# The calls below run in a child process that is asked not to see a device (HIP_VISIBLE_DEVICES=-1), so that
# they mean the same on a machine with a GPU: argument errors first, then EU_ERR_NO_DEVICE. The source handles
# come from eu_hip_diag_host_source, which needs no device and has no container.
CHILD = r'''
import ctypes as C, json, sys
import numpy as np
import envutil_amd as ea
L = ea.lib()
L.eu_hip_diag_host_source.argtypes = [C.c_void_p, C.c_int, C.c_void_p]

def source(nch=3, degree=1, w=256, h=128, hfov=360.0, masked=-1, translation=None, **kw):
    f = ea.facet_spec(ea.SPHERICAL, w, h, hfov, nchannels=nch, masked=masked, translation=translation, **kw).c_struct()
    hd = C.c_void_p()
    assert L.eu_hip_diag_host_source(C.byref(f), degree, C.byref(hd)) == 0
    return hd

W, H = 10, 4
out = np.zeros((3, H, W, 4), np.float32)
a, b, c = source(), source(), source()
masked, translated = source(4, masked=0), source(translation=dict(x=0.1))
other = dict(nch=source(4), degree=source(degree=3), size=source(w=128, h=64), hfov=source(hfov=300.0),
             yaw=source(yaw=10.0))
args = ea.arguments(ea.RECTILINEAR, W, H, 60.0, twine=2)
single = ea.facet_spec(ea.RECTILINEAR, W, H, 60.0).c_struct()

def call(layers=(a, b, c), n=None, out_ptr=out.ctypes.data, row=None, layer=None, nch=3, trg=True, prj=None,
         twine=False, null_list=False, **kw):
    t = args.target(nch)
    if not twine:
        t.ntaps, t.taps = 0, None
    if prj is not None:
        t.projection = prj
    for k, v in kw.items():
        setattr(t, k, v)
    row = W * nch * 4 if row is None else row
    layer = H * row if layer is None else layer
    arr = (C.c_void_p * max(len(layers), 1))(*[h.value if h is not None else None for h in layers])
    rc = L.eu_hip_render_layers(C.byref(t) if trg else None, None if null_list else arr, len(layers) if n is None else n,
                                C.c_void_p(out_ptr), row, layer, 0, None)
    return [rc, L.eu_hip_last_error().decode()]

res = {}
res["valid plain"] = call()
res["valid twined"] = call(twine=True)
res["valid one layer"] = call(layers=(a,))
res["valid the same layer twice"] = call(layers=(a, a))
res["valid padded"] = call(row=W * 12 + 8, layer=H * (W * 12 + 8) + 40)
res["valid repix"] = call(nch=4)
before = out.copy()
res["zero layers"] = call(n=0)
res["zero layers untouched"] = bool((out == before).all())
res["bad null target"] = call(trg=False)
res["bad null layers"] = call(null_list=True)
res["bad null out"] = call(out_ptr=None)
res["bad nlayers -1"] = call(n=-1)
res["bad stage 1"] = call(stage=1)
res["bad stage 3"] = call(stage=3, twine=True)
res["bad crop"] = call(crop_w=4, crop_h=2)
res["bad bands"] = call(band_rows=4, band_count=2, band_index=0, row_end=4)
res["bad single"] = call(single=C.pointer(single))
res["bad srgba8"] = call(out_format=ea.api.OUT_SRGBA8)
res["bad row_begin"] = call(row_begin=1)
res["bad row_end"] = call(row_end=H - 1)
res["bad row stride odd"] = call(row=W * 12 + 2)
res["bad layer stride odd"] = call(layer=H * W * 12 + 2)
res["bad row stride short"] = call(row=W * 12 - 4)
res["bad layer stride short"] = call(layer=H * W * 12 - 4)
res["bad layer stride short for padded rows"] = call(row=W * 12 + 8, layer=H * W * 12)
res["bad channels 0"] = call(nch=0)
res["bad channels 5"] = call(nch=5)
res["bad mask_for layer"] = call(layers=(source(4), masked), nch=4)
res["bad mask_for first"] = call(layers=(masked,), nch=4)
for what, h in other.items():
    res["bad differs " + what] = call(layers=(a, b, h))
res["handle null entry"] = call(layers=(a, None, c))
res["unsupported translation"] = call(layers=(translated, translated))
res["unsupported projection"] = call(prj=11)
res["devices"] = L.eu_hip_device_count()
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
    assert len(bad) == 4 + 15 + 2 + 5
    for what, (rc, msg) in bad.items():
        assert rc == ARGUMENT, (what, rc, msg)
        assert msg and "no HIP device" not in msg, (what, msg)


def test_a_differing_layer_is_named(results):
    for what, word in (("nch", "channel count"), ("degree", "spline degree"), ("size", "size"), ("hfov", "field of view"),
                       ("yaw", "orientation")):
        msg = results["bad differs " + what][1]
        assert "layer 2 differs" in msg and word in msg, (what, msg)
    assert "layer 1" in results["bad mask_for layer"][1] and "mask_for" in results["bad mask_for layer"][1]
    assert "layer 0" in results["bad mask_for first"][1]


def test_a_null_entry_is_a_handle_error(results):
    rc, msg = results["handle null entry"]
    assert rc == HANDLE and "layer 1" in msg, (rc, msg)


def test_unsupported_jobs_are_named(results):
    for what in ("unsupported translation", "unsupported projection"):
        rc, msg = results[what]
        assert rc == UNSUPPORTED and msg and "no HIP device" not in msg, (what, rc, msg)
    assert "translation" in results["unsupported translation"][1]


def test_zero_layers_is_ok_and_writes_nothing(results):
    assert results["zero layers"][0] == OK
    assert results["zero layers untouched"] is True


def test_valid_calls_end_in_no_device(results):
    good = {k: v for k, v in results.items() if k.startswith("valid ")}
    assert len(good) == 6
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
    for a in (ea.arguments(ea.RECTILINEAR, 16, 8, 60.0, crop=(0, 8, 0, 4)),
              ea.arguments(ea.RECTILINEAR, 16, 8, 60.0, tethered=True),
              ea.arguments.for_single(ea.facet_spec(ea.RECTILINEAR, 16, 8, 60.0))):
        with pytest.raises(ea.EuError):
            ea.render_layers(a, [fake])
    with pytest.raises(ea.EuError):
        ea.render_layers(plain, fake)                                                    # not a list
    with pytest.raises(ea.EuError):
        ea.render_layers(plain, [])                                                      # nothing to shape the result by
    with pytest.raises(ea.EuError):
        ea.render_layers(plain, [fake], out=np.zeros((1, 8, 16, 4), np.float32))         # out of another shape
    with pytest.raises(ea.EuError):
        ea.render_layers(plain, [fake, fake], out=np.zeros((1, 8, 16, 3), np.float32))   # one frame for two layers
    with pytest.raises(ea.EuError):
        ea.render_layers(plain, [fake], out=np.zeros((1, 8, 16, 6), np.float32)[..., ::2])   # pixels not dense
    with pytest.raises(ea.EuError):
        ea.render_layers(plain, [fake], out=np.zeros((1, 8, 16, 3), np.float64))
