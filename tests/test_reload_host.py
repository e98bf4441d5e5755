"""What eu_hip_source_reload and eu_hip_source_load_ycbcr do without a device: every refusal is EU_ERR_ARGUMENT or
EU_ERR_HANDLE with a message that names the field, before a device is looked for; a well-formed call then ends in
EU_ERR_NO_DEVICE. The handle comes from eu_hip_diag_host_source, which needs no device and has no container."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import envutil_amd as ea

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, NO_DEVICE, ARGUMENT, HANDLE = 0, -1, -2, -5

# run in a child that is asked not to see a device (HIP_VISIBLE_DEVICES=-1): the same on a machine with a GPU
CHILD = r'''
import ctypes as C, json
import numpy as np
import envutil_amd as ea
from envutil_amd import api
L = ea.lib()
L.eu_hip_diag_host_source.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
W, H = 12, 6

def source(nch, prj=ea.RECTILINEAR, w=W, h=H):
    f = ea.facet_spec(prj, w, h, 60.0, nchannels=nch).c_struct()
    s = C.c_void_p()
    assert L.eu_hip_diag_host_source(C.byref(f), 1, C.byref(s)) == 0
    return s

def vp(x):
    return C.cast(C.pointer(x), C.c_void_p) if x is not None else None

src3, src4, src1 = source(3), source(4), source(1)
floats3 = np.zeros((H, W, 3), np.float32)
bytes3 = np.zeros((H, W, 3), np.uint8)
words3 = np.zeros((H, W, 3), np.uint16)
quads = np.zeros((H, W, 4), np.uint8)
tab8 = np.zeros(256, np.float32); tab16 = np.zeros(65536, np.float32); tab_rgbe = np.zeros(65536, np.float32)
y8 = np.zeros((H, W), np.uint8); c8 = np.zeros((H // 2, W // 2, 2), np.uint8)
y16 = np.zeros((H, W + 1), np.uint16); c16 = np.zeros((H // 2, W // 2 + 1, 2), np.uint16)
px_x = np.array([1.0, 5.0, 3.0], np.float32); px_y = np.array([1.0, 1.0, 4.0], np.float32)
poly = api.MaskPolygon(3, px_x.ctypes.data, px_y.ctypes.data)

def edit(**kw):
    e = api.FacetEdit()
    e.polygons, e.npolygons = C.cast(C.pointer(poly), C.c_void_p), 1
    for k, v in kw.items():
        setattr(e, k, v)
    return e

def ycc(bits=8, **kw):
    y, c, t = (y8, c8, tab8) if bits == 8 else (y16, c16, tab16)
    size = bits // 8
    p = api.Ycbcr(y.ctypes.data, c.ctypes.data, c.ctypes.data + size, y.strides[0], c.strides[0], 2, 2, 2, bits, 0,
                  t.ctypes.data, t.ctypes.data, 1.5, -0.2, -0.5, 1.8)
    for k, v in kw.items():
        setattr(p, k, v)
    return p

def samples(bits=8, **kw):
    a, t = (bytes3, tab8) if bits == 8 else (words3, tab16)
    s = api.Samples(a.ctypes.data, bits, 0, 3, 0, t.ctypes.data, None)
    for k, v in kw.items():
        setattr(s, k, v)
    return s

def rgbe(**kw):
    r = api.Rgbe(quads.ctypes.data, 0, None)
    for k, v in kw.items():
        setattr(r, k, v)
    return r

def last(rc):
    return [rc, L.eu_hip_last_error().decode()]

def reload(src=src3, kind=api.PX_FLOATS, floats=floats3.ctypes.data, pixel_channels=3, on_device=0, smp=None, rg=None,
           yc=None, ed=None, prefilter=1):
    px = api.Pixels(kind, floats, pixel_channels, on_device, vp(smp), vp(rg), vp(yc), vp(ed))
    return last(L.eu_hip_source_reload(src, C.byref(px), prefilter, None))

def load_ycbcr(nch=3, yc=None, ed=None, degree=1, prefilter=1, out=True, prj=ea.RECTILINEAR, w=W, h=H, null_px=False):
    f = ea.facet_spec(prj, w, h, 60.0 if prj != ea.CUBEMAP else 90.0, nchannels=nch).c_struct()
    s = C.c_void_p()
    p = None if null_px else C.byref(yc if yc is not None else ycc())
    return last(L.eu_hip_source_load_ycbcr(C.byref(f), p, vp(ed), degree, prefilter, 8, 64, C.byref(s) if out else None))

res = {}
# ---- eu_hip_source_reload
res["reload valid floats"] = reload()
res["reload valid floats 3 of 4"] = reload(src=src4)
res["reload valid floats edited"] = reload(src=src4, ed=edit())
res["reload valid samples"] = reload(kind=api.PX_SAMPLES, smp=samples())
res["reload valid samples 16"] = reload(kind=api.PX_SAMPLES, smp=samples(16))
res["reload valid rgbe"] = reload(kind=api.PX_RGBE, rg=rgbe())
res["reload valid rgbe table"] = reload(kind=api.PX_RGBE, rg=rgbe(colour_table=tab_rgbe.ctypes.data), src=src4)
res["reload valid ycbcr"] = reload(kind=api.PX_YCBCR, yc=ycc())
res["reload valid ycbcr 16 edited"] = reload(kind=api.PX_YCBCR, yc=ycc(16), src=src4, ed=edit())
res["reload bad null handle|src"] = reload(src=None)
L.eu_hip_diag_host_replica.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
replica = C.c_void_p()
fr = ea.facet_spec(ea.RECTILINEAR, W, H, 60.0, nchannels=3).c_struct()
assert L.eu_hip_diag_host_replica(C.byref(fr), 1, C.byref(replica)) == 0
res["reload bad replica handle|is_replica"] = reload(src=replica)
res["reload bad null pixels|px"] = last(L.eu_hip_source_reload(src3, None, 1, None))
res["reload bad kind 4|kind"] = reload(kind=4)
res["reload bad kind -1|kind"] = reload(kind=-1)
res["reload bad null floats|floats"] = reload(floats=None)
res["reload bad floats 1 of 3|pixel_channels"] = reload(pixel_channels=1)
res["reload bad floats 4 of 3|pixel_channels"] = reload(pixel_channels=4)
res["reload bad floats gain on 3|channels"] = reload(pixel_channels=2)
res["reload bad floats mask on 3|channels"] = reload(ed=edit())
res["reload bad floats crop kind|crop kind"] = reload(src=src4, ed=edit(crop_kind=3))
res["reload bad samples missing|samples"] = reload(kind=api.PX_SAMPLES)
res["reload bad samples null data|data"] = reload(kind=api.PX_SAMPLES, smp=samples(data=None))
res["reload bad samples bits|bits"] = reload(kind=api.PX_SAMPLES, smp=samples(bits=12))
res["reload bad samples table|colour table"] = reload(kind=api.PX_SAMPLES, smp=samples(colour_table=None))
res["reload bad samples channels|pixel_channels"] = reload(kind=api.PX_SAMPLES, smp=samples(pixel_channels=1))
res["reload bad samples odd device|even address"] = reload(kind=api.PX_SAMPLES, smp=samples(16, on_device=1, data=words3.ctypes.data + 1))
res["reload bad rgbe missing|rgbe"] = reload(kind=api.PX_RGBE)
res["reload bad rgbe null data|data"] = reload(kind=api.PX_RGBE, rg=rgbe(data=None))
res["reload bad rgbe on 1 channel|channels"] = reload(kind=api.PX_RGBE, rg=rgbe(), src=src1)
res["reload bad rgbe mask on 3|channels"] = reload(kind=api.PX_RGBE, rg=rgbe(), ed=edit())
res["reload bad rgbe device alignment|4-byte"] = reload(kind=api.PX_RGBE, rg=rgbe(on_device=1, data=quads.ctypes.data + 2))
res["reload bad ycbcr missing|ycbcr"] = reload(kind=api.PX_YCBCR)
res["reload bad ycbcr on 1 channel|nchannels"] = reload(kind=api.PX_YCBCR, yc=ycc(), src=src1)
res["reload bad ycbcr bits|bits"] = reload(kind=api.PX_YCBCR, yc=ycc(bits=10))
res["reload bad ycbcr mask on 3|channels"] = reload(kind=api.PX_YCBCR, yc=ycc(), ed=edit())
res["reload bad prefilter degree|prefilter"] = reload(prefilter=10)
res["reload bad prefilter degree -1|prefilter"] = reload(kind=api.PX_YCBCR, yc=ycc(), prefilter=-1)
# ---- eu_hip_source_load_ycbcr
res["load valid 8 bit"] = load_ycbcr()
res["load valid 16 bit, 4 channels"] = load_ycbcr(nch=4, yc=ycc(16))
res["load valid edited"] = load_ycbcr(nch=4, ed=edit())
res["load valid planar 4:4:4"] = load_ycbcr(yc=ycc(c_step=1, sub_x=1, sub_y=1, cb=y8.ctypes.data, cr=y8.ctypes.data))
res["load bad null ycbcr|null"] = load_ycbcr(null_px=True)
res["load bad null out|null"] = load_ycbcr(out=False)
res["load bad null y|plane"] = load_ycbcr(yc=ycc(y=None))
res["load bad null cb|plane"] = load_ycbcr(yc=ycc(cb=None))
res["load bad null cr|plane"] = load_ycbcr(yc=ycc(cr=None))
res["load bad null y_table|table"] = load_ycbcr(yc=ycc(y_table=None))
res["load bad null c_table|table"] = load_ycbcr(yc=ycc(c_table=None))
res["load bad bits 10|bits"] = load_ycbcr(yc=ycc(bits=10))
res["load bad c_step 0|c_step"] = load_ycbcr(yc=ycc(c_step=0))
res["load bad c_step 3|c_step"] = load_ycbcr(yc=ycc(c_step=3))
res["load bad sub_x 0|sub_x"] = load_ycbcr(yc=ycc(sub_x=0))
res["load bad sub_x 4|sub_x"] = load_ycbcr(yc=ycc(sub_x=4))
res["load bad sub_y 3|sub_y"] = load_ycbcr(yc=ycc(sub_y=3))
res["load bad y_pitch short|y_pitch"] = load_ycbcr(yc=ycc(y_pitch=W - 1))
res["load bad c_pitch short|c_pitch"] = load_ycbcr(yc=ycc(c_pitch=W - 2))
res["load bad c_pitch short planar|c_pitch"] = load_ycbcr(yc=ycc(c_step=1, sub_x=1, cb=y8.ctypes.data, cr=y8.ctypes.data, c_pitch=W - 1))
res["load bad 16 bit y odd|even"] = load_ycbcr(yc=ycc(16, y=y16.ctypes.data + 1))
res["load bad 16 bit cb odd|even"] = load_ycbcr(yc=ycc(16, cb=c16.ctypes.data + 1))
res["load bad 16 bit cr odd|even"] = load_ycbcr(yc=ycc(16, cr=c16.ctypes.data + 3))
res["load bad 16 bit y_pitch odd|even"] = load_ycbcr(yc=ycc(16, y_pitch=2 * W + 1))
res["load bad 16 bit c_pitch odd|even"] = load_ycbcr(yc=ycc(16, c_pitch=2 * W + 3))
res["load bad nchannels 1|nchannels"] = load_ycbcr(nch=1)
res["load bad nchannels 2|nchannels"] = load_ycbcr(nch=2)
res["load bad edit on 3 channels|channels"] = load_ycbcr(ed=edit())
res["load bad spline degree|degree"] = load_ycbcr(degree=10)
res["load bad prefilter degree|degree"] = load_ycbcr(prefilter=-1)
# ---- eu_hip_ycbcr_floats: the same plane checks, and a host function
out = np.zeros((H, W, 3), np.float32)
res["floats valid"] = last(L.eu_hip_ycbcr_floats(C.byref(ycc()), W, H, 3, out.ctypes.data))
res["floats bad device planes|on_device"] = last(L.eu_hip_ycbcr_floats(C.byref(ycc(on_device=1)), W, H, 3, out.ctypes.data))
res["floats bad nchannels|nchannels"] = last(L.eu_hip_ycbcr_floats(C.byref(ycc()), W, H, 2, out.ctypes.data))
res["floats bad width|width"] = last(L.eu_hip_ycbcr_floats(C.byref(ycc()), 0, H, 3, out.ctypes.data))
res["floats bad out|out"] = last(L.eu_hip_ycbcr_floats(C.byref(ycc()), W, H, 3, None))
res["release without scratch"] = last(L.eu_hip_reload_scratch_release())
res["devices"] = L.eu_hip_device_count()
for s in (src3, src4, src1, replica):
    L.eu_hip_source_release(s)
print("RESULT " + json.dumps(res))
'''


@pytest.fixture(scope="module")
def results():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def test_every_refusal_names_its_field_before_the_device(results):
    bad = {k: v for k, v in results.items() if " bad " in k}
    assert sum(k.startswith("reload bad") for k in bad) >= 28 and sum(k.startswith("load bad") for k in bad) >= 26
    for what, (rc, msg) in bad.items():
        field = what.split("|")[1]
        want = HANDLE if what.startswith(("reload bad null handle", "reload bad replica handle")) else ARGUMENT
        assert rc == want, (what, rc, msg)
        assert field in msg and "no HIP device" not in msg, (what, msg)
        if what.startswith("reload"):
            assert msg.startswith("source_reload"), (what, msg)


def test_well_formed_calls_end_in_no_device(results):
    good = {k: v for k, v in results.items() if " valid" in k and not k.startswith("floats")}
    assert len(good) == 13
    for what, (rc, msg) in good.items():
        if results["devices"] == 0:
            assert rc == NO_DEVICE and "no HIP device" in msg, (what, rc, msg)
        elif what.startswith("reload"):
            # the child saw a device after all: the call gets as far as the handle, which has no container
            assert rc == HANDLE and "no container" in msg, (what, rc, msg)
        else:
            assert rc == OK, (what, rc, msg)          # a load of zero planes on the device the child saw after all


def test_host_function_and_scratch_release_need_no_device(results):
    assert results["floats valid"][0] == OK
    assert results["release without scratch"][0] == OK


def test_python_wrapper_refuses_malformed_planes():
    y = np.zeros((6, 8), np.uint8)
    m = ea.ycbcr_matrix("601")
    with pytest.raises(ea.EuError):
        ea.ycbcr_floats(y, np.zeros((3, 5, 2), np.uint8), m, None, None)           # chroma width fits neither 8 nor 4
    with pytest.raises(ea.EuError):
        ea.ycbcr_floats(y, (np.zeros((3, 4), np.uint8), np.zeros((3, 4), np.uint16)), m, None, None)   # two sample types
    with pytest.raises(ea.EuError):
        ea.ycbcr_floats(y.astype(np.float32), np.zeros((3, 4, 2), np.uint8), m, None, None)
    with pytest.raises(ea.EuError):
        ea.ycbcr_floats(np.zeros((6, 24), np.uint8)[:, ::3], np.zeros((3, 4, 2), np.uint8), m, None, None)   # luma not dense
    with pytest.raises(ea.EuError):
        ea.ycbcr_floats(y, np.zeros((3, 4, 2), np.uint8), m, np.zeros(100, np.float32), None)            # a short table
    with pytest.raises(ea.EuError):
        ea.ycbcr_floats(y, np.zeros((3, 4, 2), np.uint8), m[:3], None, None)
