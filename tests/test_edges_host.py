"""What eu_hip_source_load_pixels and eu_hip_source_edge_distance do without a device: the flags' own refusals are
EU_ERR_ARGUMENT with a message that names the cause, before a device is looked for; with flags == 0 every feed reaches
the refusals of the matching eu_hip_source_load* call, with that call's result and message; a well-formed call then
ends in EU_ERR_NO_DEVICE."""
import json
import os
import subprocess
import sys

import pytest

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
floats = np.zeros((H, W, 4), np.float32)
bytes3 = np.zeros((H, W, 3), np.uint8)
quads = np.zeros((H, W, 4), np.uint8)
tab8 = np.zeros(256, np.float32)
y8 = np.zeros((H, W), np.uint8); c8 = np.zeros((H // 2, W // 2, 2), np.uint8)
px_x = np.array([1.0, 5.0, 3.0], np.float32); px_y = np.array([1.0, 1.0, 4.0], np.float32)
poly = api.MaskPolygon(3, px_x.ctypes.data, px_y.ctypes.data)

def vp(x):
    return C.cast(C.pointer(x), C.c_void_p) if x is not None else None

def edit(**kw):
    e = api.FacetEdit()
    e.polygons, e.npolygons = C.cast(C.pointer(poly), C.c_void_p), 1
    for k, v in kw.items():
        setattr(e, k, v)
    return e

def ycc(**kw):
    p = api.Ycbcr(y8.ctypes.data, c8.ctypes.data, c8.ctypes.data + 1, y8.strides[0], c8.strides[0], 2, 2, 2, 8, 0,
                  tab8.ctypes.data, tab8.ctypes.data, 1.5, -0.2, -0.5, 1.8)
    for k, v in kw.items():
        setattr(p, k, v)
    return p

def samples(**kw):
    s = api.Samples(bytes3.ctypes.data, 8, 0, 3, 0, tab8.ctypes.data, None)
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

def facet(nch=4, prj=ea.RECTILINEAR, w=W, h=H, window=None):
    return ea.facet_spec(prj, w, h, 90.0 if prj == ea.CUBEMAP else 60.0, nchannels=nch, window=window).c_struct()

def load_pixels(flags=0, nch=4, kind=api.PX_FLOATS, data=floats.ctypes.data, pixel_channels=4, on_device=0, smp=None, rg=None,
                yc=None, ed=None, degree=1, prefilter=1, f=None, null_px=False):
    f = f if f is not None else facet(nch)
    s = C.c_void_p()
    px = api.Pixels(kind, data, pixel_channels, on_device, vp(smp), vp(rg), vp(yc), vp(ed))
    return last(L.eu_hip_source_load_pixels(C.byref(f), None if null_px else C.byref(px), degree, prefilter, 8, 64, flags, C.byref(s)))

def old(name, nch, feed, ed=None, degree=1, prefilter=1):
    f = facet(nch)
    s = C.c_void_p()
    fn = getattr(L, "eu_hip_source_load_" + name)
    return last(fn(C.byref(f), feed, vp(ed), degree, prefilter, 8, 64, C.byref(s)))

res = {}
E = api.LOAD_EDGES
# ---- the flags' own refusals
res["edges bad flag bit 2|flag"] = load_pixels(flags=2)
res["edges bad flag bits|flag"] = load_pixels(flags=E | 0x80000000)
res["edges bad cubemap|cubemap"] = load_pixels(flags=E, f=facet(4, ea.CUBEMAP, 6, 36))
res["edges bad biatan6|cubemap"] = load_pixels(flags=E, f=facet(4, ea.BIATAN6, 6, 36))
res["edges bad nchannels 3|nchannels"] = load_pixels(flags=E, nch=3, pixel_channels=3)
res["edges bad nchannels 1|nchannels"] = load_pixels(flags=E, nch=1, pixel_channels=1)
res["edges bad window width|32768"] = load_pixels(flags=E, f=facet(4, w=40000, h=10))
res["edges bad window height|32768"] = load_pixels(flags=E, f=facet(4, w=10, h=32769))
res["edges bad null pixels|px"] = load_pixels(flags=E, null_px=True)
res["edges bad kind|kind"] = load_pixels(flags=E, kind=7)
res["edges valid floats"] = load_pixels(flags=E)
res["edges valid floats 2 channels"] = load_pixels(flags=E, nch=2, pixel_channels=2)
res["edges valid side 32768"] = load_pixels(flags=E, f=facet(2, w=32768, h=1), pixel_channels=2, degree=99, ed=edit())   # (refused for its degree, not its side)
res["edges valid samples"] = load_pixels(flags=E, kind=api.PX_SAMPLES, smp=samples())
res["edges valid rgbe edited"] = load_pixels(flags=E, kind=api.PX_RGBE, rg=rgbe(), ed=edit())
res["edges valid ycbcr"] = load_pixels(flags=E, kind=api.PX_YCBCR, yc=ycc())
# ---- flags == 0: every feed reaches the matching call's refusals, with its words
pairs = {}
def pair(what, new, was):
    pairs[what] = [new, was]
e3 = edit(pixel_channels=3)
pair("floats pixel_channels", load_pixels(pixel_channels=2), old("edited", 4, floats.ctypes.data, edit(pixel_channels=2)))
pair("floats edit on 3 channels", load_pixels(nch=3, pixel_channels=3, ed=edit()), old("edited", 3, floats.ctypes.data, e3))
pair("floats null", load_pixels(data=None), old("edited", 4, None, edit(pixel_channels=4)))
pair("floats degree", load_pixels(degree=99, ed=edit()), old("edited", 4, floats.ctypes.data, edit(pixel_channels=4), degree=99))
pair("floats prefilter", load_pixels(prefilter=-1, ed=edit()), old("edited", 4, floats.ctypes.data, edit(pixel_channels=4), prefilter=-1))
pair("samples bits", load_pixels(kind=api.PX_SAMPLES, smp=samples(bits=12)), old("samples", 4, C.byref(samples(bits=12))))
pair("samples table", load_pixels(kind=api.PX_SAMPLES, smp=samples(colour_table=None)), old("samples", 4, C.byref(samples(colour_table=None))))
pair("samples data", load_pixels(kind=api.PX_SAMPLES, smp=samples(data=None)), old("samples", 4, C.byref(samples(data=None))))
pair("samples channels", load_pixels(kind=api.PX_SAMPLES, smp=samples(pixel_channels=1)), old("samples", 4, C.byref(samples(pixel_channels=1))))
pair("samples missing", load_pixels(kind=api.PX_SAMPLES), old("samples", 4, None))
pair("samples degree", load_pixels(kind=api.PX_SAMPLES, smp=samples(), degree=-1), old("samples", 4, C.byref(samples()), degree=-1))
pair("rgbe nchannels", load_pixels(nch=2, kind=api.PX_RGBE, rg=rgbe()), old("rgbe", 2, C.byref(rgbe())))
pair("rgbe alignment", load_pixels(kind=api.PX_RGBE, rg=rgbe(on_device=1, data=quads.ctypes.data + 1)), old("rgbe", 4, C.byref(rgbe(on_device=1, data=quads.ctypes.data + 1))))
pair("rgbe missing", load_pixels(kind=api.PX_RGBE), old("rgbe", 4, None))
pair("rgbe edit on 3 channels", load_pixels(nch=3, kind=api.PX_RGBE, rg=rgbe(), ed=edit()), old("rgbe", 3, C.byref(rgbe()), edit()))
pair("ycbcr c_step", load_pixels(kind=api.PX_YCBCR, yc=ycc(c_step=3)), old("ycbcr", 4, C.byref(ycc(c_step=3))))
pair("ycbcr plane", load_pixels(kind=api.PX_YCBCR, yc=ycc(cb=None)), old("ycbcr", 4, C.byref(ycc(cb=None))))
pair("ycbcr pitch", load_pixels(kind=api.PX_YCBCR, yc=ycc(y_pitch=3)), old("ycbcr", 4, C.byref(ycc(y_pitch=3))))
pair("ycbcr missing", load_pixels(kind=api.PX_YCBCR), old("ycbcr", 4, None))
pair("ycbcr prefilter", load_pixels(kind=api.PX_YCBCR, yc=ycc(), prefilter=99), old("ycbcr", 4, C.byref(ycc()), prefilter=99))
pair("valid floats", load_pixels(), old("edited", 4, floats.ctypes.data, edit(pixel_channels=4, npolygons=0)))
pair("valid samples", load_pixels(kind=api.PX_SAMPLES, smp=samples()), old("samples", 4, C.byref(samples())))
pair("valid rgbe", load_pixels(kind=api.PX_RGBE, rg=rgbe()), old("rgbe", 4, C.byref(rgbe())))
pair("valid ycbcr", load_pixels(kind=api.PX_YCBCR, yc=ycc()), old("ycbcr", 4, C.byref(ycc())))
res["pairs"] = pairs
# ---- eu_hip_source_edge_distance and its kin on a handle without a plane
f = facet(4)
src = C.c_void_p()
assert L.eu_hip_diag_host_source(C.byref(f), 1, C.byref(src)) == 0
out = np.zeros((H, W), np.float32)
res["distance bad no plane|no distance plane"] = last(L.eu_hip_source_edge_distance(src, out.ctypes.data, 4 * W, 0, None))
res["distance bad null out|out"] = last(L.eu_hip_source_edge_distance(src, None, 4 * W, 0, None))
res["distance null source"] = last(L.eu_hip_source_edge_distance(None, out.ctypes.data, 4 * W, 0, None))
res["has_edges"] = [L.eu_hip_source_has_edges(src), L.eu_hip_source_has_edges(None)]
L.eu_hip_source_release(src)
res["devices"] = L.eu_hip_device_count()
print("RESULT " + json.dumps(res))
'''


@pytest.fixture(scope="module")
def results():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def test_the_flags_refusals_name_their_cause_before_the_device(results):
    bad = {k: v for k, v in results.items() if " bad " in k}
    assert len(bad) == 12
    for what, (rc, msg) in bad.items():
        assert rc == ARGUMENT, (what, rc, msg)
        assert what.split("|")[1] in msg and "no HIP device" not in msg, (what, msg)


def test_well_formed_flagged_calls_end_in_no_device(results):
    good = {k: v for k, v in results.items() if k.startswith("edges valid")}
    assert len(good) == 6
    for what, (rc, msg) in good.items():
        if "32768" in what:
            assert rc == ARGUMENT and "degree" in msg, (what, rc, msg)       # the side itself is allowed
        elif results["devices"] == 0:
            assert rc == NO_DEVICE and "no HIP device" in msg, (what, rc, msg)
        else:
            assert rc == OK, (what, rc, msg)


def test_flags_zero_reaches_the_old_entries_refusals(results):
    pairs = results["pairs"]
    assert len(pairs) == 24
    for what, (new, was) in pairs.items():
        assert new == was, (what, new, was)
        if not what.startswith("valid"):
            assert new[0] == ARGUMENT, (what, new)


def test_a_handle_without_a_plane(results):
    assert results["distance null source"][0] == HANDLE
    assert results["has_edges"] == [0, 0]
