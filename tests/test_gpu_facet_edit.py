"""PTO exclude masks and lens crops applied on the device (envutil_amd/csrc/eu_alpha.hip) when a facet loads:
eu_hip_facet_alpha_dev against the oracle's plane (euo.facet_alpha, pinned to zimt's convolve by
tests/golden/alpha_golden.npz), eu_hip_source_load_edited against eu_hip_source_load from pixels edited by the
library's HOST function, and the same through a multi-facet render and through hip_dispatch::payload.
Everything bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import envutil_amd as ea
import euo
from envutil_amd import api
from test_facet_alpha_rows import SHAPES, shape_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "envutil_amd", "build", "dispatch_masked_demo")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def device_tensor(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


# ------------------------------------------------------------------------------ eu_hip_facet_alpha_dev

@pytest.mark.parametrize("nch", [2, 4])
@pytest.mark.parametrize("w,h", SHAPES)
def test_alpha_dev_is_the_oracles(w, h, nch):
    for kind in range(3):
        polys, crop = shape_case(w, h, kind)
        want = euo.facet_alpha(w, h, polys, crop, kind)
        rng = np.random.default_rng(w * 1000 + h)
        px0 = rng.random((h, w, nch), dtype=np.float32)
        px = px0.copy()
        plane = ea.facet_alpha_dev(px, polys, crop, kind)
        assert same(plane, want), (w, h, nch, kind, int((bits(plane) != bits(want)).sum()))
        assert same(px, px0 * want[:, :, None]), (w, h, nch, kind)
        # the plane alone: no pixels given, none touched
        only = ea.facet_alpha_dev(None, polys, crop, kind, shape=(h, w), nchannels=nch)
        assert same(only, want), (w, h, nch, kind)


@pytest.mark.parametrize("nch", [2, 4])
def test_alpha_dev_in_place_on_a_tensor_aligned_or_not(nch):
    """a torch tensor is edited where it lies; one float off a 16-byte boundary the kernel takes its narrow
    accesses and gives the same bits; without want_alpha no plane is made"""
    import torch
    w, h = 127, 33
    polys, crop = shape_case(w, h, 2)
    want = euo.facet_alpha(w, h, polys, crop, 2)
    px0 = np.random.default_rng(5).random((h, w, nch), dtype=np.float32)
    for off in (0, 1):
        flat = torch.zeros(h * w * nch + 8, dtype=torch.float32, device="cuda:0")
        t = flat[off:off + h * w * nch].view(h, w, nch)
        t.copy_(torch.from_numpy(px0))
        assert ea.facet_alpha_dev(t, polys, crop, 2, want_alpha=False) is None
        assert same(t.cpu().numpy(), px0 * want[:, :, None]), (nch, off)
        rest = flat.cpu().numpy()
        assert (rest[:off] == 0).all() and (rest[off + h * w * nch:] == 0).all()


@pytest.mark.parametrize("w,h,kind,nch", [(4096, 3072, 2, 4), (6000, 4000, 1, 2)])
def test_alpha_dev_fullsize(w, h, kind, nch):
    polys, crop = shape_case(w, h, kind, 3)
    want = euo.facet_alpha(w, h, polys, crop, kind)
    assert (want == 0).any() and (want == 1).any() and ((want > 0) & (want < 1)).any()
    px0 = np.random.default_rng(11).random((h, w, nch), dtype=np.float32)
    px = px0.copy()
    plane = ea.facet_alpha_dev(px, polys, crop, kind)
    assert same(plane, want)
    px0 *= want[:, :, None]
    assert same(px, px0)


# ------------------------------------------------------------------------------ eu_hip_source_load_edited

def host_prepared(pixels, nch, masks, crop, kind):
    """the parent's route: widen with ones, then the library's HOST function"""
    p = np.array(pixels, np.float32)           # a copy: the host function edits in place
    if p.ndim == 2:
        p = p[:, :, None]
    if p.shape[2] == nch - 1:
        p = np.concatenate([p, np.ones(p.shape[:2] + (1,), np.float32)], 2)
    p = np.ascontiguousarray(p)
    ea.facet_alpha(p, masks, crop, kind)
    return p


def facet_cases(nch):
    """(name, facet, plane width, plane height, crop kind)"""
    return [
        ("rectilinear", ea.facet_spec(ea.RECTILINEAR, 200, 150, 70.0, nchannels=nch, yaw=10, pitch=5, roll=2), 200, 150, 1),
        ("fisheye", ea.facet_spec(ea.FISHEYE, 160, 160, 170.0, nchannels=nch, yaw=-100, pitch=-20), 160, 160, 2),
        ("fullsphere", ea.facet_spec(ea.SPHERICAL, 256, 128, 360.0, nchannels=nch), 256, 128, 1),
        ("windowed", ea.facet_spec(ea.RECTILINEAR, 300, 200, 80.0, nchannels=nch, window=(131, 77, 40, 30)), 131, 77, 1),
        ("cubemap", ea.facet_spec(ea.CUBEMAP, 64, 384, 90.0, nchannels=nch), 64, 384, 1),
    ]


@pytest.mark.parametrize("degree", [0, 1, 3])
@pytest.mark.parametrize("which", range(5))
def test_load_edited_is_the_load_of_host_edited_pixels(which, degree):
    k = 0
    for nch in (4, 2):
        name, fct, w, h, kind = facet_cases(nch)[which]
        polys, crop = shape_case(w, h, kind, 2)
        for pch in (nch, nch - 1):
            rng = np.random.default_rng(100 * which + 10 * nch + pch)
            px = rng.random((h, w, pch), dtype=np.float32)
            if pch == nch:
                px[..., -1] = (rng.random((h, w)) > 0.2)      # an alpha channel of its own
            want = ea.Source.load(fct, host_prepared(px, nch, polys, crop, kind), degree).download()
            for on_device in (False, True):
                src = ea.Source.load(fct, device_tensor(px) if on_device else px, degree, masks=polys, crop=crop,
                                     crop_kind=kind)
                got = src.download()
                assert same(got, want), (name, degree, nch, pch, on_device, int((bits(got) != bits(want)).sum()))
                k += 1
    assert k == 8


def test_an_edit_that_edits_nothing_is_the_plain_load():
    L = ea.lib()
    for name, fct, w, h, kind in facet_cases(4):
        px = np.random.default_rng(3).random((h, w, 4), dtype=np.float32)
        want = ea.Source.load(fct, px, 3).download()
        # no edit at all, an empty edit, an empty edit of pixels on the device
        cf = fct.c_struct()
        for e, ptr in [(None, px.ctypes.data), (api.FacetEdit(pixel_channels=4), px.ctypes.data)]:
            hnd = C.c_void_p()
            rc = L.eu_hip_source_load_edited(C.byref(cf), C.c_void_p(ptr), C.byref(e) if e is not None else None,
                                             3, 3, 8, 64, C.byref(hnd))
            assert rc == 0, L.eu_hip_last_error()
            assert same(ea.Source(hnd, fct).download(), want), name
        assert same(ea.Source.load(fct, device_tensor(px), 3).download(), want), name
        # a crop that keeps everything, a polygon that lies outside: the plane is 1, the pixels are their own
        got = ea.Source.load(fct, px, 3, crop=(0, w, 0, h), crop_kind=1,
                             masks=[(np.array([-9, -2, -5], np.float32), np.array([-9, -9, -1], np.float32))]).download()
        assert same(got, want), name


def test_multi_facet_render_from_device_edited_sources():
    """the two facets of tests/test_cli.py::test_pto_with_mask_and_crop, degree 3, 4 channels"""
    from test_cli import synth
    a, b = synth(200, 150, 3, 1), synth(160, 160, 3, 2)
    mask = [(np.array([30, 120, 140, 40], np.float32), np.array([20, 25, 110, 100], np.float32))]
    fa = ea.facet_spec(ea.RECTILINEAR, 200, 150, 70.0, nchannels=4, yaw=10, pitch=5, roll=2)
    fb = ea.facet_spec(ea.FISHEYE, 160, 160, 170.0, nchannels=4, yaw=-100, pitch=-20, roll=0)
    args = ea.arguments(ea.SPHERICAL, 300, 150, 360.0, spline_degree=3)
    ha = ea.Source.load(fa, host_prepared(a, 4, mask, None, 0), 3)
    hb = ea.Source.load(fb, host_prepared(b, 4, [], (10, 150, 10, 150), 2), 3)
    want = ea.render(args, [ha, hb], 4)
    da = ea.Source.load(fa, a, 3, masks=mask)
    db = ea.Source.load(fb, device_tensor(b), 3, crop=(10, 150, 10, 150), crop_kind=2)
    got = ea.render(args, [da, db], 4)
    assert same(got, want)
    assert (got[..., 3] == 0).any() and (got[..., 3] == 1).any()


# ------------------------------------------------------------------------------ hip_dispatch::payload

def build_demo():
    if not os.path.exists(ea.lib_path()):
        ea.build()
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "csrc", "dispatch_masked_demo.cc"), "-o", EXE,
                           "-L" + os.path.join(ROOT, "envutil_amd", "lib"), "-leu_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "envutil_amd", "lib")])


def test_dispatch_loads_a_masked_facet_itself():
    """facets with has_pto_mask / has_lens_crop and pixels_prepared == false render through
    get_dispatch()->payload() (EU_ERR_UNSUPPORTED before), to the bits of the render from pixels prepared by
    prepare_facet_pixels; each run is a process of its own under its own time limit, the second only after the first"""
    build_demo()
    runs = []
    for argv in ([EXE], [EXE, "host"]):
        r = subprocess.run(["timeout", "-k", "10", "120"] + argv, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "rc 0" in r.stdout
        runs.append(r.stdout)
    assert runs[0].split("fnv1a")[1].strip() == runs[1].split("fnv1a")[1].strip(), runs
    clear, opaque = (int(v) for v in runs[0].split("alpha clear")[1].split("fnv1a")[0].replace("opaque", "").split())
    assert clear > 0 and opaque > 0
