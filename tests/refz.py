"""ctypes bindings of oracle/_ref/libref_zimt.so - the reference's own zimt
headers compiled in place from a reference checkout (oracle/Makefile, REF). Only
present where that checkout is; tests marked 'ref' compare with it live there, and
elsewhere with the SHA-256 of its results recorded in tests/golden/ref_digests.json and,
for the steppers, tests/golden/stepper_digests.json, for the pixel value classes (tests/pixel_values.py)
tests/golden/pixel_value_digests.json (same())."""
import ctypes as C
import hashlib
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "oracle", "_ref", "libref_zimt.so")
DIGESTS = os.path.join(ROOT, "tests", "golden", "ref_digests.json")
# the digests of the steppers' results (keys "stepper_...", tests/test_stepper_pinned.py) have a file of their own
STEPPER_DIGESTS = os.path.join(ROOT, "tests", "golden", "stepper_digests.json")
# ... and those of the pixel value classes (keys "pixval_...", tests/test_oracle_pixel_values.py)
PIXEL_DIGESTS = os.path.join(ROOT, "tests", "golden", "pixel_value_digests.json")
RECORDING = False       # tests/golden/make_ref_digests.py: collect into RECORDED, skip the check against DIGESTS
RECORDED = {}


def available(symbol=None):
    """the library is built - and, when a symbol is named, exports it (a library built from an earlier
    oracle/ref_zimt.cc does not have the steppers)"""
    return os.path.exists(LIB) and (symbol is None or hasattr(lib(), symbol))


def digest(a):
    """SHA-256 of an array's float32 bits and shape"""
    a = np.ascontiguousarray(a, np.float32)
    return hashlib.sha256(repr(a.shape).encode() + a.tobytes()).hexdigest()


_digests = None


def one_nan(a):
    """a float32 copy in which every NaN is the one pattern 0x7fc00000"""
    a = np.array(a, np.float32, order="C")
    a.view(np.uint32)[np.isnan(a)] = 0x7FC00000
    return a


def same(key, ours, reference, symbol=None, any_nan=False):
    """True when `ours` is bit for bit the reference's result: `reference()` (a call into the library) where
    the library is built (and exports `symbol`, if one is named) - and then its digest must be the one recorded
    under `key` - else the recorded digest. any_nan (data with non-finite values only): every NaN of both sides
    becomes one pattern first - where the NaNs are is compared and digested, which bits they carry is not"""
    global _digests
    if _digests is None:
        _digests = {}
        for path in (DIGESTS, STEPPER_DIGESTS, PIXEL_DIGESTS):
            if os.path.exists(path):
                _digests.update(json.load(open(path)))
    if any_nan:
        ours = one_nan(ours)
    if not available(symbol):
        return digest(ours) == _digests[key]
    ref = np.ascontiguousarray(reference(), np.float32)
    if any_nan:
        ref = one_nan(ref)
    RECORDED[key] = digest(ref)
    assert RECORDING or _digests.get(key) == RECORDED[key], f"the digest recorded under tests/golden for {key} is stale"
    ours = np.ascontiguousarray(ours, np.float32)
    return ours.shape == ref.shape and (ours.view(np.uint32) == ref.view(np.uint32)).all()


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(LIB)
        _lib.ref_bspline_new.restype = C.c_void_p
        _lib.ref_bspline_new.argtypes = [C.c_void_p, C.c_long, C.c_long, C.c_int,
                                         C.c_int, C.c_int, C.c_int]
        for n in ("free", "prefilter", "spherical", "brace", "geometry",
                  "container", "eval", "process_affine"):
            getattr(_lib, "ref_bspline_" + n).restype = None
        _lib.ref_bspline_free.argtypes = [C.c_void_p]
        _lib.ref_bspline_prefilter.argtypes = [C.c_void_p, C.c_int]
        _lib.ref_bspline_spherical.argtypes = [C.c_void_p, C.c_int]
        _lib.ref_bspline_brace.argtypes = [C.c_void_p, C.c_int]
        _lib.ref_bspline_geometry.argtypes = [C.c_void_p, C.c_void_p]
        _lib.ref_bspline_container.argtypes = [C.c_void_p, C.c_void_p]
        _lib.ref_bspline_eval.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p]
        _lib.ref_bspline_process_affine.argtypes = [C.c_void_p, C.c_long, C.c_long,
                                                    C.c_void_p, C.c_void_p]
        _lib.ref_basis_weights.argtypes = [C.c_int, C.c_float, C.c_void_p]
        _lib.ref_filter_2d.argtypes = [C.c_void_p, C.c_long, C.c_long, C.c_int,
                                       C.c_int, C.c_int, C.c_int]
    return _lib


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class RefSpline:
    def __init__(self, core, degree, bc0, bc1):
        core = np.ascontiguousarray(core, np.float32)
        h, w, nch = core.shape
        self.h_ = lib().ref_bspline_new(ptr(core), w, h, nch, degree, bc0, bc1)
        self.nch = nch

    def __del__(self):
        if getattr(self, "h_", None):
            lib().ref_bspline_free(self.h_)
            self.h_ = None

    def geometry(self):
        g = (C.c_long * 10)()
        lib().ref_bspline_geometry(self.h_, g)
        return list(g)

    def prefilter(self, degree):
        lib().ref_bspline_prefilter(self.h_, degree)

    def spherical(self, degree):
        lib().ref_bspline_spherical(self.h_, degree)

    def brace(self, axis=-1):
        lib().ref_bspline_brace(self.h_, axis)

    def container(self):
        g = self.geometry()
        out = np.zeros((g[1], g[0], self.nch), np.float32)
        lib().ref_bspline_container(self.h_, ptr(out))
        return out

    def eval(self, crd):
        crd = np.ascontiguousarray(crd, np.float32)
        out = np.zeros((crd.shape[0], self.nch), np.float32)
        lib().ref_bspline_eval(self.h_, ptr(crd), crd.shape[0], ptr(out))
        return out

    def process_affine(self, w, h, aff):
        aff = np.asarray(aff, np.float32)
        out = np.zeros((h, w, self.nch), np.float32)
        lib().ref_bspline_process_affine(self.h_, w, h, ptr(aff), ptr(out))
        return out


def basis_weights(degree, delta):
    w = np.zeros(degree + 1, np.float32)
    lib().ref_basis_weights(degree, delta, ptr(w))
    return w


def poles(degree):
    p = np.zeros(max(degree // 2, 1), np.longdouble)
    lib().ref_poles(degree, ptr(p))
    return p[:degree // 2]


def filter_2d(img, degree, bc0, bc1):
    """zimt::prefilter of a plain 2-D array (no frame), both axes, in place copy"""
    a = np.ascontiguousarray(img, np.float32).copy()
    h, w, nch = a.shape
    lib().ref_filter_2d(ptr(a), w, h, nch, degree, bc0, bc1)
    return a


def lut_eval(knots, vin):
    """lut_based_tf's zimt calls (envutil_payload.cc:251-287) on `knots`"""
    knots = np.ascontiguousarray(knots, np.float32)
    vin = np.ascontiguousarray(vin, np.float32)
    out = np.zeros_like(vin)
    f = lib().ref_lut_eval
    f.restype = None
    f.argtypes = [C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_void_p]
    f(knots.ctypes.data, len(knots), vin.ctypes.data, len(vin), out.ctypes.data)
    return out


def lcp_factor(a, b, c, x):
    """project::lcp<float, 16>(a, b, c).eval on 16-lane vectors (lens_correction.h:224-235)"""
    x = np.ascontiguousarray(x, np.float32)
    out = np.zeros_like(x)
    f = lib().ref_lcp_factor
    f.restype = None
    f.argtypes = [C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_long, C.c_void_p]
    f(a, b, c, x.ctypes.data, len(x), out.ctypes.data)
    return out


def inverse_lcp(a, b, c, r_max, sz, x):
    """project::inverse_lcp<float, 16>(a, b, c, r_max, sz).eval (lens_correction.h:236-301) and the
    prefiltered core of its spline model. NB the reference asserts when Newton's iteration does not
    find an inverse (strong coefficients at a large r_max): keep the sets mild"""
    x = np.ascontiguousarray(x, np.float32)
    out = np.zeros_like(x)
    knots = np.zeros(sz + 4, np.float32)
    f = lib().ref_inverse_lcp
    f.restype = None
    f.argtypes = [C.c_double] * 4 + [C.c_int, C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.c_int]
    f(a, b, c, r_max, sz, x.ctypes.data, len(x), out.ctypes.data, knots.ctypes.data, len(knots))
    return out, knots


def binomial_alpha(plane):
    """zimt::convolve(alpha, alpha, {REFLECT, REFLECT}, {1, 4, 6, 4, 1} / 16, 2): the call of
    environment.h:833-843 on a (h, w) float plane"""
    out = np.ascontiguousarray(plane, np.float32).copy()
    f = lib().ref_binomial_alpha
    f.restype = None
    f.argtypes = [C.c_void_p, C.c_long, C.c_long]
    f(out.ctypes.data, out.shape[1], out.shape[0])
    return out


def masking(nch, paint, n):
    """masking_t<2, nch, 16> (masking.h:74-93) on n pixels"""
    out = np.full((n, nch), np.nan, np.float32)
    f = lib().ref_masking
    f.restype = None
    f.argtypes = [C.c_int, C.c_float, C.c_long, C.c_void_p]
    f(nch, paint, n, ptr(out))
    return out


def alpha_masking(spline, paint, crd):
    """alpha_masking_t<nch, 16> (masking.h:95-135) over a RefSpline of 2 or 4 channels at spline coordinates crd"""
    crd = np.ascontiguousarray(crd, np.float32)
    out = np.zeros((crd.shape[0], spline.nch), np.float32)
    f = lib().ref_alpha_masking
    f.restype = None
    f.argtypes = [C.c_void_p, C.c_float, C.c_void_p, C.c_long, C.c_void_p]
    f(spline.h_, paint, ptr(crd), crd.shape[0], ptr(out))
    return out


def _basis(basis):
    return np.ascontiguousarray(basis, np.float64).reshape(9)


_STEPPER_TAIL = [C.c_long] * 4 + [C.c_void_p]      # off_x, off_y, out_w, out_h, out


def stepper_rays(kind, normalize, w, h, extent, basis, bias=(0.0, 0.0), offset=(0, 0), out_shape=None):
    """S<float, 16, normalize>(xx, yy, zz, w, h, extent..., bias_x, bias_y) through zimt::process with
    bill.get_offset = offset, over out_shape = (width, height) (default: the whole w x h): (rows, width, 3).
    kind: projection_t's number. basis: 3 x 3 doubles, rows xx, yy, zz - an input, not pinned (Imath)"""
    ow, oh = out_shape or (w, h)
    out = np.full((oh, ow, 3), np.nan, np.float32)
    b = _basis(basis)
    f = lib().ref_stepper_rays
    f.restype = C.c_int
    f.argtypes = [C.c_int] * 4 + [C.c_double] * 4 + [C.c_void_p, C.c_float, C.c_float] + _STEPPER_TAIL
    rc = f(kind, int(normalize), w, h, *(float(v) for v in extent), ptr(b), bias[0], bias[1], offset[0], offset[1],
           ow, oh, ptr(out))
    assert rc == 0, rc
    return out


def deriv_rays(kind, w, h, extent, basis, bias=0.25, offset=(0, 0), out_shape=None):
    """deriv_stepper<float, 16, S>(xx, yy, zz, w, h, extent..., bias): the ninepacks r00, r10, r01, (rows, width, 9)"""
    ow, oh = out_shape or (w, h)
    out = np.full((oh, ow, 9), np.nan, np.float32)
    b = _basis(basis)
    f = lib().ref_deriv_rays
    f.restype = C.c_int
    f.argtypes = [C.c_int] * 3 + [C.c_double] * 4 + [C.c_void_p, C.c_float] + _STEPPER_TAIL
    rc = f(kind, w, h, *(float(v) for v in extent), ptr(b), bias, offset[0], offset[1], ow, oh, ptr(out))
    assert rc == 0, rc
    return out


def planar(w, h, extent, bias=(0.0, 0.0), offset=(0, 0), out_shape=None):
    """planar_stepper<float, 16>(w, h, extent..., bias_x, bias_y): (rows, width, 2)"""
    ow, oh = out_shape or (w, h)
    out = np.full((oh, ow, 2), np.nan, np.float32)
    f = lib().ref_planar
    f.restype = C.c_int
    f.argtypes = [C.c_int] * 2 + [C.c_double] * 4 + [C.c_float, C.c_float] + _STEPPER_TAIL
    rc = f(w, h, *(float(v) for v in extent), bias[0], bias[1], offset[0], offset[1], ow, oh, ptr(out))
    assert rc == 0, rc
    return out


def generic_rays(normalize, w, h, extent, bias=(0.0, 0.0), offset=(0, 0), out_shape=None):
    """generic_stepper<float, 16, normalize> over the harness's own functor (x, y) -> (x, y, 1): (rows, width, 3)"""
    ow, oh = out_shape or (w, h)
    out = np.full((oh, ow, 3), np.nan, np.float32)
    f = lib().ref_generic_rays
    f.restype = C.c_int
    f.argtypes = [C.c_int] * 3 + [C.c_double] * 4 + [C.c_float, C.c_float] + _STEPPER_TAIL
    rc = f(int(normalize), w, h, *(float(v) for v in extent), bias[0], bias[1], offset[0], offset[1], ow, oh, ptr(out))
    assert rc == 0, rc
    return out
