"""Pixel VALUE classes for the parity tests: what real images hold and jobs.synth_image (a smooth 0.2 .. 0.8 field,
alpha 1.0) does not - impulses on black, the range of an HDR panorama, signed data with both zeros, denormals, values
near the top of float32, non-finite texels, and an alpha plane around every value the kernels gate on. Everything
comes from 32-bit integer arithmetic (the hash below) and from float32 bit patterns or exactly rounded float64
products, never from libm, so recorded digests do not depend on the numpy version. TEST CODE."""
import numpy as np

from test_gpu_parity import assert_bits        # float32 compared as uint32, 0 ULP: for every finite class

FINITE = ("impulse", "hdr", "signed", "denormal", "big")
CLASSES = FINITE + ("nonfinite",)
M32 = np.uint64(0xFFFFFFFF)
ALPHA_GATE = np.float32(0.000001)        # `a > 0.000001f`: repix_t, eu_synopsis_hdr, the oracle's restatements


def u32(n, seed):
    """n well-mixed uint32 from the element index: jobs.synth_image's LCG step, then two xor-shift-multiply rounds"""
    x = (np.uint64(seed & 0xFFFFFFFF) + (np.arange(n, dtype=np.uint64) + np.uint64(1)) * np.uint64(2654435761)) & M32
    x = (x * np.uint64(1664525) + np.uint64(1013904223)) & M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(2246822519)) & M32
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(3266489917)) & M32
    x ^= x >> np.uint64(16)
    return x.astype(np.uint32)


def unit(u):
    """[0, 1) with 24 bits, float64: exact"""
    return (u >> np.uint32(8)).astype(np.float64) / float(1 << 24)


def from_bits(u):
    return np.ascontiguousarray(u, np.uint32).view(np.float32)


def is_denormal(a):
    b = np.ascontiguousarray(a, np.float32).view(np.uint32)
    return ((b & np.uint32(0x7F800000)) == 0) & ((b & np.uint32(0x007FFFFF)) != 0)


def denormal_share(a):
    return float(is_denormal(a).mean())


def impulse_positions(h, w, seed=1, count=6):
    """`count` texels (y, x), distinct rows and columns where the size allows"""
    u = u32(2 * count, seed + 77)
    return [(int(u[2 * k] % h), int(u[2 * k + 1] % w)) for k in range(count)]


def impulse(h, w, nch, seed=1, lit=None):
    """zeros with a handful of lit texels, every channel 0.5 .. 4. lit: the texels (y, x); default six from the hash.
    A prefilter's poles decay from each through the denormal range before they reach zero."""
    out = np.zeros((h, w, nch), np.float32)
    lit = impulse_positions(h, w, seed) if lit is None else lit
    v = (0.5 + 3.5 * unit(u32(len(lit) * nch, seed + 5))).astype(np.float32).reshape(len(lit), nch)
    for k, (y, x) in enumerate(lit):
        out[y, x] = v[k]
    return out


def hdr(h, w, nch, seed=1):
    """log-uniform over 1e-6 .. 6e4: a uniform binade of 2^-20 .. 2^15 with a uniform mantissa, clipped"""
    u = u32(h * w * nch, seed + 11)
    expo = np.uint32(107) + (u >> np.uint32(23)) % np.uint32(36)
    v = from_bits((expo << np.uint32(23)) | (u & np.uint32(0x007FFFFF)))
    return np.clip(v, np.float32(1e-6), np.float32(6e4)).reshape(h, w, nch)


def signed(h, w, nch, seed=1):
    """about +-1e3, with about 30 % exact +0 and about 10 % -0"""
    n = h * w * nch
    v = ((2.0 * unit(u32(n, seed + 21)) - 1.0) * 1000.0).astype(np.float32)
    k = u32(n, seed + 22) % np.uint32(10)
    v[k < 3] = np.float32(0.0)
    v[k == 3] = np.float32(-0.0)
    return v.reshape(h, w, nch)


def denormal(h, w, nch, seed=1):
    """random denormals of both signs: exponent bits zero, 19 mantissa bits (up to 7.3e-40, a sixteenth of the
    smallest normal float), never zero - a prefilter up to degree 5 amplifies by less than that, so its coefficients
    are denormal too"""
    u = u32(h * w * nch, seed + 31)
    return from_bits((u & np.uint32(0x8007FFFF)) | np.uint32(1)).reshape(h, w, nch).copy()


def big(h, w, nch, seed=1, top=1e37):
    """uniform in +-top, 1e37 unless a case says otherwise. Finite through a prefilter of degree 3 or less (BIG_PREFILTER_MAX): zimt multiplies a line
    by the filter's whole gain before it recurses - 6 per axis at degree 3, 385 at degree 4 - so from degree 4 on
    the reference's own container overflows to inf and NaN and there is nothing to compare. +-1e34 (BIG_TOP_5) is
    finite through degree 5, whose gain is 120 per axis, +-1e32 (BIG_TOP_7) through degree 7 (5036 per axis)"""
    return ((2.0 * unit(u32(h * w * nch, seed + 41)) - 1.0) * top).astype(np.float32).reshape(h, w, nch)


BIG_PREFILTER_MAX = 3
BIG_TOP_5, BIG_TOP_7 = 1e34, 1e32


def ordinary(h, w, nch, seed=1):
    """0.2 .. 0.8 noise, alpha (the last of 2 or 4 channels) 1.0: what the other tests feed"""
    v = (0.2 + 0.6 * unit(u32(h * w * nch, seed + 51))).astype(np.float32).reshape(h, w, nch)
    if nch in (2, 4):
        v[:, :, nch - 1] = 1.0
    return v


NONFINITE_VALUES = np.array([np.inf, -np.inf, np.nan, 3e38, -3e38], np.float32)


def nonfinite(h, w, nch, seed=1, one_in=200):
    """an ordinary image with one texel in `one_in` (0.5 %) set, in all its channels, to +inf, -inf, NaN or +-3e38"""
    v = ordinary(h, w, nch, seed)
    u = u32(h * w, seed + 61).reshape(h, w)
    hit = u % np.uint32(one_in) == 0
    v[hit] = NONFINITE_VALUES[(u[hit] // np.uint32(one_in)) % np.uint32(5)][:, None]
    return v


_MAKE = dict(impulse=impulse, hdr=hdr, signed=signed, denormal=denormal, big=big, nonfinite=nonfinite)


def make(cls, h, w, nch, seed=1, **kw):
    """the value class `cls` as (h, w, nch) float32"""
    return _MAKE[cls](h, w, nch, seed, **kw)


def scaled_unit(cls, h, w, nch, seed=1):
    """a finite class brought into and around [0, 1] - below 0, -0, 0, inside, exactly 1, above 1 - by exact or
    correctly rounded float32 operations; every tenth float is one of the edges themselves"""
    v = make(cls, h, w, nch, seed)
    top = np.float32(np.abs(v).max())
    if cls == "denormal":
        v = (v.astype(np.float64) * 2.0 ** 126).astype(np.float32)          # exact: +-(0, 2)
    elif cls == "hdr":
        v = (v * np.float32(1.0 / 4096.0) - np.float32(0.125)).astype(np.float32)   # -0.125 .. 14.5, most below 1
    else:
        v = (v / (top * np.float32(0.75))).astype(np.float32)              # +-1.33, impulse 0 .. 1.33
    k = u32(v.size, seed + 71).reshape(v.shape) % np.uint32(40)
    for i, e in enumerate((0.0, -0.0, 1.0, np.nextafter(np.float32(1), np.float32(2)))):
        v[k == i] = np.float32(e)
    return v


ALPHA_PALETTE = np.array([
    1.0, 1.0, 0.5, 0.25, 0.75, 0.999, 0.1, 1e-3,
    np.nextafter(ALPHA_GATE, np.float32(0)), ALPHA_GATE, np.nextafter(ALPHA_GATE, np.float32(1)), 2e-6,
    1.4e-45, 1e-40, -1e-40, 1.1754942e-38,
    np.nextafter(np.float32(1), np.float32(2)), 1.25, 2.0, 1.0001,
    -1e-7, -0.01, -1e-6, -0.25], np.float32)


def alpha_plane(h, w, seed=1):
    """an alpha plane around every gate: exact +0 and -0, denormals, 0.000001f and the floats next to it, values in
    (0, 1), 1, values above 1 and small negatives (spline overshoot). Aligned groups of 16 pixels of a row take turns:
    all zero (both signs), partly zero, no zero - so a per-group `all lanes zero` shortcut meets all three."""
    u = u32(h * w, seed + 81).reshape(h, w)
    a = ALPHA_PALETTE[u % np.uint32(len(ALPHA_PALETTE))].copy()
    y, x = np.mgrid[0:h, 0:w]
    kind = (x // 16 + y) % 3                                 # 0: all zero, 1: partly, 2: none
    z = u32(h * w, seed + 82).reshape(h, w)
    zero = (kind == 0) | ((kind == 1) & (z % np.uint32(3) == 0))
    a[zero] = np.where(z[zero] % np.uint32(4) == 1, np.float32(-0.0), np.float32(0.0))
    return a


def group_kinds(alpha, lanes=16):
    """of the aligned groups of `lanes` pixels of every row (the ragged tail left out): how many are all zero, partly
    zero, free of zeros"""
    h, w = alpha.shape
    g = (alpha[:, :w // lanes * lanes] == 0).reshape(h, w // lanes, lanes).sum(2)
    return int((g == lanes).sum()), int(((g > 0) & (g < lanes)).sum()), int((g == 0).sum())


def with_alpha(img, seed=1, associated=False):
    """img with alpha_plane in the last of its 2 or 4 channels (other counts: unchanged); associated: the colour
    channels multiplied by it, as a stitcher's output holds them"""
    nch = img.shape[2]
    if nch in (2, 4):
        a = alpha_plane(img.shape[0], img.shape[1], seed)
        img = img.copy()
        if associated:
            with np.errstate(all="ignore"):
                img[:, :, :nch - 1] = img[:, :, :nch - 1] * a[:, :, None]
        img[:, :, nch - 1] = a
    return img


def nan_mask(a):
    return np.isnan(np.ascontiguousarray(a, np.float32))


def assert_bits_nan(got, ref, what=""):
    """for data with non-finite values: equal shapes, equal NaN masks, and everything that is not NaN equal as uint32
    (the signs of zero and of inf count). Which bits a NaN carries is not compared: the reference's own zimt and its
    restatement do not always agree on them."""
    got, ref = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(ref, np.float32)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    ng, nr = np.isnan(got), np.isnan(ref)
    bad = np.argwhere(ng != nr)
    if bad.size:
        i = tuple(bad[0])
        raise AssertionError(f"{what}: the NaN masks differ at {len(bad)} of {got.size} floats; first at {i}: got "
                             f"{got[i]!r} expected {ref[i]!r}")
    bad = np.argwhere((got.view(np.uint32) != ref.view(np.uint32)) & ~nr)
    if bad.size:
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {got.size} floats that are not NaN differ; first at {i}: got "
                             f"{got[i]!r} ({got.view(np.uint32)[i]:#010x}) expected {ref[i]!r} "
                             f"({ref.view(np.uint32)[i]:#010x})")


def assert_class_bits(cls, got, ref, what=""):
    (assert_bits_nan if cls == "nonfinite" else assert_bits)(got, ref, what)


def assert_exercised(cls, frame, degree, what="", some=False):
    """conditions on the ORACLE's frame (or container): the case did meet its value class. Not a measurement of the
    code under test. some: the substitute for frames whose colours were multiplied by an alpha plane of many zeros,
    composed from several facets or left black where a source misses - the shares of 5 %, 90 % and one half cannot
    hold there, so the frame must hold denormals at all (`impulse` from degree 2 on, `denormal`), a NaN and an inf
    (`nonfinite`)"""
    f = np.ascontiguousarray(frame, np.float32)
    if some:
        if cls == "denormal" or cls == "impulse" and degree >= 2:
            assert is_denormal(f).any(), f"{what}: no denormal"
        elif cls == "nonfinite":
            assert np.isnan(f).any() and np.isinf(f).any(), f"{what}: NaN {np.isnan(f).sum()}, inf {np.isinf(f).sum()}"
    elif cls == "impulse" and degree >= 2:
        assert denormal_share(f) >= 0.05, f"{what}: only {denormal_share(f):.3f} of the floats are denormal"
    elif cls == "denormal":
        assert denormal_share(f) >= 0.90, f"{what}: only {denormal_share(f):.3f} of the floats are denormal"
    elif cls == "nonfinite":
        assert np.isnan(f).any(), f"{what}: no NaN"
        assert np.isinf(f).any(), f"{what}: no inf"
        assert (~np.isfinite(f)).mean() <= 0.5, f"{what}: {(~np.isfinite(f)).mean():.2f} of the floats are not finite"


def block_edge_alignments(container, block=64):
    """along rows and along columns: at how many of the `block` possible alignments of a line's blocks do denormal
    coefficients lie on both sides of an edge between two blocks - where the streamed prefilter hands over from one
    block of samples to the next, and keeps its checkpoint"""
    d = is_denormal(container).any(axis=2)
    counts = []
    for m in (d, d.T):
        n = 0
        for o in range(block):
            left, right = m[:, o + block - 1::block], m[:, o + block::block]
            n += bool((left[:, :right.shape[1]] & right).any())
        counts.append(n)
    return tuple(counts)
