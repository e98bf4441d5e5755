"""The Radiance RGBE pixel format as a numpy float32 model, written from the format's definition and not from the
library's functions: what the RGBE tests expect. tests/test_rgbe_host.py holds it against include/eu_rgbe.h on the
CPU. TEST CODE.

decode: channel = mantissa * 2^(E - 136), E == 0 -> 0 in all three channels.
encode: v = the largest channel by two ordered compares (a NaN channel loses them); !(v >= 1e-32f) -> four zero
bytes; every channel clamped from above to 255 * 2^119; with frexp(v) = (mant, e) the factor is 2^(8 - e), a channel
that fails `> 0` has mantissa 0, the others trunc(channel * factor), and E = e + 128."""
import numpy as np

TOP = np.float32(255.0 * 2.0 ** 119)
TINY = np.float32(1e-32)


def decode(quads):
    """(..., 4) uint8 -> (..., 3) float32"""
    q = np.asarray(quads, np.uint8)
    e = q[..., 3].astype(np.int32)
    # float64 holds mantissa * 2^(E - 136) exactly, and so does float32 (denormals included): the cast is exact
    scale = np.where(e == 0, 0.0, np.ldexp(1.0, e - 136))
    return np.ascontiguousarray((q[..., :3].astype(np.float64) * scale[..., None]).astype(np.float32))


def encode(frame):
    """(..., 3) float32 -> (..., 4) uint8"""
    f = np.ascontiguousarray(frame, np.float32)
    r, g, b = f[..., 0], f[..., 1], f[..., 2]
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.where(r > g, r, g)
        v = np.where(b > v, b, v)
        some = v >= TINY                                           # False for NaN and negatives
        v = np.where(some, np.minimum(v, TOP), np.float32(1.0)).astype(np.float32)
        mant, e = np.frexp(v)
        out = np.zeros(f.shape[:-1] + (4,), np.uint8)
        for c in range(3):
            ch = f[..., c]
            ch = np.where(ch > TOP, TOP, ch)                       # NaN stays, and fails the next test
            # channel * 2^(8 - e) in float64: exact, so its truncation is the float32 product's
            m = np.where(ch > 0, np.ldexp(ch.astype(np.float64), 8 - e), 0.0)
            out[..., c] = np.where(some, np.trunc(m), 0).astype(np.int64).astype(np.uint8)
        out[..., 3] = np.where(some, e + 128, 0).astype(np.uint8)
    return out


def bits(v):
    return np.ascontiguousarray(v, np.float32).view(np.uint32)


def from_bits(u):
    return np.ascontiguousarray(u, np.uint32).view(np.float32)


def _b(v):
    """the bit pattern of one float32, as an int"""
    return int(np.float32(v).view(np.uint32))


def _f(u):
    """the float32 of one bit pattern"""
    return np.uint32(u).view(np.float32)


def targeted():
    """(n, 3) float32: every binade from 1e-32f's up to the top with random mantissas, the largest channel in each
    position, ties, negative, zero (both signs), NaN and denormal channels in each position, 1e-32f and its
    neighbours, and the values at and above 2^127"""
    rng = np.random.default_rng(5)
    px = []
    e_lo = _b(TINY) >> 23
    specials = np.array([-1.0, -0.0, 0.0, np.nan, -np.inf, -1e-40, 1e-40], np.float32)
    for e in range(e_lo, 254):
        for _ in range(4):
            v = _f((e << 23) | int(rng.integers(0, 1 << 23)))
            frac = np.float32(v * np.float32(rng.random()))
            lower = _f(int(rng.integers(0, _b(v) + 1)))
            others = [frac, lower, v, np.float32(0.5) * v, _f(_b(v) - 1)]
            a, b = others[rng.integers(0, 5)], others[rng.integers(0, 5)]
            px += [(v, a, b), (a, v, b), (a, b, v)]
            s = specials[rng.integers(0, len(specials))]
            px += [(s, v, a), (v, s, a), (v, a, s), (s, s, v), (s, v, s), (v, s, s)]
    for s in specials:
        for t in specials:
            px += [(s, t, s), (t, s, s), (s, s, t)]
    for d in (-1, 0, 1):
        v = _f(_b(TINY) + d)
        px += [(v, 0.0, 0.0), (np.float32(0.5) * v, v, -v), (np.nan, 0.0, v), (v, v, v)]
    tops = [np.float32(2.0 ** 127), np.finfo(np.float32).max, np.float32(np.inf), TOP,
            _f(_b(TOP) + 1), np.float32(3e38), np.float32(254.0 * 2.0 ** 119)]
    others = [0.0, -1.0, np.nan, 1.0, np.float32(0.5) * TOP, np.float32(2.0 ** 126), TOP, np.finfo(np.float32).max, np.inf]
    for v in tops:
        for a in others:
            for b in others:
                px += [(v, a, b), (a, v, b), (a, b, v)]
    return np.array(px, np.float32)
