"""A numpy float32 model of the Y'CbCr way out, written from its formulas - not from include/eu_ycbcr.h and not through
the library. Every product and every sum is a separate float32 operation; codes come from counting compares.
Shared by the host and the device tests, which compare the library's WHOLE destination buffers with it, byte for byte.

    Y = (k_r * R + k_g * G) + k_b * B        U = (B - Y) * c_u        V = (R - Y) * c_v

Chroma sample (i, j) is the box mean of the pixels (min(sub_x i + a, w - 1), min(sub_y j + b, h - 1)):
    2 x 2: ((U00 + U10) + (U01 + U11)) * 0.25     2 x 1: (U00 + U10) * 0.5     1 x 2: (U00 + U01) * 0.5     1 x 1: U
(first index x). code(v) = the number of k in 1 .. m with v >= steps[k]; a NaN is code 0. The stored sample is the
low `bits` bits of code << shift.
"""
import numpy as np

FILL = 0xA5
F = np.float32


def yuv(frame, forward):
    """(Y, U, V) planes of an (h, w, >= 3) float32 frame"""
    k_r, k_g, k_b, c_u, c_v = (F(v) for v in forward)
    R, G, B = (np.ascontiguousarray(frame[..., c], F) for c in range(3))
    with np.errstate(all="ignore"):
        yr = k_r * R
        yg = k_g * G
        yb = k_b * B
        yrg = yr + yg
        Y = yrg + yb
        bu = B - Y
        rv = R - Y
        U = bu * c_u
        V = rv * c_v
    for a in (yr, yg, yb, yrg, Y, bu, rv, U, V):
        assert a.dtype == np.float32
    return Y, U, V


def box(P, sub_x, sub_y):
    """the box mean of a plane with its edge replicated"""
    h, w = P.shape
    ch, cw = (h + sub_y - 1) // sub_y, (w + sub_x - 1) // sub_x
    xs = [np.minimum(sub_x * np.arange(cw) + a, w - 1) for a in range(sub_x)]
    ys = [np.minimum(sub_y * np.arange(ch) + b, h - 1) for b in range(sub_y)]
    p = lambda a, b: P[np.ix_(ys[b], xs[a])]                                # noqa: E731
    with np.errstate(all="ignore"):
        if sub_x == 2 and sub_y == 2:
            top = p(0, 0) + p(1, 0)
            bot = p(0, 1) + p(1, 1)
            s = top + bot
            out = s * F(0.25)
        elif sub_x == 2:
            s = p(0, 0) + p(1, 0)
            out = s * F(0.5)
        elif sub_y == 2:
            s = p(0, 0) + p(0, 1)
            out = s * F(0.5)
        else:
            out = p(0, 0)
    assert out.dtype == np.float32
    return out


def codes(v, steps, bits, shift):
    """samples of the floats v: counting compares over steps[1 .. m], NaN is code 0"""
    n = 1 << bits
    tail = np.isnan(steps[1:])
    m = int(np.argmax(tail)) if tail.any() else n - 1                    # steps[1 .. m] are numbers
    c = np.searchsorted(steps[1:m + 1], v, side="right")
    c = np.where(np.isnan(v), 0, c).astype(np.uint32)
    dt = np.uint8 if bits == 8 else np.uint16
    return ((c << np.uint32(shift)) & np.uint32(n - 1)).astype(dt)


def planes(frame, forward, sub_x, sub_y, bits, shift, y_steps, c_steps):
    """(y, cb, cr): dense sample planes"""
    Y, U, V = yuv(frame, forward)
    return (codes(Y, y_steps, bits, shift), codes(box(U, sub_x, sub_y), c_steps, bits, shift),
            codes(box(V, sub_x, sub_y), c_steps, bits, shift))


class Layout:
    """Padded destination buffers of a w x h frame: a luma buffer and a chroma buffer of FILL bytes with `guard` bytes
    in front of and behind every plane, rows `pad` bytes longer than their samples, the luma plane starting `y_off`
    and the chroma planes `c_off` bytes behind a 16-byte boundary of their buffer. layout: 'planar', 'nv12', 'nv21'."""

    def __init__(self, w, h, sub_x, sub_y, bits, layout, y_off=0, c_off=0, pad=0, guard=32):
        sb = bits // 8
        self.w, self.h, self.sub_x, self.sub_y, self.bits, self.layout, self.sb = w, h, sub_x, sub_y, bits, layout, sb
        self.cw, self.ch = (w + sub_x - 1) // sub_x, (h + sub_y - 1) // sub_y
        self.c_step = 1 if layout == "planar" else 2
        assert guard % 16 == 0 and pad % sb == 0 and y_off % sb == 0 and c_off % sb == 0
        self.y_pitch = w * sb + pad
        self.c_pitch = self.cw * sb * self.c_step + pad
        self.y_at = guard + y_off
        self.y_bytes = self.y_at + h * self.y_pitch + guard
        plane = self.ch * self.c_pitch
        if layout == "planar":
            self.cb_at = guard + c_off
            # the second plane at an address of the same class modulo 4 plus an odd number of samples
            self.cr_at = (self.cb_at + plane + guard + 15) // 16 * 16 + c_off + sb * (1 if pad else 0)
            self.c_bytes = self.cr_at + plane + guard
        else:
            first = guard + c_off
            self.cb_at, self.cr_at = (first, first + sb) if layout == "nv12" else (first + sb, first)
            self.c_bytes = first + plane + guard

    def buffers(self):
        return np.full(self.y_bytes, FILL, np.uint8), np.full(self.c_bytes, FILL, np.uint8)

    def fill(self, ybuf, cbuf, y, cb, cr):
        """the planes' samples into the buffers, every other byte as it was"""
        dt = np.uint8 if self.bits == 8 else np.uint16
        for buf, at, pitch, step, p in ((ybuf, self.y_at, self.y_pitch, 1, y), (cbuf, self.cb_at, self.c_pitch, self.c_step, cb),
                                        (cbuf, self.cr_at, self.c_pitch, self.c_step, cr)):
            raw = np.ascontiguousarray(p, dt).view(np.uint8).reshape(p.shape[0], p.shape[1], self.sb)
            for j in range(p.shape[0]):
                row = buf[at + j * pitch: at + j * pitch + ((p.shape[1] - 1) * step + 1) * self.sb]
                for b in range(self.sb):
                    row[b::step * self.sb] = raw[j, :, b]
        return ybuf, cbuf

    def expected(self, frame, forward, shift, y_steps, c_steps):
        y, cb, cr = planes(frame, forward, self.sub_x, self.sub_y, self.bits, shift, y_steps, c_steps)
        return self.fill(*self.buffers(), y, cb, cr)


def random_steps(rng, bits, lo=-0.2, hi=1.2, top=None, ties=0):
    """a valid step table that is no formula: sorted random floats in steps[1 .. top], `ties` runs of equal
    neighbours, NaN behind top"""
    n = 1 << bits
    top = n - 1 if top is None else top
    s = np.full(n, np.nan, F)
    s[0] = -np.inf
    v = np.sort(rng.uniform(lo, hi, top).astype(F))
    for _ in range(ties):
        k = int(rng.integers(0, max(1, top - 3)))
        v[k:k + 3] = v[k]
    s[1:top + 1] = np.sort(v)
    return s


def random_frame(rng, h, w, nch, specials=True):
    """floats around the tables' range, with NaN, both infinities and -0 among them"""
    f = rng.uniform(-0.3, 1.3, (h, w, nch)).astype(F)
    if specials and h * w >= 4:
        flat = f.reshape(-1, nch)
        idx = rng.integers(0, h * w, max(4, h * w // 16))
        vals = np.array([np.nan, np.inf, -np.inf, -0.0], F)
        flat[idx, rng.integers(0, 3, idx.size)] = vals[rng.integers(0, 4, idx.size)]
    return f
