"""A numpy float32 model of the Y'CbCr feed, written from its three formulas - not from include/eu_ycbcr.h and not
through the library: tables looked up with numpy.take, every product and every sum a separate float32 operation.
Shared by the host and the device tests, which compare the library with it bit for bit.

    R = Y + m_rv * V        G = (Y + m_gu * U) + m_gv * V        B = Y + m_bu * U
"""
import numpy as np


def expand(c, sub_x, sub_y, h, w):
    """chroma replicated: pixel (x, y) takes sample (x // sub_x, y // sub_y)"""
    return np.repeat(np.repeat(c, sub_y, axis=0), sub_x, axis=1)[:h, :w]


def floats(y, cb, cr, sub_x, sub_y, y_table, c_table, matrix, nch=3):
    h, w = y.shape
    m_rv, m_gu, m_gv, m_bu = (np.float32(v) for v in matrix)
    Y = np.take(y_table, y).astype(np.float32)
    U = np.take(c_table, expand(cb, sub_x, sub_y, h, w)).astype(np.float32)
    V = np.take(c_table, expand(cr, sub_x, sub_y, h, w)).astype(np.float32)
    rv = m_rv * V
    gu = m_gu * U
    gv = m_gv * V
    bu = m_bu * U
    yg = Y + gu
    out = np.ones((h, w, nch), np.float32)
    out[..., 0] = Y + rv
    out[..., 1] = yg + gv
    out[..., 2] = Y + bu
    for a in (rv, gu, gv, bu, yg):
        assert a.dtype == np.float32
    return out


def planes(rng, h, w, sub_x, sub_y, bits, layout, pad=0):
    """random planes of a frame: (y, cb, cr) as views with `pad` extra samples per row. layout: 'planar' (c_step 1),
    'nv12' (interleaved, cr == cb + 1 sample) or 'nv21' (cb == cr + 1 sample)"""
    dt = np.uint8 if bits == 8 else np.uint16
    top = 1 << bits
    ch, cw = (h + sub_y - 1) // sub_y, (w + sub_x - 1) // sub_x
    y = rng.integers(0, top, (h, w + pad)).astype(dt)[:, :w]
    if layout == "planar":
        cb = rng.integers(0, top, (ch, cw + pad)).astype(dt)[:, :cw]
        cr = rng.integers(0, top, (ch, cw + pad)).astype(dt)[:, :cw]
    else:
        both = rng.integers(0, top, (ch, cw + pad, 2)).astype(dt)[:, :cw]
        cb, cr = (both[..., 0], both[..., 1]) if layout == "nv12" else (both[..., 1], both[..., 0])
    return y, cb, cr


def random_tables(rng, bits):
    """tables that are no formula of the code: the library only looks them up"""
    n = 1 << bits
    return (rng.uniform(-0.1, 1.1, n).astype(np.float32), rng.uniform(-0.6, 0.6, n).astype(np.float32))
